"""The precision-weighted fusion where its weights do not sum to one (the "uncertain heads" regime).  `-m gpu`.

    w_m = factor exp(-logvar_m),  den = w_i + w_e + eps,  n_m = w_m / den,  z0 = n_i mu_i + n_e mu_e            (imf_vad.py:130-144)

With synth.make_state_dict's own weights eps / den ~ 5e-9 and `factor` cancels: every other forward, variants, trajectory, valid-row and
training test of this suite passes with ANY value of precision_factor() and of cfg.epsilon.  Here the log-variance biases are shifted by
(15.5, 17.0) (synth.shift_logvar_bias; median 1 - (w_i + w_e) = 0.036) or epsilon is 1e-2, and every site that takes `factor` / `eps` is
asked: iefvad_fusion_kernel<768 / 512>, the two bf16 heads row-block kernels, iefvad_fusion_variants_kernel, the train-mode forward,
iefvad_fusion_bwd_kernel and IEFVAD_UNIT_HEADS.  tests/test_precision_cpu.py holds the conditions that keep this file from being vacuous.

Two layers.
  Parity   the prec_*.npz captures of the reference (tests/golden/make_golden_precision.py) at H.compare_outputs' gates, max(TOL, 3 x the
           recorded floor), for the fp32-accurate arithmetics.  The bf16 mode is not held to them: its 4e-2 gate is wider than what
           separates two noise models here (1.4e-3 on `fused`).
  Formula  reference-free and mode-independent, and what covers bf16: the model returns the four heads, w_i, w_e (and with K = 0 z0 as
           `fused`) as fp32, so H.fuse_fp64 of the RETURNED heads must reproduce the returned w_i, w_e and z0 within 3 x `formula_floor`
           relative -- the fixture's record of what the literal fp32 lines (torch, CPU) lose against fp64, never measured on a kernel;
           3 x is the margin every gate of this suite keeps over a reference-side floor, and leaves room for a 2-ulp expf.
Which kernel a bf16 batch size reaches is the rule of csrc/launch_rules.h, pinned at its thresholds by tests/test_launch_rules_cpu.py
(heads row-block kernel from 2,752 rows, its persistent form from 10,880)."""
import argparse
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth
from iefvad_amd import lib as L
from tests import helpers as H

pytestmark = pytest.mark.gpu

WSEED, ISEED = 11, 12                   # the prec_k3_* fixtures' weights; inputs of other batch sizes from the same stream
NOISES = [("StudentT", 8), ("StudentT", 1), ("Gaussian", 8)]
NOISE_IDS = ["student8", "student1", "gauss"]
FIXTURE_OF = {("StudentT", 8): "k3_student8", ("StudentT", 1): "k3_student1", ("Gaussian", 8): "k3_gauss"}


@functools.lru_cache(maxsize=None)
def formula_gate(name):
    """3 x the `formula_floor` a fixture records."""
    return 3.0 * float(np.load(f"{H.GOLDEN}/prec_{name}.npz")["formula_floor"])


@functools.lru_cache(maxsize=None)
def shifted_state(K, D=768, wseed=WSEED):
    return synth.shift_logvar_bias(synth.make_state_dict(wseed, D, 2, K), *H.PRECISION_SHIFT)


@functools.lru_cache(maxsize=None)
def inputs(B, D=768):
    img, ev = synth.make_inputs(ISEED, B, D=D)
    img[B - 1, 100:] = 0      # a padded tail in the last chunk
    ev[B - 1, 100:] = 0
    return torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()


def make_model(sd, compute, noise, nu, K, D=768, lam=0.5, epsilon=None, **kw):
    args = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=K, lambda_ref=lam, noise_model=noise, nu=nu)
    m = iefvad_amd.MMFMIL(14, D, 256, D, 8, 2, 8, 10, 10, "cuda", args, compute=compute, **kw)
    m.load_state_dict(sd)
    if epsilon is not None:
        m.temporal.epsilon = epsilon      # a plain attribute, as in the reference; the handle is rebuilt when it changes (model._ensure_handle)
    return m.to("cuda:0").eval()


def run(model, img, ev, **kw):
    """The model's dict (clones: a replayed hipGraph writes where the last call wrote)."""
    with torch.no_grad():
        out = model(img, ev, None, None, None, **kw)
    torch.cuda.synchronize()
    return {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in out.items()}


def check_formula(out, noise, nu, eps, gate, what, fused, on_device=False):
    """The formula layer on one output dict.  Small results are evaluated on the host, large ones where they are."""
    if not on_device:
        out = {k: v.cpu() for k, v in out.items() if isinstance(v, torch.Tensor)}
    for k in ("image_logvar", "event_logvar", "w_i", "w_e"):
        assert bool(torch.isfinite(out[k]).all()), (what, k)
    errs = H.formula_errors(out, noise, nu, eps, fused=fused)
    blind = H.formula_errors(out, noise, nu, 0.0)          # what a dropped epsilon would cost: the regime is the one the gate can see in
    print(f"{what}: max relative |returned - fuse_fp64(returned heads)| = { {k: f'{v:.2e}' for k, v in errs.items()} } gate {gate:.2e}; "
          f"with eps = 0 instead: {max(blind.values()):.2e}")
    assert min(blind.values()) >= 100 * gate, (what, blind)
    for k, e in errs.items():
        assert e <= gate, (what, k, e, gate)
    return errs


# ---- parity with the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute,kw", [("f32", {}), ("bf16x6", {}), ("bf16x6", dict(batch_invariant=True)), ("fp16x3", {})],
                         ids=["f32", "bf16x6", "bf16x6-invariant", "fp16x3"])
@pytest.mark.parametrize("name", [n for n in H.PRECISION_CASES if not n.startswith("vitb")])
def test_parity_with_the_reference_where_factor_and_epsilon_matter(name, compute, kw):
    """All eight outputs of the four D = 768 captures (Student-8, nu = 1 and Gaussian on one set of shifted weights; Student-5 with
    epsilon = 1e-2 and K = 0) at the fp32 gates."""
    g, cfg, sd, img, ev = H.load_precision_case(name)
    model = make_model(sd, compute, cfg["noise"], cfg["nu"], cfg["K"], lam=cfg["lam"], epsilon=cfg["epsilon"], **kw)
    out = run(model, torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda())
    errs = H.compare_outputs({k: v.cpu().numpy() for k, v in out.items()}, g)
    print(name, compute, kw, errs, "gates", H.case_gates(g, (H.TOL_BIG, H.TOL_LOGIT, H.TOL_SIGMOID)))


def test_parity_with_the_reference_at_d512():
    g, cfg, sd, img, ev = H.load_precision_case("vitb_k3_student8")
    assert cfg["D"] == 512
    model = make_model(sd, "f32", cfg["noise"], cfg["nu"], cfg["K"], D=512, lam=cfg["lam"], epsilon=cfg["epsilon"])
    out = run(model, torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda())
    errs = H.compare_outputs({k: v.cpu().numpy() for k, v in out.items()}, g)
    print("vitb_k3_student8 f32", errs)


# ---- the formula layer -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise,nu", NOISES, ids=NOISE_IDS)
@pytest.mark.parametrize("compute,B,D", [("f32", 2, 768), ("bf16x6", 2, 768), ("fp16x3", 2, 768), ("f32", 2, 512),
                                         ("bf16x6", 6, 768), ("fp16x3", 6, 768),      # B = 2 runs on the fp32 kernels; from 6 chunks the split ones
                                         ("bf16", 2, 768),        # the stand-alone fusion kernel behind the ring GEMM
                                         ("bf16", 12, 768),       # iefvad_heads_chain_bf16_kernel (3,072 rows)
                                         ("bf16", 48, 768)],      # iefvad_heads_pchain_bf16_kernel (12,288 rows)
                         ids=lambda v: str(v))
def test_returned_weights_and_z0_are_the_formula_of_the_returned_heads(compute, B, D, noise, nu):
    """K = 0, so `fused` is z0 itself: w_i, w_e and z0 against fuse_fp64 of the heads the same call returned."""
    # D = 512 has one capture (Student-8); the other noise models take the D = 768 capture's floor: the same four lines on heads of the same range
    name = "vitb_k3_student8" if (D, noise, nu) == (512, "StudentT", 8) else FIXTURE_OF[(noise, nu)]
    model = make_model(shifted_state(0, D, 31 if D == 512 else WSEED), compute, noise, nu, 0, D=D)
    out = run(model, *inputs(B, D))
    check_formula(out, noise, nu, 1e-8, formula_gate(name), f"{compute} B={B} D={D} {noise} nu={nu}", fused=True, on_device=B > 2)
    assert float(out["image_logvar"].max()) < 21.0 and float(out["event_logvar"].max()) < 21.0
    assert float((1 - (out["w_i"] + out["w_e"])).median()) > 0.015          # the regime: the weights do not sum to one


def test_heads_row_block_kernel_equals_the_ring_kernel_in_the_shifted_regime(monkeypatch):
    """bf16, B = 12: the heads row-block kernel against the ring GEMM + the fusion kernel (IEFVAD_ROWBLOCK_OFF=4 at model creation),
    bit for bit, as tests/test_gpu_bf16.py::test_heads_row_block_kernel_equals_the_ring_kernel asserts it with the seeded weights --
    where a differing `factor` or `eps` between the two would not show."""
    img, ev = inputs(12)
    rows = run(make_model(shifted_state(0), "bf16", "StudentT", 8, 0), img, ev)
    monkeypatch.setenv("IEFVAD_ROWBLOCK_OFF", "4")
    ring = run(make_model(shifted_state(0), "bf16", "StudentT", 8, 0), img, ev)
    assert set(rows) == set(ring)
    for k in rows:
        assert bool(torch.isfinite(rows[k]).all()), k
        assert torch.equal(rows[k], ring[k]), (k, float((rows[k] - ring[k]).abs().max()))
    check_formula(ring, "StudentT", 8, 1e-8, formula_gate("k3_student8"), "bf16 B=12 ring kernels", fused=True, on_device=True)


@pytest.mark.parametrize("noise,nu", NOISES, ids=NOISE_IDS)
@pytest.mark.parametrize("rows", [64, 16448])
def test_heads_unit_entry_in_the_shifted_regime(rows, noise, nu):
    """IEFVAD_UNIT_HEADS (`iefvad_rowblock_unit`): the production heads kernels on rows the test supplies -- 64 rows, one block of the
    row-block kernel; 16,448 rows, 257 blocks, the persistent kernel on an uneven walk."""
    model = make_model(shifted_state(1), "bf16", noise, nu, 1)
    with torch.cuda.device(0):
        model._ensure_handle(torch.device("cuda:0"))
        model._ensure_weights(torch.device("cuda:0"), torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(rows)
    x = [(torch.randn(rows, 768, generator=g) * 0.7).to(torch.bfloat16).cuda() for _ in range(2)]
    f32 = dict(device="cuda", dtype=torch.float32)
    nan = lambda: torch.full((rows, 768), float("nan"), **f32)
    mu, lv, w, z = [nan(), nan()], [nan(), nan()], [nan(), nan()], nan()
    io = L.UnitIO()
    for m in range(2):
        io.x[m], io.mu[m], io.logvar[m], io.w[m] = x[m].data_ptr(), mu[m].data_ptr(), lv[m].data_ptr(), w[m].data_ptr()
    io.z = z.data_ptr()
    rc = L.load_library().iefvad_rowblock_unit(model._handle, L.UNIT_HEADS, 0, rows, C.byref(io), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    out = {"image_mu": mu[0], "event_mu": mu[1], "image_logvar": lv[0], "event_logvar": lv[1], "w_i": w[0], "w_e": w[1], "fused": z}
    assert 10.0 < float(lv[0].min()) and float(lv[1].max()) < 21.0          # the shifted biases reached the kernel
    check_formula(out, noise, nu, 1e-8, formula_gate(FIXTURE_OF[(noise, nu)]), f"UNIT_HEADS rows={rows} {noise} nu={nu}", fused=True, on_device=True)


@pytest.mark.parametrize("noise,nu", NOISES, ids=NOISE_IDS)
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_valid_row_route_in_the_shifted_regime(compute, noise, nu):
    """forward_videos(..., outputs="full") on videos of 1, 255 and 257 snippets (4 chunks; the tail runs on the valid rows only)."""
    lengths = [1, 255, 257]
    vids = [synth.make_video(13, i, n) for i, n in enumerate(lengths)]
    rows = [torch.from_numpy(np.concatenate([v[m] for v in vids])).cuda() for m in range(2)]
    model = make_model(shifted_state(0), compute, noise, nu, 0)
    with torch.no_grad():
        out = model.forward_videos(rows[0], rows[1], lengths, outputs="full")
    torch.cuda.synchronize()
    assert out["w_i"].shape == (sum(lengths), 768)
    check_formula(out, noise, nu, 1e-8, formula_gate(FIXTURE_OF[(noise, nu)]), f"forward_videos {compute} {noise} nu={nu}", fused=True)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_epsilon_set_on_the_model_reaches_the_fusion(compute):
    """make_state_dict's own weights, Student-5, K = 0, `model.temporal.epsilon = 1e-2` (the prec_k0_student5_eps capture's model): the
    returned weights are the formula with THAT epsilon, and restoring 1e-8 on the same module rebuilds the handle."""
    g, cfg, sd, img, ev = H.load_precision_case("k0_student5_eps")
    model = make_model(sd, compute, cfg["noise"], cfg["nu"], 0, epsilon=cfg["epsilon"])
    ti, te = torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()
    out = run(model, ti, te)
    gate = formula_gate("k0_student5_eps")
    check_formula(out, cfg["noise"], cfg["nu"], 1e-2, gate, f"epsilon = 1e-2 {compute}", fused=True)
    model.temporal.epsilon = 1e-8
    back = run(model, ti, te)
    errs = H.formula_errors({k: v.cpu() for k, v in back.items()}, cfg["noise"], cfg["nu"], 1e-8, fused=True)
    assert max(errs.values()) <= gate, errs
    assert float((back["w_i"] - out["w_i"]).abs().median()) > 1e-4          # 1 - (w_i + w_e) ~ 4e-3 with epsilon = 1e-2, ~ 5e-9 without


VARIANT_NAMES = ("fused", "image", "event", "equal")


@pytest.mark.parametrize("noise,nu", NOISES, ids=NOISE_IDS)
@pytest.mark.parametrize("compute", ["f32", "bf16x6", "bf16"])
def test_fusion_variants_are_the_substituted_formula_of_the_returned_heads(compute, noise, nu):
    """fusion_variants=True at K = 0: the four rows of `logits_variants` against classifier(z0) with z0 from fuse_fp64 of the returned heads
    under the documented substitution -- "image": w_e := 0, so n_i = w_i / (w_i + eps), about 0.95 here and not 1; "event": w_i := 0;
    "equal": both log-variances := 0, n = factor / (2 factor + eps).
    Gate per row: the fp32 logit gate H.TOL_LOGIT (the scorer's 768-term fp32 sum) plus what z0's own gate, 3 x formula_floor of
    |n_i mu_i| + |n_e mu_e| per column, can move the dot product by: sum_d |c_d| 3 ff s_d."""
    sd = shifted_state(0)
    model = make_model(sd, compute, noise, nu, 0)
    out = run(model, *inputs(2), fusion_variants=True)
    assert tuple(out["fusion_variants"]) == VARIANT_NAMES and out["logits_variants"].shape == (4, 2, 256)
    heads = [out[k].cpu().double() for k in ("image_mu", "image_logvar", "event_mu", "event_logvar")]
    c, b = sd["temporal.classifier.weight"].double().reshape(-1), sd["temporal.classifier.bias"].double()
    gate = formula_gate(FIXTURE_OF[(noise, nu)])
    inf, zero = torch.full_like(heads[1], float("inf")), torch.zeros_like(heads[1])
    subst = {"fused": heads, "image": [heads[0], heads[1], heads[2], inf], "event": [heads[0], inf, heads[2], heads[3]],
             "equal": [heads[0], zero, heads[2], zero]}          # exp(-inf) = 0: the removed branch's precision
    for v, name in enumerate(VARIANT_NAMES):
        for eps, must_pass in ((1e-8, True), (0.0, False)):
            n_i, n_e, z0 = H.fuse_fp64(*subst[name], noise, nu, eps)
            want = z0 @ c + b
            tol = H.TOL_LOGIT + gate * (((n_i * heads[0]).abs() + (n_e * heads[2]).abs()) @ c.abs())
            err = (out["logits_variants"][v].cpu().double() - want).abs()
            if must_pass:
                print(f"{compute} {noise} nu={nu} {name}: max |logits - classifier(z0)| = {float(err.max()):.2e}, largest gate {float(tol.max()):.2e}, "
                      f"median n_i {float(n_i.median()):.4f}")
                assert bool((err <= tol).all()), (name, float((err / tol).max()))
            elif name != "equal":      # without epsilon the same comparison fails by far ("equal": eps / (2 factor) = 4e-9, invisible)
                assert float((err / tol).median()) > 20, (name, float((err / tol).median()))
    n_img = H.fuse_fp64(*subst["image"], noise, nu, 1e-8)[0]
    assert 0.8 < float(n_img.median()) < 0.99, float(n_img.median())


# ---- train mode: forward and every parameter gradient --------------------------------------------------------------------------------
def oracle_grads(noise, nu):
    """(fp64 gradients, fp32 floor in gates) of the oracle at B = 3; H caches both, so every compute mode shares one evaluation."""
    torch.set_num_threads(harness.host_cpu_share())
    return H.oracle_precision_grads(noise, 3, nu=nu), H.oracle_precision_grad_floor(noise, 3, nu)[0]


def train_step(compute, noise, nu):
    """model.train() (dropout 0), B = 3, K = 2 on the shifted PRECISION_GRAD model: forward, H.precision_scalar, backward."""
    p = H.PRECISION_GRAD
    model = make_model(H.precision_grad_state(), compute, noise, nu, p["K"])
    for a in list(model.temporal.image_attn_layers) + list(model.temporal.event_attn_layers):
        a.dropout = 0.0
    model.train()
    img, ev, _, _ = synth.make_train_batch(p["bseed"], 3)
    out = model(torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda(), None, None, None)
    H.precision_scalar(out).backward()
    torch.cuda.synchronize()
    return model, out


@pytest.mark.parametrize("noise,nu", NOISES, ids=NOISE_IDS)
@pytest.mark.parametrize("compute", ["f32", "bf16x6"])
def test_train_mode_forward_in_the_shifted_regime(compute, noise, nu):
    """The train-mode forward (train.h launches the fusion kernel with a `factor` / `eps` of its own): its outputs pass the formula layer."""
    _, out = train_step(compute, noise, nu)
    check_formula({k: v.detach() for k, v in out.items()}, noise, nu, 1e-8, formula_gate(FIXTURE_OF[(noise, nu)]),
                  f"train forward {compute} {noise} nu={nu}", fused=False)


@pytest.mark.parametrize("noise,nu", NOISES, ids=NOISE_IDS)
@pytest.mark.parametrize("compute", ["f32", "bf16x6"])
def test_train_mode_gradients_in_the_shifted_regime(compute, noise, nu):
    """Every parameter gradient of H.precision_scalar (through iefvad_fusion_bwd_kernel) lies within max(1, 3 x floor) x (1e-4 |want| +
    2e-6 max |want|) of the oracle's fp64 autograd, `floor` the oracle's own fp32 autograd error in those units, measured here next to
    the fp64 gradients (H.oracle_precision_grad_floor; about 0.5, so the gate is about 1.5).  tests/test_precision_cpu.py asserts that
    the noise models' gradients differ by more than 10 such gates on at least 10 of the 46 tensors at this batch size."""
    model, _ = train_step(compute, noise, nu)
    want, floor = oracle_grads(noise, nu)
    got = {n: q.grad.detach().cpu().double() for n, q in model.named_parameters()}
    assert list(got) == list(want)
    units = H.grad_gates(got, want)
    entry_gate = max(1.0, 3.0 * floor)
    worst = max(units.items(), key=lambda t: t[1])
    print(f"train {compute} {noise} nu={nu}: worst gradient entry {worst[1]:.2f} gates ({worst[0]}), allowed {entry_gate:.2f} (floor {floor:.4f})")
    for n, u in units.items():
        assert bool(torch.isfinite(got[n]).all()), n
        assert u <= entry_gate, (n, u, entry_gate)
