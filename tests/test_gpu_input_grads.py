"""Gradients of the two input feature tensors (`iefvad_train_backward_inputs`, MMFMIL with `requires_grad` features) on the MI355X.

The reference's MMFMIL is an ordinary nn.Module (model/imf_vad.py:40-44,109-161): a feature tensor that requires grad gets its `.grad`, in
train() and in eval() alike.  Here that is the layer-0 instance of the product every encoder layer above it runs in the backward,
d x = d s (residual) + d qkv W_in, written to a buffer of the caller's.  Pinned by tests/golden/grad_inputs_*.npz (the reference's fp64
autograd, tests/golden/make_golden_input_grads.py) at the fixtures' sizes, by fp64 autograd through the oracle where the product runs
on the split kernel (B = 8), and by bit comparisons: asking for an input gradient moves nothing else."""
import argparse
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import lib as L
from iefvad_amd import losses, synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

FIXTURES = ["k2_student8", "sharp_k2_student8", "k10_student8_mask"]
KEYS = iefvad_amd.model.OUTPUT_KEYS


def make_model(wseed, L_, K, noise="StudentT", nu=8, compute="f32", p=0.0, factors=None):
    sd = synth.make_state_dict(wseed, 768, L_, K)
    if factors is not None:
        sd = synth.sharpen_qk(sd, factors)
    args = argparse.Namespace(visual_layers=L_, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model=noise, nu=nu)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, L_, 8, 10, 10, "cuda", args, compute=compute)
    m.load_state_dict(sd)
    m = m.to("cuda:0")
    for a in list(m.temporal.image_attn_layers) + list(m.temporal.event_attn_layers):
        a.dropout = p
    return m, sd


def split_scalar(o):
    """The scalar of test_bf16x6_backward_on_the_split_kernel_at_a_batch_that_fills_its_grid (tests/test_gpu_train.py)."""
    return o["logits"].sum() + 0.5 * (o["image_mu"] * o["event_logvar"]).sum() + 0.25 * (o["event_mu"] * o["image_logvar"]).sum()


def local_scalar(o):
    """An upstream gradient on chunk 0's outputs only."""
    return o["logits"][0].sum() + (o["image_mu"][0] ** 2).sum()


@functools.lru_cache(maxsize=None)
def step(compute, B, wseed=5, bseed=77, L_=2, K=2, p=0.0, masked=False, req=(True, True), frozen=False, training=True, scalar="split",
         in_dtype=torch.float32, factors=None, lams=(1.0, 1.0)):
    """One forward + backward of a fresh model; everything it leaves, on the host (shared between the tests, never modified).
    `p`: every layer's `.dropout`; `masked`: the injected mask of synth.make_dropout_mask(bseed, ...) at probability 0.1 rides along;
    `req`: which of (img, ev) require grad; `scalar`: "split" / "local" above, or "loss" (the trainers' total)."""
    model, _ = make_model(wseed, L_, K, compute=compute, p=p, factors=factors)
    if masked:
        model.dropout_mask = torch.from_numpy(synth.make_dropout_mask(bseed, L_, B, 0.1)).cuda()
    if frozen:
        for q in model.parameters():
            q.requires_grad_(False)
    model.train(training)
    img, ev, labels, lengths = synth.make_train_batch(bseed, B)
    x = [torch.from_numpy(a).cuda().to(in_dtype).requires_grad_(r) for a, r in zip((img, ev), req)]
    out = model(x[0], x[1], None, None, torch.from_numpy(lengths).cuda())
    res = {"requires_grad": {k: out[k].requires_grad for k in KEYS}, "grad_fn": {k: out[k].grad_fn is not None for k in KEYS},
           "out": {k: out[k].detach().cpu() for k in KEYS}}
    if any(res["requires_grad"].values()):
        if scalar == "loss":
            s = losses.training_loss(out, torch.from_numpy(labels).cuda(), torch.from_numpy(lengths).cuda(), "StudentT", 8, *lams)
        else:
            s = {"split": split_scalar, "local": local_scalar}[scalar](out)
        s.backward()
        res["scalar"] = float(s.detach())
    res["gin"] = [None if t.grad is None else t.grad.detach().cpu() for t in x]
    res["pg"] = {n: None if q.grad is None else q.grad.detach().cpu() for n, q in model.named_parameters()}
    return res


# ---- 1. the reference pin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_input_gradients_match_the_reference_autograd(name):
    """d img and d ev of the trainers' loss against the reference's fp64 autograd (grad_inputs_*.npz), f32, at the fixture's own batch:
    4096 sampled entries per modality within entry_gate x (1e-4 |want| + 1e-6 max|want|), entry_gate = max(1, 3 x grad_floor) with the
    floor the fixture records for the reference's OWN fp32 autograd (0.84 / 0.92 / 0.58 of the unit for k2_student8 / sharp_k2_student8 /
    k10_student8_mask, i.e. gates of 2.51 / 2.75 / 1.73 units) -- the rule of test_every_parameter_gradient_matches_the_reference_autograd;
    L1 and L2 norms within 1e-4.  Measured on MI355X (f32 kernels), worst sampled entry in units (d img / d ev): 1.27 / 0.69, 0.69 / 0.84,
    0.73 / 0.66 in the order above; norms within 5.1e-7 (profiles/input_grads_tests.log; CALLERS.md 4.7)."""
    g = np.load(os.path.join(H.GOLDEN, f"grad_inputs_{name}.npz"))
    wseed, bseed, B, L_, K, nu = (int(v) for v in g["cfg"])
    assert str(g["noise"]) == "StudentT" and nu == 8
    p = float(g["p"])
    factors = tuple(float(f) for f in g["factors"]) if "factors" in g.files else None
    r = step("f32", B, wseed, bseed, L_, K, p=p, masked=p > 0, scalar="loss", factors=factors, lams=tuple(float(v) for v in g["lams"]))
    entry_gate = max(1.0, 3.0 * float(g["grad_floor"]))
    assert abs(r["scalar"] - float(g["total"])) <= 2e-5 * max(1.0, abs(float(g["total"])))
    worst = {}
    for key, grad in zip(("img", "ev"), r["gin"]):
        assert grad is not None and grad.dtype == torch.float32 and tuple(grad.shape) == (B, 256, 768), key
        got = grad.double().numpy().reshape(-1)
        assert np.isfinite(got).all(), key
        l1, l2, mx = (float(v) for v in g[f"{key}_norms"])
        want = g[f"{key}_val"]
        err = np.abs(got[g[f"{key}_idx"]] - want)
        tol = 1e-4 * np.abs(want) + 1e-6 * mx
        worst[key] = float((err / tol).max())
        print(f"{name} d {key}: worst sampled entry {worst[key]:.3f} gate units (entry gate {entry_gate:.3f}); "
              f"L1 rel {abs(np.abs(got).sum() - l1) / l1:.2e}, L2 rel {abs(np.sqrt((got * got).sum()) - l2) / l2:.2e}")
    for key, grad in zip(("img", "ev"), r["gin"]):
        got = grad.double().numpy().reshape(-1)
        l1, l2, mx = (float(v) for v in g[f"{key}_norms"])
        assert worst[key] <= entry_gate, (key, worst[key], entry_gate)
        assert abs(np.abs(got).sum() - l1) <= 1e-4 * l1, (key, "L1")
        assert abs(np.sqrt((got * got).sum()) - l2) <= 1e-4 * l2, (key, "L2")


# ---- 2. the split route ----------------------------------------------------------------------------------------------------------------
def test_input_gradients_on_the_split_kernel_at_a_batch_that_fills_its_grid():
    """B = 8 (2048 rows, 96 >= 72 workgroups): in compute='bf16x6' layer 0's K = 2304 product runs on the exact-split kernel (EPI_BIAS_RESID,
    the transposed planes of in_proj), in 'f32' on the fp32 MFMA kernel.  Both against fp64 autograd through the oracle at the gate of the
    parameter test at this size, 1e-4 |want| + 2e-6 max; the two arithmetics' bits differ (another kernel ran); bf16x6 reproduces its bits."""
    from oracle import iefvad_oracle as orc
    B = 8
    runs = {c: step(c, B) for c in ("f32", "bf16x6")}
    again = step.__wrapped__("bf16x6", B)                  # past the cache: a second run of its own
    img, ev, _, _ = synth.make_train_batch(77, B)
    sd64 = {k: v.double() for k, v in synth.make_state_dict(5, 768, 2, 2).items()}
    x64 = [torch.from_numpy(a).double().requires_grad_(True) for a in (img, ev)]
    split_scalar(orc.forward(sd64, x64[0], x64[1], orc.OracleConfig(num_layers=2, num_refinement_steps=2, nu=8), dtype=torch.float64)).backward()
    for m, key in enumerate(("img", "ev")):
        want = x64[m].grad
        mx = float(want.abs().max())
        for c in ("f32", "bf16x6"):
            err = (runs[c]["gin"][m].double() - want).abs()
            units = float((err / (1e-4 * want.abs() + 2e-6 * mx)).max())
            print(f"B = 8 d {key} ({c}) vs fp64 autograd: worst entry {units:.3f} of the gate")
            assert units <= 1.0, (c, key, units, float(err.max()), mx)
        assert not torch.equal(runs["f32"]["gin"][m], runs["bf16x6"]["gin"][m]), key
        assert torch.equal(runs["bf16x6"]["gin"][m], again["gin"][m]), key


# ---- 3. nothing else moves ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute,B", [("f32", 3), ("bf16x6", 8)])
def test_asking_for_input_gradients_changes_no_parameter_gradient_and_no_output(compute, B):
    """Same model, batch and injected dropout mask, with and without `requires_grad` on the features: every parameter gradient and all
    eight outputs keep their bits (the residual gradient is only read; the layer-0 product writes to a buffer of its own)."""
    a = step(compute, B, p=0.1, masked=True, req=(True, True))
    b = step(compute, B, p=0.1, masked=True, req=(False, False))
    assert b["gin"] == [None, None] and all(g is not None for g in a["gin"])
    for k in KEYS:
        assert torch.equal(a["out"][k], b["out"][k]), k
    assert a["pg"].keys() == b["pg"].keys()
    for n in a["pg"]:
        assert a["pg"][n] is not None and torch.equal(a["pg"][n], b["pg"][n]), n


# ---- 4. locality ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute,B", [("f32", 3), ("bf16x6", 8)])
def test_an_upstream_gradient_on_one_chunk_reaches_that_chunk_only(compute, B):
    """Chunks do not interact: with the upstream gradient on chunk 0's outputs, the other chunks' input gradients are exactly zero."""
    r = step(compute, B, scalar="local")
    for key, g in zip(("img", "ev"), r["gin"]):
        assert float(g[1:].abs().max()) == 0.0, key
        assert float(g[0].abs().max()) > 0.0, key


# ---- 5. one side only ----------------------------------------------------------------------------------------------------------------------
def test_only_the_modality_that_requires_grad_gets_one():
    both = step("f32", 3)
    one = step("f32", 3, req=(False, True))
    assert one["gin"][0] is None
    assert torch.equal(one["gin"][1], both["gin"][1])
    for n in both["pg"]:
        assert torch.equal(one["pg"][n], both["pg"][n]), n


# ---- 6. dtypes -----------------------------------------------------------------------------------------------------------------------------
def test_the_gradient_comes_back_in_the_feature_dtype():
    """fp16 features: `.grad` is fp16 and is the fp32 run on the widened tensors, rounded (the gradient is with respect to the fp32
    values the forward computed on, cast as autograd casts through `.to(torch.float)`); fp64 features get an fp64 `.grad`."""
    model, _ = make_model(5, 2, 2)
    model.train()
    img, ev, _, _ = synth.make_train_batch(78, 1)
    h16 = [torch.from_numpy(a).cuda().half() for a in (img, ev)]
    grads = {}
    for name, cast in (("f16", lambda t: t), ("f32", lambda t: t.float()), ("f64", lambda t: t.double())):
        x = [cast(t).clone().requires_grad_(True) for t in h16]
        split_scalar(model(x[0], x[1], None, None, None)).backward()
        grads[name] = [t.grad for t in x]
    for m in range(2):
        assert grads["f16"][m].dtype == torch.float16 and grads["f32"][m].dtype == torch.float32 and grads["f64"][m].dtype == torch.float64
        assert tuple(grads["f16"][m].shape) == (1, 256, 768)
        assert float(grads["f32"][m].abs().max()) > 0.0
        assert torch.equal(grads["f16"][m], grads["f32"][m].half())
        assert torch.equal(grads["f64"][m], grads["f32"][m].double())


# ---- 7. frozen model -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute,B", [("f32", 3), ("bf16x6", 8)])
def test_a_frozen_model_still_differentiates_its_inputs(compute, B):
    """Every parameter frozen, features requiring grad: the outputs carry a grad_fn, the backward runs (it skips every weight-gradient
    product: csrc/train.h), the input gradients have the bits of the unfrozen run and no parameter has a gradient."""
    frozen = step(compute, B, frozen=True)
    live = step(compute, B)
    assert all(frozen["grad_fn"].values()) and all(frozen["requires_grad"].values())
    for m in range(2):
        assert frozen["gin"][m] is not None and torch.equal(frozen["gin"][m], live["gin"][m])
    assert all(g is None for g in frozen["pg"].values())
    for k in KEYS:
        assert torch.equal(frozen["out"][k], live["out"][k]), k


def test_a_frozen_model_differentiates_one_modality_alone():
    """Frozen, and only the event features require grad: the image side's layer 0 has nothing to produce (its attention backward is
    skipped); the event gradient keeps the bits of the unfrozen both-sides run."""
    one = step("f32", 3, frozen=True, req=(False, True))
    assert one["gin"][0] is None and torch.equal(one["gin"][1], step("f32", 3)["gin"][1])


# ---- 8. eval mode --------------------------------------------------------------------------------------------------------------------------
def test_eval_mode_differentiates_features_that_require_grad():
    """model.eval() with the layers' `.dropout = 0.1` left in place: features that require grad route the call through the train-mode
    forward with dropout off -- outputs that require grad, at the fp32 gates of the no_grad eval forward, input gradients with the bits
    of a train() run whose layers have `.dropout = 0`.  Without `requires_grad` on the features the same call is the evaluation entry:
    no grad_fn (parameters that require grad do not trigger the route), the bits of the no_grad call."""
    B = 3
    ev_run = step("f32", B, p=0.1, training=False)
    tr_run = step("f32", B, p=0.0, training=True)
    assert all(ev_run["requires_grad"].values())
    for m in range(2):
        assert torch.equal(ev_run["gin"][m], tr_run["gin"][m])
    model, _ = make_model(5, 2, 2, p=0.1)
    model.eval()
    img, ev, _, _ = synth.make_train_batch(77, B)
    img, ev = torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()
    with torch.no_grad():
        ref = model(img, ev, None, None, None)
    for k in KEYS:
        assert float((ev_run["out"][k] - ref[k].cpu()).abs().max()) <= H.TOL_BIG, k
    assert float((torch.sigmoid(ev_run["out"]["logits"]) - torch.sigmoid(ref["logits"].cpu())).abs().max()) <= H.TOL_SIGMOID
    assert any(q.requires_grad for q in model.parameters())
    plain = model(img, ev, None, None, None)
    for k in KEYS:
        assert plain[k].grad_fn is None and not plain[k].requires_grad, k
        assert torch.equal(plain[k], ref[k]), k
    # ... and under no_grad a feature tensor that requires grad keeps the evaluation entry too
    with torch.no_grad():
        quiet = model(img.clone().requires_grad_(True), ev, None, None, None)
    assert all(torch.equal(quiet[k], ref[k]) and quiet[k].grad_fn is None for k in KEYS)


def test_the_differentiable_eval_route_refuses_the_evaluation_extras_by_name():
    model, _ = make_model(5, 2, 2)
    model.eval()
    img, ev, _, _ = synth.make_train_batch(77, 1)
    img, ev = torch.from_numpy(img).cuda().requires_grad_(True), torch.from_numpy(ev).cuda()
    for kw, frag in ((dict(attn_maps=True), "attn_maps="), (dict(timed=True), "timed=True"),
                     (dict(row_scale=(torch.ones(256, device="cuda"), None)), "row_scale=")):
        with pytest.raises(ValueError, match="differentiable eval route") as e:
            model(img, ev, None, None, None, **kw)
        assert frag in str(e.value)
    out = model(img.detach(), ev, None, None, None, timed=True)          # detached: the evaluation entry serves it as before
    assert out["logits"].grad_fn is None and model.last_stage_times is not None


# ---- 9. the C entry ------------------------------------------------------------------------------------------------------------------------
def test_the_entry_with_null_dx_is_iefvad_train_backward_and_a_misaligned_buffer_is_refused_by_name():
    """Through ctypes on the model's handle: a fresh iefvad_train_forward of the same batch before each backward; dx = NULL (and a dx of two
    null members) gives the bits of iefvad_train_backward for every parameter gradient; a misaligned dx->img fails by name before any
    launch -- the forward's record is still there, and the backward that follows on the same buffer gives the same bits again."""
    lib = L.load_library()
    model, _ = make_model(5, 2, 2)
    B, T, D = 2, 256, 768
    img, ev, _, _ = synth.make_train_batch(79, B)
    img, ev = torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()
    dev = img.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    model._ensure_handle(dev)
    model._ensure_weights(dev, stream)
    h = model._handle
    ws = torch.empty(lib.iefvad_train_workspace_bytes(h, B), dtype=torch.uint8, device=dev)
    gen = torch.Generator(device="cuda").manual_seed(11)
    d_logits = torch.randn(B * T, device="cuda", generator=gen)
    d_mu = torch.randn(B * T, D, device="cuda", generator=gen) * 1e-3
    dout = L.OutputGrads()
    dout.logits, dout.image_mu, dout.event_logvar = d_logits.data_ptr(), d_mu.data_ptr(), d_mu.data_ptr()
    params = list(model.temporal.parameters())

    def forward():
        outs = {k: torch.empty(B, T, 1 if k == "logits" else D, device=dev) for k in KEYS}
        o = L.Outputs()
        for k in KEYS:
            setattr(o, k, outs[k].data_ptr())
        opt = L.TrainOptions()
        rc = lib.iefvad_train_forward(h, C.c_void_p(img.data_ptr()), C.c_void_p(ev.data_ptr()), L.IN_F32, B, C.byref(opt), C.c_void_p(ws.data_ptr()),
                                      ws.numel(), C.byref(o), C.c_void_p(stream))
        assert rc == 0, L.last_error()
        return outs

    def backward(entry, *dx):
        grads = {id(q): torch.full_like(q, float("nan")) for q in params}
        dw = L.WeightGrads()
        model._fill_weight_struct(dw, lambda q: grads[id(q)].data_ptr())
        rc = getattr(lib, entry)(h, B, C.c_void_p(ws.data_ptr()), ws.numel(), C.byref(dout), C.byref(dw), *dx, C.c_void_p(stream))
        torch.cuda.synchronize()
        return rc, [grads[id(q)] for q in params]

    keep = forward()
    rc, want = backward("iefvad_train_backward")
    assert rc == 0, L.last_error()
    assert all(bool(torch.isfinite(g).all()) for g in want)
    for dx in (None, C.byref(L.InputGrads())):
        keep = forward()
        rc, got = backward("iefvad_train_backward_inputs", dx)
        assert rc == 0, L.last_error()
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    keep = forward()
    buf = torch.empty(B * T * D + 4, device=dev)
    rc, _ = backward("iefvad_train_backward_inputs", C.byref(L.InputGrads(buf.data_ptr() + 4, None)))
    msg = L.last_error()
    assert rc != 0 and msg.startswith("iefvad_train_backward_inputs:") and "16-byte aligned" in msg, msg
    gx = torch.empty(B * T, D, device=dev)
    rc, got = backward("iefvad_train_backward_inputs", C.byref(L.InputGrads(None, gx.data_ptr())))       # the record survived the refusal
    assert rc == 0, L.last_error()
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
    del keep
