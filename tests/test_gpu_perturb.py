"""The noise study's row perturbations on the device (`iefvad_forward_perturbed`, `iefvad_forward_videos_perturbed`,
`iefvad_perturb_rows`, include/iefvad.h; csrc/common.h gauss_pair / add_row_noise4): additive Gaussian noise drawn by a counter-based
generator inside the input load, next to the row scale.  The reference declares the study's flags and implements none of them
(test2.py:35-37,214-220): nothing here is a parity test ("parity unpinned").  What is pinned is internal consistency -- the generator
against its host model (`harness.gaussian_rows`), the order of the roundings against torch's, the fused loads against perturbed rows
materialised first, the valid-row route against the padded one, and the calls without noise against the entries that were there before.
Lists are eight videos of 1 .. 300 snippets (ten chunks; a 256-snippet video, a one-row chunk), models have L = 2, K = 2."""
import argparse
import ctypes as C
import math

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth
from iefvad_amd import lib as L
from tests import helpers as H
from tests.test_perturb_cpu import normal_statistics

pytestmark = pytest.mark.gpu

LENGTHS = [1, 37, 128, 129, 255, 256, 257, 300]
N = sum(LENGTHS)
T = 256
SEED = 1234


def make_model(compute, D=768, outputs="scores", **kw):
    sd = synth.make_state_dict(41, D, 2, 2)
    args = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=2, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, D, 256, D, 8, 2, 8, 10, 10, "cuda", args, compute=compute, outputs=outputs, **kw)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


def videos(dtype=np.float32, D=768, seed=6):
    return [synth.make_video(seed, i, n, D=D, dtype=dtype) for i, n in enumerate(LENGTHS)]


def pack(vids):
    return (torch.from_numpy(np.concatenate([v[0] for v in vids])).cuda(), torch.from_numpy(np.concatenate([v[1] for v in vids])).cuda())


def pad(vids):
    """Host-side chunker (tools.py:100-114): [C, 256, D] image and event chunks on the device, the index of every valid row in them"""
    D = vids[0][0].shape[1]
    ci = [harness.process_split(v[0], T)[0].reshape(-1, T, D) for v in vids]
    ce = [harness.process_split(v[1], T)[0].reshape(-1, T, D) for v in vids]
    valid, off = [], 0
    for c, v in zip(ci, vids):
        valid.append(torch.arange(off * T, off * T + v[0].shape[0]))
        off += c.shape[0]
    return torch.from_numpy(np.concatenate(ci)).cuda(), torch.from_numpy(np.concatenate(ce)).cuda(), torch.cat(valid).cuda()


def device_eps(seed, rows, D=768, ids=None):
    """The device's own eps of both modalities: the unit entry on fp32 zeros with amplitude 1"""
    z, one = torch.zeros(rows, D, device="cuda"), torch.ones(rows, device="cuda")
    return iefvad_amd.perturb_rows(z, z, row_noise=(one, one), noise_seed=seed, noise_rows=ids)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def row_vectors(n, seed=3, big=None):
    """Packed test vectors over n rows: scales from {1, 0.01, 0, 10}, amplitudes from {0, 0.3} (and `big` on every 17th row)"""
    gen = torch.Generator().manual_seed(seed)
    s = torch.tensor([1.0, 0.01, 0.0, 10.0])[torch.randint(0, 4, (n,), generator=gen)]
    a = torch.tensor([0.0, 0.3])[torch.randint(0, 2, (n,), generator=gen)]
    if big:
        a[::17] = big
    return s.cuda(), a.cuda()


# ------------------------------------------------------------------------------------------------ generator
GEN_DIFF_RECORDED = 4.768e-07   # the first run's measurement (both modalities; one fp32 ulp of a value in [4, 8)): the gate is 4 x this


def test_generator_against_the_host_model():
    """`perturb_rows` on fp32 zeros with amplitude 1 returns eps.  Worst |device - gaussian_rows| over 1024 x 768 samples (seed 1234,
    modality 0; fp32 logf / sqrtf / sincospif on the device, fp64 rounded once on the host): the gate is 4 x the value recorded on the first run
    (4.768e-07 for either modality: GEN_DIFF_RECORDED, profiles/perturb_tests.log); the margin is for a compiler that picks other log /
    sin expansions.  The
    statistics of tests/test_perturb_cpu.py hold for the device's sample at 4 standard errors."""
    e0, e1 = device_eps(SEED, 1024)
    h0 = harness.gaussian_rows(SEED, 0, np.arange(1024), 768)
    h1 = harness.gaussian_rows(SEED, 1, np.arange(1024), 768)
    d0 = float(np.abs(e0.cpu().numpy().astype(np.float64) - h0).max())
    d1 = float(np.abs(e1.cpu().numpy().astype(np.float64) - h1).max())
    print(f"worst |device eps - host model| modality 0: {d0:.3e}, modality 1: {d1:.3e}, max |eps| {float(e0.abs().max()):.3f}")
    assert d0 <= 4 * GEN_DIFF_RECORDED and d1 <= 4 * GEN_DIFF_RECORDED
    assert float(e0.abs().max()) <= math.sqrt(48 * math.log(2)) * (1 + 1e-6)
    for name, got, want, se in normal_statistics(e0.cpu().numpy(), e1.cpu().numpy()):
        print(f"{name}: {got:+.6f} ({abs(got - want) / se:.2f} standard errors)")
        assert abs(got - want) < 4 * se, name


def test_generator_is_a_pure_function_of_seed_modality_id_and_column():
    e0, e1 = device_eps(SEED, 300)
    a0, a1 = device_eps(SEED, 300)
    assert torch.equal(bits(e0), bits(a0)) and torch.equal(bits(e1), bits(a1))          # the same call twice
    assert not torch.equal(e0, e1)                                                      # the modalities differ
    assert not torch.equal(e0, device_eps(SEED + 1, 300)[0])                            # another seed
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(1)).to(torch.int32).cuda()
    p0, p1 = device_eps(SEED, 300, ids=perm)
    assert torch.equal(bits(p0), bits(e0[perm.long()])) and torch.equal(bits(p1), bits(e1[perm.long()]))
    far = torch.tensor([2 ** 31 - 1, 0, 2 ** 20], dtype=torch.int32).cuda()            # ids past 2^21: the index needs its high word
    f0, _ = device_eps(SEED, 3, ids=far)
    want = harness.gaussian_rows(SEED, 0, [2 ** 31 - 1, 0, 2 ** 20], 768)
    assert float(np.abs(f0.cpu().numpy() - want).max()) <= 4 * GEN_DIFF_RECORDED
    assert torch.equal(bits(f0[1]), bits(e0[0]))
    d512 = device_eps(SEED, 5, D=512)[0]
    assert torch.equal(bits(d512), bits(e0[:5, :512]))                                  # a column's noise does not depend on the width


# ------------------------------------------------------------------------------------------------ rounding order
@pytest.mark.parametrize("D", [768, 512])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_rounding_order_is_torchs(dtype, D):
    """Scales {1, 0.01, 0, 10} x amplitudes {0, 0.3, 50}: `perturb_rows` equals, bit for bit, y = T(fp32(x) * scale) where scale != 1 and
    z = T(fp32(y) + amp * eps) where amp != 0, formed by torch from the device's own fp32 eps.  Rows with scale 1 and amplitude 0 keep
    their bits, NaN payloads and -0 included; with nan_to_num the replacement happens first."""
    scales, amps = [1.0, 0.01, 0.0, 10.0], [0.0, 0.3, 50.0]
    s = torch.tensor([sc for sc in scales for _ in amps] * 3).cuda()
    a = torch.tensor([am for _ in scales for am in amps] * 3).cuda()
    R = s.numel()
    gen = torch.Generator().manual_seed(2)
    x = [(torch.randn(R, D, generator=gen) * 0.45).to(dtype).cuda() for _ in (0, 1)]
    for m in (0, 1):
        x[m][:, 3] = -0.0
        x[m][:, 5] = float("nan")
        x[m][:, 9] = float("inf")
        x[m][:, 10] = -float("inf")
    if dtype == torch.float32:       # a NaN with a payload in the untouched row
        x[0].view(torch.int32)[0, 7] = 0x7FC12345
    eps = device_eps(SEED, R, D)
    for nan in (False, True):
        got = iefvad_amd.perturb_rows(x[0], x[1], row_scale=(s, s), row_noise=(a, a), noise_seed=SEED, nan_to_num=nan)
        for m in (0, 1):
            src = torch.nan_to_num(x[m]) if nan else x[m]
            y = torch.where((s != 1)[:, None], (src.float() * s[:, None]).to(dtype), src)
            z = torch.where((a != 0)[:, None], (y.float() + a[:, None] * eps[m]).to(dtype), y)
            same = bits(got[m]) == bits(z)
            both_nan = torch.isnan(got[m]) & torch.isnan(z)       # a NaN that went through arithmetic: torch and the kernel may differ in payload
            touched = ((s != 1) | (a != 0))[:, None].expand_as(same)
            assert bool((same | (both_nan & touched)).all()), (dtype, D, nan, m, int((~same).sum()))
            if not nan:
                assert torch.equal(bits(got[m][0]), bits(x[m][0]))                       # scale 1, amplitude 0: the bits of the source
        assert bool(torch.isnan(got[0]).any()) != nan
    only = iefvad_amd.perturb_rows(None, x[1], row_noise=(None, a), noise_seed=SEED)
    assert only[0] is None and only[1].dtype == dtype


# ------------------------------------------------------------------------------------------------ fused = materialised
def _fused_equals_materialised(model, dtype, D, exact, big=None):
    B = 3
    xi, xe = (torch.from_numpy(v).cuda() for v in synth.make_inputs(5, B, T, D, dtype=dtype))
    n = B * T
    s, a = row_vectors(n, big=big)
    s2, a2 = row_vectors(n, seed=4, big=big)
    ids = torch.randperm(5000, generator=torch.Generator().manual_seed(2))[:n].to(torch.int32).cuda()
    for kw in (dict(row_scale=(s, s2), row_noise=(a, a2), noise_rows=ids), dict(row_noise=(a, None)), dict(row_scale=(None, s), row_noise=(None, a2))):
        with torch.no_grad():
            got = model(xi, xe, noise_seed=SEED, **kw)
            mi, me = iefvad_amd.perturb_rows(xi.reshape(n, D), xe.reshape(n, D), noise_seed=SEED, **kw)
            want = model(mi.reshape(B, T, D), me.reshape(B, T, D))
            clean = model(xi, xe)
        assert set(got) >= set(iefvad_amd.OUTPUT_KEYS)
        for k in iefvad_amd.OUTPUT_KEYS:
            d = float((got[k] - want[k]).abs().max())
            if exact:
                assert torch.equal(got[k], want[k]), (k, d)
            else:
                assert d <= (H.TOL_LOGIT if k == "logits" else H.TOL_BIG), (k, d)
        if not exact:
            assert float((torch.sigmoid(got["logits"]) - torch.sigmoid(want["logits"])).abs().max()) <= H.TOL_SIGMOID
        assert not torch.equal(got["logits"], clean["logits"])


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("compute", ["f32", "bf16", "fp16x3"])
def test_forward_perturbed_equals_forward_of_materialised_rows(compute, dtype):
    """`model(x, row_scale=, row_noise=)` against `model(perturb_rows(x, ...))`, bit for bit on all eight outputs.  fp16x3 with amplitude
    50 on every 17th row: its per-chunk operand scale is taken from the chunker's fp32 output, so it sees the perturbed rows."""
    _fused_equals_materialised(make_model(compute, outputs="full"), dtype, 768, True, big=50.0 if compute == "fp16x3" else None)


def test_forward_perturbed_d512():
    _fused_equals_materialised(make_model("f32", D=512, outputs="full"), np.float32, 512, True)


@pytest.mark.parametrize("invariant", [False, True])
def test_forward_perturbed_bf16x6(invariant):
    """bf16x6 at the suite's fp32 gates; with batch_invariant=True bit for bit."""
    _fused_equals_materialised(make_model("bf16x6", outputs="full", batch_invariant=invariant), np.float32, 768, invariant)


def _videos_equal_materialised(model, dtype=np.float32, D=768, exact=True, nan="default", big=None):
    vids = videos(dtype, D)
    if nan == "always":
        vids[3][0][7, 5] = np.nan
        vids[4][1][200, 9] = np.inf
    rows = pack(vids)
    s, a = row_vectors(N, big=big)
    s2, a2 = row_vectors(N, seed=4, big=big)
    nan_kw = dict(nan_to_num="always") if nan == "always" else {}
    for kw in (dict(row_scale=(s, s2), row_noise=(a, a2)), dict(row_noise=(None, a))):
        with torch.no_grad():
            got = model.forward_videos(rows[0], rows[1], LENGTHS, noise_seed=SEED, weight_sums=True, **nan_kw, **kw)
            mat = iefvad_amd.perturb_rows(rows[0], rows[1], noise_seed=SEED, nan_to_num=nan == "always", **kw)
            want = model.forward_videos(mat[0], mat[1], LENGTHS, weight_sums=True, **nan_kw)
        for k in ("logits", "w_i_mean", "w_e_mean", "w_colsum"):
            assert torch.equal(torch.isnan(got[k]), torch.isnan(want[k])), k      # (3.4e38 * 10 overflows, in both: the NaN pattern is part of the result)
            g, w = torch.nan_to_num(got[k], nan=-1.0), torch.nan_to_num(want[k], nan=-1.0)
            d = float((g - w).abs().max())
            if exact:
                assert torch.equal(g, w), (k, d)
            else:
                assert d <= {"logits": H.TOL_LOGIT, "w_colsum": H.TOL_BIG * N}.get(k, 1e-5), (k, d)


@pytest.mark.parametrize("micro_batch", [0, 3])
@pytest.mark.parametrize("compute,dtype", [("f32", np.float32), ("f32", np.float16), ("bf16", np.float32), ("fp16x3", np.float32)])
def test_forward_videos_perturbed_equals_forward_videos_of_materialised_rows(compute, dtype, micro_batch):
    """The valid-row route, NULL ids (the call's packed row): with micro_batch = 3 the ten chunks fall into four passes and the two-chunk
    videos straddle them -- a pass must add its own first row to the ids and see its own slice of the vectors."""
    _videos_equal_materialised(make_model(compute, micro_batch=micro_batch), dtype, big=50.0 if compute == "fp16x3" else None)


def test_forward_videos_perturbed_dense_encoder(monkeypatch):
    monkeypatch.setenv("IEFVAD_DENSE_ENCODER", "1")
    _videos_equal_materialised(make_model("f32"))


def test_forward_videos_perturbed_nan_rule_always_comes_first():
    _videos_equal_materialised(make_model("f32"), nan="always")


def test_forward_videos_perturbed_d512_and_bf16x6():
    _videos_equal_materialised(make_model("f32", D=512), D=512)
    _videos_equal_materialised(make_model("bf16x6"), exact=False)


# ------------------------------------------------------------------------------------------------ routes agree
def test_valid_row_route_equals_padded_route_with_list_ids():
    """The valid-row entry with NULL ids against the `[0:len]` rows of the padded entry on host-padded chunks whose ids name the snippet in
    the list: bit for bit in f32 for the logits and both weight means; the column sums within the fp64 summation-order bound of
    tests/test_gpu_sweep_rows.py (n 2^-52 sum|w| per column)."""
    vids = videos()
    rows = pack(vids)
    img, ev, valid = pad(vids)
    s, a = row_vectors(N)
    s2, a2 = row_vectors(N, seed=4)
    rows_all = img.shape[0] * T
    def padded(v, fill):
        out = torch.full((rows_all,), fill, device="cuda", dtype=v.dtype)
        out[valid] = v
        return out
    ids = padded(torch.arange(N, dtype=torch.int32, device="cuda"), 0)
    with torch.no_grad():
        got = make_model("f32").forward_videos(rows[0], rows[1], LENGTHS, row_scale=(s, s2), row_noise=(a, a2), noise_seed=SEED, weight_sums=True)
        out = make_model("f32", outputs="weights")(img, ev, row_scale=(padded(s, 1.0), padded(s2, 1.0)), row_noise=(padded(a, 0.0), padded(a2, 0.0)),
                                                  noise_seed=SEED, noise_rows=ids)
    for k in ("logits", "w_i_mean", "w_e_mean"):
        assert torch.equal(got[k], out[k].reshape(-1)[valid]), k
    for m, k in enumerate(("w_i", "w_e")):
        w = out[k].reshape(-1, 768).double()[valid]
        err = (got["w_colsum"][m] - w.sum(dim=0)).abs()
        assert bool((err <= N * 2.0 ** -52 * w.abs().sum(dim=0)).all()), (k, float(err.max()))


# ------------------------------------------------------------------------------------------------ no-ops
def test_without_amplitudes_the_entries_return_the_scaled_entries_bits():
    """Both amplitude vectors NULL (the C entries called directly) or all zeros: the bits of iefvad_forward_scaled /
    iefvad_forward_videos_scaled.  A graph-replayed small-batch forward before and after a perturbed call keeps its bits."""
    model = make_model("f32")
    lib = L.load_library()
    rows = pack(videos())
    s, _ = row_vectors(N)
    zero = torch.zeros(N, device="cuda")
    with torch.no_grad():
        want = model.forward_videos(rows[0], rows[1], LENGTHS, row_scale=(s, None), weight_sums=True)
        got = model.forward_videos(rows[0], rows[1], LENGTHS, row_scale=(s, None), row_noise=(zero, zero), noise_seed=1, weight_sums=True)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    p = L.Perturb()
    p.scale[0] = s.data_ptr()
    p.seed = 77
    lens = (C.c_int32 * len(LENGTHS))(*LENGTHS)
    ws = torch.empty(lib.iefvad_videos_scaled_workspace_bytes(model._handle, lens, len(LENGTHS), 1), dtype=torch.uint8, device="cuda")
    res = {k: torch.empty(N, device="cuda") for k in ("logits", "w_i_mean", "w_e_mean")}
    res["w_colsum"] = torch.empty(2, 768, dtype=torch.float64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.iefvad_forward_videos_perturbed(model._handle, ptr(rows[0]), ptr(rows[1]), L.IN_F32, lens, len(LENGTHS), 1, C.byref(p), ptr(ws), ws.numel(),
                                             ptr(res["logits"]), ptr(res["w_i_mean"]), ptr(res["w_e_mean"]), ptr(res["w_colsum"]),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(res[k], want[k]), k
    # the padded entry: B = 2 is served by a graph replay
    xi, xe = (torch.from_numpy(v).cuda() for v in synth.make_inputs(5, 2))
    sp, ap = row_vectors(2 * T)
    with torch.no_grad():
        before = model(xi, xe)
        scaled = model(xi, xe, row_scale=(sp, None))
        zeroed = model(xi, xe, row_scale=(sp, None), row_noise=(torch.zeros_like(ap), None), noise_seed=5)
        noisy = model(xi, xe, row_scale=(sp, None), row_noise=(ap, None), noise_seed=5)
        after = model(xi, xe)
    o = L.Outputs()
    direct = {k: torch.empty_like(scaled[k]) for k in ("logits", "w_i_mean", "w_e_mean")}
    for k in direct:
        setattr(o, k, direct[k].data_ptr())
    p2 = L.Perturb()
    p2.scale[0] = sp.data_ptr()
    rc = lib.iefvad_forward_perturbed(model._handle, ptr(xi), ptr(xe), L.IN_F32, 2, C.byref(p2), ptr(model._workspace), model._workspace.numel(),
                                      C.byref(o), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    for k in ("logits", "w_i_mean", "w_e_mean"):
        assert torch.equal(zeroed[k], scaled[k]) and torch.equal(direct[k], scaled[k]), k
        assert torch.equal(before[k], after[k]), k
    assert not torch.equal(noisy["logits"], scaled["logits"])


# ------------------------------------------------------------------------------------------------ sweep
def _loader(zero=None):
    """The list as the reference's loader delivers it; `zero[v]` = the modality whose features are zeroed by hand in video v"""
    for i, n in enumerate(LENGTHS):
        img, ev = synth.make_video(6, i, n)
        if zero is not None and zero[i] == 0:
            img = np.zeros_like(img)
        if zero is not None and zero[i] == 1:
            ev = np.zeros_like(ev)
        ci, _ = harness.process_split(img, T)
        ce, _ = harness.process_split(ev, T)
        yield torch.tensor(ci).unsqueeze(0), torch.tensor(ce).unsqueeze(0), ("Normal",), torch.tensor([n])


def _sweep(ragged, zero=None):
    model = make_model("f32", outputs="scores" if ragged else "weights")
    return harness.PerturbationSweep(argparse.Namespace(visual_length=T), model, _loader(zero), synth.make_gt(6, N), "cuda:0", batch_chunks=4,
                                     ragged=ragged)


def test_sweep_levels_agree_between_the_routes():
    """One seed, a level that mixes all kinds (attenuation 0.1, noise 0.2, outliers 0.1 at 3 sigma, drop 0.5): `ragged=True` and the
    padded route (four batches) return the same 12 results -- the ten scalars exactly in f32 (same draws, same per-snippet bits), the two
    change vectors within the bound of tests/test_gpu_sweep_rows.py (fp64 summation order, then one fp32 rounding).  The same seed gives
    the same result twice; all new levels at 0 give the legacy level's bits."""
    level = dict(noise_sigma_img=0.2, noise_sigma_ev=0.2, outlier_img=0.1, outlier_ev=0.1, outlier_sigma=3.0, dropout_prob=0.5)
    res = {}
    for ragged in (True, False):
        sweep = _sweep(ragged)
        torch.manual_seed(0)
        res[ragged] = sweep.level(0.1, 0, **level)
        torch.manual_seed(0)
        again = sweep.level(0.1, 0, **level)
        assert [float(x) for x in again[:10]] == [float(x) for x in res[ragged][:10]]
        assert torch.equal(again[10], res[ragged][10]) and torch.equal(again[11], res[ragged][11])
        torch.manual_seed(0)
        legacy = sweep.level(0.1, 0.2)
        torch.manual_seed(0)
        zeros = sweep.level(0.1, 0.2, noise_sigma_img=0, noise_sigma_ev=0, outlier_img=0, outlier_ev=0, dropout_prob=0, noise_seed=9)
        assert [float(x) for x in zeros[:10]] == [float(x) for x in legacy[:10]]
        assert torch.equal(zeros[10], legacy[10]) and torch.equal(zeros[11], legacy[11])
        assert [float(x) for x in legacy[:10]] != [float(x) for x in res[ragged][:10]]
        assert sweep.clean_passes == 1
    a, b = res[True], res[False]
    print("ragged", [float(x) for x in a[:10]])
    print("padded", [float(x) for x in b[:10]])
    assert [float(x) for x in a[:10]] == [float(x) for x in b[:10]]
    for i in (10, 11):
        tol = 2 * N * 2.0 ** -52 + 2.0 ** -23 * float(b[i].abs().max())
        assert float((a[i] - b[i]).abs().max()) <= tol, (i, float((a[i] - b[i]).abs().max()), tol)


def test_dropout_prob_one_equals_rows_zeroed_by_hand():
    """dropout_prob = 1 drops one modality in every video (row scale 0 on all its rows).  Against a sweep over the same list with the
    chosen modality's features zeroed by hand: every result that depends on the perturbed pass alone -- Brier, the weight means, AUC, AP,
    the four class-conditional weight means -- is equal (the KL term and the change vectors also depend on the clean pass, which differs)."""
    sweep = _sweep(True)
    torch.manual_seed(4)
    got = sweep.level(0, 0, dropout_prob=1.0)
    torch.manual_seed(4)
    zero = []
    for _ in LENGTHS:
        u = torch.rand(2)
        zero.append(0 if float(u[1]) < 0.5 else 1)
    assert set(zero) == {0, 1}
    want = _sweep(True, zero).level(0, 0)
    for i in (0, 2, 3, 4, 5, 6, 7, 8, 9):
        assert float(got[i]) == float(want[i]), (harness.SweepResult.FIELDS[i], float(got[i]), float(want[i]))


# ------------------------------------------------------------------------------------------------ error paths
def test_error_paths_with_device_tensors():
    model = make_model("f32")
    rows = pack(videos())
    a = torch.ones(N, device="cuda")
    ids = torch.arange(N, dtype=torch.int32, device="cuda")
    fv = lambda **kw: model.forward_videos(rows[0], rows[1], LENGTHS, **kw)
    with pytest.raises(ValueError, match="noise_seed"):
        fv(row_noise=(a, None))
    for kw in (dict(row_noise=(a[:-1], None)), dict(row_noise=(a.double(), None)), dict(row_noise=(a.cpu(), None)), dict(row_noise=(a,)),
               dict(row_noise=(a, None), noise_rows=ids.long()), dict(row_noise=(a, None), noise_rows=ids[:-1])):
        with pytest.raises(ValueError, match="row_noise|noise_rows"):
            fv(noise_seed=1, **kw)
    for kw in (dict(similarity=True), dict(outputs="full"), dict(attn_maps=True)):
        with pytest.raises(ValueError, match="does not combine"):
            fv(row_noise=(a, None), noise_seed=1, **kw)
    with pytest.raises(TypeError):
        model.forward_videos_host([rows[0].cpu()], [rows[1].cpu()], [N], row_noise=(a, None), noise_seed=1)
    x = torch.zeros(1, T, 768, device="cuda")
    with pytest.raises(ValueError, match="noise_seed"):
        model(x, x, row_noise=(a[:T].contiguous(), None))
    with pytest.raises(ValueError, match="row_noise"):
        model(x, x, row_noise=(a, None), noise_seed=1)
    with pytest.raises(ValueError, match="does not combine"):
        model(x, x, row_noise=(a[:T].contiguous(), None), noise_seed=1, attn_maps=True)
    with pytest.raises(ValueError, match="one shape"):
        iefvad_amd.perturb_rows(rows[0], rows[1][:-1])
    with pytest.raises(RuntimeError, match="D must be"):
        iefvad_amd.perturb_rows(rows[0][:, :640].contiguous(), None)
