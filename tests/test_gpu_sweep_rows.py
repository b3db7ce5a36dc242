"""The robustness sweep on valid rows (`iefvad_forward_videos_scaled`, csrc/ragged.h): per-row input scales and the unconditional NaN
rule in the device chunker, the column sums of the fusion weights over the valid rows reduced on the device, and
`harness.PerturbationSweep(ragged=True)` on top of them.  The reference route throughout is the padded one: host-side process_split,
`model(padded, row_scale=...)` (`iefvad_forward_scaled`), sliced to `[0:len]` -- which tests/test_gpu_config2.py pins to the
reference's own test2.py capture."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth
from iefvad_amd import lib as L
from tests import helpers as H

pytestmark = pytest.mark.gpu

EDGE = [37, 255, 256, 257, 512, 1500, 1, 300]      # 3,118 rows, 16 chunks: a one-row chunk, a len % 256 == 0 video, a six-chunk video
N = sum(EDGE)
T = 256


def make_model(compute, D=768, L_=2, K=3, **kw):
    sd = synth.make_state_dict(41, D, L_, K)
    args = argparse.Namespace(visual_layers=L_, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, D, 256, D, 8, L_, 8, 10, 10, "cuda", args, compute=compute, **kw)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


def videos(lengths, seed=6, dtype=np.float32, D=768):
    return [synth.make_video(seed, i, int(n), D=D, dtype=dtype) for i, n in enumerate(lengths)]


def pack(vids):
    return (torch.from_numpy(np.concatenate([v[0] for v in vids])).cuda(), torch.from_numpy(np.concatenate([v[1] for v in vids])).cuda())


def pad(vids):
    """Host-side chunker: ([C, 256, D] image, event) on the device, and per video (first chunk, chunk count)."""
    D = vids[0][0].shape[1]
    ci = [harness.process_split(v[0], T)[0].reshape(-1, T, D) for v in vids]
    ce = [harness.process_split(v[1], T)[0].reshape(-1, T, D) for v in vids]
    where, off = [], 0
    for c in ci:
        where.append((off, c.shape[0]))
        off += c.shape[0]
    return torch.from_numpy(np.concatenate(ci)).cuda(), torch.from_numpy(np.concatenate(ce)).cuda(), where


def valid_index(vids, where):
    return torch.cat([torch.arange(c0 * T, c0 * T + v[0].shape[0]) for v, (c0, _) in zip(vids, where)]).cuda()


def draw_scales(lengths, where, k=77, seed=1):
    """k random time steps per video at 0.01: the packed vector of the valid-row route and the [C * 256] one of the padded route."""
    gen = torch.Generator().manual_seed(seed)
    draws = [(torch.randperm(T, generator=gen)[:k], None) for _ in lengths]
    packed = harness.sweep_row_scales(lengths, draws, T)[0]
    padded = torch.ones(sum(n for _, n in where), T)
    for (c0, nch), d in zip(where, draws):
        padded[c0:c0 + nch, d[0]] = 0.01
    return packed.cuda(), padded.reshape(-1).cuda()


def padded_results(model, img, ev, valid, row_scale=None):
    with torch.no_grad():
        out = model(img, ev, None, None, None, row_scale=row_scale)
    return {k: out[k].reshape(-1)[valid] for k in ("logits", "w_i_mean", "w_e_mean")}


def rows_results(model, rows, lengths, **kw):
    with torch.no_grad():
        return model.forward_videos(rows[0], rows[1], lengths, **kw)


def _scaled_rows_equal_scaled_padded(model, dtype, D=768, exact=True):
    vids = videos(EDGE, dtype=dtype, D=D)
    rows = pack(vids)
    img, ev, where = pad(vids)
    valid = valid_index(vids, where)
    s, sp = draw_scales(EDGE, where)
    clean = rows_results(model, rows, EDGE)
    for use_i, use_e in ((True, False), (False, True), (True, True)):
        want = padded_results(model, img, ev, valid, row_scale=(sp if use_i else None, sp if use_e else None))
        got = rows_results(model, rows, EDGE, row_scale=(s if use_i else None, s if use_e else None))
        for k in want:
            assert got[k].shape == want[k].shape == (N,)
            d = float((got[k] - want[k]).abs().max())
            print(k, use_i, use_e, "max |rows - padded| =", d)
            if exact:
                assert torch.equal(got[k], want[k]), (k, use_i, use_e, d)
        if not exact:       # bf16x6: the gates of test_forward_videos_large_batch_bf16_kernels_and_bf16x6_tolerance for the same pair of routes
            assert float((torch.sigmoid(got["logits"]) - torch.sigmoid(want["logits"])).abs().max()) <= H.TOL_SIGMOID
            assert float((got["logits"] - want["logits"]).abs().max()) <= H.TOL_LOGIT
            assert float((got["w_i_mean"] - want["w_i_mean"]).abs().max()) <= 1e-5
            assert float((got["w_e_mean"] - want["w_e_mean"]).abs().max()) <= 1e-5
        assert not torch.equal(got["logits"], clean["logits"])


@pytest.mark.parametrize("micro_batch", [0, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("compute", ["f32", "bf16", "fp16x3"])
def test_scaled_valid_rows_equal_the_scaled_padded_forward(compute, dtype, micro_batch):
    """1. `forward_videos(row_scale=(s, None) / (None, s) / (s, s))` against `model(padded, row_scale=...)[0:len]`, bit for bit
    (include/iefvad.h: "Results equal those of iefvad_forward ... bit for bit").  With micro_batch = 3 the six-chunk video straddles
    passes: a pass must see its own slice of the scale vectors."""
    _scaled_rows_equal_scaled_padded(make_model(compute, outputs="scores", micro_batch=micro_batch), dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_scaled_valid_rows_bf16x6_within_the_fp32_gates(dtype):
    _scaled_rows_equal_scaled_padded(make_model("bf16x6", outputs="scores"), dtype, exact=False)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_no_extras_is_the_old_entry(compute):
    """2. NULL or all-ones scale vectors, with and without the column sums: the per-snippet results of `forward_videos` as it was."""
    model = make_model(compute, outputs="scores")
    rows = pack(videos(EDGE))
    old = rows_results(model, rows, EDGE)
    ones = torch.ones(N, device="cuda")
    for kw in (dict(row_scale=(None, None)), dict(row_scale=(ones, ones)), dict(row_scale=(ones, None), weight_sums=True),
               dict(weight_sums=True), dict(row_scale=(None, None), weight_sums=True)):
        got = rows_results(model, rows, EDGE, **kw)
        assert ("w_colsum" in got) == bool(kw.get("weight_sums"))
        for k in old:
            assert torch.equal(got[k], old[k]), (kw.keys(), k)
    assert "w_colsum" not in old


def _column_sums(model, D=768, exact=True):
    """`w_colsum` against the fp64 torch sum over the valid rows of w_i / w_e from the padded outputs="weights" forward of the same model.
    The summands are the same fp32 values and only the fp64 summation order differs: |error| <= (n - 1) u sum|w| + O(u^2) with
    u = 2^-53 for any order of n terms, so n 2^-52 sum|w| per column (n = 3,118) holds with room to spare -- derived, not measured."""
    vids = videos(EDGE, D=D)
    rows = pack(vids)
    img, ev, where = pad(vids)
    valid = valid_index(vids, where)
    with torch.no_grad():
        out = model(img, ev, None, None, None)
    got = rows_results(model, rows, EDGE, weight_sums=True)["w_colsum"]
    again = rows_results(model, rows, EDGE, weight_sums=True)["w_colsum"]
    assert got.shape == (2, D) and got.dtype == torch.float64
    assert torch.equal(got, again)                                       # fixed-order reduction: the same bits on every run
    for m, k in enumerate(("w_i", "w_e")):
        w = out[k].reshape(-1, D).double()
        want = w[valid].sum(dim=0)
        bound = N * 2.0 ** -52 * w[valid].abs().sum(dim=0)
        err = (got[m] - want).abs()
        print(k, "max |colsum - fp64 sum| =", float(err.max()), "min bound =", float(bound.min()), "n =", N)
        if exact:
            assert bool((err <= bound).all()), (k, float(err.max()), float(bound.min()))
            # a kernel that also counted pad rows (their weights are not zero) would be off by orders of magnitude more than the bound
            with_pad = w.sum(dim=0)
            assert w.shape[0] > N and float(((with_pad - want).abs() / bound).min()) > 1e6, k
        else:
            assert float(err.max()) / N <= H.TOL_BIG, (k, float(err.max()) / N)


@pytest.mark.parametrize("compute,micro_batch", [("f32", 0), ("f32", 3), ("bf16", 0), ("bf16", 3), ("fp16x3", 0)])
def test_column_sums_over_valid_rows(compute, micro_batch):
    """3. The row-compressed set (f32, bf16: the chunk table; bf16 at full grids stores the weights from its heads kernel) and
    fp16x3's whole chunks."""
    _column_sums(make_model(compute, outputs="weights", micro_batch=micro_batch))


def test_column_sums_on_the_compacted_row_set(monkeypatch):
    """3. IEFVAD_DENSE_ENCODER=1 (read when the handle is created, on the first forward): whole chunks in the encoder, the tail on the
    gathered valid rows in packed order -- 256-row slabs instead of the chunk table."""
    monkeypatch.setenv("IEFVAD_DENSE_ENCODER", "1")
    _column_sums(make_model("f32", outputs="weights"))


def test_column_sums_bf16x6():
    _column_sums(make_model("bf16x6", outputs="weights"), exact=False)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_unconditional_nan_rule(dtype):
    """4. nan_to_num="always" is torch.nan_to_num on every video and modality (test2.py:59-60): video 1 has +inf and no NaN, video 2 a
    NaN and -inf.  Against the padded forward on torch.nan_to_num(x), bit for bit including the NaN pattern (3.4e38 overflows inside
    the first projection, in the reference too; 65504 is harmless).  The per-video rule (True) leaves the inf-only video alone.  A
    scale on top is applied after the replacement: the row that held +inf carries 65504 * 0.01 in fp16."""
    lengths = [100, 300, 50, 80]
    vids = videos(lengths, seed=9, dtype=dtype)
    vids[1][0][7, 5] = np.inf
    vids[2][1][3, 9] = np.nan
    vids[2][1][40, 100] = -np.inf
    model = make_model("f32", outputs="scores")
    rows = pack(vids)
    fixed = [(torch.nan_to_num(torch.from_numpy(a)).numpy(), torch.nan_to_num(torch.from_numpy(b)).numpy()) for a, b in vids]
    img, ev, where = pad(fixed)
    valid = valid_index(fixed, where)
    off = np.concatenate([[0], np.cumsum(lengths)])

    def same(a, b, tag):
        for k in a:
            assert torch.equal(torch.isnan(a[k]), torch.isnan(b[k])), (tag, k)
            assert torch.equal(torch.nan_to_num(a[k], nan=-1.0), torch.nan_to_num(b[k], nan=-1.0)), (tag, k)

    got = rows_results(model, rows, lengths, nan_to_num="always")
    same(got, padded_results(model, img, ev, valid), "always")
    lg = got["logits"]
    assert bool(torch.isfinite(lg[off[0]:off[1]]).all()) and bool(torch.isfinite(lg[off[3]:]).all())
    if dtype == np.float16:
        assert bool(torch.isfinite(lg).all())
    rule = rows_results(model, rows, lengths, nan_to_num=True)["logits"]
    assert bool(torch.isnan(rule[off[1]:off[1] + 256]).all())             # inf without NaN: left alone, poisons its chunk
    if dtype == np.float16:
        assert bool(torch.isfinite(rule[off[2]:off[3]]).all())            # NaN -> 0, -inf -> -65504
    # a scale on the rows that held the non-finite values, after the replacement: torch's product on the replaced tensor
    s = torch.ones(sum(lengths))
    s[off[1] + 7] = 0.01
    s[off[2] + 3] = 0.01
    s[off[2] + 40] = 0.01
    s[off[3] + 11] = 0.01
    s = s.cuda()
    sp = torch.ones(img.shape[0] * T, device="cuda")
    sp[valid] = s
    si, se = img.clone(), ev.clone()
    pick = (sp != 1).reshape(-1, T)
    si[pick] = si[pick] * 0.01
    se[pick] = se[pick] * 0.01
    if dtype == np.float16:
        assert float(si.reshape(-1, 768)[valid][off[1] + 7, 5]) == float(torch.tensor(65504.0 * 0.01).half())
    got_s = rows_results(model, rows, lengths, nan_to_num="always", row_scale=(s, s))
    same(got_s, padded_results(model, si, se, valid), "always + scale")
    same(got_s, padded_results(model, img, ev, valid, row_scale=(sp, sp)), "always + scale vs iefvad_forward_scaled")
    assert not torch.equal(torch.nan_to_num(got_s["logits"], nan=-1.0), torch.nan_to_num(got["logits"], nan=-1.0))


def test_sweep_on_valid_rows_matches_the_reference_capture(golden_dir):
    """5. `run_perturbation_test(ragged=True)` with a scores-only model against the reference's own run_test capture, at the tolerances
    of the padded-route test (tests/test_gpu_config2.py); then against the default (padded) sweep under the same seed."""
    g = np.load(os.path.join(golden_dir, "sweep_test2.npz"))
    lengths, seed = [int(v) for v in g["lengths"]], int(g["seed"])
    total = sum(lengths)
    gt = synth.make_gt(seed, total)

    def loader():
        for i, n in enumerate(lengths):
            img, ev = synth.make_video(seed, i, n)
            ci, _ = harness.process_split(img, 256)
            ce, _ = harness.process_split(ev, 256)
            yield torch.tensor(ci).unsqueeze(0), torch.tensor(ce).unsqueeze(0), ("Normal",), torch.tensor([n])

    def gpu_model(outputs):
        a = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=10, lambda_ref=0.5, noise_model="StudentT", nu=8)
        m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, "cuda", a, outputs=outputs)
        m.load_state_dict(synth.make_state_dict(int(g["wseed"])))
        return m.to("cuda:0").eval()

    args = argparse.Namespace(visual_length=256)
    levels = (("img02", dict(sigma_img=0.2, sigma_ev=0)), ("ev03", dict(sigma_img=0, sigma_ev=0.3)))
    results = {}
    for ragged, outputs in ((True, "scores"), (False, "weights")):
        model = gpu_model(outputs)
        torch.manual_seed(0)
        cache = {}
        for tag, kw in levels:
            results[ragged, tag] = harness.run_perturbation_test(args, model, loader(), gt, "cuda:0", clean_cache=cache, ragged=ragged, **kw)
        if ragged:
            sweep = cache["sweep"]
            assert sweep.ragged and sweep.clean_passes == 1
            assert all(r.is_cuda and tuple(r.shape) == (total, 768) for r in sweep.rows)       # uploaded once, valid rows only
            ptrs = [r.data_ptr() for r in sweep.rows]
            clean_rows = sweep.clean()
    for tag, _ in levels:
        r = results[True, tag]
        assert np.allclose([float(x) for x in r[:10]], g[tag + "_scalars"], rtol=0, atol=2e-6), tag
        assert np.abs(r[10].numpy() - g[tag + "_w_img_change"]).max() < 2e-6
        assert np.abs(r[11].numpy() - g[tag + "_w_ev_change"]).max() < 2e-6
    assert [r.data_ptr() for r in sweep.rows] == ptrs and sweep.clean_passes == 1
    # the two routes under one seed: same draws, same per-snippet bits in f32, so the ten scalars agree to 1e-12.  The per-dimension
    # sums differ by the fp64 summation order only: each column sum is within n 2^-52 sum|w| (test 3; the weights lie in (0, 1), so
    # sum|w| <= n), a change vector is the difference of two of them divided by `total`, and it is returned in fp32, which rounds the
    # two routes' values to within one fp32 ulp (2^-23 relative) of each other.
    clean_padded = cache["sweep"].clean()
    for k in ("wi_dim", "we_dim"):
        bound = total * 2.0 ** -52 * clean_padded[k].abs()              # n 2^-52 sum|w| / total, sum|w| = the column sum itself (w > 0)
        assert bool(((clean_rows[k] - clean_padded[k]).abs() <= bound).all()), k
    for tag, _ in levels:
        a, b = results[True, tag], results[False, tag]
        assert np.allclose([float(x) for x in a[:10]], [float(x) for x in b[:10]], rtol=0, atol=1e-12), tag
        for i in (10, 11):
            tol = 2 * total * 2.0 ** -52 + 2.0 ** -23 * float(b[i].abs().max())
            assert float((a[i] - b[i]).abs().max()) <= tol, (tag, i, float((a[i] - b[i]).abs().max()), tol)


def test_d512_scaled_rows_and_column_sums():
    """6. ViT-B/16 features (D = 512, f32 arithmetic): tests 1 and 3 once."""
    _scaled_rows_equal_scaled_padded(make_model("f32", D=512, outputs="scores"), np.float32, D=512)
    _column_sums(make_model("f32", D=512, outputs="weights"), D=512)


def test_argument_checks_of_the_scaled_entry():
    """With a live handle: the checks that need one, each refused before any launch with a message that names the entry."""
    model = make_model("f32", outputs="scores")
    rows = pack(videos([5, 7]))
    rows_results(model, rows, [5, 7])                                        # creates the handle and sets the weights
    lib = L.load_library()
    lens = (C.c_int32 * 2)(5, 7)
    bad = (C.c_int32 * 2)(5, 0)
    wb = lib.iefvad_videos_scaled_workspace_bytes
    base = lib.iefvad_videos_workspace_bytes(model._handle, lens, 2)
    assert wb(model._handle, lens, 2, 0) == base and wb(model._handle, lens, 2, 1) > base + 2 * 2 * 256 * 768 * 4
    assert wb(model._handle, None, 2, 1) == 0 and wb(model._handle, lens, 0, 1) == 0 and wb(model._handle, bad, 2, 1) == 0
    ws = torch.empty(wb(model._handle, lens, 2, 1), dtype=torch.uint8, device="cuda")
    lg = torch.empty(12, device="cuda")
    cs = torch.empty(2 * 768 + 1, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(img=rows[0], ev=rows[1], lengths=lens, nan=2, wsb=ws.numel(), logits=lg, colsum=p(cs)):
        rc = lib.iefvad_forward_videos_scaled(model._handle, p(img), p(ev), L.IN_F32, lengths, 2, nan, None, None, p(ws), wsb, p(logits), None, None,
                                              colsum, None)
        return rc, L.last_error()

    for kw, frag in [(dict(img=None), "null"), (dict(ev=None), "null"), (dict(lengths=None), "null"), (dict(logits=None), "null"),
                     (dict(nan=3), "nan_to_num"), (dict(nan=-1), "nan_to_num"), (dict(colsum=C.c_void_p(cs.data_ptr() + 4)), "w_colsum"),
                     (dict(lengths=bad), "lengths[1]"), (dict(wsb=base), "workspace too small")]:
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("iefvad_forward_videos_scaled:") and frag in msg, (kw, msg)
    assert call(wsb=base, colsum=None)[0] == 0                               # without the column sums the base workspace is enough
    assert call()[0] == 0
    torch.cuda.synchronize()
