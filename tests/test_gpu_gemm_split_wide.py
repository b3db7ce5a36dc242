"""The two tilings of the bf16x6 split projection (csrc/gemm_split.h): 128 x 128 (iefvad_gemm_split_n128_kernel) and 128 x 256 as two
column halves that share a wave's A planes (iefvad_gemm_split_n128x2_kernel).  Both sum every output element over its k-tiles in
ascending order and over the six products of a k-tile in one order, so they must agree BIT FOR BIT -- which is what lets the launch
rule (plan_gemm_split in csrc/launch_rules.h) choose a tiling by grid size alone.  The unit entry iefvad_gemm_split_unit names the
tiling; whole forwards take it from IEFVAD_SPLIT_TILE at iefvad_create.  Needs a real MI355X: run with `-m gpu`."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import lib as L
from iefvad_amd import synth
from oracle import iefvad_oracle as orc
from tests import helpers as H

pytestmark = pytest.mark.gpu

ALPHA = 0.5
# |fp32-accumulated result - fp64 result| stays far below this at K <= 768 with these operands (measured ~1e-6; the worst case
# K 2^-24 sum |a w| is ~6e-4); an element that was not written, or went to the wrong place, is off by O(1)
PLACED = 1e-3


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _operands(M, N, K, nz, seed):
    """Asymmetric operands, as in test_split_gemm_is_at_least_as_accurate_as_fp32_mfma: a transposed accumulator map would show."""
    rng = np.random.default_rng(seed)
    ops = []
    for _ in range(nz):
        A = (rng.standard_normal((M, K)) * 1.3).astype(np.float32)
        W = (rng.uniform(-1, 1, (N, K)) / np.sqrt(K)).astype(np.float32)
        b = rng.standard_normal(N).astype(np.float32)
        dA, dW, db = (torch.from_numpy(x).cuda() for x in (A, W, b))
        planes = torch.empty(3, N, K, dtype=torch.bfloat16, device="cuda")
        assert L.load_library().iefvad_split_bf16x3(dW.data_ptr(), planes.data_ptr(), N * K, _stream()) == 0, L.last_error()
        ops.append(dict(A=A, W=W, b=b, dA=dA, dW=dW, db=db, planes=planes, acc=A.astype(np.float64) @ W.astype(np.float64).T + b))
    return ops


def _unit(ops, M, N, K, ldc, epi, tile_n, C_=None, C2=None, R=None, qcols=0, alpha=ALPHA):
    io = L.GemmSplitIO()
    for m, o in enumerate(ops):
        io.A[m], io.W[m], io.bias[m] = o["dA"].data_ptr(), o["planes"].data_ptr(), o["db"].data_ptr()
        io.C[m] = C_[m].data_ptr() if C_ is not None and C_[m] is not None else None
        io.C2[m] = C2[m].data_ptr() if C2 is not None else None
        io.R[m] = R[m].data_ptr() if R is not None else None
    rc = L.load_library().iefvad_gemm_split_unit(C.byref(io), M, N, K, ldc, epi, qcols, alpha, len(ops), tile_n, _stream())
    torch.cuda.synchronize()
    return rc


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))       # bits; a NaN left in either fails the closeness checks


@pytest.mark.parametrize("nz", [1, 2])
@pytest.mark.parametrize("N", [256, 768])
@pytest.mark.parametrize("K", [64, 768])
@pytest.mark.parametrize("M", [128, 384])
def test_wide_tiling_equals_narrow_tiling(M, K, N, nz):
    """bias, bias + ReLU, bias + residual and the in-place refine epilogue, one or two problems per launch.  K = 64 is the minimum
    of two k-tiles (prologue, one steady pair of half-tiles, the zero-record tail); N = 256 is a single wide tile, M = 384 x N = 768
    a grid of 9 workgroups, both below the 8-XCD remap's size."""
    ops = _operands(M, N, K, nz, seed=M + K + N + nz)
    rng = np.random.default_rng(3)
    R0 = [torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).cuda() for _ in range(nz)]
    for epi in (L.SPLIT_EPI_BIAS, L.SPLIT_EPI_BIAS_RELU, L.SPLIT_EPI_BIAS_RESID, L.SPLIT_EPI_REFINE):
        got = {}
        for tile in (128, 256):
            if epi == L.SPLIT_EPI_REFINE:              # in place: C == R
                Cs = [r.clone() for r in R0]
                Rs = Cs
            else:
                Cs = [_nan(M, N) for _ in range(nz)]
                Rs = R0 if epi == L.SPLIT_EPI_BIAS_RESID else None
            assert _unit(ops, M, N, K, N, epi, tile, C_=Cs, R=Rs) == 0, L.last_error()
            got[tile] = Cs
        for m in range(nz):
            assert _same(got[256][m], got[128][m]), (epi, m)
            acc, r = ops[m]["acc"], R0[m].cpu().numpy().astype(np.float64)
            want = {L.SPLIT_EPI_BIAS: acc, L.SPLIT_EPI_BIAS_RELU: np.maximum(acc, 0), L.SPLIT_EPI_BIAS_RESID: acc + r,
                    L.SPLIT_EPI_REFINE: r - ALPHA * acc}[epi]
            d = np.abs(got[256][m].cpu().numpy() - want)
            assert not np.isnan(d).any() and d.max() <= PLACED, (epi, m, d.max())


def test_wide_tiling_qkv_and_heads_epilogues():
    """in_proj's epilogue (columns below qcols scaled by alpha) at N = 512, qcols = 256, and the two-output heads epilogue at
    N = 512 = 2 ldc (the second wide tile, both halves, writes C2)."""
    M, N, K = 384, 512, 768
    for nz in (1, 2):
        ops = _operands(M, N, K, nz, seed=40 + nz)
        q, h = {}, {}
        for tile in (128, 256):
            Cs = [_nan(M, N) for _ in range(nz)]
            assert _unit(ops, M, N, K, N, L.SPLIT_EPI_QKV, tile, C_=Cs, qcols=256, alpha=0.125) == 0, L.last_error()
            q[tile] = Cs
            Cs, C2 = [_nan(M, 256) for _ in range(nz)], [_nan(M, 256) for _ in range(nz)]
            assert _unit(ops, M, N, K, 256, L.SPLIT_EPI_HEADS, tile, C_=Cs, C2=C2) == 0, L.last_error()
            h[tile] = (Cs, C2)
        for m in range(nz):
            acc = ops[m]["acc"]
            assert _same(q[256][m], q[128][m])
            want = acc * np.where(np.arange(N) < 256, 0.125, 1.0)
            d = np.abs(q[256][m].cpu().numpy() - want)
            assert not np.isnan(d).any() and d.max() <= PLACED
            for part, cols in ((0, slice(0, 256)), (1, slice(256, 512))):
                assert _same(h[256][part][m], h[128][part][m])
                d = np.abs(h[256][part][m].cpu().numpy() - acc[:, cols])
                assert not np.isnan(d).any() and d.max() <= PLACED


@pytest.mark.parametrize("N,store_h", [(256, False), (768, True)])
def test_wide_tiling_dot_epilogue(N, store_h):
    """The folded scorer's epilogue: per 128-column tile the sum of relu(acc + bias) * v goes to C2[M, N / 128]; a wide block writes
    the partials of both its halves to the columns the narrow tiles write."""
    M, K = 384, 768
    ops = _operands(M, N, K, 1, seed=N)
    v = np.random.default_rng(8).standard_normal(N).astype(np.float32)
    dv = [torch.from_numpy(v).cuda()]
    got = {}
    for tile in (128, 256):
        Cs = [_nan(M, N)] if store_h else None
        part = [_nan(M, N // 128)]
        assert _unit(ops, M, N, K, N, L.SPLIT_EPI_BIAS_RELU_DOT, tile, C_=Cs, C2=part, R=dv) == 0, L.last_error()
        got[tile] = (Cs, part)
    assert _same(got[256][1][0], got[128][1][0])
    hid = np.maximum(ops[0]["acc"], 0)
    want = (hid * v.astype(np.float64)).reshape(M, N // 128, 128).sum(-1)
    d = np.abs(got[256][1][0].cpu().numpy() - want)
    assert not np.isnan(d).any() and d.max() <= 128 * PLACED * np.abs(v).max()
    if store_h:
        assert _same(got[256][0][0], got[128][0][0])
        d = np.abs(got[256][0][0].cpu().numpy() - hid)
        assert not np.isnan(d).any() and d.max() <= PLACED


def test_wide_tiling_against_fp64_at_the_fp32_kernels_bound():
    """So that the two tilings cannot be wrong together: the wide tiling's error against an fp64 product is held to the bound of
    test_split_gemm_is_at_least_as_accurate_as_fp32_mfma (the fp32 MFMA kernel's own error x 1.25 in the maximum, x 1.1 in rms)."""
    M, N, K = 384, 768, 768
    ops = _operands(M, N, K, 1, seed=1)
    o = ops[0]
    Cw, Cf = [_nan(M, N)], _nan(M, N)
    assert _unit(ops, M, N, K, N, L.SPLIT_EPI_BIAS, 256, C_=Cw) == 0, L.last_error()
    assert L.load_library().iefvad_gemm_bias(o["dA"].data_ptr(), o["dW"].data_ptr(), o["db"].data_ptr(), Cf.data_ptr(), M, N, K,
                                             L.COMPUTE_F32, _stream()) == 0, L.last_error()
    torch.cuda.synchronize()
    es, ef = np.abs(Cw[0].cpu().numpy() - o["acc"]), np.abs(Cf.cpu().numpy() - o["acc"])
    print(f"wide tiling vs fp64: max {es.max():.3e} rms {np.sqrt((es ** 2).mean()):.3e} | fp32 MFMA: max {ef.max():.3e} rms {np.sqrt((ef ** 2).mean()):.3e}")
    assert es.max() <= 1.25 * ef.max() + 1e-7, (es.max(), ef.max())
    assert np.sqrt((es ** 2).mean()) <= 1.1 * np.sqrt((ef ** 2).mean()) + 1e-9


def test_rejected_tilings_are_not_launched():
    M, N, K = 128, 384, 64
    ops = _operands(M, N, K, 1, seed=2)
    Cs = [_nan(M, N)]
    assert _unit(ops, M, N, K, N, L.SPLIT_EPI_BIAS, 256, C_=Cs) != 0
    assert "256" in L.last_error() and "N=384" in L.last_error().replace(" = ", "=")
    assert _unit(ops, M, N, K, N, L.SPLIT_EPI_BIAS, 64, C_=Cs) != 0
    assert "tile_n" in L.last_error()
    assert torch.isnan(Cs[0]).all()                     # nothing ran
    assert _unit(ops, M, N, K, N, L.SPLIT_EPI_BIAS, 128, C_=Cs) == 0, L.last_error()     # the narrow tiling takes N = 384
    assert not torch.isnan(Cs[0]).any()


def _model(sd, monkeypatch, tile, **kw):
    args = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=10, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, "cuda", args, compute="bf16x6", **kw)
    m.load_state_dict(sd)
    m = m.to("cuda:0").eval()
    monkeypatch.setenv("IEFVAD_SPLIT_TILE", str(tile))     # read by iefvad_create, which the first forward calls
    return m


def _run(model, img, ev):
    """The outputs, the projection launches of the forward and how many of them ran the 128 x 256 tiling."""
    lib = L.load_library()
    wide0 = lib.iefvad_gemm_split_wide_launches()
    with torch.no_grad():
        out = model(torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda(), None, None, None, timed=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, model.last_stage_times["gemm_launches"], lib.iefvad_gemm_split_wide_launches() - wide0


def test_forward_on_either_tiling_is_bit_equal(monkeypatch):
    """B = 48 chunks on two handles of one process, IEFVAD_SPLIT_TILE = 256 and 128: the eight outputs of the full forward and the
    three of the scores-only forward (the folded scorer's dot epilogue on the wide tiling) agree bit for bit, and the 256 handle
    meets the fp32 gates against the oracle.  At this size the launch rule alone would leave most projections on the narrow tiling,
    so the count of wide launches is asserted: every projection of the 256 handle, none of the 128 handle."""
    sd = synth.make_state_dict(0)
    img, ev = synth.make_inputs(7, 48)
    out = {}
    for tile in (256, 128):
        for outputs in ("full", "scores"):
            m = _model(sd, monkeypatch, tile, **({} if outputs == "full" else {"outputs": "scores"}))
            out[tile, outputs], launches, wide = _run(m, img, ev)      # the handle is created here, under this tile's setting
            assert launches == (25 if outputs == "full" else 24), launches      # 2 L + 1 + 2 K; the fold saves one
            assert wide == (launches if tile == 256 else 0), (tile, outputs, wide, launches)
    for k in iefvad_amd.OUTPUT_KEYS:
        assert np.array_equal(out[256, "full"][k], out[128, "full"][k]), k
    for k in ("logits", "w_i_mean", "w_e_mean"):
        assert np.array_equal(out[256, "scores"][k], out[128, "scores"][k]), k
    ref = orc.forward(sd, torch.from_numpy(img), torch.from_numpy(ev), orc.OracleConfig(num_layers=2, num_refinement_steps=10, nu=8))
    got = out[256, "full"]
    for k in H.BIG_KEYS:
        assert np.abs(got[k] - ref[k].numpy()).max() <= H.TOL_BIG, k
    for g in (got, out[256, "scores"]):
        assert np.abs(g["logits"] - ref["logits"].numpy()).max() <= H.TOL_LOGIT
        assert np.abs(H.sigmoid(g["logits"]) - H.sigmoid(ref["logits"].numpy())).max() <= H.TOL_SIGMOID
