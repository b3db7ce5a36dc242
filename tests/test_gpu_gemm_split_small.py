"""The small tiling of the bf16x6 split projection (csrc/gemm_split_small.h, iefvad_gemm_split_small_kernel: 32 x 128 workgroups of four
32 x 32 waves) against the 128 x 128 tiling (iefvad_gemm_split_n128_kernel).  Both sum every output element over its k-tiles in ascending
order and over the six products of a k-tile in one order, and both run the same row-wise epilogue code, so they must agree BIT FOR BIT on
every epilogue -- which is what lets the batch-invariant mode (iefvad_set_batch_invariant) hand small launches to the small tiling.
The unit entries name the tiling.  Needs a real MI355X: run with `-m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

from iefvad_amd import lib as L

pytestmark = pytest.mark.gpu

ALPHA = 0.5
# |fp32-accumulated result - fp64 result| stays far below this at K <= 768 with these operands (measured ~1e-6; the worst case
# K 2^-24 sum |a w| is ~6e-4); an element that was not written, or went to the wrong place, is off by O(1)
PLACED = 1e-3


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _operands(M, N, K, nz, seed):
    """Asymmetric operands: a transposed accumulator map, or a wave's columns in another wave's place, would show."""
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


def _unit(ops, M, N, K, ldc, epi, tiling, C_=None, C2=None, R=None, qcols=0, alpha=ALPHA):
    """tiling: "small" (iefvad_gemm_split_small_unit) or "n128" (iefvad_gemm_split_unit, tile_n = 128)."""
    io = L.GemmSplitIO()
    for m, o in enumerate(ops):
        io.A[m], io.W[m], io.bias[m] = o["dA"].data_ptr(), o["planes"].data_ptr(), o["db"].data_ptr()
        io.C[m] = C_[m].data_ptr() if C_ is not None and C_[m] is not None else None
        io.C2[m] = C2[m].data_ptr() if C2 is not None else None
        io.R[m] = R[m].data_ptr() if R is not None else None
    lib = L.load_library()
    if tiling == "small":
        rc = lib.iefvad_gemm_split_small_unit(C.byref(io), M, N, K, ldc, epi, qcols, alpha, len(ops), _stream())
    else:
        rc = lib.iefvad_gemm_split_unit(C.byref(io), M, N, K, ldc, epi, qcols, alpha, len(ops), 128, _stream())
    torch.cuda.synchronize()
    return rc


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))       # bits; a NaN left in either fails the closeness checks


TILINGS = ("n128", "small")


@pytest.mark.parametrize("nz", [1, 2])
@pytest.mark.parametrize("N", [128, 768])
@pytest.mark.parametrize("K", [64, 768])
@pytest.mark.parametrize("M", [128, 384])
def test_small_tiling_equals_n128_tiling(M, K, N, nz):
    """bias, bias + ReLU, bias + residual and the in-place refine epilogue, one or two problems per launch.  K = 64 is the minimum of
    two k-tiles (the prologue's two A tiles and no steady state); N = 128 is one column tile, M = 384 x N = 768 a grid of 72 workgroups
    (x nz), beyond the 8-XCD remap's size."""
    ops = _operands(M, N, K, nz, seed=M + K + N + nz)
    rng = np.random.default_rng(3)
    R0 = [torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).cuda() for _ in range(nz)]
    lib = L.load_library()
    n0 = lib.iefvad_gemm_split_small_launches()
    for epi in (L.SPLIT_EPI_BIAS, L.SPLIT_EPI_BIAS_RELU, L.SPLIT_EPI_BIAS_RESID, L.SPLIT_EPI_REFINE):
        got = {}
        for tiling in TILINGS:
            if epi == L.SPLIT_EPI_REFINE:              # in place: C == R
                Cs = [r.clone() for r in R0]
                Rs = Cs
            else:
                Cs = [_nan(M, N) for _ in range(nz)]
                Rs = R0 if epi == L.SPLIT_EPI_BIAS_RESID else None
            assert _unit(ops, M, N, K, N, epi, tiling, C_=Cs, R=Rs) == 0, L.last_error()
            got[tiling] = Cs
        for m in range(nz):
            assert _same(got["small"][m], got["n128"][m]), (epi, m)
            acc, r = ops[m]["acc"], R0[m].cpu().numpy().astype(np.float64)
            want = {L.SPLIT_EPI_BIAS: acc, L.SPLIT_EPI_BIAS_RELU: np.maximum(acc, 0), L.SPLIT_EPI_BIAS_RESID: acc + r,
                    L.SPLIT_EPI_REFINE: r - ALPHA * acc}[epi]
            d = np.abs(got["small"][m].cpu().numpy() - want)
            assert not np.isnan(d).any() and d.max() <= PLACED, (epi, m, d.max())
    assert lib.iefvad_gemm_split_small_launches() - n0 == 4      # one per epilogue: the counter sees this kernel and no other


def test_small_tiling_qkv_and_heads_epilogues():
    """in_proj's epilogue (columns below qcols scaled by alpha) at N = 512, qcols = 256, and the two-output heads epilogue at
    N = 512 = 2 ldc (column tiles 2 and 3 write C2)."""
    M, N, K = 384, 512, 768
    for nz in (1, 2):
        ops = _operands(M, N, K, nz, seed=40 + nz)
        q, h = {}, {}
        for tiling in TILINGS:
            Cs = [_nan(M, N) for _ in range(nz)]
            assert _unit(ops, M, N, K, N, L.SPLIT_EPI_QKV, tiling, C_=Cs, qcols=256, alpha=0.125) == 0, L.last_error()
            q[tiling] = Cs
            Cs, C2 = [_nan(M, 256) for _ in range(nz)], [_nan(M, 256) for _ in range(nz)]
            assert _unit(ops, M, N, K, 256, L.SPLIT_EPI_HEADS, tiling, C_=Cs, C2=C2) == 0, L.last_error()
            h[tiling] = (Cs, C2)
        for m in range(nz):
            acc = ops[m]["acc"]
            assert _same(q["small"][m], q["n128"][m])
            want = acc * np.where(np.arange(N) < 256, 0.125, 1.0)
            d = np.abs(q["small"][m].cpu().numpy() - want)
            assert not np.isnan(d).any() and d.max() <= PLACED
            for part, cols in ((0, slice(0, 256)), (1, slice(256, 512))):
                assert _same(h["small"][part][m], h["n128"][part][m])
                d = np.abs(h["small"][part][m].cpu().numpy() - acc[:, cols])
                assert not np.isnan(d).any() and d.max() <= PLACED


@pytest.mark.parametrize("store_h", [False, True])
def test_small_tiling_dot_epilogue(store_h):
    """The folded scorer's epilogue at N = 768: per 128-column tile the sum of relu(acc + bias) * v goes to C2[M, 6] -- the in-lane
    4-column sum, then the 32-lane DPP order, one partial per tile where iefvad_scorer_fold_kernel reads it.  The six partials per row
    are bit-equal, and so is h when it is stored."""
    M, N, K = 384, 768, 768
    ops = _operands(M, N, K, 1, seed=N + store_h)
    v = np.random.default_rng(8).standard_normal(N).astype(np.float32)
    dv = [torch.from_numpy(v).cuda()]
    got = {}
    for tiling in TILINGS:
        Cs = [_nan(M, N)] if store_h else None
        part = [_nan(M, N // 128)]
        assert _unit(ops, M, N, K, N, L.SPLIT_EPI_BIAS_RELU_DOT, tiling, C_=Cs, C2=part, R=dv) == 0, L.last_error()
        got[tiling] = (Cs, part)
    assert _same(got["small"][1][0], got["n128"][1][0])
    hid = np.maximum(ops[0]["acc"], 0)
    want = (hid * v.astype(np.float64)).reshape(M, N // 128, 128).sum(-1)
    d = np.abs(got["small"][1][0].cpu().numpy() - want)
    assert not np.isnan(d).any() and d.max() <= 128 * PLACED * np.abs(v).max()
    if store_h:
        assert _same(got["small"][0][0], got["n128"][0][0])
        d = np.abs(got["small"][0][0].cpu().numpy() - hid)
        assert not np.isnan(d).any() and d.max() <= PLACED


@pytest.mark.parametrize("M", [32, 96])
def test_row_counts_below_the_n128_tile(M):
    """M = 32 (one workgroup row) and M = 96 are shapes only the small tiling takes: its rows equal the first M rows of an M = 128 run
    of the n128 tiling on the same A padded with zero rows, and the sentinel rows behind the M-row output stay untouched."""
    N, K, MP, GUARD = 768, 768, 128, 32
    ops = _operands(MP, N, K, 1, seed=M)
    o = ops[0]
    o["dA"][M:].zero_()
    ref = [_nan(MP, N)]
    assert _unit(ops, MP, N, K, N, L.SPLIT_EPI_BIAS, "n128", C_=ref) == 0, L.last_error()
    out = torch.full((M + GUARD, N), -7.0, device="cuda")
    assert _unit(ops, M, N, K, N, L.SPLIT_EPI_BIAS, "small", C_=[out]) == 0, L.last_error()
    assert _same(out[:M], ref[0][:M])
    assert bool((out[M:] == -7.0).all())
    d = np.abs(out[:M].cpu().numpy() - o["acc"][:M])
    assert not np.isnan(d).any() and d.max() <= PLACED


def test_refused_shapes_are_named_and_not_launched():
    ops = _operands(128, 256, 64, 1, seed=2)
    Cs = [_nan(128, 256)]
    lib = L.load_library()
    n0 = lib.iefvad_gemm_split_small_launches()
    assert _unit(ops, 48, 256, 64, 256, L.SPLIT_EPI_BIAS, "small", C_=Cs) != 0               # M % 32
    assert "iefvad_gemm_split_small_unit" in L.last_error() and "M=48" in L.last_error()
    assert _unit(ops, 128, 192, 64, 192, L.SPLIT_EPI_BIAS, "small", C_=Cs) != 0              # N % 128
    assert "N=192" in L.last_error()
    assert _unit(ops, 128, 256, 32, 256, L.SPLIT_EPI_BIAS, "small", C_=Cs) != 0              # K = 32: one k-tile
    assert "K=32" in L.last_error()
    assert torch.isnan(Cs[0]).all() and lib.iefvad_gemm_split_small_launches() == n0         # nothing ran
    assert _unit(ops, 128, 256, 64, 256, L.SPLIT_EPI_BIAS, "small", C_=Cs) == 0, L.last_error()
    assert not torch.isnan(Cs[0]).any()
