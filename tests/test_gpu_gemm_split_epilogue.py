"""The per-kind epilogue of the 128 x 256 bf16x6 split kernels (csrc/gemm_split_epilogue.h: one kernel per epilogue kind, rows stored from a
wave-uniform row base plus one lane offset, both column halves' loads requested before the first store) against the small tiling
(csrc/gemm_split_small.h), which still runs the shared row-wise epilogue of csrc/gemm_bf16.h.  The two sum every output element in the same
order, so every kind must agree BIT FOR BIT, on the smallest shapes that reach what the specialised code can get wrong: a row stride that
is not N, the C / C2 boundary of the heads between the halves of one block, a q scale that ends inside a half, the in-place refine, the
dot kind with and without its stored h, non-finite values.  Outputs start as NaN inside two guard rows on either side; the guards and the
columns from N on must stay as they were.  Needs a real MI355X: run with `-m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from iefvad_amd import lib as L

pytestmark = pytest.mark.gpu

ALPHA = 0.3                 # not a power of two: a scale or a lambda applied twice, or not at all, changes the mantissa
GUARD = 2                   # untouched rows in front of and behind every output
# (M, N, K, nz): one wide block of two k-tiles | a second row panel, a second wide tile and a second problem
SHAPES = [(128, 256, 64, 1), (256, 512, 128, 2)]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _operands(M, N, K, nz):
    """Asymmetric operands and their W planes, made once per shape and never written again."""
    rng = np.random.default_rng(1000 * M + N + K + nz)
    ops = []
    for _ in range(nz):
        dA = torch.from_numpy((rng.standard_normal((M, K)) * 1.3).astype(np.float32)).cuda()
        dW = torch.from_numpy((rng.uniform(-1, 1, (N, K)) / np.sqrt(K)).astype(np.float32)).cuda()
        db = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).cuda()
        planes = torch.empty(3, N, K, dtype=torch.bfloat16, device="cuda")
        assert L.load_library().iefvad_split_bf16x3(dW.data_ptr(), planes.data_ptr(), N * K, _stream()) == 0, L.last_error()
        R = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).cuda()
        ops.append(dict(dA=dA, db=db, planes=planes, R=R))
    torch.cuda.synchronize()
    return tuple(ops)


class Out:
    """[GUARD + M + GUARD, ld] of NaN (or of `fill` rows); .ptr is row GUARD."""

    def __init__(self, M, ld, fill=None, width=None):
        self.M, self.ld = M, ld
        self.t = torch.full((M + 2 * GUARD, ld), float("nan"), device="cuda")
        if fill is not None:
            self.t[GUARD:GUARD + M, :fill.shape[1]] = fill
        self.width = width if width is not None else ld
        self.ptr = self.t[GUARD:].data_ptr()

    def bits(self):
        return self.t.view(torch.int32)

    def assert_guards(self, what):
        nan_bits = torch.full((1,), float("nan")).view(torch.int32).item()
        b = self.bits()
        assert (b[:GUARD] == nan_bits).all() and (b[GUARD + self.M:] == nan_bits).all(), f"{what}: a guard row was written"
        assert (b[:, self.width:] == nan_bits).all(), f"{what}: a column from {self.width} on was written"

    def body(self):
        return self.t[GUARD:GUARD + self.M, :self.width]


def _launch(tiling, ops, M, N, K, ldc, epi, C_=None, C2=None, R=None, bias=None, qcols=0, alpha=ALPHA):
    io = L.GemmSplitIO()
    for m, o in enumerate(ops):
        io.A[m], io.W[m] = o["dA"].data_ptr(), o["planes"].data_ptr()
        io.bias[m] = (bias[m] if bias is not None else o["db"]).data_ptr()
        io.C[m] = C_[m].ptr if C_ is not None else None
        io.C2[m] = C2[m].ptr if C2 is not None else None
        io.R[m] = (R[m].ptr if isinstance(R[m], Out) else R[m].data_ptr()) if R is not None else None
    lib = L.load_library()
    if tiling == "small":
        rc = lib.iefvad_gemm_split_small_unit(C.byref(io), M, N, K, ldc, epi, qcols, alpha, len(ops), _stream())
    else:
        wide0 = lib.iefvad_gemm_split_wide_launches()
        rc = lib.iefvad_gemm_split_unit(C.byref(io), M, N, K, ldc, epi, qcols, alpha, len(ops), 256, _stream())
        assert rc != 0 or lib.iefvad_gemm_split_wide_launches() - wide0 == 1      # the 128 x 256 kernel is what ran
    torch.cuda.synchronize()
    assert rc == 0, L.last_error()


def _compare(outs, what, finite=True):
    """outs: {tiling: [Out, ...]}: every buffer bit-equal between the tilings, guards untouched, the body written."""
    for w, s in zip(outs["wide"], outs["small"]):
        w.assert_guards(what)
        s.assert_guards(what)
        if finite:
            assert not torch.isnan(w.body()).any(), f"{what}: an element was not written"
        assert torch.equal(w.bits(), s.bits()), what


@pytest.mark.parametrize("M,N,K,nz", SHAPES)
@pytest.mark.parametrize("epi", ["BIAS", "BIAS_RELU", "BIAS_RESID", "REFINE", "REFINE_IN_PLACE"])
def test_row_stride_and_residual_kinds(M, N, K, nz, epi):
    """ldc = N + 64: a row stride formed from N, or from a constant, puts rows in the wrong place; columns from N on stay NaN.  The refine
    kind out of place (R apart from C) and in place (C == R, as the refinement runs it)."""
    ops = _operands(M, N, K, nz)
    ldc = N + 64
    code = getattr(L, "SPLIT_EPI_" + epi.replace("_IN_PLACE", ""))
    outs = {}
    for tiling in ("wide", "small"):
        if epi == "REFINE_IN_PLACE":
            Cs = [Out(M, ldc, fill=o["R"], width=N) for o in ops]
            Rs = Cs
        else:
            Cs = [Out(M, ldc, width=N) for _ in ops]
            Rs = [Out(M, ldc, fill=o["R"], width=N) for o in ops] if epi in ("BIAS_RESID", "REFINE") else None
        _launch(tiling, ops, M, N, K, ldc, code, C_=Cs, R=Rs)
        outs[tiling] = Cs
    _compare(outs, epi)


@pytest.mark.parametrize("M,N,K,nz", SHAPES)
def test_heads_boundary_between_the_halves(M, N, K, nz):
    """N = 2 ldc: at N = 256 the C / C2 boundary lies between the two column halves of ONE block, at N = 512 between two blocks."""
    ops = _operands(M, N, K, nz)
    ldc = N // 2
    outs = {}
    for tiling in ("wide", "small"):
        Cs, C2 = [Out(M, ldc) for _ in ops], [Out(M, ldc) for _ in ops]
        _launch(tiling, ops, M, N, K, ldc, L.SPLIT_EPI_HEADS, C_=Cs, C2=C2)
        outs[tiling] = Cs + C2
    _compare(outs, "heads")


@pytest.mark.parametrize("M,N,K,nz", SHAPES)
@pytest.mark.parametrize("qcols", [0, 8, 136, -1])
def test_qkv_scale_ends_inside_a_half(M, N, K, nz, qcols):
    """qcols = 8 and 136 end inside the first and the second half of block 0, off every tile edge: a scale chosen per tile or per half
    differs.  0: nothing scaled; N (-1): everything."""
    ops = _operands(M, N, K, nz)
    qcols = N if qcols < 0 else qcols
    outs = {}
    for tiling in ("wide", "small"):
        Cs = [Out(M, N) for _ in ops]
        _launch(tiling, ops, M, N, K, N, L.SPLIT_EPI_QKV, C_=Cs, qcols=qcols)
        outs[tiling] = Cs
    _compare(outs, f"qkv qcols={qcols}")


@pytest.mark.parametrize("M,N,K", [s[:3] for s in SHAPES])
@pytest.mark.parametrize("store_h", [False, True])
def test_dot_kind_partials_and_stored_h(M, N, K, store_h):
    """One problem (the kind takes no second): the partial sums of both halves land in the columns of C2[M, N / 128] that the narrow tiles
    write, h (row stride N + 64) is stored only where C is given."""
    ops = _operands(M, N, K, 1)
    v = [torch.from_numpy(np.random.default_rng(8).standard_normal(N).astype(np.float32)).cuda()]
    outs = {}
    for tiling in ("wide", "small"):
        Cs = [Out(M, N + 64, width=N)] if store_h else None
        part = [Out(M, N // 128)]
        _launch(tiling, ops, M, N, K, N + 64, L.SPLIT_EPI_BIAS_RELU_DOT, C_=Cs, C2=part, R=v)
        outs[tiling] = part + (Cs or [])
    _compare(outs, f"dot store_h={store_h}")


@pytest.mark.parametrize("epi", ["BIAS_RELU", "REFINE"])
def test_non_finite_bias_keeps_its_bits(epi):
    """+inf, -inf and NaN in three bias columns (one in each half, one on a half's last column): the ReLU keeps NaN (v < 0 ? 0 : v, not a
    maximum), -inf becomes 0, and the refine kind's R - alpha v gives the small tiling's bit patterns."""
    M, N, K, nz = SHAPES[0]
    ops = _operands(M, N, K, nz)
    b = ops[0]["db"].clone()
    b[5], b[127], b[131] = float("inf"), float("-inf"), float("nan")
    code = getattr(L, "SPLIT_EPI_" + epi)
    outs = {}
    for tiling in ("wide", "small"):
        Cs = [Out(M, N)]
        Rs = [Out(M, N, fill=ops[0]["R"])] if epi == "REFINE" else None
        _launch(tiling, ops, M, N, K, N, code, C_=Cs, R=Rs, bias=[b])
        outs[tiling] = Cs
    _compare(outs, "non-finite " + epi, finite=False)
    got = outs["wide"][0].body()
    assert torch.isnan(got[:, 131]).all()                                # NaN is not flushed by the ReLU
    if epi == "BIAS_RELU":
        assert torch.isinf(got[:, 5]).all() and (got[:, 127] == 0).all()
    assert not torch.isnan(got[:, [c for c in range(N) if c != 131]]).any()
