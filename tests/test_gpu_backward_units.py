"""The kernels of the training step's backward pass, ONE at a time (csrc/backward.h, csrc/gemm_split_tn.h) against fp64.

`iefvad_backward_unit` (include/iefvad.h) launches a single kernel through the launch helper the training step itself uses
(csrc/train.h), on buffers this file owns; every reference below is a plain fp64 numpy / torch restatement of the operation the
kernel's comments in backward.h describe.  Whole tensors are compared, inputs come from seeded generators with varied magnitude and
sign, and every output buffer is surrounded by sentinel values that must survive.

Gates
  bgemm       |got - want| <= K 2^-24 (|alpha| |A| |B|)_ij + 2^-23 |want| + the epilogue's own half-ulp terms: the forward bound of a
              length-K fp32 sum in any order (|A| |B| in fp64); for act != 0 the bound is applied before the activation, pushed through
              its Lipschitz constant (1.1 QuickGELU, 1 ELU) and the activation's own evaluation error is added.
  split TN    the gate tests/test_gpu_bf16x6.py::test_split_gemm_is_at_least_as_accurate_as_fp32_mfma holds the NT split kernel to
              against fp64: worst error <= 1.25 x the fp32 MFMA kernel's on the same product + 1e-7, rms <= 1.1 x + 1e-9 -- per slice
              partial and for the reduced dW.  The ride-along column sums are plain fp32 sums: n 2^-24 sum|x|.
  reductions  nparts 2^-24 sum_p |part|; multi-job == single-job bit for bit.
  row kernels no constant fixed in advance: the same formula evaluated in fp32 by torch / numpy on the CPU gives a reference-side floor
              (its worst error against fp64 on the test's own inputs), the kernel is gated at 3 x that floor, the factor ARITHMETIC.md
              uses for its reference-side floors (its section "Backward kernels one at a time" records the floors and the measured
              ratios; each test prints both).  The margin covers another legitimate summation order and expf's last-place differences.
The issue's shape list asks for grids of 7, 9 and 18 workgroups, which its batch counts {1, 3, 6} cannot produce on M in {128, 256},
N in {96, 128, 192, 256}: batch counts 7 and 9 are added for them.  Needs a real MI355X: run with `-m gpu`."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from iefvad_amd import lib as L
from tests.helpers import FLOOR_FACTOR, FloorGate, seq_sum32                # noqa: F401  (the row kernels' gate, ARITHMETIC.md)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT = np.float32(-7777.25)                      # guard value: no test input or result equals it
ROWS = (1, 4, 31, 32, 33, 130)                   # every `row >= rows` branch: below / at / past a block of 4 and of 32 rows


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _ptr(t, offset=0):
    if t is None:
        return None
    return t.data_ptr() + 4 * offset


def unit(kind, expect_ok=True, **fields):
    a = L.BWD_ARGS[kind]()
    for k, v in fields.items():
        setattr(a, k, v)
    rc = L.load_library().iefvad_backward_unit(kind, C.byref(a), C.sizeof(a), _stream())
    if expect_ok:
        assert rc == 0, L.last_error()
        torch.cuda.synchronize()
    return rc


def varied(rng, shape, spread=2.0):
    """Values of both signs whose magnitudes span e^(+-spread): a transposed, shifted or dropped element changes every sum."""
    return (rng.standard_normal(shape) * np.exp(rng.uniform(-spread, spread, shape))).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# bgemm
# ------------------------------------------------------------------------------------------------------------------------
class Bgemm:
    """One batched product on buffers with leading dimensions wider than the logical widths, two-level batch strides that differ
    between the levels and between the operands, NaN in every gap of A and B and a sentinel in every gap of C."""

    def __init__(self, rng, akc, bkc, M, N, K, nz, nz2, a_drop=0.0):
        self.akc, self.bkc, self.M, self.N, self.K, self.nz, self.nz2, self.a_drop = akc, bkc, M, N, K, nz, nz2, a_drop
        nz1 = (nz + nz2 - 1) // nz2
        self.lda = (K if akc else M) + 8
        self.ldb = (K if bkc else N) + 12
        self.ldc = N + 3
        self.a2 = (M if akc else K) * self.lda + 8
        self.a1 = nz2 * self.a2 + 12
        self.b2 = (N if bkc else K) * self.ldb + 4
        self.b1 = nz2 * self.b2 + 20
        self.c2 = M * self.ldc + 5
        self.c1 = nz2 * self.c2 + 7
        self.c0 = 16
        self.A = varied(rng, (nz, M, K))
        self.B = varied(rng, (nz, N, K))
        if a_drop:
            # the sign-carrying probabilities of the train forward: magnitudes are P, a set sign bit means dropped
            self.A = np.abs(self.A)
            drop = rng.random((nz, M, K)) < 0.3
            self.A[drop] *= -1
            self.A[:, 1, 2] = -0.0                                   # dropped, value zero
            self.A[:, 3, 5] = 0.0                                    # kept, value zero
            self.A[:, 5, 7] = np.float32(-3.0e30)                    # dropped, large: one leak and the row is gone
            self.A[:, 126, K - 1] = np.float32(-2.5e30)
        i, j, k = np.arange(M), np.arange(N), np.arange(K)
        ia = i[:, None] * self.lda + k[None, :] if akc else k[None, :] * self.lda + i[:, None]
        ib = j[:, None] * self.ldb + k[None, :] if bkc else k[None, :] * self.ldb + j[:, None]
        ic = i[:, None] * self.ldc + j[None, :]
        bufA = np.full(nz1 * self.a1 + 64, np.nan, np.float32)
        bufB = np.full(nz1 * self.b1 + 64, np.nan, np.float32)
        self.cidx = np.empty((nz, M, N), np.int64)
        for z in range(nz):
            z1, z2 = divmod(z, nz2)
            bufA[z1 * self.a1 + z2 * self.a2 + ia] = self.A[z]
            bufB[z1 * self.b1 + z2 * self.b2 + ib] = self.B[z]
            self.cidx[z] = self.c0 + z1 * self.c1 + z2 * self.c2 + ic
        self.csize = self.c0 + nz1 * self.c1 + 64
        assert np.unique(self.cidx).size == self.cidx.size and self.cidx.max() < self.csize
        self.dA, self.dB = _dev(bufA), _dev(bufB)
        if a_drop:
            s = np.float32(a_drop)
            self.Aeff = np.where(np.signbit(self.A), np.float32(0), self.A * s).astype(np.float32)       # rounded once, as the kernel forms it
        else:
            self.Aeff = self.A
        A64, B64 = self.Aeff.astype(np.float64), self.B.astype(np.float64)
        self.acc = np.einsum("zik,zjk->zij", A64, B64)
        self.absacc = np.einsum("zik,zjk->zij", np.abs(A64), np.abs(B64))

    def scatter(self, vals, fill):
        buf = np.full(self.csize, fill, np.float32)
        buf[self.cidx] = vals
        return buf

    def run(self, alpha=1.0, R=None, G=None, bias=None, act=0, alias=False):
        """R, G: [nz, M, N] in C's layout; bias [N].  alias: R IS the C buffer (accumulation in place)."""
        dC = _dev(self.scatter(R, SENT) if alias else np.full(self.csize, SENT, np.float32))
        dR = dC if alias else (_dev(self.scatter(R, np.nan)) if R is not None else None)
        dG = _dev(self.scatter(G, np.nan)) if G is not None else None
        dbias = _dev(bias) if bias is not None else None
        unit(L.BWD_BGEMM, A=_ptr(self.dA), B=_ptr(self.dB), C=_ptr(dC, self.c0), R=_ptr(dR, self.c0), G=_ptr(dG, self.c0), bias=_ptr(dbias),
             a1=self.a1, a2=self.a2, b1=self.b1, b2=self.b2, c1=self.c1, c2=self.c2, M=self.M, N=self.N, K=self.K, lda=self.lda, ldb=self.ldb,
             ldc=self.ldc, nz=self.nz, nz2=self.nz2, akc=int(self.akc), bkc=int(self.bkc), act=act, alpha=alpha, a_drop=self.a_drop)
        out = dC.cpu().numpy()
        guard = np.ones(self.csize, bool)
        guard[self.cidx.ravel()] = False
        assert (out[guard] == SENT).all(), "a write outside the logical C blocks"
        got = out[self.cidx].astype(np.float64)
        # v = alpha * acc (+ bias) (+ R), each step rounded: half an ulp of every intermediate, on top of the sum's own bound
        al = float(np.float32(alpha))
        v = al * self.acc
        bound = self.K * U * abs(al) * self.absacc
        half = np.abs(v) if al != 1.0 else 0.0
        if bias is not None:
            v = v + bias.astype(np.float64)[None, None, :]
            half = half + np.abs(v)
        if R is not None:
            v = v + R.astype(np.float64)
            half = half + np.abs(v)
        bound = bound + U * half
        if G is not None:
            keep = G > 0
            v = np.where(keep, v, 0.0)
            bound = np.where(keep, bound, 0.0)
        if act == 1:          # QuickGELU v sigmoid(1.702 v) with the kernel's fp32 constant: Lipschitz <= 1.1; its evaluation: the rounded
            c = float(np.float32(1.702))       # argument of expf (|c v| 2^-24 relative in the sigmoid), expf, the sum, the quotient, the product
            want = v / (1.0 + np.exp(-c * v))
            bound = 1.1 * bound + np.abs(want) * U * (6 + c * np.abs(v))
        elif act == 2:        # ELU: Lipschitz 1; expm1f to two ulps
            want = np.where(v > 0, v, np.expm1(v))
            bound = bound + 4 * U * np.abs(want)
        else:
            want = v
        bound = bound + 2 * U * np.abs(want)
        err = np.abs(got - want)
        bad = ~(err <= bound)
        assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist(), float((err / np.maximum(bound, 1e-300)).max()))
        return got


# (M, N, K, nz, nz2): grid = (M / 128) (N / BN) nz workgroups
BG_SHAPES = [
    (128, 128, 16, 1, 1),     # 1: one k-tile, the prefetch branch never taken
    (128, 96, 16, 1, 1),      # 1 (BN = 96)
    (128, 192, 32, 1, 1),     # 2: two BN = 96 column tiles
    (256, 128, 48, 1, 1),     # 2
    (128, 128, 32, 3, 1),     # 3
    (128, 96, 48, 3, 3),      # 3
    (128, 128, 16, 7, 1),     # 7
    (128, 96, 32, 7, 3),      # 7: the last z1 group is ragged
    (128, 128, 48, 9, 3),     # 9
    (128, 96, 16, 9, 3),      # 9
    (256, 192, 48, 3, 3),     # 12
    (128, 256, 32, 6, 3),     # 12
    (128, 192, 48, 9, 3),     # 18
    (256, 128, 32, 9, 3),     # 18
    (256, 256, 16, 1, 1),     # 4
    (256, 256, 48, 6, 3),     # 24: a multiple of the XCD count
]
LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]


@pytest.mark.parametrize("akc,bkc", LAYOUTS)
def test_bgemm_plain_product_at_every_tile_and_grid_boundary(akc, bkc):
    """All eight instantiations ({A_KC, B_KC} x BN in {128, 96}) on the bare product: one to three k-tiles, grids of 1, 2, 3, 4, 7, 9,
    12, 18 and 24 workgroups (xcd_remap with every kind of remainder), both batch levels with distinct strides per operand, sub-blocks
    of wider tensors.  A wrong row, column, k-tile or batch slab of one 32 x 32 accumulator block fails the per-element bound."""
    rng = np.random.default_rng(100 + 2 * akc + bkc)
    grids = set()
    for (M, N, K, nz, nz2) in BG_SHAPES:
        Bgemm(rng, akc, bkc, M, N, K, nz, nz2).run()
        grids.add((M // 128) * (N // (128 if N % 128 == 0 else 96)) * nz)
    assert {1, 2, 3, 7, 9, 12, 18} <= grids


@pytest.mark.parametrize("akc,bkc", LAYOUTS)
def test_bgemm_epilogue_fields_alone_and_as_the_library_combines_them(akc, bkc):
    """alpha, R, G (with exact zeros and negatives in the gate), bias, QuickGELU and ELU (arguments on both sides of 0) each alone, then
    the library's combinations: alpha with G (launch_dx behind a ReLU), alpha with R, bias + R (out_proj of a residual block),
    bias + QuickGELU (c_fc), bias + R + QuickGELU (a graph convolution), and R aliasing C (the Conv1d taps accumulate in place)."""
    rng = np.random.default_rng(200 + 2 * akc + bkc)
    for (M, N, K, nz, nz2) in [(256, 256, 48, 6, 3), (128, 192, 48, 3, 3)]:
        g = Bgemm(rng, akc, bkc, M, N, K, nz, nz2)
        scale = float(np.abs(g.acc).mean())
        R = (varied(rng, (nz, M, N), 1.0) * scale).astype(np.float32)
        G = varied(rng, (nz, M, N), 1.0)
        G[rng.random(G.shape) < 0.2] = 0.0
        G[:, 0, 0], G[:, 0, 1], G[:, 1, 0] = 0.0, -0.0, -1.0
        bias = (varied(rng, N, 1.0) * scale).astype(np.float32)
        plain = g.run()
        assert (plain > 0).any() and (plain < 0).any()                # the activations see both sides of 0
        small = float(1.0 / scale)                                    # brings the activations' arguments to O(1): both branches, no saturation
        for kw in (dict(alpha=-0.625), dict(R=R), dict(G=G), dict(bias=bias), dict(act=1, alpha=small), dict(act=2, alpha=small),
                   dict(alpha=-0.5, G=G), dict(alpha=0.3, R=R), dict(alpha=-1.7, G=G), dict(bias=bias, R=R),
                   dict(bias=(bias * small).astype(np.float32), act=1, alpha=small),
                   dict(bias=(bias * small).astype(np.float32), R=(R * small).astype(np.float32), act=1, alpha=small),
                   dict(R=R, alias=True), dict(R=R, alias=True, alpha=0.3)):
            got = g.run(**kw)
            if "G" in kw:
                assert (got[G <= 0] == 0).all()


@pytest.mark.parametrize("akc", [True, False])
def test_bgemm_forms_dropout_from_a_sign_carrying_a_operand(akc):
    """a_drop: A(i, k) = sign ? 0 : stored * a_drop in both A layouts, one and several k-tiles (the conversion sits in the prologue
    AND behind the prefetch), with -0.0 (dropped, value zero), +0.0 and dropped elements of 3e30 in the tensor."""
    rng = np.random.default_rng(300 + akc)
    a_drop = float(np.float32(1.0 / (1.0 - 0.1)))
    for bkc in (True, False):
        for (M, N, K, nz, nz2) in [(128, 96, 16, 1, 1), (128, 96, 48, 3, 3), (256, 128, 32, 1, 1), (128, 192, 32, 6, 3)]:
            g = Bgemm(rng, akc, bkc, M, N, K, nz, nz2, a_drop=a_drop)
            got = g.run()
            assert np.abs(got).max() < 1e6


def test_bgemm_refusals_surface_as_return_codes():
    t = torch.zeros(1 << 16, device="cuda")
    base = dict(A=_ptr(t), B=_ptr(t), C=_ptr(t), M=128, N=128, K=16, lda=16, ldb=16, ldc=128, nz=1, nz2=1, akc=1, bkc=1, alpha=1.0)
    for bad, frag in [(dict(M=64), "not a multiple"), (dict(N=64), "not a multiple"), (dict(K=8), "not a multiple"), (dict(nz=0), "not a multiple"),
                      (dict(nz2=0), "not a multiple"), (dict(lda=18), "multiples of 4"), (dict(ldb=22), "multiples of 4"), (dict(A=None), "needs A"),
                      (dict(A=_ptr(t, 1)), "aligned"), (dict(a2=2), "aligned"), (dict(act=3), "act")]:
        assert unit(L.BWD_BGEMM, expect_ok=False, **dict(base, **bad)) != 0
        assert frag in L.last_error(), (bad, L.last_error())
    lib = L.load_library()
    a = L.BwdBgemm()
    assert lib.iefvad_backward_unit(L.BWD_BGEMM, C.byref(a), 8, _stream()) != 0 and "argument block" in L.last_error()
    assert lib.iefvad_backward_unit(99, C.byref(a), C.sizeof(a), _stream()) != 0 and "unknown kind" in L.last_error()
    assert lib.iefvad_backward_unit(L.BWD_BGEMM, None, 0, _stream()) != 0 and "null" in L.last_error()


# ------------------------------------------------------------------------------------------------------------------------
# split TN (weight gradients of the bf16x6 arithmetic)
# ------------------------------------------------------------------------------------------------------------------------
def _f32_product(dY, X, r0, r1, out):
    """out = dY[r0:r1]^T X[r0:r1] on the fp32 MFMA kernel (both operands i-contiguous): the comparator of the split kernels' gate, and
    what launch_dw runs for the same slice in the f32 arithmetic."""
    n_out = dY.shape[1]
    unit(L.BWD_BGEMM, A=_ptr(dY, r0 * n_out), B=_ptr(X, r0 * 768), C=_ptr(out), M=n_out, N=768, K=r1 - r0, lda=n_out, ldb=768, ldc=768, nz=1, nz2=1,
         akc=0, bkc=0, alpha=1.0)
    return out.cpu().numpy().astype(np.float64)


def _split_gate(got, f32, want, what):
    es, ef = np.abs(got - want), np.abs(f32 - want)
    print(f"{what}: split worst {es.max():.3e} rms {np.sqrt((es ** 2).mean()):.3e}; fp32 MFMA worst {ef.max():.3e} rms {np.sqrt((ef ** 2).mean()):.3e}")
    assert es.max() <= 1.25 * ef.max() + 1e-7, (what, es.max(), ef.max())
    assert np.sqrt((es ** 2).mean()) <= 1.1 * np.sqrt((ef ** 2).mean()) + 1e-9, what


@pytest.mark.parametrize("n_out", [128, 768])
@pytest.mark.parametrize("rows,slice_counts", [(128, (1,)), (144, (1,)), (384, (1, 2, 3)), (1168, (1, 2, 3, 5, 9))])
def test_split_tn_partials_slice_boundaries_bias_sums_and_reduction(n_out, rows, slice_counts):
    """nk_total = rows / 16 in {8, 9, 24, 73}; 73 tiles cut in 2, 3, 5 or 9 slices are ragged.  Each slice's partial product against
    the fp64 product over exactly that slice's rows (the sum alone would not see a tile on the wrong side of a boundary), the reduced dW,
    the bias sums that ride along per slice and reduced, and two launches give the same bits."""
    rng = np.random.default_rng(rows + n_out)
    dY = (rng.standard_normal((rows, n_out)) * np.exp(rng.uniform(-1, 1, (rows, 1)))).astype(np.float32)       # row scales differ: a row in
    X = (rng.standard_normal((rows, 768)) * np.exp(rng.uniform(-1, 1, (rows, 1)))).astype(np.float32)          # the wrong slice shows
    d_dY, d_X = _dev(dY), _dev(X)
    dY64, X64 = dY.astype(np.float64), X.astype(np.float64)
    alpha = -0.75
    nk = rows // 16
    want_dw = alpha * (dY64.T @ X64)
    for slices in slice_counts:
        outs = []
        for rep in range(2):
            part = torch.full((slices * n_out * 768 + 64,), float(SENT), device="cuda")
            dW = torch.full((n_out * 768 + 64,), float(SENT), device="cuda")
            cpart = torch.full((slices * n_out + 64,), float(SENT), device="cuda")
            db = torch.full((n_out + 64,), float(SENT), device="cuda")
            unit(L.BWD_SPLIT_TN, dY=_ptr(d_dY), X=_ptr(d_X), part=_ptr(part), dW=_ptr(dW), colsum_part=_ptr(cpart), db=_ptr(db), rows=rows, n_out=n_out,
                 slices=slices, alpha=alpha)
            outs.append([t.cpu().numpy() for t in (part, dW, cpart, db)])
        for a, b in zip(*outs):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
        part, dW, cpart, db = outs[0]
        for t, n in ((part, slices * n_out * 768), (dW, n_out * 768), (cpart, slices * n_out), (db, n_out)):
            assert (t[n:] == SENT).all()
        part = part[:slices * n_out * 768].reshape(slices, n_out, 768).astype(np.float64)
        cpart = cpart[:slices * n_out].reshape(slices, n_out).astype(np.float64)
        f32_part = torch.empty(slices, n_out, 768, device="cuda")
        for z in range(slices):
            r0, r1 = 16 * (z * nk // slices), 16 * ((z + 1) * nk // slices)
            _split_gate(part[z], _f32_product(d_dY, d_X, r0, r1, f32_part[z]), dY64[r0:r1].T @ X64[r0:r1], f"n_out {n_out} rows {rows} slice {z} of {slices}")
            # plain fp32 column sums of r1 - r0 rows, any order
            assert (np.abs(cpart[z] - dY64[r0:r1].sum(0)) <= (r1 - r0) * U * np.abs(dY64[r0:r1]).sum(0)).all(), (slices, z)
        # the comparator of dW: the f32 arithmetic's dW of the same slices -- its partial products through the same fixed-order reduction
        f32_dw = _reduce_single(dict(buf=f32_part, off=0, stride=n_out * 768, nparts=slices, n=n_out * 768), alpha).reshape(n_out, 768).astype(np.float64)
        _split_gate(dW[:n_out * 768].reshape(n_out, 768).astype(np.float64), f32_dw, want_dw, f"n_out {n_out} rows {rows} dW of {slices} slices")
        want_db = alpha * dY64.sum(0)
        assert (np.abs(db[:n_out] - want_db) <= (rows + slices) * U * np.abs(dY64).sum(0)).all(), slices
    # what launch_dw cannot produce is refused
    t = torch.zeros(16, device="cuda")
    for bad, frag in [(dict(rows=rows + 8), "multiple of 16"), (dict(n_out=n_out + 64), "of 128"), (dict(slices=0), "outside 1.."),
                      (dict(slices=nk // 8 + 1), "outside 1..")]:
        kw = dict(dY=_ptr(t), X=_ptr(t), part=_ptr(t), dW=_ptr(t), rows=rows, n_out=n_out, slices=1, alpha=1.0)
        assert unit(L.BWD_SPLIT_TN, expect_ok=False, **dict(kw, **bad)) != 0
        assert frag in L.last_error(), (bad, L.last_error())


# ------------------------------------------------------------------------------------------------------------------------
# fixed-order reductions
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncols", [256, 768, 1536, 2304])
def test_colsum_blocks_of_128_rows_with_every_tail(ncols):
    """rows_per_block = 128: one block, a second block of 1 or 3 rows (the scalar tail behind the four chains), short blocks; ld > ncols."""
    rng = np.random.default_rng(ncols)
    ld = ncols + 5
    fg = FloorGate()
    for rows in ROWS + (128, 129, 131):
        Y = varied(rng, (rows, ld))
        nblk = (rows + 127) // 128
        part = torch.full((nblk * ncols + 64,), float(SENT), device="cuda")
        d_Y = _dev(Y)
        unit(L.BWD_COLSUM, Y=_ptr(d_Y), part=_ptr(part), ld=ld, rows=rows, ncols=ncols)
        out = part.cpu().numpy()
        assert (out[nblk * ncols:] == SENT).all()
        got = out[:nblk * ncols].reshape(nblk, ncols)
        want = np.stack([Y[128 * b:128 * b + 128, :ncols].astype(np.float64).sum(0) for b in range(nblk)])
        f32 = np.stack([seq_sum32(Y[128 * b:128 * b + 128, :ncols]) for b in range(nblk)])
        fg.add("colsum", f"{rows}x{ncols}", got, want, f32)
    fg.check()


def _reduce_case(rng, nparts, n, mode):
    """mode 0: 16-byte path (stride % 4 == 0, aligned pointer); 1: stride not a multiple of 4; 2: pointer 4 bytes off."""
    stride = ((n + 3) // 4) * 4 + 8 + (1 if mode == 1 else 0)
    off = 1 if mode == 2 else 0
    buf = np.full(off + nparts * stride + 16, np.nan, np.float32)
    vals = varied(rng, (nparts, n))
    idx = off + np.arange(nparts)[:, None] * stride + np.arange(n)[None, :]
    buf[idx] = vals
    return dict(buf=_dev(buf), off=off, stride=stride, nparts=nparts, n=n, vals=vals)


def _reduce_single(c, alpha):
    out = torch.full((c["n"] + 16,), float(SENT), device="cuda")
    r = L.BwdReduce()
    r.part[0], r.out[0], r.stride[0], r.n[0], r.nparts[0], r.alpha[0], r.count = _ptr(c["buf"], c["off"]), _ptr(out), c["stride"], c["n"], c["nparts"], alpha, 1
    assert L.load_library().iefvad_backward_unit(L.BWD_REDUCE_PARTS, C.byref(r), C.sizeof(r), _stream()) == 0, L.last_error()
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[c["n"]:] == SENT).all()
    return o[:c["n"]]


def _reduce_in_the_kernels_order(vals, alpha):
    """backward.h, reduce_parts_strip, restated in fp32: the partials are cut into 16 contiguous groups of ceil(nparts / 16), each group
    is added in index order from zero, the 16 group sums are added in group order from zero, and the total is scaled once.  Only
    additions and one product: the bits are determined."""
    nparts, n = vals.shape
    chunk = (nparts + 15) // 16
    r = np.zeros(n, np.float32)
    for g in range(16):
        s = np.zeros(n, np.float32)
        for p in range(g * chunk, min(g * chunk + chunk, nparts)):
            s = s + vals[p]
        r = r + s
    return np.float32(alpha) * r


def test_reduce_parts_every_group_size_strip_edge_and_alignment():
    """nparts around the 16 groups (1, 15, 16, 17), the unrolled-by-8 body (64, 1024); n around the 64-element strip (1, 63, 64, 65, 768:
    the scalar path where a quad crosses n); the unaligned paths; alpha != 1 with |alpha| <= 1, so nparts 2^-24 sum|part| bounds the sum,
    the scaling and its rounding.  The order is FIXED (gradients are bit-reproducible because of it): the result equals the fp32
    restatement of that order bit for bit.  Multi-job launches of one to four unequal jobs equal the single-job kernel bit for bit and a fifth
    job is ignored."""
    rng = np.random.default_rng(7)
    alpha = -0.75
    cases, singles = [], []
    for nparts, n, mode in itertools.product((1, 15, 16, 17, 64, 1024), (1, 63, 64, 65, 768), (0, 1, 2)):
        c = _reduce_case(rng, nparts, n, mode)
        got = _reduce_single(c, alpha)
        v64 = c["vals"].astype(np.float64)
        err = np.abs(got - alpha * v64.sum(0))
        bound = nparts * U * np.abs(v64).sum(0)
        assert (err <= bound).all(), (nparts, n, mode, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.array_equal(got.view(np.int32), _reduce_in_the_kernels_order(c["vals"], alpha).view(np.int32)), (nparts, n, mode)
        cases.append(c)
        singles.append(got)
    # multi: consecutive cases of unequal sizes, 1 to 4 (then 5, the fifth ignored) jobs per launch
    lib = L.load_library()
    pos = 0
    for count in (1, 2, 3, 4, 5, 4, 3, 5):
        group = list(range(pos, pos + count))
        pos += count + 7                                              # walk through different (nparts, n, alignment) mixes
        r = L.BwdReduce()
        outs = []
        for j, ci in enumerate(group):
            c = cases[ci]
            o = torch.full((c["n"] + 16,), float(SENT), device="cuda")
            outs.append(o)
            r.part[j], r.out[j], r.stride[j], r.n[j], r.nparts[j], r.alpha[j] = _ptr(c["buf"], c["off"]), _ptr(o), c["stride"], c["n"], c["nparts"], alpha
        r.count = count
        assert lib.iefvad_backward_unit(L.BWD_REDUCE_PARTS_MULTI, C.byref(r), C.sizeof(r), _stream()) == 0, L.last_error()
        torch.cuda.synchronize()
        for j, ci in enumerate(group):
            o = outs[j].cpu().numpy()
            if j == 4:
                assert (o == SENT).all()                              # ReduceBatch holds four jobs: the fifth is dropped, not run
                continue
            assert (o[cases[ci]["n"]:] == SENT).all()
            assert np.array_equal(o[:cases[ci]["n"]].view(np.int32), singles[ci].view(np.int32)), (count, j)


# ------------------------------------------------------------------------------------------------------------------------
# attention probabilities
# ------------------------------------------------------------------------------------------------------------------------
def _scores(rng, rows):
    S = (rng.standard_normal((rows, 256)) * 3).astype(np.float32)
    for r in range(rows):
        kind = r % 4
        if kind == 1:
            S[r, rng.integers(256)] += 30.0                           # a dominant key
        elif kind == 2:
            S[r] = np.float32(rng.standard_normal())                  # all-equal scores
        elif kind == 3:
            S[r] = rng.uniform(-80, 80, 256).astype(np.float32)       # +-80 spread: most keys underflow
    return S


def _dropout_bits(seed, idx):
    """common.h dropout_bits, restated: two rounds of murmur3's 32-bit finaliser over (seed, element index), 24 bits."""
    M32 = 0xFFFFFFFF

    def fmix32(x):
        x = x & M32
        x = x ^ (x >> 16); x = (x * 0x85EBCA6B) & M32
        x = x ^ (x >> 13); x = (x * 0xC2B2AE35) & M32
        return x ^ (x >> 16)
    a = fmix32((idx & M32) ^ (seed & M32))
    return fmix32((a + (seed >> 32) + (idx >> 32) * 0x9E3779B1) & M32) >> 8


@pytest.mark.parametrize("mode", ["off", "injected_mask", "generator"])
def test_softmax_dropout_probabilities_and_sign_bits(mode):
    """|P| against the fp64 softmax on rows with a dominant key, all-equal scores and a +-80 spread; the sign bits exactly: none
    (dropout off), the injected mask's zeros, or the library generator's draws below p, re-derived here."""
    rng = np.random.default_rng(11)
    p, seed = 0.1, 0x1234567887654321
    fg = FloorGate()
    for rows in ROWS:
        S = _scores(rng, rows)
        buf = np.full((rows + 5, 256), SENT, np.float32)
        buf[:rows] = S
        d = _dev(buf)
        keep = None
        if mode == "injected_mask":
            keep = (rng.random((rows, 256)) >= 0.3).astype(np.uint8)
            keep[:, 0] = 0
            dk = _dev(keep)
        unit(L.BWD_SOFTMAX_DROPOUT, S=_ptr(d), keep=dk.data_ptr() if keep is not None else None, seed=seed, rows=rows, drop=int(mode != "off"), p=p)
        out = d.cpu().numpy()
        assert (out[rows:] == SENT).all()
        got = out[:rows]
        want = torch.softmax(torch.from_numpy(S).double(), -1).numpy()
        f32 = torch.softmax(torch.from_numpy(S), -1).numpy()
        fg.add("softmax_dropout", f"{mode},{rows}", np.abs(got), want, f32)
        neg = np.signbit(got)
        if mode == "off":
            assert not neg.any()
        elif mode == "injected_mask":
            assert np.array_equal(neg, keep == 0)
        else:
            idx = torch.arange(rows * 256, dtype=torch.int64)
            dropped = (_dropout_bits(seed, idx) < int(p * 16777216.0)).view(rows, 256).numpy()
            assert np.array_equal(neg, dropped)
            if rows >= 130:
                assert 0.08 < neg.mean() < 0.12
    fg.check()


def test_softmax_backward_on_probabilities_with_dropped_dominant_keys():
    """dS = Pd .* dPd - P rowsum(Pd .* dPd), Pd = sign ? 0 : P scale, in place over dPd; dominant keys are among the dropped ones, where
    P is large and Pd is zero.  A second pass with no sign set and scale 1 is the plain softmax backward."""
    rng = np.random.default_rng(12)
    fg = FloorGate()
    for rows in ROWS:
        for p in (0.1, 0.0):
            P = torch.softmax(torch.from_numpy(_scores(rng, rows)), -1).numpy()
            scale = np.float32(1.0 / (1.0 - p))
            Ps = P.copy()
            if p:
                drop = rng.random(P.shape) < p
                drop[np.arange(1, rows, 8), P[1::8].argmax(1)] = True          # the dominant key of every other such row
                Ps[drop] = -Ps[drop]
            g = varied(rng, (rows, 256))
            buf = np.full((rows + 5, 256), SENT, np.float32)
            buf[:rows] = g
            d = _dev(buf)
            d_Ps = _dev(Ps)
            unit(L.BWD_SOFTMAX_BWD, Ps=_ptr(d_Ps), dPd=_ptr(d), rows=rows, scale=float(scale))
            out = d.cpu().numpy()
            assert (out[rows:] == SENT).all()

            def formula(dt):
                ps, gg, s = Ps.astype(dt), g.astype(dt), dt(scale)
                t = np.where(np.signbit(Ps), dt(0), ps * s) * gg
                return t - np.abs(ps) * t.sum(-1, keepdims=True, dtype=dt)
            fg.add("softmax_bwd", f"{rows},{p}", out[:rows], formula(np.float64), formula(np.float32))
    fg.check()


# ------------------------------------------------------------------------------------------------------------------------
# classifier, fusion, LayerNorm
# ------------------------------------------------------------------------------------------------------------------------
def _reduce_two(part_a, stride_a, n_a, part_b, stride_b, n_b, nparts):
    """The two-job reduction behind the scorer and LayerNorm backward (train.h), alpha = 1."""
    oa, ob = torch.full((n_a,), float(SENT), device="cuda"), torch.full((n_b,), float(SENT), device="cuda")
    r = L.BwdReduce()
    r.part[0], r.out[0], r.stride[0], r.n[0], r.nparts[0], r.alpha[0] = part_a, _ptr(oa), stride_a, n_a, nparts, 1.0
    r.part[1], r.out[1], r.stride[1], r.n[1], r.nparts[1], r.alpha[1] = part_b, _ptr(ob), stride_b, n_b, nparts, 1.0
    r.count = 2
    assert L.load_library().iefvad_backward_unit(L.BWD_REDUCE_PARTS_MULTI, C.byref(r), C.sizeof(r), _stream()) == 0, L.last_error()
    torch.cuda.synchronize()
    return oa.cpu().numpy(), ob.cpu().numpy()


@pytest.mark.parametrize("has_dlogit,has_dfused", [(False, False), (True, False), (False, True), (True, True)])
def test_scorer_backward_with_and_without_each_incoming_gradient(has_dlogit, has_dfused):
    """g = dlogit w (+ d fused); per 32-row block the sums of dlogit z and of dlogit, then their fixed-order reduction: d w_c, d b_c."""
    rng = np.random.default_rng(20 + 2 * has_dlogit + has_dfused)
    w = varied(rng, 768, 1.0)
    fg = FloorGate()
    for rows in ROWS:
        z, dl, df = varied(rng, (rows, 768)), varied(rng, rows), varied(rng, (rows, 768))
        nblk = (rows + 31) // 32
        g = torch.full(((rows + 3) * 768,), float(SENT), device="cuda")
        pw = torch.full(((nblk + 1) * 768,), float(SENT), device="cuda")
        pb = torch.full((nblk + 8,), float(SENT), device="cuda")
        d_dl, d_df, d_z, d_w = _dev(dl), _dev(df), _dev(z), _dev(w)
        unit(L.BWD_SCORER, dlogit=_ptr(d_dl) if has_dlogit else None, dfused=_ptr(d_df) if has_dfused else None, z=_ptr(d_z), w=_ptr(d_w),
             g=_ptr(g), part_w=_ptr(pw), part_b=_ptr(pb), rows=rows)
        og, opw, opb = g.cpu().numpy(), pw.cpu().numpy(), pb.cpu().numpy()
        assert (og[rows * 768:] == SENT).all() and (opw[nblk * 768:] == SENT).all() and (opb[nblk:] == SENT).all()

        def formula(dt):
            dlv = dl.astype(dt) if has_dlogit else np.zeros(rows, dt)
            gg = dlv[:, None] * w.astype(dt)[None, :]
            if has_dfused:
                gg = gg + df.astype(dt)
            prod = dlv[:, None] * z.astype(dt)
            if dt is np.float64:
                s = lambda x: x.sum(0)
            else:
                s = seq_sum32
            pw_ = np.stack([s(prod[32 * b:32 * b + 32]) for b in range(nblk)])
            pb_ = np.stack([s(dlv[32 * b:32 * b + 32]) for b in range(nblk)])
            return gg, pw_, pb_, s(prod), s(dlv)
        w64, w32 = formula(np.float64), formula(np.float32)
        tag = f"{rows},{int(has_dlogit)}{int(has_dfused)}"
        fg.add("scorer_bwd.g", tag, og[:rows * 768].reshape(rows, 768), w64[0], w32[0])
        fg.add("scorer_bwd.part_w", tag, opw[:nblk * 768].reshape(nblk, 768), w64[1], w32[1])
        fg.add("scorer_bwd.part_b", tag, opb[:nblk], w64[2], w32[2])
        dw, dbias = _reduce_two(_ptr(pw), 768, 768, _ptr(pb), 1, 1, nblk)
        fg.add("scorer_bwd.dw", tag, dw, w64[3], w32[3])
        fg.add("scorer_bwd.db", tag, dbias, w64[4], w32[4])
    fg.check()


FUSION_GRADS = ("d_mu_i", "d_lv_i", "d_mu_e", "d_lv_e", "d_n_i", "d_n_e")


def _fusion_reference(dt, mu_i, lv_i, mu_e, lv_e, gz, direct, factor, eps):
    """The literal expression of the reference model's fusion (imf_vad.py:130-144), differentiated by autograd in `dt`: the loss hands
    gz to `fused` and the direct gradients to the image_mu / image_logvar / event_mu / event_logvar / w_i / w_e outputs."""
    leaves = [torch.from_numpy(x).to(dt).requires_grad_(True) for x in (mu_i, lv_i, mu_e, lv_e)]
    image_mu, image_logvar, event_mu, event_logvar = leaves
    f = torch.tensor(float(factor), dtype=dt)
    weight_image = f * torch.exp(-image_logvar)
    weight_event = f * torch.exp(-event_logvar)
    denom = weight_image + weight_event + torch.tensor(float(eps), dtype=dt)
    norm_weight_image = weight_image / denom
    norm_weight_event = weight_event / denom
    fused = norm_weight_image * image_mu + norm_weight_event * event_mu
    outs = {"d_mu_i": image_mu, "d_lv_i": image_logvar, "d_mu_e": event_mu, "d_lv_e": event_logvar, "d_n_i": norm_weight_image, "d_n_e": norm_weight_event}
    loss = (fused * torch.from_numpy(gz).to(dt)).sum()
    for k, v in direct.items():
        loss = loss + (outs[k] * torch.from_numpy(v).to(dt)).sum()
    g = torch.autograd.grad(loss, leaves)
    return (torch.cat([g[0], g[1]], 1).numpy(), torch.cat([g[2], g[3]], 1).numpy())


def _fusion_case(fg, rng, rows, factor, eps, names, tag):
    mu_i, mu_e, gz = varied(rng, (rows, 768), 1.0), varied(rng, (rows, 768), 1.0), varied(rng, (rows, 768), 1.0)
    lv_i, lv_e = rng.uniform(-6, 6, (rows, 768)).astype(np.float32), rng.uniform(-6, 6, (rows, 768)).astype(np.float32)
    direct = {k: varied(rng, (rows, 768), 1.0) for k in names}
    dev = {k: _dev(v) for k, v in dict(mu_i=mu_i, lv_i=lv_i, mu_e=mu_e, lv_e=lv_e, gz=gz, **direct).items()}
    dh = [torch.full(((rows + 2) * 1536,), float(SENT), device="cuda") for _ in range(2)]
    unit(L.BWD_FUSION, dh_i=_ptr(dh[0]), dh_e=_ptr(dh[1]), rows=rows, factor=float(factor), eps=float(eps), **{k: _ptr(v) for k, v in dev.items()})
    want = _fusion_reference(torch.float64, mu_i, lv_i, mu_e, lv_e, gz, direct, factor, eps)
    f32 = _fusion_reference(torch.float32, mu_i, lv_i, mu_e, lv_e, gz, direct, factor, eps)
    for m in range(2):
        o = dh[m].cpu().numpy()
        assert (o[rows * 1536:] == SENT).all()
        fg.add("fusion_bwd.dh_" + "ie"[m], tag, o[:rows * 1536].reshape(rows, 1536), want[m], f32[m])


@pytest.mark.parametrize("nu", [None, 1, 5, 8])
def test_fusion_backward_for_every_noise_model_and_epsilon(nu):
    """Gaussian (factor 1) and Student-t with nu in {1, 5, 8}; the model's epsilon and a large one (0.5: n_i + n_e != 1, so a dropped
    or mis-signed d den term shows); logvars in [-6, 6] (one modality dominates); no direct gradients and all six."""
    rng = np.random.default_rng(30 + (nu or 0))
    factor = np.float32(1.0) if nu is None else np.float32((np.float32(nu) + np.float32(1.0)) / np.float32(nu))
    fg = FloorGate()
    for eps in (np.float32(1e-8), np.float32(0.5)):
        for rows in ROWS:
            for names in ((), FUSION_GRADS):
                _fusion_case(fg, rng, rows, factor, eps, names, f"nu={nu},eps={eps},rows={rows},{len(names)}")
    fg.check()


def test_fusion_backward_with_every_subset_of_the_direct_gradients():
    """The loss may hand a gradient to any of image_mu, image_logvar, event_mu, event_logvar, w_i, w_e: all 64 subsets."""
    rng = np.random.default_rng(40)
    factor = np.float32(np.float32(9.0) / np.float32(8.0))
    fg = FloorGate()
    for bits in range(64):
        names = tuple(k for i, k in enumerate(FUSION_GRADS) if bits >> i & 1)
        _fusion_case(fg, rng, 33, factor, np.float32(0.5), names, f"subset={bits:06b}")
    fg.check()


@pytest.mark.parametrize("alias", [True, False])
def test_layernorm_backward_with_hard_rows_in_place_and_per_block_partials(alias):
    """dx = rstd (dyg - mean(dyg) - xh mean(dyg xh)), dyg = dy gamma, with a non-trivial gamma; rows of tiny variance (a constant plus
    1e-3 noise: eps = 1e-5 is not negligible against the variance) and of large mean (offset 1e3); dx written over dy as the training
    step does, or to a buffer of its own; d gamma / d beta partial sums per 32-row block, then reduced."""
    rng = np.random.default_rng(50 + alias)
    gamma = varied(rng, 768, 1.0)
    eps = np.float32(1e-5)
    fg = FloorGate()
    for rows in ROWS:
        x = varied(rng, (rows, 768), 1.0)
        x[0::3] = (np.float32(rng.standard_normal()) + 1e-3 * rng.standard_normal(x[0::3].shape)).astype(np.float32)
        x[1::3] += np.float32(1e3)
        dy = varied(rng, (rows, 768), 1.0)
        nblk = (rows + 31) // 32
        buf = np.full((rows + 3, 768), SENT, np.float32)
        buf[:rows] = dy
        d_dy = _dev(buf)
        d_dx = d_dy if alias else torch.full(((rows + 3) * 768,), float(SENT), device="cuda")
        pg = torch.full(((nblk + 1) * 768,), float(SENT), device="cuda")
        pb = torch.full(((nblk + 1) * 768,), float(SENT), device="cuda")
        d_x, d_gamma = _dev(x), _dev(gamma)
        unit(L.BWD_LAYERNORM, x=_ptr(d_x), dy=_ptr(d_dy), g=_ptr(d_gamma), dx=_ptr(d_dx), part_g=_ptr(pg), part_b=_ptr(pb), rows=rows, eps=float(eps))
        odx, opg, opb = d_dx.cpu().numpy().reshape(-1), pg.cpu().numpy(), pb.cpu().numpy()
        assert (odx[rows * 768:] == SENT).all() and (opg[nblk * 768:] == SENT).all() and (opb[nblk * 768:] == SENT).all()
        if not alias:
            assert np.array_equal(d_dy.cpu().numpy()[:rows], dy)

        def formula(dt):
            xx, dd, gg = x.astype(dt), dy.astype(dt), gamma.astype(dt)
            inv = dt(1.0) / dt(768)
            xc = xx - xx.sum(-1, keepdims=True, dtype=dt) * inv
            var = (xc * xc).sum(-1, keepdims=True, dtype=dt) * inv
            rstd = dt(1.0) / np.sqrt(var + dt(eps))
            xh = xc * rstd
            dyg = dd * gg
            c1 = dyg.sum(-1, keepdims=True, dtype=dt) * inv
            c2 = (dyg * xh).sum(-1, keepdims=True, dtype=dt) * inv
            dx = rstd * (dyg - c1 - xh * c2)
            s = (lambda v: v.sum(0)) if dt is np.float64 else seq_sum32
            pg_ = np.stack([s((dd * xh)[32 * b:32 * b + 32]) for b in range(nblk)])
            pb_ = np.stack([s(dd[32 * b:32 * b + 32]) for b in range(nblk)])
            return dx, pg_, pb_, s(dd * xh), s(dd)
        w64, w32 = formula(np.float64), formula(np.float32)
        tag = f"{rows},{int(alias)}"
        gdx = odx[:rows * 768].reshape(rows, 768)
        for c, name in enumerate(("tiny_variance", "large_mean", "plain")):      # row r is of class r % 3: a floor per class, or the hard rows' would hide the plain ones
            if rows > c:
                fg.add("layernorm_bwd.dx." + name, tag, gdx[c::3], w64[0][c::3], w32[0][c::3])
        fg.add("layernorm_bwd.part_g", tag, opg[:nblk * 768].reshape(nblk, 768), w64[1], w32[1])
        fg.add("layernorm_bwd.part_b", tag, opb[:nblk * 768].reshape(nblk, 768), w64[2], w32[2])
        dg, db = _reduce_two(_ptr(pg), 768, 768, _ptr(pb), 768, 768, nblk)
        fg.add("layernorm_bwd.dgamma", tag, dg, w64[3], w32[3])
        fg.add("layernorm_bwd.dbeta", tag, db, w64[4], w32[4])
    fg.check()
