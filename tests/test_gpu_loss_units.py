"""The loss head, the optimiser and the NaN rule ONE kernel at a time (csrc/loss.h, the two NaN-rule kernels of csrc/train.h) against
fp64, whole tensors, at their edges.

Every kernel is reached through its existing C entry on buffers this file owns (`iefvad_loss_forward`, `iefvad_loss_backward`,
`iefvad_adamw_step`, `iefvad_adamw_step_multi`, `iefvad_nan_rule`); the forward's per-row partials `part[B T][4]` and per-video scores
`inst[B]` are read back from the caller's workspace (include/iefvad.h documents the layout).  Every output buffer sits between
sentinel guard bands that must survive.  The loss's fp64 restatement is the reference trainers' literal torch lines (torch.sigmoid,
torch.topk, F.binary_cross_entropy, F.normalize, F.cosine_similarity, torch.norm, the KL expression) run in .double() with autograd.

Gates: no constant fixed in advance.  The same torch lines in fp32 on the CPU give, per kernel output and per row class (row r is in
class r mod number-of-classes), a reference-side floor -- their worst error against fp64 on the test's own inputs -- and the kernel is
held to FLOOR_FACTOR (3) x that floor (tests/helpers.py: FloorGate; ARITHMETIC.md, section "Loss head, optimiser and NaN rule one
kernel at a time", records floors and measured ratios; each test prints both).  Where a bound is derived instead (the finish kernel's
double sums, bit-exact repairs), the derivation stands at the assertion.

Left out on purpose: rows whose norm is below 1e-19 (their squares are fp32 subnormals; see the comment in loss.h), logits with
12 < |x| < 30 (fp32 decides whether 1 - p is zero there and no floor is stable), and norms "equalised" by scaling: the sign of a
rounding-sized norm difference belongs to each arithmetic, so the equal-norm class flips signs of entries instead, which leaves the two
norms bit-identical in every arithmetic and every summation order.  Needs a real MI355X: run with `-m gpu`."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from iefvad_amd import lib as L
from iefvad_amd import losses
from tests.helpers import FLOOR_FACTOR, FloorGate

pytestmark = pytest.mark.gpu

T, D = 256, 768
SENT = np.float32(-7777.25)                      # guard value: no test input or result equals it
GUARD = 64                                       # floats on each side of an output buffer (256 bytes: keeps 16-byte alignment)
NOISES = (("Gaussian", 8.0), ("StudentT", 8.0), ("StudentT", 0.5))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


class Guarded:
    """n floats on the device between two bands of SENT; read() checks the bands and returns the n floats."""

    def __init__(self, n, init=None, guard=GUARD):
        self.n, self.g = int(n), guard
        host = np.full(self.n + 2 * guard, SENT, np.float32)
        if init is not None:
            host[guard:guard + self.n] = np.asarray(init, np.float32).ravel()
        self.buf = torch.from_numpy(host).cuda()

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 4 * self.g)

    def read(self):
        h = self.buf.cpu().numpy()
        assert (h[:self.g] == SENT).all() and (h[self.g + self.n:] == SENT).all(), "a write outside the output buffer"
        return h[self.g:self.g + self.n].copy()


def _noise_id(noise):
    return L.NOISE_STUDENT_T if noise == "StudentT" else L.NOISE_GAUSSIAN


# ------------------------------------------------------------------------------------------------------------------------
# the C entries on numpy arrays
# ------------------------------------------------------------------------------------------------------------------------
def dev_loss_forward(logits, lengths, targets, heads=None, noise="Gaussian", nu=8.0, lam=(1.0, 1.0)):
    """-> out[8], part[B T, 4] (None without heads), inst[B]: the last two read from the workspace."""
    B = logits.shape[0]
    lib = L.load_library()
    need = lib.iefvad_loss_workspace_bytes(B, T)
    assert need >= (B * T * 4 + B) * 4 and need % 4 == 0
    ws, out = Guarded(need // 4), Guarded(8)
    keep = [_dev(logits.astype(np.float32)), _dev(lengths.astype(np.int32)), _dev(targets.astype(np.float32))]
    hs = [None] * 4 if heads is None else [h if isinstance(h, torch.Tensor) else _dev(h) for h in heads]
    rc = lib.iefvad_loss_forward(_ptr(keep[0]), _ptr(hs[0]), _ptr(hs[1]), _ptr(hs[2]), _ptr(hs[3]), _ptr(keep[1]), _ptr(keep[2]), B, T,
                                 _noise_id(noise), float(nu), float(lam[0]), float(lam[1]), out.ptr, ws.ptr, need, _stream())
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    w = ws.read()
    part = w[:B * T * 4].reshape(B * T, 4) if heads is not None else None
    if heads is None:
        assert (w[:B * T * 4] == SENT).all(), "CLAS2 alone wrote row partials"
    return out.read(), part, w[B * T * 4:B * T * 4 + B]


GRADS = ("logits", "mu_i", "mu_e", "lv_i", "lv_e")


def dev_loss_backward(logits, lengths, targets, heads, noise="Gaussian", nu=8.0, lam=(1.0, 1.0), grad_scale=1.0, scale_dev=None,
                      want=GRADS):
    """-> {name: gradient} for the names in `want`; every other d_* pointer is NULL."""
    B = logits.shape[0]
    keep = [_dev(logits.astype(np.float32)), _dev(lengths.astype(np.int32)), _dev(targets.astype(np.float32))]
    hs = [None] * 4 if heads is None else [h if isinstance(h, torch.Tensor) else _dev(h) for h in heads]
    outs = {k: Guarded(B * T * (1 if k == "logits" else D)) for k in want}
    sd = _dev(np.array([scale_dev], np.float32)) if scale_dev is not None else None
    p = [outs[k].ptr if k in outs else None for k in GRADS]
    rc = L.load_library().iefvad_loss_backward(_ptr(keep[0]), _ptr(hs[0]), _ptr(hs[1]), _ptr(hs[2]), _ptr(hs[3]), _ptr(keep[1]), _ptr(keep[2]),
                                               B, T, _noise_id(noise), float(nu), float(lam[0]), float(lam[1]), float(grad_scale),
                                               p[0], p[1], p[2], p[3], p[4], _ptr(sd), _stream())
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    return {k: o.read().reshape(B * T, -1) if k != "logits" else o.read().reshape(B, T) for k, o in outs.items()}


# ------------------------------------------------------------------------------------------------------------------------
# the reference trainers' lines, in the dtype asked for
# ------------------------------------------------------------------------------------------------------------------------
def ref_inst(logits, lengths):
    """CLAS2 up to `instance_logits`: sigmoid, per video the mean of the int(len / 16 + 1) largest of the first len scores."""
    p = torch.sigmoid(logits).reshape(logits.shape[0], logits.shape[1])
    inst = torch.zeros(0, dtype=logits.dtype)
    for i in range(p.shape[0]):
        n = int(lengths[i])
        tmp, _ = torch.topk(p[i, 0:n], k=int(n / 16 + 1), largest=True)
        inst = torch.cat([inst, torch.mean(tmp).view(1)], dim=0)
    return inst


def ref_rows(mu_i, mu_e, lv_i, lv_e, noise, nu):
    """Per row: 1 - cos, |norm_i - norm_e|, and the row sums of the two KL expressions (their mean is the trainers' KL / -0.5)."""
    cos = F.cosine_similarity(F.normalize(mu_i, p=2, dim=-1), F.normalize(mu_e, p=2, dim=-1), dim=-1)
    nrm = torch.abs(torch.norm(mu_i, p=2, dim=-1) - torch.norm(mu_e, p=2, dim=-1))
    if noise == "StudentT":
        lv_i = lv_i + math.log(nu / (nu + 1))
        lv_e = lv_e + math.log(nu / (nu + 1))
    kl_i = (1 + lv_i - mu_i.pow(2) - lv_i.exp()).sum(-1)
    kl_e = (1 + lv_e - mu_e.pow(2) - lv_e.exp()).sum(-1)
    return torch.stack([1 - cos, nrm, kl_i, kl_e], dim=-1)


def ref_head_total(mu_i, mu_e, lv_i, lv_e, noise, nu, lam):
    """lambda_reg (loss_cos.mean() + loss_norm.mean()) + lambda_kl (kl_image + kl_event), the trainers' lines."""
    cos = F.cosine_similarity(F.normalize(mu_i, p=2, dim=-1), F.normalize(mu_e, p=2, dim=-1), dim=-1)
    loss_norm = torch.abs(torch.norm(mu_i, p=2, dim=-1) - torch.norm(mu_e, p=2, dim=-1))
    loss_reg = (1 - cos).mean() + loss_norm.mean()
    if noise == "StudentT":
        lv_i = lv_i + math.log(nu / (nu + 1))
        lv_e = lv_e + math.log(nu / (nu + 1))
    kl_i = -0.5 * torch.mean(1 + lv_i - mu_i.pow(2) - lv_i.exp())
    kl_e = -0.5 * torch.mean(1 + lv_e - mu_e.pow(2) - lv_e.exp())
    return lam[0] * loss_reg + lam[1] * (kl_i + kl_e)


def add_by_class(fg, kind, tag, got, want, f32, cls, names):
    for c, name in enumerate(names):
        m = cls == c
        if m.any():
            fg.add(f"{kind}/{name}", tag, np.asarray(got)[m], np.asarray(want)[m], np.asarray(f32)[m])


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
LENS = (1, 15, 16, 17, 31, 32, 240, 255, 256, 300)       # k = int(len / 16 + 1) on both sides of a multiple of 16; 300: sliced to 256, k = 19
VIDEO_KINDS = ("grid", "p=1", "p=0", "bounded")


def grid_video(rng, lo=-6.0, hi=6.0, offset=0.1):
    """A seeded permutation of an evenly spaced grid plus one offset: neighbouring sigmoids differ by >= 1e-4 on [-6.1, 6.1]."""
    return (rng.permutation(np.linspace(lo, hi, T)) + rng.uniform(-offset, offset)).astype(np.float32)


def topk_batch(seed, saturated=True):
    """-> logits [B, 256], lengths, targets, kind per video (index into VIDEO_KINDS), {"nan_in": v, "nan_behind": v}."""
    rng = np.random.default_rng(seed)
    rows, lens, tg, kinds = [], [], [], []
    for n in LENS:
        for y in (0.0, 1.0):
            rows.append(grid_video(rng)); lens.append(n); tg.append(y); kinds.append(0)
    if saturated:
        rows.append(np.full(T, 30.0, np.float32)); lens.append(256); tg.append(0.0); kinds.append(1)
        rows.append(np.full(T, -110.0, np.float32)); lens.append(200); tg.append(1.0); kinds.append(2)
    for y in (0.0, 1.0):
        rows.append(grid_video(rng, -12.0, 12.0, 0.0)); lens.append(250); tg.append(y); kinds.append(3)
    special = {}
    v = grid_video(rng); v[40] = np.nan                        # inside the valid prefix: torch.topk ranks NaN first, the mean is NaN
    special["nan_in"] = len(rows); rows.append(v); lens.append(100); tg.append(1.0); kinds.append(0)
    v = grid_video(rng); v[200] = np.nan                       # behind the prefix: nobody reads it
    special["nan_behind"] = len(rows); rows.append(v); lens.append(100); tg.append(0.0); kinds.append(0)
    lg = np.stack(rows)
    sg = np.sort(1.0 / (1.0 + np.exp(-lg[np.array(kinds) == 0].astype(np.float64))), axis=1)
    assert np.nanmin(np.diff(sg, axis=1)) >= 1e-4               # the selection is unambiguous in fp32
    return lg, np.array(lens, np.int32), np.array(tg, np.float32), np.array(kinds), special


ROW_CLASSES = ("plain", "identical", "parallel_gap1e-3", "antiparallel", "near_parallel", "mu_i_x1e3", "mu_e_x1e-4", "both_x1e-6",
               "zero_image", "zero_event", "both_zero", "equal_norms", "below_clamp_x1e-16", "logvar_i_+8", "logvar_e_-30")


def head_rows(seed, R):
    """Four [R, 768] fp32 tensors whose row r is of class r mod 15 (ROW_CLASSES) -> (mu_i, mu_e, lv_i, lv_e), class per row."""
    rng = np.random.default_rng(seed)
    mi = (0.3 * rng.standard_normal((R, D))).astype(np.float32)
    me = (0.3 * rng.standard_normal((R, D)) + 0.2 * mi).astype(np.float32)
    li = (-2.0 + rng.standard_normal((R, D))).astype(np.float32)
    le = (-2.0 + rng.standard_normal((R, D))).astype(np.float32)
    cls = np.arange(R) % len(ROW_CLASSES)
    c = lambda name: cls == ROW_CLASSES.index(name)
    me[c("identical")] = mi[c("identical")]
    me[c("parallel_gap1e-3")] = mi[c("parallel_gap1e-3")] * np.float32(1.001)
    me[c("antiparallel")] = mi[c("antiparallel")] * np.float32(-0.7)
    m = c("near_parallel")
    me[m] = (mi[m] + np.float32(1e-3) * rng.standard_normal((int(m.sum()), D)).astype(np.float32)) * np.float32(1.001)   # norm gap 8 sigma off 0
    mi[c("mu_i_x1e3")] *= np.float32(1e3)
    me[c("mu_e_x1e-4")] *= np.float32(1e-4)
    mi[c("both_x1e-6")] *= np.float32(1e-6)
    me[c("both_x1e-6")] *= np.float32(1e-6)
    mi[c("zero_image")] = 0
    me[c("zero_event")] = 0
    mi[c("both_zero")] = 0
    me[c("both_zero")] = 0
    m = c("equal_norms")                                       # the same magnitudes, half of the signs flipped: |mu_i| == |mu_e| to the bit
    me[m] = mi[m] * np.where(rng.random((int(m.sum()), D)) < 0.5, np.float32(-1), np.float32(1))
    m = np.flatnonzero(c("below_clamp_x1e-16"))                # norm ~ 8e-16 < F.normalize's 1e-12: the image row, and on odd instances both
    mi[m] *= np.float32(1e-16)
    me[m[1::2]] *= np.float32(1e-16)
    m = c("logvar_i_+8")
    li[m] = (8.0 + 0.1 * rng.standard_normal((int(m.sum()), D))).astype(np.float32)
    le[c("logvar_e_-30")] = -30.0
    # the sign of |mu_i| - |mu_e| must not hang on a rounding: either exactly zero or far from it (a row that comes too close by
    # chance gets its event row stretched by 1e-3)
    norms = lambda: (np.linalg.norm(mi.astype(np.float64), axis=1), np.linalg.norm(me.astype(np.float64), axis=1))
    ni, ne = norms()
    close = (np.abs(ni - ne) > 0) & (np.abs(ni - ne) <= 1e-5 * np.maximum(ni, ne))
    me[close] *= np.float32(1.001)
    ni, ne = norms()
    gap = np.abs(ni - ne)
    assert ((gap == 0) | (gap > 2e-6 * np.maximum(ni, ne))).all(), np.flatnonzero(~((gap == 0) | (gap > 2e-6 * np.maximum(ni, ne))))
    assert (np.minimum(ni, ne)[(ni > 0) & (ne > 0)] > 1e-19).all()
    return (mi, me, li, le), cls


def _t(x, dtype, grad=False):
    return torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_(grad)


# ------------------------------------------------------------------------------------------------------------------------
# 1. iefvad_mil_topk_kernel
# ------------------------------------------------------------------------------------------------------------------------
def test_topk_instance_scores_at_every_length_edge_saturation_and_nan():
    """inst[B] from the workspace against CLAS2's lines in fp64: lengths on both sides of every multiple of 16 that matters, 300 (sliced
    to 256, k = 19), both targets, videos at p = 1 and p = 0 exactly and one on [-12, 12], a NaN logit inside the prefix (NaN score)
    and one behind it (no effect)."""
    lg, lens, tg, kinds, special = topk_batch(1)
    _, _, inst = dev_loss_forward(lg, lens, tg)
    want = ref_inst(_t(lg, torch.float64), lens).numpy()
    f32 = ref_inst(_t(lg, torch.float32), lens).numpy()
    nanv = np.isnan(want)
    assert nanv.sum() == 1 and nanv[special["nan_in"]]
    assert np.array_equal(np.isnan(inst), nanv)
    fg = FloorGate()
    add_by_class(fg, "inst", "all", inst[~nanv], want[~nanv], f32[~nanv], kinds[~nanv], VIDEO_KINDS)
    fg.check()
    assert inst[kinds == 1][0] == 1.0 and inst[kinds == 2][0] == 0.0
    clean = lg.copy()
    clean[special["nan_behind"], 200] = 0.0
    assert np.array_equal(_bits(dev_loss_forward(clean, lens, tg)[2]), _bits(inst))


def test_topk_invalid_lengths_give_nan_for_exactly_those_videos():
    """loss.h: len <= 0 or k > len gives NaN (torch.topk raises there, so torch is not asked).  Lengths 0, -3 and 4096 (k = 257) placed
    first, in the middle and last: their inst is NaN, every other video's inst has the bits of a call without them, out[0] is NaN."""
    lg, lens, tg, _, special = topk_batch(2, saturated=False)
    good = np.array([v for v in range(lg.shape[0]) if v != special["nan_in"]])
    lg, lens, tg = lg[good], lens[good], tg[good]
    out0, _, inst0 = dev_loss_forward(lg, lens, tg)
    assert not np.isnan(inst0).any() and not np.isnan(out0[0])
    rng = np.random.default_rng(3)
    B = lg.shape[0]
    at = {0: 0, B // 2: -3, B + 2: 4096}                      # position in the widened batch -> bad length
    src = iter(range(B))
    rows, ln, y, keep = [], [], [], []
    for v in range(B + 3):
        if v in at:
            rows.append(grid_video(rng)); ln.append(at[v]); y.append(1.0)
        else:
            s = next(src)
            rows.append(lg[s]); ln.append(lens[s]); y.append(tg[s]); keep.append(v)
    out, _, inst = dev_loss_forward(np.stack(rows), np.array(ln, np.int32), np.array(y, np.float32))
    assert np.isnan(inst[list(at)]).all()
    assert np.array_equal(_bits(inst[keep]), _bits(inst0))
    assert np.isnan(out[0]) and np.isnan(out[7])


# ------------------------------------------------------------------------------------------------------------------------
# 2. iefvad_loss_rows_kernel
# ------------------------------------------------------------------------------------------------------------------------
COLS = ("1-cos", "norm_diff", "kl_sum_image", "kl_sum_event")


@pytest.mark.parametrize("noise,nu", NOISES)
def test_row_partials_whole_per_column_and_row_class(noise, nu):
    """part[256][4] from the workspace against the trainers' lines per row in fp64; floors per column and row class."""
    heads, cls = head_rows(10, T)
    lg, lens, tg = np.zeros((1, T), np.float32), np.array([256], np.int32), np.array([1.0], np.float32)
    _, part, _ = dev_loss_forward(lg, lens, tg, heads, noise, nu)
    want = ref_rows(*(_t(h, torch.float64) for h in heads), noise, nu).numpy()
    f32 = ref_rows(*(_t(h, torch.float32) for h in heads), noise, nu).numpy()
    fg = FloorGate()
    for j, col in enumerate(COLS):
        add_by_class(fg, f"part.{col}", f"{noise},{nu}", part[:, j], want[:, j], f32[:, j], cls, ROW_CLASSES)
    fg.check()


# ------------------------------------------------------------------------------------------------------------------------
# 3. iefvad_loss_finish_kernel
# ------------------------------------------------------------------------------------------------------------------------
def _bce(inst, targets, dtype):
    return float(F.binary_cross_entropy(_t(inst, dtype), _t(targets, dtype)))


def _check_finish(out, part, inst, tg, lam, fg, tag):
    """out[8] against the fp64 recombination of the kernel's OWN part / inst.  The kernel adds in double (a sum of <= 4352 fp32 values
    in double is exact to 1e-13 relative) and rounds once: terms 1-6 lie within one fp32 ulp of the rounded fp64 value."""
    B = inst.shape[0]
    if part is not None:
        s = part.astype(np.float64).sum(0)
        R = part.shape[0]
        lcos, lnorm, kli, kle = s[0] / R, s[1] / R, -0.5 * s[2] / (R * D), -0.5 * s[3] / (R * D)
    else:
        lcos = lnorm = kli = kle = 0.0
    want = np.array([lcos + lnorm, lcos, lnorm, kli + kle, kli, kle])
    assert (np.abs(out[1:7].astype(np.float64) - want) <= _ulp(want)).all(), (tag, out[1:7], want)
    if part is None:
        assert (out[1:7] == 0).all()
    if np.isnan(inst).any():
        assert np.isnan(out[0]) and np.isnan(out[7])
        return
    fg.add("out[0]", tag, out[0], _bce(inst, tg, torch.float64), _bce(inst, tg, torch.float32))
    lr, lk = float(np.float32(lam[0])), float(np.float32(lam[1]))            # the entry takes the weights as fp32
    add = np.array([float(out[0]), lr * float(out[1]), lk * float(out[4])])
    assert abs(float(out[7]) - add.sum()) <= 2 * _ulp(np.abs(add).max()), (tag, out, add)


@pytest.mark.parametrize("lam", [(1.0, 1.0), (0.01, 0.25)])
def test_finish_with_heads_at_every_block_and_tail_count(lam):
    """B in {1, 7, 8, 9, 16, 17}: the eight-rows-ahead block never, once, once + tail, twice, twice + tail."""
    fg = FloorGate()
    for B in (1, 7, 8, 9, 16, 17):
        heads, _ = head_rows(20 + B, B * T)
        rng = np.random.default_rng(30 + B)
        lg = np.stack([grid_video(rng) for _ in range(B)])
        lens = rng.integers(1, 301, B).astype(np.int32)
        tg = (rng.random(B) < 0.5).astype(np.float32)
        dh = [_dev(h) for h in heads]
        out, part, inst = dev_loss_forward(lg, lens, tg, dh, "StudentT", 8.0, lam)
        _check_finish(out, part, inst, tg, lam, fg, f"B={B}")
        out2, part2, inst2 = dev_loss_forward(lg, lens, tg, dh, "StudentT", 8.0, lam)
        assert np.array_equal(_bits(out), _bits(out2)) and np.array_equal(_bits(part), _bits(part2)) and np.array_equal(_bits(inst), _bits(inst2))
    fg.check()


def test_finish_clas2_alone_beyond_256_videos():
    """Head pointers NULL, B in {255, 256, 257, 513}: the video loop's second and third pass.  The only abnormal-target video is the
    last one, so a pass that is skipped changes the sum; at B = 513 a second run has a NaN score at video 300."""
    fg = FloorGate()
    for B in (255, 256, 257, 513):
        rng = np.random.default_rng(40 + B)
        lg = np.stack([grid_video(rng) for _ in range(B)])
        lens = rng.integers(1, 301, B).astype(np.int32)
        tg = np.zeros(B, np.float32)
        tg[B - 1] = 1.0
        for lam in ((1.0, 1.0), (0.01, 0.25)):
            out, part, inst = dev_loss_forward(lg, lens, tg, None, "Gaussian", 8.0, lam)
            assert part is None and not np.isnan(inst).any()
            _check_finish(out, None, inst, tg, lam, fg, f"B={B}")
        assert np.array_equal(_bits(out), _bits(dev_loss_forward(lg, lens, tg, None, "Gaussian", 8.0, lam)[0]))
        if B == 513:
            lg[300, 0] = np.nan
            out, _, inst = dev_loss_forward(lg, lens, tg)
            assert np.flatnonzero(np.isnan(inst)).tolist() == [300]
            _check_finish(out, None, inst, tg, (1.0, 1.0), fg, "B=513,nan")
    fg.check()


# ------------------------------------------------------------------------------------------------------------------------
# 4. iefvad_mil_topk_grad_kernel
# ------------------------------------------------------------------------------------------------------------------------
def _clas2_grad(lg, lens, tg, dtype, scale):
    """d (scale CLAS2) / d logits by autograd.  torch's CPU binary_cross_entropy refuses a NaN input, so a video whose score is NaN
    enters through BCE's definition written out (the clamps at -100 included) and the batch mean is the sum over B."""
    x, y = _t(lg, dtype, True), _t(tg, dtype)
    inst = ref_inst(x, lens)
    bad = torch.isnan(inst.detach())
    total = F.binary_cross_entropy(inst[~bad], y[~bad], reduction="sum")
    if bad.any():
        p = inst[bad]
        total = total - (y[bad] * torch.log(p).clamp_min(-100) + (1 - y[bad]) * torch.log(1 - p).clamp_min(-100)).sum()
    (scale * total / inst.numel()).backward()
    return x.grad.numpy()


def _clas2_grads(lg, lens, tg, scale, special):
    """fp64 and fp32 autograd.  torch takes the sigmoid of the whole tensor before it slices, so its gradient at a NaN logit BEHIND the
    prefix is 0 x NaN = NaN; the kernel never reads that logit and writes the exact 0 of every t >= len (loss.h).  That one element is
    asserted here and set to 0 in both references."""
    want, f32 = _clas2_grad(lg, lens, tg, torch.float64, scale), _clas2_grad(lg, lens, tg, torch.float32, scale)
    v = special["nan_behind"]
    assert np.isnan(want[v, 200]) and np.isnan(f32[v, 200]) and np.isnan(want[v]).sum() == 1
    want[v, 200] = f32[v, 200] = 0.0
    return want, f32


@pytest.mark.parametrize("grad_scale,scale_dev", [(1.0, None), (3.0, None), (1.0, 0.5), (3.0, 0.5)])
def test_topk_gradient_whole_tensor_support_and_nan_pattern(grad_scale, scale_dev):
    """d logits [B, 256] against fp64 autograd through CLAS2's lines: the nonzero set is the fp64 top-k set, everything else (t >= len
    included) is exactly 0, the NaN video's pattern is autograd's; grad_scale and the device scalar multiply."""
    lg, lens, tg, kinds, special = topk_batch(4, saturated=False)
    scale = grad_scale * (scale_dev if scale_dev is not None else 1.0)
    got = dev_loss_backward(lg, lens, tg, None, grad_scale=grad_scale, scale_dev=scale_dev, want=("logits",))["logits"]
    want, f32 = _clas2_grads(lg, lens, tg, scale, special)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == int(100 / 16 + 1)
    ok = ~np.isnan(want)
    assert np.array_equal((got != 0) & ok, (want != 0) & ok)
    for v in range(lg.shape[0]):
        assert (got[v, min(int(lens[v]), T):] == 0).all()
        if v != special["nan_in"]:
            assert np.count_nonzero(got[v]) == int(lens[v]) // 16 + 1
    fg = FloorGate()
    nn = np.array([v for v in range(lg.shape[0]) if v != special["nan_in"]])
    add_by_class(fg, "d_logits", f"{grad_scale},{scale_dev}", got[nn], want[nn], f32[nn], kinds[nn], VIDEO_KINDS)
    fg.check()


def test_topk_gradient_with_tied_scores():
    """One video with all logits equal, one with logits rounded to multiples of 0.5: torch.topk's choice among equals is its own, so
    the check is what every valid choice shares -- exactly k nonzeros, each at a score >= the k-th largest, each the value that index
    gets when selected (fp64; the top-k mean does not depend on the choice), and the per-video sum.  The gate is the untied videos'
    floor of the same call, k x it for the sum of k entries."""
    lg, lens, tg, kinds, special = topk_batch(5, saturated=False)
    rng = np.random.default_rng(6)
    tied = [lg.shape[0], lg.shape[0] + 1]
    lg = np.concatenate([lg, np.full((1, T), 0.75, np.float32), (np.round(2 * rng.uniform(-3, 3, (1, T))) / 2).astype(np.float32)])
    lens = np.concatenate([lens, np.array([100, 203], np.int32)])
    tg = np.concatenate([tg, np.array([1.0, 0.0], np.float32)])
    got = dev_loss_backward(lg, lens, tg, None, want=("logits",))["logits"]
    want, f32 = _clas2_grads(lg, lens, tg, 1.0, special)
    plain = np.array([v for v in range(lg.shape[0]) if v != special["nan_in"] and v not in tied and kinds[v] == 0])
    floor = float(np.abs(f32[plain].astype(np.float64) - want[plain]).max())
    B = lg.shape[0]
    for v in tied:
        n, k = int(lens[v]), int(lens[v]) // 16 + 1
        p = 1.0 / (1.0 + np.exp(-lg[v].astype(np.float64)))
        kth = np.sort(p[:n])[-k]
        pm = np.sort(p[:n])[-k:].mean()
        dp = (pm - float(tg[v])) / max((1 - pm) * pm, 1e-12) / B
        value = dp * p * (1 - p) / k
        nz = np.flatnonzero(got[v])
        assert nz.size == k and (nz < n).all() and (p[nz] >= kth).all()
        err = np.abs(got[v, nz] - value[nz]).max()
        serr = abs(got[v].astype(np.float64).sum() - want[v].sum())
        print(f"tied video {v}: k {k}  entry error {err:.3e}  sum error {serr:.3e}  floor {floor:.3e}")
        assert err <= FLOOR_FACTOR * floor and serr <= k * FLOOR_FACTOR * floor


# ------------------------------------------------------------------------------------------------------------------------
# 5. iefvad_loss_rows_grad_kernel
# ------------------------------------------------------------------------------------------------------------------------
def _head_grads(heads, dtype, noise, nu, lam, scale):
    x = [_t(h, dtype, True) for h in heads]
    (scale * ref_head_total(*x, noise, nu, lam)).backward()
    return [t.grad.numpy() for t in x]


@pytest.mark.parametrize("noise,nu", NOISES)
def test_row_gradients_whole_per_tensor_and_row_class(noise, nu):
    """The four gradient tensors [256, 768] against fp64 autograd through the trainers' lines, absolute floors per class and tensor
    (the identical-rows class is pure cancellation, the zero-row classes carry 1e12-scale values); weights (0.5, 0.25), grad_scale 3
    times a device scalar 0.5."""
    heads, cls = head_rows(50, T)
    lam = (0.5, 0.25)
    lg, lens, tg = np.zeros((1, T), np.float32), np.array([256], np.int32), np.array([1.0], np.float32)
    got = dev_loss_backward(lg, lens, tg, heads, noise, nu, lam, 3.0, 0.5, want=GRADS[1:])
    want = _head_grads(heads, torch.float64, noise, nu, lam, 1.5)
    f32 = _head_grads(heads, torch.float32, noise, nu, lam, 1.5)
    fg = FloorGate()
    for j, k in enumerate(GRADS[1:]):
        assert not np.isnan(got[k]).any() and not np.isnan(want[j]).any()
        add_by_class(fg, f"d_{k}", f"{noise},{nu}", got[k], want[j], f32[j], cls, ROW_CLASSES)
    fg.check()


def test_row_gradients_with_every_null_subset():
    """Each d_* pointer NULL alone and each present alone: what is written has the bits of the all-present call, at B = 2 so that
    more than one video's rows are in play; the guard bands of every written tensor stay intact (checked on read)."""
    heads, _ = head_rows(60, 2 * T)
    dh = [_dev(h) for h in heads]
    lg, lens, tg = np.zeros((2, T), np.float32), np.array([256, 100], np.int32), np.array([1.0, 0.0], np.float32)
    full = dev_loss_backward(lg, lens, tg, dh, "StudentT", 8.0, want=GRADS)
    for k in GRADS[1:]:
        for want in ((k,), tuple(q for q in GRADS[1:] if q != k)):
            got = dev_loss_backward(lg, lens, tg, dh, "StudentT", 8.0, want=want)
            for q in want:
                assert np.array_equal(_bits(got[q]), _bits(full[q])), (want, q)
    alone = dev_loss_backward(lg, lens, tg, None, "StudentT", 8.0, want=("logits",))
    assert np.array_equal(_bits(alone["logits"]), _bits(full["logits"]))


# ------------------------------------------------------------------------------------------------------------------------
# 6. AdamW
# ------------------------------------------------------------------------------------------------------------------------
HYPERS = (dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),           # the trainers' construction
          dict(lr=1e-2, betas=(0.5, 0.9), eps=1e-3, weight_decay=0.0))
STEPS = (1, 2, 1000, 100000)
ENTRY = ("plain", "g=0", "g=1e20", "g=nan")
ARENA_GUARD = 4096 + GUARD                       # a chunk of the multi-tensor kernel, so that one chunk too many still lands in a band


def adamw_state(seed, n, mag, step, special=True):
    """(p, g, m, v) and the entry class of every element.  g = mag N(0, 1) with scattered 0, 1e20 (g^2 overflows fp32) and NaN."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (mag * rng.standard_normal(n)).astype(np.float32)
    cls = np.zeros(n, np.int64)
    if not special:
        pass
    elif n >= 5:
        idx = rng.permutation(n)[:3 * max(1, n // 400)]
        for j in (1, 2, 3):
            cls[idx[j - 1::3]] = j
    elif n == 1:
        cls[0] = seed % 4
    g[cls == 1], g[cls == 2], g[cls == 3] = 0.0, 1e20, np.nan
    if step == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = (0.3 * mag * rng.standard_normal(n)).astype(np.float32)
        v = (mag * mag * (0.5 + rng.random(n))).astype(np.float32)
    return p, g, m, v, cls


def adamw_fp64(p, g, m, v, h, step):
    """The update restated in fp64, the host scalars in double."""
    p, g, m, v = (x.astype(np.float64) for x in (p, g, m, v))
    b1, b2 = h["betas"]
    with np.errstate(all="ignore"):
        p = p * (1.0 - h["lr"] * h["weight_decay"])
        m = m + (1.0 - b1) * (g - m)
        v = b2 * v + (1.0 - b2) * g * g
        denom = np.sqrt(v) / math.sqrt(1.0 - b2 ** step) + h["eps"]
        p = p - (h["lr"] / (1.0 - b1 ** step)) * (m / denom)
    return p, m, v


def adamw_torch(p, g, m, v, h, step):
    """torch.optim.AdamW(foreach=False) on the CPU in fp32 from the same state."""
    P = torch.from_numpy(p.copy()).requires_grad_(True)
    P.grad = torch.from_numpy(g.copy())
    opt = torch.optim.AdamW([P], foreach=False, **h)
    opt.state[P] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(m.copy()), exp_avg_sq=torch.from_numpy(v.copy()))
    opt.step()
    st = opt.state[P]
    return P.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def check_adamw(fg, name, tag, got, state, h, step):
    """got = (p, m, v) of the kernel.  Non-finite pattern == torch's; where torch's v overflowed (g = 1e20) the quotient m / denom is
    exactly 0, so p is the single rounding of p (1 - lr wd): bit-equal to torch's; everything else finite against fp64, floors per
    output and entry class."""
    p, g, m, v, cls = state
    if p.size == 0:
        return
    w64 = adamw_fp64(p, g, m, v, h, step)
    f32 = adamw_torch(p, g, m, v, h, step)
    over = ~np.isfinite(f32[2])
    for out, a, b, c in zip(("p", "exp_avg", "exp_avg_sq"), got, w64, f32):
        assert np.array_equal(np.isnan(a), np.isnan(c)) and np.array_equal(np.isinf(a), np.isinf(c)), (name, tag, out)
        fin = np.isfinite(c) & ~over if out == "p" else np.isfinite(c)
        add_by_class(fg, f"{out}/{name}", tag, a[fin], b[fin], c[fin], cls[fin], ENTRY)
    sel = over & ~np.isnan(f32[0])
    assert np.array_equal(_bits(got[0][sel]), _bits(f32[0][sel])), (name, tag)


def _hyper_args(h, step):
    return (float(h["lr"]), float(h["betas"][0]), float(h["betas"][1]), float(h["eps"]), float(h["weight_decay"]), int(step), _stream())


def dev_adamw_single(state, h, step):
    p, g, m, v, _ = state
    n = p.size
    P, M, V, G = Guarded(n, p), Guarded(n, m), Guarded(n, v), Guarded(n, g)
    rc = L.load_library().iefvad_adamw_step(P.ptr, G.ptr, M.ptr, V.ptr, n, *_hyper_args(h, step))
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(G.read()), _bits(g))
    return P.read(), M.read(), V.read()


def dev_adamw_multi(states, h, step):
    """All tensors in four arenas (param, grad, exp_avg, exp_avg_sq), a chunk-sized band of SENT before, between and behind them; the
    table is built as include/iefvad.h describes it (an empty tensor shares first_chunk with its successor)."""
    sizes = [s[0].size for s in states]
    off = np.cumsum([ARENA_GUARD] + [n + ARENA_GUARD for n in sizes])
    total = int(off[-1])
    arenas = []
    for q in range(4):
        a = np.full(total, SENT, np.float32)
        for s, o in zip(states, off):
            a[o:o + s[q].size] = s[q]
        arenas.append(a)
    dev = [_dev(a) for a in arenas]
    tab = np.zeros((len(states), 6), np.uint64)
    chunk = 0
    for i, (n, o) in enumerate(zip(sizes, off)):
        tab[i] = [dev[0].data_ptr() + 4 * int(o), dev[1].data_ptr() + 4 * int(o), dev[2].data_ptr() + 4 * int(o),
                  dev[3].data_ptr() + 4 * int(o), n, chunk]
        chunk += (n + 4095) // 4096
    assert all(tab[i, 5] == tab[i + 1, 5] for i, n in enumerate(sizes[:-1]) if n == 0)
    dtab = _dev(tab.view(np.int64))
    rc = L.load_library().iefvad_adamw_step_multi(_ptr(dtab), len(states), chunk, *_hyper_args(h, step))
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    host = [d.cpu().numpy() for d in dev]
    band = np.ones(total, bool)
    for n, o in zip(sizes, off):
        band[o:o + n] = False
    for q in (0, 2, 3):
        assert (host[q][band] == SENT).all(), "a write outside the tensors"
    assert np.array_equal(_bits(host[1]), _bits(arenas[1]))
    return [(host[0][o:o + n], host[2][o:o + n], host[3][o:o + n]) for n, o in zip(sizes, off)]


MAGS = (1e-3, 1.0, 1e3)
TABLE = (1, 4095, 4096, 4097, 8192, 0, 5, 12289)


@pytest.mark.parametrize("hi", (0, 1))
def test_adamw_single_tensor_entry(hi):
    """n in {1, 255, 256, 257} at every step count, and 1,048,576 + 259 (the grid is capped at 4096 x 256 threads: the grid-stride loop
    runs a second time) at steps 2 and 1000."""
    h = HYPERS[hi]
    fg = FloorGate()
    for i, n in enumerate((1, 255, 256, 257, 1048576 + 259)):
        for step in (STEPS if n < 1000 else (2, 1000)):
            for rep in range(16 if n == 1 else 1):           # a one-element tensor meets every entry class, four times each
                st = adamw_state(1000 * i + 100 * STEPS.index(step) + rep, n, MAGS[i % 3], step)
                check_adamw(fg, f"n={n}", f"h{hi},step={step},{rep}", dev_adamw_single(st, h, step), st, h, step)
    fg.check()


@pytest.mark.parametrize("hi", (0, 1))
def test_adamw_multi_tensor_entry_through_the_c_abi(hi):
    """count = 1, and the table [1, 4095, 4096, 4097, 8192, 0, 5, 12289]: chunk boundaries from both sides, an empty tensor, tensors of
    one, two and four chunks (the last one ragged)."""
    h = HYPERS[hi]
    fg = FloorGate()
    for step in STEPS:
        st = adamw_state(2000 + step, 4097, 1.0, step)
        check_adamw(fg, "count=1,n=4097", f"h{hi},step={step}", dev_adamw_multi([st], h, step)[0], st, h, step)
        sts = [adamw_state(3000 + 10 * i + STEPS.index(step), n, MAGS[i % 3], step) for i, n in enumerate(TABLE)]
        for i, (got, st) in enumerate(zip(dev_adamw_multi(sts, h, step), sts)):
            check_adamw(fg, f"table[{i}],n={TABLE[i]}", f"h{hi},step={step}", got, st, h, step)
    fg.check()


def _optimizer_on_arena(states, h, step):
    """losses.AdamW over parameters that are views into one guarded arena, its state preset to `step` - 1."""
    sizes = [s[0].size for s in states]
    off = np.cumsum([ARENA_GUARD] + [n + ARENA_GUARD for n in sizes])
    arena = np.full(int(off[-1]), SENT, np.float32)
    for s, o in zip(states, off):
        arena[o:o + s[0].size] = s[0]
    dev = _dev(arena)
    params = [dev[int(o):int(o) + n].requires_grad_(True) for n, o in zip(sizes, off)]
    opt = losses.AdamW(params, **h)
    for P, s in zip(params, states):
        if step > 1:
            opt.state[P] = dict(step=torch.tensor(float(step - 1)), exp_avg=_dev(s[2]), exp_avg_sq=_dev(s[3]))
    return dev, params, opt, off, sizes


def _read_optimizer(dev, params, opt, off, sizes, count=None):
    torch.cuda.synchronize()
    host = dev.detach().cpu().numpy()
    band = np.ones(host.size, bool)
    for n, o in zip(sizes, off):
        band[o:o + n] = False
    assert (host[band] == SENT).all(), "a write outside the parameters"
    return [(host[o:o + n].copy(), opt.state[P]["exp_avg"].cpu().numpy(), opt.state[P]["exp_avg_sq"].cpu().numpy())
            for P, n, o in list(zip(params, sizes, off))[:count]]


def test_adamw_optimizer_class_with_an_empty_parameter():
    """losses.AdamW on the table's sizes, the empty parameter included, both hyper-parameter sets at steps 1 and 1000."""
    fg = FloorGate()
    for hi, h in enumerate(HYPERS):
        for step in (1, 1000):
            sts = [adamw_state(4000 + 10 * i + step % 7, n, MAGS[i % 3], step) for i, n in enumerate(TABLE)]
            dev, params, opt, off, sizes = _optimizer_on_arena(sts, h, step)
            for P, s in zip(params, sts):
                P.grad = _dev(s[1])
            opt.step()
            for i, (got, st) in enumerate(zip(_read_optimizer(dev, params, opt, off, sizes), sts)):
                check_adamw(fg, f"opt[{i}],n={TABLE[i]}", f"h{hi},step={step}", got, st, h, step)
                assert int(opt.state[params[i]]["step"]) == step
    fg.check()


def test_adamw_optimizer_class_regrows_its_table_past_128_tensors():
    """130 small tensors.  The first step gives 8 of them a gradient (a 128-row table), the second all 130 (the table regrows): the
    other 122 start with a preset step count of 1, so that all share step 2 and the multi-tensor launch takes them."""
    h = HYPERS[0]
    sizes = [3 + (7 * i) % 61 for i in range(130)]
    s1 = [adamw_state(5000 + i, n, MAGS[i % 3], 1, special=False) for i, n in enumerate(sizes)]      # finite: its results are step 2's state
    dev, params, opt, off, sizes = _optimizer_on_arena(s1, h, 1)
    for i in range(8):
        params[i].grad = _dev(s1[i][1])
    opt.step()
    assert opt._table_host[params[0].device].shape[0] == 128
    first = _read_optimizer(dev, params, opt, off, sizes, count=8)
    fg = FloorGate()
    s2 = []
    for i, n in enumerate(sizes):
        nxt = adamw_state(6000 + i, n, MAGS[i % 3], 2)
        if i < 8:
            check_adamw(fg, f"step1,mag={MAGS[i % 3]:g}", f"t{i}", first[i], s1[i], h, 1)
            s2.append((first[i][0].copy(), nxt[1], first[i][1].copy(), first[i][2].copy(), nxt[4]))
        else:
            opt.state[params[i]] = dict(step=torch.tensor(1.0), exp_avg=_dev(nxt[2]), exp_avg_sq=_dev(nxt[3]))
            s2.append((s1[i][0], nxt[1], nxt[2], nxt[3], nxt[4]))
        params[i].grad = _dev(nxt[1])
    opt.step()
    assert opt._table_host[params[0].device].shape[0] >= 130
    for i, (got, st) in enumerate(zip(_read_optimizer(dev, params, opt, off, sizes), s2)):
        check_adamw(fg, f"step2,mag={MAGS[i % 3]:g}", f"t{i}", got, st, h, 2)
    fg.check()


# ------------------------------------------------------------------------------------------------------------------------
# 7. iefvad_nan_rule
# ------------------------------------------------------------------------------------------------------------------------
def dev_nan_rule(a, b, n):
    A, Bq = Guarded(a.size, a), Guarded(b.size, b)
    flags = torch.full((2 + 2 * 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rc = L.load_library().iefvad_nan_rule(A.ptr, Bq.ptr, n, C.c_void_p(flags.data_ptr() + 8), _stream())
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    f = flags.cpu().numpy()
    assert (f[:2] == 0x5A5A5A5A).all() and (f[4:] == 0x5A5A5A5A).all()
    return A.read(), Bq.read(), f[2:4].tolist()


def _nan_to_num(x):
    return torch.nan_to_num(torch.from_numpy(x.copy()), nan=0.0).numpy()


def test_nan_rule_beyond_one_grid_pass_and_at_the_smallest_sizes():
    """n = 4 (524,288 + 257) floats: the scan's and the repair's grid covers 524,288 float4s, so the only NaN, in the last element,
    is met in the stride loop's second pass.  The tensor with the NaN comes out as torch.nan_to_num(x, nan=0.0) bit for bit, the clean
    one (which carries +-inf) unchanged; the same with the roles swapped; n = 4 and n = 0."""
    rng = np.random.default_rng(70)
    n = 4 * (524288 + 257)
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    for x in (a, b):
        x[rng.integers(0, n - 1, 64)] = np.inf
        x[rng.integers(0, n - 1, 64)] = -np.inf
        x[rng.integers(0, n - 1, 64)] = -0.0
    a[n - 1] = np.nan
    for swapped in (False, True):
        ga, gb, flags = dev_nan_rule(*((b, a) if swapped else (a, b)), n)
        if swapped:
            ga, gb, flags = gb, ga, flags[::-1]
        assert flags == [1, 0]
        assert np.array_equal(_bits(ga), _bits(_nan_to_num(a))) and ga[n - 1] == 0 and not np.isinf(ga).any()
        assert np.array_equal(_bits(gb), _bits(b)) and np.isinf(gb).any()
    four = np.array([np.inf, np.nan, -np.inf, -0.0], np.float32)
    clean = np.array([np.inf, 1.0, -np.inf, -0.0], np.float32)
    ga, gb, flags = dev_nan_rule(four, clean, 4)
    assert flags == [1, 0] and np.array_equal(_bits(ga), _bits(_nan_to_num(four))) and np.array_equal(_bits(gb), _bits(clean))
    ga, gb, flags = dev_nan_rule(clean, four, 4)
    assert flags == [0, 1] and np.array_equal(_bits(gb), _bits(_nan_to_num(four))) and np.array_equal(_bits(ga), _bits(clean))
    ga, gb, flags = dev_nan_rule(four, four, 0)
    assert flags == [0, 0] and np.array_equal(_bits(ga), _bits(four)) and np.array_equal(_bits(gb), _bits(four))
