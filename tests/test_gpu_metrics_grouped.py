"""`iefvad_auc_ap_grouped` (csrc/metrics.h): ROC-AUC and AP of up to 64 disjoint groups of snippets in one pass -- the per-class loops
and the Ano-AUC of the reference's test() (test.py:161,165-174) -- against sklearn's roc_auc_score / average_precision_score on
np.repeat of each group's scores, at the gate of tests/test_gpu_metrics.py (1e-12).  Everything goes through the C ABI.  `-m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch
from sklearn.metrics import average_precision_score, roc_auc_score

from iefvad_amd import lib as L

pytestmark = pytest.mark.gpu

TILE = 4096                 # pairs per workgroup of the sort and the scans (MT_TILE)
NONE = 255


def grouped(scores, gt, group, ngroups, repeat=16):
    """(auc [ngroups], ap [ngroups], frames [ngroups, 2]) of one library call; the outputs start from a sentinel."""
    lib = L.load_library()
    s = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).cuda()
    g = torch.from_numpy((np.asarray(gt) != 0).astype(np.uint8)).cuda()
    grp = torch.from_numpy(np.ascontiguousarray(group, dtype=np.uint8)).cuda()
    n = s.numel()
    ws = torch.empty(lib.iefvad_auc_ap_grouped_workspace_bytes(n, ngroups) + 256, dtype=torch.uint8, device="cuda")
    off = (-ws.data_ptr()) % 256
    out = torch.full((2 * ngroups,), -7.0, dtype=torch.float64, device="cuda")
    frames = torch.full((2 * ngroups,), -7, dtype=torch.int64, device="cuda")
    rc = lib.iefvad_auc_ap_grouped(C.c_void_p(s.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(grp.data_ptr()), n, repeat, ngroups,
                                   C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 8 * ngroups), C.c_void_p(frames.data_ptr()),
                                   C.c_void_p(ws.data_ptr() + off), ws.numel() - off, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.last_error()
    o = out.cpu().numpy()
    return o[:ngroups].copy(), o[ngroups:].copy(), frames.cpu().numpy().reshape(ngroups, 2)


def ungrouped(scores, gt, repeat=16):
    lib = L.load_library()
    s = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).cuda()
    g = torch.from_numpy((np.asarray(gt) != 0).astype(np.uint8)).cuda()
    n = s.numel()
    ws = torch.empty(lib.iefvad_auc_ap_workspace_bytes(n) + 256, dtype=torch.uint8, device="cuda")
    off = (-ws.data_ptr()) % 256
    out = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    rc = lib.iefvad_auc_ap(C.c_void_p(s.data_ptr()), C.c_void_p(g.data_ptr()), n, repeat, C.c_void_p(out.data_ptr()),
                           C.c_void_p(out.data_ptr() + 8), C.c_void_p(ws.data_ptr() + off), ws.numel() - off,
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.last_error()
    return out.cpu().numpy()


def members(group, g, repeat=16):
    """snippet mask of group g and the matching frame mask"""
    m = np.asarray(group) == g
    return m, np.repeat(m, repeat)


def sk_group(scores, gt, group, g, repeat=16):
    m, fm = members(group, g, repeat)
    y = np.repeat(np.asarray(scores, dtype=np.float32)[m], repeat)
    return roc_auc_score(gt[fm], y), average_precision_score(gt[fm], y)


def check_against_sklearn(scores, gt, group, ngroups, got, repeat=16, only=None):
    auc, ap, frames = got
    for g in (range(ngroups) if only is None else only):
        m, fm = members(group, g, repeat)
        assert frames[g, 0] == repeat * int(m.sum()) and frames[g, 1] == int((gt[fm] != 0).sum()), g
        if not m.any():
            assert np.isnan(auc[g]) and np.isnan(ap[g]), g
            continue
        a0, p0 = sk_group(scores, gt, group, g, repeat)
        assert abs(auc[g] - a0) < 1e-12 and abs(ap[g] - p0) < 1e-12, (g, auc[g] - a0, ap[g] - p0)


def group_sizes(n, ngroups, rng):
    """Sizes of groups 0 .. ngroups-1 and of the snippets of no group, adding up to n: group 0 takes exactly one tile where n allows
    (its end is a tile boundary of the sorted order), group 1 a single snippet, groups 2 .. 4 a handful each (one tile holds more than
    two groups), about a tenth of the snippets belong to no group, the rest is spread unevenly; small n leave groups empty."""
    sizes = np.zeros(ngroups, np.int64)
    left = n
    none = n // 10
    left -= none
    if left > TILE:
        sizes[0] = TILE
    elif ngroups == 1:
        sizes[0] = left
    else:
        sizes[0] = (left + 1) // 2
    left -= sizes[0]
    for g, want in ((1, 1), (2, 5), (3, 7), (4, 11)):
        if g < ngroups and left > 0:
            sizes[g] = min(want, left)
            left -= sizes[g]
    if ngroups > 5 and left > 0:
        extra = rng.multinomial(left, rng.dirichlet(np.full(ngroups - 5, 0.5)))
        sizes[5:] += extra
        left = 0
    return sizes, none + left


def make_case(n, ngroups, quant):
    """scores, gt (correlated with the score, as in tests/test_gpu_metrics.py), group bytes in shuffled snippet order.  Every
    non-empty group gets one positive and one negative frame, so sklearn accepts each of them."""
    rng = np.random.default_rng([n, ngroups, quant or 0])
    s = rng.random(n).astype(np.float32)
    if quant:
        s = (np.round(s * quant) / quant).astype(np.float32)
    gt = (rng.random(16 * n) < 0.15 + 0.5 * np.repeat(s, 16)).astype(np.float64)
    sizes, none = group_sizes(n, ngroups, rng)
    assert sizes.sum() + none == n
    group = np.concatenate([np.repeat(np.arange(ngroups), sizes), np.full(none, NONE)]).astype(np.uint8)
    group[group == NONE] = rng.choice([NONE, NONE, 200, ngroups], size=none)          # any byte >= ngroups means "no group"
    rng.shuffle(group)
    for g in range(ngroups):
        idx = np.flatnonzero(group == g)
        if idx.size:
            gt[16 * idx[0]], gt[16 * idx[0] + 1] = 1.0, 0.0
    return s, gt, group, sizes


@pytest.mark.parametrize("quant", [None, 8])
@pytest.mark.parametrize("ngroups", [1, 3, 14, 64])
@pytest.mark.parametrize("n", [1, 63, 4095, 4096, 4097, 12289, 30000])
def test_grouped_equals_sklearn_per_group(n, ngroups, quant):
    s, gt, group, sizes = make_case(n, ngroups, quant)
    if n > 2 * TILE:
        assert sizes[0] == TILE                         # group 0 ends exactly on a tile boundary of the sorted order
        if ngroups >= 5:
            assert sizes[1] == 1 and sizes[1:5].sum() < TILE          # a single-snippet group; four groups inside one tile
        assert (group >= ngroups).any()
    check_against_sklearn(s, gt, group, ngroups, grouped(s, gt, group, ngroups))


def test_one_tie_never_spans_two_groups():
    """Every score of every group is 0.5: each group is ONE tie group, so its AUC is exactly 1/2 and its AP its own prevalence."""
    rng = np.random.default_rng(11)
    n, ngroups = 10000, 5
    group = rng.choice([0, 1, 2, 3, 4, NONE], size=n, p=[0.3, 0.05, 0.25, 0.1, 0.2, 0.1]).astype(np.uint8)
    prevalence = np.array([0.1, 0.5, 0.2, 0.8, 0.3, 0.6])[np.minimum(group, 5)]
    gt = (rng.random(16 * n) < np.repeat(prevalence, 16)).astype(np.float64)
    auc, ap, frames = grouped(np.full(n, 0.5, np.float32), gt, group, ngroups)
    for g in range(ngroups):
        _, fm = members(group, g)
        assert auc[g] == 0.5, (g, auc[g])
        assert abs(ap[g] - gt[fm].mean()) < 1e-15, (g, ap[g] - gt[fm].mean())
        assert frames[g, 0] == fm.sum() and frames[g, 1] == gt[fm].sum()


def test_degenerate_groups_leave_the_others_alone():
    """An empty group, one without a positive frame, one with positive frames only and one with a NaN score, all in one call with two
    ordinary groups: the ordinary ones equal sklearn, the others give what iefvad_auc_ap gives for such input."""
    rng = np.random.default_rng(12)
    n, ngroups = 9000, 6
    s = (np.round(rng.random(n) * 500) / 500).astype(np.float32)
    group = rng.choice([0, 2, 3, 4, 5, NONE], size=n).astype(np.uint8)          # group 1 stays empty
    gt = (rng.random(16 * n) < 0.1 + 0.6 * np.repeat(s, 16)).astype(np.float64)
    gt[members(group, 2)[1]] = 0.0
    gt[members(group, 3)[1]] = 1.0
    clean = s.copy()
    s[np.flatnonzero(group == 4)[17]] = np.nan
    got = grouped(s, gt, group, ngroups)
    auc, ap, frames = got
    check_against_sklearn(clean, gt, group, ngroups, got, only=(0, 5))
    assert np.isnan(auc[1]) and np.isnan(ap[1]) and tuple(frames[1]) == (0, 0)
    assert np.isnan(auc[2]) and ap[2] == 0.0 and frames[2, 1] == 0 and frames[2, 0] == 16 * (group == 2).sum()
    assert np.isnan(auc[3]) and abs(ap[3] - 1.0) < 1e-15 and frames[3, 0] == frames[3, 1] == 16 * (group == 3).sum()
    assert np.isnan(auc[4]) and np.isnan(ap[4]) and frames[4, 0] == 16 * (group == 4).sum()
    # a NaN among the snippets of NO group spoils nothing
    s = clean.copy()
    s[np.flatnonzero(group == NONE)[3]] = np.nan
    check_against_sklearn(clean, gt, group, ngroups, grouped(s, gt, group, ngroups), only=(0, 4, 5))


@pytest.mark.parametrize("n", [4097, 30000])
def test_one_group_of_everything_is_the_ungrouped_call(n):
    """ngroups = 1, every byte 0: both AUC numerators are exact integers over the same pairs, so the AUC has the same BITS as
    iefvad_auc_ap's; the AP sums the same terms and may differ in how the partials are grouped."""
    rng = np.random.default_rng(n)
    s = (np.round(rng.random(n) * 300) / 300).astype(np.float32)
    gt = (rng.random(16 * n) < 0.15 + 0.5 * np.repeat(s, 16)).astype(np.float64)
    auc, ap, frames = grouped(s, gt, np.zeros(n, np.uint8), 1)
    a0, p0 = ungrouped(s, gt)
    assert auc[0].tobytes() == a0.tobytes()
    assert abs(ap[0] - p0) < 1e-12
    assert tuple(frames[0]) == (16 * n, int(gt.sum()))


def test_snippet_order_does_not_matter_and_runs_repeat_their_bits():
    s, gt, group, _ = make_case(12289, 14, 8)
    first = grouped(s, gt, group, 14)
    again = grouped(s, gt, group, 14)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    perm = np.random.default_rng(13).permutation(s.size)
    auc, ap, frames = grouped(s[perm], gt.reshape(-1, 16)[perm].reshape(-1), group[perm], 14)
    assert auc.tobytes() == first[0].tobytes()          # exact integer numerators: no summation order to depend on
    assert np.array_equal(frames, first[2])
    assert np.abs(ap - first[1]).max() < 1e-12


def test_signed_tiny_and_saturated_scores_over_five_groups():
    """The scores of test_auc_ap_on_signed_tiny_and_saturated_scores (negative values, +-0 as one threshold, denormals, saturated 0 / 1,
    then +-inf) spread over five groups; repeat factors 1 and 20 on the finite case."""
    rng = np.random.default_rng(0)
    n = 30000
    s = rng.standard_normal(n).astype(np.float32)
    s[::5] = 1.0
    s[1::5] = 0.0
    s[2::50] = -0.0
    s[3::70] = 1e-42
    s[4::90] = -1e-42
    gt = (rng.random(16 * n) < 0.3).astype(np.float64)
    group = rng.integers(0, 5, n).astype(np.uint8)
    check_against_sklearn(s, gt, group, 5, grouped(s, gt, group, 5))
    for repeat in (1, 20):
        gtr = (rng.random(repeat * n) < 0.3).astype(np.float64)
        check_against_sklearn(s, gtr, group, 5, grouped(s, gtr, group, 5, repeat), repeat=repeat)
    # +-inf (sklearn refuses them): they must rank above / below every finite score, i.e. like +-3e38 stand-ins
    s[7::1000] = np.inf
    s[9::1000] = -np.inf
    stand_in = np.where(np.isinf(s), np.sign(s) * np.float32(3e38), s)
    check_against_sklearn(stand_in, gt, group, 5, grouped(s, gt, group, 5))
