"""The noise study's row perturbations (`iefvad_perturb`, include/iefvad.h; `MMFMIL.forward(row_noise=)`, `forward_videos(row_noise=)`,
`iefvad_amd.perturb_rows`; `harness.PerturbationSweep.level(noise_sigma_*=, outlier_*=, dropout_prob=)`) -- what can be checked without a
GPU.  The reference declares the study's flags and implements none of them (test2.py:35-37,214-220), so nothing here is a parity test
("parity unpinned"): the host model of the generator against a scalar restatement of its formula and against the moments of a standard
normal, the row-vector builders against per-video loops, the sweep's consumption of torch's RNG, the CPU plumbing path against a by-hand
perturbed copy, and the bindings and refusals that need no device."""
import argparse
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth
from iefvad_amd import lib as L
from oracle import iefvad_oracle as orc

M32 = 0xFFFFFFFF


def _fmix32(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    return x ^ (x >> 16)


def _bits(seed, idx):
    """csrc/common.h dropout_bits, one value at a time in Python integers"""
    a = _fmix32((idx & M32) ^ (seed & M32))
    return _fmix32((a + (seed >> 32) + (idx >> 32) * 0x9E3779B1) & M32) >> 8


def _eps_scalar(seed, m, rid, d):
    """The issue's formula for one element, written as a loop body would be"""
    q = d // 2
    idx = ((rid * 2 + m) << 11) | (q << 1)
    u1 = (_bits(seed, idx) + 1) * 2.0 ** -24
    u2 = _bits(seed, idx | 1) * 2.0 ** -24
    rho = math.sqrt(-2.0 * math.log(u1))
    v = rho * (math.cos(2.0 * math.pi * u2) if d % 2 == 0 else math.sin(2.0 * math.pi * u2))
    return np.float32(v)


@pytest.mark.parametrize("seed", [1234, 7, 0x9E3779B97F4A7C15])
def test_gaussian_rows_equals_the_scalar_formula(seed):
    ids = [0, 5, 2 ** 31 - 1]          # the last id pushes the index past 32 bits: the generator's `hi` word
    for m in (0, 1):
        got = harness.gaussian_rows(seed, m, ids, 16)
        assert got.dtype == np.float32 and got.shape == (3, 16)
        want = np.array([[_eps_scalar(seed, m, r, d) for d in range(16)] for r in ids], dtype=np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (seed, m)


def normal_statistics(e0, e1):
    """The statistics the generator is held to, each as (name, value, expectation, standard error) for a standard normal sample `e0`
    [rows, D] of one modality and `e1` of the other: four moments, and the correlations across modalities, columns (lag 1, 2) and rows."""
    e0, e1 = e0.astype(np.float64), e1.astype(np.float64)
    n = e0.size
    out = [("mean", e0.mean(), 0.0, 1 / math.sqrt(n)), ("variance", (e0 ** 2).mean(), 1.0, math.sqrt(2 / n)),
           ("third moment", (e0 ** 3).mean(), 0.0, math.sqrt(15 / n)), ("fourth moment", (e0 ** 4).mean(), 3.0, math.sqrt(96 / n)),
           ("modalities", (e0 * e1).mean(), 0.0, 1 / math.sqrt(n))]
    for name, a, b in (("column lag 1", e0[:, :-1], e0[:, 1:]), ("column lag 2", e0[:, :-2], e0[:, 2:]), ("row lag 1", e0[:-1], e0[1:])):
        out.append((name, (a * b).mean(), 0.0, 1 / math.sqrt(a.size)))
    return out


def test_gaussian_rows_has_the_moments_of_a_standard_normal():
    """Seed 1234, rows 0..1023, D = 768: every statistic within 4 standard errors (measured on the model: within 1.5)."""
    e0 = harness.gaussian_rows(1234, 0, np.arange(1024), 768)
    e1 = harness.gaussian_rows(1234, 1, np.arange(1024), 768)
    assert np.abs(e0).max() <= math.sqrt(48 * math.log(2))
    for name, got, want, se in normal_statistics(e0, e1):
        print(f"{name}: {got:+.6f} (expect {want}, {abs(got - want) / se:.2f} standard errors)")
        assert abs(got - want) < 4 * se, name
    assert not np.array_equal(e0, e1)
    assert not np.array_equal(e0, harness.gaussian_rows(1235, 0, np.arange(1024), 768))


LENGTHS = [1, 37, 256, 257, 300, 700]
T = 256


def _plans(seed, k_att, k_out, drops):
    gen = torch.Generator().manual_seed(seed)
    plans = []
    for v, _ in enumerate(LENGTHS):
        pick = lambda k: torch.randperm(T, generator=gen)[:k] if k else None
        plans.append(((pick(k_att[0]), pick(k_att[1])), (pick(k_out[0]), pick(k_out[1])), drops[v]))
    return plans


@pytest.mark.parametrize("k_att,k_out,sig,drops", [
    ((51, 0), (0, 25), (0.2, 0.0), [None, 0, 1, None, 0, 1]),
    ((0, 0), (0, 0), (0.0, 0.3), [None] * 6),
    ((12, 128), (25, 25), (0.0, 0.0), [1, 1, 0, 0, None, None]),
    ((0, 0), (0, 0), (0.0, 0.0), [None, None, 0, None, None, None]),
])
def test_row_vector_builders_equal_per_video_loops(k_att, k_out, sig, drops):
    plans = _plans(11, k_att, k_out, drops)
    nch = [n // T + 1 if n >= T else 1 for n in LENGTHS]           # process_split's chunk counts (tools.py:105-112)
    first = np.concatenate([[0], np.cumsum(LENGTHS)])[:-1]
    osig = 3.0
    sc_p, amp_p, ids_p = harness.sweep_row_perturbation(LENGTHS, plans, T, sig, osig)
    sc_d, amp_d, ids_d = harness.sweep_row_perturbation(LENGTHS, plans, T, sig, osig, nch, first)
    assert ids_p is None
    for m in (0, 1):
        want_s, want_a, pad_s, pad_a, pad_i = [], [], [], [], []
        for v, n in enumerate(LENGTHS):
            att, out, drop = plans[v]
            for r in range(nch[v] * T):
                t, valid = r % T, r < n
                s = 0.01 if att[m] is not None and t in att[m].tolist() else 1.0
                if drop == m and valid:
                    s = 0.0
                a = osig if out[m] is not None and t in out[m].tolist() else sig[m]
                if not valid:
                    a = 0.0
                pad_s.append(s); pad_a.append(a); pad_i.append(first[v] + r if valid else 0)
                if valid:
                    want_s.append(s); want_a.append(a)
        has_s = k_att[m] > 0 or any(d == m for d in drops)
        has_a = sig[m] != 0 or k_out[m] > 0
        for got, dense, want, wdense, has in ((sc_p[m], sc_d[m], want_s, pad_s, has_s), (amp_p[m], amp_d[m], want_a, pad_a, has_a)):
            if not has:
                assert got is None and dense is None
                continue
            assert got.dtype == torch.float32 and got.is_contiguous() and dense.is_contiguous()
            assert torch.equal(got, torch.tensor(want, dtype=torch.float32))
            assert torch.equal(dense, torch.tensor(wdense, dtype=torch.float32))
    if any(s != 0 for s in sig) or any(k_out):
        assert ids_d.dtype == torch.int32 and torch.equal(ids_d, torch.tensor(pad_i, dtype=torch.int32))
    else:
        assert ids_d is None


def _tiny_sweep(D=32, Tt=16, lengths=(1, 5, 16, 17, 40)):
    """A CPU sweep over a tiny list with the oracle as the model: T = 16, D = 32, one layer, one refinement step"""
    sd = synth.make_state_dict(3, D=D, num_layers=1, num_steps=1)
    model = orc.OracleMMFMIL(sd, orc.OracleConfig(num_layers=1, num_heads=8, num_refinement_steps=1))
    items = []
    for i, n in enumerate(lengths):
        img, ev = synth.make_video(4, i, n, D=D)
        ci, _ = harness.process_split(img, Tt)
        ce, _ = harness.process_split(ev, Tt)
        items.append((torch.tensor(ci).unsqueeze(0), torch.tensor(ce).unsqueeze(0), ("Normal",), torch.tensor([n])))
    gt = synth.make_gt(4, sum(lengths))
    sweep = harness.PerturbationSweep(argparse.Namespace(visual_length=Tt), model, iter(items), gt, "cpu", batch_chunks=3)
    return sweep, model, items, list(lengths), Tt, D


def test_legacy_level_consumes_torchs_rng_as_before():
    """After `level(0.1, 0)` torch's RNG stands where the reference's draws leave it: one `randperm(T)` per video, nothing for the event
    modality, no seed draw.  With the study's levels: the seed first, then per video attenuation, outliers, the drop draw."""
    sweep, _, _, lengths, Tt, _ = _tiny_sweep()
    sweep.clean()
    torch.manual_seed(5)
    sweep.level(0.1, 0)
    got = torch.get_rng_state()
    torch.manual_seed(5)
    for _ in lengths:
        torch.randperm(Tt)
    assert torch.equal(got, torch.get_rng_state())
    torch.manual_seed(5)
    sweep.level(0.1, 0, noise_sigma_ev=0.2, outlier_img=0.25, dropout_prob=0.5)
    got = torch.get_rng_state()
    torch.manual_seed(5)
    torch.randint(0, 2 ** 63 - 1, (1,))
    for _ in lengths:
        torch.randperm(Tt); torch.randperm(Tt); torch.rand(2)
    assert torch.equal(got, torch.get_rng_state())
    torch.manual_seed(5)
    sweep.level(0, 0, dropout_prob=0.5, noise_seed=3)           # a drop alone draws no seed
    got = torch.get_rng_state()
    torch.manual_seed(5)
    for _ in lengths:
        torch.rand(2)
    assert torch.equal(got, torch.get_rng_state())


def test_cpu_plumbing_level_equals_the_forward_of_a_hand_perturbed_copy():
    """All three kinds at once on the CPU path: the level's per-snippet probabilities equal the oracle's on a copy perturbed here, video
    by video with plain indexing, from the same draws and `gaussian_rows`."""
    sweep, model, items, lengths, Tt, D = _tiny_sweep()
    seed, sig_ev, rho, osig, p = 99, 0.2, 0.25, 3.0, 0.6
    torch.manual_seed(3)
    res = sweep.level(0.1, 0, noise_sigma_ev=sig_ev, outlier_img=rho, outlier_sigma=osig, dropout_prob=p, noise_seed=seed)
    torch.manual_seed(3)
    probs, first, dropped = [], 0, 0
    for (img, ev, _, _), n in zip(items, lengths):
        att = torch.randperm(Tt)[:int(Tt * 0.1)]
        out = torch.randperm(Tt)[:int(Tt * rho)]
        u = torch.rand(2)
        drop = (0 if u[1] < 0.5 else 1) if u[0] < p else None
        dropped += drop is not None
        x = [torch.nan_to_num(img.squeeze(0)).reshape(-1, Tt, D).clone(), torch.nan_to_num(ev.squeeze(0)).reshape(-1, Tt, D).clone()]
        x[0][:, att] = x[0][:, att] * 0.01                          # test2.py:73
        ids = np.arange(first, first + n)
        for m in (0, 1):
            flat = x[m].reshape(-1, D)
            if drop == m:
                flat[:n] = flat[:n] * 0.0
            amp = torch.full((n,), sig_ev if m == 1 else 0.0)
            if m == 0:
                amp[[r for r in range(n) if r % Tt in out.tolist()]] = osig
            eps = torch.from_numpy(harness.gaussian_rows(seed, m, ids, D))
            rows = amp != 0
            flat[:n][rows] = flat[:n][rows] + amp[rows, None] * eps[rows]
        o = model(x[0], x[1], None, None, None)
        probs.append(torch.sigmoid(o["logits"].reshape(-1)[:n]).float())
        first += n
    assert 0 < dropped < len(lengths)                               # the seed exercises both outcomes of the drop draw
    want = torch.cat(probs)
    brier = float(((want.double()[:, None] - sweep.gt) ** 2).mean())
    assert abs(res.brier - brier) < 2e-6                            # the suite's CPU gate (tests/test_harness_cpu.py): batches differ in composition
    again = sweep.level(0.1, 0)                                     # and the study's levels at 0 are the legacy level
    assert abs(again.brier - res.brier) > 1e-6


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        L.build_library()
    return L.load_library()


def test_entries_exist_and_are_bound(lib):
    for s in ("iefvad_forward_perturbed", "iefvad_forward_videos_perturbed", "iefvad_perturb_rows"):
        assert s in L.SYMBOLS and hasattr(lib, s) and getattr(lib, s).restype is C.c_int
    assert len(lib.iefvad_forward_perturbed.argtypes) == 10 and lib.iefvad_forward_perturbed.argtypes[5] is C.POINTER(L.Perturb)
    assert len(lib.iefvad_forward_videos_perturbed.argtypes) == 15 and lib.iefvad_forward_videos_perturbed.argtypes[7] is C.POINTER(L.Perturb)
    assert len(lib.iefvad_perturb_rows.argtypes) == 10 and lib.iefvad_perturb_rows.argtypes[6] is C.POINTER(L.Perturb)
    assert C.sizeof(L.Perturb) == 6 * C.sizeof(C.c_void_p)         # two scales, two amplitudes, the ids, the seed
    assert lib.iefvad_abi_version() == 8 and L.ABI_VERSION == 8     # entries were added, no struct changed


def test_refusals_before_any_launch_name_the_entry(lib):
    ok = C.c_void_p(0x10000)                                        # never read: the calls stop in their checks
    lens = (C.c_int32 * 2)(5, 7)
    p = L.Perturb()
    calls = {
        "iefvad_forward_perturbed": [
            lambda: lib.iefvad_forward_perturbed(None, ok, ok, L.IN_F32, 1, C.byref(p), ok, 1 << 30, None, None),
            lambda: lib.iefvad_forward_perturbed(ok, ok, ok, L.IN_F32, 1, None, ok, 1 << 30, None, None)],
        "iefvad_forward_videos_perturbed": [
            lambda: lib.iefvad_forward_videos_perturbed(ok, ok, ok, L.IN_F32, lens, 2, 2, None, ok, 1 << 30, ok, None, None, None, None),
            lambda: lib.iefvad_forward_videos_perturbed(None, ok, ok, L.IN_F32, lens, 2, 2, C.byref(p), ok, 1 << 30, ok, None, None, None, None)],
        "iefvad_perturb_rows": [
            lambda: lib.iefvad_perturb_rows(ok, ok, L.IN_F32, 768, 4, 0, None, ok, ok, None),
            lambda: lib.iefvad_perturb_rows(ok, ok, 7, 768, 4, 0, C.byref(p), ok, ok, None),
            lambda: lib.iefvad_perturb_rows(ok, ok, L.IN_F32, 640, 4, 0, C.byref(p), ok, ok, None),
            lambda: lib.iefvad_perturb_rows(None, ok, L.IN_F32, 768, 4, 0, C.byref(p), ok, ok, None),
            lambda: lib.iefvad_perturb_rows(ok, ok, L.IN_F32, 768, 0, 0, C.byref(p), ok, ok, None)],
    }
    for name, fs in calls.items():
        for f in fs:
            assert f() != 0
            assert L.last_error().startswith(name + ":"), L.last_error()
    bad = L.Perturb()
    bad.noise_amp[1] = 0x10002
    assert lib.iefvad_perturb_rows(ok, ok, L.IN_F32, 768, 4, 0, C.byref(bad), ok, ok, None) != 0
    assert "4-byte aligned" in L.last_error()
    assert lib.iefvad_forward_perturbed(ok, ok, ok, L.IN_F32, 1, C.byref(bad), ok, 1 << 30, None, None) != 0
    assert "4-byte aligned" in L.last_error()


def test_python_layers_validate_the_noise_arguments_before_loading_the_library(monkeypatch):
    args = argparse.Namespace(visual_layers=1, visual_head=8, num_refinement_steps=1, lambda_ref=0.5, noise_model="StudentT", nu=8)
    model = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 1, 8, 10, 10, "cuda", args).eval()

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "load_library", no_load)
    rows, amp, ids = torch.zeros(12, 768), torch.ones(12), torch.arange(12, dtype=torch.int32)
    fv = lambda **kw: model.forward_videos(rows, rows, [5, 7], **kw)
    with pytest.raises(ValueError, match="noise_seed"):
        fv(row_noise=(amp, None))
    with pytest.raises(ValueError, match="row_noise"):
        fv(row_noise=(amp[:-1], None), noise_seed=1)
    with pytest.raises(ValueError, match="row_noise"):
        fv(row_noise=(None, amp.double()), noise_seed=1)
    with pytest.raises(ValueError, match="row_noise"):
        fv(row_noise=(amp,), noise_seed=1)
    with pytest.raises(ValueError, match="noise_rows"):
        fv(row_noise=(amp, None), noise_seed=1, noise_rows=ids.long())
    with pytest.raises(ValueError, match="noise_rows"):
        fv(noise_rows=ids)
    for kw in (dict(similarity=True), dict(outputs="full"), dict(attn_maps=True)):
        with pytest.raises(ValueError, match="does not combine"):
            fv(row_noise=(amp, None), noise_seed=1, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fv(row_noise=(amp, amp), noise_seed=1, noise_rows=ids, nan_to_num="always", weight_sums=True)
    x = torch.zeros(1, 256, 768)
    a = torch.ones(256)
    with pytest.raises(ValueError, match="noise_seed"):
        model(x, x, row_noise=(a, None))
    for kw in (dict(timed=True), dict(attn_maps=True)):
        with pytest.raises(ValueError, match="does not combine"):
            model(x, x, row_noise=(a, None), noise_seed=1, **kw)
    with pytest.raises(ValueError, match="does not combine"):
        model(x.clone().requires_grad_(), x, row_noise=(a, None), noise_seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(x, x, row_noise=(a, None), noise_seed=1)
    with pytest.raises(ValueError, match="perturb_rows"):
        iefvad_amd.perturb_rows(None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        iefvad_amd.perturb_rows(rows, None, row_noise=(amp, None), noise_seed=1)
    with pytest.raises(TypeError):                                  # the host list takes no perturbation
        model.forward_videos_host([rows], [rows], [12], row_noise=(amp, None), noise_seed=1)


def test_noise_plan_lists_the_six_levels_per_kind():
    plan = harness.noise_plan()
    assert len(plan) == 5 * len(harness.SWEEP_LEVELS)
    assert [kw for name, kw in plan if name == "EV_GAUSS"] == [{"noise_sigma_ev": s} for s in harness.SWEEP_LEVELS]
    assert {name for name, _ in plan} == {"IMG_GAUSS", "EV_GAUSS", "IMG_OUTLIER", "EV_OUTLIER", "MODALITY_DROP"}
    assert len(harness.sweep_plan()) == 12
