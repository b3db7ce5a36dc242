"""The similarity series on the valid-row routes (`iefvad_forward_videos_similarity`, `iefvad_forward_videos_host_similarity`,
csrc/similarity.h; `MMFMIL.forward_videos(similarity=True)`; `harness.score_loader(similarity="rows")`; `vis_route="rows"`) -- what can
be checked without a GPU: the two entries exist and refuse bad arguments by name before the first HIP call, and the Python layers
validate their arguments; the default `vis_route` issues the `score_loader` call `_run_test` has always issued."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth, trainer
from iefvad_amd import lib as L

ROWS, HOST = "iefvad_forward_videos_similarity", "iefvad_forward_videos_host_similarity"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        L.build_library()
    return L.load_library()


def test_entries_exist_and_are_bound(lib):
    for s in (ROWS, HOST):
        assert s in L.SYMBOLS and hasattr(lib, s)
        assert getattr(lib, s).restype is C.c_int
    # the arguments of the plain entries, then the similarity pointer
    assert lib.iefvad_forward_videos_similarity.argtypes == lib.iefvad_forward_videos.argtypes + [C.c_void_p]
    assert lib.iefvad_forward_videos_host_similarity.argtypes == lib.iefvad_forward_videos_host.argtypes + [C.c_void_p]
    assert len(lib.iefvad_forward_videos_similarity.argtypes) == 14 and len(lib.iefvad_forward_videos_host_similarity.argtypes) == 15
    assert lib.iefvad_abi_version() == 8 and L.ABI_VERSION == 8          # entries were added, no struct changed


OK = C.c_void_p(0x10000)                                                 # never read: every call below stops in its checks


def _rows(lib, h=None, in_dtype=L.IN_F32, nvideos=2, sim=OK):
    lens = (C.c_int32 * 2)(5, 7)
    rc = lib.iefvad_forward_videos_similarity(h, OK, OK, in_dtype, lens, nvideos, 1, OK, 1 << 30, OK, None, None, None, sim)
    return rc, L.last_error()


def _host(lib, h=None, in_dtype=L.IN_F32, nvideos=2, sim=OK):
    lens = (C.c_int32 * 2)(5, 7)
    ptrs = (C.c_void_p * 2)(0x10000, 0x20000)
    rc = lib.iefvad_forward_videos_host_similarity(h, ptrs, ptrs, in_dtype, in_dtype, lens, nvideos, 1, 64, 0, OK, None, None, None, sim)
    return rc, L.last_error()


@pytest.mark.parametrize("call,name", [(_rows, ROWS), (_host, HOST)])
def test_bad_arguments_are_refused_and_the_message_names_the_entry(lib, call, name):
    """No handle exists without a GPU, so every call carries a null one: the similarity pointer, in_dtype and nvideos are checked
    before the handle is looked at, and the all-good call stops at the null handle."""
    for kw, frag in [(dict(sim=None), "null similarity"), (dict(sim=C.c_void_p(0x10002)), "4-byte aligned"),
                     (dict(sim=C.c_void_p(0x10001)), "4-byte aligned"), (dict(in_dtype=7), "in_dtype"), (dict(in_dtype=-1), "in_dtype"),
                     (dict(nvideos=0), "nvideos"), (dict(nvideos=-3), "nvideos"), (dict(), "null argument")]:
        rc, msg = call(lib, **kw)
        assert rc != 0 and msg.startswith(name + ":") and frag in msg, (kw, msg)


def test_the_plain_host_entry_still_names_itself(lib):
    lens = (C.c_int32 * 2)(5, 7)
    ptrs = (C.c_void_p * 2)(0x10000, 0x20000)
    rc = lib.iefvad_forward_videos_host(None, ptrs, ptrs, L.IN_F32, L.IN_F32, lens, 2, 1, 64, 0, OK, None, None, None)
    assert rc != 0 and L.last_error().startswith("iefvad_forward_videos_host:"), L.last_error()


def _model(**kw):
    args = argparse.Namespace(visual_layers=1, visual_head=8, num_refinement_steps=1, lambda_ref=0.5, noise_model="StudentT", nu=8)
    return iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 1, 8, 10, 10, "cuda", args, **kw).eval()


def test_similarity_does_not_combine_with_the_sweeps_extras(monkeypatch):
    model = _model()

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "load_library", no_load)
    rows = torch.zeros(12, 768)
    good = torch.ones(12)
    with pytest.raises(ValueError, match="similarity"):
        model.forward_videos(rows, rows, [5, 7], similarity=True, row_scale=(good, None))
    with pytest.raises(ValueError, match="similarity"):
        model.forward_videos(rows, rows, [5, 7], similarity=True, row_scale=(None, good))
    with pytest.raises(ValueError, match="similarity"):
        model.forward_videos(rows, rows, [5, 7], similarity=True, weight_sums=True)
    # alone it is a valid request: refused on host tensors as the plain call is
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.forward_videos(rows, rows, [5, 7], similarity=True)


class _Stub:
    outputs = "full"

    def __call__(self, img, ev, *_):
        raise AssertionError("no forward: the call is refused in its checks")

    def forward_videos(self, *a, **k):
        raise AssertionError("no forward on the CPU")


def _items():
    return [(torch.zeros(1, 1, 256, 8), torch.zeros(1, 1, 256, 8), ("Normal",), torch.tensor([10]))]


def test_score_loader_rows_needs_a_hip_device_and_a_known_string():
    with pytest.raises(ValueError, match='similarity="rows"'):
        harness.score_loader(_Stub(), _items(), 256, "cpu", "ucfcrime", batch_chunks=4, similarity="rows")
    with pytest.raises(ValueError, match="similarity must be"):
        harness.score_loader(_Stub(), _items(), 256, "cpu", "ucfcrime", batch_chunks=4, similarity="cols")
    with pytest.raises(ValueError, match="similarity must be"):
        harness.score_loader(_Stub(), _items(), 256, "cpu", "ucfcrime", similarity="padded")


def _run(monkeypatch, fn, *extra, **kw):
    """harness.test / ucf_test / xd_test with `score_loader` replaced by a recorder; returns the recorded (args, kwargs)."""
    calls = []

    def fake(*a, **k):
        calls.append((a, k))
        got = ([np.zeros(10, np.float32)], ["Normal"], [np.zeros(10, np.float32)], [np.zeros(10, np.float32)])
        if k.get("similarity"):
            got += ({key: [np.zeros(10, np.float32)] for key in harness.SIMILARITY_KEYS},)
        return got
    monkeypatch.setattr(harness, "score_loader", fake)
    monkeypatch.setattr(harness, "evaluate_scores", lambda *a, **k: {"roc": 0.5, "ap": 0.5})
    monkeypatch.setattr(harness, "draw_vis", lambda *a, **k: [])
    monkeypatch.setattr(harness, "vis_series", lambda *a, **k: {})
    args = argparse.Namespace(dataset="ucfcrime", exp_name="x", visual_length=256)
    model = torch.nn.Linear(1, 1)
    fn(args, model, "LOADER", 256, None, np.zeros(160), "cpu", *extra, **kw)
    assert len(calls) == 1
    return calls[0]


@pytest.mark.parametrize("vis", [False, True])
def test_the_default_route_issues_the_score_loader_call_of_before(monkeypatch, vis):
    want_kw = dict(lanes=1, return_device=False, similarity=vis)
    for fn, extra in ((harness.test, ()), (harness.ucf_test, ()), (harness.xd_test, ({"A": "normal"},))):
        for kw in ({}, {"vis_route": "padded"}):
            a, k = _run(monkeypatch, fn, *extra, vis=vis, **kw)
            assert k == want_kw and k["similarity"] is vis, (fn.__name__, k)
            assert a[1] == "LOADER" and a[2] == 256 and a[3] == "cpu" and a[4] == "ucfcrime" and a[6] == 0 and len(a) == 7


def test_vis_route_rows_asks_for_the_valid_row_series_at_64_chunks(monkeypatch):
    a, k = _run(monkeypatch, harness.ucf_test, vis=True, vis_route="rows")
    assert k["similarity"] == "rows" and a[6] == 64
    assert set(harness.ucf_test.last_result) >= {"roc", "ap", "scores", "classes", "w_i_mean", "w_e_mean", "similarity", "vis_files"}
    a, k = _run(monkeypatch, harness.ucf_test, vis=True, vis_route="rows", batch_chunks=16)
    assert k["similarity"] == "rows" and a[6] == 16
    # without vis the route is not read
    a, k = _run(monkeypatch, harness.ucf_test, vis=False, vis_route="rows")
    assert k["similarity"] is False and a[6] == 0


def test_unknown_vis_route_is_refused(monkeypatch):
    for fn, extra in ((harness.test, ()), (harness.ucf_test, ()), (harness.xd_test, ({"A": "normal"},))):
        with pytest.raises(ValueError, match="vis_route"):
            _run(monkeypatch, fn, *extra, vis=True, vis_route="ragged")
        with pytest.raises(ValueError, match="vis_route"):
            _run(monkeypatch, fn, *extra, vis_route=None)


class _Tiny(torch.nn.Module):
    def __init__(self, outputs):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.outputs = outputs


def _train_args():
    return argparse.Namespace(dataset="ucfcrime", visual_length=256, lr=1e-3, scheduler_milestones=[100], scheduler_rate=0.1, max_epoch=1,
                              print_steps=2, exp_name="sched", noise_model="StudentT", vis_steps=2)


@pytest.mark.filterwarnings("ignore:Detected call of `lr_scheduler.step")
def test_trainers_pass_the_route_on_and_accept_a_scores_only_model(tmp_path, monkeypatch):
    from torch.utils.data import DataLoader
    monkeypatch.chdir(tmp_path)
    calls = []
    monkeypatch.setattr(trainer, "train_step", lambda *a, **k: {"total": torch.tensor(0.0)} if k.get("want_terms") else None)
    monkeypatch.setattr(harness, "ucf_test", lambda *a, **k: calls.append(k) or (0.0, 0.0))
    monkeypatch.setattr(harness, "xd_test", lambda *a, **k: calls.append(k) or (0.0, 0.0))

    def loader(label):
        return DataLoader([(torch.zeros(4, 8), torch.zeros(4, 8), label, 4) for _ in range(3)], batch_size=1, shuffle=False)
    ucf_map = {c: c.lower() for c in synth.UCF_CLASSES}
    xd_map = {"A": "normal", "B1": "fighting", "B2": "shooting", "B4": "riot", "B5": "abuse", "B6": "car accident", "G": "explosion"}
    model = _Tiny("scores")
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    trainer.train_paired(_train_args(), model, loader("Normal"), loader("Arson"), "LOADER", ucf_map, "cpu", gt=np.zeros(16), optimizer=opt,
                         vis=True, vis_route="rows")
    trainer.train_single(_train_args(), model, loader("A"), "LOADER", xd_map, "cpu", gt=np.zeros(16), optimizer=opt, vis=True, vis_route="rows")
    assert calls and all(k["vis_route"] == "rows" and k["batch_chunks"] == 64 for k in calls)
    for run in (lambda **kw: trainer.train_paired(_train_args(), model, [], [], [], ucf_map, "cpu", gt=np.zeros(16), **kw),
                lambda **kw: trainer.train_single(_train_args(), model, [], [], xd_map, "cpu", gt=np.zeros(16), **kw)):
        with pytest.raises(ValueError, match="vis_route"):
            run(vis=True, vis_route="ragged")
        with pytest.raises(ValueError, match='outputs="full"'):        # the padded route keeps its start-up check
            run(vis=True)
