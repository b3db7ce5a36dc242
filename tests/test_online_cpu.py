"""The online scores without a GPU: `harness.online_windows` against the worked values of its rule, csrc/window_plan.h (compiled here
with g++ from tests/online_plan.cpp) against that host model -- windows, read-out map and pass cuts --, the C declarations, and the
refusals of `MMFMIL.forward_videos_online` and of the harness keywords on host tensors, all before a device is touched."""
import argparse
import ctypes as C
import operator
import os
import shutil
import subprocess

import pytest
import torch

import iefvad_amd
from iefvad_amd import harness
from iefvad_amd import lib as L
from iefvad_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, stride, history) -> the windows as (start, end, read0), worked out by hand from
#   end_j = min(j stride, n), start_j = max(0, end_j - history), read0_j = (j - 1) stride
WORKED = {
    (300, 128, 256): [(0, 128, 0), (0, 256, 128), (44, 300, 256)],
    (300, 256, 256): [(0, 256, 0), (44, 300, 256)],
    (5, 1, 256): [(0, 1, 0), (0, 2, 1), (0, 3, 2), (0, 4, 3), (0, 5, 4)],
    (600, 100, 256): [(0, 100, 0), (0, 200, 100), (44, 300, 200), (144, 400, 300), (244, 500, 400), (344, 600, 500)],
    (600, 100, 150): [(0, 100, 0), (50, 200, 100), (150, 300, 200), (250, 400, 300), (350, 500, 400), (450, 600, 500)],
}


def cpu_model(compute="f32", **kw):
    args = argparse.Namespace(visual_layers=1, visual_head=8, num_refinement_steps=3, lambda_ref=0.5, noise_model="StudentT", nu=8)
    return iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 1, 8, 10, 10, "cpu", args, compute=compute, **kw).eval()


@pytest.mark.parametrize("case", sorted(WORKED))
def test_online_windows_reproduces_the_worked_rows(case):
    n, stride, history = case
    assert harness.online_windows(n, stride, history) == WORKED[case]
    if history == 256:
        assert harness.online_windows(n, stride) == WORKED[case]      # the default history


def check_windows(n, stride, history):
    starts, ends, reads = zip(*harness.online_windows(n, stride, history))
    assert reads == tuple(range(0, n, stride))                       # read0_j = (j - 1) stride, ceil(n / stride) windows
    assert ends == reads[1:] + (n,)                                  # end_j = min(j stride, n): the next read0, or n
    assert starts == tuple(e - history if e > history else 0 for e in ends)
    assert all(map(operator.le, starts, reads)) and all(map(operator.lt, reads, ends))


def test_every_snippet_is_read_by_exactly_one_window():
    """The read-out ranges [read0, end) tile 0 .. n - 1 in order, read0 >= start, and a window starts where the rule says.
    Every n = 1 .. 600 over every stride 1 .. 256 at the tightest history (= stride, where start is largest) and at a grid of
    histories (256 among them: every stride once more); and the FULL triangle of 32896 (stride, history) pairs at the lengths around
    a chunk edge and the longest.  All pairs times all 600 lengths is 19.7 million calls, two minutes of pure Python, and adds nothing
    to these: ends and read0 do not depend on the history, and start = max(0, end - history) only falls as the history grows."""
    pairs = {(s, s) for s in range(1, 257)} | {(s, h) for h in (2, 16, 150, 256) for s in range(1, h + 1)}
    for stride, history in sorted(pairs):
        for n in range(1, 601):
            check_windows(n, stride, history)
    for history in range(1, 257):
        for stride in range(1, history + 1):
            for n in (1, 255, 256, 257, 600):
                check_windows(n, stride, history)


def test_online_windows_refuses_bad_parameters():
    for stride, history in ((0, 256), (257, 257), (17, 16), (1, 257), (-1, 4), (True, 4), (2.0, 4), (4, None)):
        with pytest.raises(ValueError):
            harness.online_windows(10, stride, history)
    with pytest.raises(ValueError, match="at least one snippet"):
        harness.online_windows(0, 1)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is part of this project's toolchain (tests/cabi builds with it too)"
    exe = os.path.join(str(tmp_path_factory.mktemp("online_plan")), "online_plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ief-vad_amd", "csrc"),
                        os.path.join(ROOT, "tests", "online_plan.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]

    def ask(stride, history, micro_batch, lens):
        out = subprocess.run([exe, str(stride), str(history), str(micro_batch), *map(str, lens)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        rows = {"ok": [], "n": [], "w": [], "r": [], "p": []}
        for line in out.stdout.split("\n"):
            if line:
                rows[line.split()[0]].append(tuple(int(x) for x in line.split()[1:]))
        return rows
    return ask


def host_plan(stride, history, micro_batch, lens):
    """The plan from `harness.online_windows`: windows in packed rows of the call, cut into runs of `micro_batch`; a pass's source base
    is its first window's start, its output base its first window's read0; the read-out map is (read0 - start, end - read0, read0 -
    the pass's output base)."""
    wins, base = [], 0
    for v, n in enumerate(lens):
        wins += [(v, base + s, base + e, base + r) for s, e, r in harness.online_windows(n, stride, history)]
        base += n
    passes, reads = [], []
    for c0 in range(0, len(wins), micro_batch):
        run = wins[c0:c0 + micro_batch]
        passes.append((c0, len(run), run[0][1], run[0][3], run[-1][2] - run[0][3]))
        reads += [(r - s, e - r, r - run[0][3]) for _, s, e, r in run]
    return wins, reads, passes


@pytest.mark.parametrize("stride, history, micro_batch, lens", [
    (128, 256, 3, [300]), (256, 256, 3, [300]), (1, 256, 3, [5]), (100, 256, 3, [600]), (100, 150, 3, [600]),
    (16, 256, 3, [1, 37, 255, 256, 257, 300, 600]), (100, 150, 3, [1, 37, 255, 256, 257, 300, 600]), (1, 256, 3, [1, 5, 70, 258]),
    (16, 256, 128, [1, 37, 255, 256, 257, 300, 600]), (7, 9, 1, [20, 1, 9]), (256, 256, 2, [37, 256, 512]),
])
def test_window_plan_header_matches_the_host_model(plan, stride, history, micro_batch, lens):
    got = plan(stride, history, micro_batch, lens)
    wins, reads, passes = host_plan(stride, history, micro_batch, lens)
    assert got["ok"] == [(1,)] and got["n"] == [(len(wins),)]
    assert got["w"] == wins
    assert got["r"] == reads
    assert got["p"] == passes
    # what the device code relies on: source bases never decrease, a pass's windows start at or behind its base, and the read-out
    # rows of a pass are contiguous and at most 256 per window
    assert all(a[2] <= b[2] for a, b in zip(passes, passes[1:]))
    for first, count, src_base, out_base, out_rows in passes:
        assert all(w[1] >= src_base for w in wins[first:first + count]) and 0 < out_rows <= 256 * count
        assert sum(r[1] for r in reads[first:first + count]) == out_rows
    assert sum(p[4] for p in passes) == sum(lens)


def test_window_plan_header_refuses_what_the_host_model_refuses(plan):
    for stride, history in ((0, 256), (257, 257), (17, 16), (1, 257)):
        assert plan(stride, history, 3, [10])["ok"] == [(0,)]
    assert plan(4, 8, 3, [10, 0])["n"] == [(-1,)]      # a non-positive length


def test_header_declares_the_entries_and_keeps_the_abi():
    header = open(os.path.join(ROOT, "include", "iefvad.h")).read()
    assert "#define IEFVAD_ABI_VERSION 8" in header
    assert "typedef struct iefvad_online {" in header and "} iefvad_online;" in header
    assert "int iefvad_forward_videos_online(iefvad_handle* h," in header and "size_t iefvad_videos_online_workspace_bytes(" in header
    lib = L.load_library()
    assert lib.iefvad_abi_version() == 8 and L.ABI_VERSION == 8
    for s in ("iefvad_forward_videos_online", "iefvad_videos_online_workspace_bytes"):
        assert s in L.SYMBOLS and hasattr(lib, s), s
    assert lib.iefvad_forward_videos_online.restype is C.c_int and lib.iefvad_videos_online_workspace_bytes.restype is C.c_size_t
    assert C.sizeof(L.Online) == 8 and L.ONLINE_MAX_HISTORY == 256


def test_null_arguments_are_refused_by_name():
    lib = L.load_library()
    on = L.Online(16, 256)
    lens = (C.c_int32 * 1)(5)
    assert lib.iefvad_forward_videos_online(None, None, None, 0, lens, 1, 1, C.byref(on), None, 0, None, None, None, None) != 0
    assert L.last_error().startswith("iefvad_forward_videos_online:") and "null" in L.last_error()
    assert lib.iefvad_videos_online_workspace_bytes(None, lens, 1, C.byref(on)) == 0


def test_argument_checks_come_before_the_library():
    """Host tensors throughout: every ValueError below is raised before the RuntimeErrors, and the device check comes last."""
    m = cpu_model()
    rows = torch.zeros(5, 768)
    for stride, history in ((0, 256), (257, 256), (257, 257), (17, 16), (True, 256), (2.5, 256), (4, 300)):
        with pytest.raises(ValueError, match="stride"):
            m.forward_videos_online(rows, rows, [5], stride, history=history)
    for bad in (1, 0, None, "always"):
        with pytest.raises(ValueError, match="nan_to_num must be True or False"):
            m.forward_videos_online(rows, rows, [5], 16, nan_to_num=bad)
    for lens in ([4], [5, 1]):
        with pytest.raises(ValueError, match="sum of lengths x D"):
            m.forward_videos_online(rows, rows, lens, 16)
    with pytest.raises(ValueError, match="sum of lengths x D"):
        m.forward_videos_online(rows, torch.zeros(5, 512), [5], 16)
    with pytest.raises(ValueError, match="sum of lengths x D"):
        m.forward_videos_online(torch.zeros(1, 5, 768), torch.zeros(1, 5, 768), [5], 16)
    with pytest.raises(ValueError, match="at least one snippet"):
        m.forward_videos_online(rows, rows, [5, 0], 16)
    with pytest.raises(RuntimeError, match="requires grad"):
        m.forward_videos_online(rows.clone().requires_grad_(True), rows, [5], 16)
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.forward_videos_online(rows, rows, [5], 16)
    m.train()
    with pytest.raises(RuntimeError, match=r"model.train\(\)"):
        m.forward_videos_online(rows, rows, [5], 16)
    m.eval()
    with pytest.raises(RuntimeError, match="fp16x3"):
        cpu_model(compute="fp16x3").forward_videos_online(rows, rows, [5], 16)


def test_the_entry_has_a_sibling_table():
    assert set(M._ONLINE_ENTRIES) == {"_online"}
    query, query_tail, tail = M._entry_row(M._ROW_ENTRIES, "_online")
    assert query == "_online"
    r = {"vectors": (1, 2, 3), "stream": 4, "online": 5}
    assert query_tail(r) == (5,) and tail(r) == (1, 2, 3, 4)
    # the request tables of forward / forward_videos are as they were: the online scores are a method of their own, not a keyword
    assert "_online" not in M._ROW_ENTRIES and "online" not in M._DENSE_ENTRIES and "_online" not in M._SAMPLES_ENTRIES
    assert M._entry_row(M._ROW_ENTRIES, "_samples") is M._SAMPLES_ENTRIES["_samples"] and M._entry_row(M._ROW_ENTRIES, "") is M._ROW_ENTRIES[""]
    names = M.MMFMIL.forward_videos.__code__.co_varnames + M.MMFMIL.forward.__code__.co_varnames + M.MMFMIL.forward_videos_host.__code__.co_varnames
    assert "stride" not in names and "history" not in names and "online" not in names


def test_harness_refusals():
    m = cpu_model()
    with pytest.raises(ValueError, match="host_list=False"):
        harness.score_loader(m, [], 256, "cuda", batch_chunks=64, online_stride=16)
    with pytest.raises(ValueError, match="HIP device"):
        harness.score_loader(m, [], 256, "cpu", batch_chunks=64, host_list=False, online_stride=16)
    with pytest.raises(ValueError, match="batch_chunks > 0"):
        harness.score_loader(m, [], 256, "cuda", host_list=False, online_stride=16)
    with pytest.raises(ValueError, match="stride"):
        harness.score_loader(m, [], 256, "cuda", batch_chunks=64, host_list=False, online_stride=0)
    with pytest.raises(ValueError, match="stride"):
        harness.score_loader(m, [], 256, "cuda", batch_chunks=64, host_list=False, online_stride=32, online_history=16)
    for extra in (dict(trajectory=True), dict(fusion_variants=True), dict(score_samples=4, sample_seed=1), dict(similarity="rows"),
                  dict(row_outputs="full"), dict(attn_maps=True), dict(steps=1)):
        with pytest.raises(ValueError, match="does not combine"):
            harness.score_loader(m, [], 256, "cuda", batch_chunks=64, host_list=False, online_stride=16, **extra)
    for fn in (harness.test, harness.ucf_test, harness.xd_test):
        kw = fn.__kwdefaults__ or {}
        assert kw.get("online_stride", 0) is None and kw.get("online_history") == 256
