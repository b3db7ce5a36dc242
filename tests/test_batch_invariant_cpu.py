"""The batch-invariant mode of compute="bf16x6" (`MMFMIL(..., batch_invariant=True)`, `iefvad_set_batch_invariant`, the small tiling's
unit entry and launch counter) -- what can be checked without a GPU: the keyword is stored and travels with `lanes`, fp16x3 is refused
at construction, the new entries exist, are bound and refuse bad arguments by name before the first HIP call, and CPU tensors are
refused as they always were."""
import argparse
import ctypes as C
import inspect
import os

import pytest
import torch

import iefvad_amd
from iefvad_amd import harness
from iefvad_amd import lib as L


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        L.build_library()
    return L.load_library()


def _model(**kw):
    args = argparse.Namespace(visual_layers=1, visual_head=8, num_refinement_steps=1, lambda_ref=0.5, noise_model="StudentT", nu=8)
    return iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 1, 8, 10, 10, "cuda", args, **kw).eval()


def test_keyword_is_stored_keyword_only_and_off_by_default():
    p = inspect.signature(iefvad_amd.MMFMIL.__init__).parameters["batch_invariant"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert _model(compute="bf16x6").batch_invariant is False
    assert _model().batch_invariant is False
    for compute in ("bf16x6", "f32", "bf16"):                  # accepted (and inert) in the modes that are invariant already
        assert _model(compute=compute, batch_invariant=True).batch_invariant is True
    assert _model(compute="bf16x6", batch_invariant=1).batch_invariant is True


def test_lanes_carry_the_keyword():
    model = _model(compute="bf16x6", batch_invariant=True)
    lanes = model.lanes(3)
    assert len(lanes) == 3 and lanes[0] is model
    for lane in lanes[1:]:
        assert lane.batch_invariant is True and lane.compute == "bf16x6" and lane._handle is None
        assert lane.temporal is model.temporal
    assert all(lane.batch_invariant is False for lane in _model(compute="bf16x6").lanes(2))


def test_fp16x3_is_refused_at_construction():
    with pytest.raises(ValueError, match="fp16x3"):
        _model(compute="fp16x3", batch_invariant=True)
    assert _model(compute="fp16x3").batch_invariant is False   # the mode itself stays available


def test_cpu_tensors_are_refused_as_before():
    x = torch.zeros(1, 256, 768)
    rows = torch.zeros(12, 768)
    for kw in (dict(compute="bf16x6", batch_invariant=True), dict(compute="bf16x6")):
        model = _model(**kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model(x, x, None, None, None)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.forward_videos(rows, rows, [5, 7])


def test_harness_default_route_reads_the_flag(monkeypatch):
    """`_run_test` without `batch_chunks`: 64 (the packed route) for f32, bf16 and an invariant bf16x6 model on a HIP device, 0 (one
    forward per video) for a default bf16x6 model, for fp16x3 and on the CPU."""
    seen = []

    class Done(Exception):
        pass

    def spy(model, loader, maxlen, device, dataset, label_map, batch_chunks, *a, **kw):
        seen.append(batch_chunks)
        raise Done

    monkeypatch.setattr(harness, "score_loader", spy)
    args = argparse.Namespace(dataset="ucfcrime")
    cases = [(dict(compute="bf16x6", batch_invariant=True), "cuda:0", 64), (dict(compute="bf16x6"), "cuda:0", 0),
             (dict(compute="f32"), "cuda:0", 64), (dict(compute="bf16", batch_invariant=True), "cuda:0", 64),
             (dict(compute="fp16x3"), "cuda:0", 0), (dict(compute="bf16x6", batch_invariant=True), "cpu", 0)]
    for kw, device, want in cases:
        model = _model(**kw)
        monkeypatch.setattr(model, "to", lambda *a, **k: model, raising=False)      # no device here: the route is chosen before any forward
        with pytest.raises(Done):
            harness.test(args, model, [], 256, None, None, device)
    assert seen == [c[2] for c in cases], seen


def test_entries_exist_and_are_bound(lib):
    for s in ("iefvad_gemm_split_small_unit", "iefvad_gemm_split_small_launches", "iefvad_set_batch_invariant"):
        assert s in L.SYMBOLS and hasattr(lib, s)
    # the unit entry: the arguments of iefvad_gemm_split_unit minus tile_n
    wide = list(lib.iefvad_gemm_split_unit.argtypes)
    assert lib.iefvad_gemm_split_small_unit.argtypes == wide[:9] + wide[10:]
    assert lib.iefvad_gemm_split_small_unit.restype is C.c_int and lib.iefvad_set_batch_invariant.restype is C.c_int
    assert lib.iefvad_gemm_split_small_launches.restype is C.c_uint64
    assert lib.iefvad_abi_version() == L.ABI_VERSION == 8      # entries were added, no struct changed
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iefvad.h")).read()
    assert "#define IEFVAD_ABI_VERSION 8" in header and "int iefvad_set_batch_invariant(iefvad_handle* h, int on);" in header


def test_bad_arguments_are_refused_by_name_before_any_launch(lib):
    n0 = lib.iefvad_gemm_split_small_launches()
    assert lib.iefvad_set_batch_invariant(None, 1) != 0
    assert L.last_error().startswith("iefvad_set_batch_invariant:") and "null" in L.last_error()
    io = L.GemmSplitIO()
    st = C.c_void_p(0)
    assert lib.iefvad_gemm_split_small_unit(None, 128, 128, 64, 128, 0, 0, 0.5, 1, st) != 0
    assert L.last_error().startswith("iefvad_gemm_split_small_unit:")
    for (M, N, K, epi, nz), frag in [((128, 128, 64, 7, 1), "unknown epilogue"), ((128, 128, 64, 0, 3), "nz = 3"),
                                     ((48, 128, 64, 0, 1), "M=48"), ((128, 192, 64, 0, 1), "N=192"), ((128, 128, 32, 0, 1), "K=32"),
                                     ((128, 128, 64, 0, 1), "lacks an operand")]:
        assert lib.iefvad_gemm_split_small_unit(C.byref(io), M, N, K, N, epi, 0, 0.5, nz, st) != 0
        msg = L.last_error()
        assert msg.startswith("iefvad_gemm_split_small_unit:") and frag in msg, msg
    # the 128 x 128 entry keeps its refusals, the tile in the message included
    assert lib.iefvad_gemm_split_unit(C.byref(io), 96, 128, 64, 128, 0, 0, 0.5, 1, 128, st) != 0
    assert L.last_error() == "iefvad_gemm_split_unit: shape M=96 N=128 K=64 not a multiple of the 128x128x64 tile"
    assert lib.iefvad_gemm_split_small_launches() == n0
