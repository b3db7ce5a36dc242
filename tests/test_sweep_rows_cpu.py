"""The robustness sweep on valid rows (`iefvad_forward_videos_scaled`, csrc/ragged.h; `MMFMIL.forward_videos(row_scale=, weight_sums=)`;
`harness.PerturbationSweep(ragged=True)`) -- what can be checked without a GPU: the two entries exist and refuse bad arguments before
the first HIP call, the packed scale vectors equal the padded route's at every valid row, and the Python layers validate their
arguments before they load the library."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth
from iefvad_amd import lib as L

LENGTHS = [40, 300, 17, 256, 90, 520]
T = 256


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(L.LIB_PATH):
        L.build_library()
    return L.load_library()


def test_entries_exist_and_are_bound(lib):
    for s in ("iefvad_forward_videos_scaled", "iefvad_videos_scaled_workspace_bytes"):
        assert s in L.SYMBOLS and hasattr(lib, s)
        assert getattr(lib, s).argtypes is not None
    assert len(lib.iefvad_forward_videos_scaled.argtypes) == 16 and lib.iefvad_forward_videos_scaled.restype is C.c_int
    assert len(lib.iefvad_videos_scaled_workspace_bytes.argtypes) == 4 and lib.iefvad_videos_scaled_workspace_bytes.restype is C.c_size_t
    assert lib.iefvad_abi_version() == 8 and L.ABI_VERSION == 8          # entries were added, no struct changed


def test_null_handle_is_refused_and_the_message_names_the_entry(lib):
    ok = C.c_void_p(0x10000)                                             # never read: the call stops in its checks
    lens = (C.c_int32 * 2)(5, 7)
    rc = lib.iefvad_forward_videos_scaled(None, ok, ok, L.IN_F32, lens, 2, 2, None, None, ok, 1 << 30, ok, None, None, None, None)
    assert rc != 0
    assert L.last_error().startswith("iefvad_forward_videos_scaled:"), L.last_error()


def test_workspace_query_returns_zero_for_bad_arguments(lib):
    lens = (C.c_int32 * 2)(5, 7)
    wb = lib.iefvad_videos_scaled_workspace_bytes
    for with_colsum in (0, 1):
        assert wb(None, lens, 2, with_colsum) == 0
    # (a handle needs a GPU; with one, tests/test_gpu_sweep_rows.py checks null lengths, nvideos <= 0 and a length of zero)


def _draws(seed, k_img, k_ev):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in LENGTHS:
        di = torch.randperm(T, generator=gen)[:k_img] if k_img else None
        de = torch.randperm(T, generator=gen)[:k_ev] if k_ev else None
        out.append((di, de))
    return out


def _padded_sweep(D=8):
    def loader():
        for i, n in enumerate(LENGTHS):
            img, ev = synth.make_video(3, i, n, D=D)
            ci, _ = harness.process_split(img, T)
            ce, _ = harness.process_split(ev, T)
            yield torch.tensor(ci).unsqueeze(0), torch.tensor(ce).unsqueeze(0), ("Normal",), torch.tensor([n])
    gt = synth.make_gt(3, sum(LENGTHS))
    return harness.PerturbationSweep(argparse.Namespace(visual_length=T), None, loader(), gt, "cpu", batch_chunks=3)


@pytest.mark.parametrize("k_img,k_ev", [(51, 0), (0, 76), (12, 128)])
def test_packed_scales_equal_the_padded_routes_at_every_valid_row(k_img, k_ev):
    """`sweep_row_scales` against `PerturbationSweep._scales` (the [chunks * T] vectors of the padded route): row r of video v sits at
    (chunk r // T, time step r % T) of the video's chunks."""
    sweep = _padded_sweep()
    assert len(sweep.batches) > 1
    draws = _draws(5, k_img, k_ev)
    packed = harness.sweep_row_scales(LENGTHS, draws, T)
    padded = [sweep._scales(batch, draws) for batch in sweep.batches]
    for m, k in ((0, k_img), (1, k_ev)):
        if not k:
            assert packed[m] is None and all(p[m] is None for p in padded)
            continue
        s = packed[m]
        assert s.dtype == torch.float32 and s.is_contiguous() and s.shape == (sum(LENGTHS),)
        off = 0
        for batch, p in zip(sweep.batches, padded):
            chunk0 = 0
            for v in batch:
                n = LENGTHS[v]
                want = p[m].reshape(-1, T)[chunk0:chunk0 + sweep.nchunks[v]].reshape(-1)[:n]
                assert torch.equal(s[off:off + n], want), (m, v)
                assert int((s[off:off + min(n, T)] != 1).sum()) == int((draws[v][m] < n).sum())
                off += n
                chunk0 += sweep.nchunks[v]
        assert off == sum(LENGTHS)
        assert set(s.unique().tolist()) <= {1.0, float(np.float32(0.01))}


def test_ragged_sweep_on_a_cpu_device_is_refused():
    def loader():
        img = torch.zeros(1, 1, T, 8)
        yield img, img, ("Normal",), torch.tensor([10])
    with pytest.raises(ValueError, match="HIP device only"):
        harness.PerturbationSweep(argparse.Namespace(visual_length=T), None, loader(), np.zeros(160), "cpu", ragged=True)


def test_forward_videos_validates_the_extras_before_loading_the_library(monkeypatch):
    args = argparse.Namespace(visual_layers=1, visual_head=8, num_refinement_steps=1, lambda_ref=0.5, noise_model="StudentT", nu=8)
    model = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 1, 8, 10, 10, "cuda", args).eval()

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "load_library", no_load)
    rows = torch.zeros(12, 768)
    good = torch.ones(12)
    with pytest.raises(ValueError, match="row_scale"):
        model.forward_videos(rows, rows, [5, 7], row_scale=(good[:-1], None))
    with pytest.raises(ValueError, match="row_scale"):
        model.forward_videos(rows, rows, [5, 7], row_scale=(None, good.double()))
    with pytest.raises(ValueError, match="row_scale"):
        model.forward_videos(rows, rows, [5, 7], row_scale=(torch.ones(24)[::2], None))
    with pytest.raises(ValueError, match="row_scale"):
        model.forward_videos(rows, rows, [5, 7], row_scale=(good,))
    with pytest.raises(ValueError, match="nan_to_num"):
        model.forward_videos(rows, rows, [5, 7], nan_to_num="sometimes")
    # valid extras on host tensors: refused as the plain call is, still without a library
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.forward_videos(rows, rows, [5, 7], nan_to_num="always", row_scale=(good, None), weight_sums=True)
