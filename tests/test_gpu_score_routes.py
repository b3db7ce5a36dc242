"""The routes of `harness.score_loader` -- padded chunks (packed and one forward per video), the valid-row loop around
`MMFMIL.forward_videos` (one lane and two) and the list walked inside the library -- on one list of videos whose lengths sit on the
chunk edges: same classes, and in compute="f32" (every tiling sums k in one order) the same scores and mean fusion weights bit for
bit, whichever route, packing, lane count or bytes-per-library-call produced them."""
import argparse

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth

pytestmark = pytest.mark.gpu

# one row | a short video | exactly one chunk (the loader's all-zero second chunk is dropped) | one row over a chunk |
# a ragged multi-chunk video | an exact multiple of the chunk size
LENGTHS = [1, 37, 256, 257, 600, 512]
CLASSES = ["Normal", "Abuse"] * 3
PACKED = {"padded": dict(ragged=False),
          "rows_loop": dict(ragged=True, host_list=False, lanes=1),
          "rows_loop_2_lanes": dict(ragged=True, host_list=False, lanes=2),
          "rows_list": dict(),
          "rows_list_per_video": dict(host_list_bytes=1)}
PER_VIDEO = {"per_video": dict(lanes=1), "per_video_2_lanes": dict(lanes=2)}


@pytest.fixture(scope="module")
def routes():
    """Every route's (scores, classes, w_i_mean, w_e_mean), computed once; `padded` and `rows_list` also with return_device."""
    L, K = 2, 3
    args = argparse.Namespace(visual_layers=L, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    model = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, L, 8, 10, 10, "cuda", args, compute="f32", outputs="scores")
    model.load_state_dict(synth.make_state_dict(41, 768, L, K))
    model = model.to("cuda:0").eval()
    vids = [synth.make_video(31, i, n) for i, n in enumerate(LENGTHS)]

    def items():
        for (img, ev), cls in zip(vids, CLASSES):
            ci, n = harness.process_split(img, 256)
            ce, _ = harness.process_split(ev, 256)
            yield torch.tensor(ci).unsqueeze(0), torch.tensor(ce).unsqueeze(0), (cls,), torch.tensor([n])

    res = {}
    for name, kw in PACKED.items():
        res[name] = harness.score_loader(model, items(), 256, "cuda:0", "ucfcrime", batch_chunks=2, **kw)
    for name, kw in PER_VIDEO.items():
        res[name] = harness.score_loader(model, items(), 256, "cuda:0", "ucfcrime", batch_chunks=0, **kw)
    for name in ("padded", "rows_list"):
        res[name + "/device"] = harness.score_loader(model, items(), 256, "cuda:0", "ucfcrime", batch_chunks=2, return_device=True,
                                                     **PACKED[name])
    return res


def _assert_same(got, want, name):
    assert got[1] == want[1] == CLASSES, name
    for k, what in ((0, "scores"), (2, "w_i_mean"), (3, "w_e_mean")):
        assert len(got[k]) == len(LENGTHS), (name, what)
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            assert a.shape == b.shape == (LENGTHS[i],), (name, what, i)
            print(f"{name} {what} video {i}: max |diff| = {float(np.abs(a - b).max()):.3e}")
            assert np.array_equal(a, b), (name, what, i, float(np.abs(a - b).max()))


@pytest.mark.parametrize("name", [n for n in PACKED if n != "padded"])
def test_packed_routes_give_the_same_bits(routes, name):
    assert np.isfinite(np.concatenate(routes["padded"][0])).all()
    _assert_same(routes[name], routes["padded"], name)


@pytest.mark.parametrize("name", list(PER_VIDEO))
def test_one_forward_per_video_gives_the_same_bits_on_one_lane_and_on_two(routes, name):
    _assert_same(routes[name], routes["padded"], name)


@pytest.mark.parametrize("name", ["padded", "rows_list"])
def test_return_device_is_the_concatenated_scores_on_the_device(routes, name):
    """The padded route leaves gaps between the videos (the tensor is put together from the valid spans), the list route leaves
    them back to back: either way the fifth result is the valid snippets in loader order."""
    scores, classes, wi, we, dev = routes[name + "/device"]
    assert dev.device == torch.device("cuda:0")
    assert dev.numel() == sum(LENGTHS)
    assert np.array_equal(dev.cpu().numpy(), np.concatenate(scores))
    _assert_same((scores, classes, wi, we), routes[name], name + "/device")
