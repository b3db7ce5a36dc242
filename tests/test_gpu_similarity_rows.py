"""The similarity series on the valid-row routes: `MMFMIL.forward_videos(similarity=True)` / `forward_videos_host(similarity=True)`
(`iefvad_forward_videos_similarity`, `iefvad_forward_videos_host_similarity`; `iefvad_similarity_rowset_kernel`, csrc/similarity.h),
`harness.score_loader(similarity="rows")` and `vis_route="rows"` on top of them.  `-m gpu`.

The reference throughout is the padded route as it was: an outputs="full" model of the same weights on `harness.process_split` chunks,
then `harness.similarity_rows(fused, image_mu, event_mu, index of the [0:len] slices)`.  In f32, bf16 and fp16x3 the valid-row route
performs every product and sum of the padded one and the two kernels share one row body, so equality is bit for bit; in bf16x6 (kernels
picked by batch size) the caps are those derived in tests/test_gpu_vis.py from the suite's gate on the 768-d outputs:
  |d dist| <= 2 TOL_BIG sqrt(D)          |d cos| <= 2 TOL_BIG sqrt(D) (1 / |fused| + 1 / |mu|), norms from the padded reference."""
import argparse
import functools
import math
import os

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

EDGE = [37, 255, 256, 257, 512, 1500, 1, 300]      # 3,118 rows, 16 chunks: a one-row chunk, a len % 256 == 0 video, a six-chunk video
N = sum(EDGE)
T = 256
KEYS = ("cos_i", "cos_e", "dist_i", "dist_e")
SCORE_KEYS = ("logits", "w_i_mean", "w_e_mean")


def make_model(compute, D=768, L_=2, K=3, **kw):
    sd = synth.make_state_dict(41, D, L_, K)
    args = argparse.Namespace(visual_layers=L_, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, D, 256, D, 8, L_, 8, 10, 10, "cuda", args, compute=compute, **kw)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


@functools.lru_cache(maxsize=None)
def videos(dtype, D=768):
    return tuple(synth.make_video(6, i, int(n), D=D, dtype=dtype) for i, n in enumerate(EDGE))


def pack(vids):
    return (torch.from_numpy(np.concatenate([v[0] for v in vids])).cuda(), torch.from_numpy(np.concatenate([v[1] for v in vids])).cuda())


def pad(vids):
    """Host-side chunker: ([C, 256, D] image, event) on the device and the index of the `[0:len]` slices."""
    D = vids[0][0].shape[1]
    ci = [harness.process_split(v[0], T)[0].reshape(-1, T, D) for v in vids]
    ce = [harness.process_split(v[1], T)[0].reshape(-1, T, D) for v in vids]
    index, off = [], 0
    for c, v in zip(ci, vids):
        index.append(np.arange(off * T, off * T + v[0].shape[0], dtype=np.int32))
        off += c.shape[0]
    return torch.from_numpy(np.concatenate(ci)).cuda(), torch.from_numpy(np.concatenate(ce)).cuda(), torch.from_numpy(np.concatenate(index))


@functools.lru_cache(maxsize=None)
def reference(compute, dtype, micro_batch=0, D=768):
    """The padded route, computed once per configuration and left unchanged: ([4, N] series, |fused|, |image_mu|, |event_mu| of the
    valid rows)."""
    model = make_model(compute, D=D, outputs="full", micro_batch=micro_batch)
    img, ev, index = pad(videos(dtype, D))
    with torch.no_grad():
        out = model(img, ev, None, None, None)
        sim = harness.similarity_rows(out["fused"], out["image_mu"], out["event_mu"], index)
        idx = index.long().cuda()
        norms = tuple(out[k].reshape(-1, D)[idx].double().norm(dim=1).cpu().numpy() for k in ("fused", "image_mu", "event_mu"))
    assert sim.shape == (4, N) and bool(torch.isfinite(sim).all())
    return (sim.clone(),) + norms


def rows_call(model, dtype, D=768, **kw):
    rows = pack(videos(dtype, D))
    with torch.no_grad():
        return model.forward_videos(rows[0], rows[1], EDGE, **kw)


def assert_series_equal(got, want, tag):
    assert got.shape == want.shape == (4, N) and got.dtype == torch.float32
    for j, k in enumerate(KEYS):
        d = float((got[j] - want[j]).abs().max())
        print(tag, k, "max |rows - padded| =", d)
        assert torch.equal(got[j], want[j]), (tag, k, d)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("compute,micro_batch", [("f32", 0), ("f32", 3), ("bf16", 0), ("bf16", 3), ("fp16x3", 0)])
def test_series_equal_the_padded_route_bit_for_bit(compute, micro_batch, dtype):
    """1. A scores-only model: the library keeps what it needs.  micro_batch = 3: the six-chunk video straddles passes, so a pass
    writes at its own offset with the call's stride."""
    model = make_model(compute, outputs="scores", micro_batch=micro_batch)
    got = rows_call(model, dtype, similarity=True)
    assert set(got) == set(SCORE_KEYS) | {"similarity"}
    assert_series_equal(got["similarity"], reference(compute, dtype, micro_batch)[0], (compute, micro_batch, dtype.__name__))


def test_series_on_the_compacted_row_set(monkeypatch):
    """1. IEFVAD_DENSE_ENCODER=1 (read when the handle is created): the tail runs on the gathered valid rows in packed order, the map
    is the identity and there is no table."""
    want = reference("f32", np.float32)[0]
    monkeypatch.setenv("IEFVAD_DENSE_ENCODER", "1")
    got = rows_call(make_model("f32", outputs="scores"), np.float32, similarity=True)
    assert_series_equal(got["similarity"], want, "dense encoder")


def test_series_d512():
    """1. ViT-B/16 width, f32."""
    got = rows_call(make_model("f32", D=512, outputs="scores"), np.float32, D=512, similarity=True)
    assert_series_equal(got["similarity"], reference("f32", np.float32, 0, 512)[0], "D=512")


def caps_for(D, nf, ni, ne):
    r = H.TOL_BIG * math.sqrt(D)
    return {"dist_i": 2 * r, "dist_e": 2 * r, "cos_i": 2 * r * (1 / nf + 1 / ni), "cos_e": 2 * r * (1 / nf + 1 / ne)}


def test_series_bf16x6_within_the_derived_caps():
    """2. bf16x6 picks its kernels by batch size: no exactness, the caps of tests/test_gpu_vis.py with the norms of the padded forward."""
    want, nf, ni, ne = reference("bf16x6", np.float32)
    got = rows_call(make_model("bf16x6", outputs="scores"), np.float32, similarity=True)["similarity"]
    assert got.shape == (4, N) and bool(torch.isfinite(got).all())
    caps = caps_for(768, nf, ni, ne)
    err = (got - want).abs().double().cpu().numpy()
    worst = {k: float(np.max(err[j] / caps[k])) for j, k in enumerate(KEYS)}
    print("bf16x6 worst |rows - padded| in units of the cap:", worst)
    for k in KEYS:
        assert worst[k] <= 1.0, (k, worst[k])


@pytest.mark.parametrize("compute", ["f32", "bf16", "bf16x6"])
def test_logits_and_weight_means_keep_their_bits(compute):
    """3. Keeping fused / mu changes no score: the same call with and without `similarity`."""
    model = make_model(compute, outputs="scores")
    plain = rows_call(model, np.float32)
    sim = rows_call(model, np.float32, similarity=True)
    again = rows_call(model, np.float32)
    assert "similarity" not in plain
    for k in SCORE_KEYS:
        assert torch.equal(sim[k], plain[k]), (compute, k, float((sim[k] - plain[k]).abs().max()))
        assert torch.equal(again[k], plain[k]), (compute, k)


def assert_scores_as_the_plain_entries(got, want, compute):
    """The host-list entry against the device entry as tests/test_gpu_videos.py holds the plain pair: bit for bit, except the bf16
    mode's weight means, whose row sums the ring and the row-block heads kernels add in different orders (<= 1e-6 there)."""
    for k in SCORE_KEYS:
        if compute == "bf16" and k != "logits":
            assert float((got[k] - want[k]).abs().max()) <= 1e-6, k
        else:
            assert torch.equal(got[k], want[k]), (compute, k)


def host_call(model, vids, **kw):
    with torch.no_grad():
        return model.forward_videos_host([torch.from_numpy(v[0]) for v in vids], [torch.from_numpy(v[1]) for v in vids], EDGE, **kw)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_host_list_entry_equals_the_device_entry(compute):
    """4. batch_chunks = 3: several passes on both internal lanes, each writing at its own row offset with the list's total as stride."""
    model = make_model(compute, outputs="scores")
    want = rows_call(model, np.float32, similarity=True)
    got = host_call(model, videos(np.float32), batch_chunks=3, similarity=True)
    assert set(got) == set(want)
    assert_series_equal(got["similarity"], want["similarity"], ("host list", compute))
    assert_scores_as_the_plain_entries(got, want, compute)
    assert "similarity" not in host_call(model, videos(np.float32), batch_chunks=3)


@pytest.mark.parametrize("plant_nan", [False, True])
def test_host_passes_cut_into_micro_batches_write_at_the_composed_column(plant_nan):
    """4. micro_batch = 2 under batch_chunks = 3: the 1,500-row video starts at a non-zero row of the list and spans three micro-batch
    passes of its host pass, so the series' column is (list offset of the host pass) + (offset of the micro-batch pass in it), both
    above zero.  f32 is bit-identical across pass sizes (`micro_batch=3` above), so the device entry of a default-micro-batch model is
    the reference.  With a NaN in the image rows of that video's third chunk, the per-video flag (scanned pass by pass) must reach
    every pass of the video; `torch.equal` is false on a NaN that got through."""
    vids = videos(np.float32)
    if plant_nan:
        vids = H.with_nan(vids, EDGE.index(1500), 2 * T + 88, 11)
    rows = pack(vids)
    with torch.no_grad():
        want = make_model("f32", outputs="scores").forward_videos(rows[0], rows[1], EDGE, nan_to_num=True, similarity=True)
    got = host_call(make_model("f32", outputs="scores", micro_batch=2), vids, nan_to_num=True, batch_chunks=3, similarity=True)
    assert set(got) == set(want) == set(SCORE_KEYS) | {"similarity"}
    for k in got:
        assert torch.equal(got[k], want[k]), (plant_nan, k, float((got[k] - want[k]).abs().max()))


def test_host_list_entry_on_the_bf16_wire():
    """4. fp32 host rows rounded to bf16 while they are staged: `forward_videos` on torch-rounded rows, as tests/test_gpu_videos.py
    compares the scores."""
    model = make_model("bf16", outputs="scores")
    rows = pack(videos(np.float32))
    with torch.no_grad():
        want = model.forward_videos(rows[0].to(torch.bfloat16), rows[1].to(torch.bfloat16), EDGE, similarity=True)
    got = host_call(model, videos(np.float32), batch_chunks=3, wire_dtype=torch.bfloat16, similarity=True)
    assert_series_equal(got["similarity"], want["similarity"], "bf16 wire")
    assert_scores_as_the_plain_entries(got, want, "bf16")


# ------------------------------------------------------------------------------------------------
# 5. the harness on the config-1 set
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def config1(tmp_path_factory, golden_dir):
    g, args, gt, sd = H.write_config1_set(tmp_path_factory.mktemp("cfg1rows"), golden_dir)
    args = argparse.Namespace(**vars(args), vis_dpi=40)
    return g, args, gt, sd, np.load(os.path.join(golden_dir, "vis_config1.npz"))


def config1_model(sd, **kw):
    a = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=10, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, "cuda", a, **kw)
    m.load_state_dict(sd)
    return m


def test_ucf_test_on_the_valid_row_route(config1, tmp_path, monkeypatch):
    g, args, gt, sd, fix = config1
    monkeypatch.chdir(tmp_path)
    roc, ap = harness.ucf_test(args, config1_model(sd, outputs="scores"), harness.get_test_loader(args), 256, None, gt, "cuda:0", vis=True,
                               vis_route="rows")
    res = harness.ucf_test.last_result
    caps = caps_for(768, fix["norm_f"], fix["norm_i"], fix["norm_e"])
    for k in KEYS:
        assert [len(v) for v in res["similarity"][k]] == list(fix["lengths"])
        err = np.abs(np.concatenate(res["similarity"][k]) - fix[k])
        print(f"rows {k}: worst |HIP - reference| in units of the cap = {np.max(err / caps[k]):.3e}")
        assert (err <= caps[k]).all(), k
    assert np.abs(np.concatenate(res["scores"]) - g["scores"]).max() <= H.TOL_SIGMOID
    assert abs(roc - float(g["roc"])) < 1e-4 and abs(ap - float(g["ap"])) < 1e-4
    files = sorted(res["vis_files"])
    assert files and all(os.path.getsize(p) > 500 for p in files)
    # the padded route with a full-dict model: same keys, same figure files, and in f32 the same bits
    roc_p, ap_p = harness.ucf_test(args, config1_model(sd, outputs="full"), harness.get_test_loader(args), 256, None, gt, "cuda:0", vis=True,
                                   vis_route="padded")
    padded = harness.ucf_test.last_result
    assert set(padded) == set(res) and sorted(padded["vis_files"]) == files
    assert roc_p == roc and ap_p == ap
    for k in KEYS:
        for a, b in zip(res["similarity"][k], padded["similarity"][k]):
            assert np.array_equal(a, b), k
    for a, b in zip(res["scores"], padded["scores"]):
        assert np.array_equal(a, b)
    # the weight means: in-kernel row means here, torch's mean over the full dict's [rows, 768] weights there -- the same 768 fp32
    # values in (0, 1) added in another order: |difference| <= 768 * 2^-24 for any two orders
    for k in ("w_i_mean", "w_e_mean"):
        for a, b in zip(res[k], padded[k]):
            assert np.abs(a - b).max() <= 768 * 2.0 ** -24, k


def test_score_loader_rows_on_two_lanes(config1):
    g, args, gt, sd, fix = config1
    model = config1_model(sd, outputs="scores").to("cuda:0").eval()
    runs = [harness.score_loader(model, harness.get_test_loader(args), 256, "cuda:0", "ucfcrime", batch_chunks=4, host_list=False, lanes=lanes,
                                 similarity="rows") for lanes in (1, 2)]
    assert len(runs[0]) == len(runs[1]) == 5 and runs[0][1] == runs[1][1]
    for k in KEYS:
        assert [len(v) for v in runs[0][4][k]] == list(fix["lengths"])
        for a, b in zip(runs[0][4][k], runs[1][4][k]):
            assert np.array_equal(a, b), k
    for j in (0, 2, 3):
        for a, b in zip(runs[0][j], runs[1][j]):
            assert np.array_equal(a, b), j


def test_nan_rule_precedes_the_reduction():
    """An fp16 video with a NaN and an inf (NaN -> 0, inf -> 65504 on the device, test.py:90-95) among clean ones: the valid-row series
    against the padded route's on the same loader -- finite, and the same bits in f32."""
    lengths = [100, 300, 50]
    vids = [list(synth.make_video(9, i, n, dtype=np.float16)) for i, n in enumerate(lengths)]
    vids[1][0][7, 5] = np.nan
    vids[1][0][260, 11] = np.inf
    vids[1][1][3, 9] = np.nan

    def loader():
        for (img, ev), n in zip(vids, lengths):
            ci, _ = harness.process_split(img, T)
            ce, _ = harness.process_split(ev, T)
            yield torch.tensor(ci).unsqueeze(0), torch.tensor(ce).unsqueeze(0), ("Normal",), torch.tensor([n])

    rows = harness.score_loader(make_model("f32", outputs="scores"), loader(), T, "cuda:0", "ucfcrime", batch_chunks=2, similarity="rows")
    padded = harness.score_loader(make_model("f32", outputs="full"), loader(), T, "cuda:0", "ucfcrime", batch_chunks=2, similarity=True)
    for k in KEYS:
        assert [len(v) for v in rows[4][k]] == lengths
        for a, b in zip(rows[4][k], padded[4][k]):
            assert np.isfinite(a).all() and np.array_equal(a, b), k
    for a, b in zip(rows[0], padded[0]):
        assert np.array_equal(a, b)
