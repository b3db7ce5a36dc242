"""vis=True through the HIP path on cuda:0: `harness.test / ucf_test(..., vis=True)` on the config-1 set with an outputs="full" model.
The four similarity series (`iefvad_similarity_rows` on the forward's own `fused` / `image_mu` / `event_mu`) against the reference
model's (tests/golden/vis_config1.npz, test.py:235-238 on the same videos), the scores against the reference capture and against the
vis=False call, the figures written.  `-m gpu`.

Caps per snippet, derived from the suite's gate on the 768-d outputs (each element within H.TOL_BIG of the reference's), not from
what the kernels return:
  |d dist| <= 2 TOL_BIG sqrt(768) = 1.11e-3                                   triangle inequality on two perturbed rows
  |d cos|  <= 2 TOL_BIG sqrt(768) (1 / |fused| + 1 / |mu|)  (<= 1.75e-4 here)   twice the first-order bound, norms from the fixture
tests/test_vis_cpu.py holds the CPU oracle to the same caps."""
import argparse
import math
import os

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness
from tests import helpers as H
from tests import vitb_cases as V

pytestmark = pytest.mark.gpu
KEYS = ("cos_i", "cos_e", "dist_i", "dist_e")


@pytest.fixture(scope="module")
def config1(tmp_path_factory, golden_dir):
    g, args, gt, sd = H.write_config1_set(tmp_path_factory.mktemp("cfg1vis"), golden_dir)
    args = argparse.Namespace(**vars(args), vis_dpi=40)            # small figures: the data is checked through vis_series, not the pixels
    return g, args, gt, sd, np.load(os.path.join(golden_dir, "vis_config1.npz"))


def gpu_model(sd, **kw):
    a = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=10, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, "cuda", a, **kw)
    m.load_state_dict(sd)
    return m


def class_frames(lengths, classes):
    frames = {}
    for n, c in zip(lengths, classes):
        frames[str(c)] = frames.get(str(c), 0) + 16 * int(n)
    return frames


def is_png(path):
    with open(path, "rb") as f:
        return f.read(8) == b"\x89PNG\r\n\x1a\n" and os.path.getsize(path) > 500


@pytest.mark.parametrize("compute", ["f32", "bf16x6"])
def test_root_flavour_series_scores_and_figures(config1, compute, tmp_path, monkeypatch):
    g, args, gt, sd, fix = config1
    monkeypatch.chdir(tmp_path)
    model = gpu_model(sd, outputs="full", compute=compute)
    roc, ap = harness.test(args, model, harness.get_test_loader(args), 256, None, gt, "cuda:0", attn=False, vis=True)
    res = harness.test.last_result
    # the four series against the reference model's
    r = H.TOL_BIG * math.sqrt(768)
    caps = {"dist_i": 2 * r, "dist_e": 2 * r, "cos_i": 2 * r * (1 / fix["norm_f"] + 1 / fix["norm_i"]),
            "cos_e": 2 * r * (1 / fix["norm_f"] + 1 / fix["norm_e"])}
    for k in KEYS:
        assert [len(v) for v in res["similarity"][k]] == list(fix["lengths"])
        err = np.abs(np.concatenate(res["similarity"][k]) - fix[k])
        print(f"{compute} {k}: max |HIP - reference| = {err.max():.3e} (smallest cap {np.min(caps[k]):.3e})")
        assert (err <= caps[k]).all(), k
    # scores and metrics as tests/test_gpu_harness_capture.py gates them
    scores = np.concatenate(res["scores"])
    assert np.abs(scores - g["scores"]).max() <= H.TOL_SIGMOID
    assert abs(roc - float(g["roc"])) < 1e-4 and abs(ap - float(g["ap"])) < 1e-4
    vis_files = list(res["vis_files"])
    if compute == "f32":
        harness.test(args, model, harness.get_test_loader(args), 256, None, gt, "cuda:0", attn=False, vis=False)
        plain = harness.test.last_result
        assert "similarity" not in plain and "vis_files" not in plain
        for a, b in zip(res["scores"], plain["scores"]):          # the padded route vis=True takes and the default route: same bits in f32
            assert np.array_equal(a, b)
    # one class figure per class and page of 3,000 frames, no similarity figure (test.py:190 is commented out)
    want = sorted(os.path.join("vis", args.exp_name, f"{c}_{p + 1}.png")
                  for c, n in class_frames(g["lengths"], g["classes"]).items() for p in range((n + 2999) // 3000))
    assert sorted(vis_files) == want and len(want) > len(set(str(c) for c in g["classes"]))      # some class has a second page
    assert all(is_png(p) for p in vis_files)


def test_ucf_flavour_writes_both_figures_of_every_class(config1, tmp_path, monkeypatch):
    g, args, gt, sd, fix = config1
    monkeypatch.chdir(tmp_path)
    model = gpu_model(sd, outputs="full")
    harness.ucf_test(args, model, harness.get_test_loader(args), 256, None, gt, "cuda:0", vis=True)
    res = harness.ucf_test.last_result
    present = sorted(set(str(c) for c in g["classes"]))
    want = sorted(os.path.join("vis", args.exp_name, f"{pre}{c}.png") for c in present for pre in ("", "similarity_"))
    assert sorted(res["vis_files"]) == want and all(is_png(p) for p in want)
    series = harness.vis_series(res, gt, "ucf_test")
    frames = class_frames(g["lengths"], g["classes"])
    for c in present:
        assert len(series[f"similarity_{c}.png"]["x"]) == len(series[f"{c}.png"]["x"]) == min(frames[c], 3000)
    # the plotted cosine series ARE the collected ones: first video of the first class, every snippet 16 times
    c0 = str(g["classes"][0])
    got = dict(series[f"similarity_{c0}.png"]["panels"][0])["cos_i"]
    n = min(16 * int(g["lengths"][0]), 3000)
    assert np.array_equal(got[:n], np.repeat(res["similarity"]["cos_i"][0], 16)[:n])


def test_scores_only_model_is_refused_by_name(config1, tmp_path, monkeypatch):
    g, args, gt, sd, fix = config1
    monkeypatch.chdir(tmp_path)
    model = gpu_model(sd, outputs="scores")
    with pytest.raises(ValueError, match='outputs="full"'):
        harness.test(args, model, harness.get_test_loader(args), 256, None, gt, "cuda:0", vis=True)
    assert not os.path.exists("vis")


def test_d512_series_equal_the_kernel_on_a_dense_forward(tmp_path, monkeypatch):
    """ViT-B/16 width: the harness's series equal `similarity_rows` over one dense outputs="full" forward of the same chunks (f32:
    every batch composition gives the same bits), indexed by the `[0:len]` slices."""
    g, args, gt, sd = V.write_harness_set(tmp_path)
    args = argparse.Namespace(**vars(args), vis_dpi=40)
    monkeypatch.chdir(tmp_path)
    m = iefvad_amd.MMFMIL(14, V.D, 256, V.D, 8, 2, 8, 10, 10, "cuda", V.model_args(dict(L=2, K=10, lam=0.5, noise="StudentT", nu=8)), outputs="full")
    m.load_state_dict(sd)
    harness.test(args, m, harness.get_test_loader(args), 256, None, gt, "cuda:0", vis=True)
    res = harness.test.last_result
    lengths = [int(n) for n in g["lengths"]]
    for k in KEYS:
        assert [v.shape for v in res["similarity"][k]] == [(n,) for n in lengths]
    chunks, index, off = [], [], 0
    for item in harness.get_test_loader(args):
        img, ev, n = item[0].squeeze(0).reshape(-1, 256, V.D), item[1].squeeze(0).reshape(-1, 256, V.D), int(item[3])
        keep = harness.video_chunks(n, 256)               # without the loader's all-zero chunk
        chunks.append((img[:keep], ev[:keep]))
        index.append(np.arange(off, off + n, dtype=np.int32))
        off += 256 * keep
    with torch.no_grad():
        out = m(torch.cat([c[0] for c in chunks]).cuda(), torch.cat([c[1] for c in chunks]).cuda(), None, None, None)
        dense = harness.similarity_rows(out["fused"], out["image_mu"], out["event_mu"], torch.from_numpy(np.concatenate(index))).cpu().numpy()
    assert dense.shape == (4, sum(lengths)) and np.isfinite(dense).all()
    for j, k in enumerate(KEYS):
        assert np.array_equal(np.concatenate(res["similarity"][k]), dense[j]), k
