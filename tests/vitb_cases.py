"""D = 512 (ViT-B/16 features, head dim 64) cases shared by tests/test_vitb_cpu.py and tests/test_gpu_vitb.py: the reference captures
of tests/golden/make_golden_vitb.py (vitb_*.npz) with their weights and inputs regenerated from the stored seeds."""
import argparse
import os

import numpy as np

from iefvad_amd import synth
from tests import helpers as H

D = 512
FWD_CASES = ["base", "k0_gauss_l1", "f16_k3", "sharp_k3"]     # sharp_*: peaked attention (synth.sharpen_qk by the fixture's factors)


def load_case(name):
    """(capture, cfg, state_dict, img, ev) of vitb_fwd_<name>.npz, as tests/helpers.load_case does for the D = 768 cases."""
    g = np.load(os.path.join(H.GOLDEN, f"vitb_fwd_{name}.npz"))
    wseed, iseed, B, L, K, nu = (int(v) for v in g["meta"])
    cfg = dict(L=L, K=K, nu=nu, lam=float(g["lam"]), noise=str(g["noise"]), B=B, wseed=wseed, iseed=iseed,
               in_dtype=str(g["in_dtype"]), edit=str(g["edit"]))
    img, ev = synth.make_inputs(iseed, B, D=D)
    if cfg["edit"] == "tail":
        img[B - 1, 100:] = 0
        ev[B - 1, 100:] = 0
    if cfg["in_dtype"] == "f16":
        img, ev = img.astype(np.float16), ev.astype(np.float16)
    sd = synth.make_state_dict(wseed, D, L, K)
    if "factors" in g.files:
        sd = synth.sharpen_qk(sd, tuple(float(f) for f in g["factors"]))
    return g, cfg, sd, img, ev


def model_args(cfg):
    return argparse.Namespace(visual_layers=cfg["L"], visual_head=8, num_refinement_steps=cfg["K"], lambda_ref=cfg["lam"],
                              noise_model=cfg["noise"], nu=cfg["nu"])


def write_harness_set(tmp):
    """The .npy videos of vitb_harness.npz under `tmp` (pathlib.Path), as make_golden_vitb.py wrote them for the reference's
    test() run.  Returns (capture, args namespace, gt, state_dict)."""
    g = np.load(os.path.join(H.GOLDEN, "vitb_harness.npz"))
    seed = int(g["seed"])
    rows = []
    for i, (n, c) in enumerate(zip(g["lengths"], g["classes"])):
        img, ev = synth.make_video(seed, i, int(n), D=D)
        d = tmp / "feat" / "rgb" / str(c)
        d.mkdir(parents=True, exist_ok=True)
        (tmp / "feat" / "event_thr_10" / str(c)).mkdir(parents=True, exist_ok=True)
        p = str(d / f"v{i:03d}__5.npy")
        np.save(p, img)
        np.save(p.replace("rgb", "event_thr_10"), ev)
        rows.append((p, str(c)))
    csv = tmp / "test.csv"
    csv.write_text("path,label\n" + "".join(f"{p},{c}\n" for p, c in rows))
    gt = synth.make_gt(seed, int(g["lengths"].sum()))
    sd = synth.make_state_dict(int(g["wseed"]), D)
    args = argparse.Namespace(dataset="ucfcrime", visual_length=256, test_list=str(csv), exp_name="t")
    return g, args, gt, sd
