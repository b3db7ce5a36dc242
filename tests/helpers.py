"""Shared test helpers: golden-case loading and oracle construction (tests may import oracle/)."""
import glob
import os

import numpy as np
import torch

from iefvad_amd import synth
from oracle import iefvad_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BIG_KEYS = ["fused", "image_mu", "event_mu", "image_logvar", "event_logvar", "w_i", "w_e"]

# fp32 gates: the reference (torch CPU fp32) and any other fp32 evaluation order
# differ by <= 2.3e-6 on the 768-d outputs and <= 1e-7 on sigmoid(logit) at these magnitudes.
TOL_BIG = 2e-5
TOL_LOGIT = 2e-5
TOL_SIGMOID = 2e-6


REGIMES = ("flat", "sharp", "over")


def case_regime(name):
    """"flat": make_state_dict's own weights (softmax is an almost flat average over the 256 keys); "sharp" / "over": the q / k rows
    scaled by synth.sharpen_qk with the factors the fixture records (a dominant key per query; scores beyond the range of exp)."""
    head = name.split("_")[0]
    return head if head in REGIMES[1:] else "flat"


def golden_cases(big=False, regimes=REGIMES):
    """Reference-generated forward cases; `big` selects the ones at a full-grid split-kernel batch size (B = 48; the split kernels
    take over from 6 chunks); `regimes` the attention regimes wanted (all by default; the bf16 mode leaves "over" out: its
    bf16-operand noise there is the size of its gate)."""
    names = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "fwd_*.npz")))
    return [n for n in names if ("b48" in n.split("_")) == big and case_regime(n) in regimes]


def load_case(name):
    g = np.load(os.path.join(GOLDEN, f"fwd_{name}.npz"))
    wseed, iseed, B, L, K, nu = (int(v) for v in g["meta"])
    cfg = dict(L=L, K=K, nu=nu, lam=float(g["lam"]), noise=str(g["noise"]), B=B, wseed=wseed, iseed=iseed,
               in_dtype=str(g["in_dtype"]), edit=str(g["edit"]))
    img, ev = synth.make_inputs(iseed, B)
    if cfg["edit"] == "tail":
        img[B - 1, 100:] = 0
        ev[B - 1, 100:] = 0
    elif cfg["edit"] == "allzero":
        img[B - 1] = 0
        ev[B - 1] = 0
    if cfg["in_dtype"] == "f16":
        img, ev = img.astype(np.float16), ev.astype(np.float16)
    sd = synth.make_state_dict(wseed, 768, L, K)
    if "factors" in g.files:
        cfg["factors"] = tuple(float(f) for f in g["factors"])
        sd = synth.sharpen_qk(sd, cfg["factors"])
    return g, cfg, sd, img, ev


def case_gates(g, tols, floors=("floor_big", "floor_logit", "floor_sigmoid")):
    """(768-d, logit, sigmoid) gates of one case: `tols`, and for a fixture that records reference-side floors (the reference's own
    fp32-vs-fp64 distance; for the bf16 mode pass the `bf16_floor_*` fields, the distance of the mode's fp64 emulation from the
    fixture) at least 3 x that floor -- the margin every gate of this suite keeps above its measured floor.  Never derived from
    what a kernel returns."""
    return tuple(max(t, 3.0 * float(g[f])) if f in g.files else t for t, f in zip(tols, floors))


def oracle_cfg(cfg):
    return orc.OracleConfig(num_layers=cfg["L"], num_heads=8, num_refinement_steps=cfg["K"],
                            lambda_ref=cfg["lam"], noise_model=cfg["noise"], nu=cfg["nu"])


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def compare_outputs(out, g, tol_big=TOL_BIG, tol_logit=TOL_LOGIT, tol_sig=TOL_SIGMOID):
    """`out`: dict of numpy arrays with the reference's 8 keys at full shape [B,T,D] / [B,T,1]."""
    tol_big, tol_logit, tol_sig = case_gates(g, (tol_big, tol_logit, tol_sig))
    rows = g["rows"]
    errs = {}
    lg = np.asarray(out["logits"]).reshape(g["logits"].shape)
    errs["logits"] = float(np.abs(lg - g["logits"]).max())
    errs["sigmoid"] = float(np.abs(sigmoid(lg) - sigmoid(g["logits"])).max())
    assert errs["logits"] <= tol_logit, errs
    assert errs["sigmoid"] <= tol_sig, errs
    chunks = g["chunks"] if "chunks" in g.files else None      # big cases keep the 768-d outputs of a few chunks only
    for k in BIG_KEYS:
        a = np.asarray(out[k])
        if chunks is not None:
            a = a[chunks]
        a = a[:, rows, :]
        errs[k] = float(np.abs(a - g[k]).max())
        assert errs[k] <= tol_big, (k, errs)
    return errs


def write_config1_set(tmp, golden_dir=GOLDEN):
    """The synthetic config-1 .npy set written to disk exactly as tests/golden/make_golden.py wrote it for
    the reference's own test() run: 16 videos over the 14 UCF class keys, one NaN element, one fp16 file.
    Returns (golden capture, args namespace, gt, state_dict)."""
    import argparse
    g = np.load(os.path.join(golden_dir, "harness_config1.npz"))
    seed = int(g["seed"])
    rows = []
    for i, (n, c) in enumerate(zip(g["lengths"], g["classes"])):
        img, ev = synth.make_video(seed, i, int(n))
        if i == 2:
            img[5, 7] = np.nan
        if i == 5:
            img, ev = img.astype(np.float16), ev.astype(np.float16)
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
    sd = synth.make_state_dict(int(g["wseed"]))
    args = argparse.Namespace(dataset="ucfcrime", visual_length=256, test_list=str(csv), exp_name="t")
    return g, args, gt, sd


def write_xd_set(tmp, golden_dir=GOLDEN):
    """The XD-shaped .npy set of tests/golden/make_golden.py::gen_harness_xd_case (label CODES in the list, remapped by the
    loop).  Returns (golden capture, args namespace, gt, state_dict, label_map)."""
    import argparse
    g = np.load(os.path.join(golden_dir, "harness_xd.npz"))
    seed = int(g["seed"])
    (tmp / "feat" / "rgb").mkdir(parents=True, exist_ok=True)
    (tmp / "feat" / "event_thr_10").mkdir(parents=True, exist_ok=True)
    rows = []
    for i, (n, c) in enumerate(zip(g["lengths"], g["labels"])):
        img, ev = synth.make_video(seed, i, int(n))
        p = str(tmp / "feat" / "rgb" / f"v{i:03d}_label_{c}__5.npy")
        np.save(p, img)
        np.save(p.replace("rgb", "event_thr_10"), ev)
        rows.append((p, str(c)))
    csv = tmp / "test.csv"
    csv.write_text("path,label\n" + "".join(f"{p},{c}\n" for p, c in rows))
    gt = synth.make_gt(seed, int(g["lengths"].sum()))
    sd = synth.make_state_dict(int(g["wseed"]), 768, 2, int(g["K"]))
    args = argparse.Namespace(dataset="xd", visual_length=256, test_list=str(csv), exp_name="t")
    label_map = {str(k): str(v) for k, v in zip(g["map_keys"], g["map_values"])}
    return g, args, gt, sd, label_map


def with_nan(vids, video, row, col):
    """A copy of a list of (image rows, event rows) numpy pairs with one NaN planted in the image rows of `video`."""
    vids = [(v[0].copy(), v[1].copy()) for v in vids]
    vids[video][0][row, col] = float("nan")
    return vids
