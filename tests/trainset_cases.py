"""The cases of the training-loader fixtures (tests/golden/trainset_*.npz), shared by their generator
(tests/golden/make_golden_trainset.py) and the tests: inputs are regenerated from seeds, the fixtures hold reference results only."""
import os

import numpy as np

from iefvad_amd import synth

SEED = 71
T = 256
LENGTHS = [1, 37, 255, 256, 257, 300, 511, 513, 1500, 7001, 40003]
NCOLS = 32


def sample_cols(D):
    """The fixed sample of 32 columns whose bit patterns a fixture keeps."""
    return np.linspace(0, D - 1, NCOLS).astype(np.int64)


def cases():
    """(name, rows n, dtype, D, modality 0 image / 1 event, video index, edit)"""
    out = []
    for dt in ("f32", "f16"):
        for n in LENGTHS:
            out.append((f"{dt}_{n}", n, dt, 768, 0, len(out), None))
    out.append(("nonfinite_1500", 1500, "f32", 768, 0, len(out), "nonfinite"))
    out.append(("pair_img_700", 700, "f32", 768, 0, 30, None))        # one item: the image file has 700 rows, its event file 300
    out.append(("pair_ev_300", 300, "f32", 768, 1, 30, None))
    out.append(("d512_1000", 1000, "f32", 512, 0, 31, None))
    return out


# rows / columns of the "nonfinite" edit, by segment of the n = 1500 video ((i n) >> 8 boundaries): what each plant must produce
NONFINITE_PLANTS = [(3, 0, 5, np.nan), (10, 0, 9, np.inf), (10, 1, 9, -np.inf), (20, 0, 11, np.inf), (30, 2, 13, -np.inf)]
NONFINITE_EXPECT = {(3, 5): "nan", (10, 9): "nan", (20, 11): "+inf", (30, 13): "-inf"}


def case_input(case):
    name, n, dt, D, modality, index, edit = case
    x = synth.make_video(SEED, index, n, D=D, dtype=np.float16 if dt == "f16" else np.float32)[modality]
    if edit == "nonfinite":
        for seg, off, col, val in NONFINITE_PLANTS:
            x[((seg * n) >> 8) + off, col] = val
    return x


def check_against_fixture(g, case, out, length):
    """`out` [256, D] fp32 against the fixture of `case`: clip length, bit patterns of the sampled columns (NaN positions equal, the
    other elements bit-equal), fp64 row sums (exact: they are sums of the same fp32 values in the same order)."""
    name, n, dt, D = case[:4]
    assert int(length) == int(g[f"{name}/length"]), name
    assert out.dtype == np.float32 and out.shape == (T, D), name
    sample = np.ascontiguousarray(out[:, sample_cols(D)])
    if dt == "f16":
        want = g[f"{name}/bits"].view(np.float16).astype(np.float32)
    else:
        want = g[f"{name}/bits"].view(np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(sample), nan), name
    assert np.array_equal(sample.view(np.uint32)[~nan], np.ascontiguousarray(want).view(np.uint32)[~nan]), name
    with np.errstate(invalid="ignore"):
        assert np.array_equal(out.astype(np.float64).sum(axis=1), g[f"{name}/rowsum"], equal_nan=True), name


# ---- the small lists of trainset_lists.npz: (dataset flavour, rows of (relative path under the set's root, label, image rows, event rows))
LIST_SEED = 72
LIST_BATCH = 2
LIST_TORCH_SEED = 1234
LISTS = {
    "ucfcrime": [("feat/rgb/Abuse/a0__5.npy", "Abuse", 300, 280), ("feat/rgb/Normal/n0__5.npy", "Normal", 40, 40),
                 ("feat/rgb/Arson/rgb_a1__5.npy", "Arson", 257, 100),           # `rgb` twice in one path: replace() takes every occurrence
                 ("feat/rgb/Normal/n1__5.npy", "Normal", 600, 610), ("feat/rgb/Normal/n2__5.npy", "Normal", 256, 256),
                 ("feat/rgb/Robbery/r0__5.npy", "Robbery", 1, 3), ("feat/rgb/Normal/n3__5.npy", "Normal", 90, 90),
                 ("feat/rgb/Stealing/s0__5.npy", "Stealing", 37, 37), ("feat/rgb/Normal/n4__5.npy", "Normal", 511, 500)],
    "msad": [("feat/rgb/Fire/f0__5.npy", "Fire", 270, 270), ("feat/rgb/Normal/m0__5.npy", "Normal", 20, 21),
             ("feat/rgb/Normal/m1__5.npy", "Normal", 400, 300), ("feat/rgb/Assault/x0__5.npy", "Assault", 64, 64),
             ("feat/rgb/Normal/m2__5.npy", "Normal", 256, 257), ("feat/rgb/Robbery/x1__5.npy", "Robbery", 513, 513)],
    "shang": [("feat/rgb/01_001.npy", "normal", 100, 100), ("feat/rgb/01_002.npy", "fighting", 300, 290),
              ("feat/rgb/01_003.npy", "normal", 257, 257), ("feat/rgb/01_004.npy", "Normal", 50, 50),      # not the shang key: abnormal
              ("feat/rgb/01_005.npy", "car", 30, 31), ("feat/rgb/01_006.npy", "normal", 1000, 900)],
    "xd": [("feat/rgb/v0_label_A__5.npy", "A", 300, 300), ("feat/rgb/v1_label_B1-B2__5.npy", "B1-B2", 100, 90),
           ("feat/rgb/v2_label_A__5.npy", "A", 256, 256), ("feat/rgb/v3_label_G-0-0__5.npy", "G-0-0", 700, 720),
           ("feat/rgb/v4_label_A__5.npy", "Normal", 33, 33)],
}
EVENT_DIR = {"ucfcrime": "event_thr_10", "msad": "event_thr_10", "xd": "event_thr_10", "shang": "event"}
FLAGS = {"ucfcrime": (True, False), "msad": (True, False), "shang": (True, False), "xd": (None,)}


def write_list(root, flavour, D=768):
    """The .npy files and the `path,label` csv of one flavour under `root` (a str or Path); returns the csv path."""
    root = str(root)
    lines = []
    for i, (rel, label, n_img, n_ev) in enumerate(LISTS[flavour]):
        p = os.path.join(root, flavour, rel)
        q = p.replace("rgb", EVENT_DIR[flavour])
        os.makedirs(os.path.dirname(p), exist_ok=True)
        os.makedirs(os.path.dirname(q), exist_ok=True)
        dt = np.float16 if i % 4 == 2 else np.float32
        np.save(p, synth.make_video(LIST_SEED, i, n_img, D=D, dtype=dt)[0])
        np.save(q, synth.make_video(LIST_SEED, i, n_ev, D=D, dtype=dt)[1])
        lines.append(f"{p},{label}\n")
    csv = os.path.join(root, flavour, "train.csv")
    with open(csv, "w") as f:
        f.write("path,label\n" + "".join(lines))
    return csv
