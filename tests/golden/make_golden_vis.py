"""Reference capture of the four similarity series that `vis=True` plots (test.py:235-238; train/ucf_test.py:243-247 has the same
four lines).  Run once on CPU with the reference importable:

    python tests/golden/make_golden_vis.py

The reference's MMFMIL (weight seed 11) runs over the config-1 set of make_golden.gen_harness_case -- 16 videos, 4,988 snippets, with
the NaN video, the fp16 video and the lengths 1, 256, 257 and 512 -- through the reference's own loader and the unpacking of
test.py:77-95; the four torch calls are applied to the `[0:len]` rows of every video (test.py:140-151).  Written to vis_config1.npz,
reference outputs only: cos_i, cos_e, dist_i, dist_e and the row norms norm_f, norm_i, norm_e (all [4988] fp32), lengths, classes and
the seeds.  Weights and inputs are regenerated from the seeds by the tests."""
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, build_reference  # noqa: E402
from iefvad_amd import synth  # noqa: E402

SEED, WSEED = 0, 11


def write_set(tmp):
    """The .npy videos of make_golden.gen_harness_case under `tmp`; returns the list csv."""
    rows = []
    for i, (n, c) in enumerate(zip(synth.CONFIG1_LENGTHS, synth.CONFIG1_CLASSES)):
        img, ev = synth.make_video(SEED, i, n)
        if i == 2:
            img[5, 7] = np.nan
        if i == 5:
            img, ev = img.astype(np.float16), ev.astype(np.float16)
        d_rgb = os.path.join(tmp, "feat", "rgb", c)
        os.makedirs(d_rgb, exist_ok=True)
        os.makedirs(os.path.join(tmp, "feat", "event_thr_10", c), exist_ok=True)
        p = os.path.join(d_rgb, f"v{i:03d}__5.npy")
        np.save(p, img)
        np.save(p.replace("rgb", "event_thr_10"), ev)
        rows.append((p, c))
    csv = os.path.join(tmp, "test.csv")
    with open(csv, "w") as f:
        f.write("path,label\n")
        for p, c in rows:
            f.write(f"{p},{c}\n")
    return csv


def gen_vis_case():
    sys.path.insert(0, REF)
    from data.dataset import UCF_Dataset         # the reference's data/dataset.py
    from torch.utils.data import DataLoader
    tmp = tempfile.mkdtemp(prefix="iefvad_vis_")
    loader = DataLoader(UCF_Dataset(256, write_set(tmp), True, None), batch_size=1, shuffle=False)
    model = build_reference(WSEED)
    series = {k: [] for k in ("cos_i", "cos_e", "dist_i", "dist_e", "norm_f", "norm_i", "norm_e")}
    with torch.no_grad():
        for item in loader:
            img, ev, n = item[0].squeeze(0), item[1].squeeze(0), int(item[3])
            if n < 256:
                img, ev = img.unsqueeze(0), ev.unsqueeze(0)
            if torch.isnan(img).any():
                img = torch.nan_to_num(img, nan=0.0)
            if torch.isnan(ev).any():
                ev = torch.nan_to_num(ev, nan=0.0)
            out = model(img, ev, None, None, None)
            fused, image_mu, event_mu = (out[k].reshape(-1, out[k].shape[-1])[0:n].float() for k in ("fused", "image_mu", "event_mu"))
            series["cos_i"].append(F.cosine_similarity(fused, image_mu, dim=-1))
            series["cos_e"].append(F.cosine_similarity(fused, event_mu, dim=-1))
            series["dist_i"].append(torch.norm(fused - image_mu, dim=-1))
            series["dist_e"].append(torch.norm(fused - event_mu, dim=-1))
            series["norm_f"].append(torch.norm(fused, dim=-1))
            series["norm_i"].append(torch.norm(image_mu, dim=-1))
            series["norm_e"].append(torch.norm(event_mu, dim=-1))
    store = {k: torch.cat(v).numpy().astype(np.float32) for k, v in series.items()}
    total = int(sum(synth.CONFIG1_LENGTHS))
    assert all(v.shape == (total,) and np.isfinite(v).all() for v in store.values())
    path = os.path.join(HERE, "vis_config1.npz")
    np.savez_compressed(path, lengths=np.array(synth.CONFIG1_LENGTHS), classes=np.array(synth.CONFIG1_CLASSES), seed=np.array(SEED),
                        wseed=np.array(WSEED), **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB",
          {k: (float(v.min()), float(v.max())) for k, v in store.items()})


if __name__ == "__main__":
    torch.manual_seed(0)
    gen_vis_case()
