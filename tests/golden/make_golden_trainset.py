"""Reference captures of the TRAIN-mode data path (the reference's data/tools.py process_feat, data/dataset.py with
test_mode=False, data/__getter__.py get_loader).  Run once on CPU with the reference importable (it needs pandas):

    python tests/golden/make_golden_trainset.py

Only what the reference produced is stored; inputs regenerate from seeds (tests/trainset_cases.py):
  trainset_process_feat.npz  per case: the returned clip length, the output's bit patterns on all 256 rows x 32 sampled columns
                             (fp16 cases as fp16 bits: np.mean of fp16 is fp16, and so is a padded fp16 file) and an fp64 sum of
                             every output row
  trainset_lists.npz         UCF_Dataset / XD_Dataset / Shang_Dataset + get_loader on small temporary lists (ucf, msad, shang, xd
                             flavours): kept rows and labels per (dataset, normal flag), event paths, clip lengths, and the index
                             batches of each loader's first epoch under a recorded torch.manual_seed"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"
sys.path.insert(0, REF)

from tests import trainset_cases as TC  # noqa: E402


def gen_process_feat():
    from data.tools import process_feat            # the reference's
    store = {"names": np.array([c[0] for c in TC.cases()]), "seed": np.array(TC.SEED)}
    with np.errstate(invalid="ignore", over="ignore"):
        for case in TC.cases():
            name, n, dt, D = case[:4]
            x = TC.case_input(case)
            out, length = process_feat(x, TC.T)
            assert out.shape == (TC.T, D)
            sample = np.ascontiguousarray(out[:, TC.sample_cols(D)])
            if dt == "f16":
                assert np.array_equal(sample.astype(np.float16).astype(np.float32), sample.astype(np.float32), equal_nan=True)
                bits = sample.astype(np.float16).view(np.uint16)
            else:
                assert sample.dtype == np.float32
                bits = sample.view(np.uint32)
            store[f"{name}/length"] = np.array(length)
            store[f"{name}/bits"] = bits
            store[f"{name}/rowsum"] = out.astype(np.float64).sum(axis=1)
    path = os.path.join(HERE, "trainset_process_feat.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def gen_lists():
    import data.dataset as ref_ds                  # the reference's
    from data.__getter__ import get_loader
    store = {"torch_seed": np.array(TC.LIST_TORCH_SEED), "batch_size": np.array(TC.LIST_BATCH), "seed": np.array(TC.LIST_SEED)}
    seen = []
    for cls in (ref_ds.UCF_Dataset, ref_ds.XD_Dataset, ref_ds.Shang_Dataset):
        orig = cls.__getitem__

        def rec(self, i, _orig=orig):
            seen.append(int(i))
            return _orig(self, i)
        cls.__getitem__ = rec
    with tempfile.TemporaryDirectory(prefix="iefvad_trainset_") as tmp:
        for flavour in TC.LISTS:
            csv = TC.write_list(tmp, flavour)
            args = argparse.Namespace(dataset=flavour, visual_length=TC.T, train_list=csv, test_list=csv, batch_size=TC.LIST_BATCH)
            torch.manual_seed(TC.LIST_TORCH_SEED)
            loaders = get_loader(args, None)[:-1]                  # the test loader is not this fixture's business
            assert len(loaders) == len(TC.FLAGS[flavour])
            for flag, loader in zip(TC.FLAGS[flavour], loaders):
                ds = loader.dataset
                key = f"{flavour}/{flag}"
                paths = [ds.df.loc[i]["path"] for i in range(len(ds))]
                ev_dir = TC.EVENT_DIR[flavour]
                store[f"{key}/paths"] = np.array([os.path.relpath(p, tmp) for p in paths])
                store[f"{key}/event_paths"] = np.array([os.path.relpath(p.replace("rgb", ev_dir), tmp) for p in paths])
                assert all(os.path.exists(p.replace("rgb", ev_dir)) for p in paths)
                store[f"{key}/labels"] = np.array([ds.df.loc[i]["label"] for i in range(len(ds))])
                items = [ds[i] for i in range(len(ds))]
                store[f"{key}/lengths"] = np.array([int(it[3]) for it in items])
                store[f"{key}/ev_rowsum0"] = np.array([float(it[1].double().sum()) for it in items])   # pins "resampled by its own row count"
                del seen[:]
                batches, labels = [], []
                for b in loader:                                  # first epoch
                    labels.append(list(b[2]))
                    assert b[0].shape[1:] == (TC.T, 768) and b[1].shape[1:] == (TC.T, 768)
                k = 0
                for lb in labels:
                    batches.append(seen[k:k + len(lb)])
                    k += len(lb)
                assert k == len(seen)
                store[f"{key}/batch_sizes"] = np.array([len(b) for b in batches])
                store[f"{key}/batch_indices"] = np.array([i for b in batches for i in b])
                print(key, len(ds), "videos; first epoch", batches)
    path = os.path.join(HERE, "trainset_lists.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    gen_process_feat()
    gen_lists()
