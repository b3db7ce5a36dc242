"""The training input pipeline without a GPU: harness.process_feat against the reference's process_feat (fixture
trainset_process_feat.npz, bit for bit), the segment-boundary identity, TrainFeatureDataset / get_train_loaders against the
reference's Dataset classes and get_loader (trainset_lists.npz), the new C entries' presence and their refusals (every one of them
is decided before anything is launched)."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, lib as L, trainer
from tests import trainset_cases as TC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        L.build_library()
    return L.load_library()


@pytest.mark.parametrize("case", TC.cases(), ids=[c[0] for c in TC.cases()])
def test_process_feat_equals_the_reference_bit_for_bit(case):
    g = np.load(os.path.join(GOLDEN, "trainset_process_feat.npz"))
    assert list(g["names"]) == [c[0] for c in TC.cases()]
    x = TC.case_input(case)
    keep = x.copy()
    out, length = harness.process_feat(x, TC.T)
    assert np.array_equal(x.view(np.uint8), keep.view(np.uint8))                    # the file's rows are not touched
    TC.check_against_fixture(g, case, out, length)
    if case[1] <= TC.T:
        assert not out[case[1]:].any() and not np.signbit(out[case[1]:]).any()      # pad rows are +0.0
    if case[6] == "nonfinite":
        for (seg, col), kind in TC.NONFINITE_EXPECT.items():
            v = out[seg, col]
            assert {"nan": np.isnan(v), "+inf": v == np.inf, "-inf": v == -np.inf}[kind], (seg, col, v)
        assert np.isnan(out).sum() == 2 and np.isinf(out).sum() == 2               # nothing spreads beyond its segment and column


def test_segment_boundaries_equal_linspace():
    """(i n) >> 8 == np.linspace(0, n, 257, dtype=np.int32) -- the identity the kernel's integer boundaries rest on -- and every
    segment of an n > 256 video has at least one row (uniform_extract's r[i] == r[i+1] branch is dead)."""
    rng = np.random.default_rng(3)
    ns = list(range(257, 20001)) + [int(v) for v in rng.integers(20001, 5_000_001, 4000)] + [5_000_000]
    i = np.arange(257, dtype=np.int64)
    for n in ns:
        r = np.linspace(0, n, 257, dtype=np.int32)
        assert np.array_equal((i * n) >> 8, r), n
        assert np.array_equal(harness.segment_bounds(n), r), n
        assert (np.diff(r) >= 1).all(), n
    with pytest.raises(ValueError, match="power-of-two"):
        harness.segment_bounds(1000, 100)


def test_process_feat_vectorised_form_is_the_per_segment_mean():
    """The restatement adds row j of every segment in one operation; per output element that is np.mean's own order."""
    rng = np.random.default_rng(5)
    for n, dt in ((777, np.float32), (2049, np.float16), (258, np.float32)):
        x = (rng.standard_normal((n, 64)) * 2).astype(dt)
        out, length = harness.process_feat(x, 256)
        r = np.linspace(0, n, 257, dtype=np.int32)
        want = np.stack([np.mean(x[r[k]:r[k + 1]], 0) for k in range(256)]).astype(np.float32)
        assert length == 256 and np.array_equal(out.view(np.uint32), want.view(np.uint32))


def flavour_args(tmp_path, flavour):
    csv = TC.write_list(tmp_path, flavour)
    return argparse.Namespace(dataset=flavour, visual_length=TC.T, train_list=csv, batch_size=TC.LIST_BATCH)


@pytest.mark.parametrize("flavour", list(TC.LISTS))
def test_train_dataset_and_loaders_reproduce_the_reference(tmp_path, flavour):
    g = np.load(os.path.join(GOLDEN, "trainset_lists.npz"))
    assert int(g["batch_size"]) == TC.LIST_BATCH and int(g["torch_seed"]) == TC.LIST_TORCH_SEED
    args = flavour_args(tmp_path, flavour)
    torch.manual_seed(TC.LIST_TORCH_SEED)
    loaders = harness.get_train_loaders(args)
    if flavour == "xd":
        assert isinstance(loaders, torch.utils.data.DataLoader) and not loaders.drop_last
        loaders = (loaders,)
    else:
        assert len(loaders) == 2 and all(ld.drop_last for ld in loaders)
    for flag, loader in zip(TC.FLAGS[flavour], loaders):
        key = f"{flavour}/{flag}"
        ds = loader.dataset
        assert isinstance(ds, harness.TrainFeatureDataset) and loader.batch_size == TC.LIST_BATCH
        assert [os.path.relpath(p, tmp_path) for p in ds.paths] == list(g[f"{key}/paths"])
        assert [os.path.relpath(ds.event_path(i), tmp_path) for i in range(len(ds))] == list(g[f"{key}/event_paths"])
        assert ds.labels == list(g[f"{key}/labels"])
        items = [ds[i] for i in range(len(ds))]
        assert [it[3] for it in items] == list(g[f"{key}/lengths"])
        assert all(it[0].shape == (TC.T, 768) and it[0].dtype == torch.float32 and it[1].dtype == torch.float32 for it in items)
        assert [float(it[1].double().sum()) for it in items] == list(g[f"{key}/ev_rowsum0"])       # the event file by ITS OWN row count
        # first epoch: the same batches (identified by the items' labels and lengths; indices recorded by the fixture)
        sizes, flat = list(g[f"{key}/batch_sizes"]), list(g[f"{key}/batch_indices"])
        got = [(list(b[2]), b[3].tolist()) for b in loader]
        k, want = 0, []
        for s in sizes:
            idx = flat[k:k + s]
            want.append(([ds.labels[i] for i in idx], [items[i][3] for i in idx]))
            k += s
        assert got == want
    # the same sampler arguments drive the device loader's index stream (trainer.DeviceTrainLoader): same seed, same index batches
    torch.manual_seed(TC.LIST_TORCH_SEED)
    for flag, loader in zip(TC.FLAGS[flavour], loaders):
        key = f"{flavour}/{flag}"
        idx_loader = torch.utils.data.DataLoader(list(range(len(loader.dataset))), batch_size=loader.batch_size, shuffle=True,
                                                 drop_last=loader.drop_last)
        assert [i for b in idx_loader for i in b.tolist()] == list(g[f"{key}/batch_indices"])


def test_train_dataset_filter_rules(tmp_path):
    csv = TC.write_list(tmp_path, "shang")
    whole = harness.TrainFeatureDataset(256, csv, "shang")
    assert len(whole) == len(TC.LISTS["shang"])                                       # normal=None: the whole list
    assert harness.TrainFeatureDataset(256, csv, "shang", normal=True).labels == ["normal"] * 3
    assert "Normal" in harness.TrainFeatureDataset(256, csv, "shang", normal=False).labels      # 'Normal' is not shang's key
    assert len(harness.TrainFeatureDataset(256, csv, "xd", normal=True)) == len(whole)          # XD_Dataset has no filter
    with pytest.raises(ValueError, match="not supported"):
        harness.TrainFeatureDataset(256, csv, "avenue")
    with pytest.raises(ValueError, match="not supported"):
        harness.get_train_loaders(argparse.Namespace(dataset="avenue", visual_length=256, train_list=csv, batch_size=2))


def test_new_symbols_are_exported_and_bound(lib):
    for s in ("iefvad_resample_workspace_bytes", "iefvad_resample_videos", "iefvad_gather_windows"):
        assert s in L.SYMBOLS and hasattr(lib, s)
        assert getattr(lib, s).argtypes is not None
    assert lib.iefvad_abi_version() == 8 == L.ABI_VERSION
    assert lib.iefvad_resample_workspace_bytes(0) == 0 and lib.iefvad_resample_workspace_bytes(-3) == 0
    assert lib.iefvad_resample_workspace_bytes(1) == 256 and lib.iefvad_resample_workspace_bytes(17) == 512     # 16 bytes per video
    assert len(lib.iefvad_resample_videos.argtypes) == 11 and len(lib.iefvad_gather_windows.argtypes) == 12


def resample_rc(lib, rows=0x1000, in_dtype=L.IN_F32, lengths=(300, 5), nv=None, T=256, D=768, ws=0x2000, ws_bytes=256, out=0x3000,
                out_len=0x4000):
    """The pointers are never dereferenced: every call here is refused before the library touches the device."""
    arr = (C.c_int32 * len(lengths))(*lengths) if lengths is not None else None
    rc = lib.iefvad_resample_videos(C.c_void_p(rows), in_dtype, arr, len(lengths) if nv is None else nv, T, D, C.c_void_p(ws), ws_bytes,
                                    C.c_void_p(out), C.c_void_p(out_len), None)
    return rc, L.last_error()


def test_resample_refusals_name_the_argument(lib):
    for kw, word in ((dict(T=128), "T = 128"), (dict(T=257), "T = 257"), (dict(D=772), "D = 772"), (dict(D=0), "D = 0"),
                     (dict(in_dtype=L.IN_BF16), "in_dtype 2"), (dict(in_dtype=7), "in_dtype 7"),
                     (dict(lengths=(300, 0)), "lengths[1] = 0"), (dict(lengths=(-4, 9)), "lengths[0] = -4"),
                     (dict(ws_bytes=255), "workspace too small (255 < 256"), (dict(lengths=tuple([9] * 17), ws_bytes=256), "workspace too small"),
                     (dict(rows=0x1008), "16-byte aligned"), (dict(out=0x3004), "16-byte aligned"), (dict(ws=0x2008), "16-byte aligned"),
                     (dict(out_len=0x4002), "4-byte"), (dict(rows=0), "null argument"), (dict(out=0), "null argument"),
                     (dict(nv=0), "nvideos must be positive")):
        rc, msg = resample_rc(lib, **kw)
        assert rc != 0 and msg.startswith("iefvad_resample_videos:") and word in msg, (kw, msg)


def test_gather_refusals_name_the_argument(lib):
    def rc_of(img=0x1000, ev=0x2000, lens=0x3000, nset=4, index=0x4000, B=2, T=256, D=768, io=0x5000, eo=0x6000, lo=0x7000):
        rc = lib.iefvad_gather_windows(C.c_void_p(img), C.c_void_p(ev), C.c_void_p(lens), nset, C.c_void_p(index), B, T, D, C.c_void_p(io),
                                       C.c_void_p(eo), C.c_void_p(lo), None)
        return rc, L.last_error()
    for kw, word in ((dict(T=255), "T = 255"), (dict(D=516), "D = 516"), (dict(nset=0), "nset = 0"), (dict(B=0), "B = 0"),
                     (dict(B=70000), "B = 70000"), (dict(img=0x1004), "16-byte aligned"), (dict(eo=0x6008), "16-byte aligned"),
                     (dict(index=0x4001), "4-byte"), (dict(ev=0), "null argument"), (dict(lo=0), "null argument")):
        rc, msg = rc_of(**kw)
        assert rc != 0 and msg.startswith("iefvad_gather_windows:") and word in msg, (kw, msg)


def test_python_side_refusals_need_no_gpu(tmp_path):
    s = torch.zeros(3, 256, 8)
    lens = torch.zeros(3, dtype=torch.int32)
    for bad in ([3], [-1], [0, 1, 5], []):
        with pytest.raises(IndexError):
            trainer.gather_windows(s, s, lens, bad)                 # decided on the host, before the tensors are even looked at
    with pytest.raises(ValueError, match="device tensor"):
        trainer.resample_videos(torch.zeros(5, 8), [5])
    ds = harness.TrainFeatureDataset(256, TC.write_list(tmp_path, "xd"), "xd")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        trainer.DeviceTrainSet(ds, "cpu")
