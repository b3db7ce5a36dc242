"""The training input pipeline on the GPU (csrc/resample.h): iefvad_resample_videos against harness.process_feat and the reference
fixture -- BIT for bit, no tolerance: a mismatch means the summation order, the division or the fp16 rounding differs from numpy's --
iefvad_gather_windows against torch.stack, the DeviceTrainSet loaders against DataLoader(TrainFeatureDataset), and miniature
train_paired / train_single runs fed both ways whose final weights must be identical."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import iefvad_amd
from iefvad_amd import harness, lib as L, losses, synth, trainer
from tests import trainset_cases as TC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_windows_equal(got: np.ndarray, want: np.ndarray, what):
    """fp32 arrays: NaN at the same places, every other element the same BITS (so -0.0 != +0.0 here)."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what


def resample_on_gpu(videos):
    """ONE packed call over `videos` (host arrays of one dtype): windows [nv, 256, D] and lengths as numpy."""
    rows = torch.from_numpy(np.concatenate(videos, axis=0)).to(DEV)
    out, lens = trainer.resample_videos(rows, [v.shape[0] for v in videos])
    torch.cuda.synchronize()
    res = out.cpu().numpy(), lens.cpu().numpy()
    del rows, out, lens
    torch.cuda.empty_cache()
    return res


def packed_cases(dt, D):
    return [c for c in TC.cases() if c[2] == dt and c[3] == D]


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("order", ["list", "reversed"])
def test_resample_one_packed_call_holds_every_fixture_length(dt, order):
    """n = 1, 37, 255, 256, 257 ... and the 40,003-row video beside 37-row ones in ONE call: every element bit-equal to the host
    model and to the reference's samples; pad rows exactly +0.0.  Reversed: the longest-first schedule is not visible in the result."""
    g = np.load(os.path.join(GOLDEN, "trainset_process_feat.npz"))
    cases = packed_cases(dt, 768)
    assert {1, 256, 257, 40003} <= {c[1] for c in cases}
    videos = [TC.case_input(c) for c in cases]
    extra = [synth.make_video(TC.SEED, 100 + i, 37, dtype=videos[0].dtype)[0] for i in range(3)]      # short videos around the long one
    videos = videos + extra
    names = cases + [None] * len(extra)
    if order == "reversed":
        videos, names = videos[::-1], names[::-1]
    out, lens = resample_on_gpu(videos)
    for k, (x, case) in enumerate(zip(videos, names)):
        want, n = harness.process_feat(x, 256)
        assert int(lens[k]) == n == min(x.shape[0], 256)
        assert_windows_equal(out[k], want, (dt, order, k, x.shape[0]))
        if x.shape[0] < 256:
            pad = out[k, x.shape[0]:]
            assert not pad.any() and not np.signbit(pad).any()
        if case is not None:
            TC.check_against_fixture(g, case, out[k], lens[k])


def test_resample_nonfinite_values_follow_the_arithmetic():
    case = next(c for c in TC.cases() if c[6] == "nonfinite")
    out, _ = resample_on_gpu([TC.case_input(case)])
    for (seg, col), kind in TC.NONFINITE_EXPECT.items():
        v = out[0, seg, col]
        assert {"nan": np.isnan(v), "+inf": v == np.inf, "-inf": v == -np.inf}[kind], (seg, col, v)
    assert np.isnan(out).sum() == 2 and np.isinf(out).sum() == 2


@pytest.mark.parametrize("dt", [np.float32, np.float16])
def test_resample_at_d512(dt):
    g = np.load(os.path.join(GOLDEN, "trainset_process_feat.npz"))
    case = next(c for c in TC.cases() if c[3] == 512)
    videos = [synth.make_video(TC.SEED, 200 + i, n, D=512, dtype=dt)[i % 2] for i, n in enumerate([1, 256, 257, 37, 5000, 300, 513])]
    if dt == np.float32:
        videos.append(TC.case_input(case))
    out, lens = resample_on_gpu(videos)
    for k, x in enumerate(videos):
        want, n = harness.process_feat(x, 256)
        assert int(lens[k]) == n
        assert_windows_equal(out[k], want, (dt, k, x.shape[0]))
    if dt == np.float32:
        TC.check_against_fixture(g, case, out[-1], lens[-1])


def test_resample_minus_zero_and_single_row_segments():
    """np.mean starts at +0: a segment of -0.0 rows gives +0.0, while the pad branch copies -0.0 as it is."""
    long = np.full((300, 8), -0.0, dtype=np.float32)
    short = np.full((5, 8), -0.0, dtype=np.float32)
    out, _ = resample_on_gpu([long, short])
    assert not np.signbit(out[0]).any()
    assert np.signbit(out[1, :5]).all() and not np.signbit(out[1, 5:]).any()
    assert_windows_equal(out[0], harness.process_feat(long, 256)[0], "long")
    assert_windows_equal(out[1], harness.process_feat(short, 256)[0], "short")


def test_gather_windows_equals_stack():
    gen = torch.Generator().manual_seed(11)
    N, D = 9, 768
    img = torch.randn(N, 256, D, generator=gen).to(DEV)
    ev = torch.randn(N, 256, D, generator=gen).to(DEV)
    img[2, 7, 5] = float("nan")
    lens = torch.tensor([256, 37, 1, 255, 256, 100, 64, 200, 13], dtype=torch.int32, device=DEV)
    keep = bits(img).clone()
    for index in ([4], [int(i) for i in torch.randint(0, N, (128,), generator=gen)], [3, 3, 3, 0, 8, 8]):
        a, b, ln = trainer.gather_windows(img, ev, lens, index)
        assert a.data_ptr() != img.data_ptr() and a.shape == (len(index), 256, D)
        assert torch.equal(bits(a), bits(torch.stack([img[i] for i in index])))
        assert torch.equal(bits(b), bits(torch.stack([ev[i] for i in index])))
        assert ln.dtype == torch.int32 and ln.tolist() == [int(lens[i]) for i in index]
    a, b, ln = trainer.gather_windows(img[:, :, :512].contiguous(), ev[:, :, :512].contiguous(), lens, [8, 0])       # D = 512
    assert torch.equal(bits(a), bits(img[[8, 0]][:, :, :512])) and torch.equal(bits(b), bits(ev[[8, 0]][:, :, :512]))
    for bad in ([N], [0, -1], [0, 1, 99]):
        with pytest.raises(IndexError):
            trainer.gather_windows(img, ev, lens, bad)
    assert torch.equal(bits(img), keep)
    del img, ev, a, b
    torch.cuda.empty_cache()


def write_mixed_set(root, count, seed, labels, nan_at=None, flavour="ucfcrime"):
    """`count` videos of mixed length and dtype (every third file fp16, image and event lengths different on some) under `root`."""
    lengths = [300, 40, 257, 256, 1, 700, 90, 2000, 255, 37, 513, 64, 1500]
    lines = []
    for i in range(count):
        n = lengths[i % len(lengths)] + (i // len(lengths))
        n_ev = n + (7 if i % 5 == 0 else 0) - (3 if i % 7 == 3 and n > 3 else 0)
        dt = np.float16 if i % 3 == 1 else np.float32
        label = labels[i % len(labels)]
        p = os.path.join(str(root), "feat", "rgb", f"v{i:03d}__5.npy")
        q = p.replace("rgb", TC.EVENT_DIR[flavour])
        os.makedirs(os.path.dirname(p), exist_ok=True)
        os.makedirs(os.path.dirname(q), exist_ok=True)
        img = synth.make_video(seed, i, n, dtype=dt)[0]
        ev = synth.make_video(seed, i, n_ev, dtype=dt)[1]
        if nan_at is not None and i == nan_at:
            img[min(3, n - 1), 11] = np.nan
        np.save(p, img)
        np.save(q, ev)
        lines.append(f"{p},{label}\n")
    csv = os.path.join(str(root), "train.csv")
    with open(csv, "w") as f:
        f.write("path,label\n" + "".join(lines))
    return csv


def epoch_of(loader):
    return [(b[0].cpu(), b[1].cpu(), list(b[2]), b[3].cpu().to(torch.int64)) for b in loader]


def test_device_loaders_yield_the_host_loaders_batches(tmp_path):
    """40 videos, mixed dtypes and lengths, one file with a NaN: resident and non-resident device loaders give the batches of
    DataLoader(TrainFeatureDataset) bit for bit over a whole epoch under one seed; the cached set survives the NaN rule."""
    csv = write_mixed_set(tmp_path, 40, 81, ["Normal", "Arson", "Abuse"], nan_at=9)
    ds = harness.TrainFeatureDataset(256, csv, "ucfcrime")
    torch.manual_seed(5)
    want = epoch_of(DataLoader(ds, batch_size=8, shuffle=True, drop_last=False))
    assert len(want) == 5 and any(torch.isnan(b[0]).any() for b in want)
    sets = {"resident": trainer.DeviceTrainSet(ds, DEV, staging_bytes=6 << 20),         # several groups; video 7 (2000 rows) alone exceeds it
            "streamed": trainer.DeviceTrainSet(ds, DEV, resident=False, staging_bytes=6 << 20)}
    assert sets["streamed"].img is None and sets["resident"].img.shape == (40, 256, 768)
    cached = [bits(t).clone() for t in (sets["resident"].img, sets["resident"].ev, sets["resident"].lengths)]
    for name, dset in sets.items():
        loader = dset.loader(8, shuffle=True, drop_last=False)
        assert len(loader) == 5 and loader.batch_size == 8
        torch.manual_seed(5)
        fired = 0
        for k, (img, ev, labels, lens) in enumerate(loader):
            assert img.is_cuda and img.dtype == torch.float32 and lens.dtype == torch.int32 and isinstance(labels, list)
            assert torch.equal(torch.isnan(img).cpu(), torch.isnan(want[k][0])), (name, k)
            assert torch.equal(bits(torch.nan_to_num(img, nan=0.0).cpu()), bits(torch.nan_to_num(want[k][0], nan=0.0))), (name, k)
            assert torch.equal(bits(ev.cpu()), bits(want[k][1])), (name, k)
            assert labels == want[k][2] and lens.cpu().tolist() == want[k][3].tolist(), (name, k)
            had_nan = bool(torch.isnan(img).any())
            a, b = trainer._nan_rule_pair(img, ev)                     # the trainers' in-place repair, on the step's own tensors
            if had_nan:
                fired += 1
                assert a.data_ptr() == img.data_ptr() and not torch.isnan(a).any()
        assert fired == 1, name
    for t, c in zip((sets["resident"].img, sets["resident"].ev, sets["resident"].lengths), cached):
        assert torch.equal(bits(t), c)                                 # the repair never reached the cached windows
    assert torch.isnan(sets["resident"].img[9]).sum() == 1
    # drop_last and no shuffle follow the DataLoader too
    torch.manual_seed(6)
    want = epoch_of(DataLoader(ds, batch_size=16, shuffle=False, drop_last=True))
    got = epoch_of(sets["resident"].loader(16, shuffle=False, drop_last=True))
    assert len(got) == len(want) == 2 and all(torch.equal(bits(torch.nan_to_num(g[0])), bits(torch.nan_to_num(w[0]))) and g[2] == w[2]
                                              for g, w in zip(got, want))
    with pytest.raises(trainer.TrainSetTooLarge, match=str(40 * (2 * 256 * 768 * 4 + 4))):
        trainer.DeviceTrainSet(ds, DEV, budget_bytes=1 << 20)
    with pytest.raises(IndexError):
        sets["resident"].batch([40])
    del sets, cached
    torch.cuda.empty_cache()


def make_model(wseed, L, K, noise, nu):
    sd = synth.make_state_dict(wseed, 768, L, K)
    args = argparse.Namespace(visual_layers=L, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model=noise, nu=nu)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, L, 8, 10, 10, "cuda", args)
    m.load_state_dict(sd)
    m = m.to(DEV)
    for a in list(m.temporal.image_attn_layers) + list(m.temporal.event_attn_layers):
        a.dropout = 0.0
    return m


def eval_items(seed):
    items, lens = [], [300, 40, 256, 100] + [30] * 12
    for i, n in enumerate(lens):
        img, ev = synth.make_video(seed, i, n)
        ci, _ = harness.process_split(img, 256)
        ce, _ = harness.process_split(ev, 256)
        items.append((torch.from_numpy(ci).unsqueeze(0), torch.from_numpy(ce).unsqueeze(0), (synth.UCF_CLASSES[i % 14],), torch.tensor([n])))
    return items, synth.make_gt(seed, sum(lens))


def assert_same_state(a, b):
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert torch.equal(a[k].contiguous().reshape(-1).view(torch.uint8), b[k].contiguous().reshape(-1).view(torch.uint8)), k


def test_paired_training_fed_by_the_device_set_is_bit_identical(tmp_path, monkeypatch):
    """A miniature trainer.train_paired (two epochs, evaluation every 4 samples, best checkpoint, reload) fed by DeviceTrainSet
    loaders, resident and streamed, and by the host DataLoader(TrainFeatureDataset): same seeds, identical final weights -- the step
    is bit-reproducible, so any difference would be the loader's."""
    monkeypatch.chdir(tmp_path)
    csv = write_mixed_set(tmp_path, 12, 82, ["Normal", "Arson"], nan_at=4)
    label_map = {c: c.lower() for c in synth.UCF_CLASSES}
    test_items, gt = eval_items(63)
    args = argparse.Namespace(dataset="ucfcrime", visual_length=256, lr=2e-5, scheduler_milestones=[1], scheduler_rate=0.1, max_epoch=2,
                              print_steps=4, noise_model="StudentT", train_list=csv, batch_size=2)
    results = {}
    for kind in ("host", "resident", "streamed"):
        args.exp_name = f"mini_{kind}"
        model = make_model(38, 1, 1, "StudentT", 8)
        opt = losses.AdamW(model.parameters(), lr=args.lr)
        torch.manual_seed(21)
        if kind == "host":
            normal, abnormal = harness.get_train_loaders(args)
        else:
            normal, abnormal = trainer.get_device_train_loaders(args, DEV, resident=(kind == "resident"))
        assert len(normal) == 3 and len(abnormal) == 3
        logs = []
        best = trainer.train_paired(args, model, normal, abnormal, test_items, label_map, DEV, gt=gt, log=logs.append, optimizer=opt)
        torch.cuda.synchronize()
        results[kind] = (best, [r["train/loss"] for r in logs], {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                         torch.load(f"checkpoints/mini_{kind}.pth", weights_only=True))
        del model, opt, normal, abnormal
        torch.cuda.empty_cache()
    start = synth.make_state_dict(38, 768, 1, 1)
    assert any(not torch.equal(results["host"][2][k], start[k]) for k in start)              # the runs did train
    for kind in ("resident", "streamed"):
        assert results[kind][0] == results["host"][0] and results[kind][1] == results["host"][1], kind
        assert_same_state(results[kind][2], results["host"][2])
        assert_same_state({k: v.cpu() for k, v in results[kind][3].items()}, {k: v.cpu() for k, v in results["host"][3].items()})


def test_single_loader_training_fed_by_the_device_set_is_bit_identical(tmp_path, monkeypatch):
    """The same for trainer.train_single with the xd flavour (one loader, no drop_last, multi-part labels)."""
    monkeypatch.chdir(tmp_path)
    csv = write_mixed_set(tmp_path, 7, 83, ["A", "B1-B2", "G-0-0", "B5"], flavour="xd")
    label_map = {"A": "normal", "B1": "fighting", "B2": "shooting", "B4": "riot", "B5": "abuse", "B6": "car accident", "G": "explosion"}
    args = argparse.Namespace(dataset="xd", visual_length=256, lr=2e-5, scheduler_milestones=[1], scheduler_rate=0.1, max_epoch=2,
                              print_steps=10 ** 6, noise_model="StudentT", train_list=csv, batch_size=2)
    finals = {}
    for kind in ("host", "resident"):
        args.exp_name = f"xd_{kind}"
        model = make_model(39, 1, 1, "StudentT", 8)
        opt = losses.AdamW(model.parameters(), lr=args.lr)
        torch.manual_seed(22)
        loader = harness.get_train_loaders(args) if kind == "host" else trainer.get_device_train_loaders(args, DEV)
        assert len(loader) == 4 and loader.batch_size == 2
        trainer.train_single(args, model, loader, [], label_map, DEV, gt=np.zeros(1), optimizer=opt)
        torch.cuda.synchronize()
        finals[kind] = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        del model, opt, loader
        torch.cuda.empty_cache()
    start = synth.make_state_dict(39, 768, 1, 1)
    assert any(not torch.equal(finals["host"][k], start[k]) for k in start)
    assert_same_state(finals["resident"], finals["host"])


def test_refusals_through_the_c_abi():
    """Every bad argument is refused by name before anything is launched -- with REAL device buffers this time."""
    lib = L.load_library()
    rows = torch.zeros(305, 768, device=DEV)
    out = torch.full((2, 256, 768), 7.0, device=DEV)
    olen = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def rs(lengths=(300, 5), in_dtype=L.IN_F32, T=256, D=768, ws_bytes=256, rows_off=0, out_off=0):
        arr = (C.c_int32 * len(lengths))(*lengths)
        rc = lib.iefvad_resample_videos(C.c_void_p(rows.data_ptr() + rows_off), in_dtype, arr, len(lengths), T, D, C.c_void_p(ws.data_ptr()), ws_bytes,
                                        C.c_void_p(out.data_ptr() + out_off), C.c_void_p(olen.data_ptr()), st)
        return rc, L.last_error()
    for kw, word in ((dict(T=128), "T = 128"), (dict(D=772), "D = 772"), (dict(in_dtype=L.IN_BF16), "in_dtype 2"), (dict(lengths=(300, 0)), "lengths[1] = 0"),
                     (dict(ws_bytes=100), "workspace too small"), (dict(rows_off=4), "16-byte aligned"), (dict(out_off=8), "16-byte aligned")):
        rc, msg = rs(**kw)
        assert rc != 0 and word in msg, (kw, msg)
    idx = torch.zeros(2, dtype=torch.int32, device=DEV)
    g = lib.iefvad_gather_windows(C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(olen.data_ptr()), 2, C.c_void_p(idx.data_ptr()), 2, 255, 768,
                                  C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(olen.data_ptr()), st)
    assert g != 0 and "T = 255" in L.last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and olen.tolist() == [-1, -1]          # nothing ran
    rc, msg = rs()                                                         # and the good call does
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert olen.tolist() == [256, 5] and bool((out == 0.0).all())
    del rows, out, ws
    torch.cuda.empty_cache()
