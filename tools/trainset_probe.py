#!/usr/bin/env python3
"""Measure the training input pipeline (csrc/resample.h, trainer.DeviceTrainSet) on the MI355X, one part per process:

    python3 tools/trainset_probe.py --part resample     # iefvad_resample_videos: bytes read / time, even and skewed video lengths
    python3 tools/trainset_probe.py --part gather       # iefvad_gather_windows: one B = 128 batch out of a cached set
    python3 tools/trainset_probe.py --part step         # a training step at the reference's UCF batch (128 windows, K = 10, bf16x6) fed by
                                                        # a resident synthetic batch / DeviceTrainSet(resident=True) / (resident=False)
    python3 tools/trainset_probe.py --part host         # no GPU: harness.process_feat and the reference-style per-segment np.mean loop

Every part prints JSON lines.  Device times are torch.cuda events around the call on the current stream after warm-up calls; every
figure is the median of the repeats with their minimum and maximum beside it."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import iefvad_amd  # noqa: E402
from iefvad_amd import harness, losses, synth, trainer  # noqa: E402


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": len(xs)}


def time_calls(fn, warmup, repeats):
    """ms per call: events on the current stream around each call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def part_resample(a):
    dev = torch.device("cuda", 0)
    D = a.D
    lists = {"even": np.full(a.videos, 4096, dtype=np.int64),
             "skewed": synth.lognormal_lengths(7, a.videos * 4, a.videos * 4096, lo=16, hi=40000)}
    res = {}
    for dt, name in ((torch.float32, "fp32"), (torch.float16, "fp16")):
        for kind, lens in lists.items():
            total = int(lens.sum())
            rows = torch.empty(total, D, dtype=dt, device=dev).normal_(0, 0.45)
            out = torch.empty(len(lens), 256, D, dtype=torch.float32, device=dev)
            olen = torch.empty(len(lens), dtype=torch.int32, device=dev)
            ll = [int(n) for n in lens]
            ms = time_calls(lambda: trainer.resample_videos(rows, ll, out, olen), a.warmup, a.repeats)
            read = total * D * rows.element_size()
            wrote = out.numel() * 4
            rec = {"part": "resample", "dtype": name, "lengths": kind, "videos": len(ll), "rows": total, "D": D,
                   "longest": int(lens.max()), "shortest": int(lens.min()), "over_256": int((lens > 256).sum()),
                   "gb_read": read / 1e9, "gb_written": wrote / 1e9, "ms": spread(ms),
                   "tb_per_s_read": read / (statistics.median(ms) * 1e-3) / 1e12,
                   "tb_per_s_read_plus_written": (read + wrote) / (statistics.median(ms) * 1e-3) / 1e12,
                   "note": "a call = table upload + stream wait + one kernel launch"}
            res[(name, kind)] = rec["tb_per_s_read"]
            print(json.dumps(rec), flush=True)
            del rows, out, olen
            torch.cuda.empty_cache()
        print(json.dumps({"part": "resample", "dtype": name, "skewed_over_even": res[(name, "skewed")] / res[(name, "even")]}), flush=True)


def part_gather(a):
    dev = torch.device("cuda", 0)
    D, N, B = a.D, a.set_windows, 128
    img = torch.empty(N, 256, D, device=dev).normal_()
    ev = torch.empty(N, 256, D, device=dev).normal_()
    lens = torch.randint(1, 257, (N,), dtype=torch.int32, device=dev)
    gen = torch.Generator().manual_seed(3)
    index = torch.randint(0, N, (B,), generator=gen).tolist()
    ms = time_calls(lambda: trainer.gather_windows(img, ev, lens, index), a.warmup, a.repeats)
    moved = 2 * 2 * B * 256 * D * 4                       # two sets, read + written
    print(json.dumps({"part": "gather", "set_windows": N, "B": B, "D": D, "mb_moved": moved / 1e6, "ms": spread(ms),
                      "tb_per_s_moved": moved / (statistics.median(ms) * 1e-3) / 1e12,
                      "note": "a call = host index check + index upload + three torch.empty + one kernel launch"}), flush=True)


def write_step_set(root, per_class, seed):
    """2 x per_class videos (Normal / Arson), lognormal lengths (mean ~400 rows, up to 8000), fp32, as a ucfcrime-flavoured list."""
    lens = synth.lognormal_lengths(seed, 2 * per_class, 2 * per_class * 400, lo=16, hi=8000)
    lines = []
    os.makedirs(os.path.join(root, "rgb"), exist_ok=True)
    os.makedirs(os.path.join(root, "event_thr_10"), exist_ok=True)
    for i, n in enumerate(lens):
        img, ev = synth.make_video(seed, i, int(n))
        p = os.path.join(root, "rgb", f"v{i:04d}__0.npy")
        np.save(p, img)
        np.save(p.replace("rgb", "event_thr_10"), ev)
        lines.append(f"{p},{'Normal' if i % 2 == 0 else 'Arson'}\n")
    csv = os.path.join(root, "train.csv")
    with open(csv, "w") as f:
        f.write("path,label\n" + "".join(lines))
    return csv, lens


def part_step(a):
    dev = torch.device("cuda", 0)
    K, half = 10, 64
    margs = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    model = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, "cuda", margs, compute="bf16x6")
    model.load_state_dict(synth.make_state_dict(0, 768, 2, K))
    model = model.to(dev).train()
    for m in list(model.temporal.image_attn_layers) + list(model.temporal.event_attn_layers):
        m.dropout = 0.1
    opt = losses.AdamW(model.parameters(), lr=2e-5)
    label_map = {c: c.lower() for c in synth.UCF_CLASSES}
    prompt = trainer.get_prompt_text(label_map)
    with tempfile.TemporaryDirectory(prefix="iefvad_trainset_probe_") as tmp:
        t0 = time.perf_counter()
        csv, lens = write_step_set(tmp, a.per_class, 9)
        largs = argparse.Namespace(dataset="ucfcrime", visual_length=256, train_list=csv, batch_size=half)
        print(json.dumps({"part": "step", "set": f"{len(lens)} videos, {int(lens.sum())} rows, longest {int(lens.max())}",
                          "write_s": time.perf_counter() - t0}), flush=True)

        def steps_from(normal, abnormal, count):
            """`count` steps of train_paired's body (ucf_train.py:43-106) over the two loaders, re-opened when they run out."""
            done = 0
            while done < count:
                n_it, a_it = iter(normal), iter(abnormal)
                for _ in range(min(len(normal), len(abnormal))):
                    n_img, n_ev, n_lab, n_len = next(n_it)
                    a_img, a_ev, a_lab, a_len = next(a_it)
                    img = torch.cat([n_img, a_img], dim=0).to(dev)
                    ev = torch.cat([n_ev, a_ev], dim=0).to(dev)
                    lengths = torch.cat([n_len, a_len], dim=0).to(dev)
                    labels = trainer.get_batch_label(list(n_lab) + list(a_lab), prompt, label_map).to(dev)
                    trainer.train_step(model, opt, img, ev, labels, lengths, "StudentT", 1.0, 1.0, want_terms=False)
                    done += 1
                    if done == count:
                        break

        class Fixed:
            """The baseline of tools/train_step_probe.py: one resident synthetic half batch, handed over again every step."""
            batch_size = half

            def __init__(self, label):
                gen = torch.Generator(device=dev).manual_seed(1)
                self.item = (torch.randn(half, 256, 768, device=dev, generator=gen) * 0.45, torch.randn(half, 256, 768, device=dev, generator=gen) * 0.45,
                             [label] * half, torch.full((half,), 256, dtype=torch.int32, device=dev))

            def __len__(self):
                return 4

            def __iter__(self):
                return iter([self.item] * 4)

        feeds = [("resident synthetic batch (baseline)", lambda: (Fixed("Normal"), Fixed("Arson")))]
        for resident in (True, False):
            def make(resident=resident):
                t1 = time.perf_counter()
                pair = trainer.get_device_train_loaders(largs, dev, resident=resident)
                torch.cuda.synchronize()
                print(json.dumps({"part": "step", "feed": f"DeviceTrainSet(resident={resident})", "construct_s": time.perf_counter() - t1,
                                  "set_gib_on_device": sum(ld.trainset.nbytes for ld in pair) / 2**30 if resident else 0.0}), flush=True)
                return pair
            feeds.append((f"DeviceTrainSet(resident={resident})", make))
        for name, make in feeds:
            normal, abnormal = make()
            steps_from(normal, abnormal, a.warmup)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.repeats):
                t1 = time.perf_counter()
                steps_from(normal, abnormal, a.steps)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t1) / a.steps * 1e3)
            print(json.dumps({"part": "step", "feed": name, "windows": 2 * half, "K": K, "compute": "bf16x6", "steps_per_run": a.steps,
                              "ms_per_step": spread(ms)}), flush=True)
            del normal, abnormal
            torch.cuda.empty_cache()


def mean_per_segment(feat, length=256):
    """The loader pattern this pipeline replaces, as a timing point: one np.mean call per segment, `length` calls per file."""
    n = feat.shape[0]
    if n <= length:
        return harness.process_feat(feat, length)[0]
    r = harness.segment_bounds(n, length)
    return np.stack([np.mean(feat[r[i]:r[i + 1]], 0) for i in range(length)]).astype(np.float32)


def part_host(a):
    lens = synth.lognormal_lengths(9, 2 * a.per_class, 2 * a.per_class * 400, lo=16, hi=8000)[:128]
    vids = [synth.make_video(9, i, int(n)) for i, n in enumerate(lens)]
    for name, fn in (("harness.process_feat", lambda x: harness.process_feat(x, 256)[0]), ("one np.mean call per segment (the pattern this replaces)", mean_per_segment)):
        ms = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for img, ev in vids:
                fn(img)
                fn(ev)
            ms.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"part": "host", "what": name, "batch": f"{len(vids)} videos x 2 modalities, {int(lens.sum())} rows each modality, files already in memory",
                          "cpus": harness.host_cpu_share(), "ms_per_batch": spread(ms)}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--part", required=True, choices=["resample", "gather", "step", "host"])
    p.add_argument("--D", type=int, default=768)
    p.add_argument("--videos", type=int, default=512, help="resample: videos of the even list (4096 rows each)")
    p.add_argument("--set-windows", type=int, default=2048, help="gather: windows in the cached set")
    p.add_argument("--per-class", type=int, default=128, help="step / host: normal and abnormal videos in the synthetic list")
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=20)
    a = p.parse_args()
    {"resample": part_resample, "gather": part_gather, "step": part_step, "host": part_host}[a.part](a)


if __name__ == "__main__":
    main()
