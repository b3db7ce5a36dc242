"""The full output dict of an evaluation list on its two routes (harness.score_loader):

  * padded      an outputs="full" model on whole 256-row chunks (`ragged=False`): every forward writes the seven [rows, 768] tensors of
                its chunks, pad rows included; nothing D-wide is kept or sliced here, so this is the route's floor; batch_chunks = 64
  * valid rows  `row_outputs="full"`: an outputs="scores" model, the host-list walk (`iefvad_forward_videos_host_full`), every pass
                copies the valid rows of the seven tensors to the caller's packed tensors (`iefvad_rows_out_wide_kernel`), which
                stay on the device; batch_chunks = 64

on the ShanghaiTech + MSAD-sized list of BASELINE config 5 (438 videos, 17,732 snippets, K = 5) and the UCF-Crime-sized list of
config 2 (290 videos, ~69.5 k snippets, K = 10) -- the lists of tools/vis_rows_probe.py.  One process; per list and arithmetic
(--computes, default f32 and bf16) one warm-up call of each route, then `--runs` calls of each, ALTERNATING; medians with min - max of
the wall clock of whole calls (loader walk, staging, copies, forwards, the scores' read-back).  Profiler off.  The log goes to
profiles/videos_full_probe.log (or --log PATH) and to stdout.

  --kernel-only            two `row_outputs="full"` calls per list in f32 and nothing else: run THIS under
                           `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/videos_full_probe.py --kernel-only`
                           (no counters in that run)
  --append-stats CSV       append the copy kernel's line of that run's kernel_stats.csv to the log, with the bytes its launches move
                           over their time (the row kernels of DESIGN.md 4.7 stream at 4.8-6.5 TB/s)."""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "videos_full_probe.log"))
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--computes", default="f32,bf16")
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--append-stats", default=None)
opt = ap.parse_args()
KERNEL_ONLY_CALLS = 2


def lists():
    """(name, lengths, K): the same lists in every mode of this tool."""
    from iefvad_amd import synth
    c5 = synth.config5_lists(os.path.join(ROOT, "tests", "golden"))
    shang_msad = [int(n) for d in ("shang", "msad") for n in c5[d][0]]
    ucf = [int(n) for n in synth.lognormal_lengths(1, 290, 69500)]
    assert len(shang_msad) == 438 and sum(shang_msad) == 17732 and len(ucf) == 290
    return (("Shang + MSAD-sized", shang_msad, 5), ("UCF-sized", ucf, 10))


def chunk_rows(lengths):
    """rows the padded route computes: the all-zero chunk of a len % 256 == 0 video is skipped (score_loader's skip_empty_chunks)"""
    return sum(256 if n < 256 else (n + 255) // 256 * 256 for n in lengths)


if opt.append_stats:
    cases = lists()
    rows = {}
    with open(opt.append_stats) as f:
        for r in csv.DictReader(f):
            if "rows_out_wide" in r["Name"]:
                rows[r["Name"]] = r
    out = [f"kernel stats of one `--kernel-only` run under rocprofv3 --kernel-trace --stats ({KERNEL_ONLY_CALLS} row_outputs=\"full\" calls per "
           "list, f32):"]
    # the kernel reads and writes the seven tensors' valid rows once per call: 2 x 7 x rows x 768 floats
    moved = sum(KERNEL_ONLY_CALLS * 2 * 7 * sum(lengths) * 768 * 4 for _, lengths, _ in cases)
    for name, r in rows.items():
        t = int(r["TotalDurationNs"])
        out.append(f"  {name}: {r['Calls']} launches, total {t / 1e3:.1f} us, average {float(r['AverageNs']) / 1e3:.2f} us, "
                   f"min {int(r['MinNs']) / 1e3:.2f} us, max {int(r['MaxNs']) / 1e3:.2f} us; {moved / 1e9:.3f} GB read + written = "
                   f"{moved / t / 1e3:.2f} TB/s over all its launches")
    with open(opt.log, "a") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import iefvad_amd  # noqa: E402
from iefvad_amd import harness, synth  # noqa: E402

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def model_for(K, outputs, compute):
    a = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, "cuda", a, outputs=outputs, compute=compute)
    m.load_state_dict(synth.make_state_dict(7, 768, 2, K))
    return m.to("cuda:0").eval()


def items(lengths, seed=3):
    for i, n in enumerate(lengths):
        img, ev = synth.make_video(seed, i, n)
        ci, _ = harness.process_split(img, 256)
        ce, _ = harness.process_split(ev, 256)
        yield torch.tensor(ci).unsqueeze(0), torch.tensor(ce).unsqueeze(0), ("Normal",), torch.tensor([n])


def one_call(model, data, kw):
    harness.score_loader.last_result = None               # the previous call's [N, 768] tensors are not part of this one's footprint
    t0 = time.perf_counter()
    got = harness.score_loader(model, data, 256, "cuda:0", "ucfcrime", batch_chunks=64, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, got


say("full output dict of a list: score_loader(ragged=False) [padded, outputs=\"full\": seven [rows, 768] tensors written per forward, none "
    "kept] against score_loader(row_outputs=\"full\") [valid rows, outputs=\"scores\", host list, seven [N, 768] tensors left on the "
    "device]; batch_chunks = 64; wall clock of whole calls, profiler off")
for name, lengths, K in lists():
    total = sum(lengths)
    data = list(items(lengths))
    for compute in (["f32"] if opt.kernel_only else opt.computes.split(",")):
        routes = {"valid rows": (model_for(K, "scores", compute), dict(row_outputs="full"))}
        if opt.kernel_only:
            for _ in range(KERNEL_ONLY_CALLS):
                one_call(routes["valid rows"][0], data, routes["valid rows"][1])
            continue
        routes["padded"] = (model_for(K, "full", compute), dict(ragged=False))
        times, last = {tag: [] for tag in routes}, {}
        for tag in routes:
            one_call(routes[tag][0], data, routes[tag][1])          # warm-up: handles, workspaces, staging, every shape once
        for _ in range(opt.runs):
            for tag in ("padded", "valid rows"):                      # the two routes alternate
                dt, last[tag] = one_call(routes[tag][0], data, routes[tag][1])
                times[tag].append(dt)
        worst_score = float(np.abs(np.concatenate(last["padded"][0]) - np.concatenate(last["valid rows"][0])).max())
        kept = harness.score_loader.last_result["row_outputs"]
        assert set(kept) == set(iefvad_amd.OUTPUT_KEYS) - {"logits"} and all(t.shape == (total, 768) and t.is_cuda for t in kept.values())
        say(f"{name} list, compute = {compute}: {len(lengths)} videos, {total} snippets, K = {K}; rows computed and written: padded "
            f"{chunk_rows(lengths)}, valid rows {total} (+ one pad row per chunk computed; "
            f"{100.0 * (1 - total / chunk_rows(lengths)):.0f} % of the chunk rows are padding)")
        for tag in ("padded", "valid rows"):
            t = [x * 1e3 for x in times[tag]]
            say(f"  {tag:10s}: median {statistics.median(t):8.1f} ms per call (min {min(t):.1f}, max {max(t):.1f}, {len(t)} calls)")
        mp, mr = statistics.median(times["padded"]), statistics.median(times["valid rows"])
        say(f"  padded / valid rows = {mp / mr:.2f} x; largest difference between the two routes' scores: {worst_score:.1e}")
        harness.score_loader.last_result = None
        del routes, kept
    del data

if not opt.kernel_only:
    os.makedirs(os.path.dirname(os.path.abspath(opt.log)), exist_ok=True)
    with open(opt.log, "w") as f:
        f.write("\n".join(lines) + "\n")
