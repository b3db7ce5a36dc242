"""The twelve-level robustness sweep (harness.PerturbationSweep; the reference's test2.py:29-32,35-123) on the padded route
(`iefvad_forward_scaled` on whole 256-row chunks, outputs="weights", torch sums the [N, 768] weight tensors) against the valid-row
route (`ragged=True`: `iefvad_forward_videos_scaled`, outputs="scores", column sums on the device), on

  * the ShanghaiTech + MSAD-sized list of BASELINE config 5 (438 videos, 17,732 snippets, K = 5), and
  * the UCF-Crime-sized list of config 2 (290 videos, ~69.5 k snippets, K = 10).

One process; each route's constructor (unpack + upload) is timed once; then one warm-up sweep of each route, then `--sweeps` whole
sweeps (the clean pass + twelve levels, statistics and read-backs included) of each, ALTERNATING between the two routes; medians with
min - max.  Profiler off.  The log goes to profiles/sweep_rows_probe.log (or --log PATH) and to stdout.

  --kernel-only            two valid-row sweeps per list and nothing else: run THIS under
                           `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/sweep_rows_probe.py --kernel-only`
  --append-stats CSV       append the column-sum and chunker kernels' lines of that run's kernel_stats.csv to the log, with the bytes
                           the column-sum launches read over their time (the row kernels of DESIGN.md 4.7 stream at 4.8-6.5 TB/s)."""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "sweep_rows_probe.log"))
ap.add_argument("--sweeps", type=int, default=5)
ap.add_argument("--compute", default="f32")
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--append-stats", default=None)
opt = ap.parse_args()


def lists():
    """(name, lengths, K): the same lists in every mode of this tool."""
    from iefvad_amd import synth
    c5 = synth.config5_lists(os.path.join(ROOT, "tests", "golden"))
    shang_msad = [int(n) for d in ("shang", "msad") for n in c5[d][0]]
    ucf = [int(n) for n in synth.lognormal_lengths(1, 290, 69500)]
    assert len(shang_msad) == 438 and sum(shang_msad) == 17732 and len(ucf) == 290
    return (("Shang + MSAD-sized", shang_msad, 5), ("UCF-sized", ucf, 10))


def chunk_rows(lengths):
    """rows of the padded route: process_split's len // 256 + 1 chunks per video"""
    return sum((n // 256 + 1) * 256 if n >= 256 else 256 for n in lengths)


if opt.append_stats:
    cases = lists()
    rows = {}
    with open(opt.append_stats) as f:
        for r in csv.DictReader(f):
            if "colsum" in r["Name"] or "scatter_rows" in r["Name"]:
                rows[r["Name"]] = r
    out = ["kernel stats of one `--kernel-only` run under rocprofv3 --kernel-trace --stats (two valid-row sweeps per list: 26 calls each):"]
    for name, r in rows.items():
        out.append(f"  {name}: {r['Calls']} launches, total {int(r['TotalDurationNs']) / 1e3:.1f} us, average {float(r['AverageNs']) / 1e3:.2f} us, "
                   f"min {int(r['MinNs']) / 1e3:.2f} us, max {int(r['MaxNs']) / 1e3:.2f} us")
    read = sum(2 * 13 * 2 * sum(lengths) * 768 * 4 for _, lengths, _ in cases)      # 2 sweeps x 13 calls x [2, rows, 768] floats per list
    t = sum(int(r["TotalDurationNs"]) for n, r in rows.items() if "colsum_rows" in n)
    if t:
        out.append(f"  iefvad_colsum_rows_kernel: {read / 1e9:.3f} GB read in {t / 1e3:.1f} us = {read / t / 1e3:.2f} TB/s over all its launches "
                   f"(small launches included: a {sum(cases[0][1])}-row call reads {2 * sum(cases[0][1]) * 768 * 4 / 1e6:.0f} MB)")
    with open(opt.log, "a") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))
    sys.exit(0)

import torch  # noqa: E402

import iefvad_amd  # noqa: E402
from iefvad_amd import harness, synth  # noqa: E402

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def model_for(K, outputs):
    a = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, "cuda", a, outputs=outputs, compute=opt.compute)
    m.load_state_dict(synth.make_state_dict(7, 768, 2, K))
    return m.to("cuda:0").eval()


def items(lengths, seed=3):
    for i, n in enumerate(lengths):
        img, ev = synth.make_video(seed, i, n)
        ci, _ = harness.process_split(img, 256)
        ce, _ = harness.process_split(ev, 256)
        yield torch.tensor(ci).unsqueeze(0), torch.tensor(ce).unsqueeze(0), ("Normal",), torch.tensor([n])


def one_sweep(sweep):
    """The clean pass and the twelve levels, every result read back as run_test returns it."""
    sweep._clean = None
    torch.manual_seed(0)
    t0 = time.perf_counter()
    res = [sweep.level(si, se) for _, si, se in harness.sweep_plan()]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


cases, args = lists(), argparse.Namespace(visual_length=256)
say(f"robustness sweep, twelve levels + the clean pass, compute = {opt.compute}; wall clock of whole sweeps, profiler off")
for name, lengths, K in cases:
    total = sum(lengths)
    gt = synth.make_gt(3, total)
    data = list(items(lengths))
    routes = {}
    for tag, ragged, outputs in (("padded", False, "weights"), ("valid rows", True, "scores")):
        t0 = time.perf_counter()
        sweep = harness.PerturbationSweep(args, model_for(K, outputs), data, gt, "cuda:0", ragged=ragged)
        torch.cuda.synchronize()
        routes[tag] = (sweep, time.perf_counter() - t0)
    del data
    if opt.kernel_only:
        for _ in range(2):
            one_sweep(routes["valid rows"][0])
        continue
    times = {tag: [] for tag in routes}
    last = {}
    for tag in routes:
        one_sweep(routes[tag][0])                             # warm-up: handles, workspaces, every shape once
    for _ in range(opt.sweeps):
        for tag in routes:                                    # the two routes alternate
            dt, last[tag] = one_sweep(routes[tag][0])
            times[tag].append(dt)
    worst = max(abs(float(a[i]) - float(b[i])) for a, b in zip(last["padded"], last["valid rows"]) for i in range(10))
    worst_vec = max(float((a[i] - b[i]).abs().max()) for a, b in zip(last["padded"], last["valid rows"]) for i in (10, 11))
    say(f"{name} list: {len(lengths)} videos, {total} snippets, K = {K}; rows per pass: padded {chunk_rows(lengths)}, valid rows {total} "
        f"({100.0 * (1 - total / chunk_rows(lengths)):.0f} % of the chunk rows are padding)")
    for tag in routes:
        t = [x * 1e3 for x in times[tag]]
        say(f"  {tag:10s}: median {statistics.median(t):8.1f} ms per sweep (min {min(t):.1f}, max {max(t):.1f}, {len(t)} sweeps); "
            f"constructor (unpack + upload) {routes[tag][1] * 1e3:.0f} ms once")
    mp, mr = statistics.median(times["padded"]), statistics.median(times["valid rows"])
    say(f"  padded / valid rows = {mp / mr:.2f} x; largest difference between the two routes' results under one seed: scalars {worst:.1e}, "
        f"change vectors {worst_vec:.1e}")

if not opt.kernel_only:
    os.makedirs(os.path.dirname(os.path.abspath(opt.log)), exist_ok=True)
    with open(opt.log, "w") as f:
        f.write("\n".join(lines) + "\n")
