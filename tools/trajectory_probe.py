"""What the refinement trajectory costs: whole `MMFMIL.forward_videos` calls with and without `trajectory=True`
(`iefvad_forward_videos` against `iefvad_forward_videos_trajectory`; csrc/trajectory.h) on DEVICE-resident packed rows of

  * the ShanghaiTech + MSAD-sized list of BASELINE config 5 (438 videos, 17,732 snippets, K = 5)
  * the UCF-Crime-sized list of config 2 (290 videos, ~69.5 k snippets, K = 10)

-- the lists of tools/vis_rows_probe.py.  One process; per list and arithmetic (--computes, default f32 and bf16) one warm-up call of
each variant, then `--runs` calls of each, ALTERNATING; medians with min - max of the wall clock of whole calls, each ended by a device
synchronise.  Profiler off.  In f32 the trajectory adds K + 1 launches of `iefvad_step_probe_kernel` per pass; in bf16 it also replaces
the one refinement chain kernel by 2 K GEMM launches (same bits).  The log goes to profiles/trajectory_probe.log (or --log PATH) and
to stdout.

  --kernel-only            two trajectory calls per list in f32 and nothing else: run THIS under
                           `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/trajectory_probe.py --kernel-only`
  --append-stats CSV       append the probe kernel's line of that run's kernel_stats.csv to the log, with the bytes its launches move
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
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "trajectory_probe.log"))
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--computes", default="f32,bf16")
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--append-stats", default=None)
opt = ap.parse_args()
KERNEL_ONLY_CALLS = 2
D = 768


def lists():
    """(name, lengths, K): the same lists in every mode of this tool."""
    from iefvad_amd import synth
    c5 = synth.config5_lists(os.path.join(ROOT, "tests", "golden"))
    shang_msad = [int(n) for d in ("shang", "msad") for n in c5[d][0]]
    ucf = [int(n) for n in synth.lognormal_lengths(1, 290, 69500)]
    assert len(shang_msad) == 438 and sum(shang_msad) == 17732 and len(ucf) == 290
    return (("Shang + MSAD-sized", shang_msad, 5), ("UCF-sized", ucf, 10))


def probe_bytes(rows, K):
    """(read, written) by the K + 1 probe launches of one call over `rows` valid rows: z_0 read and copied; after each step z and z_prev
    read, z stored over z_prev unless it was the last step."""
    return rows * D * 4 * (1 + 2 * K), rows * D * 4 * K


if opt.append_stats:
    found = []
    with open(opt.append_stats) as f:
        for r in csv.DictReader(f):
            if "step_probe" in r["Name"]:
                found.append(r)
    out = [f"kernel stats of one `--kernel-only` run under rocprofv3 --kernel-trace --stats ({KERNEL_ONLY_CALLS} trajectory calls per list, f32):"]
    rd = sum(KERNEL_ONLY_CALLS * probe_bytes(sum(lengths), K)[0] for _, lengths, K in lists())
    wr = sum(KERNEL_ONLY_CALLS * probe_bytes(sum(lengths), K)[1] for _, lengths, K in lists())
    for r in found:
        t = int(r["TotalDurationNs"])
        out.append(f"  {r['Name']}: {r['Calls']} launches, total {t / 1e3:.1f} us, average {float(r['AverageNs']) / 1e3:.2f} us, "
                   f"min {int(r['MinNs']) / 1e3:.2f} us, max {int(r['MaxNs']) / 1e3:.2f} us; {rd / 1e9:.3f} GB read + {wr / 1e9:.3f} GB written = "
                   f"{(rd + wr) / t / 1e3:.2f} TB/s over all its launches")
    with open(opt.log, "a") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))
    sys.exit(0)

import torch  # noqa: E402

import iefvad_amd  # noqa: E402
from iefvad_amd import synth  # noqa: E402

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def model_for(K, compute):
    a = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, D, 256, D, 8, 2, 8, 10, 10, "cuda", a, outputs="scores", compute=compute)
    m.load_state_dict(synth.make_state_dict(7, D, 2, K))
    return m.to("cuda:0").eval()


def one_call(model, rows, lengths, trajectory):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        got = model.forward_videos(rows[0], rows[1], lengths, trajectory=trajectory)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, got


say("refinement trajectory: forward_videos(rows, lengths) against forward_videos(rows, lengths, trajectory=True) on device-resident packed "
    "rows; wall clock of whole calls ended by a synchronise, profiler off")
for name, lengths, K in lists():
    total = sum(lengths)
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    rows = tuple(torch.randn(total, D, device="cuda:0", generator=gen) for _ in range(2))
    for compute in (["f32"] if opt.kernel_only else opt.computes.split(",")):
        model = model_for(K, compute)
        if opt.kernel_only:
            for _ in range(KERNEL_ONLY_CALLS):
                one_call(model, rows, lengths, True)
            continue
        variants = {"scores": False, "trajectory": True}
        times, last = {tag: [] for tag in variants}, {}
        for tag, tr in variants.items():
            one_call(model, rows, lengths, tr)                     # warm-up: handle, workspace, every shape once
        for _ in range(opt.runs):
            for tag, tr in variants.items():                       # the two variants alternate
                dt, last[tag] = one_call(model, rows, lengths, tr)
                times[tag].append(dt)
        same = all(torch.equal(last["scores"][k], last["trajectory"][k]) for k in ("logits", "w_i_mean", "w_e_mean"))
        rd, wr = probe_bytes(total, K)
        say(f"{name} list, compute = {compute}: {len(lengths)} videos, {total} snippets, K = {K}; the {K + 1} probe launches per pass read "
            f"{rd / 1e9:.3f} GB and write {wr / 1e9:.3f} GB per call")
        for tag in variants:
            t = [x * 1e3 for x in times[tag]]
            say(f"  {tag:10s}: median {statistics.median(t):8.2f} ms per call (min {min(t):.2f}, max {max(t):.2f}, {len(t)} calls)")
        ms, mt = statistics.median(times["scores"]), statistics.median(times["trajectory"])
        say(f"  trajectory / scores = {mt / ms:.3f} x (+{(mt - ms) * 1e3:.2f} ms); logits, w_i_mean, w_e_mean bit-identical: {same}; "
            f"delta_norm range {float(last['trajectory']['delta_norm'].min()):.3g} .. {float(last['trajectory']['delta_norm'].max()):.3g}")
        del model
    del rows

if not opt.kernel_only:
    os.makedirs(os.path.dirname(os.path.abspath(opt.log)), exist_ok=True)
    with open(opt.log, "w") as f:
        f.write("\n".join(lines) + "\n")
