"""What the score samples cost: whole `MMFMIL.forward_videos` calls against `MMFMIL.forward_videos_samples` with S = 8 and S = 32
(`iefvad_forward_videos` against `iefvad_forward_videos_samples`; csrc/samples.h) on DEVICE-resident packed rows of

  * the UCF-Crime-sized list of config 2 (290 videos, ~69.5 k snippets, K = 10)
  * the ShanghaiTech + MSAD-sized list of BASELINE config 5 (438 videos, 17,732 snippets, K = 5)

-- the lists of tools/variants_probe.py.  One process; per list and arithmetic (--computes, default f32, bf16x6 and bf16) one warm-up
call of each form, then `--runs` calls of each, ALTERNATING; medians with min - max of the wall clock of whole calls, each ended by a
device synchronise.  Profiler off.  Beside them, for scale, S + 1 plain calls of this tree in a row (what S forwards of an edited
model cost at the least), and the estimate from the FLOP shares alone: 1 + tail share x S plain calls (tail = 46.9 % of a K = 10
forward, 30.6 % of a K = 5 one).  The log goes to profiles/samples_probe.log (or --log PATH) and to stdout.

  --plain-only             only the plain calls (the one form the parent commit has too): run it in a checkout of the parent and in
                           this tree in turn, and compare against the parent's own spread
  --kernel-only            two S = 8 calls per list in f32 and nothing else: run THIS under
                           `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/samples_probe.py --kernel-only`
  --append-stats CSV       append the lines of the three kernels a samples call adds from that run's kernel_stats.csv to the log, with
                           the bytes their launches move over their time (the row kernels of DESIGN.md 4.7 stream at 4.8-6.5 TB/s)."""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "samples_probe.log"))
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--computes", default="f32,bf16x6,bf16")
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--append-stats", default=None)
opt = ap.parse_args()
KERNEL_ONLY_CALLS, KERNEL_ONLY_S = 2, 8
D = 768
SEED = 11
TAIL_SHARE = {10: 0.469, 5: 0.306}


def lists():
    """(name, lengths, K): the same lists in every mode of this tool."""
    from iefvad_amd import synth
    c5 = synth.config5_lists(os.path.join(ROOT, "tests", "golden"))
    shang_msad = [int(n) for d in ("shang", "msad") for n in c5[d][0]]
    ucf = [int(n) for n in synth.lognormal_lengths(1, 290, 69500)]
    assert len(shang_msad) == 438 and sum(shang_msad) == 17732 and len(ucf) == 290
    return (("UCF-sized", ucf, 10), ("Shang + MSAD-sized", shang_msad, 5))


def row_set_rows(lengths):
    """Rows of the row-compressed set the tail of a whole-video call runs on: valid rows + one pad row per partial chunk."""
    rows = 0
    for n in lengths:
        full, rest = divmod(n, 256)
        rows += 256 * full + (rest + 1 if rest else 0)
    return rows


if opt.append_stats:
    groups = KERNEL_ONLY_S // 4
    # (read, written) per call over a row set of `rows` rows and `valid` snippets
    traffic = {
        "iefvad_sample_states_kernel": lambda rows, valid: (groups * rows * D * 4 * 4, groups * rows * D * 4 * 4),
        "iefvad_variants_out_kernel": lambda rows, valid: (KERNEL_ONLY_S * valid * 4, KERNEL_ONLY_S * valid * 4),
        "iefvad_samples_reduce_kernel": lambda rows, valid: (2 * KERNEL_ONLY_S * valid * 4, 2 * valid * 4),      # two passes over the S logits
    }
    out = [f"kernel stats of one `--kernel-only` run under rocprofv3 --kernel-trace --stats ({KERNEL_ONLY_CALLS} S = {KERNEL_ONLY_S} calls per "
           "list, f32):"]
    with open(opt.append_stats) as f:
        for r in csv.DictReader(f):
            for key, fn in traffic.items():
                if key in r["Name"]:
                    rd = sum(KERNEL_ONLY_CALLS * fn(row_set_rows(lengths), sum(lengths))[0] for _, lengths, K in lists())
                    wr = sum(KERNEL_ONLY_CALLS * fn(row_set_rows(lengths), sum(lengths))[1] for _, lengths, K in lists())
                    t = int(r["TotalDurationNs"])
                    out.append(f"  {r['Name']}: {r['Calls']} launches, total {t / 1e3:.1f} us, average {float(r['AverageNs']) / 1e3:.2f} us, "
                               f"min {int(r['MinNs']) / 1e3:.2f} us, max {int(r['MaxNs']) / 1e3:.2f} us; at least {rd / 1e9:.4f} GB read + "
                               f"{wr / 1e9:.4f} GB written = {(rd + wr) / t / 1e3:.3f} TB/s over all its launches")
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


def one_call(model, rows, lengths, S, repeat=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for _ in range(repeat):
            got = model.forward_videos_samples(rows[0], rows[1], lengths, S, SEED) if S else model.forward_videos(rows[0], rows[1], lengths)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, got


say("score samples: forward_videos(rows, lengths) against forward_videos_samples(rows, lengths, S, seed) on device-resident packed rows; "
    "wall clock of whole calls ended by a synchronise, profiler off" + (" -- plain calls only" if opt.plain_only else ""))
for name, lengths, K in lists():
    total = sum(lengths)
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    rows = tuple(torch.randn(total, D, device="cuda:0", generator=gen) for _ in range(2))
    for compute in (["f32"] if opt.kernel_only else opt.computes.split(",")):
        model = model_for(K, compute)
        if opt.kernel_only:
            for _ in range(KERNEL_ONLY_CALLS):
                one_call(model, rows, lengths, KERNEL_ONLY_S)
            continue
        # form -> (S, plain calls in a row): the last two are S + 1 plain calls, for scale
        forms = {"plain": (0, 1)}
        if not opt.plain_only:
            forms.update({"S = 8": (8, 1), "S = 32": (32, 1), "9 plain calls": (0, 9), "33 plain calls": (0, 33)})
        times, last = {tag: [] for tag in forms}, {}
        for tag, (S, rep) in forms.items():
            one_call(model, rows, lengths, S, rep)                         # warm-up: handle, workspace, every shape once
        for _ in range(opt.runs):
            for tag, (S, rep) in forms.items():                            # the forms alternate
                dt, last[tag] = one_call(model, rows, lengths, S, rep)
                times[tag].append(dt)
        say(f"{name} list, compute = {compute}: {len(lengths)} videos, {total} snippets, K = {K}")
        for tag in forms:
            t = [x * 1e3 for x in times[tag]]
            say(f"  {tag:14s}: median {statistics.median(t):8.2f} ms (min {min(t):.2f}, max {max(t):.2f}, {len(t)} runs)")
        if not opt.plain_only:
            mp = statistics.median(times["plain"])
            m8, m32 = statistics.median(times["S = 8"]), statistics.median(times["S = 32"])
            same = all(torch.equal(last["plain"][k], last["S = 32"][k]) for k in ("logits", "w_i_mean", "w_e_mean"))
            say(f"  S = 8 costs {m8 / mp:.2f} plain calls (FLOP estimate {1 + TAIL_SHARE[K] * 8:.2f}; 9 forwards: 9.00), S = 32 costs {m32 / mp:.2f} "
                f"(estimate {1 + TAIL_SHARE[K] * 32:.2f}; 33 forwards: 33.00); logits, w_i_mean, w_e_mean bit-identical to the plain call: {same}; "
                f"median score_std {float(last['S = 32']['score_std'].median()):.4f}")
        del model
    del rows

if not opt.kernel_only:
    os.makedirs(os.path.dirname(os.path.abspath(opt.log)), exist_ok=True)
    with open(opt.log, "w") as f:
        f.write("\n".join(lines) + "\n")
