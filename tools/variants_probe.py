"""What the fusion ablations cost: whole `MMFMIL.forward_videos` calls without the keyword, with three variants ("image", "event",
"equal") and with all four (`iefvad_forward_videos` against `iefvad_forward_videos_variants`; csrc/variants.h) on DEVICE-resident
packed rows of

  * the UCF-Crime-sized list of config 2 (290 videos, ~69.5 k snippets, K = 10)
  * the ShanghaiTech + MSAD-sized list of BASELINE config 5 (438 videos, 17,732 snippets, K = 5)

-- the lists of tools/trajectory_probe.py.  One process; per list and arithmetic (--computes, default f32, bf16x6 and bf16) one warm-up
call of each form, then `--runs` calls of each, ALTERNATING; medians with min - max of the wall clock of whole calls, each ended by a
device synchronise.  Profiler off.  Beside them, for scale, the same V scores obtained as V + 1 plain calls of this tree (what four
forwards of an edited model cost at the least).  The log goes to profiles/variants_probe.log (or --log PATH) and to stdout.

  --plain-only             only the calls without the keyword (the one form the parent commit has too): run it in a checkout of the
                           parent and in this tree in turn, and compare against the parent's own spread
  --kernel-only            two four-variant calls per list in f32 and nothing else: run THIS under
                           `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/variants_probe.py --kernel-only`
  --append-stats CSV       append the row kernel's line of that run's kernel_stats.csv to the log, with the bytes its launches move
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
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "variants_probe.log"))
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--computes", default="f32,bf16x6,bf16")
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--append-stats", default=None)
opt = ap.parse_args()
KERNEL_ONLY_CALLS = 2
D = 768
THREE = ("image", "event", "equal")


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


def kernel_bytes(rows, V):
    """(read, written) by the row kernel over a row set of `rows` rows: the four head tensors once, V stacked states."""
    return rows * D * 4 * 4, rows * D * 4 * V


if opt.append_stats:
    found = []
    with open(opt.append_stats) as f:
        for r in csv.DictReader(f):
            if "fusion_variants" in r["Name"]:
                found.append(r)
    out = [f"kernel stats of one `--kernel-only` run under rocprofv3 --kernel-trace --stats ({KERNEL_ONLY_CALLS} four-variant calls per list, f32):"]
    rd = sum(KERNEL_ONLY_CALLS * kernel_bytes(row_set_rows(lengths), 4)[0] for _, lengths, K in lists())
    wr = sum(KERNEL_ONLY_CALLS * kernel_bytes(row_set_rows(lengths), 4)[1] for _, lengths, K in lists())
    for r in found:
        t = int(r["TotalDurationNs"])
        out.append(f"  {r['Name']}: {r['Calls']} launches, total {t / 1e3:.1f} us, average {float(r['AverageNs']) / 1e3:.2f} us, "
                   f"min {int(r['MinNs']) / 1e3:.2f} us, max {int(r['MaxNs']) / 1e3:.2f} us; at least {rd / 1e9:.3f} GB read + {wr / 1e9:.3f} GB "
                   f"written (row sets before rounding to whole tiles) = {(rd + wr) / t / 1e3:.2f} TB/s over all its launches")
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


def one_call(model, rows, lengths, names, repeat=1):
    kw = dict(fusion_variants=names) if names else {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for _ in range(repeat):
            got = model.forward_videos(rows[0], rows[1], lengths, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, got


say("fusion ablations: forward_videos(rows, lengths) against forward_videos(rows, lengths, fusion_variants=...) on device-resident packed "
    "rows; wall clock of whole calls ended by a synchronise, profiler off" + (" -- plain calls only" if opt.plain_only else ""))
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
        # form -> (names, plain calls in a row): the last two are V + 1 plain calls, for scale
        forms = {"plain": (None, 1)}
        if not opt.plain_only:
            forms.update({"three variants": (THREE, 1), "four variants": (True, 1), "4 plain calls": (None, 4), "5 plain calls": (None, 5)})
        times, last = {tag: [] for tag in forms}, {}
        for tag, (names, rep) in forms.items():
            one_call(model, rows, lengths, names, rep)                     # warm-up: handle, workspace, every shape once
        for _ in range(opt.runs):
            for tag, (names, rep) in forms.items():                        # the forms alternate
                dt, last[tag] = one_call(model, rows, lengths, names, rep)
                times[tag].append(dt)
        say(f"{name} list, compute = {compute}: {len(lengths)} videos, {total} snippets, K = {K}")
        for tag in forms:
            t = [x * 1e3 for x in times[tag]]
            say(f"  {tag:14s}: median {statistics.median(t):8.2f} ms (min {min(t):.2f}, max {max(t):.2f}, {len(t)} runs)")
        if not opt.plain_only:
            mp = statistics.median(times["plain"])
            m3, m4 = statistics.median(times["three variants"]), statistics.median(times["four variants"])
            same = all(torch.equal(last["plain"][k], last["four variants"][k]) for k in ("logits", "w_i_mean", "w_e_mean"))
            fused = float((last["four variants"]["logits_variants"][0] - last["four variants"]["logits"]).abs().max())
            say(f"  three variants add {(m3 - mp) / mp:.2f} x of a plain call (+{(m3 - mp) * 1e3:.2f} ms; three more forwards: 3.00 x), four add "
                f"{(m4 - mp) / mp:.2f} x; logits, w_i_mean, w_e_mean bit-identical to the plain call: {same}; max |fused row - logits| = {fused:.3g}")
        del model
    del rows

if not opt.kernel_only:
    os.makedirs(os.path.dirname(os.path.abspath(opt.log)), exist_ok=True)
    with open(opt.log, "w") as f:
        f.write("\n".join(lines) + "\n")
