"""What the encoder's head-averaged attention maps cost (`MMFMIL.forward_videos(attn_maps=)`, `iefvad_forward_videos_attn`,
csrc/attention_maps.h): whole `forward_videos` calls on device-resident packed rows of the ShanghaiTech + MSAD-sized list of BASELINE
config 5 (438 videos, 17,732 snippets, K = 5) and the UCF-Crime-sized list of config 2 (290 videos, ~69.5 k snippets, K = 10), f32
arithmetic, three variants:

  * no maps      the plain call (`iefvad_forward_videos`)
  * last layer   attn_maps=[L - 1]: one launch of the maps kernel per pass, two [N, 256] fp32 maps written
  * all layers   attn_maps=True: L launches per pass, 2 L maps

One process; one warm-up call of each variant, then `--runs` calls of each, ALTERNATING; medians with min - max of the wall clock of
whole calls (result allocation, launches, a device synchronisation).  Profiler off.  The log goes to profiles/attn_maps_probe.log (or
--log PATH) and to stdout.

  --plain-only             the "no maps" variant alone (it uses nothing this feature added, so the same file times a checkout of the
                           parent commit on the same box; run the two checkouts in turn); prints, writes no log
  --kernel-only            two attn_maps=True calls per list and nothing else: run THIS under
                           `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/attn_maps_probe.py --kernel-only`
                           (no counters in that run)
  --append-stats CSV       append the maps kernels' lines of that run's kernel_stats.csv to the log, with the bytes their launches
                           write over their time (iefvad_rows_out_wide_kernel streams at 3.58 TB/s, the row kernels of DESIGN.md 4.7
                           at 4.8-6.5 TB/s; this kernel is bound by its matrix work, not by its stores)."""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "attn_maps_probe.log"))
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--append-stats", default=None)
opt = ap.parse_args()
KERNEL_ONLY_CALLS = 2
L_, T = 2, 256


def lists():
    """(name, lengths, K): the same lists in every mode of this tool."""
    from iefvad_amd import synth
    c5 = synth.config5_lists(os.path.join(ROOT, "tests", "golden"))
    shang_msad = [int(n) for d in ("shang", "msad") for n in c5[d][0]]
    ucf = [int(n) for n in synth.lognormal_lengths(1, 290, 69500)]
    assert len(shang_msad) == 438 and sum(shang_msad) == 17732 and len(ucf) == 290
    return (("Shang + MSAD-sized", shang_msad, 5), ("UCF-sized", ucf, 10))


if opt.append_stats:
    found = {}
    with open(opt.append_stats) as f:
        for r in csv.DictReader(f):
            if "attention_maps" in r["Name"]:
                found[r["Name"]] = r
    out = [f"kernel stats of one `--kernel-only` run under rocprofv3 --kernel-trace --stats ({KERNEL_ONLY_CALLS} attn_maps=True calls per "
           "list, f32):"]
    # every call writes L x 2 maps of [N, 256] floats once; the kernel reads q and k of its rows (2 x 768 floats per row and launch)
    written = sum(KERNEL_ONLY_CALLS * L_ * 2 * sum(lengths) * T * 4 for _, lengths, _ in lists())
    total = sum(int(r["TotalDurationNs"]) for r in found.values())
    for name, r in found.items():
        out.append(f"  {name}: {r['Calls']} launches, total {int(r['TotalDurationNs']) / 1e3:.1f} us, average {float(r['AverageNs']) / 1e3:.2f} us, "
                   f"min {int(r['MinNs']) / 1e3:.2f} us, max {int(r['MaxNs']) / 1e3:.2f} us")
    if total:
        out.append(f"  all launches: {written / 1e9:.3f} GB written in {total / 1e3:.1f} us = {written / total / 1e3:.3f} TB/s")
    with open(opt.log, "a") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import iefvad_amd  # noqa: E402
from iefvad_amd import synth  # noqa: E402

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def model_for(K):
    a = argparse.Namespace(visual_layers=L_, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, L_, 8, 10, 10, "cuda", a, outputs="scores", compute="f32")
    m.load_state_dict(synth.make_state_dict(7, 768, L_, K))
    return m.to("cuda:0").eval()


def packed(lengths, seed=3):
    vids = [synth.make_video(seed, i, n) for i, n in enumerate(lengths)]
    return (torch.from_numpy(np.concatenate([v[0] for v in vids])).cuda(), torch.from_numpy(np.concatenate([v[1] for v in vids])).cuda())


def one_call(model, img, ev, lengths, kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        out = model.forward_videos(img, ev, lengths, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


VARIANTS = (("no maps", {}), ("last layer", dict(attn_maps=[L_ - 1])), ("all layers", dict(attn_maps=True)))
if opt.plain_only:
    VARIANTS = VARIANTS[:1]
if opt.kernel_only:
    VARIANTS = VARIANTS[2:]

say("attention maps of a list: MMFMIL.forward_videos on device-resident packed rows, outputs=\"scores\", compute = f32; wall clock of "
    "whole calls, profiler off")
for name, lengths, K in lists():
    total = sum(lengths)
    img, ev = packed(lengths)
    model = model_for(K)
    if opt.kernel_only:
        for _ in range(KERNEL_ONLY_CALLS):
            one_call(model, img, ev, lengths, VARIANTS[0][1])
        continue
    times, last = {tag: [] for tag, _ in VARIANTS}, {}
    for tag, kw in VARIANTS:
        one_call(model, img, ev, lengths, kw)                    # warm-up: handle, workspace, every shape once
    for _ in range(opt.runs):
        for tag, kw in VARIANTS:                                 # the variants alternate
            dt, last[tag] = one_call(model, img, ev, lengths, kw)
            times[tag].append(dt)
    say(f"{name} list: {len(lengths)} videos, {total} snippets, K = {K}, L = {L_}; a map is [{total}, {T}] fp32 = {total * T * 4 / 1e6:.1f} MB")
    for tag, _ in VARIANTS:
        t = [x * 1e3 for x in times[tag]]
        say(f"  {tag:10s}: median {statistics.median(t):8.2f} ms per call (min {min(t):.2f}, max {max(t):.2f}, {len(t)} calls)")
    if not opt.plain_only:
        base = statistics.median(times["no maps"])
        for tag in ("last layer", "all layers"):
            extra = statistics.median(times[tag]) - base
            say(f"  {tag} - no maps = {extra * 1e3:.2f} ms ({100 * extra / base:.0f} % of the plain call)")
            assert torch.equal(last[tag]["logits"], last["no maps"]["logits"])
        assert torch.equal(last["all layers"]["image_attn"][L_ - 1], last["last layer"]["image_attn"][0])
    del img, ev, model, last

if not (opt.kernel_only or opt.plain_only):
    os.makedirs(os.path.dirname(os.path.abspath(opt.log)), exist_ok=True)
    with open(opt.log, "w") as f:
        f.write("\n".join(lines) + "\n")
