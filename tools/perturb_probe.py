"""One level of the noise study (harness.PerturbationSweep.level, valid-row route, compute f32) three ways, on the lists of
tools/sweep_rows_probe.py (Shang + MSAD-sized: 438 videos, 17,732 snippets, K = 5; UCF-sized: 290 videos, ~69.5 k snippets, K = 10):

  attenuation        level(0.2, 0.2): the reference's perturbation, two packed scale vectors (`iefvad_forward_videos_scaled`)
  gaussian, device   level(noise_sigma_img=0.2, noise_sigma_ev=0.2): two packed amplitude vectors, the noise drawn by the chunker
                     (`iefvad_forward_videos_perturbed`); the clean rows stay resident
  gaussian, host     the same level the only way possible without that entry: `torch.randn` of [N, 768] per modality on the host, the
                     perturbed copy uploaded, the plain `forward_videos` call, the same statistics

Whole level() calls, results read back as run_test returns them.  After one warm-up of each variant: `--repeats` rounds, the variants
ALTERNATING; medians with min - max.  Profiler off.  The log goes to profiles/perturb_probe.log (or --log PATH) and to stdout.

  --kernel-only            per list two attenuation levels and two device Gaussian levels and nothing else: run THIS under
                           `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/perturb_probe.py --kernel-only`
  --append-stats CSV       append the chunker kernels' lines of that run's kernel_stats.csv to the log, with the bytes they move over
                           their time: the noise instantiation beside the scaled one in the same trace, and the kernel names of the
                           attenuation-only levels."""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "perturb_probe.log"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--sigma", type=float, default=0.2)
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--append-stats", default=None)
opt = ap.parse_args()


def lists():
    """(name, lengths, K): the lists of tools/sweep_rows_probe.py."""
    from iefvad_amd import synth
    c5 = synth.config5_lists(os.path.join(ROOT, "tests", "golden"))
    shang_msad = [int(n) for d in ("shang", "msad") for n in c5[d][0]]
    ucf = [int(n) for n in synth.lognormal_lengths(1, 290, 69500)]
    return (("Shang + MSAD-sized", shang_msad, 5), ("UCF-sized", ucf, 10))


if opt.append_stats:
    cases = lists()
    per_call = sum(2 * 2 * sum(lengths) * 768 * 4 for _, lengths, _ in cases)      # one level on both lists: 2 modalities x (read + write) x [rows, 768] floats
    out = ["kernel stats of one `--kernel-only` run under rocprofv3 --kernel-trace --stats (per list: the clean pass, two attenuation levels, two "
           "device Gaussian levels):"]
    with open(opt.append_stats) as f:
        for r in csv.DictReader(f):
            if "scatter_rows" not in r["Name"]:
                continue
            levels = 2 if "RowNoise" in r["Name"] else 3        # the noise instantiation: the Gaussian levels; the scaled one: clean + attenuation
            t = int(r["TotalDurationNs"])
            out.append(f"  {r['Name']}: {r['Calls']} launches, total {t / 1e3:.1f} us, average {float(r['AverageNs']) / 1e3:.2f} us, "
                       f"min {int(r['MinNs']) / 1e3:.2f} us, max {int(r['MaxNs']) / 1e3:.2f} us; {levels * per_call / 1e9:.3f} GB read + written = "
                       f"{levels * per_call / t / 1e3:.2f} TB/s")
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


def model_for(K):
    a = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, "cuda", a, outputs="scores", compute="f32")
    m.load_state_dict(synth.make_state_dict(7, 768, 2, K))
    return m.to("cuda:0").eval()


def items(lengths, seed=3):
    for i, n in enumerate(lengths):
        img, ev = synth.make_video(seed, i, n)
        ci, _ = harness.process_split(img, 256)
        ce, _ = harness.process_split(ev, 256)
        yield torch.tensor(ci).unsqueeze(0), torch.tensor(ce).unsqueeze(0), ("Normal",), torch.tensor([n])


def attenuation(sweep, host_rows):
    return sweep.level(opt.sigma, opt.sigma)


def gaussian_device(sweep, host_rows):
    return sweep.level(noise_sigma_img=opt.sigma, noise_sigma_ev=opt.sigma)


def gaussian_host(sweep, host_rows):
    """What a caller had to do before: draw on the host, upload a perturbed copy of the list, call the plain forward"""
    c = sweep.clean()
    rows = tuple((x + opt.sigma * torch.randn(x.shape)).to(sweep.device) for x in host_rows)
    return sweep._result(c, sweep._pass_rows(rows=rows))


VARIANTS = (("attenuation", attenuation), ("gaussian, device", gaussian_device), ("gaussian, host", gaussian_host))

say(f"one level of the noise study on the valid-row route, compute = f32, sigma = {opt.sigma}; wall clock of whole level() calls, profiler off")
for name, lengths, K in lists():
    total = sum(lengths)
    sweep = harness.PerturbationSweep(argparse.Namespace(visual_length=256), model_for(K), items(lengths), synth.make_gt(3, total), "cuda:0",
                                      ragged=True)
    torch.manual_seed(0)
    sweep.clean()
    if opt.kernel_only:
        for _ in range(2):
            attenuation(sweep, None)
            gaussian_device(sweep, None)
        torch.cuda.synchronize()
        continue
    host_rows = tuple(r.cpu() for r in sweep.rows)
    times = {tag: [] for tag, _ in VARIANTS}
    for tag, f in VARIANTS:                                   # warm-up: workspaces, every shape once
        f(sweep, host_rows)
    for _ in range(opt.repeats):
        for tag, f in VARIANTS:                               # the variants alternate
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f(sweep, host_rows)
            torch.cuda.synchronize()
            times[tag].append(time.perf_counter() - t0)
    say(f"{name} list: {len(lengths)} videos, {total} snippets, K = {K}; {2 * total * 768 / 1e6:.0f} M normals per Gaussian level")
    for tag, _ in VARIANTS:
        t = [x * 1e3 for x in times[tag]]
        say(f"  {tag:17s}: median {statistics.median(t):8.1f} ms per level (min {min(t):.1f}, max {max(t):.1f}, {len(t)} levels)")
    say(f"  gaussian host / device = {statistics.median(times['gaussian, host']) / statistics.median(times['gaussian, device']):.1f} x")

if not opt.kernel_only:
    os.makedirs(os.path.dirname(os.path.abspath(opt.log)), exist_ok=True)
    with open(opt.log, "w") as f:
        f.write("\n".join(lines) + "\n")
