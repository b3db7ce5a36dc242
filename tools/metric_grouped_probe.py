"""The per-class / Ano-AUC metric tail on the device (iefvad_auc_ap_grouped, csrc/metrics.h; harness.evaluate_scores_device) against
what it replaces, in one process, after a warm-up, every figure the median of repeated timed calls:

  1. the HOST tail (harness.evaluate_scores: sklearn, 1 global + 1 Ano-AUC + one AUC / AP pair per class on the x16 repeat) on the
     UCF-Crime-sized list of bench.py --full's ucf_eval (290 videos, ~69.5 k snippets) and on the XD-Violence-sized one (753 videos,
     ~145 k snippets) -- the first line: is this tail worth moving at all beside a packed list walk;
  2. harness.evaluate_scores_device on the same lists and scores (scores and gt resident on the device), with the largest difference
     between the two results;
  3. iefvad_auc_ap_grouped with 14 groups against iefvad_auc_ap at the same n (69,500 / 145,000 / 2,097,152), both through the
     harness wrappers, read-back included.

Scores are synthetic (sigmoid of seeded normals): the tail's cost depends on the list's shape, not on the model.  The log goes to
profiles/metric_grouped_probe.log (or the path given as the first argument) and to stdout."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from iefvad_amd import harness, synth  # noqa: E402

log_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "metric_grouped_probe.log")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def median_ms(fn, reps):
    fn()                                                   # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times) * 1e3


def ucf_list():
    lengths = synth.lognormal_lengths(1, 290, 69500)       # bench.py ucf_eval
    abnormal = [c for c in synth.UCF_CLASSES if c != "Normal"]
    classes = ["Normal" if i % 2 == 0 else abnormal[(i // 2) % 13] for i in range(290)]
    return "ucfcrime", lengths, classes, synth.make_gt(1, int(lengths.sum())), ("Normal",)


def xd_list():
    lengths = synth.lognormal_lengths(2, 753, 145000)      # bench.py xd_parts
    keys = harness.CLASS_KEYS["xd"]
    classes = [keys[i % len(keys)] for i in range(753)]
    return "xd", lengths, classes, synth.make_gt(2, int(lengths.sum())), ("normal",)


def worst_difference(a, b):
    d = [abs(a[k] - b[k]) for k in ("roc", "ap", "ano_auc")]
    d += [abs(x - y) for c in a["per_class"] for x, y in zip(a["per_class"][c], b["per_class"][c])]
    return max(d)


cases = []
for dataset, lengths, classes, gt, normal_keys in (ucf_list(), xd_list()):
    rng = np.random.default_rng(len(lengths))
    scores = [(1.0 / (1.0 + np.exp(-2.0 * rng.standard_normal(int(n))))).astype(np.float32) for n in lengths]
    cases.append((dataset, [int(n) for n in lengths], classes, gt, normal_keys, scores))

host_ms = {}
for dataset, lengths, classes, gt, normal_keys, scores in cases:
    host_ms[dataset] = median_ms(lambda: harness.evaluate_scores(scores, classes, gt, dataset, verbose=False, normal_keys=normal_keys), 3)
say("host metric tail (harness.evaluate_scores, sklearn): " + "; ".join(
    f"{d} list of {len(c[1])} videos / {sum(c[1])} snippets {host_ms[d]:.1f} ms" for d, c in zip(host_ms, cases)))

for dataset, lengths, classes, gt, normal_keys, scores in cases:
    flat = torch.from_numpy(np.concatenate(scores)).cuda()
    gt_dev = torch.from_numpy(gt).to(torch.uint8).cuda()
    host = harness.evaluate_scores(scores, classes, gt, dataset, verbose=False, normal_keys=normal_keys)
    dev = harness.evaluate_scores_device((flat, lengths), classes, gt_dev, dataset, verbose=False, normal_keys=normal_keys)
    ms = median_ms(lambda: harness.evaluate_scores_device((flat, lengths), classes, gt_dev, dataset, verbose=False, normal_keys=normal_keys), 20)
    up = median_ms(lambda: harness.evaluate_scores_device(scores, classes, gt, dataset, verbose=False, normal_keys=normal_keys), 10)
    say(f"device metric tail (harness.evaluate_scores_device) on the {dataset} list: {ms:.3f} ms with scores and gt resident on the device, "
        f"{up:.3f} ms from host arrays (float64 gt uploaded); host tail {host_ms[dataset]:.1f} ms = {host_ms[dataset] / ms:.0f} x; "
        f"{len(host['per_class'])} classes, largest |device - host| over all figures {worst_difference(dev, host):.1e}")

for n in (69500, 145000, 2097152):
    gen = torch.Generator(device="cuda").manual_seed(5)
    s = torch.sigmoid(torch.randn(n, device="cuda", generator=gen) * 2)
    gt_dev = torch.from_numpy(synth.make_gt(5, n)).to(torch.uint8).cuda()
    group = torch.randint(0, 14, (n,), device="cuda", generator=gen).to(torch.uint8)
    one = median_ms(lambda: harness.device_auc_ap(s, gt_dev), 20)
    many = median_ms(lambda: harness.device_grouped_auc_ap(s, gt_dev, group, 14), 20)
    say(f"n = {n}: iefvad_auc_ap {one:.3f} ms, iefvad_auc_ap_grouped (14 groups) {many:.3f} ms per call incl. the read-back = {many / one:.2f} x")

os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
with open(log_path, "w") as f:
    f.write("\n".join(lines) + "\n")
