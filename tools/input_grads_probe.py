"""What the gradients of the input features cost (`MMFMIL` with `requires_grad` features, `iefvad_train_backward_inputs`,
csrc/train.h): whole training steps at the benched training batch -- 128 chunks of [256, 768], K = 10, L = 2, StudentT nu = 8, attention
dropout 0.1 -- in compute="bf16x6" and "f32", three variants:

  * plain    forward, the trainers' loss, backward, AdamW: no input gradient asked for (`iefvad_train_backward`)
  * inputs   the same step with `requires_grad` on both feature tensors: two more 32,768 x 768 x 2304 products in the backward
  * frozen   every parameter frozen, features requiring grad: forward, loss, backward (the input gradients alone; no optimiser)

One process per run; one warm-up step of each variant, then `--runs` steps of each, ALTERNATING; medians with min - max of the device
time of whole steps (torch.cuda events on the current stream, which every launch goes to).  Profiler off.  The log goes to
profiles/input_grads_probe.log (or --log PATH) and to stdout.

  --plain-only             the "plain" variant alone (it uses nothing this feature added, so the same file times a checkout of the
                           parent commit on the same box; run the two checkouts in turn); prints, writes no log
  --kernel-only            1 + 3 plain steps per arithmetic and nothing else: run THIS under
                           `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/input_grads_probe.py --kernel-only`
                           in each checkout
  --compare-stats A B      the kernel names and launch counts of two such runs' kernel_stats.csv (A: parent, B: this tree), appended to
                           the log: the condition is that they are the same
  --append TEXTFILE        append a file of `--plain-only` output lines (the parent's and this tree's, in turn) to the log"""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "input_grads_probe.log"))
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--chunks", type=int, default=128)
ap.add_argument("--label", default="")
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--compare-stats", nargs=2, default=None)
ap.add_argument("--append", default=None)
opt = ap.parse_args()
KERNEL_ONLY_STEPS = 3

if opt.append:
    with open(opt.append) as f, open(opt.log, "a") as g:
        g.write(f.read())
    sys.exit(0)

if opt.compare_stats:
    def counts(path):
        with open(path) as f:
            return {r["Name"]: int(r["Calls"]) for r in csv.DictReader(f)}
    a, b = (counts(p) for p in opt.compare_stats)
    out = [f"kernel names and launch counts of `--kernel-only` (1 + {KERNEL_ONLY_STEPS} plain steps per arithmetic) under rocprofv3 --kernel-trace "
           "--stats, parent commit vs this tree:",
           f"  parent: {len(a)} kernel names, {sum(a.values())} launches; this tree: {len(b)} kernel names, {sum(b.values())} launches"]
    diff = sorted(n for n in set(a) | set(b) if a.get(n) != b.get(n))
    for n in diff:
        out.append(f"  DIFFERS {n}: parent {a.get(n)}, this tree {b.get(n)}")
    out.append("  same kernel names and launch counts: " + ("yes" if not diff else "NO"))
    with open(opt.log, "a") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))
    sys.exit(1 if diff else 0)

import torch  # noqa: E402

import iefvad_amd  # noqa: E402
from iefvad_amd import losses, synth  # noqa: E402

K, B = 10, opt.chunks
dev = torch.device("cuda", 0)
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def run(compute):
    args = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    model = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, "cuda", args, compute=compute)
    model.load_state_dict(synth.make_state_dict(0, 768, 2, K))
    model = model.to(dev).train()
    for m in list(model.temporal.image_attn_layers) + list(model.temporal.event_attn_layers):
        m.dropout = 0.1
    optim = losses.AdamW(model.parameters(), lr=2e-5)
    gen = torch.Generator(device=dev).manual_seed(1)
    img = torch.randn(B, 256, 768, device=dev, generator=gen) * 0.45
    ev = torch.randn(B, 256, 768, device=dev, generator=gen) * 0.45
    labels = torch.zeros(B, 14, device=dev)
    labels[: B // 2, 0] = 1
    labels[B // 2:, 3] = 1
    lengths = torch.full((B,), 256, dtype=torch.int64, device=dev)

    def step(variant):
        want = variant != "plain"
        for q in model.parameters():
            q.requires_grad_(variant != "frozen")
        x = [t.detach().requires_grad_(want) for t in (img, ev)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = model(x[0], x[1], None, None, lengths)
        total = losses.training_loss(out, labels, lengths, "StudentT", 8, 1.0, 1.0)
        if variant != "frozen":
            optim.zero_grad()
        total.backward()
        if variant != "frozen":
            optim.step()
        e1.record()
        torch.cuda.synchronize()
        assert all((t.grad is not None) == want for t in x)
        return e0.elapsed_time(e1)

    if opt.kernel_only:
        for _ in range(1 + KERNEL_ONLY_STEPS):
            step("plain")
        return
    variants = ("plain",) if opt.plain_only else ("plain", "inputs", "frozen")
    for v in variants:
        step(v)
    ms = {v: [] for v in variants}
    for _ in range(opt.runs):
        for v in variants:
            ms[v].append(step(v))
    for v in variants:
        say(f"  {opt.label}{compute:7s} {v:7s} median {statistics.median(ms[v]):8.3f} ms  (min {min(ms[v]):8.3f} - max {max(ms[v]):8.3f}, {opt.runs} steps)")
    if not opt.plain_only:
        md = {v: statistics.median(ms[v]) for v in variants}
        say(f"  {compute:7s} inputs - plain = {md['inputs'] - md['plain']:+.3f} ms ({100 * (md['inputs'] / md['plain'] - 1):+.2f} %); "
            f"frozen / plain = {md['frozen'] / md['plain']:.3f}")


if not opt.plain_only and not opt.kernel_only:
    say(f"input-gradient probe: whole training steps, {B} chunks x 256 x 768, K = {K}, L = 2, StudentT nu = 8, attention dropout 0.1, "
        f"{torch.cuda.get_device_name(0)}; device time per step, variants alternating in one process after a warm-up step of each")
for compute in ("bf16x6", "f32"):
    run(compute)
    torch.cuda.empty_cache()
if lines and not opt.plain_only:
    with open(opt.log, "w") as f:
        f.write("\n".join(lines) + "\n")
