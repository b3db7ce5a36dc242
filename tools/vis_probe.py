"""The similarity series of a vis=True evaluation on the device (iefvad_similarity_rows, csrc/similarity.h; harness.similarity_rows)
against the host route they replace, in one process, after a warm-up, every figure the median of 20 timed calls with its min - max:

  1. the similarity launches of ONE evaluation of the UCF-Crime-sized list of bench.py --full's ucf_eval (290 videos, ~69.5 k snippets)
     on the padded route with batch_chunks = 64: per forward one launch over the `[0:len]` slices of its videos, index upload included,
     and the one read-back of the [4, N] result;
  2. the reference's route (test.py:140-151, ucf_test.py:243-247): per video three `.cpu()` copies of the padded [chunks * 256, 768]
     tensors, the `[0:len]` slices, then the four torch CPU calls on the concatenated rows (without the x16 repeat the reference forms
     first -- its cost would only add to this side);
  3. the largest difference between the two results.

The tensors are seeded normals of the evaluation's shapes: the cost depends on the list's shape, not on the model.  `--kernel-only`
runs the launches alone (warm-up + 20 evaluations), for a `rocprofv3 --kernel-trace --stats` run of its own; kernel time comes from
that trace, never from the host clock.  Bytes per launch are counted from the shapes: nout x (3 D x 4 read + 4 index + 16 written).
The log goes to profiles/vis_similarity_probe.log (or the path given with --log) and to stdout."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from iefvad_amd import harness, synth  # noqa: E402

D, T, REPS = 768, 256, 20

p = argparse.ArgumentParser()
p.add_argument("--kernel-only", action="store_true")
p.add_argument("--log", default=os.path.join(ROOT, "profiles", "vis_similarity_probe.log"))
a = p.parse_args()
if not torch.cuda.is_available():
    sys.exit("vis_probe needs a HIP device: nothing here is measured on the CPU")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


# the forwards of one evaluation: videos packed until a batch holds 64 chunks (harness._score_padded), all-zero chunks skipped
lengths = [int(n) for n in synth.lognormal_lengths(1, 290, 69500)]
batches, cur, cur_chunks = [], [], 0
for n in lengths:
    cur.append(n)
    cur_chunks += harness.video_chunks(n, T)
    if cur_chunks >= 64:
        batches.append(cur)
        cur, cur_chunks = [], 0
if cur:
    batches.append(cur)
gen = torch.Generator(device="cuda").manual_seed(1)
forwards = []          # (fused, image_mu, event_mu [chunks, 256, 768] device tensors, index (host int32), per-video (row offset, chunks, length))
for b in batches:
    chunks = [harness.video_chunks(n, T) for n in b]
    f, i, e = (torch.randn(sum(chunks), T, D, device="cuda", generator=gen) for _ in range(3))
    starts = np.concatenate([[0], np.cumsum(chunks)[:-1]]) * T
    index = torch.from_numpy(np.concatenate([np.arange(o, o + n, dtype=np.int32) for o, n in zip(starts, b)]))
    forwards.append((f, i, e, index, list(zip(starts.tolist(), chunks, b))))
total = sum(lengths)
padded = sum(int(fw[0].shape[0]) for fw in forwards) * T
say(f"list: {len(lengths)} videos, {total} snippets in {len(forwards)} forwards of >= 64 chunks ({padded} padded rows, D = {D})")


def device_route():
    parts = [harness.similarity_rows(f, i, e, index) for f, i, e, index, _ in forwards]
    return torch.cat(parts, dim=1).cpu()


def launches_only():
    for f, i, e, index, _ in forwards:
        harness.similarity_rows(f, i, e, index)


def host_route():
    rows = [[], [], []]
    for f, i, e, _, videos in forwards:
        for off, chunks, n in videos:
            for m, t in enumerate((f, i, e)):
                rows[m].append(t.reshape(-1, D)[off:off + chunks * T].cpu()[0:n])
    f, i, e = (torch.cat(r) for r in rows)
    F = torch.nn.functional
    return torch.stack([F.cosine_similarity(f, i, dim=-1), F.cosine_similarity(f, e, dim=-1), torch.norm(f - i, dim=-1), torch.norm(f - e, dim=-1)])


def timed(fn, reps=REPS):
    fn()                                                   # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


if a.kernel_only:
    launches_only()
    torch.cuda.synchronize()
    for _ in range(REPS):
        launches_only()
    torch.cuda.synchronize()
    read = total * 3 * D * 4
    print(f"kernel-only: {REPS + 1} evaluations x {len(forwards)} launches; per evaluation {read / 1e6:.1f} MB of rows read, "
          f"{total * 20 / 1e6:.2f} MB of index and results", flush=True)
    sys.exit(0)

dev = timed(device_route)
lo = timed(launches_only)
host = timed(host_route)
say(f"device route (harness.similarity_rows per forward + one read-back of [4, {total}]): median {dev[0]:.2f} ms (min {dev[1]:.2f}, max {dev[2]:.2f}) of {REPS}")
say(f"  of which the {len(forwards)} launches with their index uploads, synchronised: median {lo[0]:.2f} ms (min {lo[1]:.2f}, max {lo[2]:.2f})")
say(f"host route (3 x .cpu() of the padded tensors per video, [0:len], four torch CPU calls on {total} rows): "
    f"median {host[0]:.1f} ms (min {host[1]:.1f}, max {host[2]:.1f}) of {REPS}")
say(f"  moved to the host: {3 * padded * D * 4 / 1e6:.0f} MB against {16 * total / 1e6:.2f} MB")
diff = (device_route() - host_route()).abs()
say(f"largest |device - host| : cos {float(diff[:2].max()):.3e}, distance {float(diff[2:].max()):.3e}")
say(f"bytes the kernel reads per evaluation (from the shapes): {total * 3 * D * 4 / 1e6:.1f} MB of rows + {total * 4 / 1e6:.2f} MB of index; "
    f"kernel time: see the kernel-trace run (tools/vis_probe.py --kernel-only under rocprofv3 --kernel-trace --stats)")
os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
with open(a.log, "w") as fh:
    fh.write("\n".join(lines) + "\n")
