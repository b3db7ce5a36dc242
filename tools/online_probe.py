"""What the online scores cost: whole `MMFMIL.forward_videos_online` calls (`iefvad_forward_videos_online`; csrc/online.h) at strides
256, 64 and 16 (history 256) against the plain `MMFMIL.forward_videos` call on DEVICE-resident packed rows of

  * the UCF-Crime-sized list of config 2 (290 videos, ~69.5 k snippets, K = 10)
  * the ShanghaiTech + MSAD-sized list of BASELINE config 5 (438 videos, 17,732 snippets, K = 5)

-- the lists of tools/samples_probe.py.  One process; per list and arithmetic (--computes, default f32, bf16x6 and bf16) one warm-up
call of each form, then `--runs` calls of each, ALTERNATING; medians with min - max of the wall clock of whole calls, each ended by a
device synchronise.  Profiler off.  Each cost is given as a multiple of the plain call, beside the estimate from the FLOP shares alone:
(windows / chunks of the plain call) x the encoder's share + one tail (tail = 46.9 % of a K = 10 forward, 30.6 % of a K = 5 one).  Once
per list, in f32 at stride 64: the alternative the entry replaces -- every window built on the host, uploaded, one dense `forward`,
the read-out rows sliced -- timed from host rows to device results.  The log goes to profiles/online_probe.log (or --log PATH) and to
stdout.

  --plain-only             only the plain calls (the one form the parent commit has too): run it in a checkout of the parent and in
                           this tree in turn, and compare against the parent's own spread
  --kernel-only            two stride-16 calls per list in f32 and nothing else: run THIS under
                           `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/online_probe.py --kernel-only`
  --append-stats CSV       append the line of the read-out gather kernel from that run's kernel_stats.csv to the log, with the bytes its
                           launches move over their time (the other row-copy kernels stream at 3.6-5.7 TB/s)."""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "online_probe.log"))
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--computes", default="f32,bf16x6,bf16")
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--append-stats", default=None)
opt = ap.parse_args()
KERNEL_ONLY_CALLS, KERNEL_ONLY_STRIDE = 2, 16
STRIDES = (256, 64, 16)
HOST_STRIDE = 64
D = 768
TAIL_SHARE = {10: 0.469, 5: 0.306}


def lists():
    """(name, lengths, K): the same lists in every mode of this tool."""
    from iefvad_amd import synth
    c5 = synth.config5_lists(os.path.join(ROOT, "tests", "golden"))
    shang_msad = [int(n) for d in ("shang", "msad") for n in c5[d][0]]
    ucf = [int(n) for n in synth.lognormal_lengths(1, 290, 69500)]
    assert len(shang_msad) == 438 and sum(shang_msad) == 17732 and len(ucf) == 290
    return (("UCF-sized", ucf, 10), ("Shang + MSAD-sized", shang_msad, 5))


def windows_of(lengths, stride):
    return sum(-(-n // stride) for n in lengths)


def chunks_of(lengths):
    return sum(max(1, -(-n // 256)) for n in lengths)


if opt.append_stats:
    out = [f"kernel stats of one `--kernel-only` run under rocprofv3 --kernel-trace --stats ({KERNEL_ONLY_CALLS} stride-{KERNEL_ONLY_STRIDE} calls "
           "per list, f32):"]
    with open(opt.append_stats) as f:
        for r in csv.DictReader(f):
            if "iefvad_readout_rows_kernel" in r["Name"]:
                # every snippet's row is read once and written once, per modality, in fp32
                moved = sum(KERNEL_ONLY_CALLS * 2 * 2 * sum(lengths) * D * 4 for _, lengths, K in lists())
                t = int(r["TotalDurationNs"])
                out.append(f"  {r['Name']}: {r['Calls']} launches, total {t / 1e3:.1f} us, average {float(r['AverageNs']) / 1e3:.2f} us, "
                           f"min {int(r['MinNs']) / 1e3:.2f} us, max {int(r['MaxNs']) / 1e3:.2f} us; {moved / 1e9:.4f} GB read + written = "
                           f"{moved / t / 1e3:.3f} TB/s over all its launches")
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


def model_for(K, compute):
    a = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, D, 256, D, 8, 2, 8, 10, 10, "cuda", a, outputs="scores", compute=compute)
    m.load_state_dict(synth.make_state_dict(7, D, 2, K))
    return m.to("cuda:0").eval()


def one_call(model, rows, lengths, stride):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        got = model.forward_videos_online(rows[0], rows[1], lengths, stride) if stride else model.forward_videos(rows[0], rows[1], lengths)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, got


def host_windows_call(model, host_rows, lengths, stride):
    """The alternative: windows built on the host from host rows, uploaded, one dense forward, the read-out rows sliced."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nwin = windows_of(lengths, stride)
    blocks = [np.zeros((nwin, 256, D), np.float32) for _ in range(2)]
    index, w, base = [], 0, 0
    for n in lengths:
        for start, end, read0 in harness.online_windows(n, stride):
            for m in range(2):
                blocks[m][w, :end - start] = host_rows[m][base + start:base + end]
            index.append(np.arange(256 * w + read0 - start, 256 * w + end - start))
            w += 1
        base += n
    t_build = time.perf_counter() - t0
    with torch.no_grad():
        out = model(torch.from_numpy(blocks[0]).cuda(), torch.from_numpy(blocks[1]).cuda(), None, None, None)
        idx = torch.from_numpy(np.concatenate(index)).cuda()
        got = {k: out[k].reshape(-1)[idx] for k in ("logits", "w_i_mean", "w_e_mean")}
    torch.cuda.synchronize()
    return time.perf_counter() - t0, t_build, got, 2 * blocks[0].nbytes


say("online scores: forward_videos(rows, lengths) against forward_videos_online(rows, lengths, stride) on device-resident packed rows; "
    "wall clock of whole calls ended by a synchronise, profiler off" + (" -- plain calls only" if opt.plain_only else ""))
for name, lengths, K in lists():
    total = sum(lengths)
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    rows = tuple(torch.randn(total, D, device="cuda:0", generator=gen) for _ in range(2))
    for compute in (["f32"] if opt.kernel_only else opt.computes.split(",")):
        model = model_for(K, compute)
        if opt.kernel_only:
            for _ in range(KERNEL_ONLY_CALLS):
                one_call(model, rows, lengths, KERNEL_ONLY_STRIDE)
            continue
        forms = {"plain": 0}
        if not opt.plain_only:
            forms.update({f"stride {s}": s for s in STRIDES})
        times, last = {tag: [] for tag in forms}, {}
        for tag, stride in forms.items():
            one_call(model, rows, lengths, stride)                         # warm-up: handle, workspace, every shape once
        for _ in range(opt.runs):
            for tag, stride in forms.items():                              # the forms alternate
                dt, last[tag] = one_call(model, rows, lengths, stride)
                times[tag].append(dt)
        say(f"{name} list, compute = {compute}: {len(lengths)} videos, {total} snippets, {chunks_of(lengths)} chunks, K = {K}")
        for tag in forms:
            t = [x * 1e3 for x in times[tag]]
            say(f"  {tag:11s}: median {statistics.median(t):8.2f} ms (min {min(t):.2f}, max {max(t):.2f}, {len(t)} runs)")
        if not opt.plain_only:
            mp = statistics.median(times["plain"])
            for s in STRIDES:
                nw = windows_of(lengths, s)
                est = nw / chunks_of(lengths) * (1 - TAIL_SHARE[K]) + TAIL_SHARE[K]
                say(f"  stride {s}: {nw} windows, costs {statistics.median(times[f'stride {s}']) / mp:.2f} plain calls "
                    f"(FLOP estimate: {nw / chunks_of(lengths):.2f} x the encoder's {1 - TAIL_SHARE[K]:.3f} + one tail = {est:.2f})")
            if compute == "f32":
                host_rows = tuple(r.cpu().numpy() for r in rows)
                dt, t_build, got, nbytes = host_windows_call(model, host_rows, lengths, HOST_STRIDE)
                same = all(torch.equal(got[k], last[f"stride {HOST_STRIDE}"][k]) for k in got)
                say(f"  stride {HOST_STRIDE} from host-built windows (one run: build {t_build * 1e3:.0f} ms, upload of {nbytes / 1e9:.2f} GB against "
                    f"{2 * total * D * 4 / 1e9:.2f} GB of rows, dense forward, slice): {dt * 1e3:.0f} ms = "
                    f"{dt / statistics.median(times[f'stride {HOST_STRIDE}']):.1f} x the online call on device-resident rows; same bits: {same}")
                del host_rows
        del model
    del rows

if not opt.kernel_only:
    os.makedirs(os.path.dirname(os.path.abspath(opt.log)), exist_ok=True)
    with open(opt.log, "w") as f:
        f.write("\n".join(lines) + "\n")
