"""What the batch-invariant mode of compute="bf16x6" costs and buys (MMFMIL(..., batch_invariant=True), csrc/gemm_split_small.h):

  1. gemm      the small tiling (iefvad_gemm_split_small_unit) against the forced 128 x 128 tiling (iefvad_gemm_split_unit, tile_n = 128)
               at M = 256 B, B = 1 .. 8, N in {768, 1536, 2304}, K = 768, bias epilogue, one problem: the crossover between the two
               (kSplitMinWgs in csrc/launch_rules.h)
  2. forward   a B = 1 and a B = 3 forward (outputs="scores", hipGraph replay as users get it) in f32, default bf16x6 and invariant
               bf16x6: what invariance costs per small call
  3. eval      harness.test on the UCF-Crime-sized list (290 videos, ~69.5 k snippets, K = 10) and on the ShanghaiTech + MSAD-sized list
               (438 videos, 17,732 snippets, K = 5): the default bf16x6 model (one forward per video, the route harness.test picks for
               it) against the invariant model (the packed route it picks for that one); class lists and scores are compared

One process; every variant is warmed up once, then the variants ALTERNATE; medians of `--runs` with min - max.  Device times of 1 and 2
are hip events around `--reps` back-to-back calls, 3 is the wall clock of whole calls.  Profiler off.  The log goes to
profiles/batch_invariant_probe.log (or --log PATH) and to stdout.

  --sections gemm,forward,eval   which of the three to run
  --kernel-only                  one warmed-up pass over section 1's launches and nothing else: run THIS under
                                 `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/batch_invariant_probe.py --kernel-only`
                                 (no counters in that run)
  --append-stats CSV             append the two tilings' lines of that run's kernel_stats.csv to the log"""
import argparse
import csv
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "batch_invariant_probe.log"))
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--sections", default="gemm,forward,eval")
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--append-stats", default=None)
opt = ap.parse_args()

if opt.append_stats:
    out = ["kernel stats of one `--kernel-only` run under rocprofv3 --kernel-trace --stats (section 1's launches, every shape once per tiling "
           "after a warm-up of each):"]
    with open(opt.append_stats) as f:
        for r in csv.DictReader(f):
            if "gemm_split_small" in r["Name"] or "gemm_split_n128_kernel" in r["Name"]:
                out.append(f"  {r['Name']}: {r['Calls']} launches, total {int(r['TotalDurationNs']) / 1e3:.1f} us, average "
                           f"{float(r['AverageNs']) / 1e3:.2f} us, min {int(r['MinNs']) / 1e3:.2f} us, max {int(r['MaxNs']) / 1e3:.2f} us")
    with open(opt.log, "a") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import iefvad_amd  # noqa: E402
from iefvad_amd import harness, synth  # noqa: E402
from iefvad_amd import lib as L  # noqa: E402

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def med(ts, unit=1e3):
    t = [x * unit for x in ts]
    return f"median {statistics.median(t):9.2f} (min {min(t):.2f}, max {max(t):.2f})"


def device_time(fn, reps):
    """seconds per call: hip events around `reps` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


# ------------------------------------------------------------------ 1. the two tilings
def gemm_cases():
    lib = L.load_library()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    K = 768
    for N in (768, 1536, 2304):
        W = torch.randn(N, K, device="cuda") / K ** 0.5
        planes = torch.empty(3, N, K, dtype=torch.bfloat16, device="cuda")
        assert lib.iefvad_split_bf16x3(W.data_ptr(), planes.data_ptr(), N * K, st) == 0, L.last_error()
        bias = torch.randn(N, device="cuda")
        for B in range(1, 9):
            M = 256 * B
            A, Cm = torch.randn(M, K, device="cuda"), torch.empty(M, N, device="cuda")
            io = L.GemmSplitIO()
            io.A[0], io.W[0], io.bias[0], io.C[0] = A.data_ptr(), planes.data_ptr(), bias.data_ptr(), Cm.data_ptr()

            def small(io=io, M=M, N=N):
                assert lib.iefvad_gemm_split_small_unit(C.byref(io), M, N, K, N, L.SPLIT_EPI_BIAS, 0, 0.0, 1, st) == 0, L.last_error()

            def n128(io=io, M=M, N=N):
                assert lib.iefvad_gemm_split_unit(C.byref(io), M, N, K, N, L.SPLIT_EPI_BIAS, 0, 0.0, 1, 128, st) == 0, L.last_error()
            yield N, B, small, n128, (A, Cm, W, planes, bias)


def section_gemm():
    say("1. small tiling (32 x 128 workgroups) against the forced 128 x 128 tiling: M = 256 B, K = 768, bias epilogue, one problem; us per "
        f"launch, hip events around {opt.reps} back-to-back launches")
    for N, B, small, n128, _keep in gemm_cases():
        if opt.kernel_only:
            for fn in (small, n128, small, n128):
                fn()
            torch.cuda.synchronize()
            continue
        device_time(small, 5), device_time(n128, 5)
        ts, tn = [], []
        for _ in range(opt.runs):
            ts.append(device_time(small, opt.reps))
            tn.append(device_time(n128, opt.reps))
        wg128 = (256 * B // 128) * (N // 128)
        clear = "small wins" if max(ts) < min(tn) else "n128 wins" if max(tn) < min(ts) else "overlap"
        say(f"  N = {N:4d} B = {B} ({wg128:3d} workgroups of 128 x 128, {4 * wg128:4d} of 32 x 128): small {med(ts, 1e6)} us | n128 {med(tn, 1e6)} us | "
            f"small / n128 = {statistics.median(ts) / statistics.median(tn):.2f} ({clear})")


# ------------------------------------------------------------------ 2. small forwards
def model_for(K, compute, **kw):
    a = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, "cuda", a, outputs="scores", compute=compute, **kw)
    m.load_state_dict(synth.make_state_dict(7, 768, 2, K))
    return m.to("cuda:0").eval()


def section_forward():
    say(f"2. one forward, outputs=\"scores\", K = 10, hipGraph replay; ms per call, hip events around {opt.reps} back-to-back calls")
    variants = {"f32": model_for(10, "f32"), "bf16x6 default": model_for(10, "bf16x6"),
                "bf16x6 invariant": model_for(10, "bf16x6", batch_invariant=True)}
    for B in (1, 3):
        img, ev = (torch.from_numpy(x).cuda() for x in synth.make_inputs(5, B))
        calls = {}
        for tag, m in variants.items():
            def call(m=m):
                with torch.no_grad():
                    m(img, ev, None, None, None)
            calls[tag] = call
            device_time(call, 5)
        times = {tag: [] for tag in calls}
        for _ in range(opt.runs):
            for tag, call in calls.items():
                times[tag].append(device_time(call, opt.reps))
        for tag in calls:
            say(f"  B = {B} {tag:17s}: {med(times[tag])} ms")
        say(f"  B = {B} invariant / default = {statistics.median(times['bf16x6 invariant']) / statistics.median(times['bf16x6 default']):.2f} x")


# ------------------------------------------------------------------ 3. whole evaluations
def lists():
    c5 = synth.config5_lists(os.path.join(ROOT, "tests", "golden"))
    shang_msad = [int(n) for d in ("shang", "msad") for n in c5[d][0]]
    ucf = [int(n) for n in synth.lognormal_lengths(1, 290, 69500)]
    assert len(shang_msad) == 438 and sum(shang_msad) == 17732 and len(ucf) == 290
    return (("UCF-sized", ucf, 10), ("Shang + MSAD-sized", shang_msad, 5))


def items(lengths, classes, seed=3):
    for i, (n, c) in enumerate(zip(lengths, classes)):
        img, ev = synth.make_video(seed, i, n)
        ci, _ = harness.process_split(img, 256)
        ce, _ = harness.process_split(ev, 256)
        yield torch.tensor(ci).unsqueeze(0), torch.tensor(ce).unsqueeze(0), (c,), torch.tensor([n])


def section_eval():
    import contextlib
    import io
    say("3. harness.test(args, model, loader, ...) with batch_chunks unset: the default bf16x6 model takes one forward per video, the "
        "invariant model the packed route (the list walked inside the library); wall clock of whole calls, metric tail included")
    args = argparse.Namespace(dataset="ucfcrime")
    picked = []
    real = harness.score_loader

    def spy(model, loader, maxlen, device, dataset, label_map, batch_chunks, *a, **kw):
        picked.append(batch_chunks)
        return real(model, loader, maxlen, device, dataset, label_map, batch_chunks, *a, **kw)
    harness.score_loader = spy
    for name, lengths, K in lists():
        classes = ["Normal" if i % 2 == 0 else synth.UCF_CLASSES[(i // 2) % 13] for i in range(len(lengths))]
        data = list(items(lengths, classes))
        gt = synth.make_gt(1, sum(lengths))
        models = {"default, per video": model_for(K, "bf16x6"), "invariant, packed": model_for(K, "bf16x6", batch_invariant=True)}

        def one(tag):
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                harness.test(args, models[tag], data, 256, None, gt, "cuda:0")
            torch.cuda.synchronize()
            return time.perf_counter() - t0, harness.test.last_result
        times, last = {tag: [] for tag in models}, {}
        for tag in models:
            one(tag)
        for _ in range(opt.runs):
            for tag in models:
                dt, last[tag] = one(tag)
                times[tag].append(dt)
        a, b = last["default, per video"], last["invariant, packed"]
        worst = float(np.abs(np.concatenate(a["scores"]) - np.concatenate(b["scores"])).max())
        say(f"  {name} list: {len(lengths)} videos, {sum(lengths)} snippets, K = {K}; batch_chunks picked: {sorted(set(picked))}")
        for tag in models:
            say(f"    {tag:19s}: {med(times[tag])} ms per evaluation, {sum(lengths) / statistics.median(times[tag]):10.0f} snippets / s")
        say(f"    per video / packed = {statistics.median(times['default, per video']) / statistics.median(times['invariant, packed']):.2f} x; "
            f"class lists identical: {a['classes'] == b['classes']}; largest |score difference| {worst:.2e} (TOL_SIGMOID 2e-6); "
            f"AUC {a['roc']:.6f} / {b['roc']:.6f}")
        picked.clear()
        del data, models
    harness.score_loader = real


sections = ["gemm"] if opt.kernel_only else opt.sections.split(",")
say(f"batch-invariant bf16x6 probe on {torch.cuda.get_device_name(0)}; runs = {opt.runs}; medians with min - max; variants alternate after a warm-up of each")
if "gemm" in sections:
    section_gemm()
if "forward" in sections:
    section_forward()
if "eval" in sections:
    section_eval()
if not opt.kernel_only:
    os.makedirs(os.path.dirname(os.path.abspath(opt.log)), exist_ok=True)
    with open(opt.log, "w") as f:
        f.write("\n".join(lines) + "\n")
