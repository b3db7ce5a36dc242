"""D = 512 (ViT-B/16 features, head dim 64) against D = 768 on one box, f32 arithmetic: snippets/s of a B = 2048 forward (scores
output, device inputs) and the latency of a B = 1 forward (the graph replay), both from device-synchronised wall clocks, plus the
per-stage times of one timed B = 2048 forward.  Prints one line per width and one JSON line.  Needs a GPU.

    python tools/vitb_probe.py [--chunks 2048] [--reps 5] [--lat-reps 200] [--widths 512,768]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import iefvad_amd  # noqa: E402
from iefvad_amd import synth  # noqa: E402


def measure(D, B, reps, lat_reps):
    args = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=10, lambda_ref=0.5, noise_model="StudentT", nu=8)
    model = iefvad_amd.MMFMIL(14, D, 256, D, 8, 2, 8, 10, 10, "cuda", args, outputs="scores", compute="f32")
    model.load_state_dict(synth.make_state_dict(3, D, 2, 10))
    model = model.to("cuda:0").eval()
    g = torch.Generator(device="cuda:0").manual_seed(1)
    img = torch.randn(B, 256, D, device="cuda:0", generator=g) * 0.45
    ev = torch.randn(B, 256, D, device="cuda:0", generator=g) * 0.45
    res = {}
    with torch.no_grad():
        model(img, ev, None, None, None)                                   # warm-up: handle, weights, workspace
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            model(img, ev, None, None, None)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        res["batch_ms_median"] = 1e3 * statistics.median(times)
        res["snippets_per_s"] = B * 256 / statistics.median(times)
        model(img, ev, None, None, None, timed=True)
        res["stage_ms"] = {k: round(float(v), 3) for k, v in model.last_stage_times.items()} if isinstance(model.last_stage_times, dict) else str(model.last_stage_times)
        x1, y1 = img[:1].contiguous(), ev[:1].contiguous()
        for _ in range(20):
            model(x1, y1, None, None, None)
        torch.cuda.synchronize()
        lat = []
        for _ in range(lat_reps):
            t0 = time.perf_counter()
            model(x1, y1, None, None, None)
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t0)
        res["b1_ms_median"] = 1e3 * statistics.median(lat)
        res["b1_ms_p10"] = 1e3 * sorted(lat)[len(lat) // 10]
    del img, ev, model
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lat-reps", type=int, default=200)
    ap.add_argument("--widths", default="512,768", help="comma-separated embed dims to measure")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "chunks": a.chunks}
    widths = [int(w) for w in a.widths.split(",")]
    for D in widths:
        r = measure(D, a.chunks, a.reps, a.lat_reps)
        out[f"D{D}"] = r
        print(f"D={D}: {r['snippets_per_s'] / 1e6:.3f} M snippets/s at B={a.chunks} ({r['batch_ms_median']:.2f} ms), "
              f"B=1 {r['b1_ms_median']:.3f} ms (p10 {r['b1_ms_p10']:.3f})", flush=True)
    if "D512" in out and "D768" in out:
        out["ratio_512_over_768_rate"] = out["D512"]["snippets_per_s"] / out["D768"]["snippets_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
