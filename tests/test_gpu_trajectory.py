"""The call-time step count (`MMFMIL.set_steps`, `iefvad_set_steps`) and the refinement trajectory (`forward(..., trajectory=True)`,
`forward_videos(..., trajectory=True)`; `iefvad_forward_trajectory`, `iefvad_forward_videos_trajectory`, `iefvad_step_probe_kernel` in
csrc/trajectory.h) with the harness on top (`score_loader` / `test(..., steps=, trajectory=)`).  `-m gpu`.

The reference fixes K at construction; its definition of "k of K steps" is the model built with K = k on the first k blocks
(tests/golden/make_golden_trajectory.py).  So: `set_steps(k)` against such a truncated model of this package, bit for bit (both launch
the same kernels on the same data); the trajectory against `set_steps(k)` calls of the same model; and both against the reference's
capture."""
import argparse
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth
from iefvad_amd import lib as L
from tests import helpers as H
from tests import test_gpu_bf16 as TB
from tests import test_gpu_videos_full as VF
from tests.test_trajectory_cpu import TOL_DELTA, load_trajectory_case, truncated

pytestmark = pytest.mark.gpu

LENGTHS = [37, 256, 257, 1]      # a short video, a len % 256 == 0 one, one row past the chunk edge, a one-row video: 5 chunks, 551 rows
SCORE_KEYS = ("logits", "w_i_mean", "w_e_mean")
# delta_norm against the fp64 norm of the difference of two returned states: an fp32 sum of D squared fp32 differences has a
# relative error of at most (D + 2) 2^-24 = 4.6e-5 at D = 768 (each difference and each square rounds once, the D - 1 additions
# once each), halved by the root, plus one rounding of the root: below 5e-5
REL_DELTA = 5e-5


def make_model(sd, compute="f32", D=768, L_=2, K=5, **kw):
    args = argparse.Namespace(visual_layers=L_, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, D, 256, D, 8, L_, 8, 10, 10, "cuda", args, compute=compute, **kw)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


def run(model, img, ev, **kw):
    """The model's dict (clones: a replayed hipGraph writes where the last call wrote)."""
    with torch.no_grad():
        out = model(img, ev, None, None, None, **kw)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def state(D, K):
    return synth.make_state_dict(43, D, 2, K)


@functools.lru_cache(maxsize=None)
def inputs(B, D=768):
    img, ev = synth.make_inputs(9, B, D=D)
    img[B - 1, 100:] = 0      # a padded tail in the last chunk
    ev[B - 1, 100:] = 0
    return torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()


@functools.lru_cache(maxsize=None)
def videos(D=768):
    return tuple(synth.make_video(8, i, n, D=D, dtype=np.float32) for i, n in enumerate(LENGTHS))


# ---- 1. set_steps(k) is the truncated model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute,B,D,kw", [
    ("f32", 1, 768, {}),
    ("bf16", 1, 768, {}),                                   # 4 row blocks: the chain kernel reads a prefix of its stream; k = 0 skips it
    ("bf16x6", 6, 768, {}),                                 # 72 workgroups: the smallest batch of the split kernels and the folded scorer
    ("bf16x6", 6, 768, dict(outputs="scores")),             # ... where the fold drops the last W2 launch
    ("bf16x6", 1, 768, {}),                                 # on the fp32 kernels
    ("fp16x3", 6, 768, {}),
    ("bf16x6", 1, 768, dict(batch_invariant=True)),         # the small tiling, folded at every size
    ("f32", 1, 512, {}),
], ids=lambda v: str(v).replace(" ", ""))
def test_set_steps_equals_the_truncated_model(compute, B, D, kw):
    K = 5
    sd = state(D, K)
    img, ev = inputs(B, D)
    model = make_model(sd, compute, D, K=K, **kw)
    untouched = run(model, img, ev)
    keys = iefvad_amd.OUTPUT_KEYS if kw.get("outputs", "full") == "full" else SCORE_KEYS
    assert set(untouched) == set(keys)
    for k in (0, 1, 4, 5):
        model.set_steps(k)
        assert model.steps == k
        got = run(model, img, ev)
        want = run(make_model(truncated(sd, k), compute, D, K=k, **kw), img, ev)
        for key in keys:
            assert bool(torch.isfinite(got[key]).all()), (k, key)
            assert torch.equal(got[key], want[key]), (compute, B, k, key, float((got[key] - want[key]).abs().max()))
        if k < K:
            assert not torch.equal(got["logits"], untouched["logits"]), k      # the count is really in force
    model.set_steps(None)
    again = run(model, img, ev)
    for key in keys:
        assert torch.equal(again[key], untouched[key]), key


@pytest.mark.parametrize("compute", ["f32", "bf16", "bf16x6"])
def test_set_steps_on_the_valid_row_route(compute):
    K = 5
    sd = state(768, K)
    rows = VF.pack(videos())
    model = make_model(sd, compute, K=K)
    with torch.no_grad():
        untouched = model.forward_videos(rows[0], rows[1], LENGTHS, outputs="full")
        for k in (0, 1, 4, 5):
            model.set_steps(k)
            got = model.forward_videos(rows[0], rows[1], LENGTHS, outputs="full")
            want = make_model(truncated(sd, k), compute, K=k).forward_videos(rows[0], rows[1], LENGTHS, outputs="full")
            for key in want:
                assert torch.equal(got[key], want[key]), (compute, k, key, float((got[key] - want[key]).abs().max()))
        model.set_steps(None)
        again = model.forward_videos(rows[0], rows[1], LENGTHS, outputs="full")
    for key in untouched:
        assert torch.equal(again[key], untouched[key]), key


def test_range_and_training_refusals():
    K = 3
    model = make_model(state(768, K), K=K)
    img, ev = inputs(1)
    run(model, img, ev)                      # the handle exists
    lib = L.load_library()
    for bad in (-1, K + 1):
        assert lib.iefvad_set_steps(model._handle, bad) != 0
        assert L.last_error().startswith("iefvad_set_steps:") and str(bad) in L.last_error()
    o, t = L.Outputs(), L.Trajectory(None, None, 256)
    ws = torch.empty(lib.iefvad_trajectory_workspace_bytes(model._handle, 1), dtype=torch.uint8, device="cuda")
    args = (model._handle, C.c_void_p(img.data_ptr()), C.c_void_p(ev.data_ptr()), L.IN_F32, 1, C.c_void_p(ws.data_ptr()), ws.numel(), C.byref(o))
    assert lib.iefvad_forward_trajectory(*args, C.byref(t), None) != 0
    assert L.last_error().startswith("iefvad_forward_trajectory:") and "both null" in L.last_error()
    buf = torch.empty(K + 1, 256, device="cuda")
    t = L.Trajectory(buf.data_ptr(), None, 255)
    assert lib.iefvad_forward_trajectory(*args, C.byref(t), None) != 0
    assert L.last_error().startswith("iefvad_forward_trajectory:") and "stride" in L.last_error()
    t = L.Trajectory(buf.data_ptr(), None, 256)
    assert lib.iefvad_forward_trajectory(*args[:6], lib.iefvad_workspace_bytes(model._handle, 1), args[7], C.byref(t), None) != 0
    assert L.last_error().startswith("iefvad_forward_trajectory:") and "workspace too small" in L.last_error()
    model.set_steps(2)
    model.train()
    with pytest.raises(RuntimeError, match="iefvad_train_forward.*iefvad_set_steps"):
        model(img, ev, None, None, None)
    model.eval()
    model.set_steps(None)
    model.train()
    out = model(img, ev, None, None, None)      # all K steps: training runs
    assert bool(torch.isfinite(out["logits"]).all())


# ---- 2. graph replay ----------------------------------------------------------------------------------------------------------------
def test_a_graph_captured_at_one_count_never_replays_for_another():
    K = 4
    sd = state(768, K)
    img, ev = inputs(2)
    graphed, direct = make_model(sd, K=K, graph_chunks=8), make_model(sd, K=K, graph_chunks=-1)
    want = {}
    for k in (K, 2):
        direct.set_steps(k)
        want[k] = run(direct, img, ev)
    assert not torch.equal(want[K]["logits"], want[2]["logits"])
    for k in (K, 2, K, 2):
        graphed.set_steps(k)
        got = run(graphed, img, ev)
        for key in iefvad_amd.OUTPUT_KEYS:
            assert torch.equal(got[key], want[k][key]), (k, key)


# ---- 3. the trajectory against the rest of the library -------------------------------------------------------------------------------
@pytest.mark.parametrize("compute,B", [("f32", 1), ("bf16", 1), ("bf16x6", 6), ("fp16x3", 6)])
def test_trajectory_against_set_steps_calls(compute, B):
    K = 3
    model = make_model(state(768, K), compute, K=K)
    img, ev = inputs(B)
    plain = run(model, img, ev)
    got = run(model, img, ev, trajectory=True)
    assert list(got) == list(iefvad_amd.OUTPUT_KEYS) + ["logits_steps", "delta_norm"]
    for key in iefvad_amd.OUTPUT_KEYS:
        assert torch.equal(got[key], plain[key]), (compute, key, float((got[key] - plain[key]).abs().max()))
    ls, dn = got["logits_steps"], got["delta_norm"]
    assert ls.shape == (K + 1, B, 256, 1) and dn.shape == (K, B, 256) and bool(torch.isfinite(ls).all()) and bool(torch.isfinite(dn).all())
    assert torch.equal(ls[K], got["logits"])
    at = {}
    for k in range(K + 1):
        model.set_steps(k)
        at[k] = run(model, img, ev)
    model.set_steps(None)
    for k in range(K + 1):
        d = float((ls[k] - at[k]["logits"]).abs().max())
        print(compute, "logits_steps", k, "max |trajectory - set_steps| =", d)
        if compute == "bf16x6":      # that call takes the folded scorer (another summation order); both are held to the logit gate
            assert d <= H.TOL_LOGIT, (k, d)
        else:
            assert torch.equal(ls[k], at[k]["logits"]), (compute, k, d)
    for k in range(K):
        want = (at[k + 1]["fused"].double() - at[k]["fused"].double()).norm(dim=-1)
        rel = float(((dn[k].double() - want).abs() / want).max())
        print(compute, "delta_norm", k, "max relative error =", rel, "range", float(want.min()), float(want.max()))
        assert float(want.min()) > 0.1
        assert rel <= REL_DELTA, (compute, k, rel)


def test_trajectory_with_a_partial_step_count():
    """set_steps(2) on a K = 3 model: [3, ...] and [2, ...], the rows of the full trajectory (f32: one arithmetic at every size)."""
    K = 3
    model = make_model(state(768, K), K=K)
    img, ev = inputs(1)
    full = run(model, img, ev, trajectory=True)
    model.set_steps(2)
    part = run(model, img, ev, trajectory=True)
    assert part["logits_steps"].shape[0] == 3 and part["delta_norm"].shape[0] == 2
    assert torch.equal(part["logits_steps"], full["logits_steps"][:3]) and torch.equal(part["delta_norm"], full["delta_norm"][:2])
    assert torch.equal(part["logits"], full["logits_steps"][2])
    model.set_steps(0)
    none = run(model, img, ev, trajectory=True)
    assert none["logits_steps"].shape[0] == 1 and none["delta_norm"].shape[0] == 0
    assert torch.equal(none["logits_steps"][0], full["logits_steps"][0]) and torch.equal(none["logits"], full["logits_steps"][0])


def test_trajectory_across_micro_batch_passes():
    """B = 5 on a micro_batch = 2 model: three passes, the last one partial, each writing its columns of the call's series."""
    K = 3
    sd = state(768, K)
    img, ev = inputs(5)
    one = run(make_model(sd, K=K, micro_batch=0), img, ev, trajectory=True)
    three = run(make_model(sd, K=K, micro_batch=2), img, ev, trajectory=True)
    for key in one:
        assert torch.equal(one[key], three[key]), key


# ---- 4. valid rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [768, 512])
def test_forward_videos_trajectory_equals_the_padded_rows(D):
    K = 3
    model = make_model(state(D, K), "f32", D, K=K)
    vids = videos(D)
    img, ev, index = VF.pad(vids)
    dense = run(model, img, ev, trajectory=True)
    rows = VF.pack(vids)
    with torch.no_grad():
        plain = model.forward_videos(rows[0], rows[1], LENGTHS)
        got = model.forward_videos(rows[0], rows[1], LENGTHS, trajectory=True)
    n = sum(LENGTHS)
    assert got["logits_steps"].shape == (K + 1, n) and got["delta_norm"].shape == (K, n)
    for key in SCORE_KEYS:
        assert torch.equal(got[key], plain[key]), key
    assert torch.equal(got["logits_steps"], dense["logits_steps"].reshape(K + 1, -1)[:, index])
    assert torch.equal(got["delta_norm"], dense["delta_norm"].reshape(K, -1)[:, index])
    assert torch.equal(got["logits_steps"][K], got["logits"])


@pytest.mark.parametrize("compute", ["bf16", "bf16x6", "fp16x3"])
def test_forward_videos_trajectory_keeps_the_scores(compute):
    """The other arithmetics on the valid-row route: the three vectors keep their bits, the last row is the call's logits."""
    K = 3
    model = make_model(state(768, K), compute, K=K)
    rows = VF.pack(videos())
    with torch.no_grad():
        plain = model.forward_videos(rows[0], rows[1], LENGTHS)
        got = model.forward_videos(rows[0], rows[1], LENGTHS, trajectory=True)
    for key in SCORE_KEYS:
        assert torch.equal(got[key], plain[key]), (compute, key)
    assert torch.equal(got["logits_steps"][K], got["logits"])
    assert bool(torch.isfinite(got["logits_steps"]).all()) and bool(torch.isfinite(got["delta_norm"]).all()) and float(got["delta_norm"].min()) > 0.1


# ---- 5. the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute,kw,tol_logit,tol_big", [
    ("f32", {}, H.TOL_LOGIT, H.TOL_BIG),
    ("bf16x6", dict(batch_invariant=True), H.TOL_LOGIT, H.TOL_BIG),       # B = 2 in the split arithmetic, not on the fp32 kernels
    ("bf16", {}, TB.TOL_LOGIT_BF16, TB.TOL_BIG_BF16),                     # the bf16 mode's own gates in the same formula
], ids=["f32", "bf16x6", "bf16"])
def test_trajectory_against_the_reference(golden_dir, compute, kw, tol_logit, tol_big):
    """The reference built with K = k on the first k blocks, k = 0 .. 5 (trajectory_k5.npz): logits within the logit gate, update norms
    within 2 x (768-d output gate) x sqrt(768) of the reference's fp64 values."""
    g, cfg, sd, img, ev = load_trajectory_case(golden_dir)
    K = cfg["K"]
    model = make_model(sd, compute, K=K, **kw)
    got = run(model, torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda(), trajectory=True)
    ls = got["logits_steps"].reshape(K + 1, cfg["B"], 256).cpu().numpy()
    dn = got["delta_norm"].cpu().numpy().astype(np.float64)
    e_logit = float(np.abs(ls - g["logits_steps"]).max())
    e_delta = float(np.abs(dn - g["delta_norm"]).max())
    tol_delta = 2 * tol_big * np.sqrt(768.0)
    assert compute != "f32" or tol_delta == TOL_DELTA
    print(f"{compute}: max |logits_steps - reference| = {e_logit:.3e} (reference fp32 floor {float(g['floor_logit']):.1e}, gate {tol_logit:.1e}); "
          f"max |delta_norm - reference fp64| = {e_delta:.3e} (reference fp32 floor {float(g['floor_delta']):.1e}, gate {tol_delta:.2e})")
    assert e_logit <= max(tol_logit, 3.0 * float(g["floor_logit"])), e_logit
    assert e_delta <= tol_delta, e_delta


# ---- 6. the harness -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def config1_k3(tmp_path_factory, golden_dir):
    g, args, gt, _ = H.write_config1_set(tmp_path_factory.mktemp("cfg1traj"), golden_dir)
    return g, args, gt, synth.make_state_dict(int(g["wseed"]), 768, 2, 3)


@pytest.mark.parametrize("batch_chunks", [0, 8])
def test_harness_trajectory(config1_k3, capsys, batch_chunks):
    g, args, gt, sd = config1_k3
    K = 3
    model = make_model(sd, K=K)
    loader = lambda: harness.get_test_loader(args)      # noqa: E731
    capsys.readouterr()
    base = harness.test(args, model, loader(), 256, None, gt, "cuda:0", batch_chunks=batch_chunks)
    printed = capsys.readouterr().out
    ret = harness.test(args, model, loader(), 256, None, gt, "cuda:0", batch_chunks=batch_chunks, trajectory=True)
    assert capsys.readouterr().out == printed
    last = harness.test.last_result
    assert ret == base and model.steps == K
    tr = last["trajectory"]
    n = int(g["lengths"].sum())
    assert tr["scores_steps"].shape == (K + 1, n) and tr["delta_norm"].shape == (K, n) and list(np.diff(tr["row_offsets"])) == list(g["lengths"])
    assert np.array_equal(tr["scores_steps"][K], np.concatenate(last["scores"]))
    assert len(last["auc_steps"]) == K + 1 and len(last["ap_steps"]) == K + 1
    assert (last["auc_steps"][K], last["ap_steps"][K]) == ret
    for k in range(K + 1):
        at = harness.test(args, model, loader(), 256, None, gt, "cuda:0", batch_chunks=batch_chunks, steps=k)
        assert model.steps == K                           # restored behind the walk
        assert np.array_equal(np.concatenate(harness.test.last_result["scores"]), tr["scores_steps"][k]), k
        assert (last["auc_steps"][k], last["ap_steps"][k]) == at, k
    capsys.readouterr()
    dev = harness.test(args, model, loader(), 256, None, gt, "cuda:0", batch_chunks=batch_chunks, trajectory=True, metric_tail="device")
    dl = harness.test.last_result
    assert (dl["auc_steps"][K], dl["ap_steps"][K]) == dev
    for k in range(K + 1):
        assert abs(dl["auc_steps"][k] - last["auc_steps"][k]) <= 1e-12 and abs(dl["ap_steps"][k] - last["ap_steps"][k]) <= 1e-12, k
    with pytest.raises(ValueError, match="host_list"):
        harness.score_loader(model, loader(), 256, "cuda:0", "ucfcrime", batch_chunks=8, host_list=True, trajectory=True)
