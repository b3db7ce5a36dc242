"""`MMFMIL.forward_videos_online` / `iefvad_forward_videos_online` (include/iefvad.h, csrc/online.h, csrc/window_plan.h): every video
evaluated over trailing windows, so that a snippet's score depends on fewer than `stride` snippets after it.  The reference never does
this; what pins the semantics is the HOST MODEL below: every window of `harness.online_windows` built in numpy as a zero-padded
[256, D] chunk, the existing dense `model(...)` on the stack of windows, and the read-out rows of each window taken from its result."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth
from iefvad_amd import lib as L
from tests import helpers as H

pytestmark = pytest.mark.gpu

LENGTHS = [1, 37, 255, 256, 257, 300, 600]
SHORT = [1, 5, 70, 258]
KEYS = ("logits", "w_i_mean", "w_e_mean")


def make_model(compute="f32", D=768, L_=2, K=3, **kw):
    sd = synth.make_state_dict(41, D, L_, K)
    args = argparse.Namespace(visual_layers=L_, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, D, 256, D, 8, L_, 8, 10, 10, "cuda", args, compute=compute, outputs="scores", **kw)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


def videos(lengths, seed=6, D=768, dtype=np.float32):
    return [synth.make_video(seed, i, int(n), D=D, dtype=dtype) for i, n in enumerate(lengths)]


def host_rule(x):
    """test.py:90-95 on one modality of one WHOLE video, in its own dtype."""
    t = torch.from_numpy(x)
    return torch.nan_to_num(t, nan=0.0).numpy() if bool(torch.isnan(t).any()) else x


def host_model(model, vids, stride, history=256, nan_rule=False):
    """The semantics, spelled out on the host: windows as zero-padded chunks, one dense forward, the read-out rows."""
    D = vids[0][0].shape[1]
    chunks, index = ([], []), []
    for img, ev in vids:
        if nan_rule:
            img, ev = host_rule(img), host_rule(ev)
        for start, end, read0 in harness.online_windows(img.shape[0], stride, history):
            first = 256 * len(chunks[0])
            for m, x in enumerate((img, ev)):
                c = np.zeros((256, D), x.dtype)
                c[:end - start] = x[start:end]
                chunks[m].append(c)
            index.append(np.arange(first + read0 - start, first + end - start))
    with torch.no_grad():
        out = model(torch.from_numpy(np.stack(chunks[0])).cuda(), torch.from_numpy(np.stack(chunks[1])).cuda(), None, None, None)
    idx = torch.from_numpy(np.concatenate(index)).cuda()
    return {k: out[k].reshape(-1)[idx] for k in KEYS}


def rows_of(vids):
    return (torch.from_numpy(np.concatenate([v[0] for v in vids])).cuda(), torch.from_numpy(np.concatenate([v[1] for v in vids])).cuda(),
            [v[0].shape[0] for v in vids])


def online(model, vids, stride, history=256, **kw):
    img, ev, lens = rows_of(vids)
    with torch.no_grad():
        return model.forward_videos_online(img, ev, lens, stride, history=history, **kw)


def assert_same_bits(got, want, n):
    for k in KEYS:
        assert got[k].shape == want[k].shape == (n,), k
        diff = (got[k] - want[k]).abs()
        print(f"{k}: max |online - host model| = {float(torch.nan_to_num(diff, nan=0.0).max()):.3e}")
        nan = torch.isnan(want[k])
        assert torch.equal(torch.isnan(got[k]), nan), k                                  # the same NaN pattern ...
        assert torch.equal(got[k][~nan], want[k][~nan]), k                               # ... and the same bits everywhere else


# ---- 1. f32: the host model, bit for bit ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def f32_model():
    return make_model("f32")


@pytest.mark.parametrize("stride, history", [(16, 256), (100, 256), (256, 256), (100, 150)])
def test_equals_the_host_model_bit_for_bit(f32_model, stride, history):
    vids = videos(LENGTHS)
    assert_same_bits(online(f32_model, vids, stride, history), host_model(f32_model, vids, stride, history), sum(LENGTHS))


def test_stride_one_is_334_windows(f32_model):
    vids = videos(SHORT, seed=7)
    assert sum(len(harness.online_windows(n, 1)) for n in SHORT) == 334
    assert_same_bits(online(f32_model, vids, 1), host_model(f32_model, vids, 1), sum(SHORT))


@pytest.mark.parametrize("stride, history", [(16, 256), (100, 150)])
def test_videos_straddle_passes_with_a_small_micro_batch(stride, history):
    model = make_model("f32", micro_batch=3)
    vids = videos(LENGTHS, seed=8)
    assert_same_bits(online(model, vids, stride, history), host_model(model, vids, stride, history), sum(LENGTHS))


def test_fp16_rows(f32_model):
    vids = videos(LENGTHS, seed=9, dtype=np.float16)
    assert_same_bits(online(f32_model, vids, 16), host_model(f32_model, vids, 16), sum(LENGTHS))


def test_whole_chunk_encoder(f32_model, monkeypatch):
    """IEFVAD_DENSE_ENCODER=1: whole 256-row chunks in the encoder, the read-out gather behind them.  The library reads the switch when
    the handle is created, which is on the model's first call: the variable stays set until that call has been made."""
    vids = videos(LENGTHS, seed=10)
    dense = make_model("f32", micro_batch=5)
    monkeypatch.setenv("IEFVAD_DENSE_ENCODER", "1")
    first = online(dense, vids, 16)
    monkeypatch.delenv("IEFVAD_DENSE_ENCODER")
    assert_same_bits(first, host_model(f32_model, vids, 16), sum(LENGTHS))
    assert_same_bits(online(dense, vids, 100, 150), host_model(f32_model, vids, 100, 150), sum(LENGTHS))


@pytest.mark.parametrize("stride, history", [(16, 256), (100, 150)])
def test_d512(stride, history):
    model = make_model("f32", D=512)
    vids = videos(LENGTHS, seed=11, D=512)
    assert_same_bits(online(model, vids, stride, history), host_model(model, vids, stride, history), sum(LENGTHS))


def test_nan_rule_is_per_whole_video(f32_model):
    """NaN plus +-inf as test_gpu_videos.py places them: video 1 has a NaN and infinities in its image rows -> replaced in all its
    windows, also the ones that end before the NaN (the rule is not causal); video 3 has an inf only -> nothing is replaced and its
    windows' scores go NaN as on every other route; video 4 has a NaN in the event rows of its second chunk."""
    lengths = [100, 300, 50, 80, 600, 256]
    vids = videos(lengths, seed=9)
    vids[1][0][7, 5] = np.nan
    vids[1][0][290, 100] = np.inf
    vids[1][0][3, 9] = -np.inf
    vids[3][0][10, 10] = np.inf
    vids[4][1][400, 767] = np.nan
    got = online(f32_model, vids, 16)
    assert_same_bits(got, host_model(f32_model, vids, 16, nan_rule=True), sum(lengths))
    off = np.concatenate([[0], np.cumsum(lengths)])
    assert bool(torch.isfinite(got["logits"][off[4]:off[5]]).all())          # also in the windows that end before row 400
    assert bool(torch.isnan(got["logits"][off[3]:off[4]]).all())             # row 10 lies in every window of video 3 (80 <= history)
    raw = online(f32_model, vids, 16, nan_to_num=False)
    assert_same_bits(raw, host_model(f32_model, vids, 16, nan_rule=False), sum(lengths))


# ---- 2. bf16 ------------------------------------------------------------------------------------------------------------------------------
def test_bf16_equals_the_host_model_bit_for_bit(monkeypatch):
    """All three results, bit for bit, wherever both sides run the same kernels.  In bf16 the weight means come from one of two kernels,
    picked by the tail's row count (plan_tail, launch_rules.h): the fused heads + fusion kernel from 128 workgroups on (2752 rows), the
    stand-alone fusion kernel below; they sum a row's 768 weights in different orders (tests/test_gpu_videos.py gates that difference
    at 1e-6).  The online tail runs on the 1706 read-out rows, the host model's on 110 x 256 = 28160 rows, so with the default
    micro-batch of 1024 chunks the two sides sit on different sides of that threshold: measured there, logits 0 and w_i_mean 1.2e-7
    (one ulp) apart -- the bit equality of the weight means that the issue asks for is not attainable in that configuration without
    touching the kernels or the launch rule.  It is asserted in the two configurations of the same inputs in which both sides take the
    stand-alone kernel: IEFVAD_ROWBLOCK_OFF=4 (default micro-batch) and micro_batch = 8 (every pass of either
    side has at most 2048 rows).  At the plain default the logits, which do not depend on that choice, are asserted bit for bit and
    the weight means within the project's gate for the two kernels' summation orders, 1e-6: a mean of 768 fp32 weights near 0.5
    has an ulp of 6e-8, and a wrong or stale row would be off by the spread of the means (asserted above 1e-3)."""
    vids = videos(LENGTHS)
    model = make_model("bf16")
    monkeypatch.setenv("IEFVAD_ROWBLOCK_OFF", "4")                    # read when the handle is created: on the model's first call
    first = online(model, vids, 16)
    monkeypatch.delenv("IEFVAD_ROWBLOCK_OFF")
    assert_same_bits(first, host_model(model, vids, 16), sum(LENGTHS))
    del model
    model = make_model("bf16", micro_batch=8)
    assert_same_bits(online(model, vids, 16), host_model(model, vids, 16), sum(LENGTHS))
    del model
    model = make_model("bf16")
    got, want = online(model, vids, 16), host_model(model, vids, 16)
    assert torch.equal(got["logits"], want["logits"])
    assert float(want["w_i_mean"].std()) > 1e-3                      # the gate below is far inside the spread of the means
    for k in ("w_i_mean", "w_e_mean"):
        e = float((got[k] - want[k]).abs().max())
        print(f"default micro-batch, {k}: max |online - host model| = {e:.3e} (gate 1e-6)")
        assert e <= 1e-6, (k, e)


def test_bf16_fused_heads_kernel_on_the_gathered_rows():
    """A list whose read-out rows cross the row-block threshold (3000 >= 2752) in one pass: the online tail takes the fused heads +
    fusion kernel and the refinement chain on the gathered bf16 operand copy, as the host model's 49 x 256 rows do -- the same kernels
    on both sides, so all three results are compared bit for bit."""
    lengths = [600, 900, 700, 800]
    model = make_model("bf16")
    vids = videos(lengths, seed=16)
    assert sum(lengths) >= 2752 and sum(len(harness.online_windows(n, 64)) for n in lengths) == 49
    assert_same_bits(online(model, vids, 64), host_model(model, vids, 64), sum(lengths))


# ---- 3. bf16x6 ----------------------------------------------------------------------------------------------------------------------------
def test_bf16x6_meets_the_host_model_inside_the_fp32_gates():
    model = make_model("bf16x6")
    vids = videos(LENGTHS)
    got, want = online(model, vids, 16), host_model(model, vids, 16)
    e_logit = float((got["logits"] - want["logits"]).abs().max())
    e_w = max(float((got[k] - want[k]).abs().max()) for k in ("w_i_mean", "w_e_mean"))
    print(f"bf16x6: max |logits - host model| = {e_logit:.3e} (gate {H.TOL_LOGIT:.1e}); weight means {e_w:.3e} (gate 2e-6)")
    assert e_logit <= H.TOL_LOGIT and e_w <= 2e-6


def test_bf16x6_batch_invariant_is_bit_identical():
    model = make_model("bf16x6", batch_invariant=True)
    vids = videos(LENGTHS)
    assert_same_bits(online(model, vids, 16), host_model(model, vids, 16), sum(LENGTHS))


# ---- 4. the degenerate case ---------------------------------------------------------------------------------------------------------------
def test_stride_and_history_256_is_forward_videos(f32_model):
    lengths = [37, 256, 512]          # <= 256 or a multiple of 256: the windows are the chunks of the plain call
    vids = videos(lengths, seed=12)
    img, ev, lens = rows_of(vids)
    with torch.no_grad():
        want = f32_model.forward_videos(img, ev, lens)
    assert_same_bits(online(f32_model, vids, 256, 256), want, sum(lengths))


# ---- 5. causality ---------------------------------------------------------------------------------------------------------------------------
def test_the_future_does_not_reach_the_past(f32_model):
    """Every row of video 0 from p = 130 on is replaced: at stride 16 all snippets below 128 -- the last window end <= p -- keep
    their bits, while the offline scores of the same snippets (one 256-row chunk attends over the change) move; video 1 keeps all
    its bits on both routes."""
    lengths, p, stride = [300, 90], 130, 16
    vids = videos(lengths, seed=13)
    other = [(v[0].copy(), v[1].copy()) for v in vids]
    repl = synth.make_video(99, 0, lengths[0])
    other[0][0][p:], other[0][1][p:] = repl[0][p:], repl[1][p:]
    safe = max(e for _, e, _ in harness.online_windows(lengths[0], stride) if e <= p)
    assert safe == 128
    a, b = online(f32_model, vids, stride), online(f32_model, other, stride)
    with torch.no_grad():
        pa, pb = f32_model.forward_videos(*rows_of(vids)), f32_model.forward_videos(*rows_of(other))
    for k in KEYS:
        assert torch.equal(a[k][:safe], b[k][:safe]), k
        assert not torch.equal(a[k][safe:lengths[0]], b[k][safe:lengths[0]]), k
        assert not torch.equal(pa[k][:safe], pb[k][:safe]), k                  # the offline protocol looks ahead
        assert torch.equal(a[k][lengths[0]:], b[k][lengths[0]:]) and torch.equal(pa[k][lengths[0]:], pb[k][lengths[0]:]), k


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(f32_model):
    vids = videos([40, 20], seed=14)
    img, ev, lens = rows_of(vids)
    with pytest.raises(RuntimeError, match="fp16x3"):
        make_model("fp16x3").forward_videos_online(img, ev, lens, 16)
    with pytest.raises(RuntimeError, match="requires grad"):
        f32_model.forward_videos_online(img.clone().requires_grad_(True), ev, lens, 16)
    with pytest.raises(RuntimeError, match="HIP device only"):
        f32_model.forward_videos_online(img.cpu(), ev.cpu(), lens, 16)
    f32_model.train()
    try:
        with pytest.raises(RuntimeError, match=r"model.train\(\)"):
            f32_model.forward_videos_online(img, ev, lens, 16)
    finally:
        f32_model.eval()


def test_c_entry_refuses_before_any_launch(f32_model):
    vids = videos([40, 20], seed=14)
    img, ev, lens = rows_of(vids)
    with torch.no_grad():
        want = f32_model.forward_videos_online(img, ev, lens, 16)         # creates the handle, sets the weights
    lib, h = L.load_library(), f32_model._handle
    larr = (C.c_int32 * 2)(*lens)
    on = L.Online(16, 256)
    need = lib.iefvad_videos_online_workspace_bytes(h, larr, 2, C.byref(on))
    # ceil(40 / 16) + ceil(20 / 16) = 5 windows: the base workspace of a five-chunk pass, nothing behind it, whatever the history
    assert need == lib.iefvad_workspace_bytes(h, 5) and need == lib.iefvad_videos_online_workspace_bytes(h, larr, 2, C.byref(L.Online(16, 16)))
    assert lib.iefvad_videos_online_workspace_bytes(h, larr, 2, C.byref(L.Online(0, 256))) == 0
    assert lib.iefvad_videos_online_workspace_bytes(h, larr, 2, C.byref(L.Online(32, 16))) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = [torch.full((60,), -7.0, device="cuda") for _ in range(3)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(online_struct, nbytes, compute_handle=h):
        return lib.iefvad_forward_videos_online(compute_handle, C.c_void_p(img.data_ptr()), C.c_void_p(ev.data_ptr()), L.IN_F32, larr, 2, 1,
                                                C.byref(online_struct) if online_struct is not None else None, C.c_void_p(ws.data_ptr()), nbytes,
                                                *(C.c_void_p(t.data_ptr()) for t in out), stream)

    assert call(on, need - 1) != 0
    assert L.last_error().startswith("iefvad_forward_videos_online:") and "workspace too small" in L.last_error()
    for bad in (L.Online(0, 256), L.Online(257, 257), L.Online(32, 16), L.Online(1, 257)):
        assert call(bad, need) != 0
        assert "stride" in L.last_error() and "history" in L.last_error()
    assert call(None, need) != 0 and "null" in L.last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in out)                        # nothing was launched
    assert call(on, need) == 0
    torch.cuda.synchronize()
    for t, k in zip(out, KEYS):
        assert torch.equal(t, want[k]), k


# ---- 7. the harness -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def config1_k3(tmp_path_factory, golden_dir):
    g, args, gt, _ = H.write_config1_set(tmp_path_factory.mktemp("cfg1online"), golden_dir)
    return g, args, gt


def test_score_loader_online_equals_the_call_on_the_concatenated_rows(f32_model, config1_k3):
    g, args, gt = config1_k3
    items = list(harness.get_test_loader(args))[:8]                          # eight videos: one NaN element, one fp16 file among them
    lens = [int(it[3]) for it in items]
    got = harness.score_loader(f32_model, items, 256, "cuda:0", "ucfcrime", batch_chunks=3, host_list=False, online_stride=16)
    on = harness.score_loader.last_result["online"]
    assert set(on) == {"scores", "scores_device", "row_offsets", "stride", "history"} and (on["stride"], on["history"]) == (16, 256)
    assert list(np.diff(on["row_offsets"])) == lens and len(got) == 4
    img = torch.cat([it[0].reshape(-1, 768)[:n].float() for it, n in zip(items, lens)]).cuda()
    ev = torch.cat([it[1].reshape(-1, 768)[:n].float() for it, n in zip(items, lens)]).cuda()
    with torch.no_grad():
        want = f32_model.forward_videos_online(img, ev, lens, 16)
    assert torch.equal(on["scores_device"], torch.sigmoid(want["logits"]))
    assert np.array_equal(np.concatenate(on["scores"]), on["scores_device"].cpu().numpy())
    assert np.array_equal(np.concatenate(got[0]), np.concatenate(on["scores"]))
    assert np.array_equal(np.concatenate(got[2]), want["w_i_mean"].cpu().numpy()) and np.array_equal(np.concatenate(got[3]), want["w_e_mean"].cpu().numpy())
    with pytest.raises(ValueError, match="host_list=False"):
        harness.score_loader(f32_model, items, 256, "cuda:0", "ucfcrime", batch_chunks=3, online_stride=16)


@pytest.mark.parametrize("metric_tail", ["host", "device"])
def test_harness_test_adds_the_online_metrics_and_changes_nothing_else(f32_model, config1_k3, capsys, metric_tail):
    from sklearn.metrics import average_precision_score, roc_auc_score
    g, args, gt = config1_k3
    loader = lambda: harness.get_test_loader(args)      # noqa: E731
    capsys.readouterr()
    base = harness.test(args, f32_model, loader(), 256, None, gt, "cuda:0", metric_tail=metric_tail)
    printed, before = capsys.readouterr().out, harness.test.last_result
    ret = harness.test(args, f32_model, loader(), 256, None, gt, "cuda:0", metric_tail=metric_tail, online_stride=16)
    assert capsys.readouterr().out == printed and ret == base
    last = harness.test.last_result
    assert set(last) == set(before) | {"online", "auc_online", "ap_online"}
    for k in before:
        if k in ("scores", "w_i_mean", "w_e_mean"):
            assert all(np.array_equal(a, b) for a, b in zip(last[k], before[k])), k
        else:
            assert last[k] == before[k], k
    flat = np.repeat(np.concatenate(last["online"]["scores"]).tolist(), 16)
    assert abs(last["auc_online"] - roc_auc_score(gt, flat)) <= 1e-12 and abs(last["ap_online"] - average_precision_score(gt, flat)) <= 1e-12
    assert list(np.diff(last["online"]["row_offsets"])) == list(g["lengths"])
    assert not np.array_equal(np.concatenate(last["online"]["scores"]), np.concatenate(last["scores"]))      # another protocol, other scores


# ---- 8. a plain call is untouched ---------------------------------------------------------------------------------------------------------
def test_plain_calls_keep_their_bits_around_an_online_call():
    model = make_model("f32")                      # default graph_chunks (8): a dense call of B <= 8 replays a captured hipGraph
    direct = make_model("f32", graph_chunks=-1)    # the same kernels launched one by one: what the replays must equal
    vids = videos([37, 300, 256], seed=15)
    img, ev, lens = rows_of(vids)
    a, b = synth.make_inputs(16, 2)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    with torch.no_grad():
        dense0 = {k: v.clone() for k, v in model(da, db, None, None, None).items()}      # captures
        dense1 = {k: v.clone() for k, v in model(da, db, None, None, None).items()}      # replays
        plain0 = {k: v.clone() for k, v in model.forward_videos(img, ev, lens).items()}
        model.forward_videos_online(img, ev, lens, 16)
        model.forward_videos_online(img, ev, lens, 100, history=150)
        plain1 = model.forward_videos(img, ev, lens)
        dense2 = model(da, db, None, None, None)
        want = direct(da, db, None, None, None)
    for k in KEYS:
        assert torch.equal(plain0[k], plain1[k]), k
        assert torch.equal(dense0[k], dense1[k]) and torch.equal(dense0[k], dense2[k]) and torch.equal(dense2[k], want[k]), k
