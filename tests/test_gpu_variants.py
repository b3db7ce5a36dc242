"""The fusion ablations (`forward(..., fusion_variants=)`, `forward_videos(..., fusion_variants=)`; `iefvad_forward_variants`,
`iefvad_forward_videos_variants`, `iefvad_fusion_variants_kernel` in csrc/variants.h) with the harness on top (`score_loader` /
`test(..., fusion_variants=)`).  `-m gpu`.

The reference forms `fused` inline; tests/golden/make_golden_variants.py captures the four substitutions from the reference's own
pieces (variants_k3.npz), tests/variants_cases.py restates them in fp64 where the fixture has no capture."""
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
from tests import variants_cases as VC
from tests.test_trajectory_cpu import truncated

pytestmark = pytest.mark.gpu

T = 256
NAMES = VC.NAMES
LENGTHS = [1, 37, 128, 255, 256, 257, 300]      # one row; short; half; one short of / exactly / one past the chunk edge; two chunks: 9 chunks
SCORE_KEYS = ("logits", "w_i_mean", "w_e_mean")
assert (TB.TOL_LOGIT_BF16, TB.TOL_SIGMOID_BF16) == (VC.TOL_LOGIT_BF16, VC.TOL_SIGMOID_BF16)


def make_model(sd, compute="f32", D=768, L_=2, K=3, noise="StudentT", **kw):
    args = argparse.Namespace(visual_layers=L_, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model=noise, nu=8)
    m = iefvad_amd.MMFMIL(14, D, 256, D, 8, L_, 8, 10, 10, "cuda", args, compute=compute, **kw)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


def run(model, img, ev, **kw):
    """The model's dict (clones: a replayed hipGraph writes where the last call wrote)."""
    with torch.no_grad():
        out = model(img, ev, None, None, None, **kw)
    torch.cuda.synchronize()
    return {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in out.items()}


def run_videos(model, rows, lengths, **kw):
    with torch.no_grad():
        out = model.forward_videos(rows[0], rows[1], lengths, **kw)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def state(D, K):
    return synth.make_state_dict(44, D, 2, K)


@functools.lru_cache(maxsize=None)
def inputs(B, D=768):
    img, ev = synth.make_inputs(10, B, D=D)
    img[B - 1, 100:] = 0      # a padded tail in the last chunk
    ev[B - 1, 100:] = 0
    return torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()


@functools.lru_cache(maxsize=None)
def videos(D=768, dtype=np.float32):
    return tuple(synth.make_video(12, i, n, D=D, dtype=dtype) for i, n in enumerate(LENGTHS))


def max_abs(a, b):
    return float((a.double() - b.double()).abs().max())


# ---- 1. the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,noise,K", [("studentt", "StudentT", 3), ("gaussian", "Gaussian", 3), ("k0", "StudentT", 0)])
@pytest.mark.parametrize("compute,kw,tol_logit,tol_sig", [
    ("f32", {}, H.TOL_LOGIT, H.TOL_SIGMOID),
    ("bf16x6", dict(batch_invariant=True), H.TOL_LOGIT, H.TOL_SIGMOID),      # B = 2 in the split arithmetic, not on the fp32 kernels
    ("bf16", {}, TB.TOL_LOGIT_BF16, TB.TOL_SIGMOID_BF16),
], ids=["f32", "bf16x6", "bf16"])
def test_variants_against_the_reference(golden_dir, compute, kw, tol_logit, tol_sig, tag, noise, K):
    """The reference's capture of the four substitutions (variants_k3.npz): logits within the arithmetic's logit gate, their sigmoid
    within its sigmoid gate; each gate never below 3 x the reference's own fp32-versus-fp64 distance on that quantity."""
    g, cfg, sd, img, ev = VC.load_variants_case(golden_dir)
    off = ~np.eye(4, dtype=bool)
    assert float(g["sep_median_" + tag][off].min()) >= 3 * TB.TOL_LOGIT_BF16      # no gate can hide a swapped or dropped substitution
    model = make_model(sd if K else VC.without_refinement(sd), compute, K=K, noise=noise, **kw)
    got = run(model, torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda(), fusion_variants=True)
    assert got["fusion_variants"] == NAMES and got["logits_variants"].shape == (4, cfg["B"], 256)
    lv = got["logits_variants"].cpu().numpy()
    want32, want64 = g["logits_variants_" + tag], g["logits_variants_" + tag + "_f64"]
    for v, name in enumerate(NAMES):
        floor = float(g["floor_" + tag][v])
        floor_sig = float(np.abs(H.sigmoid(want32[v]) - H.sigmoid(want64[v])).max())
        e_logit = float(np.abs(lv[v] - want32[v]).max())
        e_sig = float(np.abs(H.sigmoid(lv[v]) - H.sigmoid(want32[v])).max())
        gate, gate_sig = max(tol_logit, 3.0 * floor), max(tol_sig, 3.0 * floor_sig)
        print(f"{compute} {tag} {name}: max |logits - reference| = {e_logit:.3e} (floor {floor:.1e}, gate {gate:.1e}); "
              f"sigmoid {e_sig:.3e} (floor {floor_sig:.1e}, gate {gate_sig:.1e})")
        assert e_logit <= gate, (name, e_logit)
        assert e_sig <= gate_sig, (name, e_sig)


# ---- 2. "fused" is the call's own score ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute,B,kw,exact", [
    ("f32", 1, {}, True), ("f32", 2, {}, True), ("f32", 3, {}, True),
    ("bf16", 1, {}, True),                               # 4 row blocks: the call's chain launch, and one chain launch over the 16 stacked blocks
    ("bf16", 6, {}, True),
    ("bf16x6", 2, {}, False),                            # on the fp32 kernels
    ("bf16x6", 6, {}, False),                            # 72 workgroups: the split kernels and the folded scorer, in the call and in the stacked tail
    ("bf16x6", 2, dict(batch_invariant=True), True),
    ("bf16x6", 6, dict(batch_invariant=True), True),
], ids=lambda v: str(v).replace(" ", ""))
def test_fused_row_is_the_calls_logits(compute, B, kw, exact):
    model = make_model(state(768, 3), compute, **kw)
    img, ev = inputs(B)
    got = run(model, img, ev, fusion_variants=True)
    fused, logits = got["logits_variants"][0], got["logits"].reshape(B, T)
    assert bool(torch.isfinite(got["logits_variants"]).all())
    d = max_abs(fused, logits)
    print(compute, B, kw, "max |fused row - logits| =", d)
    if exact:
        assert torch.equal(fused, logits), d
    else:
        assert d <= H.TOL_LOGIT, d
    for v in range(1, 4):      # the other rows are other scores: a copy of the fused row would lie within the loosest gate of it
        assert float((got["logits_variants"][v] - logits).abs().median()) > TB.TOL_LOGIT_BF16, NAMES[v]


@pytest.mark.parametrize("env,names", [
    (dict(IEFVAD_CHAIN_MIN_BLOCKS="8"), NAMES),             # the call's 4 blocks launch per projection, the 16 stacked ones take the chain kernel
    (dict(IEFVAD_CHAIN_MIN_BLOCKS="8"), ("fused",)),        # 4 stacked blocks: launch per projection on the bf16 copy of the stacked state
    (dict(IEFVAD_ROWBLOCK_OFF="8"), NAMES),                 # no chain kernel at all
    (dict(IEFVAD_ROWBLOCK_MIN_WGS="12"), NAMES),            # the heads row-block kernel stores mu / logvar for the variants
], ids=lambda v: str(v).replace(" ", ""))
def test_fused_row_on_every_bf16_route(monkeypatch, env, names):
    """The switches are read when the handle is created, i.e. on the model's first call."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model = make_model(state(768, 3), "bf16")
    img, ev = inputs(1)
    plain = run(model, img, ev)
    got = run(model, img, ev, fusion_variants=names)
    assert torch.equal(got["logits_variants"][names.index("fused")], got["logits"].reshape(1, T))
    for key in iefvad_amd.OUTPUT_KEYS:
        assert torch.equal(got[key], plain[key]), key
    for k in env:
        monkeypatch.delenv(k)
    want = run(make_model(state(768, 3), "bf16"), img, ev, fusion_variants=names)      # the default routes: the same bits
    assert torch.equal(got["logits_variants"], want["logits_variants"])


def test_fused_row_on_the_whole_video_route():
    model = make_model(state(768, 3))
    got = run_videos(model, VF.pack(videos()), LENGTHS, fusion_variants=True)
    assert torch.equal(got["logits_variants"][0], got["logits"])


# ---- 3. everything else keeps its bits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", ["full", "scores"])
@pytest.mark.parametrize("compute,B", [("f32", 2), ("bf16x6", 6), ("bf16", 2)])
def test_the_calls_outputs_keep_their_bits(compute, B, outputs):
    """All eight outputs / both weight means of a call with variants equal the call without; a graph-replayed plain call before and
    after the (directly launched) variants call is unchanged."""
    model = make_model(state(768, 3), compute, outputs=outputs, graph_chunks=8)
    direct = make_model(state(768, 3), compute, outputs=outputs, graph_chunks=-1)
    img, ev = inputs(B)
    want = run(direct, img, ev)
    before = run(model, img, ev)
    got = run(model, img, ev, fusion_variants=True)
    after = run(model, img, ev)
    keys = iefvad_amd.OUTPUT_KEYS if outputs == "full" else SCORE_KEYS
    assert set(want) == set(keys) and set(got) == set(keys) | {"logits_variants", "fusion_variants"}
    for key in keys:
        assert torch.equal(got[key], want[key]), (compute, key, max_abs(got[key], want[key]))
        assert torch.equal(before[key], want[key]) and torch.equal(after[key], want[key]), (compute, key)


# ---- 4. routes ----------------------------------------------------------------------------------------------------------------------------
def dense_variants(model, vids, **kw):
    """The variants of the dense call on host-padded chunks, `[0:len]` rows of every video."""
    img, ev, index = VF.pad(vids)
    out = run(model, img, ev, fusion_variants=True, **kw)
    return out["logits_variants"].reshape(4, -1)[:, index], out["logits"].reshape(-1)[index]


@pytest.mark.parametrize("how", ["default", "micro_batch3", "fp16_rows", "dense_encoder", "d512", "nan"])
def test_forward_videos_variants_equal_the_padded_rows_f32(monkeypatch, how):
    D = 512 if how == "d512" else 768
    vids = videos(D, np.float16 if how == "fp16_rows" else np.float32)
    dense_vids = vids
    if how == "nan":       # test.py:90-95 replaces in the whole image tensor of the video with the NaN: the two-chunk video, second chunk
        vids = H.with_nan(vids, LENGTHS.index(300), T + 20, 11)
        dense_vids = [(np.nan_to_num(v[0]), v[1]) if i == LENGTHS.index(300) else v for i, v in enumerate(vids)]
    if how == "dense_encoder":
        monkeypatch.setenv("IEFVAD_DENSE_ENCODER", "1")
    model = make_model(state(D, 3), "f32", D, micro_batch=3 if how == "micro_batch3" else 0)      # 3: the 257-row video straddles two passes
    plain = run_videos(model, VF.pack(vids), LENGTHS)
    got = run_videos(model, VF.pack(vids), LENGTHS, fusion_variants=True)
    if how == "dense_encoder":
        monkeypatch.delenv("IEFVAD_DENSE_ENCODER")
    n = sum(LENGTHS)
    assert got["logits_variants"].shape == (4, n) and got["fusion_variants"] == NAMES       # no column for a pad row or an empty chunk
    for key in SCORE_KEYS:
        assert torch.equal(got[key], plain[key]), key
    want, want_logits = dense_variants(make_model(state(D, 3), "f32", D), dense_vids)
    assert torch.equal(got["logits"], want_logits)
    assert torch.equal(got["logits_variants"], want), max_abs(got["logits_variants"], want)
    assert bool(torch.isfinite(got["logits_variants"]).all())


@pytest.mark.parametrize("compute,exact", [("bf16", True), ("bf16x6", False)])
def test_forward_videos_variants_equal_the_padded_rows(compute, exact):
    model = make_model(state(768, 3), compute)
    vids = videos()
    plain = run_videos(model, VF.pack(vids), LENGTHS)
    got = run_videos(model, VF.pack(vids), LENGTHS, fusion_variants=True)
    for key in SCORE_KEYS:
        assert torch.equal(got[key], plain[key]), key
    want, _ = dense_variants(model, vids)
    d = max_abs(got["logits_variants"], want)
    print(compute, "max |valid-row variants - padded variants| =", d)
    if exact:
        assert torch.equal(got["logits_variants"], want), d
    else:
        assert d <= H.TOL_LOGIT, d


def test_variants_across_micro_batch_passes():
    """B = 5 on a micro_batch = 2 model: three passes, the last one partial, each writing its columns of the call's result."""
    img, ev = inputs(5)
    one = run(make_model(state(768, 3), micro_batch=0), img, ev, fusion_variants=True)
    three = run(make_model(state(768, 3), micro_batch=2), img, ev, fusion_variants=True)
    assert torch.equal(one["logits_variants"], three["logits_variants"])


# ---- 5. order, subsets, stride ---------------------------------------------------------------------------------------------------------
def test_order_and_subsets():
    model = make_model(state(768, 3))
    img, ev = inputs(2)
    full = run(model, img, ev, fusion_variants=True)
    two = run(model, img, ev, fusion_variants=("event", "image"))
    assert two["fusion_variants"] == ("event", "image") and two["logits_variants"].shape == (2, 2, T)
    assert torch.equal(two["logits_variants"][0], full["logits_variants"][2]) and torch.equal(two["logits_variants"][1], full["logits_variants"][1])
    for v, name in enumerate(NAMES):      # V = 1
        one = run(model, img, ev, fusion_variants=name)
        assert one["logits_variants"].shape == (1, 2, T) and torch.equal(one["logits_variants"][0], full["logits_variants"][v]), name
    rows = VF.pack(videos())
    vfull = run_videos(model, rows, LENGTHS, fusion_variants=True)
    vtwo = run_videos(model, rows, LENGTHS, fusion_variants=["equal", "fused"])
    assert torch.equal(vtwo["logits_variants"][0], vfull["logits_variants"][3]) and torch.equal(vtwo["logits_variants"][1], vfull["logits_variants"][0])


def c_call(model, img, ev, B, variants, workspace_bytes=None, out=None):
    lib = L.load_library()
    need = lib.iefvad_variants_workspace_bytes(model._handle, B, max(1, min(4, variants.count)) if variants is not None else 1)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    o = out if out is not None else L.Outputs()
    return lib.iefvad_forward_variants(model._handle, C.c_void_p(img.data_ptr()), C.c_void_p(ev.data_ptr()), L.IN_F32, B, C.c_void_p(ws.data_ptr()),
                                       ws.numel() if workspace_bytes is None else workspace_bytes, C.byref(o),
                                       C.byref(variants) if variants is not None else None, C.c_void_p(torch.cuda.current_stream().cuda_stream)), ws


def variants_struct(kinds, buf, stride):
    v = L.Variants()
    v.count = len(kinds)
    for j, k in enumerate(kinds[:4]):
        v.kind[j] = k
    v.logits, v.stride = (buf.data_ptr() if buf is not None else None), stride
    return v


def test_sentinels_around_a_strided_result_survive():
    """A [V, stride] result with stride > rows inside a larger buffer: only [v, 0 : rows] is written."""
    B, stride, guard = 2, 2 * T + 24, 8
    model = make_model(state(768, 3))
    img, ev = inputs(B)
    full = run(model, img, ev, fusion_variants=True)
    buf = torch.full((guard + 3 * stride + guard,), -777.0, device="cuda")
    logits = torch.empty(B * T, device="cuda")
    o = L.Outputs()
    o.logits = logits.data_ptr()
    rc, _ = c_call(model, img, ev, B, variants_struct([3, 1, 0], buf[guard:], stride), out=o)
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    body = buf[guard:guard + 3 * stride].reshape(3, stride)
    for j, v in enumerate((3, 1, 0)):
        assert torch.equal(body[j, :B * T], full["logits_variants"][v].reshape(-1)), NAMES[v]
    assert bool((body[:, B * T:] == -777.0).all()) and bool((buf[:guard] == -777.0).all()) and bool((buf[-guard:] == -777.0).all())
    assert torch.equal(logits, full["logits"].reshape(-1))


# ---- 6. the step count --------------------------------------------------------------------------------------------------------------------
def test_variants_follow_set_steps():
    sd = state(768, 3)
    img, ev = inputs(2)
    model = make_model(sd)
    full = run(model, img, ev, fusion_variants=True)
    model.set_steps(1)
    got = run(model, img, ev, fusion_variants=True)
    want = run(make_model(truncated(sd, 1), K=1), img, ev, fusion_variants=True)
    assert torch.equal(got["logits_variants"], want["logits_variants"]) and torch.equal(got["logits"], want["logits"])
    assert not torch.equal(got["logits_variants"], full["logits_variants"])
    model.set_steps(None)
    assert torch.equal(run(model, img, ev, fusion_variants=True)["logits_variants"], full["logits_variants"])


# ---- 7. D = 512 ---------------------------------------------------------------------------------------------------------------------------
def test_d512_against_the_restatement_on_the_calls_heads():
    D, K = 512, 3
    sd = state(D, K)
    model = make_model(sd, "f32", D)
    img, ev = inputs(2, D)
    got = run(model, img, ev, fusion_variants=True)
    heads = [got[k].cpu().numpy() for k in ("image_mu", "image_logvar", "event_mu", "event_logvar")]
    want = VC.variant_logits(sd, *heads, K=K, lam=0.5, noise="StudentT", nu=8)
    lv = got["logits_variants"].cpu().numpy()
    for v, name in enumerate(NAMES):
        err = float(np.abs(lv[v] - want[v]).max())
        print(f"D = 512 {name}: max |logits - fp64 restatement| = {err:.3e} (gate {H.TOL_LOGIT:.1e})")
        assert err <= H.TOL_LOGIT, (name, err)
    sep = np.abs(want[:, None] - want[None, :]).reshape(4, 4, -1)
    assert float(np.median(sep, axis=2)[~np.eye(4, dtype=bool)].min()) > 100 * H.TOL_LOGIT      # the four rows are four scores
    assert torch.equal(got["logits_variants"][0], got["logits"].reshape(2, T))


# ---- 8. refusals through the C entry ------------------------------------------------------------------------------------------------------
def test_c_entry_refusals():
    lib = L.load_library()
    B = 1
    img, ev = inputs(B)
    model = make_model(state(768, 3))
    run(model, img, ev)                      # the handle exists
    buf = torch.empty(4, B * T + 8, device="cuda")
    who = "iefvad_forward_variants:"

    def refused(rc, *words):
        assert rc != 0
        assert L.last_error().startswith(who) and all(w in L.last_error() for w in words), L.last_error()

    ok = variants_struct([0, 1, 2, 3], buf, B * T)
    refused(c_call(model, img, ev, B, ok, workspace_bytes=lib.iefvad_workspace_bytes(model._handle, B))[0], "workspace too small")
    assert lib.iefvad_variants_workspace_bytes(model._handle, B, 4) > lib.iefvad_variants_workspace_bytes(model._handle, B, 1) > \
        lib.iefvad_workspace_bytes(model._handle, B)
    assert lib.iefvad_variants_workspace_bytes(model._handle, B, 0) == 0 and lib.iefvad_variants_workspace_bytes(model._handle, B, 5) == 0
    refused(c_call(model, img, ev, B, variants_struct([0, 1], buf, B * T - 1))[0], "stride")
    refused(c_call(model, img, ev, B, variants_struct([1, 2, 1], buf, B * T))[0], "repeated")
    refused(c_call(model, img, ev, B, variants_struct([0, 4], buf, B * T))[0], "unknown variant kind")
    refused(c_call(model, img, ev, B, variants_struct([], buf, B * T))[0], "count 0")
    refused(c_call(model, img, ev, B, variants_struct([0, 1, 2, 3, 0], buf, B * T))[0], "count 5")
    refused(c_call(model, img, ev, B, None)[0], "null variants")
    refused(c_call(model, img, ev, B, variants_struct([0], None, B * T))[0], "null variants logits")
    refused(c_call(model, img, ev, B, variants_struct([0], buf.reshape(-1).view(torch.uint8)[2:], B * T))[0], "4-byte aligned")
    f16 = make_model(state(768, 3), "fp16x3")
    run(f16, img, ev)
    refused(c_call(f16, img, ev, B, ok)[0], "FP16X3")
    # the whole-video entry: the same checks under its own name
    who = "iefvad_forward_videos_variants:"
    rows = VF.pack(videos())
    lens = (C.c_int32 * len(LENGTHS))(*LENGTHS)
    n = sum(LENGTHS)
    vec = torch.empty(3, n, device="cuda")
    big = torch.empty(4, n, device="cuda")
    need = lib.iefvad_videos_variants_workspace_bytes(model._handle, lens, len(LENGTHS), 4)
    assert need > lib.iefvad_videos_workspace_bytes(model._handle, lens, len(LENGTHS))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def vcall(m, variants, nbytes):
        return lib.iefvad_forward_videos_variants(m._handle, C.c_void_p(rows[0].data_ptr()), C.c_void_p(rows[1].data_ptr()), L.IN_F32, lens, len(LENGTHS), 1,
                                                  C.c_void_p(ws.data_ptr()), nbytes, C.c_void_p(vec[0].data_ptr()), C.c_void_p(vec[1].data_ptr()),
                                                  C.c_void_p(vec[2].data_ptr()), C.byref(variants) if variants is not None else None, None)
    refused(vcall(model, variants_struct([0, 1, 2, 3], big, n), need - 1), "workspace too small")
    refused(vcall(model, variants_struct([0, 1, 2, 3], big, n - 1), need), "stride")
    refused(vcall(model, variants_struct([2, 2], big, n), need), "repeated")
    refused(vcall(model, variants_struct([], big, n), need), "count 0")
    refused(vcall(model, None, need), "null variants")
    refused(vcall(f16, variants_struct([0], big, n), need), "FP16X3")
    with pytest.raises(RuntimeError, match="fp16x3"):
        f16(img, ev, None, None, None, fusion_variants=True)
    # nothing was launched or disturbed: the model still answers as before
    again = run(model, img, ev, fusion_variants=True)
    assert torch.equal(again["logits_variants"][0], again["logits"].reshape(B, T))


# ---- 9. the harness -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def config1_k3(tmp_path_factory, golden_dir):
    g, args, gt, _ = H.write_config1_set(tmp_path_factory.mktemp("cfg1var"), golden_dir)
    return g, args, gt, synth.make_state_dict(int(g["wseed"]), 768, 2, 3)


@pytest.mark.parametrize("batch_chunks", [0, 8])
def test_harness_variants(config1_k3, capsys, batch_chunks):
    g, args, gt, sd = config1_k3
    model = make_model(sd)
    loader = lambda: harness.get_test_loader(args)      # noqa: E731
    capsys.readouterr()
    base = harness.test(args, model, loader(), 256, None, gt, "cuda:0", batch_chunks=batch_chunks)
    printed = capsys.readouterr().out
    base_last = harness.test.last_result
    ret = harness.test(args, model, loader(), 256, None, gt, "cuda:0", batch_chunks=batch_chunks, fusion_variants=True)
    assert capsys.readouterr().out == printed                     # nothing new is printed
    last = harness.test.last_result
    assert ret == base
    assert set(last) == set(base_last) | {"variants", "auc_variants", "ap_variants"}
    assert last["classes"] == base_last["classes"]
    assert all(np.array_equal(a, b) for a, b in zip(last["scores"], base_last["scores"])) and len(last["scores"]) == len(base_last["scores"])
    va = last["variants"]
    n = int(g["lengths"].sum())
    assert va["names"] == NAMES and tuple(va["scores_device"].shape) == (4, n) and list(np.diff(va["row_offsets"])) == list(g["lengths"])
    assert [s.shape for s in va["scores"]] == [(4, int(k)) for k in g["lengths"]]
    assert np.array_equal(np.concatenate([s[0] for s in va["scores"]]), np.concatenate(last["scores"]))      # "fused" is the call's score
    assert set(last["auc_variants"]) == set(NAMES) == set(last["ap_variants"])
    assert (last["auc_variants"]["fused"], last["ap_variants"]["fused"]) == ret
    assert len({last["auc_variants"][k] for k in NAMES}) == 4                       # four scores, four figures
    capsys.readouterr()
    dev = harness.test(args, model, loader(), 256, None, gt, "cuda:0", batch_chunks=batch_chunks, fusion_variants=True, metric_tail="device")
    dl = harness.test.last_result
    assert (dl["auc_variants"]["fused"], dl["ap_variants"]["fused"]) == dev
    for k in NAMES:
        assert abs(dl["auc_variants"][k] - last["auc_variants"][k]) <= 1e-12 and abs(dl["ap_variants"][k] - last["ap_variants"][k]) <= 1e-12, k
    sub = harness.ucf_test(args, model, loader(), 256, None, gt, "cuda:0", batch_chunks=batch_chunks, fusion_variants=("event", "image"))
    ul = harness.ucf_test.last_result
    assert sub == base and ul["variants"]["names"] == ("event", "image")
    assert ul["auc_variants"] == {k: last["auc_variants"][k] for k in ("event", "image")}
    with pytest.raises(ValueError, match="host_list"):
        harness.score_loader(model, loader(), 256, "cuda:0", "ucfcrime", batch_chunks=8, host_list=True, fusion_variants=True)
