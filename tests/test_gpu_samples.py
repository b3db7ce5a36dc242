"""The score samples (`MMFMIL.forward_samples`, `MMFMIL.forward_videos_samples`; `iefvad_forward_samples`,
`iefvad_forward_videos_samples`, the kernels of csrc/samples.h) with the harness on top (`score_loader` / `test(..., score_samples=)`).
`-m gpu`.

The reference never samples; tests/golden/make_golden_samples.py captures S = 4 samples from the reference's own pieces and the host
model of the generator (samples_k3.npz).  The shapes are those of tests/test_gpu_variants.py."""
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
from tests import samples_cases as SC
from tests import test_gpu_bf16 as TB
from tests import test_gpu_videos_full as VF

pytestmark = pytest.mark.gpu

T = 256
SEED = 977
LENGTHS = [1, 37, 128, 255, 256, 257, 300]      # one row; short; half; one short of / exactly / one past the chunk edge; two chunks: 9 chunks
SCORE_KEYS = ("logits", "w_i_mean", "w_e_mean")
SAMPLE_KEYS = ("logits_samples", "score_mean", "score_std")
assert TB.TOL_LOGIT_BF16 == SC.TOL_LOGIT_BF16


def make_model(sd, compute="f32", D=768, L_=2, K=3, noise="StudentT", **kw):
    args = argparse.Namespace(visual_layers=L_, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model=noise, nu=8)
    m = iefvad_amd.MMFMIL(14, D, 256, D, 8, L_, 8, 10, 10, "cuda", args, compute=compute, **kw)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


def run(model, img, ev):
    """The model's plain dict (clones: a replayed hipGraph writes where the last call wrote)."""
    with torch.no_grad():
        out = model(img, ev, None, None, None)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


def run_samples(model, img, ev, S, seed=SEED, **kw):
    with torch.no_grad():
        out = model.forward_samples(img, ev, S, seed, **kw)
    torch.cuda.synchronize()
    return out


def run_videos_samples(model, rows, lengths, S, seed=SEED, **kw):
    with torch.no_grad():
        out = model.forward_videos_samples(rows[0], rows[1], lengths, S, seed, **kw)
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


def f32_gate(g, tag="studentt"):
    """The f32 / bf16x6 gate: the suite's logit gate, never below 3 x (the reference's own fp32 floor + the generator's floor)."""
    return max(H.TOL_LOGIT, 3.0 * (float(g["floor_" + tag]) + float(g["eps_floor_" + tag])))


# ---- 1. the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,noise,K", SC.TAGS)
@pytest.mark.parametrize("compute,kw", [("f32", {}), ("bf16x6", dict(batch_invariant=True)), ("bf16", {})], ids=["f32", "bf16x6", "bf16"])
def test_samples_against_the_reference(golden_dir, compute, kw, tag, noise, K):
    """The capture of S = 4 samples from the reference's own pieces (samples_k3.npz).  f32 and bf16x6: max(TOL_LOGIT, 3 x (floor +
    eps_floor)); bf16: 1.5e-2 x max(1, amp), the suite's bf16 logit gate scaled by how much larger the sampled states are than z0.
    Measured on an MI355X (profiles/samples_tests.log), worst over the three tags: f32 1.07e-6, bf16x6 8.3e-7, bf16 2.6e-3."""
    g, cfg, sd, img, ev = SC.load_samples_case(golden_dir)
    S = cfg["S"]
    assert float(g["sep_median_" + tag][~np.eye(S, dtype=bool)].min()) >= 3 * TB.TOL_LOGIT_BF16      # no gate can hide a reused or dropped draw
    model = make_model(sd if K else SC.without_refinement(sd), compute, K=K, noise=noise, **kw)
    got = run_samples(model, torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda(), S, cfg["seed"], scale=cfg["scale"])
    assert got["logits_samples"].shape == (S, cfg["B"], 256)
    ls = got["logits_samples"].cpu().numpy()
    want32 = g["logits_samples_" + tag]
    amp = float(g["amp_" + tag])
    gate = TB.TOL_LOGIT_BF16 * max(1.0, amp) if compute == "bf16" else f32_gate(g, tag)
    err = float(np.abs(ls - want32).max())
    print(f"{compute} {tag}: max |logits_samples - reference| = {err:.3e} (floor {float(g['floor_' + tag]):.1e}, eps_floor "
          f"{float(g['eps_floor_' + tag]):.1e}, amp {amp:.2f}, gate {gate:.1e})")
    assert err <= gate, err


# ---- 2. determinism and routing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_a_sample_does_not_depend_on_the_sample_count(compute):
    model = make_model(state(768, 3), compute)
    img, ev = inputs(2)
    four = run_samples(model, img, ev, 4)
    two = run_samples(model, img, ev, 2)
    again = run_samples(model, img, ev, 4)
    assert torch.equal(four["logits_samples"][:2], two["logits_samples"])
    for k in SAMPLE_KEYS:
        assert torch.equal(four[k], again[k]), k                                  # the same call, the same bits
    other = run_samples(model, img, ev, 2, seed=SEED + 1)
    assert float((other["logits_samples"] - two["logits_samples"]).abs().median()) > TB.TOL_LOGIT_BF16
    assert float((four["logits_samples"][1] - four["logits_samples"][0]).abs().median()) > TB.TOL_LOGIT_BF16


def test_a_snippet_keeps_its_draws_in_any_batch():
    """B = 1 and B = 3 calls with `sample_rows` = the rows' indices in a B = 5 call equal that call's slices, bit for bit (f32)."""
    model = make_model(state(768, 3))
    img, ev = inputs(5)
    five = run_samples(model, img, ev, 4)
    ids = torch.arange(5 * T, dtype=torch.int32, device="cuda")
    for a, b in ((1, 2), (2, 5)):
        part = run_samples(model, img[a:b].contiguous(), ev[a:b].contiguous(), 4, sample_rows=ids[a * T:b * T].contiguous())
        assert torch.equal(part["logits_samples"], five["logits_samples"][:, a:b]), (a, b)
        assert torch.equal(part["score_mean"], five["score_mean"][a:b]) and torch.equal(part["score_std"], five["score_std"][a:b])
    moved = run_samples(model, img[1:2].contiguous(), ev[1:2].contiguous(), 4)    # without ids the chunk is rows 0 .. 255: other draws
    assert float((moved["logits_samples"] - five["logits_samples"][:, 1:2]).abs().median()) > TB.TOL_LOGIT_BF16


def test_samples_across_micro_batch_passes():
    """B = 5 on a micro_batch = 2 model: three passes, the last one partial, each writing its columns and drawing by the row of the CALL."""
    img, ev = inputs(5)
    one = run_samples(make_model(state(768, 3), micro_batch=0), img, ev, 5)
    three = run_samples(make_model(state(768, 3), micro_batch=2), img, ev, 5)
    for k in SAMPLE_KEYS:
        assert torch.equal(one[k], three[k]), k


# ---- 3. scale = 0 ---------------------------------------------------------------------------------------------------------------------
def test_scale_zero_collapses_to_the_calls_score():
    model = make_model(state(768, 3))
    img, ev = inputs(2)
    got = run_samples(model, img, ev, 5, scale=0.0)
    ls = got["logits_samples"]
    for s in range(1, 5):
        assert torch.equal(ls[s], ls[0]), s
    d = max_abs(ls[0], got["logits"].reshape(2, T))
    print("scale = 0: max |sample - logits| =", d, " max score_std =", float(got["score_std"].max()))
    assert d <= H.TOL_LOGIT, d
    assert float(got["score_std"].max()) <= 1e-6
    assert max_abs(got["score_mean"], torch.sigmoid(got["logits"].reshape(2, T))) <= H.TOL_SIGMOID


# ---- 4. valid rows against padded --------------------------------------------------------------------------------------------------------
def dense_samples(model, vids, S, **kw):
    """The samples of the dense call on host-padded chunks with `sample_rows` = the snippet's index in the packed list, `[0:len]` rows."""
    img, ev, index = VF.pad(vids)
    ids = torch.zeros(img.shape[0] * T, dtype=torch.int32, device="cuda")
    ids[index] = torch.arange(index.numel(), dtype=torch.int32, device="cuda")
    out = run_samples(model, img, ev, S, sample_rows=ids, **kw)
    return {"logits_samples": out["logits_samples"].reshape(S, -1)[:, index], "score_mean": out["score_mean"].reshape(-1)[index],
            "score_std": out["score_std"].reshape(-1)[index], "logits": out["logits"].reshape(-1)[index]}


@pytest.mark.parametrize("how", ["default", "micro_batch3", "fp16_rows", "dense_encoder", "d512", "nan"])
def test_forward_videos_samples_equal_the_padded_rows_f32(monkeypatch, how):
    D = 512 if how == "d512" else 768
    vids = videos(D, np.float16 if how == "fp16_rows" else np.float32)
    dense_vids = vids
    if how == "nan":       # test.py:90-95 replaces in the whole image tensor of the video with the NaN: the two-chunk video, second chunk
        vids = H.with_nan(vids, LENGTHS.index(300), T + 20, 11)
        dense_vids = [(np.nan_to_num(v[0]), v[1]) if i == LENGTHS.index(300) else v for i, v in enumerate(vids)]
    if how == "dense_encoder":
        monkeypatch.setenv("IEFVAD_DENSE_ENCODER", "1")
    model = make_model(state(D, 3), "f32", D, micro_batch=3 if how == "micro_batch3" else 0)      # 3: the 257-row video straddles two passes
    with torch.no_grad():
        plain = model.forward_videos(*VF.pack(vids), LENGTHS)
    got = run_videos_samples(model, VF.pack(vids), LENGTHS, 5)
    if how == "dense_encoder":
        monkeypatch.delenv("IEFVAD_DENSE_ENCODER")
    n = sum(LENGTHS)
    assert got["logits_samples"].shape == (5, n) and got["score_mean"].shape == (n,) == got["score_std"].shape      # no column for a pad row
    for key in SCORE_KEYS:
        assert torch.equal(got[key], plain[key]), key
    want = dense_samples(make_model(state(D, 3), "f32", D), dense_vids, 5)
    assert torch.equal(got["logits"], want["logits"])
    for key in SAMPLE_KEYS:
        assert torch.equal(got[key], want[key]), (key, max_abs(got[key], want[key]))
    assert bool(torch.isfinite(got["logits_samples"]).all())
    assert float((got["logits_samples"][4] - got["logits_samples"][0]).abs().median()) > TB.TOL_LOGIT_BF16


@pytest.mark.parametrize("compute,kw,exact", [("bf16", {}, True), ("bf16x6", {}, False), ("bf16x6", dict(batch_invariant=True), True)],
                         ids=["bf16", "bf16x6", "bf16x6-invariant"])
def test_forward_videos_samples_equal_the_padded_rows(golden_dir, compute, kw, exact):
    model = make_model(state(768, 3), compute, **kw)
    vids = videos()
    with torch.no_grad():
        plain = model.forward_videos(*VF.pack(vids), LENGTHS)
    got = run_videos_samples(model, VF.pack(vids), LENGTHS, 4)
    for key in SCORE_KEYS:
        assert torch.equal(got[key], plain[key]), key
    want = dense_samples(model, vids, 4)
    d = max_abs(got["logits_samples"], want["logits_samples"])
    print(compute, kw, "max |valid-row samples - padded samples| =", d)
    if exact:
        for key in SAMPLE_KEYS:
            assert torch.equal(got[key], want[key]), (key, d)
    else:
        assert d <= f32_gate(SC.load_samples_case(golden_dir)[0]), d
        assert max_abs(got["score_mean"], want["score_mean"]) <= H.TOL_SIGMOID


def test_videos_sample_rows_override_the_packed_row():
    model = make_model(state(768, 3))
    rows = VF.pack(videos())
    n = sum(LENGTHS)
    base = run_videos_samples(model, rows, LENGTHS, 2)
    same = run_videos_samples(model, rows, LENGTHS, 2, sample_rows=torch.arange(n, dtype=torch.int32, device="cuda"))
    assert torch.equal(base["logits_samples"], same["logits_samples"])
    moved = run_videos_samples(model, rows, LENGTHS, 2, sample_rows=torch.arange(n, dtype=torch.int32, device="cuda") + 5000)
    assert float((moved["logits_samples"] - base["logits_samples"]).abs().median()) > TB.TOL_LOGIT_BF16


# ---- 5. everything else keeps its bits; S = 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", ["full", "scores"])
@pytest.mark.parametrize("compute,B", [("f32", 2), ("bf16x6", 6), ("bf16", 2)])
def test_the_calls_outputs_keep_their_bits(compute, B, outputs):
    """All eight outputs / the three score vectors of a samples call equal the plain call; a graph-replayed plain call before and after
    the (directly launched) samples call is unchanged."""
    model = make_model(state(768, 3), compute, outputs=outputs, graph_chunks=8)
    direct = make_model(state(768, 3), compute, outputs=outputs, graph_chunks=-1)
    img, ev = inputs(B)
    want = run(direct, img, ev)
    before = run(model, img, ev)
    got = run_samples(model, img, ev, 5)
    after = run(model, img, ev)
    keys = iefvad_amd.OUTPUT_KEYS if outputs == "full" else SCORE_KEYS
    assert set(want) == set(keys) and set(got) == set(keys) | set(SAMPLE_KEYS)
    assert list(got)[-3:] == list(SAMPLE_KEYS)
    for key in keys:
        assert torch.equal(got[key], want[key]), (compute, key, max_abs(got[key], want[key]))
        assert torch.equal(before[key], want[key]) and torch.equal(after[key], want[key]), (compute, key)
    assert bool(torch.isfinite(got["logits_samples"]).all()) and got["logits_samples"].shape == (5, B, T)


def test_a_last_group_of_one():
    """S = 5: a group of four and a group of one (another row count in the stacked tail); S = 8: two full groups."""
    model = make_model(state(768, 3))
    img, ev = inputs(2)
    five = run_samples(model, img, ev, 5)
    eight = run_samples(model, img, ev, 8)
    one = run_samples(model, img, ev, 1)
    assert torch.equal(five["logits_samples"], eight["logits_samples"][:5])
    assert torch.equal(one["logits_samples"], five["logits_samples"][:1])
    sep = (five["logits_samples"][4] - five["logits_samples"][:4]).abs().reshape(4, -1).median(dim=1).values
    assert float(sep.min()) > TB.TOL_LOGIT_BF16                                   # the fifth sample is a fifth draw
    assert float(one["score_std"].max()) == 0.0 and max_abs(one["score_mean"], torch.sigmoid(one["logits_samples"][0])) <= H.TOL_SIGMOID


# ---- 6. the reduction ---------------------------------------------------------------------------------------------------------------------
def test_mean_and_std_of_64_samples():
    """S = 64 on 337 rows: score_mean within TOL_SIGMOID, score_std^2 within 2e-6 of the fp64 reduction of the call's own logits_samples
    (the variance, not its ill-conditioned square root at 0)."""
    model = make_model(state(768, 3))
    vids = tuple(synth.make_video(12, i, n) for i, n in enumerate([37, 300]))
    got = run_videos_samples(model, VF.pack(vids), [37, 300], 64)
    sc = torch.sigmoid(got["logits_samples"].double())
    e_mean = max_abs(got["score_mean"], sc.mean(0))
    e_var = max_abs(got["score_std"].double() ** 2, sc.var(0, unbiased=False))
    print(f"S = 64: max |score_mean - fp64| = {e_mean:.3e}, max |score_std^2 - fp64| = {e_var:.3e}, median std {float(got['score_std'].median()):.3f}")
    assert e_mean <= H.TOL_SIGMOID and e_var <= 2e-6
    assert float(got["score_std"].median()) > 1e-3                                # a spread is there to be reduced


# ---- 7. the C entries ---------------------------------------------------------------------------------------------------------------------
def samples_struct(S, ls, mean, std, stride, seed=SEED, scale=1.0, ids=None):
    p = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    return L.Samples(S, seed, scale, p(ids), p(ls), stride, p(mean), p(std))


def c_call(model, img, ev, B, sm, workspace_bytes=None, out=None):
    lib = L.load_library()
    ws = torch.empty(max(lib.iefvad_samples_workspace_bytes(model._handle, B), 16), dtype=torch.uint8, device="cuda")
    o = out if out is not None else L.Outputs()
    return lib.iefvad_forward_samples(model._handle, C.c_void_p(img.data_ptr()), C.c_void_p(ev.data_ptr()), L.IN_F32, B, C.c_void_p(ws.data_ptr()),
                                      ws.numel() if workspace_bytes is None else workspace_bytes, C.byref(o),
                                      C.byref(sm) if sm is not None else None, C.c_void_p(torch.cuda.current_stream().cuda_stream)), ws


def test_sentinels_around_a_strided_result_survive():
    """A [S, stride] result with stride > rows inside a larger buffer: only [s, 0 : rows] is written; likewise the two vectors."""
    B, S, stride, guard = 2, 5, 2 * T + 24, 8
    model = make_model(state(768, 3))
    img, ev = inputs(B)
    full = run_samples(model, img, ev, S)
    buf = torch.full((guard + S * stride + guard,), -777.0, device="cuda")
    vec = torch.full((2, guard + B * T + guard), -777.0, device="cuda")
    logits = torch.empty(B * T, device="cuda")
    o = L.Outputs()
    o.logits = logits.data_ptr()
    rc, _ = c_call(model, img, ev, B, samples_struct(S, buf[guard:], vec[0, guard:], vec[1, guard:], stride), out=o)
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    body = buf[guard:guard + S * stride].reshape(S, stride)
    assert torch.equal(body[:, :B * T], full["logits_samples"].reshape(S, -1))
    assert bool((body[:, B * T:] == -777.0).all()) and bool((buf[:guard] == -777.0).all()) and bool((buf[-guard:] == -777.0).all())
    assert torch.equal(vec[0, guard:-guard], full["score_mean"].reshape(-1)) and torch.equal(vec[1, guard:-guard], full["score_std"].reshape(-1))
    assert bool((vec[:, :guard] == -777.0).all()) and bool((vec[:, -guard:] == -777.0).all())
    assert torch.equal(logits, full["logits"].reshape(-1))


def test_c_entry_refusals():
    lib = L.load_library()
    B, S = 1, 4
    img, ev = inputs(B)
    model = make_model(state(768, 3))
    run(model, img, ev)                      # the handle exists
    buf = torch.empty(S, B * T + 8, device="cuda")
    mean, std = torch.empty(B * T, device="cuda"), torch.empty(B * T, device="cuda")
    who = "iefvad_forward_samples:"

    def refused(rc, *words):
        assert rc != 0
        assert L.last_error().startswith(who) and all(w in L.last_error() for w in words), L.last_error()

    ok = samples_struct(S, buf, mean, std, B * T)
    refused(c_call(model, img, ev, B, ok, workspace_bytes=lib.iefvad_workspace_bytes(model._handle, B))[0], "workspace too small")
    assert lib.iefvad_samples_workspace_bytes(model._handle, B) == lib.iefvad_variants_workspace_bytes(model._handle, B, 4) > \
        lib.iefvad_workspace_bytes(model._handle, B)
    refused(c_call(model, img, ev, B, samples_struct(0, buf, mean, std, B * T))[0], "samples 0 outside 1..64")
    refused(c_call(model, img, ev, B, samples_struct(65, buf, mean, std, B * T))[0], "samples 65 outside 1..64")
    refused(c_call(model, img, ev, B, samples_struct(S, buf, mean, std, B * T, scale=-1.0))[0], "scale")
    refused(c_call(model, img, ev, B, samples_struct(S, buf, mean, std, B * T, scale=float("inf")))[0], "scale")
    refused(c_call(model, img, ev, B, samples_struct(S, buf, mean, std, B * T, scale=float("nan")))[0], "scale")
    refused(c_call(model, img, ev, B, samples_struct(S, buf, mean, std, B * T - 1))[0], "stride")
    refused(c_call(model, img, ev, B, None)[0], "null samples")
    refused(c_call(model, img, ev, B, samples_struct(S, None, mean, std, B * T))[0], "null logits_samples")
    refused(c_call(model, img, ev, B, samples_struct(S, buf, None, std, B * T))[0], "null score_mean")
    refused(c_call(model, img, ev, B, samples_struct(S, buf, mean, None, B * T))[0], "null score_std")
    refused(c_call(model, img, ev, B, samples_struct(S, buf.reshape(-1).view(torch.uint8)[2:], mean, std, B * T))[0], "4-byte aligned")
    f16 = make_model(state(768, 3), "fp16x3")
    run(f16, img, ev)
    refused(c_call(f16, img, ev, B, ok)[0], "FP16X3")
    # the whole-video entry: the same checks under its own name
    who = "iefvad_forward_videos_samples:"
    rows = VF.pack(videos())
    lens = (C.c_int32 * len(LENGTHS))(*LENGTHS)
    n = sum(LENGTHS)
    vec = torch.empty(5, n, device="cuda")
    big = torch.empty(S, n, device="cuda")
    need = lib.iefvad_videos_samples_workspace_bytes(model._handle, lens, len(LENGTHS))
    assert need == lib.iefvad_videos_variants_workspace_bytes(model._handle, lens, len(LENGTHS), 4) > \
        lib.iefvad_videos_workspace_bytes(model._handle, lens, len(LENGTHS))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def vcall(m, sm, nbytes):
        return lib.iefvad_forward_videos_samples(m._handle, C.c_void_p(rows[0].data_ptr()), C.c_void_p(rows[1].data_ptr()), L.IN_F32, lens, len(LENGTHS), 1,
                                                 C.c_void_p(ws.data_ptr()), nbytes, C.c_void_p(vec[0].data_ptr()), C.c_void_p(vec[1].data_ptr()),
                                                 C.c_void_p(vec[2].data_ptr()), C.byref(sm) if sm is not None else None, None)
    refused(vcall(model, samples_struct(S, big, vec[3], vec[4], n), need - 1), "workspace too small")
    refused(vcall(model, samples_struct(S, big, vec[3], vec[4], n - 1), need), "stride")
    refused(vcall(model, samples_struct(0, big, vec[3], vec[4], n), need), "samples 0 outside")
    refused(vcall(model, samples_struct(S, big, vec[3], vec[4], n, scale=-0.5), need), "scale")
    refused(vcall(model, samples_struct(S, big, None, vec[4], n), need), "null score_mean")
    refused(vcall(model, None, need), "null samples")
    refused(vcall(f16, samples_struct(S, big, vec[3], vec[4], n), need), "FP16X3")
    with pytest.raises(RuntimeError, match="fp16x3"):
        f16.forward_samples(img, ev, 4, 1)
    # nothing was launched or disturbed: the model still answers as before
    again = run_samples(model, img, ev, 2, scale=0.0)
    assert max_abs(again["logits_samples"][0], again["logits"].reshape(B, T)) <= H.TOL_LOGIT


# ---- 8. the harness -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def config1_k3(tmp_path_factory, golden_dir):
    g, args, gt, _ = H.write_config1_set(tmp_path_factory.mktemp("cfg1smp"), golden_dir)
    return g, args, gt, synth.make_state_dict(int(g["wseed"]), 768, 2, 3)


def test_harness_samples(config1_k3, capsys):
    from sklearn.metrics import average_precision_score, roc_auc_score
    g, args, gt, sd = config1_k3
    model = make_model(sd)
    loader = lambda: harness.get_test_loader(args)      # noqa: E731
    S = 4
    per_route = []
    for batch_chunks in (0, 8):
        capsys.readouterr()
        base = harness.test(args, model, loader(), 256, None, gt, "cuda:0", batch_chunks=batch_chunks)
        printed = capsys.readouterr().out
        base_last = harness.test.last_result
        ret = harness.test(args, model, loader(), 256, None, gt, "cuda:0", batch_chunks=batch_chunks, score_samples=S, sample_seed=SEED)
        assert capsys.readouterr().out == printed                     # nothing new is printed
        last = harness.test.last_result
        assert ret == base                                            # the returned AUC / AP are those of the call without the keyword
        assert set(last) == set(base_last) | {"samples", "auc_samples", "ap_samples", "auc_mean_score", "ap_mean_score"}
        assert all(np.array_equal(a, b) for a, b in zip(last["scores"], base_last["scores"])) and len(last["scores"]) == len(base_last["scores"])
        sm = last["samples"]
        n = int(g["lengths"].sum())
        assert set(sm) == {"scores_mean", "scores_std", "logits_samples_device", "row_offsets"}
        assert tuple(sm["logits_samples_device"].shape) == (S, n) and list(np.diff(sm["row_offsets"])) == list(g["lengths"])
        assert [a.shape for a in sm["scores_mean"]] == [(int(k),) for k in g["lengths"]] == [a.shape for a in sm["scores_std"]]
        sc = torch.sigmoid(sm["logits_samples_device"]).cpu().numpy()
        mean = np.concatenate(sm["scores_mean"])
        assert float(np.abs(mean - sc.astype(np.float64).mean(0)).max()) <= H.TOL_SIGMOID
        assert len(last["auc_samples"]) == S == len(last["ap_samples"]) and len(set(last["auc_samples"])) == S      # S draws, S figures
        for s in range(S):
            assert abs(last["auc_samples"][s] - roc_auc_score(gt, np.repeat(sc[s].tolist(), 16))) <= 1e-12
            assert abs(last["ap_samples"][s] - average_precision_score(gt, np.repeat(sc[s].tolist(), 16))) <= 1e-12
        assert abs(last["auc_mean_score"] - roc_auc_score(gt, np.repeat(mean.tolist(), 16))) <= 1e-12
        assert abs(last["ap_mean_score"] - average_precision_score(gt, np.repeat(mean.tolist(), 16))) <= 1e-12
        per_route.append(sm["logits_samples_device"].clone())
    assert torch.equal(per_route[0], per_route[1])      # f32: a snippet's samples depend neither on the route nor on the batches
    dev = harness.test(args, model, loader(), 256, None, gt, "cuda:0", batch_chunks=8, score_samples=S, sample_seed=SEED, metric_tail="device")
    dl = harness.test.last_result
    capsys.readouterr()
    assert abs(dev[0] - ret[0]) <= 1e-12
    for s in range(S):
        assert abs(dl["auc_samples"][s] - last["auc_samples"][s]) <= 1e-12 and abs(dl["ap_samples"][s] - last["ap_samples"][s]) <= 1e-12, s
    assert abs(dl["auc_mean_score"] - last["auc_mean_score"]) <= 1e-12 and abs(dl["ap_mean_score"] - last["ap_mean_score"]) <= 1e-12
    sub = harness.ucf_test(args, model, loader(), 256, None, gt, "cuda:0", batch_chunks=8, score_samples=2, sample_seed=SEED)
    assert sub == ret and harness.ucf_test.last_result["auc_samples"] == last["auc_samples"][:2]
    with pytest.raises(ValueError, match="host_list=False"):
        harness.score_loader(model, loader(), 256, "cuda:0", "ucfcrime", batch_chunks=8, host_list=True, score_samples=S, sample_seed=SEED)
