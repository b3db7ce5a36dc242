"""The batch-invariant mode of compute="bf16x6" (`MMFMIL(..., batch_invariant=True)`, `iefvad_set_batch_invariant`,
LaunchPolicy::split_always in csrc/launch_rules.h, the small tiling of csrc/gemm_split_small.h): every projection and attention of the
evaluation forward runs in the split arithmetic at every row count, so a chunk's or a video's results are the same bits whatever else
is in the launch -- B = 1 or 48, padded or valid rows, per video, packed or from host lists, launched directly or replayed from a
hipGraph.  The default bf16x6 model keeps its selection (the fp32 kernels below 6 chunks).  `-m gpu`."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth
from iefvad_amd import lib as L
from oracle import iefvad_oracle as orc
from tests import helpers as H
from tests import test_gpu_similarity_rows as VS
from tests import test_gpu_videos_full as VF      # the edge-length videos, the host chunker and the padded reference of the valid-row suite

pytestmark = pytest.mark.gpu

SCORE_KEYS = ("logits", "w_i_mean", "w_e_mean")
B_BIG = 48
# (B, first chunk) of the small forwards: slices of the B = 48 batch that do not start at its origin
SMALL = ((1, 5), (2, 0), (3, 9), (5, 17), (6, 30), (9, 39))


def make_model(sd, compute="bf16x6", L_=2, K=10, nu=8, **kw):
    args = argparse.Namespace(visual_layers=L_, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=nu)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, L_, 8, 10, 10, "cuda", args, compute=compute, **kw)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


def run(model, img, ev):
    """The model's dict on the device (clones: a replayed hipGraph writes where the last call wrote)."""
    with torch.no_grad():
        out = model(img if torch.is_tensor(img) else torch.from_numpy(img).cuda(), ev if torch.is_tensor(ev) else torch.from_numpy(ev).cuda(),
                    None, None, None)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


@pytest.fixture(scope="module")
def batch48():
    sd = synth.make_state_dict(0)
    img, ev = synth.make_inputs(7, B_BIG)
    return sd, torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()


@pytest.mark.parametrize("outputs", ["full", "scores"])
def test_small_forwards_equal_the_slices_of_a_big_forward(batch48, outputs):
    """B = 1, 2, 3, 5 (the fp32 kernels' sizes in the default mode), 6, 9 (partially filled split grids) against B = 48: every key, bit
    for bit.  B <= 8 replays a hipGraph, B = 9 and 48 launch directly.  outputs="scores": the folded scorer takes one branch at every
    size (fold = K >= 1), which the logits' bits need."""
    sd, img, ev = batch48
    model = make_model(sd, outputs=outputs, batch_invariant=True)
    assert model.batch_invariant is True
    keys = iefvad_amd.OUTPUT_KEYS if outputs == "full" else SCORE_KEYS
    big = run(model, img, ev)
    assert set(big) == set(keys)
    lib = L.load_library()
    for B, c0 in SMALL:
        n0 = lib.iefvad_gemm_split_small_launches()
        got = run(model, img[c0:c0 + B].contiguous(), ev[c0:c0 + B].contiguous())
        if B < 6:
            assert lib.iefvad_gemm_split_small_launches() > n0, B      # (a graph counts at capture: first call at this size)
        for k in keys:
            assert bool(torch.isfinite(got[k]).all()), (B, k)
            assert torch.equal(got[k], big[k][c0:c0 + B]), (outputs, B, k, float((got[k] - big[k][c0:c0 + B]).abs().max()))


def test_the_default_model_keeps_its_selection(batch48):
    """B = 3: a default bf16x6 model runs the fp32 kernels (the bits of compute="f32") and launches no small tiling; the invariant model
    runs another arithmetic, on the small tiling."""
    sd, img, ev = batch48
    a, b = img[:3].contiguous(), ev[:3].contiguous()
    lib = L.load_library()
    f32 = run(make_model(sd, "f32"), a, b)
    n0 = lib.iefvad_gemm_split_small_launches()
    dflt_model = make_model(sd)
    assert dflt_model.batch_invariant is False
    dflt = run(dflt_model, a, b)
    assert lib.iefvad_gemm_split_small_launches() == n0
    inv = run(make_model(sd, batch_invariant=True), a, b)
    # 768 rows: the 2 K refinement projections (N = 768, one problem: 36 workgroups of 128 x 128) and the L out_proj launches (two
    # problems: 72) are within the small tiling's 128; in_proj (216) and the heads (144) stay on the 128 x 128 tiling
    assert lib.iefvad_gemm_split_small_launches() - n0 == 22
    for k in iefvad_amd.OUTPUT_KEYS:
        assert torch.equal(dflt[k], f32[k]), k
    assert not torch.equal(inv["logits"], f32["logits"])
    assert not torch.equal(inv["fused"], f32["fused"])


def _accuracy(sd, img, ev, cfg, **model_kw):
    """The gates of test_gpu_bf16x6.py on the invariant model: the fp32 gates against the CPU oracle, and against the fp64 oracle an
    error of at most 1.25 x the f32 mode's + 2e-7."""
    ti, te = torch.from_numpy(img).float(), torch.from_numpy(ev).float()
    ref32 = orc.forward(sd, ti, te, cfg)
    ref64 = orc.forward(sd, ti, te, cfg, dtype=torch.float64)
    got = {k: v.cpu().numpy() for k, v in run(make_model(sd, batch_invariant=True, **model_kw), img, ev).items()}
    f32 = {k: v.cpu().numpy() for k, v in run(make_model(sd, "f32", **model_kw), img, ev).items()}
    tol_big, tol_logit, tol_sig = H.TOL_BIG, H.TOL_LOGIT, H.TOL_SIGMOID
    for k in H.BIG_KEYS + ["logits"]:
        e32 = np.abs(got[k] - ref32[k].numpy()).max()
        e_inv, e_f32 = np.abs(got[k] - ref64[k].numpy()).max(), np.abs(f32[k] - ref64[k].numpy()).max()
        print(f"B={img.shape[0]} {k}: |inv - oracle32| {e32:.3e}  |inv - oracle64| {e_inv:.3e}  |f32 - oracle64| {e_f32:.3e}")
        assert e32 <= (tol_logit if k == "logits" else tol_big), (k, e32)
        assert e_inv <= 1.25 * e_f32 + 2e-7, (k, e_inv, e_f32)
    e = np.abs(H.sigmoid(got["logits"]) - H.sigmoid(ref32["logits"].numpy())).max()
    assert e <= tol_sig, e
    assert not np.array_equal(got["logits"], f32["logits"])          # the split arithmetic really ran


@pytest.mark.parametrize("B", [1, 3])
def test_accuracy_at_the_sizes_the_default_mode_leaves_to_the_fp32_kernels(B):
    sd = synth.make_state_dict(4)
    img, ev = synth.make_inputs(21, B)
    _accuracy(sd, img, ev, orc.OracleConfig(num_layers=2, num_refinement_steps=10, nu=8))


def test_accuracy_in_the_sharpened_regime():
    """synth.sharpen_qk weights (a dominant key per query) on the fixture's own batch (B = 3): the same gates, and the fixture's numbers
    themselves on the rows it holds (helpers.compare_outputs)."""
    g, cfg, sd, img, ev = H.load_case("sharp_k3_student8")
    assert cfg["B"] < 6                                            # a size the default mode leaves to the fp32 kernels
    kw = dict(L_=cfg["L"], K=cfg["K"], nu=cfg["nu"])
    _accuracy(sd, img, ev, H.oracle_cfg(cfg), **kw)
    out = run(make_model(sd, batch_invariant=True, **kw), img, ev)
    H.compare_outputs({k: v.cpu().numpy() for k, v in out.items()}, g)


# ------------------------------------------------------------------ the valid-row routes
def _padded_reference(dtype, micro_batch=0):
    model = VF.make_model("bf16x6", outputs="full", micro_batch=micro_batch, batch_invariant=True)
    img, ev, index = VF.pad(VF.videos(dtype))
    ref = VF.padded_full(model, img, ev, index)
    with torch.no_grad():
        out = model(img, ev, None, None, None)
        ref["similarity"] = harness.similarity_rows(out["fused"], out["image_mu"], out["event_mu"], index).clone()
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    return ref


@pytest.fixture(scope="module")
def padded():
    """The host-padded dense forward of the invariant model on the edge-length videos (16 chunks in one pass), computed once."""
    return {np.float32: _padded_reference(np.float32), np.float16: _padded_reference(np.float16)}


@pytest.mark.parametrize("dtype,micro_batch,dense", [(np.float32, 0, False), (np.float32, 3, False), (np.float16, 0, False),
                                                      (np.float32, 0, True), (np.float32, 3, True)])
def test_valid_row_route_equals_the_padded_dense_forward(padded, monkeypatch, dtype, micro_batch, dense):
    """Lengths [37, 255, 256, 257, 512, 1500, 1, 300]: `forward_videos` against the host-padded forward, all seven tensors and the
    three vectors (outputs="full") and the four series (similarity=True).  micro_batch = 3: passes of 768 rows and fewer run on the
    small tiling while the reference's one pass of 16 chunks ran on the 128 x 128 one.  IEFVAD_DENSE_ENCODER=1: the tail runs on the
    compacted row set, whose smaller row count selects the fp32 tilings in the default mode."""
    if dense:
        monkeypatch.setenv("IEFVAD_DENSE_ENCODER", "1")            # read when the handle is created
    model = VF.make_model("bf16x6", outputs="scores", micro_batch=micro_batch, batch_invariant=True)
    want = padded[dtype]
    got = VF.rows_call(model, dtype, outputs="full")
    VF.assert_all_equal(got, want, ("invariant", dtype.__name__, micro_batch, dense))
    sim = VF.rows_call(model, dtype, similarity=True)
    assert set(sim) == set(SCORE_KEYS) | {"similarity"}
    VS.assert_series_equal(sim["similarity"], want["similarity"], ("invariant", dtype.__name__, micro_batch, dense))
    for k in SCORE_KEYS:
        assert torch.equal(sim[k], want[k]), k


def test_padded_route_does_not_depend_on_the_pass_size(padded):
    """The padded forward itself at micro_batch = 3 (five passes of three chunks and one of one) against one pass of 16."""
    ref = _padded_reference(np.float32, micro_batch=3)
    for k, v in padded[np.float32].items():
        assert torch.equal(ref[k], v), k


@pytest.mark.parametrize("batch_chunks", [4, 128])
def test_host_list_route_equals_the_padded_dense_forward(padded, batch_chunks):
    model = VF.make_model("bf16x6", outputs="scores", batch_invariant=True)
    got = VF.host_call(model, VF.videos(np.float32), batch_chunks=batch_chunks, outputs="full")
    VF.assert_all_equal(got, padded[np.float32], ("host list", batch_chunks))
    sim = VF.host_call(model, VF.videos(np.float32), batch_chunks=batch_chunks, similarity=True)
    VS.assert_series_equal(sim["similarity"], padded[np.float32]["similarity"], ("host list", batch_chunks))


# ------------------------------------------------------------------ hipGraphs and the C entry
@pytest.mark.parametrize("B", [1, 2])
def test_graph_replay_equals_direct_launches(batch48, B):
    sd, img, ev = batch48
    a, b = img[7:7 + B].contiguous(), ev[7:7 + B].contiguous()
    direct = run(make_model(sd, batch_invariant=True, graph_chunks=-1), a, b)
    graphed = make_model(sd, batch_invariant=True)
    first, again = run(graphed, a, b), run(graphed, a, b)             # capture, then replay
    for k in iefvad_amd.OUTPUT_KEYS:
        assert torch.equal(first[k], direct[k]) and torch.equal(again[k], direct[k]), (B, k)


def test_toggling_the_mode_after_a_captured_call_changes_the_bits(batch48):
    """iefvad_set_batch_invariant releases the handle's cached graphs: the next B = 2 call captures the other mode's launches."""
    sd, img, ev = batch48
    a, b = img[:2].contiguous(), ev[:2].contiguous()
    lib = L.load_library()
    inv = run(make_model(sd, batch_invariant=True), a, b)
    model = make_model(sd)
    dflt = run(model, a, b)
    run(model, a, b)                                                  # replayed once
    assert not torch.equal(dflt["logits"], inv["logits"])
    assert lib.iefvad_set_batch_invariant(model._handle, 1) == 0, L.last_error()
    on = run(model, a, b)
    assert lib.iefvad_set_batch_invariant(model._handle, 1) == 0      # already on: nothing to do
    assert lib.iefvad_set_batch_invariant(model._handle, 0) == 0, L.last_error()
    off = run(model, a, b)
    for k in iefvad_amd.OUTPUT_KEYS:
        assert torch.equal(on[k], inv[k]), k
        assert torch.equal(off[k], dflt[k]), k


def test_refusals_and_the_modes_that_are_invariant_already(batch48):
    sd, img, ev = batch48
    a, b = img[:1].contiguous(), ev[:1].contiguous()
    with pytest.raises(ValueError, match="fp16x3"):
        make_model(sd, "fp16x3", batch_invariant=True)
    lib = L.load_library()
    h16 = make_model(sd, "fp16x3")
    run(h16, a, b)
    assert lib.iefvad_set_batch_invariant(h16._handle, 1) != 0
    assert "iefvad_set_batch_invariant" in L.last_error() and "FP16X3" in L.last_error()
    assert lib.iefvad_set_batch_invariant(None, 1) != 0
    for compute in ("f32", "bf16"):
        plain = run(make_model(sd, compute), a, b)
        n0 = lib.iefvad_gemm_split_small_launches()
        inert = run(make_model(sd, compute, batch_invariant=True), a, b)
        assert lib.iefvad_gemm_split_small_launches() == n0
        for k in iefvad_amd.OUTPUT_KEYS:
            assert torch.equal(plain[k], inert[k]), (compute, k)


# ------------------------------------------------------------------ the harness
def _items(seed, lengths, classes):
    for i, (n, c) in enumerate(zip(lengths, classes)):
        img, ev = synth.make_video(seed, i, int(n))
        ci, _ = harness.process_split(img, 256)
        ce, _ = harness.process_split(ev, 256)
        yield torch.tensor(ci).unsqueeze(0), torch.tensor(ce).unsqueeze(0), (c,), torch.tensor([int(n)])


def test_per_video_packed_and_host_list_scores_are_bit_identical():
    """A 12-video list (one to seven chunks a video): one forward per video, packed forward_videos calls and the walk inside the
    library give the same scores and weight means."""
    seed = 4
    lengths = [300, 37, 256, 1, 700, 255, 1500, 257, 512, 90, 1030, 64]
    classes = [synth.UCF_CLASSES[i % len(synth.UCF_CLASSES)] for i in range(len(lengths))]
    model = make_model(synth.make_state_dict(0), outputs="scores", batch_invariant=True)
    per_video = harness.score_loader(model, _items(seed, lengths, classes), 256, "cuda:0", "ucfcrime", batch_chunks=0)
    packed = harness.score_loader(model, _items(seed, lengths, classes), 256, "cuda:0", "ucfcrime", batch_chunks=64, host_list=False)
    host = harness.score_loader(model, _items(seed, lengths, classes), 256, "cuda:0", "ucfcrime", batch_chunks=64, host_list=True)
    assert per_video[1] == packed[1] == host[1] == classes
    for other, tag in ((packed, "packed"), (host, "host list")):
        for j in (0, 2, 3):                                           # scores, w_i_mean, w_e_mean: one array per video
            assert len(other[j]) == len(lengths)
            for v, (x, y) in enumerate(zip(per_video[j], other[j])):
                assert x.shape == (lengths[v],) and np.array_equal(x, y), (tag, j, v, float(np.abs(x - y).max()))


@pytest.fixture(scope="module")
def config1(tmp_path_factory, golden_dir):
    return H.write_config1_set(tmp_path_factory.mktemp("cfg1inv"), golden_dir)


def test_harness_test_takes_the_packed_route_for_the_invariant_model(config1, monkeypatch, capsys):
    g, args, gt, sd = config1
    seen = []
    real = harness.score_loader

    def spy(model, loader, maxlen, device, dataset, label_map, batch_chunks, *a, **kw):
        seen.append(batch_chunks)
        return real(model, loader, maxlen, device, dataset, label_map, batch_chunks, *a, **kw)

    monkeypatch.setattr(harness, "score_loader", spy)
    scores = {}
    for inv in (True, False):
        model = make_model(sd, outputs="scores", batch_invariant=inv)
        harness.test(args, model, harness.get_test_loader(args), 256, None, gt, "cuda:0")
        scores[inv] = np.concatenate(harness.test.last_result["scores"])
    assert seen == [64, 0], seen
    assert np.abs(scores[True] - g["scores"]).max() <= H.TOL_SIGMOID
    assert np.abs(scores[True] - scores[False]).max() <= H.TOL_SIGMOID
    capsys.readouterr()


# ------------------------------------------------------------------ non-finite inputs
@pytest.mark.parametrize("B,invariant", [(2, True), (6, False)])
def test_non_finite_rows_in_one_chunk_match_the_oracle_pattern(B, invariant):
    """The bf16x6 twin of test_gpu_fp16x3.py::test_non_finite_inputs_at_split_batch_size_match_the_oracle_pattern, at B = 2 in the
    invariant mode (the small tiling) and at B = 6 in the default mode (the 128 x 128 tiling): one +inf, one -inf and one NaN row in
    the image features of ONE chunk.  The reference lets them propagate (test.py:90-95 replaces only NaN, and the forward is called
    here without that rule), attention spreads them over their chunk, the fusion over both weights.  Per output and chunk the
    finite / non-finite pattern must equal the oracle's (computed here), no infinity may come out, finite values stay within the fp32
    gates and no other chunk is touched.  The operand rule of csrc/gemm_split.h (inf - inf in the split's remainder turns an inf
    operand into NaN where the fp32 path would carry the inf one projection further) does not show at this granularity: the first
    attention turns an inf row's chunk into NaN in the oracle as well."""
    sd = synth.make_state_dict(81, 768, 2, 2)
    img, ev = synth.make_inputs(31, B)
    bad = B - 1
    img[bad, 10, :] = np.inf
    img[bad, 77, :] = -np.inf
    img[bad, 200, :] = np.nan
    ref = orc.forward(sd, torch.from_numpy(img), torch.from_numpy(ev), orc.OracleConfig(num_layers=2, num_refinement_steps=2, nu=8))
    lib = L.load_library()
    n0 = lib.iefvad_gemm_split_small_launches()
    got = {k: v.cpu().numpy() for k, v in run(make_model(sd, K=2, batch_invariant=invariant), img, ev).items()}
    assert (lib.iefvad_gemm_split_small_launches() > n0) == invariant
    for k in H.BIG_KEYS + ["logits"]:
        r = ref[k].numpy()
        bad_got = (~np.isfinite(got[k])).reshape(B, -1).any(1)
        bad_ref = (~np.isfinite(r)).reshape(B, -1).any(1)
        assert np.array_equal(bad_got, bad_ref), (k, bad_got, bad_ref)
        assert not bad_ref[:bad].any(), k                             # only the poisoned chunk
        assert not np.isinf(got[k]).any() and not np.isinf(r).any(), k
        fin = np.isfinite(r) & np.isfinite(got[k])
        assert np.abs(got[k][fin] - r[fin]).max() <= (H.TOL_LOGIT if k == "logits" else H.TOL_BIG), k
    assert (~np.isfinite(got["logits"])).reshape(B, -1).any(1).tolist() == [False] * bad + [True]
