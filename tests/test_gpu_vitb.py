"""D = 512 on the GPU (ViT-B/16 features, the reference's `--ds vitb_rgb`: 8 heads of 64, `iefvad_create_ex`, f32 arithmetic): the
reference captures of tests/golden/make_golden_vitb.py through every evaluation entry -- the dense forward at the D = 768 f32 gates,
batch sizes that pick every fp32 GEMM tiling at N = 512 / 1536, K = 512 and the head-dim-64 attention kernels, the hipGraph replay,
whole videos (device chunker, list walk) and the reference's test() loop -- and the refusals of what D = 512 does not build."""
import argparse

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, losses, synth
from iefvad_amd import lib as _lib
from oracle import iefvad_oracle as orc
from tests import helpers as H
from tests import vitb_cases as V

pytestmark = pytest.mark.gpu

D = V.D


def make_model(sd, cfg, **kw):
    m = iefvad_amd.MMFMIL(14, D, 256, D, 8, cfg["L"], 8, 10, 10, "cuda", V.model_args(cfg), **kw)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


def run(model, img, ev):
    with torch.no_grad():
        out = model(torch.as_tensor(img).cuda(), torch.as_tensor(ev).cuda(), None, None, None)
    torch.cuda.synchronize()
    return out


BASE = dict(L=2, K=3, lam=0.5, noise="StudentT", nu=8)


def base_model(**kw):
    return make_model(synth.make_state_dict(51, D, 2, 3), BASE, **kw)


@pytest.mark.parametrize("name", V.FWD_CASES)
def test_forward_matches_the_reference_at_d512(name):
    g, cfg, sd, img, ev = V.load_case(name)
    out = run(make_model(sd, cfg), img, ev)
    for k in H.BIG_KEYS:
        assert tuple(out[k].shape) == (cfg["B"], 256, D)
    errs = H.compare_outputs({k: v.cpu().numpy() for k, v in out.items()}, g)
    assert np.abs(out["w_i"].mean(-1).cpu().numpy() - g["w_i_mean"]).max() < 2e-6
    print(name, errs)


def test_scores_and_weights_outputs_equal_the_full_dict():
    g, cfg, sd, img, ev = V.load_case("base")
    full = run(make_model(sd, cfg), img, ev)
    scores = run(make_model(sd, cfg, outputs="scores"), img, ev)
    weights = run(make_model(sd, cfg, outputs="weights"), img, ev)
    for o in (scores, weights):
        assert torch.equal(o["logits"], full["logits"])
        assert torch.equal(o["w_i_mean"], scores["w_i_mean"]) and torch.equal(o["w_e_mean"], scores["w_e_mean"])
    assert torch.equal(weights["w_i"], full["w_i"]) and torch.equal(weights["w_e"], full["w_e"])
    # the library's row means against the full tensors' means (the reduction order differs: not bit-pinned)
    assert float((scores["w_i_mean"].reshape(-1) - full["w_i"].mean(-1).reshape(-1)).abs().max()) < 2e-6


def test_small_batches_equal_rows_of_larger_batches_bit_for_bit():
    """B = 1, 2, 3, 5 (the 32 x 32 tiny GEMM), B = 40 (128 x 128 and 64 x 64) and B = 512 (the 128 x 256 ring) take different fp32
    tilings at N = 512 / 1536 and K = 512; all of them keep one k order, so every output row has the same bits.  B = 512 is
    also checked against the CPU oracle on a few chunks."""
    model = base_model()
    img, ev = synth.make_inputs(61, 40, D=D)
    big = run(model, img, ev)
    for B, c0 in ((1, 0), (2, 7), (3, 20), (5, 35)):
        small = run(model, img[c0:c0 + B], ev[c0:c0 + B])
        for k in iefvad_amd.OUTPUT_KEYS:
            assert torch.equal(small[k], big[k][c0:c0 + B]), (B, k)
    del big
    torch.cuda.empty_cache()
    model = base_model(outputs="weights")
    img, ev = synth.make_inputs(62, 512, D=D)
    huge = run(model, img, ev)
    one = run(model, img[300:301], ev[300:301])
    for k in one:
        assert torch.equal(one[k], huge[k][300:301]), k
    sd = synth.make_state_dict(51, D, 2, 3)
    ref = orc.forward(sd, torch.from_numpy(img[[0, 511]]), torch.from_numpy(ev[[0, 511]]),
                      orc.OracleConfig(num_layers=2, num_refinement_steps=3, nu=8))
    assert float((huge["logits"][[0, 511]].cpu() - ref["logits"]).abs().max()) <= H.TOL_LOGIT
    assert float((huge["w_i"][[0, 511]].cpu() - ref["w_i"]).abs().max()) <= H.TOL_BIG


def test_graph_replay_equals_direct_launches():
    img, ev = synth.make_inputs(63, 2, D=D)
    graphed = base_model()                                   # graph_chunks = 0: B <= 8 replays a captured graph
    direct = base_model(graph_chunks=-1)
    for B in (1, 2):
        for _ in range(2):                                   # capture, then replay
            a = run(graphed, img[:B], ev[:B])
        b = run(direct, img[:B], ev[:B])
        for k in iefvad_amd.OUTPUT_KEYS:
            assert torch.equal(a[k], b[k]), (B, k)


EDGE_LENGTHS = [37, 255, 256, 257, 512, 1500, 1, 300]


def videos(lengths, seed=6, dtype=np.float32):
    return [synth.make_video(seed, i, int(n), D=D, dtype=dtype) for i, n in enumerate(lengths)]


def dense_reference(model, vids):
    ci = [harness.process_split(v[0], 256)[0].reshape(-1, 256, D) for v in vids]
    ce = [harness.process_split(v[1], 256)[0].reshape(-1, 256, D) for v in vids]
    out = run(model, np.concatenate(ci), np.concatenate(ce))
    lg, wi, we = out["logits"].reshape(-1), out["w_i_mean"].reshape(-1), out["w_e_mean"].reshape(-1)
    res, off = {"logits": [], "w_i_mean": [], "w_e_mean": []}, 0
    for v, c in zip(vids, ci):
        n = v[0].shape[0]
        for k, t in (("logits", lg), ("w_i_mean", wi), ("w_e_mean", we)):
            res[k].append(t[off:off + n])
        off += c.shape[0] * 256
    return {k: torch.cat(v) for k, v in res.items()}


def ragged(model, vids, **kw):
    img = torch.from_numpy(np.concatenate([v[0] for v in vids])).cuda()
    ev = torch.from_numpy(np.concatenate([v[1] for v in vids])).cuda()
    with torch.no_grad():
        return model.forward_videos(img, ev, [v[0].shape[0] for v in vids], **kw)


@pytest.mark.parametrize("micro_batch", [0, 3])
def test_forward_videos_equals_the_padded_forward(micro_batch):
    model = base_model(outputs="scores", micro_batch=micro_batch)
    vids = videos(EDGE_LENGTHS)
    want = dense_reference(model, vids)
    got = ragged(model, vids)
    for k in want:
        assert got[k].shape == want[k].shape == (sum(EDGE_LENGTHS),)
        assert torch.equal(got[k], want[k]), (k, (got[k] - want[k]).abs().max().item())


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_forward_videos_nan_rule_matches_the_host_rule(dtype):
    """The rule of test.py:90-95 at D = 512, as tests/test_gpu_videos.py pins it at 768: NaN -> 0 and then +-inf -> the dtype's
    max / min, per video and modality; inf without NaN is left alone and poisons its chunk."""
    lengths = [100, 300, 50, 80, 600, 256]
    vids = videos(lengths, seed=9, dtype=dtype)
    vids[1][0][7, 5] = np.nan
    vids[1][0][290, 100] = np.inf
    vids[3][0][10, 10] = np.inf
    vids[4][1][400, 511] = np.nan
    model = base_model(outputs="scores")

    def items():
        for img, ev in vids:
            ci, n = harness.process_split(img, 256)
            ce, _ = harness.process_split(ev, 256)
            yield torch.tensor(ci).unsqueeze(0), torch.tensor(ce).unsqueeze(0), ("Normal",), torch.tensor([n])

    host, _, _, _ = harness.score_loader(model, items(), 256, "cuda:0", "ucfcrime", batch_chunks=4, ragged=False)
    dev, _, _, _ = harness.score_loader(model, items(), 256, "cuda:0", "ucfcrime", batch_chunks=4, ragged=True)
    for i, (a, b) in enumerate(zip(host, dev)):
        assert np.array_equal(np.nan_to_num(a, nan=-1.0), np.nan_to_num(b, nan=-1.0)), i
    assert np.isfinite(dev[4]).all()
    assert np.isnan(dev[3]).all()
    assert all(np.isfinite(dev[i]).all() for i in (0, 2, 5))


def test_host_list_entry_equals_forward_videos():
    lengths = EDGE_LENGTHS + [90, 33]
    model = base_model(outputs="scores")
    for dtype in (np.float32, np.float16):
        vids = videos(lengths, seed=23, dtype=dtype)
        padded_i = [torch.from_numpy(harness.process_split(v[0], 256)[0]) for v in vids]
        padded_e = [torch.from_numpy(harness.process_split(v[1], 256)[0]) for v in vids]
        for bc in (4, 128):
            got = model.forward_videos_host(padded_i, padded_e, lengths, batch_chunks=bc)
            want = ragged(model, vids)
            for k in want:
                assert got[k].shape == (sum(lengths),)
                assert torch.equal(got[k], want[k]), (dtype, bc, k)
        if dtype == np.float16:      # fp16 features widen to fp32 on the device: within the fp32 gates of the fp32 features' scores
            f32 = ragged(model, [(a.astype(np.float32), b.astype(np.float32)) for a, b in vids])
            assert torch.equal(got["logits"], f32["logits"])
    # bf16 feature files: the list walk and the device chunker read the same bf16 rows
    bi = [t.to(torch.bfloat16) for t in padded_i]
    be = [t.to(torch.bfloat16) for t in padded_e]
    got = model.forward_videos_host(bi, be, lengths, batch_chunks=8)
    rows_i = torch.cat([t.reshape(-1, D)[:n] for t, n in zip(bi, lengths)]).cuda()
    rows_e = torch.cat([t.reshape(-1, D)[:n] for t, n in zip(be, lengths)]).cuda()
    with torch.no_grad():
        want = model.forward_videos(rows_i, rows_e, lengths)
    for k in want:
        assert torch.equal(got[k], want[k]), ("bf16", k)
    # the narrowed (bf16) wire belongs to the bf16 arithmetic, which D = 512 does not build
    with pytest.raises(RuntimeError, match="wire"):
        model.forward_videos_host(padded_i, padded_e, lengths, wire_dtype=torch.bfloat16)


def test_reference_test_loop_through_the_hip_path(tmp_path, capsys):
    g, args, gt, sd = V.write_harness_set(tmp_path)
    model = make_model(sd, dict(L=2, K=10, lam=0.5, noise="StudentT", nu=8))
    roc, ap = harness.test(args, model, harness.get_test_loader(args), 256, None, gt, "cuda:0")
    res = harness.test.last_result
    scores = np.concatenate(res["scores"])
    assert scores.shape == g["scores"].shape
    assert np.abs(scores - g["scores"]).max() <= H.TOL_SIGMOID
    assert abs(roc - float(g["roc"])) < 1e-4 and abs(ap - float(g["ap"])) < 1e-4
    assert abs(res["ano_auc"] - float(g["ano_auc"])) < 1e-4
    out = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    ref_lines = [ln for ln in str(g["stdout"]).splitlines() if ln.strip()]
    assert out[0] == ref_lines[0] and out[1] == ref_lines[1]


def test_what_d512_does_not_build_is_refused_before_any_launch():
    sd = synth.make_state_dict(51, D, 2, 3)
    img, ev = synth.make_inputs(64, 1, D=D)
    x, y = torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()
    for compute in ("bf16", "bf16x6", "fp16x3"):
        m = make_model(sd, BASE, compute=compute)
        with pytest.raises(RuntimeError, match="D=512.*f32"):
            m(x, y, None, None, None)
    m = make_model(sd, BASE).train()
    with pytest.raises(RuntimeError, match="D=768"):
        m(x, y, None, None, None)
    outs = {k: torch.zeros(2, 256, D, device="cuda") for k in ("image_mu", "event_mu", "image_logvar", "event_logvar")}
    outs["logits"] = torch.zeros(2, 256, 1, device="cuda")
    with pytest.raises(ValueError, match="768"):
        losses.training_loss(outs, torch.zeros(2, 14), [256, 256])
    # the C entries with no D = 512 path name the width too
    m = make_model(sd, BASE)
    run(m, img, ev)
    lib = _lib.load_library()
    assert lib.iefvad_train_workspace_bytes(m._handle, 1) == 0 and "D=768" in _lib.last_error()


def test_create_ex_at_d768_is_create(monkeypatch):
    g, cfg, sd, img, ev = H.load_case("base_k10_student8")
    args = argparse.Namespace(visual_layers=cfg["L"], visual_head=8, num_refinement_steps=cfg["K"], lambda_ref=cfg["lam"],
                              noise_model=cfg["noise"], nu=cfg["nu"])

    def m768():
        m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, cfg["L"], 8, 10, 10, "cuda", args)
        m.load_state_dict(sd)
        return m.to("cuda:0").eval()

    a = run(m768(), img, ev)
    lib = _lib.load_library()
    monkeypatch.setattr(lib, "iefvad_create", lib.iefvad_create_ex)
    b = run(m768(), img, ev)
    for k in iefvad_amd.OUTPUT_KEYS:
        assert torch.equal(a[k], b[k]), k
    H.compare_outputs({k: v.cpu().numpy() for k, v in b.items()}, g)
