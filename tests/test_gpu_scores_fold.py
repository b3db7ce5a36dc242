"""The folded scorer of the bf16x6 inference forward (csrc/iefvad.hip forward_pass, step 4): with v = -lambda W2^T c and
s0 = b_c - lambda (c . b2) of the LAST refinement block formed at iefvad_set_weights,

    logits = c . z_K + b_c = c . z_{K-1} + v . h + s0,      h = relu(W1 z_{K-1} + b1),

so a forward that does not return `fused` stores no h and launches no last W2 projection; one that does still forms z_K as before, and
both take their logits from the folded form.  Gates: tests/helpers.py (the fp32 gates every mode is held to) and the relation
tests/test_gpu_bf16x6.py uses against the fp64 oracle.  Measured on an MI355X (the tests print their figures, `pytest -s`): |logits - fp32
oracle| 6.0e-7 .. 8.3e-7, sigmoid 1.5e-7 .. 1.8e-7, |logits - fp64 oracle| 4.9e-7 .. 5.6e-7 against the f32 mode's 5.5e-7 .. 6.5e-7,
|folded - unfolded logits| <= 3.0e-7, `fused` bit-equal to the unfolded forward's.  Needs a real MI355X: run with `-m gpu`."""
import argparse

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import synth
from oracle import iefvad_oracle as orc
from tests import helpers as H

pytestmark = pytest.mark.gpu

B_SPLIT = 48     # chunks: every projection of the micro-batch runs on the split kernel (from 6 chunks on)
L = 2


def make_model(sd, compute, K, lam=0.5, **kw):
    args = argparse.Namespace(visual_layers=L, visual_head=8, num_refinement_steps=K, lambda_ref=lam, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, L, 8, 10, 10, "cuda", args, compute=compute, **kw)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


def run(model, img, ev, timed=False):
    with torch.no_grad():
        out = model(torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda(), None, None, None, timed=timed)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def with_idle_last_step(sd, K):
    """The K-step weights plus a step K+1 whose second projection is all zero: z_{K+1} = z_K - lambda (0 h + 0) = z_K exactly, and the
    folded scorer of that model has v = 0, s0 = b_c, i.e. it is the plain c . z_K + b_c.  Its steps 1..K run on the unfolded launches
    (EPI_BIAS_RELU, EPI_REFINE), so its `fused` and `logits` are what the forward without the fold computes for the K-step model."""
    ext = dict(sd)
    rng = np.random.default_rng(77)
    ext[f"temporal.refinement_blocks.{K}.0.weight"] = torch.from_numpy((rng.uniform(-1, 1, (768, 768)) / np.sqrt(768)).astype(np.float32))
    ext[f"temporal.refinement_blocks.{K}.0.bias"] = torch.from_numpy((0.1 * rng.standard_normal(768)).astype(np.float32))
    ext[f"temporal.refinement_blocks.{K}.2.weight"] = torch.zeros(768, 768)
    ext[f"temporal.refinement_blocks.{K}.2.bias"] = torch.zeros(768)
    return ext


@pytest.mark.parametrize("K,lam,wseed", [(1, 0.5, 0), (2, 0.5, 3), (10, 0.5, 9), (2, 0.3, 3)])
def test_folded_logits_and_fused(K, lam, wseed):
    sd = synth.make_state_dict(wseed, 768, L, K)
    img, ev = synth.make_inputs(13 + K, B_SPLIT)
    cfg = orc.OracleConfig(num_layers=L, num_refinement_steps=K, lambda_ref=lam, nu=8)
    ti, te = torch.from_numpy(img), torch.from_numpy(ev)
    ref32 = orc.forward(sd, ti, te, cfg)
    ref64 = orc.forward(sd, ti, te, cfg, dtype=torch.float64)

    m_full = make_model(sd, "bf16x6", K, lam)
    m_sc = make_model(sd, "bf16x6", K, lam, outputs="scores")
    full = run(m_full, img, ev, timed=True)
    sc = run(m_sc, img, ev, timed=True)
    f32 = run(make_model(sd, "f32", K, lam), img, ev)
    n_full, n_sc = m_full.last_stage_times["gemm_launches"], m_sc.last_stage_times["gemm_launches"]
    print(f"K={K} lambda={lam}: gemm launches full {n_full}, scores {n_sc}")

    r32, r64 = ref32["logits"].numpy(), ref64["logits"].numpy()
    e_log, e_sig = np.abs(full["logits"] - r32).max(), np.abs(H.sigmoid(full["logits"]) - H.sigmoid(r32)).max()
    e64, e64_f32 = np.abs(full["logits"] - r64).max(), np.abs(f32["logits"] - r64).max()
    e_fused = np.abs(full["fused"] - ref32["fused"].numpy()).max()
    print(f"  |logits - fp32 oracle| {e_log:.3e}  sigmoid {e_sig:.3e}  |logits - fp64 oracle| {e64:.3e} (f32 mode {e64_f32:.3e})  "
          f"|fused - fp32 oracle| {e_fused:.3e}")

    # one launch fewer per internal pass (B_SPLIT chunks are one pass): the last W2 projection is gone, not renamed
    assert n_full == 2 * L + 1 + 2 * K, n_full          # in_proj and out_proj per layer, the heads, two projections per step
    assert n_sc == n_full - 1, (n_sc, n_full)
    # the two output sets take their logits from the same arithmetic
    assert np.array_equal(sc["logits"], full["logits"])
    assert not np.array_equal(full["logits"], f32["logits"])          # the split kernels really ran
    for got in (full, sc):
        assert np.abs(got["logits"] - r32).max() <= H.TOL_LOGIT
        assert np.abs(H.sigmoid(got["logits"]) - H.sigmoid(r32)).max() <= H.TOL_SIGMOID
        assert np.abs(got["logits"] - r64).max() <= 1.25 * e64_f32 + 2e-7, (e64, e64_f32)
    assert e_fused <= H.TOL_BIG

    # `fused` in full mode: the bits of the unfolded forward; its logits: the folded ones differ from it at rounding level only
    plain = run(make_model(with_idle_last_step(sd, K), "bf16x6", K + 1, lam), img, ev)
    d_plain = np.abs(full["logits"] - plain["logits"]).max()
    print(f"  |folded logits - unfolded logits| {d_plain:.3e}")
    assert np.array_equal(full["fused"], plain["fused"])
    assert np.abs(plain["logits"] - r32).max() <= H.TOL_LOGIT          # the comparison model is the K-step model
    assert d_plain <= H.TOL_LOGIT


def test_no_refinement_steps_and_small_batches_are_unchanged():
    """K = 0 has no block to fold: the plain scorer runs, in both output sets.  A 3-chunk batch stays below the split threshold and
    runs on the fp32 kernels, bit-identical to compute="f32", whatever the outputs."""
    sd0 = synth.make_state_dict(5, 768, L, 0)
    img, ev = synth.make_inputs(31, B_SPLIT)
    m_full, m_sc = make_model(sd0, "bf16x6", 0), make_model(sd0, "bf16x6", 0, outputs="scores")
    full, sc = run(m_full, img, ev, timed=True), run(m_sc, img, ev, timed=True)
    assert m_full.last_stage_times["gemm_launches"] == m_sc.last_stage_times["gemm_launches"]
    assert np.array_equal(full["logits"], sc["logits"])
    ref = orc.forward(sd0, torch.from_numpy(img), torch.from_numpy(ev), orc.OracleConfig(num_layers=L, num_refinement_steps=0, nu=8))
    assert np.abs(full["logits"] - ref["logits"].numpy()).max() <= H.TOL_LOGIT
    assert np.abs(H.sigmoid(full["logits"]) - H.sigmoid(ref["logits"].numpy())).max() <= H.TOL_SIGMOID
    assert np.abs(full["fused"] - ref["fused"].numpy()).max() <= H.TOL_BIG

    sd = synth.make_state_dict(1)
    img, ev = synth.make_inputs(5, 3)
    a = run(make_model(sd, "bf16x6", 10), img, ev)
    b = run(make_model(sd, "f32", 10), img, ev)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    a_sc = run(make_model(sd, "bf16x6", 10, outputs="scores"), img, ev)
    b_sc = run(make_model(sd, "f32", 10, outputs="scores"), img, ev)
    assert np.array_equal(a_sc["logits"], b_sc["logits"])
    assert np.array_equal(a_sc["logits"], a["logits"])


def test_duplicated_chunk_in_another_micro_batch_scores_identically():
    """Two internal passes of 48 chunks: a row's logit is formed from its own row in a fixed column order, so a chunk repeated in the
    second pass gets the same bits; and the scores-only forward saves one launch in EACH pass."""
    K = 10
    sd = synth.make_state_dict(9, 768, L, K)
    img, ev = synth.make_inputs(17, 2 * B_SPLIT)
    img[B_SPLIT + 7], ev[B_SPLIT + 7] = img[11], ev[11]
    m_sc = make_model(sd, "bf16x6", K, outputs="scores", micro_batch=B_SPLIT)
    m_full = make_model(sd, "bf16x6", K, micro_batch=B_SPLIT)
    sc, full = run(m_sc, img, ev, timed=True), run(m_full, img, ev, timed=True)
    assert np.array_equal(sc["logits"][11], sc["logits"][B_SPLIT + 7])
    assert np.array_equal(sc["logits"], full["logits"])
    assert m_sc.last_stage_times["gemm_launches"] == m_full.last_stage_times["gemm_launches"] - 2
    # one pass of 96 chunks: other grids, the same per-row arithmetic
    one = run(make_model(sd, "bf16x6", K, outputs="scores"), img, ev)
    assert np.array_equal(one["logits"], sc["logits"])
