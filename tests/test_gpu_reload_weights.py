"""Weights given twice.  iefvad_set_weights allocates the fp32 arena and the arena of each derived form (bf16 copies and the row-block
kernels' weight streams, three-plane splits, fp16 planes and their running-max words, the transposed planes of the bf16x6 backward) on
its first call and carves them again, in the same walk over the projection matrices (csrc/iefvad.hip for_each_proj), on every later
one.  A model that was given state dict A, ran, and was then given state dict B by `load_state_dict` must therefore compute what a
fresh model given B computes, bit for bit: nothing of A may survive in a reused arena, a weight stream, a captured graph or a plane
that is rebuilt lazily.

Batch sizes: 6 chunks is the smallest batch at which the split kernels take the projections (kSplitMinWgs = 72 workgroups, csrc/launch_rules.h), and a
batch the library replays from a captured hipGraph; the bf16 mode runs once more at 8 chunks = 2,048 rows, the row count
tests/test_gpu_rowblock_units.py gives the one-block row-block kernels, with the forward's own threshold lowered to that grid
(IEFVAD_ROWBLOCK_MIN_WGS) so that all four of them read their re-packed streams.  Needs a real MI355X: run with `-m gpu`."""
import argparse

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import synth

pytestmark = pytest.mark.gpu

L, K = 2, 2
SEED_A, SEED_B = 21, 22


def make_model(sd, compute):
    args = argparse.Namespace(visual_layers=L, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, L, 8, 10, 10, "cuda", args, compute=compute)
    m.load_state_dict(sd)
    for a in list(m.temporal.image_attn_layers) + list(m.temporal.event_attn_layers):
        a.dropout = 0.0
    return m.to("cuda:0").eval()


def run(model, img, ev, timed=False):
    with torch.no_grad():
        out = model(img, ev, None, None, None, timed=timed)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def train_grads(model, img, ev):
    """One train-mode forward + backward of a scalar that reaches every parameter; the gradients as numpy arrays."""
    model.train()
    model.zero_grad(set_to_none=True)
    out = model(img, ev, None, None, None)
    (out["logits"].sum() + 0.5 * (out["image_mu"] * out["event_logvar"]).sum() + 0.25 * (out["fused"] * out["w_e"]).sum()).backward()
    torch.cuda.synchronize()
    model.eval()
    return {n: p.grad.detach().cpu().numpy() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("compute,B", [("f32", 6), ("bf16", 6), ("bf16", 8), ("bf16x6", 6), ("fp16x3", 6)])
def test_reloaded_model_equals_fresh_model(compute, B, monkeypatch):
    rowblock = compute == "bf16" and B == 8
    if rowblock:
        monkeypatch.setenv("IEFVAD_ROWBLOCK_MIN_WGS", "64")       # read at handle creation: 2,048 rows are 64 workgroups of in_proj / out_proj
    sd_a, sd_b = synth.make_state_dict(SEED_A, 768, L, K), synth.make_state_dict(SEED_B, 768, L, K)
    img, ev = (torch.from_numpy(x).cuda() for x in synth.make_inputs(40 + B, B))
    train = compute == "bf16x6"

    reloaded = make_model(sd_a, compute)
    first = run(reloaded, img, ev)
    if train:
        train_grads(reloaded, img, ev)          # builds the transposed planes of A: the reload must invalidate them
    reloaded.load_state_dict(sd_b)
    again = run(reloaded, img, ev, timed=rowblock)
    fresh_model = make_model(sd_b, compute)
    fresh = run(fresh_model, img, ev)

    if rowblock:
        # out_proj + LayerNorm and heads + fusion ran as row-block kernels: no stand-alone LayerNorm or fusion launch was timed
        st = reloaded.last_stage_times
        assert st["layernorm_ms"] == 0.0 and st["fusion_ms"] == 0.0 and st["gemm_launches"] == 2 * L + 2, st
    assert sorted(again) == sorted(fresh) == sorted(iefvad_amd.OUTPUT_KEYS)
    for k in fresh:
        assert not np.array_equal(first[k], fresh[k]), k          # A and B are different models
        assert np.array_equal(again[k], fresh[k]), (compute, B, k, float(np.abs(again[k] - fresh[k]).max()))

    if train:
        g_again, g_fresh = train_grads(reloaded, img, ev), train_grads(fresh_model, img, ev)
        assert sorted(g_again) == sorted(g_fresh) and len(g_fresh) == 38 + 4 * K          # every tensor iefvad_set_weights uploads
        for n in g_fresh:
            assert np.any(g_fresh[n] != 0), n
            assert np.array_equal(g_again[n], g_fresh[n]), (n, float(np.abs(g_again[n] - g_fresh[n]).max()))
