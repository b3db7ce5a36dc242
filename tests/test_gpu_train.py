"""f-4: the train-mode forward, the model's backward pass and a whole optimiser step on the MI355X, against
fixtures the REFERENCE produced (tests/golden/make_golden.py: `gen_model_grad_cases`, `gen_train_step_case`):

  * grad_*.npz       the reference MMFMIL in train() mode (fp64 copy), its own CLAS2 + the trainers' regulariser / KL calls,
                     `loss.backward()`: norms and 192 sampled entries of EVERY parameter gradient, for K in {0, 2, 10}, both noise
                     models, L in {1, 2}, without dropout and with an injected attention-dropout mask (p = 0.1)
  * train_step_*.npz two whole steps of train/ucf_train.py:60-106 in the reference's own fp32 (forward, loss, backward,
                     torch.optim.AdamW(lr=2e-5).step()): sampled entries of all parameters after each step

The library's own mask generator (p > 0 without an injected mask) cannot reproduce torch's Philox stream: "parity unpinned";
what is checked for it is determinism per seed and the gradient against finite differences of the same masked function."""
import argparse
import os

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import losses, synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

GRAD_CASES = ["k2_student8", "k10_student8_mask", "k0_gauss_l1", "sharp_k2_student8"]


def make_model(wseed, L, K, noise, nu, compute="f32", p=0.0, factors=None):
    sd = synth.make_state_dict(wseed, 768, L, K)
    if factors is not None:
        sd = synth.sharpen_qk(sd, factors)
    args = argparse.Namespace(visual_layers=L, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model=noise, nu=nu)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, L, 8, 10, 10, "cuda", args, compute=compute)
    m.load_state_dict(sd)
    m = m.to("cuda:0")
    for a in list(m.temporal.image_attn_layers) + list(m.temporal.event_attn_layers):
        a.dropout = p
    return m, sd


def batch(bseed, B):
    img, ev, labels, lengths = synth.make_train_batch(bseed, B)
    return torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(lengths).cuda()


def run_case(name, compute="f32"):
    g = np.load(os.path.join(H.GOLDEN, f"grad_{name}.npz"))
    wseed, bseed, B, L, K, nu = (int(v) for v in g["cfg"])
    noise, p = str(g["noise"]), float(g["p"])
    lam_reg, lam_kl = (float(v) for v in g["lams"])
    factors = tuple(float(f) for f in g["factors"]) if "factors" in g.files else None      # peaked attention: synth.sharpen_qk
    model, _ = make_model(wseed, L, K, noise, nu, compute, p, factors)
    if p > 0:
        model.dropout_mask = torch.from_numpy(synth.make_dropout_mask(bseed, L, B, p)).cuda()
    model.train()
    img, ev, labels, lengths = batch(bseed, B)
    out = model(img, ev, None, None, lengths)
    total = losses.training_loss(out, labels, lengths, noise, nu, lam_reg, lam_kl)
    total.backward()
    return g, model, out, total


@pytest.mark.parametrize("name", GRAD_CASES)
def test_every_parameter_gradient_matches_the_reference_autograd(name):
    """Done-criterion of the round-3 verdict: every parameter gradient within 1e-4 relative (+ 1e-6 x the tensor's scale) of the
    reference's fp64 autograd, on sampled entries and in both norms.

    sharp_k2_student8 (peaked attention, synth.sharpen_qk (8, 4): the softmax backward P o (dP - sum P o dP) where P is not ~ 1/256): here
    the per-entry gate lies below what fp32 can give.  The reference's OWN fp32 autograd misses it against its fp64 gradients by 1.22x
    on its worst sampled entry (fixture field `grad_floor`, recorded by the generator; 0.65x on k2_student8, the same seeds with flat
    attention), so for a fixture that records such a floor the per-entry gate is max(1, 3 x floor) times the usual one -- 3.66x here,
    the margin over a reference-side floor the forward cases use; nothing in it comes from a kernel.  Measured on MI355X (f32 kernels):
    worst entry 2.6x the usual gate (event layer-0 out_proj.bias; 0.97x on k2_student8), i.e. 2.2x the reference's own fp32 error; both
    norms within 5.2e-7, and they keep the 1e-4 gate.  ARITHMETIC.md, "Gradients under peaked attention"."""
    g, model, out, total = run_case(name)
    entry_gate = max(1.0, 3.0 * float(g["grad_floor"])) if "grad_floor" in g.files else 1.0
    assert abs(float(total.detach()) - float(g["total"])) <= 2e-5 * max(1.0, abs(float(g["total"])))
    assert float(np.abs(out["logits"].detach().cpu().numpy().reshape(g["logits"].shape) - g["logits"]).max()) <= H.TOL_LOGIT
    names = [str(n) for n in g["names"]]
    params = dict(model.named_parameters())
    assert list(params.keys()) == names                              # the reference's registration order
    worst = {}
    for i, n in enumerate(names):
        grad = params[n].grad
        assert grad is not None, n
        got = grad.detach().cpu().double().numpy().reshape(-1)
        assert np.isfinite(got).all(), n
        l1, l2, mx = (float(v) for v in g[f"g{i}_norms"])
        want = g[f"g{i}_val"]
        err = np.abs(got[g[f"g{i}_idx"]] - want)
        tol = 1e-4 * np.abs(want) + 1e-6 * mx
        worst[n] = float((err / tol).max())
        assert (err <= entry_gate * tol).all(), (n, float(err.max()), mx, worst[n], entry_gate)
        assert abs(np.abs(got).sum() - l1) <= 1e-4 * l1 + 1e-12, (n, "L1")
        assert abs(np.sqrt((got * got).sum()) - l2) <= 1e-4 * l2 + 1e-12, (n, "L2")
    print(name, "worst sampled entry in units of the 1e-4 gate:", max(worst.items(), key=lambda t: t[1]), "entry gate", entry_gate)


def test_gradients_bf16x6_forward_arithmetic_meets_the_same_gate():
    """compute='bf16x6': the train forward's dense projections run on the exact-split kernels when the batch fills their grid (it does
    not at B = 3: fp32 kernels, same bits as f32) -- checked at the fixture's size for the dispatch, gradients to the same gate."""
    g, model, out, total = run_case("k2_student8", compute="bf16x6")
    params = dict(model.named_parameters())
    for i, n in enumerate(str(x) for x in g["names"]):
        got = params[n].grad.detach().cpu().double().numpy().reshape(-1)
        want, mx = g[f"g{i}_val"], float(g[f"g{i}_norms"][2])
        assert (np.abs(got[g[f"g{i}_idx"]] - want) <= 1e-4 * np.abs(want) + 1e-6 * mx).all(), n


def test_bf16x6_backward_on_the_split_kernel_at_a_batch_that_fills_its_grid():
    """B = 8 (2048 rows, 96 workgroups >= the 72 of the dispatch): in compute='bf16x6' the forward projections AND the backward's
    input-gradient products (dX = dY W, on three-plane splits of W^T; train.h `launch_dx`) run on the exact-split kernel.  Every
    parameter gradient against fp64 autograd through the oracle (itself pinned by the grad_*.npz fixtures at B = 3), the same
    gate as the fixtures'; the f32 handle at the same size alongside, whose bits must differ (another arithmetic ran); weight gradients
    on the split TN kernel (gemm_split_tn.h), bit-reproducible from run to run."""
    from oracle import iefvad_oracle as orc
    L, K, B = 2, 2, 8
    img, ev, _, _ = synth.make_train_batch(77, B)

    def scalar(o):
        return o["logits"].sum() + 0.5 * (o["image_mu"] * o["event_logvar"]).sum() + 0.25 * (o["event_mu"] * o["image_logvar"]).sum()

    grads = {}
    for compute in ("f32", "bf16x6", "bf16x6 again"):
        model, sd = make_model(5, L, K, "StudentT", 8, compute.split()[0], 0.0)
        model.train()
        scalar(model(torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda(), None, None, None)).backward()
        grads[compute] = {n: p.grad.detach().cpu().double() for n, p in model.named_parameters()}
    for n in grads["bf16x6"]:          # split-K partials reduced in index order, no atomics: the split kernels reproduce their bits
        assert torch.equal(grads["bf16x6"][n], grads["bf16x6 again"][n]), n
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    scalar(orc.forward(sd64, torch.from_numpy(img), torch.from_numpy(ev), orc.OracleConfig(num_layers=L, num_refinement_steps=K, nu=8),
                       dtype=torch.float64)).backward()
    differ = 0
    for n, want in ((k, v.grad) for k, v in sd64.items()):
        mx = float(want.abs().max())
        for compute in ("f32", "bf16x6"):
            err = (grads[compute][n] - want).abs()
            assert bool((err <= 1e-4 * want.abs() + 2e-6 * mx).all()), (compute, n, float(err.max()), mx)
        differ += int(not torch.equal(grads["f32"][n], grads["bf16x6"][n]))
    assert differ > len(sd64) // 2


@pytest.mark.parametrize("compute", ["bf16x6", "f32"])
def test_gradients_at_the_benched_batch_equal_the_sum_over_sub_batches(compute):
    """bench.py times the training step at the reference's UCF batch -- 128 chunks = 32,768 rows (/root/reference/train/ucf_train.py:44-48
    with parser.py's batch_size 64 per loader), K = 10 -- where the weight-gradient products run split-K over 16 - 32 row slices, the
    split NT / TN kernels at full grids and the attention products over 1,024 (chunk, head) pairs per launch; no fixture reaches that
    size (the reference's fp64 autograd at B = 128 is out of reach for a test).  A scalar that is a SUM OVER ROWS of the outputs
    makes every parameter gradient additive over chunks, so the B = 128 gradient must equal the sum, in fp64, of the gradients of
    sixteen B = 8 sub-batches -- each of which is the size the fp64-autograd test above pins -- to the fp32 gate; and the step
    must reproduce its bits from run to run at this size too.  p = 0 (the dropout generator indexes elements by their position in
    the batch, so a sub-batch would draw another mask)."""
    L, K, B, SUB = 2, 10, 128, 8
    img, ev, _, _ = synth.make_train_batch(91, B)
    img, ev = torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()

    def scalar(o):
        return (o["logits"].sum() + 0.5 * (o["image_mu"] * o["event_logvar"]).sum() + 0.25 * (o["event_mu"] * o["image_logvar"]).sum()
                + 0.125 * (o["fused"] * o["w_i"]).sum())

    model, _ = make_model(6, L, K, "StudentT", 8, compute, 0.0)
    model.train()
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        scalar(model(img, ev, None, None, None)).backward()
        runs.append({n: p.grad.detach().clone() for n, p in model.named_parameters()})
    for n in runs[0]:
        assert torch.equal(runs[0][n], runs[1][n]), n                  # fixed-order reductions at full grids
    total = {n: torch.zeros_like(g, dtype=torch.float64) for n, g in runs[0].items()}
    for b0 in range(0, B, SUB):
        model.zero_grad(set_to_none=True)
        scalar(model(img[b0:b0 + SUB].contiguous(), ev[b0:b0 + SUB].contiguous(), None, None, None)).backward()
        for n, p in model.named_parameters():
            total[n] += p.grad.detach().double()
    worst = 0.0
    for n, want in total.items():
        got = runs[0][n].double()
        mx = float(want.abs().max())
        err = (got - want).abs()
        ok = err <= 1e-4 * want.abs() + 2e-6 * mx
        assert bool(ok.all()), (compute, n, float(err.max()), mx)
        worst = max(worst, float(err.max()) / max(mx, 1e-30))
    print(f"B = 128 gradients vs the sum over sixteen B = 8 sub-batches ({compute}): worst max-relative error {worst:.2e}")


def test_gradients_are_bit_reproducible_and_accumulate():
    """No atomics in any reduction: two runs give the same bits; a second backward into existing .grad accumulates, as autograd does."""
    _, m1, _, _ = run_case("k2_student8")
    g1 = {n: p.grad.clone() for n, p in m1.named_parameters()}
    _, m2, _, _ = run_case("k2_student8")
    for n, p in m2.named_parameters():
        assert torch.equal(p.grad, g1[n]), n
    # accumulate: run the same step again on m2 without zeroing
    img, ev, labels, lengths = batch(41, 3)
    out = m2(img, ev, None, None, lengths)
    losses.training_loss(out, labels, lengths, "StudentT", 8, 1.0, 1.0).backward()
    for n, p in m2.named_parameters():
        assert torch.allclose(p.grad, 2 * g1[n], rtol=1e-6, atol=1e-12), n


@pytest.mark.parametrize("mode", ["library_generator", "injected_mask", "no_dropout"])
def test_fused_train_attention_equals_the_three_launch_path(mode, monkeypatch):
    """bf16x6 train-mode forward: ONE attention launch per layer (attention_split.h TRAIN: S -> softmax -> dropout -> Pd v with P and Pd
    stored) against the three launches it replaced (IEFVAD_TRAIN_ATTN=unfused: fp32-MFMA products, stand-alone softmax + dropout): same
    mask element for element (injected, or the counter-based bits of common.h), all eight outputs and every parameter gradient at the
    fp32 gates.  /root/reference/model/imf_vad.py:69-72,115,121 under model.train()."""
    _fused_train_attention_equals_unfused(mode, monkeypatch, None)


def test_fused_train_attention_equals_the_three_launch_path_with_peaked_attention(monkeypatch):
    """The same (injected mask) with the q / k rows sharpened (synth.sharpen_qk (8, 4)): P is far from 1/256, so the stored P, the
    dropout of a dominant key and the softmax backward P o (dP - sum P o dP) all carry weight."""
    _fused_train_attention_equals_unfused("injected_mask", monkeypatch, (8, 4))


def _fused_train_attention_equals_unfused(mode, monkeypatch, factors):
    p = 0.0 if mode == "no_dropout" else 0.1
    B, L = 3, 2
    img, ev, labels, lengths = batch(52, B)
    res = {}
    for which in ("fused", "unfused"):
        if which == "unfused":
            monkeypatch.setenv("IEFVAD_TRAIN_ATTN", "unfused")
        else:
            monkeypatch.delenv("IEFVAD_TRAIN_ATTN", raising=False)
        model, _ = make_model(41, L, 2, "StudentT", 8, "bf16x6", p, factors)
        if mode == "injected_mask":
            model.dropout_mask = torch.from_numpy(synth.make_dropout_mask(7, L, B, p)).cuda()
        model.dropout_seed = 4321
        model.train()
        out = model(img, ev, None, None, lengths)
        total = losses.training_loss(out, labels, lengths, "StudentT", 8, 1.0, 1.0)
        total.backward()
        res[which] = ({k: v.detach().clone() for k, v in out.items()}, {n: q.grad.clone() for n, q in model.named_parameters()}, float(total.detach()))
    (o1, g1, l1), (o2, g2, l2) = res["fused"], res["unfused"]
    assert abs(l1 - l2) <= 1e-5 * abs(l2)
    for k in o1:
        assert float((o1[k] - o2[k]).abs().max()) <= H.TOL_BIG, k
    for n in g1:
        scale = float(g2[n].abs().max())
        assert float((g1[n] - g2[n]).abs().max()) <= 1e-4 * scale + 1e-9, n
    if mode != "no_dropout":       # the mask did something: the outputs differ from a no-dropout forward
        model, _ = make_model(41, L, 2, "StudentT", 8, "bf16x6", 0.0, factors)
        model.train()
        o0 = model(img, ev, None, None, lengths)
        assert float((o0["image_mu"].detach() - o1["image_mu"]).abs().mean()) > 1e-4


@pytest.mark.parametrize("mode", ["library_generator", "injected_mask"])
def test_train_forward_keeps_probabilities_and_mask_in_one_tensor(mode):
    """bf16x6 train forward (csrc/attention_split.h TRAIN): ONE [B, 8, 256, 256] fp32 tensor per modality and layer carries
    P = softmax(q k^T) in its magnitudes and the dropout mask in its sign bits (set = dropped).  Read straight out of the training
    buffer (image modality, layer 0: behind x_0..x_L, q|k|v, the attention output and the pre-LayerNorm sum = (L + 6) U floats):
    |stored| against the softmax of the stored q | k in fp64, the sign bits against the injected mask / the counter-based generator of
    csrc/common.h re-derived here, the stored attention output against dropout(P) v.  (The first build passed an element of a register
    vector to __builtin_bit_cast and hipcc read element 0 for all sixteen: 18 % sign bits and |P| off by 2e-3 -- this test is that
    probe.)  /root/reference/model/imf_vad.py:70 (nn.MultiheadAttention(dropout=0.1) under train())."""
    B, L, p = 3, 2, 0.1
    img, ev, labels, lengths = batch(52, B)
    model, _ = make_model(41, L, 2, "StudentT", 8, "bf16x6", p)
    model.dropout_seed = 4321
    mask = None
    if mode == "injected_mask":
        mask = torch.from_numpy(synth.make_dropout_mask(7, L, B, p)).cuda()
        model.dropout_mask = mask
    model.train()
    out = model(img, ev, None, None, lengths)
    ws = out["logits"].grad_fn.ws.view(torch.float32)
    U, PU = B * 256 * 768, B * 8 * 256 * 256
    qkv = ws[(L + 1) * U:(L + 4) * U].view(B, 256, 3, 8, 96)
    att = ws[(L + 4) * U:(L + 5) * U].view(B, 256, 8, 96)
    P = ws[(L + 6) * U:(L + 6) * U + PU].view(B, 8, 256, 256)
    neg = P.view(torch.int32) < 0
    q, k, v = (qkv[:, :, j].permute(0, 2, 1, 3).double() for j in range(3))      # q is stored pre-scaled by 1 / sqrt(96)
    want = torch.softmax(q @ k.transpose(-1, -2), -1)
    assert float((P.abs().double() - want).abs().max()) <= 1e-6
    if mask is not None:
        dropped = mask[0, 0] == 0
    else:
        M32 = 0xFFFFFFFF

        def fmix32(x):
            x = x & M32
            x = x ^ (x >> 16); x = (x * 0x85EBCA6B) & M32
            x = x ^ (x >> 13); x = (x * 0xC2B2AE35) & M32
            return x ^ (x >> 16)
        seed = (4321 * 0x100000001B3 + 1 * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF      # train.h: modality 0, layer 0
        idx = torch.arange(PU, dtype=torch.int64, device="cuda")
        a = fmix32((idx & M32) ^ (seed & M32))
        bits = fmix32((a + (seed >> 32) + (idx >> 32) * 0x9E3779B1) & M32) >> 8
        dropped = (bits < int(p * 16777216.0)).view(B, 8, 256, 256)
    assert torch.equal(neg, dropped)
    assert 0.08 < float(neg.float().mean()) < 0.12
    Pd = torch.where(neg, torch.zeros_like(P), P * np.float32(1.0 / (1.0 - p))).double()
    assert float((att.double() - (Pd @ v).permute(0, 2, 1, 3)).abs().max()) <= 2e-6
    # ... and the backward reads the same tensor: gradients at the fp32 gates are covered by the fused-vs-three-launch test above


def test_train_forward_without_dropout_equals_the_eval_forward():
    """p = 0: train() changes nothing in the reference's forward; here the train path computes attention on other kernels (scores
    and probabilities materialised) -- fp32 gates against the eval path, all eight outputs."""
    model, sd = make_model(35, 2, 3, "StudentT", 8)
    img, ev, _, lengths = batch(45, 5)
    model.eval()
    with torch.no_grad():
        ref = model(img, ev, None, None, lengths)
    model.train()
    out = model(img, ev, None, None, lengths)
    assert list(out.keys()) == list(ref.keys()) == list(iefvad_amd.model.OUTPUT_KEYS)
    for k in ref:
        assert out[k].shape == ref[k].shape and out[k].requires_grad
        assert float((out[k].detach() - ref[k]).abs().max()) <= H.TOL_BIG, k
    assert float((torch.sigmoid(out["logits"].detach()) - torch.sigmoid(ref["logits"])).abs().max()) <= H.TOL_SIGMOID


def test_whole_training_steps_match_the_reference():
    """train/ucf_train.py:60-106, twice: model.train(), forward, CLAS2 + regulariser + KL, zero_grad, backward, AdamW step -- all
    parameters within 2e-6 of the reference's own fp32 run after each step, the losses within 1e-5."""
    g = np.load(os.path.join(H.GOLDEN, "train_step_k3_student8.npz"))
    wseed, bseed, B, L, K, nu, nsteps = (int(v) for v in g["cfg"])
    lam_reg, lam_kl = (float(v) for v in g["lams"])
    model, sd = make_model(wseed, L, K, str(g["noise"]), nu)
    names = [str(n) for n in g["names"]]
    params = dict(model.named_parameters())
    assert list(params.keys()) == names
    opt = losses.AdamW(model.parameters(), lr=float(g["lr"]))
    for step in range(nsteps):
        model.train()
        img, ev, labels, lengths = batch(bseed + step, B)
        out = model(img, ev, None, None, lengths)
        total = losses.training_loss(out, labels, lengths, str(g["noise"]), nu, lam_reg, lam_kl)
        opt.zero_grad()
        total.backward()
        opt.step()
        assert abs(float(total) - float(g["losses"][step])) <= 1e-5 * abs(float(g["losses"][step])), step
        moved = 0.0
        for i, n in enumerate(names):
            idx = g[f"p{i}_idx"]
            got = params[n].detach().cpu().numpy().reshape(-1)[idx]
            want = g[f"p{i}_step{step}"]
            err = np.abs(got - want)
            tol = np.full(err.shape, 2e-6)
            if n.endswith("in_proj_bias"):
                # the KEY bias has an exactly zero gradient (a constant added to every key's score leaves the softmax unchanged), so
                # what both sides feed to Adam there is fp32 rounding noise (~1e-10), which Adam's g / (|g| + eps) turns into an
                # update of up to lr per step: bounded, not comparable
                tol[(idx >= 768) & (idx < 1536)] = float(g["lr"]) * (step + 1) * 1.01
            assert (err <= tol).all(), (step, n, float(err.max()))
            moved = max(moved, float(np.abs(got - sd[n].numpy().reshape(-1)[idx]).max()))
        assert moved > 1e-5                                       # the step did move the parameters (lr 2e-5 per step)
    # the eval forward sees the updated weights (the shim's weight cache notices the in-place update)
    model.eval()
    with torch.no_grad():
        o1 = model(img, ev, None, None, lengths)["logits"]
    model.refresh_weights()
    with torch.no_grad():
        o2 = model(img, ev, None, None, lengths)["logits"]
    assert torch.equal(o1, o2)


def test_library_dropout_generator_is_deterministic_per_seed_and_differentiable():
    """p = 0.1 with the library's own counter-based mask ("parity unpinned": torch's Philox stream is not reproducible).  Same
    seed -> same bits; another seed -> another mask; about p of the attention weight mass is dropped; and the gradient is the
    gradient of THAT masked function (central differences along two random directions, same seed)."""
    model, _ = make_model(36, 1, 1, "StudentT", 8, p=0.1)
    model.train()
    img, ev, labels, lengths = batch(46, 2)

    def loss_at(seed):
        model.dropout_seed = seed
        out = model(img, ev, None, None, lengths)
        return out, losses.training_loss(out, labels, lengths, "StudentT", 8, 1.0, 1.0)

    o1, l1 = loss_at(1234)
    o2, l2 = loss_at(1234)
    o3, l3 = loss_at(99)
    assert torch.equal(o1["logits"], o2["logits"]) and float(l1) == float(l2)
    assert not torch.equal(o1["logits"], o3["logits"])
    for a in list(model.temporal.image_attn_layers) + list(model.temporal.event_attn_layers):
        a.dropout = 0.0
    o0, _ = loss_at(1234)
    d13 = float((o1["image_mu"] - o3["image_mu"]).abs().mean())
    d10 = float((o1["image_mu"] - o0["image_mu"]).abs().mean())
    assert d13 > 1e-4 and d10 > 1e-4                              # the mask matters, and differs between seeds
    for a in list(model.temporal.image_attn_layers) + list(model.temporal.event_attn_layers):
        a.dropout = 0.1
    model.zero_grad()
    _, l = loss_at(1234)
    l.backward()
    gen = torch.Generator(device="cuda").manual_seed(3)
    plist = [p for p in model.parameters()]
    for trial in range(2):
        dirs = [torch.randn(p.shape, device="cuda", generator=gen) for p in plist]
        an = sum(float((p.grad.double() * d.double()).sum()) for p, d in zip(plist, dirs))
        eps = 2e-4
        vals = []
        for sgn in (1, -1):
            with torch.no_grad():
                for p, d in zip(plist, dirs):
                    p.add_(sgn * eps * d)
            with torch.no_grad():
                vals.append(float(loss_at(1234)[1]))
            with torch.no_grad():
                for p, d in zip(plist, dirs):
                    p.sub_(sgn * eps * d)
        fd = (vals[0] - vals[1]) / (2 * eps)
        assert abs(an - fd) <= 2e-2 * max(abs(fd), 1e-3), (trial, an, fd)


def test_adamw_is_a_torch_optimizer_scheduler_and_state_dict_interchange():
    """The trainers' optimiser plumbing (ucf_train.py:28-33,141-153): MultiStepLR drives `losses.AdamW`; its state_dict loads into
    torch.optim.AdamW and back; the per-step UPDATE equals torch's to 1e-6 of its own magnitude (the hyper-parameter scalars are
    formed in double on the host, as torch forms them)."""
    from torch.optim.lr_scheduler import MultiStepLR
    g = torch.Generator().manual_seed(7)
    shapes = [(768, 768), (2304,), (5,)]
    ref = [torch.randn(s, generator=g).requires_grad_(True) for s in shapes]
    dev = [r.detach().clone().cuda().requires_grad_(True) for r in ref]
    o_ref, o_dev = torch.optim.AdamW(ref, lr=3e-4), losses.AdamW(dev, lr=3e-4)
    s_ref, s_dev = MultiStepLR(o_ref, [2, 4], 0.1), MultiStepLR(o_dev, [2, 4], 0.1)
    assert isinstance(o_dev, torch.optim.Optimizer)
    for step in range(6):
        before = [d.detach().clone() for d in dev]
        for r, d in zip(ref, dev):
            gr = torch.randn(r.shape, generator=g) * (10.0 ** (step - 3))
            r.grad, d.grad = gr.clone(), gr.clone().cuda()
        b_ref = [r.detach().clone() for r in ref]
        o_ref.step()
        o_dev.step()
        s_ref.step()
        s_dev.step()
        assert o_dev.param_groups[0]["lr"] == pytest.approx(o_ref.param_groups[0]["lr"])
        for r, d, b0, br in zip(ref, dev, before, b_ref):
            upd_ref = (r.detach() - br).double()
            upd_dev = (d.detach().cpu() - b0.cpu()).double()
            # the update is a difference of fp32 parameters: half an ulp of the parameter each side, plus 1e-6 of the update itself
            tol = 1e-6 * upd_ref.abs() + 1.2e-7 * br.abs().double() + 1e-12
            assert bool(((upd_ref - upd_dev).abs() <= tol).all()), step
    # state_dict interchange, both directions
    import copy
    sd = copy.deepcopy(o_dev.state_dict())          # state_dict() hands out the live state tensors, as torch's does
    assert set(sd["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 6.0
    o_ref2 = torch.optim.AdamW([r.detach().clone().cuda().requires_grad_(True) for r in ref], lr=3e-4)
    o_ref2.load_state_dict(sd)
    o_dev2 = losses.AdamW([d.detach().clone().requires_grad_(True) for d in dev], lr=1.0)
    o_dev2.load_state_dict(copy.deepcopy(o_ref2.state_dict()))
    assert o_dev2.param_groups[0]["lr"] == o_dev.param_groups[0]["lr"]
    for a, b in zip(o_dev2.param_groups[0]["params"], dev):
        gr = torch.ones_like(b)
        a.grad, b.grad = gr, gr.clone()
    o_dev2.step()
    o_dev.step()
    for a, b in zip(o_dev2.param_groups[0]["params"], dev):
        assert torch.equal(a.detach(), b.detach())
    with pytest.raises(ValueError, match="no CPU fallback"):
        losses.AdamW([torch.zeros(4)])


def test_nan_rule_on_the_device_is_the_trainers_rule():
    """/root/reference/train/ucf_train.py:50-53 per input tensor: `if torch.isnan(x).any(): x = torch.nan_to_num(x, nan=0.0)` --
    a tensor WITH a NaN is rewritten as nan_to_num does (its infinities too), one without keeps every bit (its infinities too);
    `iefvad_nan_rule` does it without the host reading the flag (trainer._nan_rule_pair), in place."""
    from iefvad_amd import trainer
    gen = torch.Generator(device="cuda").manual_seed(3)
    img = torch.randn(4, 256, 768, device="cuda", generator=gen)
    ev = torch.randn(4, 256, 768, device="cuda", generator=gen)
    img[1, 7, 5] = float("nan"); img[3, 255, 767] = float("nan"); img[0, 0, 0] = float("inf"); img[2, 9, 9] = float("-inf")
    ev[2, 3, 4] = float("inf"); ev[0, 1, 2] = float("-inf")
    want_img = torch.nan_to_num(img, nan=0.0)
    want_ev = ev.clone()
    a, b = trainer._nan_rule_pair(img, ev)
    assert a.data_ptr() == img.data_ptr() and b.data_ptr() == ev.data_ptr()
    assert torch.equal(a.view(torch.int32), want_img.view(torch.int32))
    assert torch.equal(b.view(torch.int32), want_ev.view(torch.int32))
    assert trainer._NAN_FLAGS[img.device].tolist() == [1, 0]
    # the other way round, and the torch form for what the kernel does not take (fp16 rows)
    a, b = trainer._nan_rule_pair(ev, want_img)
    assert torch.equal(a.view(torch.int32), want_ev.view(torch.int32)) and trainer._NAN_FLAGS[img.device].tolist() == [0, 0]
    h = torch.tensor([1.0, float("nan"), float("inf"), 2.0], device="cuda", dtype=torch.float16)
    a, _ = trainer._nan_rule_pair(h, h.clone())
    assert torch.equal(a, torch.nan_to_num(h, nan=0.0))


def test_train_mode_error_paths():
    model, _ = make_model(37, 1, 0, "StudentT", 8, compute="bf16")
    model.train()
    x = torch.zeros(1, 256, 768, device="cuda")
    with pytest.raises(RuntimeError, match="fp32-accurate"):
        model(x, x, None, None, None)
    model, _ = make_model(37, 1, 0, "StudentT", 8)
    model.train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(x.cpu(), x.cpu(), None, None, None)
    model.dropout_mask = torch.ones(3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="dropout_mask"):
        model(x, x, None, None, None)
    model.dropout_mask = None
    out = model(x, x, None, None, None)
    ws = out["logits"].grad_fn.ws                 # keep the training buffer past the node's own release
    out["logits"].sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="twice"):
        out["fused"].sum().backward()
    # ... and the library itself: the backward's scratch overwrote saved states, so the forward's record is retired and a second
    # iefvad_train_backward on the same buffer fails by name instead of differentiating garbage (include/iefvad.h)
    import ctypes as C
    from iefvad_amd import lib as L_
    lib = L_.load_library()
    dout, dw = L_.OutputGrads(), L_.WeightGrads()
    rc = lib.iefvad_train_backward(model._handle, 1, C.c_void_p(ws.data_ptr()), ws.numel(), C.byref(dout), C.byref(dw),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0 and "no iefvad_train_forward" in L_.last_error()
    # an in-place edit of an output the library reads again in the backward raises, as autograd does for the reference's modules
    out = model(x, x, None, None, None)
    out["image_mu"].add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out["logits"].sum().backward()


def test_paired_training_loop_keeps_the_reference_bookkeeping(tmp_path, monkeypatch):
    """`trainer.train_paired` (counterpart of train/ucf_train.py:16-156) on a tiny synthetic set: steps run, the periodic evaluation
    goes through harness.test, the best checkpoint holds model + optimiser state (torch.optim format), the epoch end steps the
    scheduler and reloads the best weights, and the file ends as a bare state_dict that the model loads."""
    from torch.utils.data import DataLoader, Dataset
    from iefvad_amd import harness, trainer
    monkeypatch.chdir(tmp_path)

    class Vids(Dataset):
        def __init__(self, seed, n, label):
            self.seed, self.n, self.label = seed, n, label

        def __len__(self):
            return self.n

        def __getitem__(self, i):
            length = [256, 90, 200, 37][i % 4]
            img, ev = synth.make_video(self.seed, i, 256)
            img[length:] = 0
            ev[length:] = 0
            return torch.from_numpy(img), torch.from_numpy(ev), self.label, length

    label_map = {c: c.lower() for c in synth.UCF_CLASSES}
    normal = DataLoader(Vids(61, 4, "Normal"), batch_size=2, shuffle=False, drop_last=True)
    abnormal = DataLoader(Vids(62, 4, "Arson"), batch_size=2, shuffle=False, drop_last=True)
    test_items, lens = [], [300, 40, 256, 100] + [30] * 12
    for i, n in enumerate(lens):
        img, ev = synth.make_video(63, i, n)
        ci, _ = harness.process_split(img, 256)
        ce, _ = harness.process_split(ev, 256)
        test_items.append((torch.from_numpy(ci).unsqueeze(0), torch.from_numpy(ce).unsqueeze(0), (synth.UCF_CLASSES[i % 14],), torch.tensor([n])))
    gt = synth.make_gt(63, sum(lens))
    args = argparse.Namespace(dataset="ucfcrime", visual_length=256, lr=2e-5, scheduler_milestones=[1], scheduler_rate=0.1, max_epoch=2,
                              print_steps=4, exp_name="mini", noise_model="StudentT")
    model, sd = make_model(38, 1, 1, "StudentT", 8)
    opt = losses.AdamW(model.parameters(), lr=args.lr)
    logs = []
    best = trainer.train_paired(args, model, normal, abnormal, test_items, label_map, "cuda:0", gt=gt, log=logs.append, optimizer=opt)
    assert len(logs) == 2 and all(r["step"] == 4 for r in logs) and 0.0 < best <= 1.0          # i = 1 of each epoch: step 1 * 2 * 2
    assert {"train/loss", "train/loss_classification", "train/loss_reg", "train/loss_kl", "auc", "ap"} <= set(logs[0])
    assert opt.param_groups[0]["lr"] == pytest.approx(2e-6)                                     # MultiStepLR stepped at epoch 1
    final = torch.load("checkpoints/mini.pth", weights_only=True)
    assert list(final.keys()) == list(sd.keys())                                                # bare state_dict, reference key order
    moved = max(float((final[k].cpu() - sd[k]).abs().max()) for k in sd)
    assert 1e-6 < moved < 1e-3
    model.load_state_dict(final)
    model.eval()
    with torch.no_grad():
        assert torch.isfinite(model(test_items[0][0][0].cuda(), test_items[0][1][0].cuda(), None, None, None)["logits"]).all()
