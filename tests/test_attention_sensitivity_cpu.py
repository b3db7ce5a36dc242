"""What the forward tests can see of a wrong attention, measured on the CPU oracle (no GPU): five mutations of
softmax(q k^T / sqrt d) v in oracle/iefvad_oracle.py::_self_attention, and how far each moves the 768-d outputs (worst of fused /
mu / logvar / w, max abs, fp64).

With synth.make_state_dict's own weights the scores are tiny and softmax is an almost flat average over the 256 keys (weights seed
11, inputs seed 12, B = 2, L = 2, K = 3: max |score| 0.36 / 1.8 in layer 0 / 1, mean over queries of max_k P 0.0047 / 0.0096, flat =
0.0039).  There the mutations move the outputs by

    P replaced by 1/256          2.5e-2        under the bf16 gate (4e-2): a bf16 forward with NO attention passes
    last key left out            6.6e-3        under the bf16 gate
    P of keys 3 and 4 swapped    5.4e-3        under the bf16 gate (and under the 6e-3 "fp64 of rounded operands" gate)
    score scale off by 1 %       2.6e-4        13 x the f32 gate (2e-5) only
    no max subtraction           0             nothing, in any arithmetic: no score exceeds 1.8

which is why the suite also runs weights whose q / k rows are scaled up (synth.sharpen_qk; fixtures fwd_sharp_*, fwd_over_*,
vitb_fwd_sharp_*, grad_sharp_*).  This file asserts that THOSE inputs can see: the GPU tests that compare a forward on the sharpened
weights with the reference's fixture at the bf16 gate would fail on each structural mutation, the fp32-class ones (f32, bf16x6,
fp16x3) on all four.  The 1 % scale error moves the outputs by ~1e-2, BELOW the bf16 gate: it stays the fp32-class arithmetics' to
catch, and for the bf16 kernels the attention unit test's (tests/test_gpu_rowblock_units.py::test_attention_kernel_alone)."""
import math

import numpy as np
import pytest
import torch

from iefvad_amd import synth
from oracle import iefvad_oracle as orc
from tests import helpers as H
from tests import vitb_cases as V

TOL_BIG_BF16 = 4e-2                        # tests/test_gpu_bf16.py
SHARP, OVER = (8, 4), (16, 4)


def mutated_attention(kind):
    def attn(x, w_in, b_in, w_out, b_out, heads):
        B, T, D = x.shape
        dh = D // heads
        q, k, v = ((x @ w_in.t() + b_in).split(D, dim=-1))
        q, k, v = (t.reshape(B, T, heads, dh).transpose(1, 2) for t in (q, k, v))
        s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
        if kind == "scale":
            s = s * 1.01
        if kind == "drop_last":
            s = s[..., :-1]
            v = v[..., :-1, :]
        if kind != "no_max":
            s = s - s.max(dim=-1, keepdim=True).values
        p = torch.exp(s)
        p = p / p.sum(dim=-1, keepdim=True)
        if kind == "flat":
            p = torch.full_like(p, 1.0 / T)
        if kind == "swap":
            p = p.clone()
            p[..., [3, 4]] = p[..., [4, 3]]
        return (p @ v).transpose(1, 2).reshape(B, T, D) @ w_out.t() + b_out
    return attn


def forward(monkeypatch, kind, sd, img, ev, dtype):
    if kind is not None:
        monkeypatch.setattr(orc, "_self_attention", mutated_attention(kind))
    out = orc.forward(sd, torch.from_numpy(img), torch.from_numpy(ev), orc.OracleConfig(num_layers=2, num_refinement_steps=3, nu=8), dtype)
    monkeypatch.undo()
    return out


def test_the_unmutated_restatement_is_the_oracles_attention(monkeypatch):
    sd = synth.sharpen_qk(synth.make_state_dict(11, 768, 2, 3), SHARP)
    img, ev = synth.make_inputs(12, 1)
    a, b = forward(monkeypatch, None, sd, img, ev, torch.float64), forward(monkeypatch, "none", sd, img, ev, torch.float64)
    for k in a:
        assert float((a[k] - b[k]).abs().max()) <= 1e-12, k


@pytest.mark.parametrize("kind", ["flat", "drop_last", "swap", "scale"])
def test_sharpened_weights_see_a_wrong_attention(monkeypatch, kind):
    """(8, 4), B = 2, fp64: flat 0.92, dropped key 0.35, swap 0.45, 1 % scale 1.0e-2 when this was written."""
    sd = synth.sharpen_qk(synth.make_state_dict(11, 768, 2, 3), SHARP)
    img, ev = synth.make_inputs(12, 2)
    good = forward(monkeypatch, None, sd, img, ev, torch.float64)
    bad = forward(monkeypatch, kind, sd, img, ev, torch.float64)
    moved = max(float((good[k] - bad[k]).abs().max()) for k in H.BIG_KEYS)
    print(kind, "moves the 768-d outputs by", moved)
    assert moved >= 100 * H.TOL_BIG, (kind, moved)
    if kind != "scale":            # a 1 % scale error is below the bf16 gate: see the module docstring
        assert moved >= 5 * TOL_BIG_BF16, (kind, moved)


def test_overflow_weights_need_the_max_subtraction(monkeypatch):
    sd = synth.sharpen_qk(synth.make_state_dict(11, 768, 2, 3), OVER)
    img, ev = synth.make_inputs(12, 2)
    out = forward(monkeypatch, "no_max", sd, img, ev, torch.float32)
    assert not torch.isfinite(out["fused"]).all()
    assert torch.isfinite(forward(monkeypatch, None, sd, img, ev, torch.float32)["fused"]).all()


def regime_fixtures():
    out = [("fwd", n) for n in H.golden_cases(regimes=("sharp", "over")) + H.golden_cases(big=True, regimes=("sharp", "over"))]
    return out + [("vitb_fwd", n) for n in V.FWD_CASES if n.startswith("sharp")]


def test_every_regime_has_its_fixtures():
    names = [n for _, n in regime_fixtures()]
    assert {"sharp_k3_student8", "sharp_b48_k3", "over_k3_student8", "sharp_k3"} <= set(names)


@pytest.mark.parametrize("family,name", regime_fixtures())
def test_recorded_attention_statistics_stay_in_their_regime(family, name):
    """A later change of seeds or factors must not quietly return these fixtures to the flat regime: every (modality, layer) keeps
    a dominant key on average, the overflow case a score beyond exp2's fp32 range without the max subtraction (log2 units, the
    kernels' own: score x log2 e > 128).  The recorded floors are the reference's own fp32-vs-fp64 distance: 3 x floor stays
    under the fp32 gates, so those remain the binding ones."""
    g = np.load(H.GOLDEN + f"/{family}_{name}.npz")
    L = int(g["meta"][3])
    assert g["factors"].shape == (L,) and g["att_mean_max_p"].shape == g["att_max_score"].shape == (2, L)
    assert (g["att_mean_max_p"] >= 0.3).all(), g["att_mean_max_p"]
    if H.case_regime(name) == "over":
        assert float(g["att_max_score"].max()) * math.log2(math.e) > 128
    else:
        assert float(g["att_max_score"].max()) * math.log2(math.e) < 126      # a sharp case does not depend on the max subtraction
    assert H.case_gates(g, (H.TOL_BIG, H.TOL_LOGIT, H.TOL_SIGMOID)) == (H.TOL_BIG, H.TOL_LOGIT, H.TOL_SIGMOID)


def test_attention_unit_inputs_keep_the_boundary_cap_in_the_model_alone():
    """tests/test_gpu_rowblock_units.py::test_attention_kernel_alone lets an output differ from the fp64 model only where the model says
    the value is within its allowance of a bf16 rounding boundary, and caps those at 8 % of the outputs.  The designed q, k, v must
    leave room under that cap before any kernel runs: one chunk of each kind per modality, the model against itself."""
    from tests import test_gpu_rowblock_units as U
    for m in range(2):
        q, k, v = U.attention_case(len(U.ATT_KINDS), m, 7 + m)
        ref, tol, P = U.attention_model(q, k, v)
        assert torch.isfinite(ref).all() and float(P.sum(-1).sub(1).abs().max()) < 0.02
        frac = U.check_bf16_output(U.bf(ref).to(torch.bfloat16), ref, tol, "model")
        print("modality", m, "fraction of outputs on a boundary:", frac)
        assert frac < 0.03, frac
        s = q @ k.transpose(-1, -2)
        kinds = [U.ATT_KINDS[(c + m) % len(U.ATT_KINDS)] for c in range(len(U.ATT_KINDS))]
        ext, flat = kinds.index("extreme"), kinds.index("flat")
        assert float(s[ext].max()) > 115 and float(s[ext].min()) < -115 and float(s[ext, :, 128:].max()) < -110
        assert float(s[flat].abs().max()) < 2.5 and float(s[kinds.index("std20")].std()) > 15
