"""The "uncertain heads" regime on the CPU: the oracle against the prec_*.npz captures of the reference, and the conditions that keep
tests/test_gpu_precision.py from being vacuous.

The fusion (imf_vad.py:130-144) is  w_m = factor exp(-logvar_m), den = w_i + w_e + eps, n_m = w_m / den, z0 = n_i mu_i + n_e mu_e.
With synth.make_state_dict's own weights eps / den ~ 5e-9: the weights sum to one, `factor` cancels, and every fwd_* fixture pins the
same numbers whatever nu and epsilon are.  The prec_* fixtures (tests/golden/make_golden_precision.py) shift the two log-variance biases
by (15.5, 17.0), or raise epsilon to 1e-2, so that neither cancels.  This is the first place the oracle's own `factor` / `epsilon` lines
are pinned by the reference.  Nothing here needs a GPU."""
import itertools

import numpy as np
import pytest
import torch

from iefvad_amd import synth
from oracle import iefvad_oracle as orc
from tests import helpers as H

SHIFTED = ("k3_student8", "k3_student1", "k3_gauss")          # one set of weights and inputs, three noise models


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", H.PRECISION_CASES)
def test_oracle_matches_the_reference_where_factor_and_epsilon_matter(name, dtype):
    g, cfg, sd, img, ev = H.load_precision_case(name)
    out = orc.forward(sd, torch.from_numpy(img), torch.from_numpy(ev), H.precision_oracle_cfg(cfg), dtype)
    out = {k: v.numpy() for k, v in out.items()}
    errs = H.compare_outputs(out, g)
    assert np.abs(out["w_i"].mean(-1) - g["w_i_mean"]).max() < 2e-6
    assert np.abs(out["w_e"].mean(-1) - g["w_e_mean"]).max() < 2e-6
    print(name, errs)


@pytest.mark.parametrize("name", H.PRECISION_CASES)
def test_fixture_records_its_floors_and_its_formula_floor(name):
    """The recorded fields are what the generator says they are: `formula_floor` is reproduced from the stored heads (the literal fp32
    lines in torch against fuse_fp64), the fixture's own w_i / w_e / fused (K = 0) lie within it, and 3 x the recorded forward floors
    stays under the fp32 gates -- the regime costs no precision."""
    g, cfg, _, _, _ = H.load_precision_case(name)
    ff = float(g["formula_floor"])
    assert 1e-8 < ff < 4e-7, ff                                    # a handful of fp32 roundings: exp, factor, two additions, the division
    assert 3 * float(g["floor_big"]) <= H.TOL_BIG and 3 * float(g["floor_logit"]) <= H.TOL_LOGIT and 3 * float(g["floor_sigmoid"]) <= H.TOL_SIGMOID
    errs = H.formula_errors(g, cfg["noise"], cfg["nu"], cfg["epsilon"], fused=cfg["K"] == 0)
    assert max(errs.values()) <= ff * (1 + 1e-6), (errs, ff)      # the generator's maximum is over these very elements
    assert max(float(g[k].max()) for k in ("image_logvar", "event_logvar")) < 21.0
    if name != "k0_student5_eps":
        assert float(g["one_minus_sum"]) > 0.02, float(g["one_minus_sum"])


def test_shifted_cases_are_separated_far_beyond_the_gates():
    """Any two of the three noise models differ in w_i by a median of at least 20 x the gate the parity tests apply."""
    gs = {n: H.load_precision_case(n)[0] for n in SHIFTED}
    for a, b in itertools.combinations(SHIFTED, 2):
        gate = max(H.case_gates(gs[a], (H.TOL_BIG,))[0], H.case_gates(gs[b], (H.TOL_BIG,))[0])
        sep = {k: float(np.median(np.abs(gs[a][k] - gs[b][k]))) for k in ("w_i", "fused", "logits")}
        print(a, b, sep, "gate", gate)
        assert sep["w_i"] >= 20 * gate, (a, b, sep)
        assert sep["fused"] >= 20 * gate and sep["logits"] >= 20 * gate, (a, b, sep)
        for k in ("image_mu", "event_mu", "image_logvar", "event_logvar"):      # the heads do not depend on the noise model
            assert np.array_equal(gs[a][k], gs[b][k]), k


@pytest.mark.parametrize("name", H.PRECISION_CASES)
def test_a_wrong_factor_or_a_dropped_epsilon_misses_the_formula_gate_everywhere(name):
    """What the formula layer of the GPU tests can see: fuse_fp64 of the fixture's heads with the factor forced to 1, or with epsilon
    forced to 0, misses the fixture's w_i by at least 100 x the gate (3 x formula_floor, relative) on at least 90 % of the elements."""
    g, cfg, _, _, _ = H.load_precision_case(name)
    gate = 3 * float(g["formula_floor"])
    heads = [g[k] for k in ("image_mu", "image_logvar", "event_mu", "event_logvar")]
    wrong = {"eps = 0": (cfg["noise"], 0.0)}
    if cfg["noise"] == "StudentT":
        wrong["factor = 1"] = ("Gaussian", cfg["epsilon"])
    for what, (noise, eps) in wrong.items():
        n_i = H.fuse_fp64(*heads, noise, cfg["nu"], eps)[0]
        rel = np.abs(g["w_i"] - n_i) / n_i
        frac = float((rel >= 100 * gate).mean())
        print(name, what, "fraction of elements missed by >= 100 gates:", frac, "10th percentile in gates:", float(np.percentile(rel, 10) / gate))
        assert frac >= 0.9, (name, what, frac)


def test_seeded_regime_separates_nothing():
    """Why the regime exists: with make_state_dict's own weights, Student-8, Student-5, nu = 1 and Gaussian give the same outputs to
    1e-7 (fp64), and no parameter gradient of the scalar moves by a hundredth of a gate."""
    g, cfg, sd, img, ev = H.load_precision_case("k3_student8")
    sd = synth.make_state_dict(cfg["wseed"], 768, cfg["L"], cfg["K"])      # the same weights, unshifted
    outs = []
    for noise, nu in (("StudentT", 8), ("StudentT", 5), ("StudentT", 1), ("Gaussian", 8)):
        c = orc.OracleConfig(num_layers=cfg["L"], num_refinement_steps=cfg["K"], lambda_ref=cfg["lam"], noise_model=noise, nu=nu)
        outs.append(orc.forward(sd, torch.from_numpy(img), torch.from_numpy(ev), c, torch.float64))
    worst = max(float((o[k] - outs[0][k]).abs().max()) for o in outs[1:] for k in ("fused", "w_i", "w_e", "logits"))
    print("seeded regime, worst difference between noise models:", worst)
    assert worst <= 1e-7, worst
    sep = H.grad_gates(H.oracle_precision_grads("Gaussian", 1, shift=(0.0, 0.0)), H.oracle_precision_grads("StudentT", 1, shift=(0.0, 0.0)))
    print("seeded regime, worst gradient separation in gates:", max(sep.values()))
    assert max(sep.values()) <= 1e-2, max(sep.items(), key=lambda t: t[1])


def test_gradients_separate_gaussian_from_student8_in_the_shifted_regime():
    """At least 10 of the 46 parameter gradients of the scalar move by at least 10 gates between the two noise models (fp64 autograd
    through the oracle, B = 1), while the oracle's own fp32 autograd stays below one gate."""
    s8, ga = H.oracle_precision_grads("StudentT", 1), H.oracle_precision_grads("Gaussian", 1)
    assert len(s8) == 46
    sep = H.grad_gates(ga, s8)
    n = sum(v >= 10 for v in sep.values())
    floor = H.grad_gates(H.oracle_precision_grads("StudentT", 1, torch.float32), s8)
    print("tensors separated by >= 10 gates:", n, "worst", max(sep.items(), key=lambda t: t[1]), "fp32 floor", max(floor.items(), key=lambda t: t[1]))
    assert n >= 10, sep
    assert max(floor.values()) < 1.0, floor


GRAD_NOISES = [("StudentT", 8), ("StudentT", 1), ("Gaussian", 8)]


@pytest.mark.parametrize("noise,nu", GRAD_NOISES, ids=["student8", "student1", "gauss"])
def test_gradient_floor_of_the_oracle_at_the_gpu_tests_batch(noise, nu):
    """The floor the GPU gradient gate max(1, 3 x floor) is built on, re-measured at B = 3: the oracle's fp32 autograd against its fp64
    autograd (H.oracle_precision_grad_floor, the function the GPU tests call -- there is no recorded figure to pad).  It lies below one
    gate (0.52 Student-8, 0.50 Gaussian on this CPU), so the GPU gate stays under 3 of the usual gates whatever BLAS sums the oracle."""
    floor, name = H.oracle_precision_grad_floor(noise, 3, nu)
    print(noise, nu, "fp32 autograd floor at B = 3 in gates:", floor, name)
    assert 0.05 <= floor < 1.0, (floor, name)


def test_gradients_separate_the_noise_models_at_the_gpu_tests_batch():
    """At B = 3, where the GPU tests hold the gradients: Gaussian and nu = 1 each move at least 10 of the 46 tensors by at least 10 of
    the gates the GPU tests allow (max(1, 3 x floor)) away from Student-8."""
    s8 = H.oracle_precision_grads("StudentT", 3)
    for noise, nu in GRAD_NOISES[1:]:
        allowed = max(1.0, 3.0 * max(H.oracle_precision_grad_floor("StudentT", 3, 8)[0], H.oracle_precision_grad_floor(noise, 3, nu)[0]))
        sep = H.grad_gates(H.oracle_precision_grads(noise, 3, nu=nu), s8)
        n = sum(v >= 10 * allowed for v in sep.values())
        print(noise, nu, "tensors separated from Student-8 by >= 10 allowed gates at B = 3:", n, "of", len(sep), "worst", max(sep.values()))
        assert n >= 10, (noise, nu, sep)
