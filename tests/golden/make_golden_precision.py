"""Reference captures of the "uncertain heads" regime, in which the Student-t factor and epsilon of the precision-weighted fusion
(imf_vad.py:130-144) do not cancel.  Run once on CPU with the reference importable:

    python tests/golden/make_golden_precision.py

With synth.make_state_dict's own weights the log-variances lie in about [-2.8, 3.0]: eps / (w_i + w_e + eps) ~ 5e-9, the normalised
weights sum to one and `factor` divides out of every output -- the fwd_*_student8 / _student5 / _gauss fixtures pin the same numbers
to fp32 rounding.  Here the two log-variance biases are shifted (synth.shift_logvar_bias) until w_i + w_e is of the size of epsilon,
or epsilon is raised on the reference instance (`model.temporal.epsilon`, a plain attribute its forward reads, :142).

Reference outputs only -- weights and inputs are regenerated from the seeds by tests/helpers.load_precision_case:
  prec_k3_student8 / prec_k3_student1 / prec_k3_gauss   shift (15.5, 17.0), B = 2, L = 2, K = 3, ONE set of weights and inputs
  prec_k0_student5_eps                                  no shift, K = 0 (`fused` is z0 itself), epsilon = 1e-2
  prec_vitb_k3_student8                                 the D = 512 model, shifted
Each file holds what a fwd_*.npz holds (logits, the w row means, ROW_SUBSET rows of the seven wide outputs, meta) and
  shift [2], epsilon, dim
  floor_big / floor_logit / floor_sigmoid   the reference's fp32 run against its own .double() copy (make_golden.sharp_fields' fields)
  formula_floor    the largest relative error of the literal fp32 evaluation (torch, CPU) of the four formula lines against their fp64
                   evaluation, both on the fixture's own fp32 head tensors (the stored rows): |n32 - n64| / n64 for the two weights,
                   |z32 - z64| / (|n_i mu_i| + |n_e mu_e|) for z0 (the sum may cancel; its terms are what the roundings scale with)
  one_minus_sum    median of 1 - (w_i + w_e) over the stored rows (fp64 run): how far the regime is from "the weights sum to one"
The files are named prec_* so that tests/helpers.golden_cases() (fwd_*.npz) does not enrol them in the existing parametrised tests.
The second chunk has rows 100.. zeroed (a padded tail)."""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import BIG_KEYS, REF, ROW_SUBSET, ref_args  # noqa: E402
from iefvad_amd import synth  # noqa: E402

SHIFT = (15.5, 17.0)
B, L, LAM, TAIL = 2, 2, 0.5, 100
# (name, D, weight seed, input seed, K, noise, nu, shift, epsilon)
CASES = [
    ("k3_student8", 768, 11, 12, 3, "StudentT", 8, SHIFT, 1e-8),
    ("k3_student1", 768, 11, 12, 3, "StudentT", 1, SHIFT, 1e-8),
    ("k3_gauss", 768, 11, 12, 3, "Gaussian", 8, SHIFT, 1e-8),
    ("k0_student5_eps", 768, 11, 12, 0, "StudentT", 5, (0.0, 0.0), 1e-2),
    ("vitb_k3_student8", 512, 31, 41, 3, "StudentT", 8, SHIFT, 1e-8),
]


def case_inputs(iseed, D):
    img, ev = synth.make_inputs(iseed, B, D=D)
    img[B - 1, TAIL:] = 0
    ev[B - 1, TAIL:] = 0
    return img, ev


def build(D, wseed, K, noise, nu, shift, epsilon):
    sys.path.insert(0, REF)
    from model.imf_vad import MMFMIL  # the reference model
    model = MMFMIL(14, D, 256, D, 8, L, 8, 10, 10, device="cpu", args=ref_args(L, 8, K, LAM, noise, nu))
    sd = synth.shift_logvar_bias(synth.make_state_dict(wseed, D, L, K), *shift)
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.temporal.epsilon = epsilon      # read by the forward as a plain attribute (imf_vad.py:142); MMFMIL never forwards one (:30-38)
    return model.eval()


def formula_floor(heads, noise, nu, epsilon):
    """The literal four lines (imf_vad.py:130-144) in fp32 against fp64, both on the fp32 head tensors `heads` (numpy, any shape)."""
    precision = (nu + 1) / nu if noise == "StudentT" else 1.0

    def lines(dt):
        mu_i, lv_i, mu_e, lv_e = (torch.from_numpy(np.ascontiguousarray(heads[k])).to(dt)
                                  for k in ("image_mu", "image_logvar", "event_mu", "event_logvar"))
        w_i, w_e = precision * torch.exp(-lv_i), precision * torch.exp(-lv_e)      # a product by 1.0 (Gaussian) is exact
        den = w_i + w_e + epsilon
        n_i, n_e = w_i / den, w_e / den
        return n_i, n_e, n_i * mu_i + n_e * mu_e, (n_i * mu_i).abs() + (n_e * mu_e).abs()
    a, b = lines(torch.float32), lines(torch.float64)
    rel = [float(((a[j].double() - b[j]).abs() / b[j]).max()) for j in (0, 1)]
    rel.append(float(((a[2].double() - b[2]).abs() / b[3]).max()))
    return max(rel)


def main():
    sig = lambda t: torch.sigmoid(t.double())
    for name, D, wseed, iseed, K, noise, nu, shift, epsilon in CASES:
        model = build(D, wseed, K, noise, nu, shift, epsilon)
        img, ev = case_inputs(iseed, D)
        m64 = copy.deepcopy(model).double()
        assert m64.temporal.epsilon == epsilon
        with torch.no_grad():
            out = model(torch.from_numpy(img), torch.from_numpy(ev), None, None, None)
            o64 = m64.temporal(torch.from_numpy(img).double(), torch.from_numpy(ev).double())     # MMFMIL.forward narrows to fp32 (:41-42)
        lv_max = max(float(out[k].max()) for k in ("image_logvar", "event_logvar"))
        assert lv_max < 21.0, lv_max                                                              # exp(-logvar) far from underflow
        store = {"logits": out["logits"].numpy().reshape(B, 256),
                 "w_i_mean": out["w_i"].mean(dim=-1).numpy(), "w_e_mean": out["w_e"].mean(dim=-1).numpy(),
                 "rows": np.array(ROW_SUBSET), "meta": np.array([wseed, iseed, B, L, K, nu]), "lam": np.array(LAM),
                 "noise": np.array(noise), "in_dtype": np.array("f32"), "edit": np.array("tail"),
                 "dim": np.array(D), "shift": np.array(shift, np.float64), "epsilon": np.array(epsilon, np.float64),
                 "floor_big": np.array(max(float((out[k].double() - o64[k]).abs().max()) for k in BIG_KEYS)),
                 "floor_logit": np.array(float((out["logits"].double() - o64["logits"]).abs().max())),
                 "floor_sigmoid": np.array(float((sig(out["logits"]) - sig(o64["logits"])).abs().max()))}
        for k in BIG_KEYS:
            assert out[k].shape == (B, 256, D)
            store[k] = out[k].numpy()[:, ROW_SUBSET, :]
        store["formula_floor"] = np.array(formula_floor(store, noise, nu, epsilon))
        store["one_minus_sum"] = np.array(float((1 - (o64["w_i"] + o64["w_e"]))[:, ROW_SUBSET, :].median()))
        path = os.path.join(HERE, f"prec_{name}.npz")
        np.savez_compressed(path, **store)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB",
              {k: float(store[k]) for k in ("floor_big", "floor_logit", "floor_sigmoid", "formula_floor", "one_minus_sum")}, "max logvar", lv_max)


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
