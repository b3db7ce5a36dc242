"""Generate tests/golden/grad_inputs_<name>.npz: the gradients of the two INPUT feature tensors, by the REFERENCE itself.

Run once where the reference is mounted (the path `make_golden.py` names), from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_input_grads.py [case ...]

For the seeds and the loss of three of `make_golden.py`'s GRAD_CASES (k2_student8, sharp_k2_student8, k10_student8_mask) the
reference MMFMIL runs in train() mode as an fp64 copy, with `requires_grad` on both feature tensors; the loss is the trainers' total
(CLAS2 + regulariser + KL, train/ucf_train.py:73-102) with the reference's own CLAS2; k10_student8_mask gets its injected dropout mask
the way `gen_model_grad_cases` feeds it.  Stored per modality (`img`, `ev`): INPUT_SAMPLES seeded entries of the gradient (`idx` into the
flattened [B, 256, 768] tensor, `val`) and the L1 / L2 / max norms of the whole tensor; and `grad_floor`: the worst sampled entry of the
reference's OWN fp32 autograd against its fp64 gradient, in units of 1e-4 |want| + 1e-6 max|want| -- the field and the unit the
parameter fixtures record.  Arrays and short strings only; weights, inputs and masks are regenerated from their seeds by the tests.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (puts the repository root on sys.path; names the reference's path)
from iefvad_amd import synth  # noqa: E402

INPUT_GRAD_CASES = ("k2_student8", "sharp_k2_student8", "k10_student8_mask")
INPUT_SAMPLES = 4096
MODALITIES = ("img", "ev")


def _input_grads(case, dtype, CLAS2):
    """(d img, d ev, total) of one GRAD_CASES row with the reference model in `dtype`."""
    name, wseed, bseed, B, L, K, noise, nu, lam_reg, lam_kl, p, factors = case
    mask = synth.make_dropout_mask(bseed, L, B, p) if p > 0 else None
    model, inject = MG._reference_train_model(wseed, L, K, noise, nu, dtype, p, mask, factors)
    img, ev, labels, lengths = synth.make_train_batch(bseed, B)
    x = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (img, ev)]
    with inject():
        # one level below MMFMIL.forward (imf_vad.py:40-44 is `.to(torch.float)` + this call), so that an fp64 graph stays fp64
        out = model.temporal(x[0], x[1])
    total = MG._trainer_loss(out, torch.from_numpy(labels).to(dtype), torch.from_numpy(lengths), noise, nu, lam_reg, lam_kl, CLAS2)
    total.backward()
    return x[0].grad.double().numpy().reshape(-1), x[1].grad.double().numpy().reshape(-1), float(total.detach())


def gen_input_grad_cases(only=None):
    sys.path.insert(0, MG.REF)
    from train.loss import CLAS2
    for case in MG.GRAD_CASES:
        name, wseed, bseed, B, L, K, noise, nu, lam_reg, lam_kl, p, factors = case
        if name not in INPUT_GRAD_CASES or (only and name not in only):
            continue
        g64 = _input_grads(case, torch.float64, CLAS2)
        # the reference's own arithmetic, one thread so that the summation order -- and with it the floor -- reproduces
        threads = torch.get_num_threads()
        torch.set_num_threads(1)
        g32 = _input_grads(case, torch.float32, CLAS2)
        torch.set_num_threads(threads)
        store = {"cfg": np.array([wseed, bseed, B, L, K, nu]), "noise": np.array(noise), "lams": np.array([lam_reg, lam_kl]),
                 "p": np.array(p), "total": np.array(g64[2])}
        if factors is not None:
            store["factors"] = np.array(factors, np.float64)
        floor = 0.0
        for m, key in enumerate(MODALITIES):
            g = g64[m]
            rng = np.random.default_rng([bseed, 1900 + m])
            idx = np.sort(rng.choice(g.size, INPUT_SAMPLES, replace=False))
            mx = np.abs(g).max()
            store[f"{key}_idx"] = idx.astype(np.int64)
            store[f"{key}_val"] = g[idx]
            store[f"{key}_norms"] = np.array([np.abs(g).sum(), np.sqrt((g * g).sum()), mx])
            units = float((np.abs(g32[m][idx] - g[idx]) / (1e-4 * np.abs(g[idx]) + 1e-6 * mx)).max())
            print(name, key, "reference fp32 autograd vs fp64, worst sampled entry in gate units:", units)
            floor = max(floor, units)
        store["grad_floor"] = np.array(floor)
        path = os.path.join(HERE, f"grad_inputs_{name}.npz")
        np.savez_compressed(path, **store)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB; total", g64[2], "grad_floor", floor)


if __name__ == "__main__":
    gen_input_grad_cases(sys.argv[1:])
