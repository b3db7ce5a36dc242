"""Reference capture of the refinement trajectory.  Run once on CPU with the reference importable:

    python tests/golden/make_golden_trajectory.py

The reference fixes its step count at construction, so its own definition of "the score after k of K steps" is the model built with
num_refinement_steps = k that loads the first k refinement blocks of the K-step state dict (strict=True; at k = K it is the full model).
This script builds those K + 1 models of one seeded K = 5 state dict (synth.make_state_dict, loaded strictly) and writes reference
outputs only -- weights and inputs are regenerated from the seeds by the tests:
  trajectory_k5.npz   logits_steps [K + 1, B, 256] fp32: `logits` of the reference built with K = k, k = 0 .. K
                      delta_norm   [K, B, 256] fp64: ||fused(K = k + 1) - fused(K = k)||_2 of the same models run in fp64
                      floor_logit, floor_delta, floor_delta_rel: the reference's own fp32-versus-fp64 distance of both quantities
                      delta_range, z_norm: min / max of the update norms and the mean ||z_K|| (nothing is near zero)
                      checksum: sum and sum of |.| over every weight, in state-dict order
The second chunk has rows 37.. zeroed (a padded tail).  The file is named trajectory_* so that tests/helpers.golden_cases() (fwd_*.npz)
does not pick it up."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, ref_args  # noqa: E402
from iefvad_amd import synth  # noqa: E402

WSEED, ISEED, B, L, K, LAM, NOISE, NU, TAIL = 51, 61, 2, 2, 5, 0.5, "StudentT", 8, 37


def truncated(sd, k):
    """The state dict of the first k refinement blocks (every other tensor as it is)."""
    def keep(name):
        parts = name.split(".")
        return "refinement_blocks" not in parts or int(parts[parts.index("refinement_blocks") + 1]) < k
    return {n: v for n, v in sd.items() if keep(n)}


def case_inputs():
    img, ev = synth.make_inputs(ISEED, B)
    img[B - 1, TAIL:] = 0
    ev[B - 1, TAIL:] = 0
    return img, ev


def build(sd, k):
    sys.path.insert(0, REF)
    from model.imf_vad import MMFMIL  # the reference model
    model = MMFMIL(14, 768, 256, 768, 8, L, 8, 10, 10, device="cpu", args=ref_args(L, 8, k, LAM, NOISE, NU))
    res = model.load_state_dict(truncated(sd, k), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model.eval()


def main():
    sd = synth.make_state_dict(WSEED, 768, L, K)
    img, ev = (torch.from_numpy(a) for a in case_inputs())
    lg32, lg64, z32, z64 = [], [], [], []
    with torch.no_grad():
        for k in range(K + 1):
            model = build(sd, k)
            out = model(img, ev, None, None, None)
            lg32.append(out["logits"].reshape(B, 256).numpy())
            z32.append(out["fused"].double().numpy())
            out = model.double().temporal(img.double(), ev.double())      # MMFMIL.forward itself narrows to fp32 (imf_vad.py:41-42)
            lg64.append(out["logits"].reshape(B, 256).numpy())
            z64.append(out["fused"].numpy())
        full = build(sd, K)
        full.load_state_dict(sd, strict=True)
        whole = full(img, ev, None, None, None)
    assert np.array_equal(whole["logits"].reshape(B, 256).numpy(), lg32[K])      # k = K is the full model, bit for bit
    lg32, lg64 = np.stack(lg32), np.stack(lg64)
    d32 = np.stack([np.linalg.norm(z32[k + 1] - z32[k], axis=-1) for k in range(K)])
    d64 = np.stack([np.linalg.norm(z64[k + 1] - z64[k], axis=-1) for k in range(K)])
    store = {"logits_steps": lg32.astype(np.float32), "delta_norm": d64,
             "floor_logit": np.array(np.abs(lg32 - lg64).max()), "floor_delta": np.array(np.abs(d32 - d64).max()),
             "floor_delta_rel": np.array((np.abs(d32 - d64) / d64).max()), "delta_range": np.array([d64.min(), d64.max()]),
             "z_norm": np.array(np.linalg.norm(z64[K], axis=-1).mean()),
             "meta": np.array([WSEED, ISEED, B, L, K, NU]), "lam": np.array(LAM), "noise": np.array(NOISE), "tail": np.array(TAIL),
             "checksum": np.array([sum(float(v.double().sum()) for v in sd.values()), sum(float(v.double().abs().sum()) for v in sd.values())])}
    path = os.path.join(HERE, "trajectory_k5.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    for k in ("floor_logit", "floor_delta", "floor_delta_rel", "delta_range", "z_norm"):
        print(k, store[k])


if __name__ == "__main__":
    main()
