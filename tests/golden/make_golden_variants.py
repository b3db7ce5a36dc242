"""Reference capture of the fusion ablations.  Run once on CPU with the reference importable:

    python tests/golden/make_golden_variants.py

The reference forms `fused` inline (imf_vad.py:130-144), so a variant is captured from its own pieces: the four head tensors come out of
the reference's forward, the four substitutions are applied in torch exactly as imf_vad.py:130-144 writes the expression, and the
reference's own `temporal.refinement_blocks[i]` and `temporal.classifier` modules run on the result (:146-150):
  "fused"  no substitution          "image"  weight_event := 0          "event"  weight_image := 0          "equal"  both logvars := 0
One seeded K = 3 state dict (synth.make_state_dict, loaded strictly), once as StudentT nu = 8 and once as Gaussian, and the K = 0 model
(Identity, loop skipped) of the same weights.  Reference outputs only -- weights and inputs are regenerated from the seeds by the tests:
  variants_k3.npz   logits_variants_{studentt,gaussian,k0} [4, B, 256] fp32, and *_f64: the same run in fp64 (model.double().temporal)
                    floor_{...} [4]: the worst fp32-versus-fp64 difference per variant
                    sep_median_{...}, sep_min_{...} [4, 4]: median / smallest |difference| between two variants over all rows (fp64)
                    checksum: sum and sum of |.| over every weight, in state-dict order
The second chunk has rows 37.. zeroed (a padded tail).  The script asserts that the "fused" capture IS the reference's `logits`, bit for
bit, and that every pair of variants is separated by at least 3 x the loosest gate a test applies (1.5e-2, the bf16 logit gate), so that
no gate can hide a swapped or dropped substitution."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, ref_args  # noqa: E402
from iefvad_amd import synth  # noqa: E402

WSEED, ISEED, B, L, K, LAM, NU, TAIL = 52, 62, 2, 2, 3, 0.5, 8, 37
NAMES = ("fused", "image", "event", "equal")
LOOSEST_GATE = 1.5e-2      # TOL_LOGIT_BF16


def case_inputs():
    img, ev = synth.make_inputs(ISEED, B)
    img[B - 1, TAIL:] = 0
    ev[B - 1, TAIL:] = 0
    return img, ev


def build(sd, k, noise):
    sys.path.insert(0, REF)
    from model.imf_vad import MMFMIL  # the reference model
    model = MMFMIL(14, 768, 256, 768, 8, L, 8, 10, 10, device="cpu", args=ref_args(L, 8, k, LAM, noise, NU))
    keep = {n: v for n, v in sd.items() if k > 0 or "refinement_blocks" not in n.split(".")}
    res = model.load_state_dict(keep, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model.eval()


def variants_of(t, out):
    """The four variants from the head tensors of `out`, by the temporal module `t`'s own expression and modules."""
    rows = []
    for name in NAMES:
        image_mu, event_mu = out["image_mu"], out["event_mu"]
        image_logvar, event_logvar = out["image_logvar"], out["event_logvar"]
        if name == "equal":
            image_logvar, event_logvar = torch.zeros_like(image_logvar), torch.zeros_like(event_logvar)
        if t.noise_model == "Gaussian":
            weight_image = torch.exp(-image_logvar)
            weight_event = torch.exp(-event_logvar)
        else:
            factor = (t.nu + 1) / t.nu
            weight_image = factor * torch.exp(-image_logvar)
            weight_event = factor * torch.exp(-event_logvar)
        if name == "image":
            weight_event = torch.zeros_like(weight_event)
        if name == "event":
            weight_image = torch.zeros_like(weight_image)
        denom = weight_image + weight_event + t.epsilon
        norm_weight_image = weight_image / denom
        norm_weight_event = weight_event / denom
        fused = norm_weight_image * image_mu + norm_weight_event * event_mu
        fused_refined = fused
        for i in range(t.num_refinement_steps):
            residual = t.refinement_blocks[i](fused_refined)
            fused_refined = fused_refined - t.lambda_ref * residual
        rows.append(t.classifier(fused_refined).reshape(B, 256).numpy())
    return np.stack(rows)


def capture(sd, k, noise, img, ev):
    model = build(sd, k, noise)
    with torch.no_grad():
        out = model(img, ev, None, None, None)
        v32 = variants_of(model.temporal, out)
        assert np.array_equal(v32[0], out["logits"].reshape(B, 256).numpy())      # "fused" IS the reference's forward, bit for bit
        m64 = model.double()
        out64 = m64.temporal(img.double(), ev.double())      # MMFMIL.forward itself narrows to fp32 (imf_vad.py:41-42)
        v64 = variants_of(m64.temporal, out64)
    diff = np.abs(v64[:, None] - v64[None, :]).reshape(4, 4, -1)
    return {"logits_variants": v32.astype(np.float32), "logits_variants_f64": v64,
            "floor": np.abs(v32 - v64).reshape(4, -1).max(axis=1), "sep_median": np.median(diff, axis=2), "sep_min": diff.min(axis=2)}


def main():
    sd = synth.make_state_dict(WSEED, 768, L, K)
    img, ev = (torch.from_numpy(a) for a in case_inputs())
    store = {"meta": np.array([WSEED, ISEED, B, L, K, NU]), "lam": np.array(LAM), "tail": np.array(TAIL), "names": np.array(NAMES),
             "checksum": np.array([sum(float(v.double().sum()) for v in sd.values()), sum(float(v.double().abs().sum()) for v in sd.values())])}
    for tag, k, noise in (("studentt", K, "StudentT"), ("gaussian", K, "Gaussian"), ("k0", 0, "StudentT")):
        c = capture(sd, k, noise, img, ev)
        for key, v in c.items():
            store[key.replace("logits_variants", "logits_variants_" + tag) if key.startswith("logits") else key + "_" + tag] = v
        off = c["sep_median"][~np.eye(4, dtype=bool)]
        print(tag, "floor", c["floor"], "smallest pairwise median separation", off.min(), "smallest single-row separation",
              c["sep_min"][~np.eye(4, dtype=bool)].min())
        assert off.min() >= 3 * LOOSEST_GATE, (tag, off.min())
    path = os.path.join(HERE, "variants_k3.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
