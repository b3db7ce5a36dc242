"""Reference capture of the score samples.  Run once on CPU with the reference importable:

    python tests/golden/make_golden_samples.py

The reference never samples (imf_vad.py:130-144 collapses each head's Gaussian to its mean), so a sample is captured from the reference's
own pieces, as make_golden_variants.py captures an ablation: the four head tensors come out of the reference's forward, the standard
normals come from `harness.gaussian_rows(harness.sample_seed(SEED, s), m, ids, D)` (the host model of the library's generator; ids =
b * 256 + t), the sampled means
    mu~_m = mu_m + eps_m * (scale * exp(0.5 * logvar_m) / sqrt(factor))
and the fusion are written in torch exactly as imf_vad.py:130-144 writes the expression, with the call's own weights, and the reference's
own `temporal.refinement_blocks[i]` and `temporal.classifier` modules run on the result (:146-150), in fp32 and in fp64.
The weights, inputs and tags are make_golden_variants.py's: one seeded K = 3 state dict as StudentT nu = 8 and as Gaussian, and the K = 0
model, B = 2 with the padded tail; S = 4, scale = 1, one seed.  Reference outputs and metadata only:
  samples_k3.npz    logits_samples_{studentt,gaussian,k0} [4, B, 256] fp32, and *_f64: the same run in fp64
                    floor_{...}: the worst fp32-versus-fp64 difference
                    eps_floor_{...}: the worst change of an fp64 sample logit when every eps is multiplied by 1 + 2^-22 -- twice the
                        measured device-versus-host difference of the generator (profiles/perturb_tests.log) relative to |eps| >= 4
                    amp_{...}: largest |z0_s| over largest |z0| (the bf16 gate scales with the operand's magnitude)
                    sep_median_{...}, sep_min_{...} [4, 4]: median / smallest |difference| between two samples over all rows (fp64)
                    meta, lam, tail, seed, scale, checksum (sum and sum of |.| over every weight, in state-dict order)
The script asserts that any two samples are at least 3 x 1.5e-2 (the bf16 logit gate) apart in the median, so that no gate can hide a
reused or dropped draw -- the seeded regime gives that as it stands (no synth.shift_logvar_bias is applied) -- and that with scale = 0
its own expression reproduces the reference's `logits` within `floor`."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_variants import B, K, L, LAM, NU, TAIL, WSEED, ISEED, LOOSEST_GATE, build, case_inputs  # noqa: E402
from iefvad_amd import harness, synth  # noqa: E402

S, SEED, SCALE = 4, 20261020, 1.0


def normals(s, dtype, scale_eps=1.0):
    ids = np.arange(B * 256)
    return [torch.from_numpy(harness.gaussian_rows(harness.sample_seed(SEED, s), m, ids, 768)).reshape(B, 256, 768).to(dtype) * scale_eps
            for m in (0, 1)]


def samples_of(t, out, dtype, scale=SCALE, scale_eps=1.0):
    """([S, B, 256] logits, largest |z0_s|) from the head tensors of `out`, by the temporal module `t`'s own expression and modules."""
    rows, zmax = [], 0.0
    image_logvar, event_logvar = out["image_logvar"], out["event_logvar"]
    if t.noise_model == "Gaussian":
        factor = 1.0
        weight_image = torch.exp(-image_logvar)
        weight_event = torch.exp(-event_logvar)
    else:
        factor = (t.nu + 1) / t.nu
        weight_image = factor * torch.exp(-image_logvar)
        weight_event = factor * torch.exp(-event_logvar)
    denom = weight_image + weight_event + t.epsilon
    norm_weight_image = weight_image / denom
    norm_weight_event = weight_event / denom
    for s in range(S):
        eps_i, eps_e = normals(s, dtype, scale_eps)
        image_mu = out["image_mu"] + eps_i * (scale * torch.exp(0.5 * image_logvar) / factor ** 0.5)
        event_mu = out["event_mu"] + eps_e * (scale * torch.exp(0.5 * event_logvar) / factor ** 0.5)
        fused = norm_weight_image * image_mu + norm_weight_event * event_mu
        zmax = max(zmax, float(fused.abs().max()))
        fused_refined = fused
        for i in range(t.num_refinement_steps):
            residual = t.refinement_blocks[i](fused_refined)
            fused_refined = fused_refined - t.lambda_ref * residual
        rows.append(t.classifier(fused_refined).reshape(B, 256).numpy())
    return np.stack(rows), zmax


def capture(sd, k, noise, img, ev):
    model = build(sd, k, noise)
    with torch.no_grad():
        out = model(img, ev, None, None, None)
        v32, _ = samples_of(model.temporal, out, torch.float32)
        z32, _ = samples_of(model.temporal, out, torch.float32, scale=0.0)
        ref_logits = out["logits"].reshape(B, 256).numpy()
        m64 = model.double()
        out64 = m64.temporal(img.double(), ev.double())      # MMFMIL.forward itself narrows to fp32 (imf_vad.py:41-42)
        v64, zmax = samples_of(m64.temporal, out64, torch.float64)
        p64, _ = samples_of(m64.temporal, out64, torch.float64, scale_eps=1.0 + 2.0 ** -22)
        z0max = float(out64["fused"].abs().max())
    floor = float(np.abs(v32 - v64).max())
    assert float(np.abs(z32 - ref_logits[None]).max()) <= floor, (float(np.abs(z32 - ref_logits[None]).max()), floor)   # scale = 0 IS the forward
    diff = np.abs(v64[:, None] - v64[None, :]).reshape(S, S, -1)
    return {"logits_samples": v32.astype(np.float32), "logits_samples_f64": v64, "floor": np.array(floor),
            "eps_floor": np.array(float(np.abs(p64 - v64).max())), "amp": np.array(zmax / z0max),
            "sep_median": np.median(diff, axis=2), "sep_min": diff.min(axis=2)}


def main():
    sd = synth.make_state_dict(WSEED, 768, L, K)
    img, ev = (torch.from_numpy(a) for a in case_inputs())
    store = {"meta": np.array([WSEED, ISEED, B, L, K, NU]), "lam": np.array(LAM), "tail": np.array(TAIL), "seed": np.array(SEED),
             "scale": np.array(SCALE), "samples": np.array(S),
             "checksum": np.array([sum(float(v.double().sum()) for v in sd.values()), sum(float(v.double().abs().sum()) for v in sd.values())])}
    for tag, k, noise in (("studentt", K, "StudentT"), ("gaussian", K, "Gaussian"), ("k0", 0, "StudentT")):
        c = capture(sd, k, noise, img, ev)
        for key, v in c.items():
            store[key.replace("logits_samples", "logits_samples_" + tag) if key.startswith("logits") else key + "_" + tag] = v
        off = c["sep_median"][~np.eye(S, dtype=bool)]
        print(tag, "floor", c["floor"], "eps_floor", c["eps_floor"], "amp", c["amp"], "smallest pairwise median separation", off.min(),
              "smallest single-row separation", c["sep_min"][~np.eye(S, dtype=bool)].min())
        assert off.min() >= 3 * LOOSEST_GATE, (tag, off.min())
    path = os.path.join(HERE, "samples_k3.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
