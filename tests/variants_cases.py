"""The fusion ablations restated in torch (fp64 by default): the four substitutions into the reference's literal fusion expression
(imf_vad.py:130-144), its refinement loop (:146-149) and classifier (:150), from a state dict and the four head tensors.  Used where
tests/golden/variants_k3.npz has no capture (another width, another step count), and to load that fixture's case."""
import os

import numpy as np
import torch

from iefvad_amd import synth

NAMES = ("fused", "image", "event", "equal")
EPSILON = 1e-8                      # MultiModal_Fusion_Attn_Iter's default epsilon (imf_vad.py:58)
TOL_LOGIT_BF16 = 1.5e-2             # the bf16 arithmetic's logit gate (tests/test_gpu_bf16.py)
TOL_SIGMOID_BF16 = 4e-3


def fuse_variant(name, mu_i, lv_i, mu_e, lv_e, noise="StudentT", nu=8, eps=EPSILON):
    """z0 of one variant: the reference's expression with the variant's substitution, operation for operation."""
    if name not in NAMES:
        raise ValueError(name)
    if name == "equal":
        lv_i, lv_e = torch.zeros_like(lv_i), torch.zeros_like(lv_e)
    factor = (nu + 1) / nu if noise == "StudentT" else 1.0
    w_i = factor * torch.exp(-lv_i)
    w_e = factor * torch.exp(-lv_e)
    if name == "image":
        w_e = torch.zeros_like(w_e)
    if name == "event":
        w_i = torch.zeros_like(w_i)
    den = w_i + w_e + eps
    return (w_i / den) * mu_i + (w_e / den) * mu_e


def variant_logits(sd, mu_i, lv_i, mu_e, lv_e, names=NAMES, *, K, lam=0.5, noise="StudentT", nu=8, dtype=torch.float64, prefix="temporal."):
    """[V, ...] logits of the named variants: substitution, the first K refinement blocks of `sd`, the classifier, all in `dtype`."""
    t = [torch.as_tensor(np.asarray(a)).to(dtype) for a in (mu_i, lv_i, mu_e, lv_e)]
    w = lambda n: sd[prefix + n].to(dtype)      # noqa: E731
    out = []
    for name in names:
        z = fuse_variant(name, *t, noise=noise, nu=nu)
        for k in range(K):
            h = torch.relu(z @ w(f"refinement_blocks.{k}.0.weight").T + w(f"refinement_blocks.{k}.0.bias"))
            z = z - lam * (h @ w(f"refinement_blocks.{k}.2.weight").T + w(f"refinement_blocks.{k}.2.bias"))
        out.append((z @ w("classifier.weight").T + w("classifier.bias")).squeeze(-1))
    return torch.stack(out).numpy()


def load_variants_case(golden_dir):
    """The fixture, and the weights / inputs it was captured with, regenerated from its seeds (checksum checked)."""
    g = np.load(os.path.join(golden_dir, "variants_k3.npz"))
    wseed, iseed, B, L, K, nu = (int(v) for v in g["meta"])
    sd = synth.make_state_dict(wseed, 768, L, K)
    chk = np.array([sum(float(v.double().sum()) for v in sd.values()), sum(float(v.double().abs().sum()) for v in sd.values())])
    assert np.allclose(chk, g["checksum"], rtol=1e-12, atol=1e-9)      # the weights the reference ran with
    img, ev = synth.make_inputs(iseed, B)
    img[B - 1, int(g["tail"]):] = 0
    ev[B - 1, int(g["tail"]):] = 0
    cfg = dict(L=L, K=K, nu=nu, lam=float(g["lam"]), B=B)
    return g, cfg, sd, img, ev


def without_refinement(sd):
    """The state dict of the K = 0 model: every refinement block dropped (the reference's Identity has no parameters)."""
    return {n: v for n, v in sd.items() if "refinement_blocks" not in n.split(".")}
