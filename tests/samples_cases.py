"""What the score-sample tests share: the fixture's case (tests/golden/samples_k3.npz, make_golden_samples.py), regenerated from its
seeds, and the tail of the CPU oracle -- its refinement loop and classifier (oracle/iefvad_oracle.py:107-112) -- restated on a given
fused state, so that `harness.sample_states_host` can be followed to logits without a GPU."""
import os

import numpy as np
import torch

from iefvad_amd import harness, synth
from tests.variants_cases import EPSILON, TOL_LOGIT_BF16, without_refinement  # noqa: F401

TAGS = (("studentt", "StudentT", 3), ("gaussian", "Gaussian", 3), ("k0", "StudentT", 0))


def load_samples_case(golden_dir):
    """The fixture, and the weights / inputs it was captured with, regenerated from its seeds (checksum checked)."""
    g = np.load(os.path.join(golden_dir, "samples_k3.npz"))
    wseed, iseed, B, L, K, nu = (int(v) for v in g["meta"])
    sd = synth.make_state_dict(wseed, 768, L, K)
    chk = np.array([sum(float(v.double().sum()) for v in sd.values()), sum(float(v.double().abs().sum()) for v in sd.values())])
    assert np.allclose(chk, g["checksum"], rtol=1e-12, atol=1e-9)      # the weights the reference ran with
    img, ev = synth.make_inputs(iseed, B)
    img[B - 1, int(g["tail"]):] = 0
    ev[B - 1, int(g["tail"]):] = 0
    cfg = dict(L=L, K=K, nu=nu, lam=float(g["lam"]), B=B, S=int(g["samples"]), seed=int(g["seed"]), scale=float(g["scale"]))
    return g, cfg, sd, img, ev


def factor_of(noise, nu):
    return (nu + 1) / nu if noise == "StudentT" else 1.0


def tail_logits(sd, z, *, K, lam=0.5, dtype=torch.float64, prefix="temporal."):
    """The first K refinement blocks of `sd` and the classifier on the state `z` [..., D], in `dtype` -> [...] logits (numpy)."""
    z = torch.as_tensor(np.asarray(z)).to(dtype)
    w = lambda n: sd[prefix + n].to(dtype)      # noqa: E731
    for k in range(K):
        h = torch.relu(z @ w(f"refinement_blocks.{k}.0.weight").T + w(f"refinement_blocks.{k}.0.bias"))
        z = z - lam * (h @ w(f"refinement_blocks.{k}.2.weight").T + w(f"refinement_blocks.{k}.2.bias"))
    return (z @ w("classifier.weight").T + w("classifier.bias")).squeeze(-1).numpy()


def host_sample_logits(sd, heads, S, seed, ids, *, K, lam, noise, nu, scale=1.0):
    """[S, ...] fp64 logits of the host model: `harness.sample_states_host` on the four head tensors (image_mu, image_logvar, event_mu,
    event_logvar), then the oracle's tail."""
    mu_i, lv_i, mu_e, lv_e = heads
    return np.stack([tail_logits(sd, harness.sample_states_host(mu_i, lv_i, mu_e, lv_e, seed, s, ids, factor_of(noise, nu), EPSILON, scale),
                                 K=K, lam=lam) for s in range(S)])
