"""Cases shared by tests/test_attn_maps_cpu.py and tests/test_gpu_attn_maps.py: the reference captures of
tests/golden/make_golden_attn.py (attn_*.npz, vitb_attn_*.npz) with their weights and inputs regenerated from the stored seeds, and a
torch-only restatement of the encoder layers that returns the head-averaged attention maps -- the expected values for shapes the
fixtures do not hold."""
import argparse
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from iefvad_amd import synth
from tests import helpers as H

FIXTURES = ["attn_flat_k3", "attn_sharp_k3", "vitb_attn_sharp_k3"]
SHARP = [n for n in FIXTURES if "sharp" in n]
MODALITIES = ("image", "event")
T, HEADS = 256, 8
VALID_LAST = 100          # rows 100.. of the fixtures' last chunk are zero


def encoder_maps(sd, img, ev, L, dtype=torch.float64):
    """The temporal encoder of imf_vad.py:113-123 in `dtype`: per layer nn.MultiheadAttention's functional form with need_weights=True
    (head-averaged weights), residual, LayerNorm.  `img`, `ev`: [B, T, D] tensors.  Returns {(modality index, layer): [B, T, T]}."""
    out = {}
    for m, (name, x) in enumerate(zip(MODALITIES, (img, ev))):
        x = x.to(dtype)
        D = x.shape[-1]
        for l in range(L):
            w = {k: sd[f"temporal.{name}_attn_layers.{l}.{k}"].to(dtype) for k in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")}
            xt = x.transpose(0, 1)                     # [T, B, D]: the functional form is sequence-first
            att, wts = F.multi_head_attention_forward(xt, xt, xt, D, HEADS, w["in_proj_weight"], w["in_proj_bias"], None, None, False, 0.0,
                                                      w["out_proj.weight"], w["out_proj.bias"], training=False, need_weights=True,
                                                      average_attn_weights=True)
            out[(m, l)] = wts
            x = F.layer_norm(x + att.transpose(0, 1), (D,), sd[f"temporal.{name}_norms.{l}.weight"].to(dtype),
                             sd[f"temporal.{name}_norms.{l}.bias"].to(dtype), 1e-5)
    return out


@functools.lru_cache(maxsize=None)
def load_fixture(name):
    """(capture, cfg, state_dict, img, ev) of tests/golden/<name>.npz."""
    g = np.load(os.path.join(H.GOLDEN, name + ".npz"))
    wseed, iseed, B, L, K, D = (int(v) for v in g["meta"])
    sd = synth.make_state_dict(wseed, D, L, K)
    if "factors" in g.files:
        sd = synth.sharpen_qk(sd, tuple(float(f) for f in g["factors"]))
    img, ev = synth.make_inputs(iseed, B, D=D)
    img[B - 1, VALID_LAST:] = 0
    ev[B - 1, VALID_LAST:] = 0
    return g, dict(B=B, L=L, K=K, D=D, wseed=wseed, iseed=iseed), sd, img, ev


def model_args(L, K):
    return argparse.Namespace(visual_layers=L, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)


def fixture_rows(g, maps, m, l):
    """The fixture's query rows of a full [B, T, T] map -> [B, 16, T]."""
    rows = g["rows"]
    return np.stack([np.asarray(maps[b])[rows[b]] for b in range(rows.shape[0])])
