"""D = 512 (the reference's `--ds vitb_rgb` model: ViT-B/16 features, 8 heads of 64) without a GPU: the CPU oracle reproduces the
reference captures of tests/golden/make_golden_vitb.py, which pins those fixtures for the GPU tests, and `iefvad_create_ex` -- the
create entry that also accepts D = 512 in the f32 arithmetic -- refuses every other configuration before it touches the device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from iefvad_amd import harness
from iefvad_amd import lib as L
from oracle import iefvad_oracle as orc
from tests import helpers as H
from tests import vitb_cases as V


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        L.build_library()
    return L.load_library()


@pytest.mark.parametrize("name", V.FWD_CASES)
def test_oracle_matches_the_reference_at_d512(name):
    g, cfg, sd, img, ev = V.load_case(name)
    out = orc.forward(sd, torch.from_numpy(img), torch.from_numpy(ev), H.oracle_cfg(cfg))
    out = {k: v.numpy() for k, v in out.items()}
    for k in H.BIG_KEYS:
        assert out[k].shape == (cfg["B"], 256, 512)
    H.compare_outputs(out, g)
    assert np.abs(out["w_i"].mean(-1) - g["w_i_mean"]).max() < 2e-6
    assert np.abs(out["w_e"].mean(-1) - g["w_e_mean"]).max() < 2e-6


def test_oracle_matches_the_reference_test_loop_scores_at_d512(tmp_path):
    """vitb_harness.npz: the reference's test() scores, per video from its zero-padded chunks (tools.py:100-114, test.py:119-121)."""
    g, args, gt, sd = V.write_harness_set(tmp_path)
    cfg = orc.OracleConfig(num_layers=2, num_refinement_steps=10, nu=8)
    scores = []
    for i, n in enumerate(g["lengths"]):
        img = np.load(str(tmp_path / "feat" / "rgb" / str(g["classes"][i]) / f"v{i:03d}__5.npy"))
        ev = np.load(str(tmp_path / "feat" / "event_thr_10" / str(g["classes"][i]) / f"v{i:03d}__5.npy"))
        ci, _ = harness.process_split(img, 256)
        ce, _ = harness.process_split(ev, 256)
        out = orc.forward(sd, torch.from_numpy(ci.reshape(-1, 256, 512)), torch.from_numpy(ce.reshape(-1, 256, 512)), cfg)
        scores.append(H.sigmoid(out["logits"].reshape(-1).numpy()[:int(n)]))
    scores = np.concatenate(scores)
    assert scores.shape == g["scores"].shape == (int(g["lengths"].sum()),)
    assert np.abs(scores - g["scores"]).max() <= H.TOL_SIGMOID


def test_create_ex_rejects_bad_configs_without_touching_the_gpu(lib):
    h = C.c_void_p()
    base = dict(abi_version=L.ABI_VERSION, embed_dim=512, seq_len=256, num_heads=8, num_layers=2, num_steps=10,
                noise_model=1, compute=L.COMPUTE_F32, lambda_ref=0.5, nu=8.0, epsilon=1e-8, micro_batch=0)
    bad_cases = [(dict(compute=L.COMPUTE_BF16), ("D=512", "f32")), (dict(compute=L.COMPUTE_BF16X6), ("D=512", "f32")),
                 (dict(compute=L.COMPUTE_FP16X3), ("D=512", "f32")), (dict(embed_dim=640), ("D=768", "D=640")),
                 (dict(num_heads=16), ("D=512", "H=16")), (dict(seq_len=128), ("D=512", "T=128")),
                 (dict(abi_version=9), ("abi_version",)), (dict(embed_dim=768, num_heads=12), ("D=768",)),
                 (dict(num_layers=0), ("num_layers",)), (dict(noise_model=7), ("Unsupported noise_model",))]
    for bad, frags in bad_cases:
        cfg = L.Config(**dict(base, **bad))
        assert lib.iefvad_create_ex(C.byref(cfg), C.byref(h)) != 0, bad
        for frag in frags:
            assert frag in L.last_error(), (bad, L.last_error())
        if "noise_model" not in bad:                # that message is the reference's own text (imf_vad.py:138)
            assert "iefvad_create_ex" in L.last_error()
        assert not h.value
    assert lib.iefvad_create_ex(None, C.byref(h)) != 0 and "null" in L.last_error()
    # the original entry keeps its contract: D = 512 is refused there, with the message it always gave
    cfg = L.Config(**base)
    assert lib.iefvad_create(C.byref(cfg), C.byref(h)) != 0 and "D=768" in L.last_error() and not h.value
