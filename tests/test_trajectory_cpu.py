"""The refinement trajectory and the call-time step count without a GPU: the C declarations and exported symbols, the refusals of the
entries and of the Python keywords (all before a device is touched), and the committed reference capture
(tests/golden/trajectory_k5.npz, make_golden_trajectory.py) against the CPU oracle run with the truncated state dict and K = k."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth
from iefvad_amd import lib as L
from oracle import iefvad_oracle as orc
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("iefvad_set_steps", "iefvad_forward_trajectory", "iefvad_forward_videos_trajectory")
# ||z_{k+1} - z_k|| against the reference's fp64 value: two states, each within the 768-d output gate (2e-5) per element, so the
# difference vector is off by at most 2 x 2e-5 per element and its norm by at most 2 x 2e-5 x sqrt(768) = 1.1e-3 (the derivation of the
# distance cap of the similarity series)
TOL_DELTA = 2 * H.TOL_BIG * np.sqrt(768.0)


def truncated(sd, k):
    """The first k refinement blocks of a state dict, everything else as it is (what tests/golden/make_golden_trajectory.py loads)."""
    def keep(name):
        parts = name.split(".")
        return "refinement_blocks" not in parts or int(parts[parts.index("refinement_blocks") + 1]) < k
    return {n: v for n, v in sd.items() if keep(n)}


def load_trajectory_case(golden_dir):
    g = np.load(os.path.join(golden_dir, "trajectory_k5.npz"))
    wseed, iseed, B, L_, K, nu = (int(v) for v in g["meta"])
    sd = synth.make_state_dict(wseed, 768, L_, K)
    chk = np.array([sum(float(v.double().sum()) for v in sd.values()), sum(float(v.double().abs().sum()) for v in sd.values())])
    assert np.allclose(chk, g["checksum"], rtol=1e-12, atol=1e-9)      # the weights the reference ran with
    img, ev = synth.make_inputs(iseed, B)
    img[B - 1, int(g["tail"]):] = 0
    ev[B - 1, int(g["tail"]):] = 0
    cfg = dict(L=L_, K=K, nu=nu, lam=float(g["lam"]), noise=str(g["noise"]), B=B)
    return g, cfg, sd, img, ev


def cpu_model(K=3, **kw):
    args = argparse.Namespace(visual_layers=1, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    return iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 1, 8, 10, 10, "cpu", args, **kw).eval()


def test_header_declares_the_entries_and_keeps_the_abi():
    header = open(os.path.join(ROOT, "include", "iefvad.h")).read()
    assert "#define IEFVAD_ABI_VERSION 8" in header
    assert "int iefvad_set_steps(iefvad_handle* h, int32_t steps);" in header
    assert "typedef struct iefvad_trajectory { float* logits_steps; float* delta_norm; size_t stride; } iefvad_trajectory;" in header
    assert "int iefvad_forward_trajectory(iefvad_handle* h," in header and "int iefvad_forward_videos_trajectory(iefvad_handle* h," in header
    assert "size_t iefvad_trajectory_workspace_bytes(" in header and "size_t iefvad_videos_trajectory_workspace_bytes(" in header
    lib = L.load_library()
    assert lib.iefvad_abi_version() == 8 and L.ABI_VERSION == 8


def test_library_exports_the_symbols():
    lib = L.load_library()
    for s in ENTRIES + ("iefvad_trajectory_workspace_bytes", "iefvad_videos_trajectory_workspace_bytes"):
        assert s in L.SYMBOLS and hasattr(lib, s), s
    assert lib.iefvad_set_steps.restype is C.c_int and lib.iefvad_forward_trajectory.restype is C.c_int
    assert C.sizeof(L.Trajectory) == 2 * C.sizeof(C.c_void_p) + C.sizeof(C.c_size_t)


def test_null_arguments_are_refused_by_name():
    lib = L.load_library()
    assert lib.iefvad_set_steps(None, 1) != 0
    assert L.last_error().startswith("iefvad_set_steps:") and "null" in L.last_error()
    t = L.Trajectory(None, None, 256)
    o = L.Outputs()
    lens = (C.c_int32 * 1)(5)
    assert lib.iefvad_forward_trajectory(None, None, None, 0, 1, None, 0, C.byref(o), C.byref(t), None) != 0
    assert L.last_error().startswith("iefvad_forward_trajectory:") and "null" in L.last_error()
    assert lib.iefvad_forward_videos_trajectory(None, None, None, 0, lens, 1, 1, None, 0, None, None, None, C.byref(t), None) != 0
    assert L.last_error().startswith("iefvad_forward_videos_trajectory:") and "null" in L.last_error()
    assert lib.iefvad_trajectory_workspace_bytes(None, 1) == 0 and lib.iefvad_videos_trajectory_workspace_bytes(None, lens, 1) == 0


def test_set_steps_range_in_python():
    m = cpu_model(K=3)
    assert m.steps == 3
    for bad in (-1, 4, 1.5, True, "2"):
        with pytest.raises(ValueError, match="set_steps"):
            m.set_steps(bad)
    m.set_steps(2)
    assert m.steps == 2
    assert [c.steps for c in m.lanes(2)] == [2, 2]
    m.set_steps(0)
    assert [c.steps for c in m.lanes(2)] == [0, 0]
    m.set_steps(None)
    assert m.steps == 3


def test_trajectory_refusals_come_before_a_device_is_touched():
    """Host tensors throughout: a call that got as far as the device check would raise RuntimeError ("runs on a HIP device only")."""
    m = cpu_model()
    x = torch.zeros(1, 256, 768)
    v = torch.zeros(256)
    for kw, word in ((dict(timed=True), "timed"), (dict(attn_maps=True), "attn_maps"), (dict(row_scale=(v, None)), "row_scale"),
                     (dict(row_noise=(v, None), noise_seed=1), "row_noise")):
        with pytest.raises(ValueError, match="trajectory=True does not combine with " + word):
            m(x, x, None, None, None, trajectory=True, **kw)
    with pytest.raises(ValueError, match="require grad"):
        m(x.clone().requires_grad_(True), x, None, None, None, trajectory=True)
    rows = torch.zeros(5, 768)
    for kw, word in ((dict(attn_maps=[0]), "attn_maps"), (dict(row_scale=(None, v[:5])), "row_scale"), (dict(row_noise=(v[:5], None), noise_seed=1), "row_noise"),
                     (dict(similarity=True), "similarity"), (dict(outputs="full"), "outputs="), (dict(weight_sums=True), "weight_sums"),
                     (dict(nan_to_num="always"), "nan_to_num='always'")):
        with pytest.raises(ValueError, match="trajectory=True does not combine with " + word):
            m.forward_videos(rows, rows, [5], trajectory=True, **kw)
    m.train()
    with pytest.raises(RuntimeError, match="model.train()"):
        m(x, x, None, None, None, trajectory=True)
    with pytest.raises(RuntimeError, match="model.train()"):
        m.forward_videos(rows, rows, [5], trajectory=True)
    m.eval()
    assert "trajectory" not in m.forward_videos_host.__code__.co_varnames       # the host-list entry does not take it


def test_harness_refusals():
    m = cpu_model()
    with pytest.raises(ValueError, match="HIP device"):
        harness.score_loader(m, [], 256, "cpu", trajectory=True)
    with pytest.raises(ValueError, match="set_steps"):
        harness.score_loader(lambda *a: None, [], 256, "cpu", steps=1)
    with pytest.raises(ValueError, match="similarity"):
        harness.score_loader(m, [], 256, "cuda", trajectory=True, similarity=True)
    with pytest.raises(ValueError, match="host_list"):      # the default walk of a packed evaluation is the host list
        harness.score_loader(m, [], 256, "cuda", batch_chunks=8, trajectory=True)
    # the step count is set for the walk and restored behind it
    m.set_steps(2)
    harness.score_loader(m, [], 256, "cpu", steps=1)
    assert m.steps == 2


def test_oracle_reproduces_the_reference_trajectory(golden_dir):
    """The reference built with K = k on the first k blocks (the golden) against the oracle run the same way: logits within the
    oracle-vs-reference gate of tests/test_oracle_golden.py, the update norms within TOL_DELTA of the reference's fp64 values."""
    g, cfg, sd, img, ev = load_trajectory_case(golden_dir)
    K = cfg["K"]
    assert g["logits_steps"].shape == (K + 1, cfg["B"], 256) and g["delta_norm"].shape == (K, cfg["B"], 256)
    assert float(g["delta_range"][0]) > 1.0 and float(g["floor_delta_rel"]) < 1e-6      # nothing near zero; the reference's own fp32 floor
    tol_logit = max(H.TOL_LOGIT, 3.0 * float(g["floor_logit"]))
    ti, te = torch.from_numpy(img), torch.from_numpy(ev)
    fused = []
    for k in range(K + 1):
        c = dict(cfg, K=k)
        out = orc.forward(truncated(sd, k), ti, te, H.oracle_cfg(c))
        err = float(np.abs(out["logits"].numpy().reshape(cfg["B"], 256) - g["logits_steps"][k]).max())
        assert err <= tol_logit, (k, err)
        fused.append(out["fused"].double().numpy())
    for k in range(K):
        d = np.linalg.norm(fused[k + 1] - fused[k], axis=-1)
        err = float(np.abs(d - g["delta_norm"][k]).max())
        assert err <= TOL_DELTA, (k, err)
