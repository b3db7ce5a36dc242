"""Gradients of the input features, the part that needs no GPU: the C entry and its binding exist with the documented layout, bad
requests are refused by name before any device call, host tensors still get "no CPU fallback", and the reference fixtures
(tests/golden/grad_inputs_*.npz, written by tests/golden/make_golden_input_grads.py) are well-formed."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import lib as L
from tests import helpers as H

ENTRY = "iefvad_train_backward_inputs"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iefvad.h")
FIXTURES = ["k2_student8", "sharp_k2_student8", "k10_student8_mask"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        L.build_library()
    return L.load_library()


def test_the_entry_and_its_struct_exist_with_the_documented_layout(lib):
    assert ENTRY in L.SYMBOLS and hasattr(lib, ENTRY)
    old = lib.iefvad_train_backward.argtypes
    assert lib.iefvad_train_backward_inputs.restype is C.c_int
    assert lib.iefvad_train_backward_inputs.argtypes == old[:6] + [C.POINTER(L.InputGrads)] + old[6:] and len(old) == 7
    assert [n for n, _ in L.InputGrads._fields_] == ["img", "ev"] and C.sizeof(L.InputGrads) == 2 * C.sizeof(C.c_void_p)
    assert L.InputGrads.img.offset == 0 and L.InputGrads.ev.offset == C.sizeof(C.c_void_p)
    assert lib.iefvad_abi_version() == 8 and L.ABI_VERSION == 8          # an entry was added, no struct changed


def test_the_header_declares_the_entry():
    text = open(HEADER).read()
    assert ENTRY + "(" in text and "typedef struct iefvad_input_grads { float* img; float* ev; } iefvad_input_grads;" in text
    assert "#define IEFVAD_ABI_VERSION 8" in text


def test_bad_requests_are_refused_by_name_with_no_device(lib):
    """No handle exists without a GPU: a null handle is refused first; a non-null (never dereferenced) handle word then shows that a
    misaligned input-gradient buffer is refused before the handle is looked at -- hence before any HIP call."""
    fake, ok = C.c_void_p(0x10000), 0x10000
    dout, dw = L.OutputGrads(), L.WeightGrads()
    for h, dx, frag in [(None, L.InputGrads(ok, ok), "null handle"), (fake, L.InputGrads(ok + 4, None), "16-byte aligned"),
                        (fake, L.InputGrads(None, ok + 8), "16-byte aligned")]:
        rc = lib.iefvad_train_backward_inputs(h, 1, C.c_void_p(ok), 1 << 30, C.byref(dout), C.byref(dw), C.byref(dx), None)
        msg = L.last_error()
        assert rc != 0 and msg.startswith(ENTRY + ":") and frag in msg, (frag, msg)
    rc = lib.iefvad_train_backward(None, 1, C.c_void_p(ok), 1 << 30, C.byref(dout), C.byref(dw), None)
    assert rc != 0 and L.last_error().startswith("iefvad_train_backward: null handle")


@pytest.mark.parametrize("training", [True, False])
def test_host_features_that_require_grad_still_have_no_cpu_fallback(training):
    args = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=1, lambda_ref=0.5, noise_model="StudentT", nu=8)
    model = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, "cuda", args).train(training)
    x = torch.zeros(1, 256, 768, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(x, x.detach(), None, None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(x.detach(), x, None, None, None)


def test_the_differentiable_eval_route_names_the_extras_it_refuses():
    """Checked before anything is loaded or launched: host tensors suffice."""
    args = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=1, lambda_ref=0.5, noise_model="StudentT", nu=8)
    model = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, "cuda", args).eval()
    x = torch.zeros(1, 256, 768, requires_grad=True)
    for kw, frag in ((dict(timed=True), "timed=True"), (dict(row_scale=(torch.ones(256), None)), "row_scale="), (dict(attn_maps=[0]), "attn_maps=")):
        with pytest.raises(ValueError, match="differentiable eval route") as e:
            model(x, x, None, None, None, **kw)
        assert frag in str(e.value)
    with torch.no_grad():                                     # no graph is being built: the evaluation entry's own refusal
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model(x, x, None, None, None, timed=True)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_load_and_are_well_formed(name):
    g = np.load(os.path.join(H.GOLDEN, f"grad_inputs_{name}.npz"))
    par = np.load(os.path.join(H.GOLDEN, f"grad_{name}.npz"))
    assert (g["cfg"] == par["cfg"]).all() and float(g["total"]) == float(par["total"])      # the seeds and the loss of the parameter fixture
    B = int(g["cfg"][2])
    n = B * 256 * 768
    for key in ("img", "ev"):
        idx, val, norms = g[f"{key}_idx"], g[f"{key}_val"], g[f"{key}_norms"]
        assert idx.dtype == np.int64 and idx.shape == val.shape and 2000 <= idx.size <= 8192
        assert idx.min() >= 0 and idx.max() < n and (np.diff(idx) > 0).all()
        assert np.isfinite(val).all() and np.isfinite(norms).all() and norms.shape == (3,)
        l1, l2, mx = norms
        assert mx > 0 and l2 >= mx and l1 >= l2 and np.abs(val).max() <= mx
    floor = float(g["grad_floor"])
    assert np.isfinite(floor) and 0.0 < floor < 10.0
    for f in g.files:                                         # arrays and short strings only
        assert g[f].dtype.kind in "ifU" and (g[f].dtype.kind != "U" or g[f].size == 1), f
