"""The full output dict on the valid-row routes (`iefvad_videos_full_workspace_bytes`, `iefvad_forward_videos_full`,
`iefvad_forward_videos_host_full`; `MMFMIL.forward_videos(outputs=...)` / `forward_videos_host(outputs=...)`;
`harness.score_loader(row_outputs=...)`) -- what can be checked without a GPU: the three entries exist with the documented
signatures, refuse a null handle, a null `out` and a null `out->logits` by name before any HIP call, and the Python layers validate
their arguments before the library is loaded."""
import argparse
import ctypes as C
import os

import pytest
import torch

import iefvad_amd
from iefvad_amd import harness
from iefvad_amd import lib as L

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iefvad.h")
WS, ROWS, HOST = "iefvad_videos_full_workspace_bytes", "iefvad_forward_videos_full", "iefvad_forward_videos_host_full"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        L.build_library()
    return L.load_library()


def test_entries_exist_with_the_documented_signatures(lib):
    for s in (WS, ROWS, HOST):
        assert s in L.SYMBOLS and hasattr(lib, s)
    out_p = C.POINTER(L.Outputs)
    assert lib.iefvad_videos_full_workspace_bytes.restype is C.c_size_t
    assert lib.iefvad_videos_full_workspace_bytes.argtypes == lib.iefvad_videos_workspace_bytes.argtypes + [out_p]
    # the arguments of the plain entries with the three result pointers replaced by one `const iefvad_outputs*`
    plain, host = lib.iefvad_forward_videos.argtypes, lib.iefvad_forward_videos_host.argtypes
    assert lib.iefvad_forward_videos_full.restype is C.c_int and lib.iefvad_forward_videos_host_full.restype is C.c_int
    assert lib.iefvad_forward_videos_full.argtypes == plain[:9] + [out_p] + plain[12:] and len(plain) == 13
    assert lib.iefvad_forward_videos_host_full.argtypes == host[:10] + [out_p] + host[13:] and len(host) == 14
    assert lib.iefvad_abi_version() == 8 and L.ABI_VERSION == 8          # entries were added, no struct changed
    assert [n for n, _ in L.Outputs._fields_] == ["fused", "logits", "image_mu", "event_mu", "image_logvar", "event_logvar", "w_i", "w_e",
                                                  "w_i_mean", "w_e_mean"]


def test_the_header_declares_the_entries_and_their_limits():
    text = open(HEADER).read()
    for s in (WS, ROWS, HOST):
        assert s + "(" in text
    assert "#define IEFVAD_ABI_VERSION 8" in text
    assert "do not combine with iefvad_forward_videos_scaled" in text


OK = 0x10000                                                             # never read: every call below stops in its checks


def _out(logits=OK, **kw):
    o = L.Outputs()
    o.logits = logits
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _rows(lib, h=None, out=None, in_dtype=L.IN_F32, nvideos=2):
    lens = (C.c_int32 * 2)(5, 7)
    rc = lib.iefvad_forward_videos_full(h, C.c_void_p(OK), C.c_void_p(OK), in_dtype, lens, nvideos, 1, C.c_void_p(OK), 1 << 30,
                                        C.byref(out) if out is not None else None, None)
    return rc, L.last_error()


def _host(lib, h=None, out=None, in_dtype=L.IN_F32, nvideos=2):
    lens = (C.c_int32 * 2)(5, 7)
    ptrs = (C.c_void_p * 2)(0x10000, 0x20000)
    rc = lib.iefvad_forward_videos_host_full(h, ptrs, ptrs, in_dtype, in_dtype, lens, nvideos, 1, 64, 0,
                                             C.byref(out) if out is not None else None, None)
    return rc, L.last_error()


@pytest.mark.parametrize("call,name", [(_rows, ROWS), (_host, HOST)])
def test_null_arguments_are_refused_and_the_message_names_the_entry(lib, call, name):
    """No handle exists without a GPU: the null handle is refused first; a non-null (never dereferenced) handle word then shows that a
    null `out` and a null `out->logits` are refused before the handle is looked at -- hence before any HIP call."""
    fake = C.c_void_p(0x10000)
    for kw, frag in [(dict(h=None, out=_out()), "null handle"), (dict(h=fake, out=None), "null out"),
                     (dict(h=fake, out=_out(logits=None)), "null logits"), (dict(h=fake, out=_out(fused=OK + 4)), "16-byte aligned"),
                     (dict(h=fake, out=_out(w_e=OK + 8)), "16-byte aligned"), (dict(h=fake, out=_out(), in_dtype=7), "in_dtype"),
                     (dict(h=fake, out=_out(), nvideos=0), "nvideos")]:
        rc, msg = call(lib, **kw)
        assert rc != 0 and msg.startswith(name + ":") and frag in msg, (kw, msg)


def test_workspace_query_without_a_handle_is_zero(lib):
    lens = (C.c_int32 * 2)(5, 7)
    assert lib.iefvad_videos_full_workspace_bytes(None, lens, 2, C.byref(_out(w_i=OK))) == 0
    assert lib.iefvad_videos_full_workspace_bytes(None, lens, 2, None) == 0


def _model(**kw):
    args = argparse.Namespace(visual_layers=1, visual_head=8, num_refinement_steps=1, lambda_ref=0.5, noise_model="StudentT", nu=8)
    return iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 1, 8, 10, 10, "cuda", args, **kw).eval()


@pytest.fixture
def no_library(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "load_library", no_load)


def test_forward_videos_refuses_bad_outputs_by_cause(no_library):
    model = _model()
    rows = torch.zeros(12, 768)
    good = torch.ones(12)
    with pytest.raises(ValueError, match="unknown output key.*'scores'"):
        model.forward_videos(rows, rows, [5, 7], outputs=("image_logvar", "scores"))
    with pytest.raises(ValueError, match="unknown output key"):
        model.forward_videos(rows, rows, [5, 7], outputs="everything")
    with pytest.raises(ValueError, match="outputs= does not combine with similarity"):
        model.forward_videos(rows, rows, [5, 7], outputs="full", similarity=True)
    for extras in (dict(row_scale=(good, None)), dict(row_scale=(None, good)), dict(weight_sums=True), dict(nan_to_num="always")):
        with pytest.raises(ValueError, match="outputs= does not combine with the sweep's extras"):
            model.forward_videos(rows, rows, [5, 7], outputs=("w_i",), **extras)
    # alone it is a valid request: refused on host tensors as the plain call is
    for outputs in ("full", ("image_logvar", "w_e"), iefvad_amd.OUTPUT_KEYS, None):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.forward_videos(rows, rows, [5, 7], outputs=outputs)


def test_forward_videos_host_refuses_bad_outputs_by_cause(no_library):
    model = _model()
    vids = [torch.zeros(5, 768), torch.zeros(7, 768)]
    with pytest.raises(ValueError, match="unknown output key.*'w'"):
        model.forward_videos_host(vids, vids, [5, 7], outputs=["w"])
    with pytest.raises(ValueError, match="outputs= does not combine with similarity"):
        model.forward_videos_host(vids, vids, [5, 7], outputs="full", similarity=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # the model's parameters live on the host here
        model.forward_videos_host(vids, vids, [5, 7], outputs="full")


def test_train_mode_raises_as_before(no_library):
    model = _model().train()
    rows = torch.zeros(12, 768)
    with pytest.raises(RuntimeError, match="evaluation entry point"):
        model.forward_videos(rows, rows, [5, 7], outputs="full")
    with pytest.raises(RuntimeError, match="evaluation entry point"):
        model.forward_videos_host([rows[:5], rows[:7]], [rows[:5], rows[:7]], [5, 7], outputs="full")


def test_wide_keys_follow_the_reference_order():
    from iefvad_amd.model import WIDE_KEYS, _row_output_keys
    assert WIDE_KEYS == ("fused", "image_mu", "event_mu", "image_logvar", "event_logvar", "w_i", "w_e")
    assert _row_output_keys(None) == () and _row_output_keys("full") == WIDE_KEYS
    assert _row_output_keys(("w_e", "logits", "image_logvar")) == ("image_logvar", "w_e")
    assert _row_output_keys("fused") == ("fused",)


class _Stub:
    outputs = "scores"

    def __call__(self, img, ev, *_):
        raise AssertionError("no forward: the call is refused in its checks")

    def forward_videos(self, *a, **k):
        raise AssertionError("no forward on the CPU")


def _items():
    return [(torch.zeros(1, 1, 256, 8), torch.zeros(1, 1, 256, 8), ("Normal",), torch.tensor([10]))]


def test_score_loader_row_outputs_is_checked_before_any_forward():
    with pytest.raises(ValueError, match="row_outputs takes the valid-row routes"):
        harness.score_loader(_Stub(), _items(), 256, "cpu", "ucfcrime", batch_chunks=4, row_outputs="full")
    with pytest.raises(ValueError, match="row_outputs takes the valid-row routes"):
        harness.score_loader(_Stub(), _items(), 256, "cuda:0", "ucfcrime", batch_chunks=0, row_outputs=("w_i",))
    with pytest.raises(ValueError, match="row_outputs takes the valid-row routes"):
        harness.score_loader(_Stub(), _items(), 256, "cuda:0", "ucfcrime", batch_chunks=4, ragged=False, row_outputs=("w_i",))
    with pytest.raises(ValueError, match="unknown output key"):
        harness.score_loader(_Stub(), _items(), 256, "cpu", "ucfcrime", batch_chunks=4, row_outputs=("image_sigma",))
    for sim in (True, "rows"):
        with pytest.raises(ValueError, match="row_outputs does not combine with similarity"):
            harness.score_loader(_Stub(), _items(), 256, "cuda:0", "ucfcrime", batch_chunks=4, row_outputs="full", similarity=sim)
