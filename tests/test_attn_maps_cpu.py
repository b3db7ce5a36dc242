"""The encoder's head-averaged attention maps (`iefvad_forward_attn`, `iefvad_forward_videos_attn`; `MMFMIL.forward(attn_maps=)`,
`forward_videos(attn_maps=)`; `harness.score_loader(attn_maps=)`) -- what can be checked without a GPU: the fixtures are what the
torch restatement of tests/attn_cases.py computes (so the GPU tests may use it for other shapes) and the sharp fixtures are peaked, the
two entries exist with the documented signatures and refuse bad requests by name before any HIP call, and the Python layers validate
their arguments before the library is loaded."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness
from iefvad_amd import lib as L
from iefvad_amd.model import attn_map_layers
from tests import attn_cases as A

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iefvad.h")
DENSE, ROWS = "iefvad_forward_attn", "iefvad_forward_videos_attn"


@pytest.mark.parametrize("name", A.FIXTURES)
def test_restatement_reproduces_the_fixture_within_its_floor(name):
    """fp64 against the reference's fp64 capture: 1e-12 (both are fp64 evaluations of the same formula; the weights are <= 1).  fp32
    against it: the fixture's own floor, the reference's fp32 error, times 3 -- the margin the GPU test gives the kernel."""
    g, cfg, sd, img, ev = A.load_fixture(name)
    ti, te = torch.from_numpy(img), torch.from_numpy(ev)
    m64 = A.encoder_maps(sd, ti, te, cfg["L"], torch.float64)
    m32 = A.encoder_maps(sd, ti, te, cfg["L"], torch.float32)
    assert g["rows"].shape == (cfg["B"], 16) and {0, A.VALID_LAST - 1, 200} <= set(g["rows"][-1].tolist())
    for m, mod in enumerate(A.MODALITIES):
        assert g[mod].shape == (cfg["L"], cfg["B"], 16, A.T) and g[mod].dtype == np.float64
        for l in range(cfg["L"]):
            want = g[mod][l]
            assert np.abs(want.sum(-1) - 1).max() < 1e-12
            d64 = np.abs(A.fixture_rows(g, m64[(m, l)].numpy(), m, l) - want).max()
            d32 = np.abs(A.fixture_rows(g, m32[(m, l)].double().numpy(), m, l) - want).max()
            print(f"{name} {mod} layer {l}: fp64 {d64:.2e}, fp32 {d32:.2e}, floor {g['attn_floor'][m, l]:.2e}, max {g['attn_max'][m, l]:.4f}")
            assert d64 <= 1e-12, (mod, l, d64)
            assert d32 <= 3 * g["attn_floor"][m, l], (mod, l, d32, g["attn_floor"][m, l])


@pytest.mark.parametrize("name", A.SHARP)
def test_sharp_fixtures_are_peaked(name):
    """A flat average (every weight 1/256 = 0.0039) must not pass the accuracy gates: the sharp fixtures have a dominant key."""
    g = A.load_fixture(name)[0]
    assert g["attn_max"].shape == (2, 2) and g["attn_max"].min() >= 0.1, g["attn_max"]
    assert np.abs(g["image"] - 1.0 / 256).max() > 100 * 3 * g["attn_floor"].max()


def test_flat_fixture_is_the_almost_flat_average():
    g = A.load_fixture("attn_flat_k3")[0]
    assert 1.0 / 256 < g["attn_max"].max() < 0.01


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        L.build_library()
    return L.load_library()


def test_entries_exist_with_the_documented_signatures(lib):
    for s in (DENSE, ROWS):
        assert s in L.SYMBOLS and hasattr(lib, s)
    maps_p = C.POINTER(L.AttnMaps)
    dense, plain = lib.iefvad_forward.argtypes, lib.iefvad_forward_videos.argtypes
    assert lib.iefvad_forward_attn.restype is C.c_int and lib.iefvad_forward_videos_attn.restype is C.c_int
    assert lib.iefvad_forward_attn.argtypes == dense[:8] + [maps_p] + dense[8:] and len(dense) == 9
    assert lib.iefvad_forward_videos_attn.argtypes == plain[:12] + [maps_p] + plain[12:] and len(plain) == 13
    assert lib.iefvad_abi_version() == 8 and L.ABI_VERSION == 8          # entries were added, no struct changed
    assert [n for n, _ in L.AttnMaps._fields_] == ["image", "event"] and C.sizeof(L.AttnMaps) == 2 * L.MAX_LAYERS * C.sizeof(C.c_void_p)


def test_the_header_declares_the_entries_and_their_limits():
    text = open(HEADER).read()
    for s in (DENSE, ROWS):
        assert s + "(" in text
    assert "typedef struct iefvad_attn_maps" in text and "#define IEFVAD_ABI_VERSION 8" in text
    assert "compute = BF16" in text


OK = 0x10000                                                             # never read: every call below stops in its checks


def _maps(**kw):
    m = L.AttnMaps()
    for k, (l, v) in kw.items():
        getattr(m, k)[l] = v
    return m


def _dense(lib, h, maps):
    o = L.Outputs()
    o.logits = OK
    rc = lib.iefvad_forward_attn(h, C.c_void_p(OK), C.c_void_p(OK), L.IN_F32, 1, C.c_void_p(OK), 1 << 30, C.byref(o),
                                 C.byref(maps) if maps is not None else None, None)
    return rc, L.last_error()


def _rows(lib, h, maps):
    lens = (C.c_int32 * 2)(5, 7)
    rc = lib.iefvad_forward_videos_attn(h, C.c_void_p(OK), C.c_void_p(OK), L.IN_F32, lens, 2, 1, C.c_void_p(OK), 1 << 30, C.c_void_p(OK),
                                        None, None, C.byref(maps) if maps is not None else None, None)
    return rc, L.last_error()


@pytest.mark.parametrize("call,name", [(_dense, DENSE), (_rows, ROWS)])
def test_bad_requests_are_refused_by_name_with_no_device(lib, call, name):
    """No handle exists without a GPU: the null handle is refused first; a non-null (never dereferenced) handle word then shows that
    null maps, all-null maps and a misaligned map are refused before the handle is looked at -- hence before any HIP call."""
    fake = C.c_void_p(0x10000)
    for h, maps, frag in [(None, _maps(image=(0, OK)), "null handle"), (fake, None, "null maps"), (fake, _maps(), "every map is null"),
                          (fake, _maps(image=(1, OK + 4)), "16-byte aligned"), (fake, _maps(event=(0, OK + 8)), "16-byte aligned")]:
        rc, msg = call(lib, h, maps)
        assert rc != 0 and msg.startswith(name + ":") and frag in msg, (frag, msg)


def test_attn_map_layers_rules():
    assert attn_map_layers(None, 2) == () and attn_map_layers(False, 2) == ()
    assert attn_map_layers(True, 3) == (0, 1, 2)
    assert attn_map_layers([1, 0, 1], 2) == (0, 1) and attn_map_layers(1, 2) == (1,) and attn_map_layers(iter((0,)), 2) == (0,)
    for bad in ([2], [-1], [0.0], "0", [], [True], 2, 1.5):
        with pytest.raises(ValueError, match="attn_maps takes True or"):
            attn_map_layers(bad, 2)


def _model(**kw):
    return iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, "cuda", A.model_args(2, 1), **kw).eval()


@pytest.fixture
def no_library(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "load_library", no_load)


def test_forward_refuses_bad_requests_by_cause(no_library):
    model = _model()
    x = torch.zeros(1, 256, 768)
    with pytest.raises(ValueError, match="attn_maps takes True or layer indices in 0..1"):
        model(x, x, None, None, None, attn_maps=[2])
    with pytest.raises(ValueError, match="does not combine with timed=True or row_scale"):
        model(x, x, None, None, None, attn_maps=True, timed=True)
    with pytest.raises(ValueError, match="does not combine with timed=True or row_scale"):
        model(x, x, None, None, None, attn_maps=[0], row_scale=(torch.ones(256), None))
    with pytest.raises(RuntimeError, match='compute="bf16"'):
        _model(compute="bf16")(x, x, None, None, None, attn_maps=True)
    with pytest.raises(RuntimeError, match=r"model\.train\(\)"):
        _model().train()(x, x, None, None, None, attn_maps=True)
    for ok in (True, [1], None):                   # a valid request: refused on host tensors as the plain call is
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model(x, x, None, None, None, attn_maps=ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # return_attn stays accepted and ignored, as in the reference
        model(x, x, None, None, None, True)


def test_forward_videos_refuses_bad_requests_by_cause(no_library):
    model = _model()
    rows = torch.zeros(12, 768)
    good = torch.ones(12)
    with pytest.raises(ValueError, match="attn_maps takes True or layer indices"):
        model.forward_videos(rows, rows, [5, 7], attn_maps=[0, 5])
    for extras in (dict(similarity=True), dict(outputs="full"), dict(outputs=("w_i",)), dict(row_scale=(good, None)), dict(row_scale=(None, good)),
                   dict(weight_sums=True), dict(nan_to_num="always")):
        with pytest.raises(ValueError, match="attn_maps= does not combine with"):
            model.forward_videos(rows, rows, [5, 7], attn_maps=True, **extras)
    with pytest.raises(RuntimeError, match='compute="bf16"'):
        _model(compute="bf16").forward_videos(rows, rows, [5, 7], attn_maps=True)
    with pytest.raises(RuntimeError, match=r"model\.train\(\)"):
        _model().train().forward_videos(rows, rows, [5, 7], attn_maps=[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.forward_videos(rows, rows, [5, 7], attn_maps=[1])


class _Stub:
    outputs = "scores"
    temporal = type("T", (), {"num_layers": 2})()

    def __call__(self, img, ev, *_):
        raise AssertionError("no forward: the call is refused in its checks")

    def forward_videos(self, *a, **k):
        raise AssertionError("no forward on the CPU")


def _items():
    return [(torch.zeros(1, 1, 256, 8), torch.zeros(1, 1, 256, 8), ("Normal",), torch.tensor([10]))]


def test_score_loader_attn_maps_is_checked_before_any_forward():
    with pytest.raises(ValueError, match="attn_maps takes the forward_videos loop"):
        harness.score_loader(_Stub(), _items(), 256, "cpu", "ucfcrime", batch_chunks=4, attn_maps=True)
    with pytest.raises(ValueError, match="attn_maps takes the forward_videos loop"):
        harness.score_loader(_Stub(), _items(), 256, "cuda:0", "ucfcrime", batch_chunks=4, ragged=False, attn_maps=[0])
    with pytest.raises(ValueError, match="attn_maps takes the forward_videos loop"):
        harness.score_loader(_Stub(), _items(), 256, "cuda:0", "ucfcrime", batch_chunks=0, attn_maps=[0])
    with pytest.raises(ValueError, match="attn_maps does not combine with similarity or row_outputs"):
        harness.score_loader(_Stub(), _items(), 256, "cuda:0", "ucfcrime", batch_chunks=4, attn_maps=True, row_outputs="full")
    for sim in (True, "rows"):
        with pytest.raises(ValueError, match="attn_maps does not combine with similarity or row_outputs"):
            harness.score_loader(_Stub(), _items(), 256, "cuda:0", "ucfcrime", batch_chunks=4, attn_maps=True, similarity=sim)
    with pytest.raises(ValueError, match="attn_maps takes True or layer indices"):
        harness.score_loader(_Stub(), _items(), 256, "cuda:0", "ucfcrime", batch_chunks=4, attn_maps=[3])


def test_test_functions_take_attn_maps_keyword_only():
    import inspect
    for fn in (harness.test, harness.ucf_test, harness.xd_test):
        p = inspect.signature(fn).parameters["attn_maps"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
