"""Which library entry and workspace query every kind of request reaches (`model._DENSE_ENTRIES`, `model._ROW_ENTRIES`), and what comes
back: the keys in order, every shape and dtype, and `logits` bit for bit where the docstrings promise that every other result keeps its
bits.  A proxy in the place of `lib.load_library()` records the `iefvad_forward*` and `*_workspace_bytes` calls.  Nothing here provokes
an error on the device: the refusals are tests/test_request_refusals_cpu.py's.  `-m gpu`."""
import argparse

import pytest
import torch

import iefvad_amd
from iefvad_amd import model as M
from iefvad_amd import synth

pytestmark = pytest.mark.gpu

T, D = 256, 768
LENGTHS = [5, 300]      # one short video and one that crosses a chunk boundary: three chunks
N = sum(LENGTHS)
F32, F64 = torch.float32, torch.float64
SCORES = {"logits": ((N,), F32), "w_i_mean": ((N,), F32), "w_e_mean": ((N,), F32)}
NAMES = ("fused", "image", "event", "equal")


class Recorder:
    """The library, with the names of the forward entries and workspace queries that were called."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not (name.startswith("iefvad_forward") or name.endswith("_workspace_bytes")):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


@pytest.fixture(scope="module")
def model():
    args = argparse.Namespace(visual_layers=1, visual_head=8, num_refinement_steps=1, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, D, T, D, 8, 1, 8, 10, 10, "cuda", args, compute="f32")
    m.load_state_dict(synth.make_state_dict(5, D, 1, 1))
    return m.to("cuda:0").eval()


@pytest.fixture(scope="module")
def data():
    img, ev = (torch.from_numpy(x).cuda() for x in synth.make_inputs(6, 1))
    vids = [synth.make_video(7, i, n) for i, n in enumerate(LENGTHS)]
    host = [[torch.from_numpy(v[m]) for v in vids] for m in (0, 1)]
    rows = [torch.cat(h).cuda() for h in host]
    return {"img": img, "ev": ev, "rows": rows, "host": host, "ones": torch.ones(T, device="cuda"), "zeros": torch.zeros(T, device="cuda"),
            "row_ones": torch.ones(N, device="cuda"), "row_zeros": torch.zeros(N, device="cuda")}


def recorded(monkeypatch, call):
    """`call()` under the recorder -> (its result with the tensors cloned -- a replayed graph writes where the last call wrote --, the calls)."""
    rec = Recorder(M._lib.load_library())
    monkeypatch.setattr(M._lib, "load_library", lambda: rec)
    with torch.no_grad():
        out = call()
    torch.cuda.synchronize()
    monkeypatch.undo()
    return {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in out.items()}, rec.calls


def check(out, calls, want_calls, want):
    """`want`: {key: (shape, dtype) for a tensor, else the value itself}, in the order of the returned dict."""
    assert sorted(calls) == sorted(want_calls), calls
    assert list(out) == list(want)
    for k, w in want.items():
        if isinstance(out[k], torch.Tensor):
            assert (tuple(out[k].shape), out[k].dtype) == w, (k, out[k].shape, out[k].dtype)
            assert out[k].is_cuda
        else:
            assert out[k] == w, k


@pytest.fixture(scope="module")
def plain(model, data):
    """`logits` of the three plain entries, computed once."""
    with torch.no_grad():
        dense = model(data["img"], data["ev"], None, None, None)["logits"].clone()
        rows = model.forward_videos(data["rows"][0], data["rows"][1], LENGTHS)["logits"].clone()
        host = model.forward_videos_host(data["host"][0], data["host"][1], LENGTHS)["logits"].clone()
    torch.cuda.synchronize()
    return {"dense": dense, "rows": rows, "host": host}


FULL = {k: ((1, T, 1 if k == "logits" else D), F32) for k in M.OUTPUT_KEYS}
DENSE = [
    # kind, keywords (tensors by their name in `data`), entry, query, extra results behind OUTPUT_KEYS, logits keep the plain entry's bits
    ("plain", {}, "iefvad_forward", "iefvad_workspace_bytes", {}, True),
    ("timed", dict(timed=True), "iefvad_forward_timed", "iefvad_workspace_bytes", {}, False),
    ("scaled", dict(row_scale=("ones", None)), "iefvad_forward_scaled", "iefvad_workspace_bytes", {}, False),
    ("perturbed", dict(row_noise=(None, "zeros"), noise_seed=3), "iefvad_forward_perturbed", "iefvad_workspace_bytes", {}, False),
    ("attn", dict(attn_maps=True), "iefvad_forward_attn", "iefvad_workspace_bytes",
     {"image_attn": ((1, 1, T, T), F32), "event_attn": ((1, 1, T, T), F32), "attn_layers": (0,)}, True),
    ("trajectory", dict(trajectory=True), "iefvad_forward_trajectory", "iefvad_trajectory_workspace_bytes",
     {"logits_steps": ((2, 1, T, 1), F32), "delta_norm": ((1, 1, T), F32)}, True),
    ("variants", dict(fusion_variants=True), "iefvad_forward_variants", "iefvad_variants_workspace_bytes",
     {"logits_variants": ((4, 1, T), F32), "fusion_variants": NAMES}, True),
]


def _keywords(kw, data, prefix=""):
    return {k: tuple(data[prefix + x] if isinstance(x, str) else x for x in v) if isinstance(v, tuple) else v for k, v in kw.items()}


@pytest.mark.parametrize("kind,kw,entry,query,extra,same_bits", DENSE, ids=[d[0] for d in DENSE])
def test_dense_kinds(monkeypatch, model, data, plain, kind, kw, entry, query, extra, same_bits):
    assert kind in M._DENSE_ENTRIES and len(M._DENSE_ENTRIES) == len(DENSE)
    model.last_stage_times = None
    out, calls = recorded(monkeypatch, lambda: model(data["img"], data["ev"], None, None, None, **_keywords(kw, data)))
    check(out, calls, [entry, query], {**FULL, **extra})
    assert (model.last_stage_times is not None) == (kind == "timed")
    if same_bits:
        assert torch.equal(out["logits"], plain["dense"])


WIDE = {k: ((N, D), F32) for k in M.WIDE_KEYS}
ROWS = [
    # suffix, keywords, the suffix of the workspace query, extra results behind the three score vectors, logits keep the plain entry's bits
    ("", {}, "", {}, True),
    ("_similarity", dict(similarity=True), "", {"similarity": ((4, N), F32)}, True),
    ("_full", dict(outputs="full"), "_full", WIDE, True),
    ("_scaled", dict(weight_sums=True), "_scaled", {"w_colsum": ((2, D), F64)}, False),
    ("_perturbed", dict(row_noise=("zeros", None), noise_seed=3), "_scaled", {}, False),
    ("_attn", dict(attn_maps=True), "", {"image_attn": ((1, N, T), F32), "event_attn": ((1, N, T), F32), "attn_layers": (0,)}, True),
    ("_trajectory", dict(trajectory=True), "_trajectory", {"logits_steps": ((2, N), F32), "delta_norm": ((1, N), F32)}, True),
    ("_variants", dict(fusion_variants=True), "_variants", {"logits_variants": ((4, N), F32), "fusion_variants": NAMES}, True),
]


@pytest.mark.parametrize("suffix,kw,query,extra,same_bits", ROWS, ids=[r[0] or "plain" for r in ROWS])
def test_row_suffixes(monkeypatch, model, data, plain, suffix, kw, query, extra, same_bits):
    assert suffix in M._ROW_ENTRIES and len(M._ROW_ENTRIES) == len(ROWS)
    out, calls = recorded(monkeypatch, lambda: model.forward_videos(data["rows"][0], data["rows"][1], LENGTHS, **_keywords(kw, data, "row_")))
    check(out, calls, ["iefvad_forward_videos" + suffix, f"iefvad_videos{query}_workspace_bytes"], {**SCORES, **extra})
    if same_bits:
        assert torch.equal(out["logits"], plain["rows"])


@pytest.mark.parametrize("suffix,kw,extra", [("", {}, {}), ("_similarity", dict(similarity=True), {"similarity": ((4, N), F32)}),
                                             ("_full", dict(outputs="full"), WIDE)], ids=["plain", "_similarity", "_full"])
def test_host_list_suffixes(monkeypatch, model, data, plain, suffix, kw, extra):
    out, calls = recorded(monkeypatch, lambda: model.forward_videos_host(data["host"][0], data["host"][1], LENGTHS, **kw))
    check(out, calls, ["iefvad_forward_videos_host" + suffix], {**SCORES, **extra})      # the library owns this entry's workspace: no query
    assert torch.equal(out["logits"], plain["host"])
