"""The fusion ablations without a GPU: the C declarations and exported symbols, the refusals of the entries and of the Python keywords
(all before a device is touched), the fp64 restatement (tests/variants_cases.py) against the committed reference capture
(tests/golden/variants_k3.npz, make_golden_variants.py) on the CPU oracle's head tensors, and the harness's AUC / AP table from a
stubbed score_loader."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth
from iefvad_amd import lib as L
from iefvad_amd.model import fusion_variant_names
from oracle import iefvad_oracle as orc
from tests import helpers as H
from tests import variants_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("iefvad_forward_variants", "iefvad_forward_videos_variants")


def cpu_model(K=3, compute="f32", **kw):
    args = argparse.Namespace(visual_layers=1, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    return iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 1, 8, 10, 10, "cpu", args, compute=compute, **kw).eval()


def test_header_declares_the_entries_and_keeps_the_abi():
    header = open(os.path.join(ROOT, "include", "iefvad.h")).read()
    assert "#define IEFVAD_ABI_VERSION 8" in header
    assert "enum { IEFVAD_VARIANT_FUSED = 0, IEFVAD_VARIANT_IMAGE = 1, IEFVAD_VARIANT_EVENT = 2, IEFVAD_VARIANT_EQUAL = 3 };" in header
    assert "typedef struct iefvad_variants { int32_t count; int32_t kind[4]; float* logits; size_t stride; } iefvad_variants;" in header
    assert "int iefvad_forward_variants(iefvad_handle* h," in header and "int iefvad_forward_videos_variants(iefvad_handle* h," in header
    assert "size_t iefvad_variants_workspace_bytes(" in header and "size_t iefvad_videos_variants_workspace_bytes(" in header
    lib = L.load_library()
    assert lib.iefvad_abi_version() == 8 and L.ABI_VERSION == 8


def test_library_exports_the_symbols():
    lib = L.load_library()
    for s in ENTRIES + ("iefvad_variants_workspace_bytes", "iefvad_videos_variants_workspace_bytes"):
        assert s in L.SYMBOLS and hasattr(lib, s), s
    assert lib.iefvad_forward_variants.restype is C.c_int and lib.iefvad_variants_workspace_bytes.restype is C.c_size_t
    assert C.sizeof(L.Variants) == 24 + C.sizeof(C.c_void_p) + C.sizeof(C.c_size_t)      # count + kind[4], padded to the pointer
    assert L.VARIANT_NAMES == ("fused", "image", "event", "equal") == VC.NAMES


def test_null_arguments_are_refused_by_name():
    lib = L.load_library()
    v = L.Variants()
    o = L.Outputs()
    lens = (C.c_int32 * 1)(5)
    assert lib.iefvad_forward_variants(None, None, None, 0, 1, None, 0, C.byref(o), C.byref(v), None) != 0
    assert L.last_error().startswith("iefvad_forward_variants:") and "null" in L.last_error()
    assert lib.iefvad_forward_videos_variants(None, None, None, 0, lens, 1, 1, None, 0, None, None, None, C.byref(v), None) != 0
    assert L.last_error().startswith("iefvad_forward_videos_variants:") and "null" in L.last_error()
    assert lib.iefvad_variants_workspace_bytes(None, 1, 4) == 0 and lib.iefvad_videos_variants_workspace_bytes(None, lens, 1, 4) == 0


def test_names():
    assert fusion_variant_names(None) == () and fusion_variant_names(False) == ()
    assert fusion_variant_names(True) == ("fused", "image", "event", "equal")
    assert fusion_variant_names(("event", "image")) == ("event", "image")
    assert fusion_variant_names("equal") == ("equal",)
    for bad in (("fused", "average"), ["Image"], 3, ()):
        with pytest.raises(ValueError, match="fusion_variants takes True or"):
            fusion_variant_names(bad)
    with pytest.raises(ValueError, match="more than once"):
        fusion_variant_names(("image", "event", "image"))


def test_refusals_come_before_a_device_is_touched():
    """Host tensors throughout: a call that got as far as the device check would raise RuntimeError ("runs on a HIP device only")."""
    m = cpu_model()
    x = torch.zeros(1, 256, 768)
    v = torch.zeros(256)
    with pytest.raises(ValueError, match="unknown fusion variant"):
        m(x, x, None, None, None, fusion_variants=("mean",))
    with pytest.raises(ValueError, match="more than once"):
        m(x, x, None, None, None, fusion_variants=("equal", "equal"))
    for kw, word in ((dict(timed=True), "timed"), (dict(trajectory=True), "trajectory"), (dict(attn_maps=True), "attn_maps"),
                     (dict(row_scale=(v, None)), "row_scale"), (dict(row_noise=(v, None), noise_seed=1), "row_noise")):
        with pytest.raises(ValueError, match="fusion_variants= does not combine with " + word):
            m(x, x, None, None, None, fusion_variants=True, **kw)
    with pytest.raises(RuntimeError, match="requires grad"):
        m(x.clone().requires_grad_(True), x, None, None, None, fusion_variants=True)
    rows = torch.zeros(5, 768)
    with pytest.raises(ValueError, match="unknown fusion variant"):
        m.forward_videos(rows, rows, [5], fusion_variants=["fuse"])
    for kw, word in ((dict(trajectory=True), "trajectory"), (dict(attn_maps=[0]), "attn_maps"), (dict(row_scale=(None, v[:5])), "row_scale"),
                     (dict(row_noise=(v[:5], None), noise_seed=1), "row_noise"), (dict(similarity=True), "similarity"),
                     (dict(outputs="full"), "outputs="), (dict(weight_sums=True), "weight_sums"), (dict(nan_to_num="always"), "nan_to_num='always'")):
        with pytest.raises(ValueError, match="fusion_variants= does not combine with " + word):
            m.forward_videos(rows, rows, [5], fusion_variants=True, **kw)
    with pytest.raises(RuntimeError, match="requires grad"):
        m.forward_videos(rows.clone().requires_grad_(True), rows, [5], fusion_variants=("image",))
    m.train()
    with pytest.raises(RuntimeError, match="model.train()"):
        m(x, x, None, None, None, fusion_variants=True)
    with pytest.raises(RuntimeError, match="model.train()"):
        m.forward_videos(rows, rows, [5], fusion_variants=True)
    m.eval()
    f = cpu_model(compute="fp16x3")
    with pytest.raises(RuntimeError, match="fp16x3"):
        f(x, x, None, None, None, fusion_variants=True)
    with pytest.raises(RuntimeError, match="fp16x3"):
        f.forward_videos(rows, rows, [5], fusion_variants=True)
    assert "fusion_variants" not in m.forward_videos_host.__code__.co_varnames       # the host-list entry does not take it


def test_harness_refusals():
    m = cpu_model()
    with pytest.raises(ValueError, match="HIP device"):
        harness.score_loader(m, [], 256, "cpu", fusion_variants=True)
    with pytest.raises(ValueError, match="iefvad_amd.MMFMIL"):
        harness.score_loader(lambda *a: None, [], 256, "cuda", fusion_variants=True)
    with pytest.raises(ValueError, match="unknown fusion variant"):
        harness.score_loader(m, [], 256, "cuda", fusion_variants=("both",))
    for kw in (dict(similarity=True), dict(trajectory=True), dict(attn_maps=True), dict(row_outputs="full")):
        with pytest.raises(ValueError, match="fusion_variants does not combine"):
            harness.score_loader(m, [], 256, "cuda", fusion_variants=True, **kw)
    with pytest.raises(ValueError, match="host_list"):      # the default walk of a packed evaluation is the host list
        harness.score_loader(m, [], 256, "cuda", batch_chunks=8, fusion_variants=True)
    args = argparse.Namespace(dataset="ucfcrime", exp_name="x")
    for kw in (dict(vis=True), dict(trajectory=True), dict(attn_maps=True)):
        with pytest.raises(ValueError, match="fusion_variants does not combine"):
            harness.test(args, m, [], 256, None, np.zeros(16), "cpu", fusion_variants=True, **kw)


@pytest.mark.parametrize("tag, noise, K", [("studentt", "StudentT", 3), ("gaussian", "Gaussian", 3), ("k0", "StudentT", 0)])
def test_restatement_meets_the_fixture_on_the_oracle_heads(golden_dir, tag, noise, K):
    """The four substitutions + refinement + classifier restated in fp64 (variants_cases.variant_logits), on the head tensors of the CPU
    oracle, against the reference's capture: within 3 x the reference's own fp32 floor of each variant."""
    g, cfg, sd, img, ev = VC.load_variants_case(golden_dir)
    assert tuple(str(n) for n in g["names"]) == VC.NAMES
    off = ~np.eye(4, dtype=bool)
    assert float(g["sep_median_" + tag][off].min()) >= 3 * VC.TOL_LOGIT_BF16      # no gate can hide a swapped or dropped substitution
    sdk = sd if K else VC.without_refinement(sd)
    c = dict(cfg, K=K, noise=noise)
    out = orc.forward(sdk, torch.from_numpy(img), torch.from_numpy(ev), H.oracle_cfg(c))
    got = VC.variant_logits(sdk, out["image_mu"], out["image_logvar"], out["event_mu"], out["event_logvar"], K=K, lam=cfg["lam"], noise=noise,
                            nu=cfg["nu"]).reshape(4, cfg["B"], 256)
    assert g["logits_variants_" + tag].shape == got.shape
    for v, name in enumerate(VC.NAMES):
        err = float(np.abs(got[v] - g["logits_variants_" + tag + "_f64"][v]).max())
        gate = 3.0 * float(g["floor_" + tag][v])
        print(f"{tag} {name}: restatement vs reference fp64 {err:.3e}  floor {float(g['floor_' + tag][v]):.3e}  gate {gate:.3e}")
        assert err <= gate, (name, err)
        assert float(np.abs(g["logits_variants_" + tag][v] - g["logits_variants_" + tag + "_f64"][v]).max()) == float(g["floor_" + tag][v])
    # the oracle's own logits are the "fused" row
    err = float(np.abs(out["logits"].numpy().reshape(cfg["B"], 256) - got[0]).max())
    assert err <= H.TOL_LOGIT, err


def test_harness_adds_the_table_from_a_stubbed_walk(monkeypatch, capsys):
    """`test(..., fusion_variants=)` on a stubbed score_loader: "auc_variants" / "ap_variants" by sklearn's calls on each variant's
    scores, the returned tuple, the existing keys and the printed text unchanged."""
    from sklearn.metrics import average_precision_score, roc_auc_score
    rng = np.random.default_rng(3)
    classes = list(harness.CLASS_KEYS["ucfcrime"])      # every class once: the metric tail raises on an empty class, as the reference does
    lens = [3 + (7 * i) % 5 for i in range(len(classes))]
    n = sum(lens)
    gt = (rng.random(n * 16) > 0.6).astype(np.float64)
    names = ("event", "fused", "equal")
    var = rng.random((3, n)).astype(np.float32)
    scores = [var[1, a:a + k].copy() for a, k in zip(np.cumsum([0] + lens[:-1]), lens)]      # the call's own scores: the "fused" row
    wi = [np.full(k, 0.5, np.float32) for k in lens]
    calls = []

    def stub(model, loader, maxlen, device, *a, **kw):
        calls.append(kw)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        stub.last_result = None
        if kw.get("fusion_variants"):
            stub.last_result = {"variants": {"names": names, "scores": [var[:, a:b] for a, b in zip(off[:-1], off[1:])],
                                             "scores_device": None, "row_offsets": off}}
        return scores, classes, wi, wi

    monkeypatch.setattr(harness, "score_loader", stub)

    class M:
        def to(self, d): return self
        def eval(self): return self
    args = argparse.Namespace(dataset="ucfcrime", exp_name="x")
    plain = harness.test(args, M(), [], 256, None, gt, "cpu")
    text_plain = capsys.readouterr().out
    keys_plain = set(harness.test.last_result)
    got = harness.test(args, M(), [], 256, None, gt, "cpu", fusion_variants=names)
    text = capsys.readouterr().out
    assert got == plain and text == text_plain                                   # nothing new is printed, the tuple is unchanged
    assert calls[0].get("fusion_variants") is None and calls[1]["fusion_variants"] == names and calls[1]["host_list"] is False
    last = harness.test.last_result
    assert set(last) == keys_plain | {"variants", "auc_variants", "ap_variants"}
    for v, name in enumerate(names):
        assert last["auc_variants"][name] == roc_auc_score(gt, np.repeat(var[v].tolist(), 16))
        assert last["ap_variants"][name] == average_precision_score(gt, np.repeat(var[v].tolist(), 16))
    assert last["auc_variants"]["fused"] == plain[0]
