"""The score samples without a GPU: the C declarations and exported symbols, `harness.sample_seed`, the host model
(`harness.sample_states_host` + the CPU oracle's tail, tests/samples_cases.py) against the committed reference capture
(tests/golden/samples_k3.npz, make_golden_samples.py), the refusals of the entries and of the Python methods on host tensors (all
before a device is touched), and the harness's plumbing from a stubbed model / a stubbed score_loader."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness
from iefvad_amd import lib as L
from oracle import iefvad_oracle as orc
from tests import helpers as H
from tests import samples_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cpu_model(K=3, compute="f32", **kw):
    args = argparse.Namespace(visual_layers=1, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    return iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 1, 8, 10, 10, "cpu", args, compute=compute, **kw).eval()


def test_header_declares_the_entries_and_keeps_the_abi():
    header = open(os.path.join(ROOT, "include", "iefvad.h")).read()
    assert "#define IEFVAD_ABI_VERSION 8" in header
    assert "typedef struct iefvad_samples {" in header and "} iefvad_samples;" in header
    assert "int iefvad_forward_samples(iefvad_handle* h," in header and "int iefvad_forward_videos_samples(iefvad_handle* h," in header
    assert "size_t iefvad_samples_workspace_bytes(" in header and "size_t iefvad_videos_samples_workspace_bytes(" in header
    lib = L.load_library()
    assert lib.iefvad_abi_version() == 8 and L.ABI_VERSION == 8
    for s in ("iefvad_forward_samples", "iefvad_forward_videos_samples", "iefvad_samples_workspace_bytes", "iefvad_videos_samples_workspace_bytes"):
        assert s in L.SYMBOLS and hasattr(lib, s), s
    assert lib.iefvad_forward_samples.restype is C.c_int and lib.iefvad_samples_workspace_bytes.restype is C.c_size_t
    # int32, pad, uint64, float, pad, four pointers and a size_t
    assert C.sizeof(L.Samples) == 8 + 8 + 8 + 4 * C.sizeof(C.c_void_p) + C.sizeof(C.c_size_t)
    assert L.MAX_SAMPLES == 64


def test_sample_seed_wraps_mod_2_64():
    step = 0x9E3779B97F4A7C15
    assert harness.SAMPLE_SEED_STEP == step
    assert harness.sample_seed(7, 0) == 7
    assert harness.sample_seed(7, 1) == 7 + step
    assert harness.sample_seed(2 ** 64 - 1, 1) == step - 1                       # the sum wraps
    assert harness.sample_seed(0, 2) == (2 * step) % 2 ** 64 and 2 * step >= 2 ** 64      # so does the product
    assert harness.sample_seed(5, 63) == (5 + 63 * step) % 2 ** 64
    assert harness.sample_seed(-1, 0) == 2 ** 64 - 1                              # a negative seed is its residue, as the C entry's uint64_t takes it
    assert len({harness.sample_seed(11, s) for s in range(64)}) == 64


def test_null_arguments_are_refused_by_name():
    lib = L.load_library()
    sm = L.Samples()
    o = L.Outputs()
    lens = (C.c_int32 * 1)(5)
    assert lib.iefvad_forward_samples(None, None, None, 0, 1, None, 0, C.byref(o), C.byref(sm), None) != 0
    assert L.last_error().startswith("iefvad_forward_samples:") and "null" in L.last_error()
    assert lib.iefvad_forward_videos_samples(None, None, None, 0, lens, 1, 1, None, 0, None, None, None, C.byref(sm), None) != 0
    assert L.last_error().startswith("iefvad_forward_videos_samples:") and "null" in L.last_error()
    assert lib.iefvad_samples_workspace_bytes(None, 1) == 0 and lib.iefvad_videos_samples_workspace_bytes(None, lens, 1) == 0


@pytest.mark.parametrize("tag, noise, K", SC.TAGS)
def test_host_model_meets_the_fixture_on_the_oracle_heads(golden_dir, tag, noise, K):
    """`sample_states_host` on the fp64 head tensors of the CPU oracle, then the oracle's tail, against the reference's fp64 capture:
    within floor + eps_floor, both read from the fixture.  This validates the fixture and the host model together."""
    g, cfg, sd, img, ev = SC.load_samples_case(golden_dir)
    S, B = cfg["S"], cfg["B"]
    off = ~np.eye(S, dtype=bool)
    assert float(g["sep_median_" + tag][off].min()) >= 3 * SC.TOL_LOGIT_BF16      # no gate can hide a reused or dropped draw
    sdk = sd if K else SC.without_refinement(sd)
    out = orc.forward(sdk, torch.from_numpy(img), torch.from_numpy(ev), H.oracle_cfg(dict(cfg, K=K, noise=noise)), dtype=torch.float64)
    heads = [out[k] for k in ("image_mu", "image_logvar", "event_mu", "event_logvar")]
    got = SC.host_sample_logits(sdk, heads, S, cfg["seed"], np.arange(B * 256), K=K, lam=cfg["lam"], noise=noise, nu=cfg["nu"], scale=cfg["scale"])
    want32, want64 = g["logits_samples_" + tag], g["logits_samples_" + tag + "_f64"]
    assert got.shape == want64.shape == (S, B, 256)
    floor, eps_floor = float(g["floor_" + tag]), float(g["eps_floor_" + tag])
    assert float(np.abs(want32 - want64).max()) == floor
    err = float(np.abs(got - want64).max())
    print(f"{tag}: host model vs reference fp64 {err:.3e}  floor {floor:.3e}  eps_floor {eps_floor:.3e}  amp {float(g['amp_' + tag]):.3f}")
    assert err <= floor + eps_floor, err
    # scale = 0: every sample is the oracle's own logits
    zero = SC.host_sample_logits(sdk, heads, 2, cfg["seed"], np.arange(B * 256), K=K, lam=cfg["lam"], noise=noise, nu=cfg["nu"], scale=0.0)
    assert np.array_equal(zero[0], zero[1])
    assert float(np.abs(zero[0] - out["logits"].numpy().reshape(B, 256)).max()) <= floor


def test_host_model_takes_its_draws_by_snippet_id():
    rng = np.random.default_rng(5)
    t = [torch.from_numpy(rng.standard_normal((6, 768))) for _ in range(4)]
    ids = np.array([3, 900, 4, 5, 70000, 3])
    z = harness.sample_states_host(*t, 9, 2, ids, 9 / 8, 1e-8)
    one = harness.sample_states_host(*[x[4:5] for x in t], 9, 2, ids[4:5], 9 / 8, 1e-8)
    assert torch.equal(z[4:5], one)                                               # a row's state depends on its id alone
    same = harness.sample_states_host(*[x[[0, 0]] for x in t], 9, 2, ids[[0, 5]], 9 / 8, 1e-8)
    assert torch.equal(same[0], same[1])                                          # the same id, the same draw
    assert not torch.equal(z, harness.sample_states_host(*t, 9, 3, ids, 9 / 8, 1e-8))
    # sample s of seed is sample 0 of sample_seed(seed, s)
    assert torch.equal(z, harness.sample_states_host(*t, harness.sample_seed(9, 2), 0, ids, 9 / 8, 1e-8))


def test_refusals_on_host_tensors():
    """Host tensors throughout: every refusal below is raised before the device check, which comes last ("runs on a HIP device only")."""
    m = cpu_model()
    x = torch.zeros(1, 256, 768)
    rows = torch.zeros(5, 768)
    for bad in (0, 65, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="samples must be an int in 1..64"):
            m.forward_samples(x, x, bad, 1)
        with pytest.raises(ValueError, match="samples must be an int in 1..64"):
            m.forward_videos_samples(rows, rows, [5], bad, 1)
    for bad in (-0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scale must be finite and >= 0"):
            m.forward_samples(x, x, 4, 1, scale=bad)
        with pytest.raises(ValueError, match="scale must be finite and >= 0"):
            m.forward_videos_samples(rows, rows, [5], 4, 1, scale=bad)
    with pytest.raises(ValueError, match="seed must be an int"):
        m.forward_samples(x, x, 4, 1.5)
    with pytest.raises(RuntimeError, match="requires grad"):
        m.forward_samples(x.clone().requires_grad_(True), x, 4, 1)
    with pytest.raises(RuntimeError, match="requires grad"):
        m.forward_videos_samples(rows.clone().requires_grad_(True), rows, [5], 4, 1)
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.forward_samples(x, x, 4, 1)
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.forward_videos_samples(rows, rows, [5], 4, 1)
    m.train()
    with pytest.raises(RuntimeError, match=r"model.train\(\)"):
        m.forward_samples(x, x, 4, 1)
    with pytest.raises(RuntimeError, match=r"model.train\(\)"):
        m.forward_videos_samples(rows, rows, [5], 4, 1)
    m.eval()
    f = cpu_model(compute="fp16x3")
    with pytest.raises(RuntimeError, match="fp16x3"):
        f.forward_samples(x, x, 4, 1)
    with pytest.raises(RuntimeError, match="fp16x3"):
        f.forward_videos_samples(rows, rows, [5], 4, 1)
    assert "samples" not in m.forward_videos_host.__code__.co_varnames            # there is no host-list entry
    # the request tables of forward / forward_videos are as they were: the samples are methods of their own
    from iefvad_amd import model as M
    assert "samples" not in M._DENSE_ENTRIES and "_samples" not in M._ROW_ENTRIES


def test_harness_refusals():
    m = cpu_model()
    kw = dict(score_samples=4, sample_seed=1)
    with pytest.raises(ValueError, match="HIP device"):
        harness.score_loader(m, [], 256, "cpu", **kw)
    with pytest.raises(ValueError, match="iefvad_amd.MMFMIL"):
        harness.score_loader(lambda *a: None, [], 256, "cuda", **kw)
    with pytest.raises(ValueError, match="sample_seed"):
        harness.score_loader(m, [], 256, "cuda", score_samples=4)
    for extra in (dict(similarity=True), dict(trajectory=True), dict(attn_maps=True), dict(row_outputs="full"), dict(fusion_variants=True), dict(steps=1)):
        with pytest.raises(ValueError, match="score_samples does not combine"):
            harness.score_loader(m, [], 256, "cuda", **kw, **extra)
    with pytest.raises(ValueError, match="host_list=False"):      # the default walk of a packed evaluation is the host list
        harness.score_loader(m, [], 256, "cuda", batch_chunks=8, **kw)
    args = argparse.Namespace(dataset="ucfcrime", exp_name="x")
    for extra in (dict(vis=True), dict(trajectory=True), dict(attn_maps=True), dict(fusion_variants=True), dict(steps=1)):
        with pytest.raises(ValueError, match="score_samples does not combine"):
            harness.test(args, m, [], 256, None, np.zeros(16), "cpu", **kw, **extra)


class _StubModel:
    """What `score_loader(score_samples=)` needs of a model, without a device kernel: results that are a function of the snippet id."""
    outputs = "scores"

    def __init__(self):
        self.calls = []

    def forward_videos(self, *a, **k):       # presence selects the valid-row loop
        raise AssertionError("the samples walk calls forward_videos_samples")

    def forward_samples(self, img, ev, samples, seed, *, scale=1.0, sample_rows=None):
        self.calls.append(("dense", samples, seed, scale, sample_rows.clone()))
        B, T = img.shape[:2]
        ids = sample_rows.reshape(B, T).float()
        ls = torch.stack([ids * 0.01 + s for s in range(samples)])
        return {"logits": ids.reshape(B, T, 1) * 0.01, "w_i_mean": ids, "w_e_mean": -ids, "logits_samples": ls,
                "score_mean": torch.sigmoid(ls).mean(0), "score_std": torch.sigmoid(ls).std(0, unbiased=False)}


def test_score_loader_plumbing_with_a_stubbed_model():
    """The per-video route on a stub: the ids are the snippets' indices in the whole list (0 on pad rows), the sink slices the padded
    slots back to valid snippets, and `last_result["samples"]` has the four documented entries."""
    lens = [3, 256, 300]
    loader = []
    for n in lens:
        c = -(-n // 256) + (1 if n % 256 == 0 else 0)
        shape = (1, 256, 768) if n < 256 else (1, c, 256, 768)                # the loader's shape rule (test.py:77-88)
        loader.append((torch.zeros(shape), torch.zeros(shape), ("Normal",), torch.tensor([n])))
    m = _StubModel()
    sink = harness._ScoreSink()
    sink.dev_traj = []
    harness._score_padded([m], [None], [None], loader, sink, 256, "cpu", "ucfcrime", None, 0, True, samples=(3, 17, 0.5))
    assert [(c[1], c[2], c[3]) for c in m.calls] == [(3, 17, 0.5)] * 3
    start = 0
    for (kind, _, _, _, ids), n in zip(m.calls, lens):
        assert ids.dtype == torch.int32 and torch.equal(ids[:n], torch.arange(start, start + n, dtype=torch.int32)) and not bool(ids[n:].any())
        start += n
    assert [n for _, n in sink.spans] == lens and len(sink.dev_traj) == 3
    assert all(t[0].shape[0] == 3 and t[1].shape[0] == 2 and t[0].shape[1] == t[1].shape[1] for t in sink.dev_traj)


def test_harness_adds_the_figures_from_a_stubbed_walk(monkeypatch, capsys):
    """`test(..., score_samples=)` on a stubbed score_loader: "auc_samples" / "ap_samples" / "auc_mean_score" / "ap_mean_score" by
    sklearn's calls on the returned arrays, the returned tuple, the existing keys and the printed text unchanged."""
    from sklearn.metrics import average_precision_score, roc_auc_score
    rng = np.random.default_rng(4)
    classes = list(harness.CLASS_KEYS["ucfcrime"])
    lens = [3 + (7 * i) % 5 for i in range(len(classes))]
    n = sum(lens)
    gt = (rng.random(n * 16) > 0.6).astype(np.float64)
    S = 3
    ls = rng.standard_normal((S, n)).astype(np.float32)
    sc = torch.sigmoid(torch.from_numpy(ls))
    mean, std = sc.mean(0).numpy(), sc.std(0, unbiased=False).numpy()
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    scores = [rng.random(k).astype(np.float32) for k in lens]
    wi = [np.full(k, 0.5, np.float32) for k in lens]
    calls = []

    def stub(model, loader, maxlen, device, *a, **kw):
        calls.append(kw)
        stub.last_result = None
        if kw.get("score_samples") is not None:
            stub.last_result = {"samples": {"scores_mean": [mean[a:b] for a, b in zip(off[:-1], off[1:])],
                                            "scores_std": [std[a:b] for a, b in zip(off[:-1], off[1:])],
                                            "logits_samples_device": torch.from_numpy(ls), "row_offsets": off}}
        return scores, classes, wi, wi

    monkeypatch.setattr(harness, "score_loader", stub)

    class M:
        def to(self, d): return self
        def eval(self): return self
    args = argparse.Namespace(dataset="ucfcrime", exp_name="x")
    plain = harness.test(args, M(), [], 256, None, gt, "cpu")
    text_plain = capsys.readouterr().out
    keys_plain = set(harness.test.last_result)
    got = harness.test(args, M(), [], 256, None, gt, "cpu", score_samples=S, sample_seed=5)
    text = capsys.readouterr().out
    assert got == plain and text == text_plain                                   # nothing new is printed, the tuple is unchanged
    assert calls[0].get("score_samples") is None
    assert calls[1]["score_samples"] == S and calls[1]["sample_seed"] == 5 and calls[1]["host_list"] is False
    last = harness.test.last_result
    assert set(last) == keys_plain | {"samples", "auc_samples", "ap_samples", "auc_mean_score", "ap_mean_score"}
    assert len(last["auc_samples"]) == S == len(last["ap_samples"])
    for s in range(S):
        assert last["auc_samples"][s] == roc_auc_score(gt, np.repeat(sc[s].numpy().tolist(), 16))
        assert last["ap_samples"][s] == average_precision_score(gt, np.repeat(sc[s].numpy().tolist(), 16))
    assert last["auc_mean_score"] == roc_auc_score(gt, np.repeat(mean.tolist(), 16))
    assert last["ap_mean_score"] == average_precision_score(gt, np.repeat(mean.tolist(), 16))
