"""Generate the golden vectors under tests/golden/ by running the REFERENCE itself.

Run once in the build container (where /root/reference is mounted):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py

It imports `model.imf_vad.MMFMIL` and (for the harness fixture) `test.test` from
/root/reference, loads seeded weights produced by `iefvad_amd.synth.make_state_dict`
into the reference model with `load_state_dict`, runs seeded inputs through it and stores the
reference's OUTPUTS only.  Weights and inputs are regenerated from their seeds by the tests,
so the committed files stay small and contain no reference source.

The reference never travels to the GPU box; these .npz files and this script do.
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"

from iefvad_amd import synth  # noqa: E402

ROW_SUBSET = [0, 1, 37, 99, 100, 101, 128, 200, 254, 255]   # rows of each chunk kept for the 768-d outputs
BIG_KEYS = ["fused", "image_mu", "event_mu", "image_logvar", "event_logvar", "w_i", "w_e"]


def ref_args(L=2, H=8, K=10, lam=0.5, noise="StudentT", nu=8):
    return argparse.Namespace(visual_layers=L, visual_head=H, num_refinement_steps=K, lambda_ref=lam,
                              noise_model=noise, nu=nu)


def build_reference(seed, L=2, K=10, lam=0.5, noise="StudentT", nu=8, factors=None):
    sys.path.insert(0, REF)
    from model.imf_vad import MMFMIL  # the reference model
    model = MMFMIL(14, 768, 256, 768, 8, L, 8, 10, 10, device="cpu", args=ref_args(L, 8, K, lam, noise, nu))
    sd = synth.make_state_dict(seed, 768, L, K)
    if factors is not None:
        sd = synth.sharpen_qk(sd, factors)
    missing = model.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    model.eval()
    return model


# (name, weight seed, input seed, B, L, K, lambda, noise, nu, input dtype, input edit)
CASES = [
    ("base_k10_student8", 11, 21, 3, 2, 10, 0.5, "StudentT", 8, "f32", "tail"),      # chunk 2 zero-padded after row 100
    ("allzero_chunk", 11, 22, 2, 2, 10, 0.5, "StudentT", 8, "f32", "allzero"),       # chunk 1 entirely zero
    ("fp16_in", 11, 23, 1, 2, 10, 0.5, "StudentT", 8, "f16", None),
    ("k0_gauss", 12, 24, 1, 2, 0, 0.5, "Gaussian", 5, "f32", None),
    ("k3_student5", 13, 25, 1, 2, 3, 0.5, "StudentT", 5, "f32", None),
    ("k5_gauss_lam03", 14, 26, 2, 2, 5, 0.3, "Gaussian", 8, "f32", "tail"),
    ("l1_k2", 15, 27, 1, 1, 2, 0.5, "StudentT", 8, "f32", None),
    ("l3_k1", 16, 28, 1, 3, 1, 0.5, "StudentT", 8, "f32", None),
]


def case_inputs(in_seed, B, dtype, edit):
    img, ev = synth.make_inputs(in_seed, B)
    if edit == "tail":
        img[B - 1, 100:] = 0
        ev[B - 1, 100:] = 0
    elif edit == "allzero":
        img[B - 1] = 0
        ev[B - 1] = 0
    if dtype == "f16":
        img, ev = img.astype(np.float16), ev.astype(np.float16)
    return img, ev


# A batch large enough for the split kernels of the bf16x6 / fp16x3 arithmetics (>= 43 chunks): every chunk's logits and
# weight means, the 768-d outputs of three chunks only (keeps the fixture under 1 MB).
BIG_CASE = ("b48_k10_student8", 17, 29, 48, 2, 10, 0.5, "StudentT", 8, "f32", "tail")
BIG_CASE_CHUNKS = [0, 17, 47]


def gen_forward_cases(cases=None, chunk_subset=None):
    for name, wseed, iseed, B, L, K, lam, noise, nu, dt, edit in (cases or CASES):
        model = build_reference(wseed, L, K, lam, noise, nu)
        img, ev = case_inputs(iseed, B, dt, edit)
        with torch.no_grad():
            out = model(torch.from_numpy(img), torch.from_numpy(ev), None, None, None)
        store = {"logits": out["logits"].numpy().reshape(B, 256),
                 "w_i_mean": out["w_i"].mean(dim=-1).numpy(), "w_e_mean": out["w_e"].mean(dim=-1).numpy(),
                 "rows": np.array(ROW_SUBSET),
                 "meta": np.array([wseed, iseed, B, L, K, nu]), "lam": np.array(lam),
                 "noise": np.array(noise), "in_dtype": np.array(dt), "edit": np.array(str(edit))}
        for k in BIG_KEYS:
            store[k] = out[k].numpy()[:, ROW_SUBSET, :]
            if chunk_subset is not None:
                store[k] = store[k][chunk_subset]
        if chunk_subset is not None:
            store["chunks"] = np.array(chunk_subset)
        path = os.path.join(HERE, f"fwd_{name}.npz")
        np.savez_compressed(path, **store)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB")


# The peaked-attention regime (synth.sharpen_qk): with make_state_dict's own weights softmax is an almost flat average over the 256
# keys, so a forward could run with broken attention and stay inside the bf16 gates.  "sharp" = q / k rows x (8, 4): a dominant key per
# query; "over" = x (16, 4): layer-0 scores beyond what exp can represent without the max subtraction.
# (name, weight seed, input seed, B, L, K, lambda, noise, nu, input dtype, input edit, factors, chunk subset)
SHARP_CASES = [
    ("sharp_k3_student8", 11, 12, 3, 2, 3, 0.5, "StudentT", 8, "f32", "tail", (8, 4), None),   # pad keys in a peaked softmax
    ("sharp_b48_k3", 17, 29, 48, 2, 3, 0.5, "StudentT", 8, "f32", "tail", (8, 4), [17, 47]),   # two chunks' 768-d outputs: file size
    ("over_k3_student8", 11, 12, 2, 2, 3, 0.5, "StudentT", 8, "f32", None, (16, 4), None),
]


def attention_statistics(model, run, L, D):
    """Per (modality, layer) of a reference model: max |q k^T / sqrt(d)| and the mean over queries of max_k P, in fp64 from the
    model's own in_proj parameters on the inputs its attention layers receive during `run()` (forward pre-hooks)."""
    seen, hooks = {}, []
    for m, layers in enumerate((model.temporal.image_attn_layers, model.temporal.event_attn_layers)):
        for l, mod in enumerate(layers):
            hooks.append(mod.register_forward_pre_hook(lambda _m, a, key=(m, l): seen.__setitem__(key, a[0].detach().double())))
    run()
    for h in hooks:
        h.remove()
    smax, pmax = np.zeros((2, L)), np.zeros((2, L))
    for m, layers in enumerate((model.temporal.image_attn_layers, model.temporal.event_attn_layers)):
        for l, mod in enumerate(layers):
            x = seen[(m, l)]
            qk = x @ mod.in_proj_weight.detach().double()[: 2 * D].t() + mod.in_proj_bias.detach().double()[: 2 * D]
            q, k = (t.reshape(x.shape[0], 256, 8, D // 8).transpose(1, 2) for t in qk.split(D, dim=-1))
            sc = q @ k.transpose(-1, -2) / np.sqrt(D // 8)
            smax[m, l] = float(sc.abs().max())
            pmax[m, l] = float(torch.softmax(sc, dim=-1).amax(-1).mean())
    return smax, pmax


def sharp_fields(model, img, ev, out, factors, L, D=768):
    """The three fields every peaked-regime fixture carries besides the outputs: the factors, the reference's own fp32-vs-fp64
    distance on the three gated quantities (the model once more in .double()), and the attention statistics per (modality, layer).
    Returns (fields, fp64 outputs)."""
    import copy
    m64 = copy.deepcopy(model).double()
    with torch.no_grad():
        o64 = m64.temporal(torch.from_numpy(img).double(), torch.from_numpy(ev).double())   # MMFMIL.forward casts to float
    sig = lambda t: torch.sigmoid(t.double())
    fields = {"factors": np.array(factors, np.float64),
              "floor_big": np.array(max(float((out[k].double() - o64[k]).abs().max()) for k in BIG_KEYS)),
              "floor_logit": np.array(float((out["logits"].double() - o64["logits"]).abs().max())),
              "floor_sigmoid": np.array(float((sig(out["logits"]) - sig(o64["logits"])).abs().max()))}
    run = lambda: m64.temporal(torch.from_numpy(img).double(), torch.from_numpy(ev).double())
    with torch.no_grad():
        fields["att_max_score"], fields["att_mean_max_p"] = attention_statistics(m64, run, L, D)
    return fields, o64


def gen_sharp_cases(only=None):
    """Forward fixtures of the peaked regime, written as gen_forward_cases writes them plus `sharp_fields`, plus -- for the cases
    the bf16 mode is gated on -- the distance between the fp64 restatement of that mode's rounding points
    (tests/test_gpu_bf16.py::bf16_mode_emulation, CPU only) and the fixture: the mode's own rounding noise, which has to fit
    under the bf16 gates without a kernel being asked."""
    from tests.test_gpu_bf16 import bf16_mode_emulation
    for name, wseed, iseed, B, L, K, lam, noise, nu, dt, edit, factors, chunk_subset in SHARP_CASES:
        if only and name not in only:
            continue
        model = build_reference(wseed, L, K, lam, noise, nu, factors)
        img, ev = case_inputs(iseed, B, dt, edit)
        with torch.no_grad():
            out = model(torch.from_numpy(img), torch.from_numpy(ev), None, None, None)
        fields, _ = sharp_fields(model, img, ev, out, factors, L)
        sd = synth.sharpen_qk(synth.make_state_dict(wseed, 768, L, K), factors)
        emu = bf16_mode_emulation(sd, torch.from_numpy(img), torch.from_numpy(ev), L, K, lam, nu)
        sig = lambda t: torch.sigmoid(t.double())
        fields["bf16_floor_big"] = np.array(max(float((emu[k] - out[k].double()).abs().max()) for k in BIG_KEYS))
        fields["bf16_floor_logit"] = np.array(float((emu["logits"] - out["logits"].double()).abs().max()))
        fields["bf16_floor_sigmoid"] = np.array(float((sig(emu["logits"]) - sig(out["logits"])).abs().max()))
        store = {"logits": out["logits"].numpy().reshape(B, 256),
                 "w_i_mean": out["w_i"].mean(dim=-1).numpy(), "w_e_mean": out["w_e"].mean(dim=-1).numpy(),
                 "rows": np.array(ROW_SUBSET),
                 "meta": np.array([wseed, iseed, B, L, K, nu]), "lam": np.array(lam),
                 "noise": np.array(noise), "in_dtype": np.array(dt), "edit": np.array(str(edit)), **fields}
        for k in BIG_KEYS:
            store[k] = out[k].numpy()[:, ROW_SUBSET, :]
            if chunk_subset is not None:
                store[k] = store[k][chunk_subset]
        if chunk_subset is not None:
            store["chunks"] = np.array(chunk_subset)
        path = os.path.join(HERE, f"fwd_{name}.npz")
        np.savez_compressed(path, **store)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB", {k: np.round(v, 9).tolist() for k, v in fields.items()})


def gen_harness_case():
    """Config 1: a synthetic UCF-shaped .npy set through the reference's own
    `test.test()` loop (/root/reference/test.py:46-212)."""
    sys.path.insert(0, REF)
    seed = 0
    lengths, classes = synth.CONFIG1_LENGTHS, synth.CONFIG1_CLASSES
    tmp = tempfile.mkdtemp(prefix="iefvad_cfg1_")
    rows = []
    for i, (n, c) in enumerate(zip(lengths, classes)):
        img, ev = synth.make_video(seed, i, n)
        if i == 2:            # one NaN element exercises the conditional nan_to_num (test.py:90-95)
            img[5, 7] = np.nan
        if i == 5:            # one fp16 file: dtype is preserved by the loader (dataset.py:49-50)
            img, ev = img.astype(np.float16), ev.astype(np.float16)
        d_rgb = os.path.join(tmp, "feat", "rgb", c)
        d_ev = os.path.join(tmp, "feat", "event_thr_10", c)
        os.makedirs(d_rgb, exist_ok=True)
        os.makedirs(d_ev, exist_ok=True)
        p = os.path.join(d_rgb, f"v{i:03d}__5.npy")
        np.save(p, img)
        np.save(p.replace("rgb", "event_thr_10"), ev)
        rows.append((p, c))
    csv = os.path.join(tmp, "test.csv")
    with open(csv, "w") as f:
        f.write("path,label\n")
        for p, c in rows:
            f.write(f"{p},{c}\n")
    gt = synth.make_gt(seed, int(sum(lengths)))

    cwd = os.getcwd()
    os.chdir(tmp)     # test() does os.makedirs('vis') (test.py:59-62)
    try:
        import test as ref_test                      # /root/reference/test.py
        from data.dataset import UCF_Dataset         # /root/reference/data/dataset.py
        from torch.utils.data import DataLoader
        model = build_reference(11)
        captured = {"logits": [], "ano": None}

        class Recorder(torch.nn.Module):
            def __init__(self, inner):
                super().__init__()
                self.inner = inner

            def forward(self, *a, **k):
                o = self.inner(*a, **k)
                captured["logits"].append(o["logits"].detach().clone())
                return o

        orig_ano = ref_test.compute_ano_auc

        def ano_wrap(*a, **k):
            captured["ano"] = orig_ano(*a, **k)
            return captured["ano"]

        ref_test.compute_ano_auc = ano_wrap
        loader = DataLoader(UCF_Dataset(256, csv, True, None), batch_size=1, shuffle=False)
        args = argparse.Namespace(exp_name="golden", dataset="ucfcrime")
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            roc, ap = ref_test.test(args, Recorder(model), loader, 256, None, gt, "cpu", attn=False, vis=False)
        print(buf.getvalue())
    finally:
        os.chdir(cwd)
    probs = []
    for lg, n in zip(captured["logits"], lengths):
        probs.append(torch.sigmoid(lg.reshape(-1)[:n]).numpy())
    path = os.path.join(HERE, "harness_config1.npz")
    np.savez_compressed(path, scores=np.concatenate(probs), lengths=np.array(lengths),
                        classes=np.array(classes), roc=np.array(roc), ap=np.array(ap),
                        ano_auc=np.array(captured["ano"]), seed=np.array(seed), wseed=np.array(11),
                        chunks=np.array([lg.shape[0] for lg in captured["logits"]]),
                        stdout=np.array(buf.getvalue()))
    print("wrote", path, os.path.getsize(path) // 1024, "KiB", "ROC", roc, "AP", ap, "ano", captured["ano"])


XD_LENGTHS = [60, 256, 130, 300, 45, 90, 513, 20, 77]
XD_LABELS = ["A", "B1-0-0", "B2-0-0", "B4-0-0", "B5-0-0", "B6-0-0", "G-0-0", "B1-B2-0", "A"]


def gen_harness_xd_case():
    """The XD-Violence form of the evaluation loop: labels are codes ("B1-0-0", "B1-B2-0", "A") remapped through
    configs/xd_label_map.json by their first field (/root/reference/test.py:80-81, train/xd_test.py:68), seven class keys
    (test.py:29-33).  train/xd_test.py cannot be imported here (wandb), so the capture runs root `test.test()` with
    args.dataset = 'xd' and the module global `label_map` set as test.py's `__main__` block sets it (test.py:419-422);
    the loop body is xd_test.py's line for line.  Per-video scores, ROC1, AP1 pin `harness.xd_test`; its
    Ano-AUC filter ('normal', xd_test.py:334) differs from test.py:336's and is recomputed by the test from the
    captured scores with sklearn."""
    import json
    sys.path.insert(0, REF)
    seed = 5
    tmp = tempfile.mkdtemp(prefix="iefvad_xd_")
    os.makedirs(os.path.join(tmp, "feat", "rgb"))
    os.makedirs(os.path.join(tmp, "feat", "event_thr_10"))
    rows = []
    for i, (n, c) in enumerate(zip(XD_LENGTHS, XD_LABELS)):
        img, ev = synth.make_video(seed, i, n)
        p = os.path.join(tmp, "feat", "rgb", f"v{i:03d}_label_{c}__5.npy")
        np.save(p, img)
        np.save(p.replace("rgb", "event_thr_10"), ev)
        rows.append((p, c))
    csv = os.path.join(tmp, "test.csv")
    with open(csv, "w") as f:
        f.write("path,label\n" + "".join(f"{p},{c}\n" for p, c in rows))
    gt = synth.make_gt(seed, int(sum(XD_LENGTHS)))
    with open(os.path.join(REF, "configs", "xd_label_map.json")) as f:
        label_map = json.load(f)
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        import test as ref_test
        from data.dataset import XD_Dataset
        from torch.utils.data import DataLoader
        model = build_reference(12, K=3)
        logits = []

        class Recorder(torch.nn.Module):
            def __init__(self, inner):
                super().__init__()
                self.inner = inner

            def forward(self, *a, **k):
                o = self.inner(*a, **k)
                logits.append(o["logits"].detach().clone())
                return o

        ref_test.label_map = label_map
        loader = DataLoader(XD_Dataset(256, csv, True, label_map), batch_size=1, shuffle=False)
        args = argparse.Namespace(exp_name="golden", dataset="xd")
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            roc, ap = ref_test.test(args, Recorder(model), loader, 256, None, gt, "cpu", attn=False, vis=False)
        print(buf.getvalue())
    finally:
        os.chdir(cwd)
    probs = [torch.sigmoid(lg.reshape(-1)[:n]).numpy() for lg, n in zip(logits, XD_LENGTHS)]
    path = os.path.join(HERE, "harness_xd.npz")
    np.savez_compressed(path, scores=np.concatenate(probs), lengths=np.array(XD_LENGTHS), labels=np.array(XD_LABELS),
                        classes=np.array([label_map[c.split('-')[0]] for c in XD_LABELS]),
                        map_keys=np.array(list(label_map.keys())), map_values=np.array(list(label_map.values())),
                        roc=np.array(roc), ap=np.array(ap), seed=np.array(seed), wseed=np.array(12), K=np.array(3),
                        stdout=np.array(buf.getvalue()))
    print("wrote", path, os.path.getsize(path), "B", "ROC", roc, "AP", ap)


VC_ROWS = [0, 1, 7, 64, 127, 128, 199, 200, 215, 216, 255]      # time steps kept of each sequence's outputs


def gen_vadclip_cases():
    """SURVEY 8 rows a12 / a13 (= f-5): the classes of /root/reference/model/layers.py and model/module.py, run HERE on the CPU -- dead
    code upstream, but importable (torch + scipy only) except DistanceAdj, which hard-codes .to('cuda') (layers.py:176,178) and stays
    unpinned.  Each class is constructed under a torch seed (the mirrors in iefvad_amd.layers / .module register and initialise their
    parameters in the same order, so the same seed gives the same tensors; checksums stored), perturbed by synth.perturb_module (biases
    and LayerNorm terms are trivial after the default init), and run on seeded inputs; OUTPUTS only are stored, a few time steps per
    sequence."""
    sys.path.insert(0, REF)
    import warnings
    warnings.simplefilter("ignore")
    from model import layers as RL                    # /root/reference/model/layers.py
    from model import module as RM                    # /root/reference/model/module.py
    out = {}

    def checks(mod):
        return np.array([[float(p.detach().double().sum()), float(p.detach().double().abs().sum())] for _, p in mod.named_parameters()])

    # SimilarityAdj(768, 384): seq_len None and given.  The 0.7 threshold is a discontinuity: the input seed is the first one for which
    # no similarity of a STORED row comes closer to it than 2e-5 (fp32 evaluation orders differ by ~1e-6; a row of adj, and a row of
    # every graph-layer output, depends on that row's similarities only)
    torch.manual_seed(101)
    sim = synth.perturb_module(RL.SimilarityAdj(768, 384), 1).eval()
    for xseed in range(3, 200):
        x = torch.from_numpy(synth.smooth_features(xseed, 2))
        with torch.no_grad():
            th = x @ sim.weight0
            cs = (th @ th.transpose(1, 2)) / (th.norm(dim=2, keepdim=True) @ th.norm(dim=2, keepdim=True).transpose(1, 2) + 1e-20)
        margin = float((cs[:, VC_ROWS] - 0.7).abs().min())
        if margin > 2e-5:
            break
    with torch.no_grad():
        adj_full = sim(x, None)
        adj_len = sim(x, [200, 256])
    out["x_seed"] = np.array(xseed)
    out["sim_checks"] = checks(sim)
    out["adj_full"] = adj_full[:, VC_ROWS].numpy()
    out["adj_len"] = adj_len[:, VC_ROWS].numpy()
    out["sim_threshold_margin"] = np.array(margin)
    out["sim_above_threshold"] = np.array(float((cs > 0.7).double().mean()))
    # GraphConvolution(768, 384): Conv1d residual; (384, 384): identity residual, with a bias
    torch.manual_seed(102)
    gc1 = synth.perturb_module(RL.GraphConvolution(768, 384, residual=True), 2).eval()
    torch.manual_seed(103)
    gc2 = synth.perturb_module(RL.GraphConvolution(384, 384, bias=True, residual=True), 3).eval()
    with torch.no_grad():
        y1 = gc1(x, adj_len)
        x1 = y1 * torch.sigmoid(1.702 * y1)          # the QuickGELU VadCLIP put between its graph layers
        y2 = gc2(x1, adj_len)
    out["gc1_checks"], out["gc2_checks"] = checks(gc1), checks(gc2)
    out["gc1_out"], out["gc1_gelu"], out["gc2_out"] = y1[:, VC_ROWS].numpy(), x1[:, VC_ROWS].numpy(), y2[:, VC_ROWS].numpy()
    # GraphAttentionLayer(768, 128): 256 nodes, a sparse adjacency with three empty rows (the -9e15 branch on a whole row)
    torch.manual_seed(104)
    gat = synth.perturb_module(RL.GraphAttentionLayer(768, 128, dropout=0.0, alpha=0.2, concat=True), 4).eval()
    g = torch.Generator().manual_seed(9)
    gadj = (torch.rand(256, 256, generator=g) < 0.1).float() * torch.rand(256, 256, generator=g)
    gadj[[5, 77, 255]] = 0
    with torch.no_grad():
        out["gat_out"] = gat(x[0], gadj).numpy()[VC_ROWS + [5, 77]]
    out["gat_checks"] = checks(gat)
    # ResidualAttentionBlock(768, 8) at [256, 2, 768]: plain; and with VadCLIP's block-diagonal window mask + a key padding mask
    xs = torch.from_numpy(synth.smooth_features(4, 2)).permute(1, 0, 2).contiguous() * 0.3
    torch.manual_seed(105)
    blk = synth.perturb_module(RM.ResidualAttentionBlock(768, 8, None), 5).eval()
    with torch.no_grad():
        yb, _ = blk((xs, None))
    out["blk_checks"] = checks(blk)
    out["blk_out"] = yb[VC_ROWS].numpy()
    win = 64
    mask = torch.full((256, 256), float("-inf"))
    for c in range(256 // win):
        mask[c * win:(c + 1) * win, c * win:(c + 1) * win] = 0
    pad = torch.zeros(2, 256, dtype=torch.bool)
    pad[1, 216:] = True
    torch.manual_seed(105)
    blk2 = synth.perturb_module(RM.ResidualAttentionBlock(768, 8, mask), 5).eval()
    with torch.no_grad():
        ym, _ = blk2((xs, pad))
    out["blk_masked_out"] = ym[VC_ROWS].numpy()        # queries 216.. of sequence 1 are padding themselves (still finite: their window holds real keys)
    out["rows"] = np.array(VC_ROWS)
    path = os.path.join(HERE, "vadclip_modules.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB; similarity margin to 0.7:", float(out["sim_threshold_margin"]),
          "fraction above:", float(out["sim_above_threshold"]), "finite:", {k: bool(np.isfinite(v).all()) for k, v in out.items() if v.dtype.kind == "f"})


SWEEP_LENGTHS = [40, 300, 17, 256, 90, 520]


def gen_sweep_case():
    """The robustness sweep's `run_test` (/root/reference/test2.py:35-123) on a small synthetic set, two
    levels drawn from one torch RNG stream (seed 0): IMG_NOISE 0.2 then EV_NOISE 0.3."""
    sys.path.insert(0, REF)
    import test2 as ref_test2                     # /root/reference/test2.py
    model = build_reference(11)
    seed = 4
    gt = synth.make_gt(seed, int(sum(SWEEP_LENGTHS)))

    def loader():
        for i, n in enumerate(SWEEP_LENGTHS):
            img, ev = synth.make_video(seed, i, n)
            from data.tools import process_split      # the reference's chunker
            ci, _ = process_split(img, 256)
            ce, _ = process_split(ev, 256)
            yield torch.tensor(ci).unsqueeze(0), torch.tensor(ce).unsqueeze(0), ("Normal",), torch.tensor([n])

    args = argparse.Namespace(visual_length=256)
    torch.manual_seed(0)
    out = {}
    for tag, kw in (("img02", dict(sigma_img=0.2, sigma_ev=0)), ("ev03", dict(sigma_img=0, sigma_ev=0.3))):
        r = ref_test2.run_test(args, model, loader(), gt, "cpu", **kw)
        out[tag + "_scalars"] = np.array([float(x) for x in r[:10]])
        out[tag + "_w_img_change"] = r[10].numpy()
        out[tag + "_w_ev_change"] = r[11].numpy()
    path = os.path.join(HERE, "sweep_test2.npz")
    np.savez_compressed(path, lengths=np.array(SWEEP_LENGTHS), seed=np.array(seed), wseed=np.array(11), **out)
    print("wrote", path, out["img02_scalars"])


def gen_init_checksums():
    """Default-initialised reference weights under torch.manual_seed(123): per-tensor sums and the first
    four elements, so the tests can check that iefvad_amd.MMFMIL registers and initialises its
    parameters in the reference's order (same RNG stream -> identical tensors)."""
    sys.path.insert(0, REF)
    from model.imf_vad import MMFMIL
    out = {}
    for K in (10, 0):
        torch.manual_seed(123)
        m = MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, device="cpu", args=ref_args(2, 8, K))
        sd = m.state_dict()
        out[f"keys_k{K}"] = np.array(list(sd.keys()))
        out[f"sums_k{K}"] = np.array([float(v.double().sum()) for v in sd.values()])
        out[f"head_k{K}"] = np.stack([np.resize(v.reshape(-1)[:4].double().numpy(), 4) for v in sd.values()])
    path = os.path.join(HERE, "init_checksums.npz")
    np.savez_compressed(path, **out)
    print("wrote", path)


def gen_config5_gt():
    """BASELINE config 5's REAL ground truth: the two frame-level gt arrays the reference ships
    (/root/reference/list/shang/rgb/vitl/gt.npy, 139,568 frames = 8,723 snippets; list/msad/rgb/vitl/gt.npy, 144,144
    frames = 9,009 snippets; both float64 0/1), bit-packed, plus the label column of the two test lists
    (list/{shang,msad}/rgb/vitl/test.csv: 197 and 241 videos, in list order).  Data only: no feature file exists for these
    lists in the container, so the videos' lengths stay synthetic (synth.config5_lists makes them sum to the gt exactly)."""
    out = {}
    for d in ("shang", "msad"):
        gt = np.load(os.path.join(REF, "list", d, "rgb", "vitl", "gt.npy"))          # allow_pickle=False (default)
        assert gt.dtype == np.float64 and set(np.unique(gt)) <= {0.0, 1.0} and len(gt) % 16 == 0
        out[f"{d}_bits"] = np.packbits(gt.astype(np.uint8))
        out[f"{d}_frames"] = np.array(len(gt))
        with open(os.path.join(REF, "list", d, "rgb", "vitl", "test.csv")) as f:
            rows = [ln.rstrip("\n").rsplit(",", 1) for ln in f][1:]
        out[f"{d}_labels"] = np.array([r[1] for r in rows])
    path = os.path.join(HERE, "config5_gt.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB", {k: (v.shape if v.ndim else int(v)) for k, v in out.items()})


def gen_loss_case():
    """f-4: the trainers' loss terms on seeded stand-ins of a batch's model outputs.  CLAS2 is the reference's own
    function (/root/reference/train/loss.py:18-30 imports only torch); the trainer modules cannot be imported (wandb), so the
    regulariser and KL terms are evaluated here with the torch calls train/ucf_train.py:75-98 makes, in its order.  Outputs only."""
    import math
    import torch.nn.functional as F
    sys.path.insert(0, REF)
    from train.loss import CLAS2
    store = {}
    for seed in (1, 2):
        o, labels, lengths = synth.make_loss_inputs(seed)
        t = {k: torch.from_numpy(v) for k, v in o.items()}
        cls = CLAS2(t["logits"], torch.from_numpy(labels), torch.from_numpy(lengths), "cpu")
        image_mu, event_mu = t["image_mu"], t["event_mu"]
        cos_sim = F.cosine_similarity(F.normalize(image_mu, p=2, dim=-1), F.normalize(event_mu, p=2, dim=-1), dim=-1)   # :75-77
        loss_cos = (1 - cos_sim).mean()                                                                                 # :78,82
        loss_norm = torch.abs(torch.norm(image_mu, p=2, dim=-1) - torch.norm(event_mu, p=2, dim=-1)).mean()            # :79-82
        vals = [float(cls), float(loss_cos), float(loss_norm)]
        for noise, nu in (("Gaussian", 8), ("StudentT", 8), ("StudentT", 5)):
            sh = math.log(nu / (nu + 1)) if noise == "StudentT" else 0.0                                                # :94-95
            kl = []
            for mu, lv in ((image_mu, t["image_logvar"]), (event_mu, t["event_logvar"])):
                e = lv + sh
                kl.append(float(-0.5 * torch.mean(1 + e - mu.pow(2) - e.exp())))                                        # :88-89,96-97
            vals += kl
        store[f"seed{seed}"] = np.array(vals, np.float64)
    store["layout"] = np.array("classification, cos, norm, kl_image Gaussian, kl_event Gaussian, kl_image StudentT nu=8, kl_event, "
                               "kl_image StudentT nu=5, kl_event")
    path = os.path.join(HERE, "loss_terms.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, store["seed1"])


def gen_loss_grad_case():
    """f-4, backward of the loss head: autograd through the reference's own CLAS2 (/root/reference/train/loss.py:18-30) and the
    trainers' torch calls (train/ucf_train.py:75-101) on the seeded stand-ins of gen_loss_case, evaluated in fp64.  Stored: 2048
    sampled gradient entries per tensor (seeded indices; for d logits only from videos without tied scores -- with ties
    torch.topk's choice among equals decides who gets the gradient), the per-video sums of d logits (tie-invariant), the whole
    gradient row of the all-zero image_mu row (the clamp branches of F.normalize / F.cosine_similarity) and the abs-sums."""
    import math
    import torch.nn.functional as F
    sys.path.insert(0, REF)
    from train.loss import CLAS2
    store = {}
    for seed, noise, nu, lam_reg, lam_kl in ((1, "StudentT", 8, 1.0, 1.0), (2, "Gaussian", 8, 0.01, 0.01)):
        o, labels, lengths = synth.make_loss_inputs(seed)
        t = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in o.items()}
        cls = CLAS2(t["logits"], torch.from_numpy(labels).double(), torch.from_numpy(lengths), "cpu")
        image_mu, event_mu = t["image_mu"], t["event_mu"]
        cos_sim = F.cosine_similarity(F.normalize(image_mu, p=2, dim=-1), F.normalize(event_mu, p=2, dim=-1), dim=-1)   # :75-77
        loss_cos = (1 - cos_sim).mean()
        loss_norm = torch.abs(torch.norm(image_mu, p=2, dim=-1) - torch.norm(event_mu, p=2, dim=-1)).mean()
        sh = math.log(nu / (nu + 1)) if noise == "StudentT" else 0.0
        kl = 0.0
        for mu, lv in ((image_mu, t["image_logvar"]), (event_mu, t["event_logvar"])):
            e = lv + sh
            kl = kl + (-0.5 * torch.mean(1 + e - mu.pow(2) - e.exp()))
        total = cls + lam_reg * (loss_cos + loss_norm) + lam_kl * kl                                                   # :100-102
        total.backward()
        rng = np.random.default_rng([seed, 77])
        tag = f"seed{seed}"
        store[tag + "_cfg"] = np.array([nu, lam_reg, lam_kl, 1.0 if noise == "StudentT" else 0.0])
        store[tag + "_total"] = np.array(float(total))
        for k in ("logits", "image_mu", "event_mu", "image_logvar", "event_logvar"):
            g = t[k].grad.numpy().reshape(-1)
            if k == "logits":
                B, T = t[k].shape[0], t[k].shape[1]
                ok = [v for v in range(B) if v not in (0, 2)]                  # videos 0 and 2 hold exactly tied scores
                idx = np.concatenate([v * T + rng.choice(T, 256, replace=False) for v in ok])
                store[tag + "_logits_video_sums"] = t[k].grad.numpy().reshape(B, T).sum(1)
            else:
                idx = rng.choice(g.size, 2048, replace=False)
                idx = idx[(idx // 768) != (1 * 256 + 5)]                       # the zero row is stored whole below
            store[tag + "_" + k + "_idx"] = idx.astype(np.int64)
            store[tag + "_" + k + "_val"] = g[idx]
            store[tag + "_" + k + "_abssum"] = np.array(np.abs(g[np.isfinite(g)]).sum())
        store[tag + "_image_mu_zero_row"] = t["image_mu"].grad.numpy()[1, 5]
        store[tag + "_event_mu_zero_row"] = t["event_mu"].grad.numpy()[1, 5]
    path = os.path.join(HERE, "loss_grads.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes;", float(store["seed1_total"]), np.abs(store["seed1_image_mu_zero_row"]).max())


# (name, weight seed, batch seed, B, L, K, noise, nu, lambda_reg, lambda_kl, dropout p with an injected mask (0 = no dropout),
#  synth.sharpen_qk factors or None)
GRAD_CASES = [
    ("k2_student8", 31, 41, 3, 2, 2, "StudentT", 8, 1.0, 1.0, 0.0, None),
    ("k10_student8_mask", 32, 42, 2, 2, 10, "StudentT", 8, 1.0, 1.0, 0.1, None),
    ("k0_gauss_l1", 33, 43, 2, 1, 0, "Gaussian", 8, 0.01, 0.01, 0.0, None),
    ("sharp_k2_student8", 31, 41, 3, 2, 2, "StudentT", 8, 1.0, 1.0, 0.0, (8, 4)),     # the softmax backward where P is not ~ 1/256
]
GRAD_SAMPLES = 192


def _reference_train_model(wseed, L, K, noise, nu, dtype, p, mask, factors=None):
    """The reference MMFMIL in train() mode with seeded weights.  Attention dropout: every nn.MultiheadAttention's `.dropout` is
    set to `p`; for p > 0 torch.nn.functional.dropout is replaced, for the duration of the caller's forward, by a function that
    applies the NEXT injected keep mask exactly as F.dropout applies its own (x * mask / (1 - p)) -- so the reference and the
    build see the same mask.  Returns (model, context manager)."""
    import contextlib
    import torch.nn.functional as F
    model = build_reference(wseed, L, K, 0.5, noise, nu, factors)
    model = model.to(dtype)
    model.train()
    for mod in list(model.temporal.image_attn_layers) + list(model.temporal.event_attn_layers):
        mod.dropout = float(p)

    @contextlib.contextmanager
    def inject():
        if p <= 0:
            yield
            return
        # forward order of imf_vad.py:113-123: image layers 0..L-1, then event layers 0..L-1; mask is [2, L, B, H, T, T]
        queue = [torch.from_numpy(mask[m, l]).reshape(-1, 256, 256).to(dtype) for m in range(2) for l in range(L)]
        orig = F.dropout

        def fake(x, p=0.5, training=True, inplace=False):
            keep = queue.pop(0)
            assert keep.shape == x.shape
            return x * keep * (1.0 / (1.0 - p))

        F.dropout = fake
        try:
            yield
            assert not queue, "every injected mask must have been consumed"
        finally:
            F.dropout = orig
    return model, inject


def _trainer_loss(outputs, labels, lengths, noise, nu, lam_reg, lam_kl, CLAS2):
    """The total the trainers form (/root/reference/train/ucf_train.py:68-102, xd_train.py:54-75), with the reference's own CLAS2."""
    import math
    import torch.nn.functional as F
    image_mu, event_mu = outputs["image_mu"], outputs["event_mu"]
    cls = CLAS2(outputs["logits"], labels, lengths, "cpu")
    cos_sim = F.cosine_similarity(F.normalize(image_mu, p=2, dim=-1), F.normalize(event_mu, p=2, dim=-1), dim=-1)
    loss_reg = (1 - cos_sim).mean() + torch.abs(torch.norm(image_mu, p=2, dim=-1) - torch.norm(event_mu, p=2, dim=-1)).mean()
    sh = math.log(nu / (nu + 1)) if noise == "StudentT" else 0.0
    kl = 0.0
    for mu, lv in ((image_mu, outputs["image_logvar"]), (event_mu, outputs["event_logvar"])):
        e = lv + sh
        kl = kl + (-0.5 * torch.mean(1 + e - mu.pow(2) - e.exp()))
    return cls + lam_reg * loss_reg + lam_kl * kl


def gen_model_grad_cases(only=None):
    """f-4, the model's backward pass: the REFERENCE model in train() mode (fp64 copy), the reference's own CLAS2 and the trainers'
    torch calls, `loss.backward()` -- every parameter gradient of SURVEY.md Appendix B.  Stored per parameter: its L1 and L2
    norms and GRAD_SAMPLES seeded entries; plus the total loss and the logits (forward check of the train-mode path)."""
    sys.path.insert(0, REF)
    from train.loss import CLAS2
    for name, wseed, bseed, B, L, K, noise, nu, lam_reg, lam_kl, p, factors in GRAD_CASES:
        if only and name not in only:
            continue
        mask = synth.make_dropout_mask(bseed, L, B, p) if p > 0 else None
        model, inject = _reference_train_model(wseed, L, K, noise, nu, torch.float64, p, mask, factors)
        img, ev, labels, lengths = synth.make_train_batch(bseed, B)
        with inject():
            # MMFMIL.forward (imf_vad.py:40-44) is `.to(torch.float)` + this call; entering one level below keeps the graph in fp64
            out = model.temporal(torch.from_numpy(img).double(), torch.from_numpy(ev).double())
        total = _trainer_loss(out, torch.from_numpy(labels).double(), torch.from_numpy(lengths), noise, nu, lam_reg, lam_kl, CLAS2)
        total.backward()
        store = {"cfg": np.array([wseed, bseed, B, L, K, nu]), "noise": np.array(noise), "lams": np.array([lam_reg, lam_kl]),
                 "p": np.array(p), "total": np.array(float(total)), "logits": out["logits"].detach().numpy().reshape(B, 256)}
        if factors is not None:
            store["factors"] = np.array(factors, np.float64)
        names = []
        for i, (key, prm) in enumerate(model.named_parameters()):
            g = prm.grad.numpy().reshape(-1)
            rng = np.random.default_rng([bseed, 900 + i])
            idx = np.sort(rng.choice(g.size, min(g.size, GRAD_SAMPLES), replace=False))
            names.append(key)
            store[f"g{i}_idx"] = idx.astype(np.int64)
            store[f"g{i}_val"] = g[idx]
            store[f"g{i}_norms"] = np.array([np.abs(g).sum(), np.sqrt((g * g).sum()), np.abs(g).max()])
        if factors is not None:
            # the reference's OWN fp32 autograd (what its trainers run) against the fp64 gradients just stored, in units of the gate of
            # tests/test_gpu_train.py (1e-4 |want| + 1e-6 max|grad| per sampled entry), worst over all parameters: the floor of the
            # number format on this case.  One thread, so that the summation order -- and with it this field -- reproduces.
            threads = torch.get_num_threads()
            torch.set_num_threads(1)
            m32, _ = _reference_train_model(wseed, L, K, noise, nu, torch.float32, p, mask, factors)
            o32 = m32.temporal(torch.from_numpy(img), torch.from_numpy(ev))
            _trainer_loss(o32, torch.from_numpy(labels), torch.from_numpy(lengths), noise, nu, lam_reg, lam_kl, CLAS2).backward()
            torch.set_num_threads(threads)
            floor = 0.0
            for i, (key, prm) in enumerate(m32.named_parameters()):
                g32 = prm.grad.double().numpy().reshape(-1)[store[f"g{i}_idx"]]
                want = store[f"g{i}_val"]
                floor = max(floor, float((np.abs(g32 - want) / (1e-4 * np.abs(want) + 1e-6 * store[f"g{i}_norms"][2])).max()))
            store["grad_floor"] = np.array(floor)
            print("reference fp32 autograd vs fp64, worst sampled entry in units of the 1e-4 gate:", floor)
        store["names"] = np.array(names)
        path = os.path.join(HERE, f"grad_{name}.npz")
        np.savez_compressed(path, **store)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB; total", float(total), "params", len(names))


STEP_CASE = ("k3_student8", 34, 44, 4, 2, 3, "StudentT", 8, 1.0, 1.0, 2)       # ... , optimiser steps


def gen_train_step_case():
    """One (and a second) whole step of /root/reference/train/ucf_train.py:60-106 by the reference in its own arithmetic (fp32):
    model.train() with the attention dropout at 0, forward, CLAS2 + regulariser + KL, loss.backward(),
    torch.optim.AdamW(model.parameters(), lr=2e-5).step() (main.py:69's default lr, the trainers' AdamW defaults).  Stored:
    the losses, and GRAD_SAMPLES seeded entries of every parameter after each step."""
    sys.path.insert(0, REF)
    from train.loss import CLAS2
    name, wseed, bseed, B, L, K, noise, nu, lam_reg, lam_kl, nsteps = STEP_CASE
    model, inject = _reference_train_model(wseed, L, K, noise, nu, torch.float32, 0.0, None)
    opt = torch.optim.AdamW(model.parameters(), lr=2e-5)
    store = {"cfg": np.array([wseed, bseed, B, L, K, nu, nsteps]), "noise": np.array(noise), "lams": np.array([lam_reg, lam_kl]),
             "lr": np.array(2e-5)}
    losses = []
    for step in range(nsteps):
        img, ev, labels, lengths = synth.make_train_batch(bseed + step, B)
        out = model(torch.from_numpy(img), torch.from_numpy(ev), None, None, torch.from_numpy(lengths))
        total = _trainer_loss(out, torch.from_numpy(labels), torch.from_numpy(lengths), noise, nu, lam_reg, lam_kl, CLAS2)
        opt.zero_grad()
        total.backward()
        opt.step()
        losses.append(float(total))
        for i, (key, prm) in enumerate(model.named_parameters()):
            v = prm.detach().numpy().reshape(-1)
            rng = np.random.default_rng([bseed, 700 + i])
            idx = np.sort(rng.choice(v.size, min(v.size, GRAD_SAMPLES), replace=False))
            if step == 0:
                store[f"p{i}_idx"] = idx.astype(np.int64)
            store[f"p{i}_step{step}"] = v[idx].copy()
    store["names"] = np.array([k for k, _ in model.named_parameters()])
    store["losses"] = np.array(losses)
    path = os.path.join(HERE, f"train_step_{name}.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB; losses", losses)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "modelgrad":
        gen_model_grad_cases(sys.argv[2:])
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "trainstep":
        gen_train_step_case()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "lossgrad":
        gen_loss_grad_case()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "loss":
        gen_loss_case()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "config5":
        gen_config5_gt()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "init":
        gen_init_checksums()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "sharp":
        gen_sharp_cases(sys.argv[2:])
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "b48":
        gen_forward_cases([BIG_CASE], BIG_CASE_CHUNKS)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "vadclip":
        gen_vadclip_cases()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "xd":
        gen_harness_xd_case()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "sweep":
        gen_sweep_case()
        sys.exit(0)
    torch.manual_seed(0)
    gen_forward_cases()
    gen_forward_cases([BIG_CASE], BIG_CASE_CHUNKS)
    gen_sharp_cases()
    gen_harness_case()
    gen_harness_xd_case()
    gen_init_checksums()
    gen_sweep_case()
    gen_config5_gt()
    gen_loss_case()
    gen_loss_grad_case()
    gen_model_grad_cases()
    gen_train_step_case()
    gen_vadclip_cases()
