"""Reference captures at D = 512 (ViT-B/16 features, the reference's `--ds vitb_rgb`: embed_dim = visual_width = 512, visual_head = 8,
head dim 64; the reference's parser.py, update_ucf_args).  Run once on CPU with the reference importable:

    python tests/golden/make_golden_vitb.py

It builds the reference's MMFMIL(14, 512, 256, 512, 8, L, ...) with seeded weights (synth.make_state_dict(seed, 512, L, K), loaded
strictly) and writes reference outputs only -- weights and inputs are regenerated from the seeds by the tests:
  vitb_fwd_*.npz   logits, w_i / w_e row means and ROW_SUBSET rows of the seven 512-wide outputs of one forward
  vitb_harness.npz the reference's own test.test() loop on 14 synthetic .npy videos (one per UCF class key): scores, AUC, AP, Ano-AUC, printed lines
The files are named vitb_* so that tests/helpers.golden_cases() (fwd_*.npz, the D = 768 parity cases) does not pick them up."""
import argparse
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import BIG_KEYS, REF, ROW_SUBSET, ref_args, sharp_fields  # noqa: E402
from iefvad_amd import synth  # noqa: E402

D = 512

# (name, weight seed, input seed, B, L, K, lambda, noise, nu, input dtype, input edit)
CASES = [
    ("base", 31, 41, 3, 2, 10, 0.5, "StudentT", 8, "f32", "tail"),       # chunk 2 zero after row 100
    ("k0_gauss_l1", 32, 42, 1, 1, 0, 0.5, "Gaussian", 8, "f32", None),
    ("f16_k3", 33, 43, 2, 2, 3, 0.3, "StudentT", 5, "f16", None),
]

# Peaked attention at head dim 64 (the d64 kernels; make_golden.SHARP_CASES has the regime's description).  Factors tried on the CPU
# with `python make_golden_vitb.py try F0 F1` (max |score| layer 0 / 1, mean max P layer 0 / 1, image modality):
#   (8, 4)   23 / 27    0.44 / 0.61     chosen: same factors as D = 768, every layer's mean max P >= 0.3, floors 4.1e-6 / 1.1e-6 / 2.7e-7
#   (12, 6)  52 / 60    0.65 / 0.85     floor_big 5.7e-6
#   (8, 8)   23 / 109   0.44 / 0.89     floor_big 7.4e-6: 3 x floor passes the 2e-5 gate
#   (16, 4)  93 / 27    0.76 / 0.66     the overflow regime; floor_big 8.1e-6
SHARP_CASE = ("sharp_k3", 31, 41, 3, 2, 3, 0.5, "StudentT", 8, "f32", "tail", (8, 4))

# the harness capture: the five lengths around the chunk edge and one long video first, then short videos so that every UCF
# class key has one (test.py:166-167 concatenates every class's list)
HARNESS_SEED, HARNESS_WSEED = 5, 31
HARNESS_LENGTHS = [37, 256, 1, 257, 640, 20, 64, 100, 12, 300, 8, 50, 129, 90]
HARNESS_CLASSES = list(synth.UCF_CLASSES)


def build_reference_vitb(seed, L=2, K=10, lam=0.5, noise="StudentT", nu=8, factors=None):
    sys.path.insert(0, REF)
    from model.imf_vad import MMFMIL  # the reference model
    model = MMFMIL(14, D, 256, D, 8, L, 8, 10, 10, device="cpu", args=ref_args(L, 8, K, lam, noise, nu))
    sd = synth.make_state_dict(seed, D, L, K)
    if factors is not None:
        sd = synth.sharpen_qk(sd, factors)
    missing = model.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    model.eval()
    return model


def case_inputs(in_seed, B, dtype, edit):
    img, ev = synth.make_inputs(in_seed, B, D=D)
    if edit == "tail":
        img[B - 1, 100:] = 0
        ev[B - 1, 100:] = 0
    if dtype == "f16":
        img, ev = img.astype(np.float16), ev.astype(np.float16)
    return img, ev


def gen_forward_cases(cases=None):
    for name, wseed, iseed, B, L, K, lam, noise, nu, dt, edit, *factors in (cases or CASES):
        factors = factors[0] if factors else None
        model = build_reference_vitb(wseed, L, K, lam, noise, nu, factors)
        img, ev = case_inputs(iseed, B, dt, edit)
        with torch.no_grad():
            out = model(torch.from_numpy(img), torch.from_numpy(ev), None, None, None)
        fields = sharp_fields(model, img, ev, out, factors, L, D)[0] if factors else {}
        store = {**fields, "logits": out["logits"].numpy().reshape(B, 256),
                 "w_i_mean": out["w_i"].mean(dim=-1).numpy(), "w_e_mean": out["w_e"].mean(dim=-1).numpy(),
                 "rows": np.array(ROW_SUBSET),
                 "meta": np.array([wseed, iseed, B, L, K, nu]), "lam": np.array(lam),
                 "noise": np.array(noise), "in_dtype": np.array(dt), "edit": np.array(str(edit))}
        for k in BIG_KEYS:
            assert out[k].shape == (B, 256, D)
            store[k] = out[k].numpy()[:, ROW_SUBSET, :]
        path = os.path.join(HERE, f"vitb_fwd_{name}.npz")
        np.savez_compressed(path, **store)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB", {k: np.round(v, 9).tolist() for k, v in fields.items()})


def write_harness_set(tmp):
    """The .npy videos of the harness capture under `tmp` (the layout of make_golden.gen_harness_case); returns the list csv."""
    rows = []
    for i, (n, c) in enumerate(zip(HARNESS_LENGTHS, HARNESS_CLASSES)):
        img, ev = synth.make_video(HARNESS_SEED, i, n, D=D)
        d_rgb = os.path.join(tmp, "feat", "rgb", c)
        os.makedirs(d_rgb, exist_ok=True)
        os.makedirs(os.path.join(tmp, "feat", "event_thr_10", c), exist_ok=True)
        p = os.path.join(d_rgb, f"v{i:03d}__5.npy")
        np.save(p, img)
        np.save(p.replace("rgb", "event_thr_10"), ev)
        rows.append((p, c))
    csv = os.path.join(tmp, "test.csv")
    with open(csv, "w") as f:
        f.write("path,label\n")
        for p, c in rows:
            f.write(f"{p},{c}\n")
    return csv


def gen_harness_case():
    """The reference's test.test() (test.py:46-212) on the D = 512 model; follows make_golden.gen_harness_case."""
    sys.path.insert(0, REF)
    tmp = tempfile.mkdtemp(prefix="iefvad_vitb_")
    csv = write_harness_set(tmp)
    gt = synth.make_gt(HARNESS_SEED, int(sum(HARNESS_LENGTHS)))
    cwd = os.getcwd()
    os.chdir(tmp)     # test() does os.makedirs('vis') (test.py:59-62)
    try:
        import test as ref_test                      # the reference's test.py
        from data.dataset import UCF_Dataset         # the reference's data/dataset.py
        from torch.utils.data import DataLoader
        model = build_reference_vitb(HARNESS_WSEED)
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
    probs = [torch.sigmoid(lg.reshape(-1)[:n]).numpy() for lg, n in zip(captured["logits"], HARNESS_LENGTHS)]
    path = os.path.join(HERE, "vitb_harness.npz")
    np.savez_compressed(path, scores=np.concatenate(probs), lengths=np.array(HARNESS_LENGTHS), classes=np.array(HARNESS_CLASSES),
                        roc=np.array(roc), ap=np.array(ap), ano_auc=np.array(captured["ano"]), seed=np.array(HARNESS_SEED),
                        wseed=np.array(HARNESS_WSEED), chunks=np.array([lg.shape[0] for lg in captured["logits"]]),
                        stdout=np.array(buf.getvalue()))
    print("wrote", path, os.path.getsize(path) // 1024, "KiB", "ROC", roc, "AP", ap, "ano", captured["ano"])


if __name__ == "__main__":
    torch.manual_seed(0)
    if len(sys.argv) > 1 and sys.argv[1] == "sharp":
        gen_forward_cases([SHARP_CASE])
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "try":       # python make_golden_vitb.py try 8 4: the statistics only
        gen_forward_cases([("try", *SHARP_CASE[1:-1], tuple(float(f) for f in sys.argv[2:]))])
        os.remove(os.path.join(HERE, "vitb_fwd_try.npz"))
        sys.exit(0)
    gen_forward_cases()
    gen_forward_cases([SHARP_CASE])
    gen_harness_case()
