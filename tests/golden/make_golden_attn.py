"""Reference captures of the encoder's head-averaged attention maps.  Run once on CPU with the reference importable:

    python tests/golden/make_golden_attn.py

The reference computes the maps on every call and discards them: `nn.MultiheadAttention(...)(x, x, x)` at imf_vad.py:115,121 runs with
need_weights=True and the second result is dropped (`attn_out, _ = ...`).  A forward hook on `temporal.image_attn_layers[l]` /
`temporal.event_attn_layers[l]` captures that second result, [B, 256, 256] per layer and modality.  The model is run twice on the same
seeded weights and inputs: in fp32 through MMFMIL.forward, and in fp64 (`model.temporal.double()` on fp64 inputs; MMFMIL.forward itself
casts to float, imf_vad.py:41-42).  Stored, per file (weights and inputs are regenerated from the seeds by the tests):
  rows        [B, 16] the query rows kept of each chunk: seeded, and always row 0, the last valid row (99) and a pad row (200) of the
              edited chunk
  image, event  [L, B, 16, 256] fp64: the fp64 run's maps at those query rows, all 256 keys
  attn_floor  [2, L] max |fp32 run - fp64 run| over the FULL maps (modality, layer): the reference's own fp32 error
  attn_max    [2, L] the largest weight of the fp64 run's full maps (flat regime ~ 1/256; the sharp fixtures are required >= 0.1)
  meta        wseed, iseed, B, L, K, D; factors (the sharp fixtures: synth.sharpen_qk)
Files: attn_flat_k3.npz, attn_sharp_k3.npz (D = 768) and vitb_attn_sharp_k3.npz (D = 512, head dim 64); the last chunk has rows 100..
zeroed in all of them.  No reference source is stored."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, ref_args  # noqa: E402
from iefvad_amd import synth  # noqa: E402

WSEED, ISEED, B, L, K = 5, 7, 2, 2, 3
VALID_LAST = 100          # rows 100.. of the last chunk are zero
NROWS = 16
FACTORS = (8, 4)
# (file, D, factors)
CASES = [("attn_flat_k3", 768, None), ("attn_sharp_k3", 768, FACTORS), ("vitb_attn_sharp_k3", 512, FACTORS)]


def query_rows():
    """[B, NROWS] sorted query rows per chunk; the edited (last) chunk always has 0, VALID_LAST - 1 and the pad row 200."""
    rng = np.random.default_rng([WSEED, ISEED, 99])
    rows = []
    for b in range(B):
        must = [0, VALID_LAST - 1, 200] if b == B - 1 else [0, 255]
        rest = [r for r in rng.permutation(256) if r not in must][: NROWS - len(must)]
        rows.append(sorted(must + [int(r) for r in rest]))
    return np.asarray(rows, np.int64)


def case_inputs(D):
    img, ev = synth.make_inputs(ISEED, B, D=D)
    img[B - 1, VALID_LAST:] = 0
    ev[B - 1, VALID_LAST:] = 0
    return img, ev


def hooked_maps(model, run):
    """{(modality, layer): [B, 256, 256] tensor}: the second result of every attention module's call during `run()`."""
    got, handles = {}, []
    for m, name in enumerate(("image", "event")):
        for l, mod in enumerate(getattr(model.temporal, f"{name}_attn_layers")):
            handles.append(mod.register_forward_hook(lambda _mod, _inp, out, key=(m, l): got.__setitem__(key, out[1].detach().clone())))
    try:
        with torch.no_grad():
            run()
    finally:
        for h in handles:
            h.remove()
    return got


def capture(name, D, factors):
    sys.path.insert(0, REF)
    from model.imf_vad import MMFMIL  # the reference model
    sd = synth.make_state_dict(WSEED, D, L, K)
    if factors is not None:
        sd = synth.sharpen_qk(sd, factors)
    img, ev = case_inputs(D)
    model = MMFMIL(14, D, 256, D, 8, L, 8, 10, 10, device="cpu", args=ref_args(L, 8, K))
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.eval()
    m32 = hooked_maps(model, lambda: model(torch.from_numpy(img), torch.from_numpy(ev), None, None, None))
    model.double()
    m64 = hooked_maps(model, lambda: model.temporal(torch.from_numpy(img).double(), torch.from_numpy(ev).double()))
    rows = query_rows()
    floor, amax = np.zeros((2, L)), np.zeros((2, L))
    kept = np.zeros((2, L, B, NROWS, 256), np.float64)
    for (m, l), a64 in m64.items():
        assert a64.dtype == torch.float64 and tuple(a64.shape) == (B, 256, 256) and m32[(m, l)].dtype == torch.float32
        assert float((a64.sum(-1) - 1).abs().max()) < 1e-12
        floor[m, l] = float((m32[(m, l)].double() - a64).abs().max())
        amax[m, l] = float(a64.max())
        for b in range(B):
            kept[m, l, b] = a64[b, rows[b]].numpy()
    out = dict(rows=rows, image=kept[0], event=kept[1], attn_floor=floor, attn_max=amax,
               meta=np.asarray([WSEED, ISEED, B, L, K, D], np.int64))
    if factors is not None:
        out["factors"] = np.asarray(factors, np.float64)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path)} bytes; floor {floor.min():.2e} .. {floor.max():.2e}; max weight {amax.min():.4f} .. {amax.max():.4f}")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    for case in CASES:
        capture(*case)
