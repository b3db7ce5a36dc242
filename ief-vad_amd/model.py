"""Drop-in `MMFMIL` for the reference's evaluation loops, backed by libiefvad.so.

Mirrors the interface of /root/reference/model/imf_vad.py:
  * constructor signature of `MMFMIL` (:6-18) and the hyper-parameters it forwards (:30-38);
  * `state_dict()` keys and shapes so `load_state_dict(torch.load(ckpt))`
    (/root/reference/test.py:377-378) works unchanged;
  * `forward(img, ev, padding_mask, text, lengths, return_attn=False) -> dict` with the eight keys of
    :152-161; `padding_mask`, `text`, `lengths`, `return_attn` are accepted and ignored (:40-44);
  * attribute `model.temporal.nu` read by the training loss (/root/reference/train/ucf_train.py:94-95);
  * `ValueError` for an unsupported `noise_model`, raised at forward time (:137-138).

The modules below only HOLD parameters (same names, shapes and default initialisation as the
torch.nn modules the reference instantiates); no torch op computes the forward.  Inputs must live
on a HIP device: there is no CPU path, a CPU tensor raises.

`model.train()` switches `forward` to the train-mode path (attention dropout, activations kept for the backward): the returned
tensors are differentiable with respect to every parameter, `loss.backward()` runs `iefvad_train_backward`.
A feature tensor that requires grad receives its gradient too (`iefvad_train_backward_inputs`), in train() and -- dropout off -- in eval().
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import lib as _lib

_IN_DTYPES = {torch.float32: _lib.IN_F32, torch.float16: _lib.IN_F16, torch.bfloat16: _lib.IN_BF16}
OUTPUT_KEYS = ("fused", "logits", "image_mu", "event_mu", "image_logvar", "event_logvar", "w_i", "w_e")
WIDE_KEYS = tuple(k for k in OUTPUT_KEYS if k != "logits")      # the seven [rows, D] tensors


def _row_output_keys(outputs) -> tuple:
    """`outputs=` of the valid-row calls -> the [rows, D] keys asked for, in OUTPUT_KEYS order: None -> none, "full" -> all seven, else a
    key or an iterable of keys from OUTPUT_KEYS ("logits" is returned anyway)."""
    if outputs is None:
        return ()
    if outputs == "full":
        return WIDE_KEYS
    names = [outputs] if isinstance(outputs, str) else list(outputs)
    bad = [k for k in names if k not in OUTPUT_KEYS]
    if bad:
        raise ValueError(f'unknown output key(s) {bad}: outputs= takes "full" or names from OUTPUT_KEYS {OUTPUT_KEYS}')
    return tuple(k for k in WIDE_KEYS if k in names)


# The valid-row entries by the suffix of their names (`iefvad_forward_videos<suffix>`, `iefvad_forward_videos_host<suffix>`), each with:
# the device entry's workspace query (`iefvad_videos<query>_workspace_bytes`) and its arguments behind (handle, lengths, nvideos); the
# entry's arguments behind the common head.  `r` holds the call's pointers (`MMFMIL._rows_call` sets every key; None = not asked for).
_ROW_ENTRIES = {
    "": ("", lambda r: (), lambda r: (*r["vectors"], r["stream"])),
    "_similarity": ("", lambda r: (), lambda r: (*r["vectors"], r["stream"], r["similarity"])),
    "_full": ("_full", lambda r: (r["out"],), lambda r: (r["out"], r["stream"])),
    "_scaled": ("_scaled", lambda r: (r["with_colsum"],), lambda r: (*r["vectors"], r["w_colsum"], r["stream"])),
    "_perturbed": ("_scaled", lambda r: (r["with_colsum"],), lambda r: (*r["vectors"], r["w_colsum"], r["stream"])),
    "_attn": ("", lambda r: (), lambda r: (*r["vectors"], r["attn"], r["stream"])),
    "_trajectory": ("_trajectory", lambda r: (), lambda r: (*r["vectors"], r["trajectory"], r["stream"])),
    "_variants": ("_variants", lambda r: (r["nvariants"],), lambda r: (*r["vectors"], r["variants"], r["stream"])),
}


def fusion_variant_names(fusion_variants) -> tuple:
    """`fusion_variants=` -> the names asked for, in the caller's order: None / False -> none, True -> all four in the order of
    `lib.VARIANT_NAMES` ("fused", "image", "event", "equal"), else a name or an iterable of names, each at most once (ValueError
    otherwise)."""
    if fusion_variants is None or fusion_variants is False:
        return ()
    if fusion_variants is True:
        return tuple(_lib.VARIANT_NAMES)
    try:
        names = [fusion_variants] if isinstance(fusion_variants, str) else list(fusion_variants)
    except TypeError:
        raise ValueError(f"fusion_variants takes True or an iterable of names from {_lib.VARIANT_NAMES} (got {fusion_variants!r})") from None
    bad = [n for n in names if n not in _lib.VARIANT_NAMES]
    if bad or not names:
        raise ValueError(f"unknown fusion variant(s) {bad}: fusion_variants takes True or names from {_lib.VARIANT_NAMES} (got {fusion_variants!r})")
    if len(set(names)) != len(names):
        raise ValueError(f"fusion_variants names a variant more than once: {names}")
    return tuple(names)


def _variants_struct(names, logits: torch.Tensor, stride: int) -> "_lib.Variants":
    """`iefvad_variants` over the [V, ...] result tensor: row v is variant names[v]."""
    v = _lib.Variants()
    v.count = len(names)
    for j, n in enumerate(names):
        v.kind[j] = _lib.VARIANT_NAMES.index(n)
    v.logits, v.stride = logits.data_ptr(), stride
    return v


def attn_map_layers(attn_maps, num_layers: int) -> tuple:
    """`attn_maps=` -> the encoder layers whose head-averaged attention maps are asked for, ascending: None / False -> none, True -> all
    `num_layers`, else an int or an iterable of layer indices in 0 .. num_layers - 1 (ValueError otherwise)."""
    if attn_maps is None or attn_maps is False:
        return ()
    if attn_maps is True:
        return tuple(range(num_layers))
    try:
        want = [attn_maps] if isinstance(attn_maps, int) else list(attn_maps)
    except TypeError:
        raise ValueError(f"attn_maps takes True or an iterable of layer indices (got {attn_maps!r})") from None
    bad = [l for l in want if isinstance(l, bool) or not isinstance(l, int) or not 0 <= l < num_layers]
    if bad or not want:
        raise ValueError(f"attn_maps takes True or layer indices in 0..{num_layers - 1} (got {attn_maps!r})")
    return tuple(sorted(set(want)))


def _attn_maps_struct(image: torch.Tensor, event: torch.Tensor, layers) -> "_lib.AttnMaps":
    """`iefvad_attn_maps` over the [n, ...] result tensors: slice j is layer layers[j]."""
    m = _lib.AttnMaps()
    for j, l in enumerate(layers):
        m.image[l] = image[j].data_ptr()
        m.event[l] = event[j].data_ptr()
    return m


def attn_maps_asked(attn_maps) -> bool:
    """Whether `attn_maps=` asks for maps at all -- the raw fact, before `attn_map_layers` parses (and may refuse) the value."""
    return attn_maps is not None and attn_maps is not False


def _given(pair) -> bool:      # a `row_scale` / `row_noise` pair that names at least one vector
    return pair is not None and any(v is not None for v in pair)


def _differentiable(a: torch.Tensor, b: torch.Tensor) -> bool:      # a call on these features has to be differentiable
    return torch.is_grad_enabled() and (a.requires_grad or b.requires_grad)


class _Request:
    """What one call of `forward`, `forward_videos` or `forward_videos_host` asked for: built once from the raw keywords, each fact computed
    once.  `maps_asked` is the raw view of `attn_maps=` and `layers` the parsed one: () until the checks parse it at its place in their order,
    so a value that does not parse is refused there and not sooner.  `_PLAIN` is the call that asks for nothing."""
    __slots__ = ("kind", "training", "grad", "eval_grad", "fp16x3", "bf16", "timed", "row_scale", "scaled", "attn_maps", "maps_asked", "layers", "row_noise",
                 "noisy", "noise_seed", "noise_rows", "trajectory", "variants", "samples", "similarity", "outputs", "outputs_asked", "weight_sums", "nan_always", "extras", "online")

    def __init__(self, training=False, grad=False, compute="f32", *, timed=False, row_scale=None, attn_maps=None, row_noise=None, noise_seed=None,
                 noise_rows=None, trajectory=False, fusion_variants=None, similarity=False, outputs=None, weight_sums=False, nan_to_num=True):
        self.variants = fusion_variant_names(fusion_variants)      # parses, and may refuse, before anything else is looked at
        self.training, self.grad, self.eval_grad = training, grad, grad and not training      # eval_grad: the differentiable eval route
        self.fp16x3, self.bf16, self.timed, self.trajectory = compute == "fp16x3", compute == "bf16", timed, trajectory
        self.attn_maps, self.maps_asked, self.layers = attn_maps, attn_maps_asked(attn_maps), ()
        self.row_scale, self.scaled = row_scale, _given(row_scale)
        self.row_noise, self.noisy, self.noise_seed, self.noise_rows = row_noise, _given(row_noise), noise_seed, noise_rows
        self.similarity, self.outputs, self.outputs_asked, self.weight_sums = similarity, outputs, outputs is not None, weight_sums
        self.nan_always = isinstance(nan_to_num, str) and nan_to_num == "always"
        self.extras = self.nan_always or weight_sums or self.scaled or self.noisy      # the sweep's extras of the valid-row calls
        self.samples = None      # `forward_samples` / `forward_videos_samples`: (S, seed, scale, sample_rows)
        self.online = None       # `forward_videos_online`: the call's `lib.Online`
        self.kind = "plain"      # the row of `_DENSE_ENTRIES` that serves the request: `forward` names it once the checks have passed


_PLAIN = _Request()


def _noise_rules(noisy: bool, noise_seed, noise_rows):
    """The seed and `noise_rows` rules of a noise request."""
    if noisy and noise_seed is None:
        raise ValueError("row_noise needs noise_seed: the noise is a pure function of (seed, modality, noise id, column)")
    if noise_rows is not None and not noisy:
        raise ValueError("noise_rows without row_noise: the noise ids name rows of a noise request")


# The checks of a request, in the order they fire -- the order decides which error a caller sees, and tests/request_refusals.json pins it.
# A step is a rule (owner, ((label, member), ...), exception, message): where the request's `owner` holds, the members that hold too are
# refused, their labels joined into the message's {}; or a function of (model, request) that raises, or fills a fact in.
_IN_TRAIN = (("model.train()", "training"),)
_PARSE_LAYERS = lambda m, q: setattr(q, "layers", attn_map_layers(q.attn_maps, m.temporal.num_layers))
_VARIANTS_SERVED = (      # where a fusion-variants request cannot be served: the fp16x3 arithmetic, training, differentiable features
    ("variants", (("", "fp16x3"),), RuntimeError, 'fusion_variants= is not available with compute="fp16x3" (its per-chunk running-max words '
     'have no home for the stacked states); use "f32", "bf16x6" or "bf16"'),
    ("variants", _IN_TRAIN, RuntimeError, "fusion_variants= is an evaluation request; it is not available under {} (call model.eval() first)"),
    ("variants", (("", "grad"),), RuntimeError, "fusion_variants= is an evaluation request: nothing it returns is differentiable, and a feature "
     "tensor requires grad (detach the features, or call under torch.no_grad())"))
_TRAJECTORY_IN_EVAL = ("trajectory", _IN_TRAIN, RuntimeError, "trajectory=True is an evaluation request; it is not available under {} (call model.eval() first)")
_MAPS_SERVED = (      # where a maps request cannot be served: the bf16 arithmetic (its q | k | v are bf16 planes) and training
    ("layers", (("", "bf16"),), RuntimeError, 'attn_maps= is not available with compute="bf16" (its q | k | v are bf16 planes in another layout); '
     'use "f32", "bf16x6" or "fp16x3"'),
    ("layers", _IN_TRAIN, RuntimeError, "attn_maps= is an evaluation request; it is not available under {} (call model.eval() first)"))
_FORWARD_CHECKS = (
    ("variants", (("timed=True", "timed"), ("trajectory=True", "trajectory"), ("attn_maps=", "maps_asked"), ("row_scale=", "scaled"), ("row_noise=", "noisy")),
     ValueError, "fusion_variants= does not combine with {}: iefvad_forward_variants is a plain evaluation forward"),
    *_VARIANTS_SERVED,
    ("trajectory", (("timed=True", "timed"), ("attn_maps=", "maps_asked"), ("row_scale=", "scaled"), ("row_noise=", "noisy"), ("features that require grad", "grad")),
     ValueError, "trajectory=True does not combine with {}: iefvad_forward_trajectory is a plain evaluation forward"),
    _TRAJECTORY_IN_EVAL,
    _PARSE_LAYERS,
    lambda m, q: _noise_rules(q.noisy, q.noise_seed, q.noise_rows),
    ("noisy", (("attn_maps=", "layers"), ("timed=True", "timed"), ("model.train()", "training"), ("features that require grad", "grad")),
     ValueError, "row_noise= does not combine with {}: iefvad_forward_perturbed is a plain evaluation forward"),
    ("layers", (("timed=True", "timed"), ("row_scale", "scaled")),
     ValueError, "attn_maps= does not combine with timed=True or row_scale: iefvad_forward_attn takes neither"),
    *_MAPS_SERVED,
    # eval() with a feature tensor that requires grad: the reference differentiates here too, dropout simply off
    ("eval_grad", (("attn_maps=", "layers"), ("timed=True", "timed"), ("row_scale=", "scaled")),
     ValueError, "{} with a feature tensor that requires grad in eval(): the differentiable eval route runs the train-mode forward without "
     "dropout, which takes none of attn_maps, timed and row_scale (detach the features, or call under torch.no_grad())"),
)
_SWEEP_MEMBERS = (("row_scale=", "scaled"), ("row_noise=", "noisy"), ("similarity=True", "similarity"), ("outputs=", "outputs_asked"),
                  ("weight_sums=True", "weight_sums"), ("nan_to_num='always'", "nan_always"))
_VIDEOS_CHECKS = (
    ("variants", (("trajectory=True", "trajectory"), ("attn_maps=", "maps_asked")) + _SWEEP_MEMBERS,
     ValueError, "fusion_variants= does not combine with {}: iefvad_forward_videos_variants takes none of them"),
    *_VARIANTS_SERVED,
    ("trajectory", (("attn_maps=", "maps_asked"),) + _SWEEP_MEMBERS,
     ValueError, "trajectory=True does not combine with {}: iefvad_forward_videos_trajectory takes none of them"),
    _TRAJECTORY_IN_EVAL,
    _PARSE_LAYERS,
    ("layers", _SWEEP_MEMBERS, ValueError, "attn_maps= does not combine with similarity=True, outputs=, row_scale, row_noise, weight_sums or "
     "nan_to_num='always': iefvad_forward_videos_attn takes none of them"),
    *_MAPS_SERVED,
    ("training", _IN_TRAIN, RuntimeError, "iefvad_amd.MMFMIL.forward_videos is an evaluation entry point; call model.eval() first"),
)


def _check_request(model, q: _Request, checks):
    """Walk one of the tables above; the first step that objects raises."""
    for step in checks:
        if callable(step):
            step(model, q)
        elif getattr(q, step[0]):
            asked = [label for label, member in step[1] if getattr(q, member)]
            if asked:
                raise step[2](step[3].format(" / ".join(asked)))


def _row_entry_suffix(q: _Request, full_entry: str):
    """The exclusion rules between `similarity=`, `outputs=` and the sweep's extras of the valid-row calls -> (the [rows, D] keys asked
    for, the suffix of the entry that serves the request).  `full_entry`: the full entry's name, for the message."""
    if q.similarity and q.extras:
        raise ValueError("similarity=True does not combine with the sweep's extras (row_scale, weight_sums, nan_to_num='always'): "
                         "iefvad_forward_videos_scaled takes no similarity buffer")
    wide = _row_output_keys(q.outputs)
    if wide and q.similarity:
        raise ValueError(f"outputs= does not combine with similarity=True: {full_entry} takes no similarity buffer "
                         "(reduce the returned rows with harness.similarity_rows)")
    if wide and q.extras:
        raise ValueError("outputs= does not combine with the sweep's extras (row_scale, weight_sums, nan_to_num='always'): "
                         "iefvad_forward_videos_scaled returns no [rows, D] tensor")
    return wide, "_perturbed" if q.noisy else "_variants" if q.variants else "_trajectory" if q.trajectory else "_attn" if q.layers else \
        "_scaled" if q.extras else "_full" if wide else "_similarity" if q.similarity else ""


def _vector_pair(name: str, pair, nrows: int, device, what: str) -> tuple:
    """`row_scale` / `row_noise` -> the pair of None or contiguous fp32 vectors of `nrows` elements on `device` (ValueError otherwise)."""
    pair = (None, None) if pair is None else tuple(pair)
    if len(pair) != 2:
        raise ValueError(f"{name} must be a pair (image vector, event vector), either may be None")
    for v in pair:
        if v is not None and (not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.device != device or v.numel() != nrows
                              or not v.is_contiguous()):
            raise ValueError(f"{name} vectors must be contiguous fp32 tensors of {nrows} elements ({what}) on {device}")
    return pair


def _perturb_struct(nrows: int, device, row_scale, row_noise, noise_seed, noise_rows, what: str):
    """The `iefvad_perturb` of a call over `nrows` rows on `device`, and whether it carries noise.  `row_scale` / `row_noise`: None or a pair
    of contiguous fp32 device vectors of `nrows` elements (either may be None); `noise_rows`: None or a contiguous int32 device vector of
    noise ids; `noise_seed`: the generator's seed, required with `row_noise` (ValueError).  `what` names the row count in the messages."""
    scale = _vector_pair("row_scale", row_scale, nrows, device, what)
    amp = _vector_pair("row_noise", row_noise, nrows, device, what)
    noisy = _given(amp)
    _noise_rules(noisy, noise_seed, noise_rows)
    if noise_rows is not None and (not isinstance(noise_rows, torch.Tensor) or noise_rows.dtype != torch.int32 or noise_rows.device != device
                                   or noise_rows.numel() != nrows or not noise_rows.is_contiguous()):
        raise ValueError(f"noise_rows must be a contiguous int32 tensor of {nrows} elements ({what}) on {device}")
    p = _lib.Perturb()
    for m in (0, 1):
        p.scale[m] = scale[m].data_ptr() if scale[m] is not None else None
        p.noise_amp[m] = amp[m].data_ptr() if amp[m] is not None else None
    p.noise_row = noise_rows.data_ptr() if noise_rows is not None else None
    p.seed = (int(noise_seed) & 0xFFFFFFFFFFFFFFFF) if noise_seed is not None else 0
    return p, noisy


def _samples_struct(S, seed, scale, sample_rows, res, stride) -> "_lib.Samples":
    return _lib.Samples(S, seed, scale, sample_rows.data_ptr() if sample_rows is not None else None, res["logits_samples"].data_ptr(), stride,
                        res["score_mean"].data_ptr(), res["score_std"].data_ptr())


# What an attn / trajectory / variants / samples request adds to a call on either route: (the results, in the order they are returned behind the
# others, as a function of (request, steps, shape of `logits`, shape of one per-row vector -- (B, T) dense, (total,) on valid rows --, T,
# new fp32 tensor of a shape); the entry's argument that points at them, as a function of (request, those results, rows in all)).
_EXTRA_RESULTS = {
    "attn": (lambda q, steps, logits, rows, T, new: {"image_attn": new(len(q.layers), *rows, T), "event_attn": new(len(q.layers), *rows, T),
                                                     "attn_layers": q.layers},
             lambda q, res, n: C.byref(_attn_maps_struct(res["image_attn"], res["event_attn"], q.layers))),
    "trajectory": (lambda q, steps, logits, rows, T, new: {"logits_steps": new(steps + 1, *logits), "delta_norm": new(steps, *rows)},
                   lambda q, res, n: C.byref(_lib.Trajectory(res["logits_steps"].data_ptr(), res["delta_norm"].data_ptr() if len(res["delta_norm"]) else None, n))),
    "variants": (lambda q, steps, logits, rows, T, new: {"logits_variants": new(len(q.variants), *rows), "fusion_variants": q.variants},
                 lambda q, res, n: C.byref(_variants_struct(q.variants, res["logits_variants"], n))),
    "samples": (lambda q, steps, logits, rows, T, new: {"logits_samples": new(q.samples[0], *rows), "score_mean": new(*rows), "score_std": new(*rows)},
                lambda q, res, n: C.byref(_samples_struct(*q.samples, res, n))),
}


def _timed_arg(m, q, n, device):
    st = _lib.StageTimes()
    return (C.byref(st),), lambda: setattr(m, "last_stage_times", st.as_dict())


def _scaled_arg(m, q, n, device):
    for sv in q.row_scale:
        if sv is not None and (sv.dtype != torch.float32 or sv.device != device or sv.numel() != n or not sv.is_contiguous()):
            raise ValueError(f"row_scale vectors must be contiguous fp32 tensors of {n} elements on {device}")
    return tuple(C.c_void_p(sv.data_ptr()) if sv is not None else None for sv in q.row_scale), None


# The dense entries ([B, T, D] in, `MMFMIL._dense_call`) by the kind of the request (`_Request.kind`), each with: the entry; the
# prefix of the RuntimeError of a failed call; its workspace query and the query's arguments behind (handle, B); the index at which its
# own argument(s) stand in the plain entry's argument list; the function of (model, request, B * T, device) that forms them and says what
# to do after the call -- None where the kind has a row in `_EXTRA_RESULTS`, which also names the results behind OUTPUT_KEYS in the full dict.
_DENSE_ENTRIES = {
    "plain": ("iefvad_forward", "iefvad_forward", "iefvad_workspace_bytes", lambda q: (), 9, None),
    "timed": ("iefvad_forward_timed", "iefvad_forward", "iefvad_workspace_bytes", lambda q: (), 9, _timed_arg),
    "scaled": ("iefvad_forward_scaled", "iefvad_forward", "iefvad_workspace_bytes", lambda q: (), 5, _scaled_arg),
    "perturbed": ("iefvad_forward_perturbed", "iefvad_forward_perturbed", "iefvad_workspace_bytes", lambda q: (), 5,
                  lambda m, q, n, device: ((C.byref(_perturb_struct(n, device, q.row_scale, q.row_noise, q.noise_seed, q.noise_rows, "B*T")[0]),), None)),
    "attn": ("iefvad_forward_attn", "iefvad_forward_attn", "iefvad_workspace_bytes", lambda q: (), 8, None),
    "trajectory": ("iefvad_forward_trajectory", "iefvad_forward_trajectory", "iefvad_trajectory_workspace_bytes", lambda q: (), 8, None),
    "variants": ("iefvad_forward_variants", "iefvad_forward_variants", "iefvad_variants_workspace_bytes", lambda q: (len(q.variants),), 8, None),
}
# The samples entries, one row in the form of each table above.  They stand beside the tables, which list exactly the kinds a request of
# `forward` / `forward_videos` can reach: `forward_samples` / `forward_videos_samples` name these rows and `_entry_row` finds them.
_SAMPLES_ENTRIES = {
    "samples": ("iefvad_forward_samples", "iefvad_forward_samples", "iefvad_samples_workspace_bytes", lambda q: (), 8, None),
    "_samples": ("_samples", lambda r: (), lambda r: (*r["vectors"], r["samples"], r["stream"])),
}


# The online entry, a sibling in the same way: `forward_videos_online` names the row.  Its `iefvad_online` stands behind nan_to_num in the
# call's front arguments and behind (handle, lengths, nvideos) in the query's.
_ONLINE_ENTRIES = {
    "_online": ("_online", lambda r: (r["online"],), lambda r: (*r["vectors"], r["stream"])),
}


def _entry_row(table: dict, key: str) -> tuple:
    return table[key] if key in table else _SAMPLES_ENTRIES[key] if key in _SAMPLES_ENTRIES else _ONLINE_ENTRIES[key]


def online_params(stride, history=_lib.ONLINE_MAX_HISTORY) -> tuple:
    """The (stride, history) of an online call, checked: ints with 1 <= stride <= history <= 256 (ValueError otherwise)."""
    for name, v in (("stride", stride), ("history", history)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an int (got {v!r})")
    if not 1 <= stride <= history <= _lib.ONLINE_MAX_HISTORY:
        raise ValueError(f"1 <= stride <= history <= {_lib.ONLINE_MAX_HISTORY} required (got stride={stride}, history={history})")
    return stride, history


# what `MMFMIL(outputs=)` makes every dense call return, in the order of the returned dict: (key, its shape behind [B, T]; None = D)
_DENSE_OUTPUTS = {"full": tuple((k, (1,) if k == "logits" else None) for k in OUTPUT_KEYS),
                  "weights": (("logits", (1,)), ("w_i", None), ("w_e", None), ("w_i_mean", ()), ("w_e_mean", ())),
                  "scores": (("logits", (1,)), ("w_i_mean", ()), ("w_e_mean", ()))}


def perturb_rows(img_rows: Optional[torch.Tensor], ev_rows: Optional[torch.Tensor], *, row_scale=None, row_noise=None, noise_seed=None,
                 noise_rows=None, nan_to_num: bool = False):
    """The perturbation of input rows on its own (`iefvad_perturb_rows`, include/iefvad.h): [rows, D] device tensors (fp32, fp16 or bf16,
    D = 768 or 512; either may be None) -> (image rows, event rows) of the same dtype after, in this order, `nan_to_num` (torch.nan_to_num
    on every row), the row scale and the row noise, exactly as the input loads of `MMFMIL.forward(row_scale=, row_noise=)` and
    `MMFMIL.forward_videos(...)` form them.  The noise study's semantics are this package's own (the reference implements none:
    "parity unpinned"); this entry is what the fused loads are tested against."""
    src = [t for t in (img_rows, ev_rows) if t is not None]
    if not src:
        raise ValueError("perturb_rows needs at least one of img_rows, ev_rows")
    x0 = src[0]
    if any(t.dim() != 2 or t.shape != x0.shape or t.dtype != x0.dtype or t.device != x0.device for t in src):
        raise ValueError("perturb_rows takes [rows, D] tensors of one shape, dtype and device")
    if x0.dtype not in _IN_DTYPES:
        raise ValueError(f"feature dtype {x0.dtype} is not supported (fp32, fp16 or bf16)")
    if not x0.is_cuda:
        raise RuntimeError("iefvad_amd.perturb_rows runs on a HIP device only; there is no CPU fallback (harness.gaussian_rows is the host model)")
    rows, D = x0.shape
    p, _ = _perturb_struct(rows, x0.device, row_scale, row_noise, noise_seed, noise_rows, "the rows")
    lib = _lib.load_library()
    ins = [t.contiguous() if t is not None else None for t in (img_rows, ev_rows)]
    outs = [torch.empty_like(t) if t is not None else None for t in ins]
    with torch.cuda.device(x0.device):
        stream = torch.cuda.current_stream(x0.device).cuda_stream
        ptr = [C.c_void_p(t.data_ptr()) if t is not None else None for t in ins + outs]
        rc = lib.iefvad_perturb_rows(ptr[0], ptr[1], _IN_DTYPES[x0.dtype], D, rows, 1 if nan_to_num else 0, C.byref(p), ptr[2], ptr[3],
                                     C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("iefvad_perturb_rows: " + _lib.last_error())
    return outs[0], outs[1]


class _LinearParams(nn.Module):
    """Parameter holder with nn.Linear's names, shapes and default init (kaiming-uniform a=sqrt(5))."""

    def __init__(self, in_features: int, out_features: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(in_features)
        nn.init.uniform_(self.bias, -bound, bound)


class _LayerNormParams(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))


class _AttentionParams(nn.Module):
    """Parameter holder with nn.MultiheadAttention's packed layout: in_proj_weight [3D, D] in (q, k, v)
    order, in_proj_bias [3D], out_proj.{weight,bias}; same init order as torch (out_proj first, then
    xavier-uniform in_proj, zero biases) so a seeded construction reproduces the reference's weights."""

    def __init__(self, dim: int, dropout: float = 0.0):
        super().__init__()
        self.dropout = dropout          # nn.MultiheadAttention.dropout: applied to the attention weights in train mode
        self.in_proj_weight = nn.Parameter(torch.empty(3 * dim, dim))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * dim))
        self.out_proj = _LinearParams(dim, dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.in_proj_bias, 0.0)
        nn.init.constant_(self.out_proj.bias, 0.0)


class _RefinementBlockParams(nn.Module):
    """Sequential(Linear, ReLU, Linear): parameters live at indices 0 and 2 (imf_vad.py:97-104)."""

    def __init__(self, dim: int):
        super().__init__()
        self.add_module("0", _LinearParams(dim, dim))
        self.add_module("2", _LinearParams(dim, dim))


class FusionParams(nn.Module):
    """Parameters and hyper-parameters of MultiModal_Fusion_Attn_Iter (imf_vad.py:48-107), registered
    in the reference's order."""

    def __init__(self, embed_dim, num_layers=2, num_heads=8, dropout=0.1, num_refinement_steps=3,
                 lambda_ref=0.5, noise_model="StudentT", nu=5, epsilon=1e-8):
        super().__init__()
        self.embed_dim = embed_dim
        self.num_layers = num_layers
        self.num_heads = num_heads
        self.num_refinement_steps = num_refinement_steps
        self.lambda_ref = lambda_ref
        self.noise_model = noise_model
        self.nu = nu
        self.epsilon = epsilon
        self.image_attn_layers = nn.ModuleList([_AttentionParams(embed_dim, dropout) for _ in range(num_layers)])
        self.image_norms = nn.ModuleList([_LayerNormParams(embed_dim) for _ in range(num_layers)])
        self.event_attn_layers = nn.ModuleList([_AttentionParams(embed_dim, dropout) for _ in range(num_layers)])
        self.event_norms = nn.ModuleList([_LayerNormParams(embed_dim) for _ in range(num_layers)])
        self.whiten_image = _LayerNormParams(embed_dim)
        self.whiten_event = _LayerNormParams(embed_dim)
        self.image_mu = _LinearParams(embed_dim, embed_dim)
        self.event_mu = _LinearParams(embed_dim, embed_dim)
        self.image_logvar = _LinearParams(embed_dim, embed_dim)
        self.event_logvar = _LinearParams(embed_dim, embed_dim)
        if num_refinement_steps == 0:
            self.refinement_blocks = nn.ModuleList([nn.Identity()])
        else:
            self.refinement_blocks = nn.ModuleList(
                [_RefinementBlockParams(embed_dim) for _ in range(num_refinement_steps)])
        self.classifier = _LinearParams(embed_dim, 1)


class _TrainForward(torch.autograd.Function):
    """The train-mode forward of the whole model as ONE autograd node: forward = `iefvad_train_forward` (keeps the activations in
    a buffer this node owns), backward = `iefvad_train_backward` (every parameter gradient).  The parameters are inputs of the
    node, so `loss.backward()` accumulates into their `.grad` exactly as with the reference's modules.  So are the two feature
    tensors: where one requires grad, the backward is `iefvad_train_backward_inputs` and the tensor receives its gradient in its own
    dtype and shape (the library's fp32 gradient with respect to the widened rows, cast as autograd casts through `.to(torch.float)`).
    `no_dropout` (the differentiable eval route): every dropout probability 0 and no mask, whatever the layers and the model carry."""

    @staticmethod
    def forward(ctx, model, no_dropout, img, ev, *params):
        lib = _lib.load_library()
        t = model.temporal
        device = img.device
        B, T, D = img.shape
        ctx.in_meta = ((img.dtype, img.shape), (ev.dtype, ev.shape))
        img = model._prepare_input(img)
        ev = model._prepare_input(ev)
        if ev.dtype != img.dtype:
            img, ev = img.to(torch.float), ev.to(torch.float)
        opt = _lib.TrainOptions()
        for m, name in enumerate(("image", "event")):
            for l, a in enumerate(getattr(t, f"{name}_attn_layers")):
                opt.dropout_p[m][l] = 0.0 if no_dropout else float(a.dropout)
        seed = 0 if no_dropout else model.__dict__.get("dropout_seed")      # no mask is drawn without dropout: torch's RNG stays where it is
        if seed is None:      # a fresh stream per step, reproducible under torch.manual_seed
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
        opt.seed = seed & 0xFFFFFFFFFFFFFFFF
        mask = None if no_dropout else model.__dict__.get("dropout_mask")
        if mask is not None:
            want = (2, t.num_layers, B, t.num_heads, T, T)
            if tuple(mask.shape) != want or mask.dtype != torch.uint8 or mask.device != device or not mask.is_contiguous():
                raise ValueError(f"dropout_mask must be a contiguous uint8 tensor of shape {want} on {device}")
            opt.keep_mask = mask.data_ptr()
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            model._ensure_handle(device)
            model._ensure_weights(device, stream)
            need = lib.iefvad_train_workspace_bytes(model._handle, B)
            if need == 0:
                raise RuntimeError(f"iefvad_train_workspace_bytes: unsupported batch size {B}")
            ws = torch.empty(need, dtype=torch.uint8, device=device)
            f32 = dict(dtype=torch.float32, device=device)
            res = {k: torch.empty(B, T, 1 if k == "logits" else D, **f32) for k in OUTPUT_KEYS}
            o = _lib.Outputs()
            for k in OUTPUT_KEYS:
                setattr(o, k, res[k].data_ptr())
            rc = lib.iefvad_train_forward(model._handle, C.c_void_p(img.data_ptr()), C.c_void_p(ev.data_ptr()), _IN_DTYPES[img.dtype], B,
                                          C.byref(opt), C.c_void_p(ws.data_ptr()), ws.numel(), C.byref(o), C.c_void_p(stream))
        if rc != 0:
            raise RuntimeError("iefvad_train_forward: " + _lib.last_error())
        ctx.model, ctx.ws, ctx.B, ctx.mask = model, ws, B, mask
        ctx.params = params
        ctx.set_materialize_grads(False)     # backward takes None as "no gradient": no zero-filled [B,T,768] tensors for unused outputs
        outs = tuple(res[k] for k in OUTPUT_KEYS)
        # the library wrote five of the outputs in place and reads them, and fp32 inputs, again in the backward (include/iefvad.h):
        # saved here so that they stay alive and an in-place edit between the two passes raises as it would in the reference
        ctx.save_for_backward(img, ev, *(res[k] for k in ("fused", "image_mu", "event_mu", "image_logvar", "event_logvar")))
        return outs

    @staticmethod
    def backward(ctx, *gouts):
        lib = _lib.load_library()
        model, ws = ctx.model, ctx.ws
        if ws is None:
            raise RuntimeError("iefvad_amd.MMFMIL: backward through the same forward twice (the activations were released)")
        _ = ctx.saved_tensors               # version check of the tensors the library reads again
        device = ws.device
        keep = []
        dout = _lib.OutputGrads()
        for k, g in zip(OUTPUT_KEYS, gouts):
            if g is not None:
                g = g.contiguous().float()
                keep.append(g)
                setattr(dout, k, g.data_ptr())
        needs = ctx.needs_input_grad[4:]
        grads = [torch.empty_like(p, memory_format=torch.contiguous_format) if n else None for p, n in zip(ctx.params, needs)]
        by_id = {id(p): g for p, g in zip(ctx.params, grads)}
        dw = _lib.WeightGrads()
        model._fill_weight_struct(dw, lambda p: by_id[id(p)].data_ptr() if by_id.get(id(p)) is not None else None)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            args = (model._handle, ctx.B, C.c_void_p(ws.data_ptr()), ws.numel(), C.byref(dout), C.byref(dw))
            # the gradients of the feature tensors: fp32 [B, T, D] for the ones asked for, and the entry that takes them
            gin = [torch.empty(ctx.B, *shape[1:], dtype=torch.float32, device=device) if n else None
                   for (_, shape), n in zip(ctx.in_meta, ctx.needs_input_grad[2:4])]
            if gin[0] is not None or gin[1] is not None:
                name = "iefvad_train_backward_inputs"
                dx = _lib.InputGrads(*(g.data_ptr() if g is not None else None for g in gin))
                rc = lib.iefvad_train_backward_inputs(*args, C.byref(dx), C.c_void_p(stream))
            else:
                name = "iefvad_train_backward"
                rc = lib.iefvad_train_backward(*args, C.c_void_p(stream))
        ctx.ws = None                       # the library retired the forward's record, on failure too: its scratch overwrites saved states
        if rc != 0:
            raise RuntimeError(name + ": " + _lib.last_error())
        gin = [g if g is None or g.dtype == dtype else g.to(dtype) for g, (dtype, _) in zip(gin, ctx.in_meta)]
        return (None, None, *gin, *grads)


class MMFMIL(nn.Module):
    """Same constructor as the reference's MMFMIL (/root/reference/model/imf_vad.py:6-18).

    Extra, keyword-only knobs (not in the reference):
      outputs      "full" (default; all eight tensors, the drop-in behaviour), "scores"
                   (only `logits` plus the per-row means `w_i_mean`, `w_e_mean`; nothing 768-wide
                   is written to HBM) or "weights" (the scores set plus the full `w_i`, `w_e`: what the
                   robustness sweep reads, test2.py:65-68).
      micro_batch  chunks per internal pass of the library (0 = library default).
      graph_chunks calls with B <= graph_chunks replay a cached hipGraph of the forward instead of launching its ~31
                   kernels one by one (0 = library default, 8; negative = never).  Same bits either way.
      compute      "f32" (default): exact-fp32 MFMA projections, the parity mode;
                   "bf16": bf16 MFMA operands with fp32 accumulation in the dense projections and in the two
                   attention products; softmax, LayerNorm, the residual stream, the fusion and the refinement
                   state stay fp32 (BASELINE config 3);
                   "bf16x6": the fp32 path with every dense projection computed as six bf16 MFMA products of the exact
                 three-term bf16 split of both fp32 operands (csrc/gemm_split.h): fp32-accurate -- held to the same
                 tolerances as "f32" -- at the bf16 matrix-core rate.  Batches too small to fill the chip run on the
                 "f32" kernels, so scores are fp32-accurate but not bit-identical across batch sizes in this mode
                 (unless `batch_invariant=True`, below).
                   "fp16x3" (opt-in, near-fp32): the "bf16x6" flow with two fp16 terms per operand and three products per
                 multiply-add (22-bit products, half the MFMAs); operands are scaled by powers of two from running max |.|
                 words the producing kernels maintain (range-safe).  Per-projection error vs fp64 ~1.8x the fp32 path's.
      batch_invariant  (default False) with compute="bf16x6": every projection and attention of the evaluation forward runs in the
                   split arithmetic at EVERY batch size (`iefvad_set_batch_invariant`; small launches on the small tiling of
                   csrc/gemm_split_small.h), so a video's results are the same bits at B = 1 and B = 8192, padded or on the valid-row
                   routes, per video, packed or from host lists -- the guarantee "f32" gives.  Still held to the "f32" tolerances; a small
                   call costs more than in the default mode.  Accepted and inert with "f32" and "bf16" (already invariant); ValueError
                   with "fp16x3".  Carried by `lanes(n)`; training is not affected.

    The K-step refinement at call time (not in the reference, whose K is fixed at construction):
      set_steps(k)  every evaluation call runs only the first k of the K refinement blocks, then the classifier (`iefvad_set_steps`) --
                   bit for bit what a model built with num_refinement_steps = k and given the first k blocks returns.  `None` restores K.
      trajectory=True  (`forward`, `forward_videos`) adds `logits_steps` (the logits after 0 .. steps steps) and `delta_norm`
                   (||z_{k+1} - z_k|| per step) from the one forward; every other result keeps its bits.

    The fusion ablations of a trained model (not in the reference, which forms `fused` inline, imf_vad.py:130-150):
      fusion_variants=True or names  (`forward`, `forward_videos`) adds `logits_variants`: the logits the model gives with the event
                   branch ("image") or the image branch ("event") removed at the fusion, with both precisions forced equal ("equal"),
                   and unchanged ("fused" = `logits`) -- encoder and heads run once, the refinement and classifier once more on the
                   stacked variants.  Every other result keeps its bits.

    The uncertainty of the score itself (not in the reference, which never samples the heads' Gaussians):
      forward_samples(img, ev, samples, seed) / forward_videos_samples(img_rows, ev_rows, lengths, samples, seed)  methods of their
                   own: the plain call's results with unchanged bits plus `logits_samples` (S Monte Carlo draws of every snippet's
                   logit, the means sampled from N(mu_m, scale^2 / w_m) and fused under the call's own precisions), `score_mean` and
                   `score_std` -- encoder and heads run once, the refinement and classifier once per group of four samples.

    Without any keyword (the reference's behaviour, imf_vad.py:40-44,109-161 being an ordinary nn.Module):
      gradients of the features  a feature tensor with `requires_grad=True` receives its `.grad` from `loss.backward()`, in its own dtype
                   and shape, in train() and in eval() alike -- an adapter or a learned projection upstream of the model trains, and
                   feature-space saliency works.  In train() the step is the usual one plus the layer-0 product d x = d s + d qkv W_in
                   per modality asked for (`iefvad_train_backward_inputs`; no parameter gradient changes by a bit).  In eval() with
                   grad enabled, a feature tensor that requires grad routes the call through the train-mode forward with every
                   dropout probability forced to 0 and no mask (the reference's eval(): dropout simply off); `attn_maps=`, `timed=True`
                   and `row_scale=` raise ValueError there.  Every other eval() call -- parameters that require grad included --
                   keeps the evaluation entry, its graph replay and its bits: the trigger is the inputs, never the parameters.  With
                   every parameter frozen the backward computes the input gradients alone (no weight-gradient product runs).
                   compute "f32" / "bf16x6" and D = 768 only, as training; `forward_videos` / `forward_videos_host` stay
                   evaluation-only and non-differentiable.
    """

    def __init__(self, num_class: int, embed_dim: int, visual_length: int, visual_width: int, visual_head: int,
                 visual_layers: int, attn_window: int, prompt_prefix: int, prompt_postfix: int, device, args,
                 *, outputs: str = "full", micro_batch: int = 0, compute: str = "f32", graph_chunks: int = 0,
                 batch_invariant: bool = False):
        super().__init__()
        self.num_class = num_class
        self.visual_length = visual_length
        self.visual_width = visual_width
        self.embed_dim = embed_dim
        self.attn_window = attn_window
        self.prompt_prefix = prompt_prefix
        self.prompt_postfix = prompt_postfix
        self.device = device
        self.temporal = FusionParams(embed_dim, num_layers=args.visual_layers, num_heads=args.visual_head,
                                     num_refinement_steps=args.num_refinement_steps, lambda_ref=args.lambda_ref,
                                     noise_model=args.noise_model, nu=args.nu)
        if outputs not in ("full", "scores", "weights"):
            raise ValueError("outputs must be 'full', 'scores' or 'weights'")
        if compute not in _lib.COMPUTE_CODES:
            raise ValueError("compute must be 'f32', 'bf16', 'bf16x6' or 'fp16x3'")
        self.outputs = outputs
        self.micro_batch = micro_batch
        if batch_invariant and compute == "fp16x3":
            raise ValueError('batch_invariant=True is not available with compute="fp16x3" (its operand scales are per chunk and per '
                             'running maximum); use "bf16x6" ("f32" and "bf16" are batch-invariant as they are)')
        self.compute = compute
        self.graph_chunks = graph_chunks
        self.batch_invariant = bool(batch_invariant)
        self._steps: Optional[int] = None      # set_steps: None = all K refinement steps
        self._handle: Optional[C.c_void_p] = None
        self._handle_key = None
        self._weights_sig = None
        self._workspace: Optional[torch.Tensor] = None
        self.last_stage_times: Optional[dict] = None

    # ------------------------------------------------------------------ library plumbing
    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _release(self):
        if self._handle is not None:
            _lib.load_library().iefvad_destroy(self._handle)
            self._handle = None
            self._handle_key = None
            self._weights_sig = None

    def _noise_code(self) -> int:
        nm = self.temporal.noise_model
        if nm == "Gaussian":
            return _lib.NOISE_GAUSSIAN
        if nm == "StudentT":
            return _lib.NOISE_STUDENT_T
        raise ValueError("Unsupported noise_model. Choose 'Gaussian' or 'StudentT'.")   # imf_vad.py:137-138

    def _ensure_handle(self, device: torch.device):
        t = self.temporal
        key = (device.index, t.embed_dim, self.visual_length, t.num_heads, t.num_layers, t.num_refinement_steps,
               self._noise_code(), float(t.lambda_ref), float(t.nu), float(t.epsilon), int(self.micro_batch), self.compute,
               int(self.graph_chunks), bool(self.batch_invariant))
        if self._handle is not None and key == self._handle_key:
            return
        self._release()
        lib = _lib.load_library()
        cfg = _lib.Config(abi_version=_lib.ABI_VERSION, embed_dim=t.embed_dim, seq_len=self.visual_length,
                          num_heads=t.num_heads, num_layers=t.num_layers, num_steps=t.num_refinement_steps,
                          noise_model=self._noise_code(),
                          compute=_lib.COMPUTE_CODES[self.compute], lambda_ref=float(t.lambda_ref),
                          nu=float(t.nu), epsilon=float(t.epsilon), micro_batch=int(self.micro_batch),
                          graph_chunks=int(self.graph_chunks))
        h = C.c_void_p()
        # D = 768 keeps the original entry; other widths (D = 512, the f32 forward of ViT-B/16 features) need iefvad_create_ex
        create = lib.iefvad_create if t.embed_dim == 768 else lib.iefvad_create_ex
        with torch.cuda.device(device):
            rc = create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise RuntimeError("iefvad_create: " + _lib.last_error())
        self._handle, self._handle_key = h, key
        if self.batch_invariant:
            with torch.cuda.device(device):
                rc = lib.iefvad_set_batch_invariant(h, 1)
            if rc != 0:
                raise RuntimeError("iefvad_set_batch_invariant: " + _lib.last_error())
        if self._steps is not None and lib.iefvad_set_steps(h, int(self._steps)) != 0:
            raise RuntimeError("iefvad_set_steps: " + _lib.last_error())

    @property
    def steps(self) -> int:
        """Refinement steps an evaluation call runs: K, or what `set_steps` chose."""
        return self.temporal.num_refinement_steps if self._steps is None else self._steps

    def set_steps(self, k: Optional[int]):
        """Run only the first `k` of the K refinement blocks in every evaluation call (`iefvad_set_steps`): 0 <= k <= K, `None` restores K.
        The results are bit for bit those of a model built with num_refinement_steps = k that was given the first k blocks.  Carried to
        the lanes of `lanes(n)`.  model.train() forwards refuse a model whose count is not K (RuntimeError from the library)."""
        K = self.temporal.num_refinement_steps
        if k is not None:
            if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= K:
                raise ValueError(f"set_steps takes None or an integer in 0..{K} (the model's num_refinement_steps), got {k!r}")
        for m in [self] + list(self.__dict__.get("_lane_copies", [])):
            m._steps = k
            if m._handle is not None and _lib.load_library().iefvad_set_steps(m._handle, K if k is None else int(k)) != 0:
                raise RuntimeError("iefvad_set_steps: " + _lib.last_error())

    def _params(self) -> list:
        # (owner's _parameters dict, name) of every parameter, resolved once: walking the module tree on every call costs
        # more host time than the rest of a one-chunk forward's enqueue; looking the slots up each time still sees a
        # Parameter that was re-assigned
        slots = self.__dict__.get("_param_slots")
        if slots is None:
            slots = [(m._parameters, n) for m in self.temporal.modules() for n in m._parameters if m._parameters[n] is not None]
            self.__dict__["_param_slots"] = slots
        return [d[n] for d, n in slots]

    def _ensure_weights(self, device: torch.device, stream: int):
        params = self._params()
        sig = tuple((p.data_ptr(), p._version) for p in params)
        if sig == self._weights_sig:
            return
        for p in params:
            if p.device != device or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("MMFMIL parameters must be contiguous fp32 tensors on the input's device "
                                   f"({device}); call model.to(device)")
        w = _lib.Weights()
        self._fill_weight_struct(w, lambda p: p.data_ptr())
        rc = _lib.load_library().iefvad_set_weights(self._handle, C.byref(w), C.c_void_p(stream))
        if rc != 0:
            raise RuntimeError("iefvad_set_weights: " + _lib.last_error())
        self._weights_sig = sig

    def _fill_weight_struct(self, w, ptr):
        """Fill an `iefvad_weights`-shaped ctypes structure (Weights or WeightGrads) with `ptr(parameter)` per field."""
        t = self.temporal
        for m, name in enumerate(("image", "event")):
            attn = getattr(t, f"{name}_attn_layers")
            norms = getattr(t, f"{name}_norms")
            for l in range(t.num_layers):
                w.in_proj_w[m][l] = ptr(attn[l].in_proj_weight)
                w.in_proj_b[m][l] = ptr(attn[l].in_proj_bias)
                w.out_proj_w[m][l] = ptr(attn[l].out_proj.weight)
                w.out_proj_b[m][l] = ptr(attn[l].out_proj.bias)
                w.norm_w[m][l] = ptr(norms[l].weight)
                w.norm_b[m][l] = ptr(norms[l].bias)
            wh = getattr(t, f"whiten_{name}")
            w.whiten_w[m], w.whiten_b[m] = ptr(wh.weight), ptr(wh.bias)
            mu, lv = getattr(t, f"{name}_mu"), getattr(t, f"{name}_logvar")
            w.mu_w[m], w.mu_b[m] = ptr(mu.weight), ptr(mu.bias)
            w.logvar_w[m], w.logvar_b[m] = ptr(lv.weight), ptr(lv.bias)
        for k in range(t.num_refinement_steps):
            blk = t.refinement_blocks[k]
            l1, l2 = getattr(blk, "0"), getattr(blk, "2")
            w.ref_w1[k], w.ref_b1[k] = ptr(l1.weight), ptr(l1.bias)
            w.ref_w2[k], w.ref_b2[k] = ptr(l2.weight), ptr(l2.bias)
        w.cls_w, w.cls_b = ptr(t.classifier.weight), ptr(t.classifier.bias)

    def lanes(self, n: int):
        """`n` forward lanes over ONE set of parameters: lane 0 is this module, the others are shallow copies that share
        `self.temporal` (the same Parameter objects) and own a library handle, repacked weights and workspace each, so that
        forwards issued on different HIP streams can run at the same time (harness.score_loader(lanes=...): the one-chunk
        forwards of the reference's per-video loop leave most of the chip idle).  Cached on the module."""
        import copy
        have = self.__dict__.setdefault("_lane_copies", [])
        while len(have) < n - 1:
            c = copy.copy(self)
            c.__dict__["_lane_copies"] = []
            c.__dict__["_stagers"] = {}          # a lane stages through buffers of its own (harness.score_loader), never lane 0's
            c.__dict__.pop("_param_slots", None)
            c._handle = c._handle_key = c._weights_sig = c._workspace = None
            have.append(c)
        return [self] + have[:max(n - 1, 0)]

    def refresh_weights(self):
        """Force the library to re-read (and re-pack / re-split) the parameters on the next forward.  The shim notices
        `load_state_dict`, `.to()`, optimizer steps and any in-place op on a Parameter (they change the storage pointer
        or the tensor version), but NOT writes made through `param.data` (e.g. `p.data.mul_(0.999)` in an EMA or a
        clipping utility): those bypass the version counter, so call this after them."""
        self._weights_sig = None
        for c in self.__dict__.get("_lane_copies", []):
            c._weights_sig = None

    def load_state_dict(self, *args, **kw):
        self.refresh_weights()
        return super().load_state_dict(*args, **kw)

    def _apply(self, fn, *args, **kw):
        self.refresh_weights()
        return super()._apply(fn, *args, **kw)

    # ------------------------------------------------------------------ forward
    def _prepare_input(self, x: torch.Tensor) -> torch.Tensor:
        if x.dtype not in _IN_DTYPES:
            x = x.to(torch.float)        # imf_vad.py:41-42 for fp64 / integer inputs
        return x.contiguous()

    def _prepare_pair(self, img: torch.Tensor, ev: torch.Tensor) -> tuple:
        """Both feature tensors as the library takes them: contiguous, of one supported dtype."""
        img, ev = self._prepare_input(img), self._prepare_input(ev)
        return (img, ev) if ev.dtype == img.dtype else (img.to(torch.float), ev.to(torch.float))

    def forward(self, img_visual, ev_visual, padding_mask=None, text=None, lengths=None, return_attn=False,
                *, timed: bool = False, row_scale=None, attn_maps=None, row_noise=None, noise_seed=None, noise_rows=None,
                trajectory: bool = False, fusion_variants=None) -> Dict[str, torch.Tensor]:
        """The reference's call (imf_vad.py:40-44; `padding_mask`, `text`, `lengths`, `return_attn` accepted and ignored as there).
        Keyword-only extras: `timed` (per-stage device times in `last_stage_times`), `row_scale=(s_img, s_ev)`: fp32 DEVICE vectors
        of [B*T] (either may be None) that multiply the input rows inside the library's input load (`iefvad_forward_scaled`: the
        robustness sweep's `x[:, idx] * 0.01`, test2.py:71-77, without touching the caller's tensors).
        `attn_maps=True` (every encoder layer) or an iterable of layer indices (`iefvad_forward_attn`) adds `image_attn` and `event_attn`,
        [n, B, T, T] fp32 in ascending layer order -- the head-averaged attention weights the reference's nn.MultiheadAttention calls
        form and discard (imf_vad.py:115,121) -- and `attn_layers`, the n layer indices.  Every other result keeps its bits.  Not with
        `timed` or `row_scale` (ValueError), compute="bf16" or model.train() (RuntimeError).
        `row_noise=(a_img, a_ev)` with `noise_seed=` (`iefvad_forward_perturbed`): fp32 DEVICE vectors of [B*T] (either may be None); behind
        the scale, row r of modality m gets a_m[r] * eps added in the input load, eps the library's counter-based standard normal of
        (noise_seed, m, noise id, column) (include/iefvad.h; host model `harness.gaussian_rows`); the noise id is `noise_rows[r]` (int32
        DEVICE vector) or the row index b*T + t.  Give pad rows amplitude 0.  The reference implements no such noise: these semantics are
        this package's own ("parity unpinned").  `row_noise` without `noise_seed`, with `timed`, `attn_maps`, model.train() or features
        that require grad raises ValueError.
        In eval() with grad enabled, a feature tensor that requires grad makes the call differentiable (the train-mode forward with every
        dropout probability forced to 0, the class docstring's keyword-free section); the three extras raise ValueError there.
        `trajectory=True` (`iefvad_forward_trajectory`) adds `logits_steps`, [steps + 1, B, T, 1]: c . z_k + b_c for the states z_0 ..
        z_steps of the refinement (logits; apply the sigmoid), and `delta_norm`, [steps, B, T]: ||z_{k+1} - z_k||_2 = lambda ||r_k||, with
        steps = `self.steps`.  Row k of `logits_steps` is what `set_steps(k)` returns as `logits`; every other result keeps its bits.
        compute="bf16" runs such a call with two GEMM launches per step in place of its one chain kernel (same bits, slower).  It combines
        with none of `timed`, `attn_maps`, `row_scale`, `row_noise` and features that require grad (ValueError), and not with model.train()
        (RuntimeError).
        `fusion_variants=True` (all four, in the order "fused", "image", "event", "equal") or an iterable of those names
        (`iefvad_forward_variants`) adds `logits_variants`, [V, B, T] fp32 in the order named, and `fusion_variants`, the names: the logits
        (apply the sigmoid) of the model with one substitution in the fusion w_m = f exp(-lv_m), z0 = (w_i mu_i + w_e mu_e) / (w_i + w_e + eps)
        -- "image": w_e := 0, "event": w_i := 0, "equal": lv_i := lv_e := 0, "fused": none (equal to `logits`; bit for bit with "f32" and
        "bf16") -- followed by the `self.steps` refinement steps and the classifier.  Every other result keeps its bits.  An unknown or
        repeated name, and a combination with `timed`, `trajectory`, `attn_maps`, `row_scale` or `row_noise`, is a ValueError;
        compute="fp16x3", model.train() and a feature tensor that requires grad are RuntimeErrors."""
        self._noise_code()   # ValueError for an unsupported noise_model, as the reference raises
        grad = _differentiable(img_visual, ev_visual)
        if not (grad or self.training or timed or trajectory or row_scale is not None or attn_maps is not None or row_noise is not None
                or noise_rows is not None or fusion_variants is not None):
            q = _PLAIN      # nothing asked for: nothing to check
        else:
            q = _Request(self.training, grad, self.compute, timed=timed, row_scale=row_scale, attn_maps=attn_maps, row_noise=row_noise, noise_seed=noise_seed,
                         noise_rows=noise_rows, trajectory=trajectory, fusion_variants=fusion_variants)
            _check_request(self, q, _FORWARD_CHECKS)
            if q.training or q.grad:
                return self._forward_train(img_visual, ev_visual, no_dropout=not q.training)
            q.kind = "trajectory" if q.trajectory else "variants" if q.variants else "attn" if q.layers else "perturbed" if q.noisy else \
                "scaled" if q.scaled else "timed" if q.timed else "plain"      # the checks have refused what no entry serves
        return self._dense_call(q, img_visual, ev_visual, *self._check_dense_inputs(img_visual, ev_visual))

    def _check_dense_inputs(self, img_visual, ev_visual) -> tuple:
        """The device, shape and [B, T, D] against the model checks of a dense call -> (B, T, D)."""
        if not (img_visual.is_cuda and ev_visual.is_cuda):
            raise RuntimeError("iefvad_amd.MMFMIL runs on a HIP device only; there is no CPU fallback (move the inputs with .to('cuda'))")
        if img_visual.shape != ev_visual.shape or img_visual.dim() != 3:
            raise ValueError(f"expected two [B, T, D] tensors of equal shape, got {tuple(img_visual.shape)} and {tuple(ev_visual.shape)}")
        B, T, D = img_visual.shape
        if T != self.visual_length or D != self.temporal.embed_dim:
            raise ValueError(f"expected [B, {self.visual_length}, {self.temporal.embed_dim}] inputs, got [B, {T}, {D}]")
        return B, T, D

    def _ensure_workspace(self, device, need: int) -> torch.Tensor:
        """The workspace the caller of the library owns, grown to `need` bytes on `device`."""
        if self._workspace is None or self._workspace.device != device or self._workspace.numel() < need:
            self._workspace = None
            self._workspace = torch.empty(need, dtype=torch.uint8, device=device)
        return self._workspace

    def _dense_call(self, q: _Request, img_visual, ev_visual, B, T, D) -> Dict[str, torch.Tensor]:
        """One dense call, the row of `_DENSE_ENTRIES` that serves `q`: sizes the workspace by the row's query, allocates the results
        `self.outputs` names and the row's own, and calls the entry with its own argument(s) at their place."""
        kind = q.kind
        entry, prefix, query, query_args, at, own = _entry_row(_DENSE_ENTRIES, kind)
        device = img_visual.device
        img, ev = self._prepare_pair(img_visual, ev_visual)
        lib = _lib.load_library()
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            self._ensure_handle(device)
            self._ensure_weights(device, stream)
            ws = self._ensure_workspace(device, getattr(lib, query)(self._handle, B, *query_args(q)))
            f32 = dict(dtype=torch.float32, device=device)
            res: Dict[str, torch.Tensor] = {}
            o = _lib.Outputs()
            for k, tail in _DENSE_OUTPUTS[self.outputs]:      # "weights": the sweep's set (test2.py:65-68,86-87), both weight tensors and their row means
                res[k] = torch.empty(B, T, *((D,) if tail is None else tail), **f32)
                setattr(o, k, res[k].data_ptr())
            call = [self._handle, C.c_void_p(img.data_ptr()), C.c_void_p(ev.data_ptr()), _IN_DTYPES[img.dtype], B,
                    C.c_void_p(ws.data_ptr()), ws.numel(), C.byref(o), C.c_void_p(stream)]
            extra, after = {}, None
            if kind in _EXTRA_RESULTS:
                extra = _EXTRA_RESULTS[kind][0](q, self.steps, (B, T, 1), (B, T), T, lambda *shape: torch.empty(shape, **f32))
                res.update(extra)
                call.insert(at, _EXTRA_RESULTS[kind][1](q, extra, B * T))
            elif own is not None:
                call[at:at], after = own(self, q, B * T, device)
            rc = getattr(lib, entry)(*call)
            if after is not None:
                after()
            if rc != 0:
                raise RuntimeError(prefix + ": " + _lib.last_error())
        if self.outputs == "full":
            return {k: res[k] for k in (*OUTPUT_KEYS, *extra)}   # the reference's key order
        return res

    def forward_videos_host(self, imgs, evs, lengths, nan_to_num: bool = True, batch_chunks: int = 128, host_threads: int = 0,
                            wire_dtype: Optional[torch.dtype] = None, similarity: bool = False, *, outputs=None) -> Dict[str, torch.Tensor]:
        """A whole list of videos in ONE library call (`iefvad_forward_videos_host`): `imgs[v]`, `evs[v]` are contiguous HOST tensors
        of one dtype whose first `lengths[v]` rows ([..., D]) are video v's features -- e.g. the padded tensors a DataLoader
        delivers (data/dataset.py:34-52).  The library packs whole videos into passes of >= `batch_chunks` chunks, stages and sends
        pass k + 1 while pass k computes, and returns DEVICE vectors `logits`, `w_i_mean`, `w_e_mean` of [sum(lengths)] in list
        order (stream-ordered on the current stream).  Same results as `forward_videos` on the same batches.
        `wire_dtype=torch.bfloat16` (fp32 features, compute="bf16" only): the gather threads round the rows to bf16 while staging, so
        half the bytes cross PCIe; same results as `forward_videos` on `rows.to(torch.bfloat16)` (include/iefvad.h).
        `similarity=True` (`iefvad_forward_videos_host_similarity`) adds "similarity" as `forward_videos` does.
        `outputs="full"` or an iterable of OUTPUT_KEYS names (`iefvad_forward_videos_host_full`) adds those keys as [sum(lengths), D]
        fp32 device tensors in list order, as `forward_videos` does; it does not combine with `similarity=True` (ValueError).
        An evaluation entry: nothing it returns is differentiable (features that require grad get no gradient here; use `forward`)."""
        if self.training:
            raise RuntimeError("iefvad_amd.MMFMIL.forward_videos_host is an evaluation entry point; call model.eval() first")
        self._noise_code()
        q = _Request(similarity=similarity, outputs=outputs)
        wide, suffix = _row_entry_suffix(q, "iefvad_forward_videos_host_full")
        lens = [int(n) for n in lengths]
        if not lens or min(lens) < 1 or len(imgs) != len(lens) or len(evs) != len(lens):
            raise ValueError("imgs, evs and lengths must list the same videos, every video at least one snippet")
        dt = imgs[0].dtype
        D = self.temporal.embed_dim
        if dt not in _IN_DTYPES:
            raise ValueError(f"feature dtype {dt} is not supported by the list entry (fp32, fp16 or bf16)")
        wire = dt if wire_dtype is None else wire_dtype
        if wire not in _IN_DTYPES:
            raise ValueError(f"wire dtype {wire} is not supported (the feature dtype, or torch.bfloat16 for fp32 features)")
        n = len(lens)
        # validation as C-speed sweeps (a per-video Python loop costs more than the library call on lists of short videos)
        for parts in (imgs, evs):
            if any(t.dtype != dt for t in parts) or any(t.is_cuda for t in parts) or not all(t.is_contiguous() for t in parts) \
                    or any(t.shape[-1] != D for t in parts) or any(t.numel() < ln * D for t, ln in zip(parts, lens)):
                raise ValueError(f"expected contiguous host tensors of dtype {dt} with at least lengths[v] rows of {D} each")
        pi = (C.c_void_p * n)(*[t.data_ptr() for t in imgs])
        pe = (C.c_void_p * n)(*[t.data_ptr() for t in evs])
        device = next(self.temporal.parameters()).device
        if device.type != "cuda":
            raise RuntimeError("iefvad_amd.MMFMIL runs on a HIP device only; there is no CPU fallback (call model.to('cuda'))")
        front = (pi, pe, _IN_DTYPES[dt], _IN_DTYPES[wire], (C.c_int32 * n)(*lens), n, 1 if nan_to_num else 0, int(batch_chunks), int(host_threads))
        return self._rows_call("iefvad_forward_videos_host", suffix, q, device, sum(lens), front, wide=wide)

    def _rows_call(self, base, suffix, q: _Request, device, total, front, *, wide=(), workspace_for=None):
        """One valid-row call, the entry `base + suffix` (`_ROW_ENTRIES`): allocates the results -- the three [total] vectors, a
        [total, D] tensor per key of `wide`, the similarity entries' [4, total] series, `w_colsum`, the suffix's `_EXTRA_RESULTS` -- and calls the
        entry with (handle, *front, [workspace, bytes,] the suffix's tail).  `workspace_for=(lengths array, nvideos)`: the device entries, whose
        workspace the caller owns; it is sized by the suffix's query."""
        lib, name = _lib.load_library(), base + suffix
        query, query_tail, tail = _entry_row(_ROW_ENTRIES, suffix)
        D = self.temporal.embed_dim
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            self._ensure_handle(device)
            self._ensure_weights(device, stream)
            f32 = dict(dtype=torch.float32, device=device)
            res = {k: torch.empty(total, **f32) for k in ("logits", "w_i_mean", "w_e_mean")}
            r = {"vectors": tuple(C.c_void_p(res[k].data_ptr()) for k in ("logits", "w_i_mean", "w_e_mean")), "stream": C.c_void_p(stream), "out": None,
                 "similarity": None, "w_colsum": None, "with_colsum": 1 if q.weight_sums else 0, "attn": None, "trajectory": None,
                 "variants": None, "nvariants": len(q.variants), "samples": None,
                 "online": C.byref(q.online) if q.online is not None else None}
            if suffix[1:] in _EXTRA_RESULTS:
                extra = _EXTRA_RESULTS[suffix[1:]][0](q, self.steps, (total,), (total,), self.visual_length, lambda *shape: torch.empty(shape, **f32))
                res.update(extra)
                r[suffix[1:]] = _EXTRA_RESULTS[suffix[1:]][1](q, extra, total)
            if suffix == "_full":
                o = _lib.Outputs()
                for k in res:
                    setattr(o, k, res[k].data_ptr())
                for k in wide:
                    res[k] = torch.empty(total, D, **f32)
                    setattr(o, k, res[k].data_ptr())
                r["out"] = C.byref(o)
            if suffix == "_similarity":
                res["similarity"] = torch.empty(4, total, **f32)
                r["similarity"] = C.c_void_p(res["similarity"].data_ptr())
            if q.weight_sums:
                res["w_colsum"] = torch.empty(2, D, dtype=torch.float64, device=device)
                r["w_colsum"] = C.c_void_p(res["w_colsum"].data_ptr())
            front = (self._handle, *front)
            if workspace_for is not None:
                ws = self._ensure_workspace(device, getattr(lib, f"iefvad_videos{query}_workspace_bytes")(self._handle, *workspace_for, *query_tail(r)))
                front += (C.c_void_p(ws.data_ptr()), ws.numel())
            rc = getattr(lib, name)(*front, *tail(r))
        if rc != 0:
            raise RuntimeError(name + ": " + _lib.last_error())
        return res

    # ------------------------------------------------------------------ train mode
    def _forward_train(self, img_visual, ev_visual, no_dropout: bool = False) -> Dict[str, torch.Tensor]:
        """`model.train()` forward (/root/reference/train/ucf_train.py:43,60-66): the same dict, differentiable with respect to
        every parameter and to the feature tensors that require grad -- `iefvad_train_forward` keeps the activations,
        `loss.backward()` reaches `iefvad_train_backward` / `iefvad_train_backward_inputs` through `_TrainForward`.
        `no_dropout=True`: the eval() route for features that require grad (dropout off whatever the layers say).  Attention dropout (imf_vad.py:70) uses each layer's `.dropout` (as nn.MultiheadAttention
        keeps it); the mask comes from the library's counter-based generator seeded from torch's RNG (`self.dropout_seed` pins
        it), or from `self.dropout_mask` (uint8 [2, L, B, 8, T, T], 1 = keep) when a test injects one."""
        if self.compute not in ("f32", "bf16x6"):
            raise RuntimeError("iefvad_amd.MMFMIL trains in the fp32-accurate arithmetics only: compute='f32' or 'bf16x6'")
        if self.temporal.embed_dim != 768:
            raise RuntimeError(f"iefvad_amd.MMFMIL trains at D=768 only (this model has D={self.temporal.embed_dim}: "
                               "the D=512 path is the f32 evaluation forward)")
        self._check_dense_inputs(img_visual, ev_visual)
        params = self._params()
        # a feature tensor that requires grad is an input of the node as it is (its dtype, its strides: the widening and the
        # contiguous copy happen inside the node, so the gradient lands on the caller's tensor); the others are detached
        img_in = img_visual if img_visual.requires_grad else img_visual.detach()
        ev_in = ev_visual if ev_visual.requires_grad else ev_visual.detach()
        outs = _TrainForward.apply(self, bool(no_dropout), img_in, ev_in, *params)
        return dict(zip(OUTPUT_KEYS, outs))

    def forward_videos(self, img_rows: torch.Tensor, ev_rows: torch.Tensor, lengths, nan_to_num=True, *, row_scale=None,
                       weight_sums: bool = False, similarity: bool = False, outputs=None, attn_maps=None, row_noise=None, noise_seed=None,
                       noise_rows=None, trajectory: bool = False, fusion_variants=None) -> Dict[str, torch.Tensor]:
        """Scores of whole videos (`iefvad_forward_videos`, include/iefvad.h): `img_rows`, `ev_rows` are the videos' VALID
        feature rows concatenated in list order, [sum(lengths), D] on the device; `lengths` the snippets per video.  The
        chunker (tools.py:100-114), the conditional nan_to_num of test.py:90-95 and the `[0:len]` slicing of
        test.py:119-121,131-138 happen on the device.  Returns `logits`, `w_i_mean`, `w_e_mean`, each [sum(lengths)].
        The robustness sweep's extras (`iefvad_forward_videos_scaled`; with none of them the entry above is called, unchanged):
        `nan_to_num="always"` replaces in every video and modality (test2.py:59-60); `row_scale=(s_img, s_ev)`, contiguous fp32
        DEVICE vectors of sum(lengths) elements (either may be None), multiply the packed rows inside the library's input load,
        after the NaN rule (test2.py:70-77 on valid rows); `weight_sums=True` adds `w_colsum`, a [2, D] float64 device tensor: the
        sums over all valid rows of w_i / w_e (test2.py:86-87), reduced on the device.
        `row_noise=(a_img, a_ev)` with `noise_seed=` (`iefvad_forward_videos_perturbed`), fp32 DEVICE vectors of sum(lengths) elements
        (either may be None), is a further extra of the sweep: behind the scale, packed row r gets a_m[r] * eps added, as in `forward`;
        the noise id is `noise_rows[r]` (int32 DEVICE vector) or the packed row r of the call, in whatever micro-batch pass it falls.  The
        semantics are this package's own ("parity unpinned": the reference implements no noise); without a seed it is a ValueError.
        `similarity=True` (`iefvad_forward_videos_similarity`) adds "similarity", a [4, sum(lengths)] fp32 device tensor: the series of
        `harness.SIMILARITY_KEYS` (test.py:235-238) of every valid snippet, reduced inside the library from the pass's own fused / mu
        rows -- whatever `outputs=` the model was built with; the other three results keep their bits.  The sweep's extras do not
        combine with it (ValueError).
        `outputs="full"`, or an iterable of names from OUTPUT_KEYS (`iefvad_forward_videos_full`), adds those keys of the reference's
        dict (imf_vad.py:152-161) as [sum(lengths), D] fp32 device tensors in packed order: the pass keeps them for its row set and
        copies the valid rows out -- whatever `outputs=` the model was built with; no padding is computed or written, and the other
        three results keep their bits.  An unknown key, `similarity=True` and the sweep's extras are each refused (ValueError).
        `attn_maps=True` or an iterable of layer indices (`iefvad_forward_videos_attn`) adds `image_attn` and `event_attn`,
        [n, sum(lengths), T] fp32 in ascending layer order, and `attn_layers`: row r is the head-averaged attention of valid snippet r
        over the T keys of its chunk (columns >= the chunk's valid rows hold the weight of a pad key, as on the padded route); the other
        three results keep their bits.  It combines with none of `similarity`, `outputs`, `row_scale`, `weight_sums` and
        nan_to_num="always" (ValueError); compute="bf16" and model.train() raise RuntimeError.
        `trajectory=True` (`iefvad_forward_videos_trajectory`) adds `logits_steps`, [steps + 1, sum(lengths)], and `delta_norm`,
        [steps, sum(lengths)], as `forward` does, in packed order, valid rows only; the other three results keep their bits.  It combines
        with none of `attn_maps`, `row_scale`, `row_noise`, `similarity`, `outputs`, `weight_sums` and nan_to_num="always" (ValueError);
        model.train() raises RuntimeError.
        `fusion_variants=True` or an iterable of names (`iefvad_forward_videos_variants`) adds `logits_variants`, [V, sum(lengths)], and
        `fusion_variants`, the names, as `forward` does, in packed order, valid rows only; the other three results keep their bits.  It
        combines with none of `trajectory`, `attn_maps`, `row_scale`, `row_noise`, `similarity`, `outputs`, `weight_sums` and
        nan_to_num="always" (ValueError); compute="fp16x3", model.train() and rows that require grad raise RuntimeError.
        An evaluation entry: nothing it returns is differentiable (rows that require grad get no gradient here; use `forward`)."""
        if not (self.training or row_scale is not None or weight_sums or similarity or outputs is not None or attn_maps is not None
                or row_noise is not None or noise_rows is not None or trajectory or fusion_variants is not None or isinstance(nan_to_num, str)):
            q = _PLAIN      # nothing asked for: nothing to check
        else:
            q = _Request(self.training, _differentiable(img_rows, ev_rows), self.compute, row_scale=row_scale, attn_maps=attn_maps, row_noise=row_noise,
                         noise_seed=noise_seed, noise_rows=noise_rows, trajectory=trajectory, fusion_variants=fusion_variants,
                         similarity=similarity, outputs=outputs, weight_sums=weight_sums, nan_to_num=nan_to_num)
            _check_request(self, q, _VIDEOS_CHECKS)
        self._noise_code()
        if isinstance(nan_to_num, str) and not q.nan_always:
            raise ValueError(f"nan_to_num must be True, False or 'always' (got {nan_to_num!r})")
        nan_mode = 2 if q.nan_always else 1 if nan_to_num else 0
        lens = [int(n) for n in lengths]
        total = sum(lens)
        scales, wide, suffix, pert = (None, None), (), "", None
        if q is not _PLAIN:
            scales = _vector_pair("row_scale", row_scale, total, img_rows.device, "sum of lengths")
            _noise_rules(q.noisy, noise_seed, noise_rows)
            wide, suffix = _row_entry_suffix(q, "iefvad_forward_videos_full")
            if q.noisy:
                pert, _ = _perturb_struct(total, img_rows.device, row_scale, row_noise, noise_seed, noise_rows, "sum of lengths")
        if not (img_rows.is_cuda and ev_rows.is_cuda):
            raise RuntimeError("iefvad_amd.MMFMIL runs on a HIP device only; there is no CPU fallback")
        D = self.temporal.embed_dim
        if img_rows.shape != ev_rows.shape or img_rows.dim() != 2 or tuple(img_rows.shape) != (total, D):
            raise ValueError(f"expected two [{total}, {D}] tensors (sum of lengths x D), got {tuple(img_rows.shape)} and "
                             f"{tuple(ev_rows.shape)}")
        if not lens or min(lens) < 1:
            raise ValueError("every video needs at least one snippet")
        device = img_rows.device
        img, ev = self._prepare_pair(img_rows, ev_rows)
        larr = (C.c_int32 * len(lens))(*lens)
        front = (C.c_void_p(img.data_ptr()), C.c_void_p(ev.data_ptr()), _IN_DTYPES[img.dtype], larr, len(lens), nan_mode)
        if pert is not None:      # the perturbed entry: one struct in the place of the two scale vectors
            front += (C.byref(pert),)
        elif suffix == "_scaled":    # the scaled entry alone takes the two scale vectors, behind nan_to_num
            front += tuple(C.c_void_p(sv.data_ptr()) if sv is not None else None for sv in scales)
        return self._rows_call("iefvad_forward_videos", suffix, q, device, total, front, wide=wide, workspace_for=(larr, len(lens)))

    # ------------------------------------------------------------------ score samples
    def _samples_request(self, who: str, feats, samples, seed, scale) -> tuple:
        """The checks of a score-samples call that need no device -> (S, seed mod 2^64, scale)."""
        if self.training:
            raise RuntimeError(f"iefvad_amd.MMFMIL.{who} is an evaluation entry point; it is not available under model.train() (call model.eval() first)")
        if _differentiable(*feats):
            raise RuntimeError(f"iefvad_amd.MMFMIL.{who} is an evaluation entry point: nothing it returns is differentiable, and a feature tensor "
                               "that requires grad would get no gradient (detach it)")
        if self.compute == "fp16x3":
            raise RuntimeError(f'{who} is not available with compute="fp16x3" (its per-chunk running-max words have no home for the stacked '
                               'sample states); use "f32", "bf16x6" or "bf16"')
        self._noise_code()
        if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples <= _lib.MAX_SAMPLES:
            raise ValueError(f"samples must be an int in 1..{_lib.MAX_SAMPLES} (got {samples!r})")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an int (got {seed!r})")
        scale = float(scale)
        if not (math.isfinite(scale) and scale >= 0.0):
            raise ValueError(f"scale must be finite and >= 0 (got {scale!r})")
        if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in feats):
            raise RuntimeError(f"iefvad_amd.MMFMIL.{who} runs on a HIP device only; there is no CPU fallback (move the inputs with .to('cuda'); "
                               "harness.sample_states_host is the host model of the sampled states)")
        return samples, seed & 0xFFFFFFFFFFFFFFFF, scale

    def forward_samples(self, img_visual, ev_visual, samples: int, seed: int, *, scale: float = 1.0, sample_rows=None) -> Dict[str, torch.Tensor]:
        """One forward and `samples` (1..64) Monte Carlo draws of every snippet's score from the heads' own Gaussians
        (`iefvad_forward_samples`, include/iefvad.h).  The reference never samples; these semantics are this package's own ("parity
        unpinned", as for `row_noise`).  For sample s, modality m, snippet id r and column c: eps = the standard normal of
        `harness.gaussian_rows(harness.sample_seed(seed, s), m, ids, D)`, sd_m = scale exp(0.5 lv_m) / sqrt(f) (f the Student-t factor: the
        variance the fusion itself assigns to m), mu~_m = mu_m + eps sd_m, z0_s = the fusion of the sampled means under the call's own
        precisions, then the `self.steps` refinement steps and the classifier (`harness.sample_states_host` is the host model of z0_s).
        The snippet id is `sample_rows[b*T + t]` (a contiguous int32 DEVICE vector of B*T ids) or b*T + t, so a snippet keeps its draws
        whatever else is in the batch.  Returns what the plain call returns, with unchanged bits, plus `logits_samples` [S, B, T] fp32
        (apply the sigmoid), `score_mean` and `score_std` [B, T]: mean and population standard deviation (ddof = 0) of the S scores,
        formed on the device.  Encoder and heads run once.  model.train(), features that require grad and compute="fp16x3" raise
        RuntimeError, as do host tensors; samples outside 1..64, a negative or non-finite scale raise ValueError.  It takes none of
        `forward`'s keyword extras."""
        S, seed, scale = self._samples_request("forward_samples", (img_visual, ev_visual), samples, seed, scale)
        B, T, D = self._check_dense_inputs(img_visual, ev_visual)
        device = img_visual.device
        if sample_rows is not None and (not isinstance(sample_rows, torch.Tensor) or sample_rows.dtype != torch.int32 or sample_rows.device != device
                                        or sample_rows.numel() != B * T or not sample_rows.is_contiguous()):
            raise ValueError(f"sample_rows must be a contiguous int32 tensor of {B * T} elements (B*T) on {device}")
        q = _Request()
        q.kind, q.samples = "samples", (S, seed, scale, sample_rows)
        return self._dense_call(q, img_visual, ev_visual, B, T, D)

    def forward_videos_samples(self, img_rows, ev_rows, lengths, samples: int, seed: int, *, scale: float = 1.0,
                               nan_to_num: bool = True, sample_rows=None) -> Dict[str, torch.Tensor]:
        """`forward_samples` on whole videos (`iefvad_forward_videos_samples`): the valid rows [sum(lengths), D] and the lengths as
        `forward_videos` takes them.  Returns `logits`, `w_i_mean`, `w_e_mean` with the bits of `forward_videos`, plus `logits_samples`
        [S, sum(lengths)], `score_mean` and `score_std` [sum(lengths)], in packed order, valid rows only.  The snippet id is the packed row
        of the call, in whatever micro-batch pass it falls -- the draws of the dense call on the padded chunks with `sample_rows` = packed
        row -- or `sample_rows[r]` (a contiguous int32 DEVICE vector of sum(lengths) ids).  The refusals are `forward_samples`'s."""
        S, seed, scale = self._samples_request("forward_videos_samples", (img_rows, ev_rows), samples, seed, scale)
        if not isinstance(nan_to_num, bool):
            raise ValueError(f"nan_to_num must be True or False (got {nan_to_num!r})")
        lens = [int(n) for n in lengths]
        total = sum(lens)
        D = self.temporal.embed_dim
        if img_rows.shape != ev_rows.shape or img_rows.dim() != 2 or tuple(img_rows.shape) != (total, D):
            raise ValueError(f"expected two [{total}, {D}] tensors (sum of lengths x D), got {tuple(img_rows.shape)} and {tuple(ev_rows.shape)}")
        if not lens or min(lens) < 1:
            raise ValueError("every video needs at least one snippet")
        device = img_rows.device
        if sample_rows is not None and (not isinstance(sample_rows, torch.Tensor) or sample_rows.dtype != torch.int32 or sample_rows.device != device
                                        or sample_rows.numel() != total or not sample_rows.is_contiguous()):
            raise ValueError(f"sample_rows must be a contiguous int32 tensor of {total} elements (sum of lengths) on {device}")
        img, ev = self._prepare_pair(img_rows, ev_rows)
        larr = (C.c_int32 * len(lens))(*lens)
        q = _Request()
        q.samples = (S, seed, scale, sample_rows)
        front = (C.c_void_p(img.data_ptr()), C.c_void_p(ev.data_ptr()), _IN_DTYPES[img.dtype], larr, len(lens), 1 if nan_to_num else 0)
        return self._rows_call("iefvad_forward_videos", "_samples", q, device, total, front, workspace_for=(larr, len(lens)))

    # ------------------------------------------------------------------ online scores
    def forward_videos_online(self, img_rows, ev_rows, lengths, stride: int, *, history: int = 256, nan_to_num: bool = True) -> Dict[str, torch.Tensor]:
        """What the model would have said live (`iefvad_forward_videos_online`, include/iefvad.h): the valid rows [sum(lengths), D] and
        the lengths as `forward_videos` takes them, every video evaluated over trailing windows.  With 1 <= stride <= history <= 256
        (ValueError otherwise), a video of n snippets has windows j = 1 .. ceil(n / stride): end = min(j stride, n), start =
        max(0, end - history), read0 = (j - 1) stride (`harness.online_windows`).  Window j is the 256-row chunk of rows [start, end) and
        zero rows behind them; it goes through the unchanged model, and only snippets [read0, end) are read out.  Every snippet belongs to
        exactly one window and its results depend on no snippet at or beyond that window's end: the look-ahead is below `stride`, and
        stride=1 is strictly causal.  The reference never does this; these semantics are this package's own ("parity unpinned"), pinned
        by the dense `forward` on host-built windows.  Returns `logits`, `w_i_mean`, `w_e_mean`, each [sum(lengths)] in packed order.
        `nan_to_num=True` is the per-video rule of test.py:90-95, decided over the WHOLE video as everywhere: a NaN anywhere in a video
        changes how all its windows are loaded, so this one rule is not causal.  The encoder runs once per window; heads, fusion,
        refinement and scorer run on the read-out rows only.  model.train(), features that require grad, host tensors and
        compute="fp16x3" raise RuntimeError.  It takes none of `forward_videos`'s keyword extras."""
        stride, history = online_params(stride, history)
        if not isinstance(nan_to_num, bool):
            raise ValueError(f"nan_to_num must be True or False (got {nan_to_num!r})")
        if not (isinstance(img_rows, torch.Tensor) and isinstance(ev_rows, torch.Tensor)):
            raise ValueError("img_rows and ev_rows must be tensors")
        lens = [int(n) for n in lengths]
        total = sum(lens)
        D = self.temporal.embed_dim
        if img_rows.shape != ev_rows.shape or img_rows.dim() != 2 or tuple(img_rows.shape) != (total, D):
            raise ValueError(f"expected two [{total}, {D}] tensors (sum of lengths x D), got {tuple(img_rows.shape)} and {tuple(ev_rows.shape)}")
        if not lens or min(lens) < 1:
            raise ValueError("every video needs at least one snippet")
        who = "iefvad_amd.MMFMIL.forward_videos_online"
        if self.training:
            raise RuntimeError(f"{who} is an evaluation entry point; it is not available under model.train() (call model.eval() first)")
        if _differentiable(img_rows, ev_rows):
            raise RuntimeError(f"{who} is an evaluation entry point: nothing it returns is differentiable, and a feature tensor that requires "
                               "grad would get no gradient (detach it)")
        if self.compute == "fp16x3":
            raise RuntimeError('forward_videos_online is not available with compute="fp16x3" (its operand scales are per chunk and its tail '
                               'keeps whole chunks); use "f32", "bf16x6" or "bf16"')
        self._noise_code()
        if not (img_rows.is_cuda and ev_rows.is_cuda):
            raise RuntimeError(f"{who} runs on a HIP device only; there is no CPU fallback (move the inputs with .to('cuda'); "
                               "harness.online_windows is the host model of the windows)")
        device = img_rows.device
        img, ev = self._prepare_pair(img_rows, ev_rows)
        larr = (C.c_int32 * len(lens))(*lens)
        q = _Request()
        q.online = _lib.Online(stride, history)
        front = (C.c_void_p(img.data_ptr()), C.c_void_p(ev.data_ptr()), _IN_DTYPES[img.dtype], larr, len(lens), 1 if nan_to_num else 0, C.byref(q.online))
        return self._rows_call("iefvad_forward_videos", "_online", q, device, total, front, workspace_for=(larr, len(lens)))
