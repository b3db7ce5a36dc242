"""The enumeration behind tests/test_request_refusals_cpu.py: every way `MMFMIL.forward`, `forward_videos`, `forward_videos_host` and
`harness.score_loader` are asked for their keyword extras, on HOST tensors, so that each case ends in an exception before a device is
touched -- a refusal, or the final "HIP device only" error, which itself pins that nothing else was refused.  `run(group)` gives the
(case id, [exception type, full message]) list of a group; the expected outcomes are tests/request_refusals.json."""
import argparse
import itertools

import torch

import iefvad_amd
from iefvad_amd import harness

COMPUTES = ("f32", "bf16", "fp16x3")
_models = {}


def model(compute="f32", noise_model="StudentT"):
    if (compute, noise_model) not in _models:
        args = argparse.Namespace(visual_layers=1, visual_head=8, num_refinement_steps=3, lambda_ref=0.5, noise_model=noise_model, nu=8)
        _models[compute, noise_model] = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 1, 8, 10, 10, "cpu", args, compute=compute)
    return _models[compute, noise_model]


def configs():
    """(tag, model, train, grad): eval / train x the three arithmetics x features without / with requires_grad, and one model with an
    unsupported noise_model."""
    for train, compute, grad in itertools.product((False, True), COMPUTES, (False, True)):
        yield f"{'train' if train else 'eval'}|{compute}|{'grad' if grad else 'nograd'}", model(compute), train, grad
    yield "eval|f32|nograd|noise_model=Laplace", model("f32", "Laplace"), False, False


def subsets(items, triples):
    """Every subset of size 0, 1 and 2 of `items` ({name: keywords}) whose members name different keywords, then `triples`."""
    names = list(items)
    for k in (0, 1, 2):
        for pick in itertools.combinations(names, k):
            keys = [key for n in pick for key in items[n]]
            if len(set(keys)) == len(keys):
                yield pick
    yield from triples


def outcome(call):
    try:
        call()
    except Exception as e:      # noqa: BLE001 -- the exception IS the result
        return [type(e).__name__, str(e)]
    return ["returned", ""]


def _vec(n, dtype=torch.float32):
    return torch.zeros(n, dtype=dtype)


FORWARD_ITEMS = {
    "timed": dict(timed=True),
    "row_scale": dict(row_scale=(_vec(256), None)),
    "row_noise+seed": dict(row_noise=(_vec(256), None), noise_seed=1),
    "row_noise": dict(row_noise=(None, _vec(256))),
    "noise_rows": dict(noise_rows=_vec(256, torch.int32)),
    "attn_maps=True": dict(attn_maps=True),
    "attn_maps=[99]": dict(attn_maps=[99]),
    "trajectory": dict(trajectory=True),
    "variants=True": dict(fusion_variants=True),
    "variants=mean": dict(fusion_variants=("mean",)),
}
FORWARD_TRIPLES = (
    ("variants=True", "trajectory", "timed"), ("variants=True", "trajectory", "attn_maps=True"), ("variants=True", "attn_maps=[99]", "row_noise"),
    ("variants=mean", "trajectory", "attn_maps=[99]"), ("trajectory", "row_noise+seed", "attn_maps=True"), ("trajectory", "row_noise", "attn_maps=[99]"),
    ("row_noise+seed", "attn_maps=True", "timed"), ("row_noise+seed", "noise_rows", "timed"), ("row_noise", "noise_rows", "attn_maps=True"),
    ("attn_maps=True", "timed", "row_scale"), ("row_scale", "row_noise+seed", "attn_maps=True"), ("row_scale", "row_noise+seed", "trajectory"),
    ("row_scale", "timed", "trajectory"), ("noise_rows", "attn_maps=True", "timed"), ("noise_rows", "trajectory", "variants=True"),
)

# `forward_videos`: two videos' worth of keywords over ONE video of 5 rows; "_rows" / "_lengths" replace the positional arguments
VIDEOS_ITEMS = {
    "row_scale": dict(row_scale=(_vec(5), None)),
    "row_scale=short": dict(row_scale=(None, _vec(4))),
    "row_noise+seed": dict(row_noise=(_vec(5), None), noise_seed=1),
    "row_noise": dict(row_noise=(None, _vec(5))),
    "noise_rows": dict(noise_rows=_vec(5, torch.int32)),
    "attn_maps=True": dict(attn_maps=True),
    "attn_maps=[99]": dict(attn_maps=[99]),
    "trajectory": dict(trajectory=True),
    "variants=True": dict(fusion_variants=True),
    "variants=mean": dict(fusion_variants=("mean",)),
    "similarity": dict(similarity=True),
    "outputs=full": dict(outputs="full"),
    "outputs=nope": dict(outputs=("nope",)),
    "weight_sums": dict(weight_sums=True),
    "nan=always": dict(nan_to_num="always"),
    "nan=sometimes": dict(nan_to_num="sometimes"),
    "lengths=[5,0]": dict(_lengths=[5, 0]),
    "rows=[5,767]": dict(_rows=torch.zeros(5, 767)),
}
VIDEOS_TRIPLES = (
    ("variants=True", "trajectory", "attn_maps=True"), ("variants=True", "similarity", "outputs=full"), ("variants=True", "attn_maps=[99]", "nan=sometimes"),
    ("variants=mean", "trajectory", "similarity"), ("trajectory", "attn_maps=True", "similarity"), ("trajectory", "attn_maps=[99]", "row_noise"),
    ("trajectory", "weight_sums", "nan=always"), ("attn_maps=True", "similarity", "outputs=nope"), ("attn_maps=True", "row_scale=short", "nan=sometimes"),
    ("attn_maps=True", "row_noise", "noise_rows"), ("similarity", "outputs=full", "weight_sums"), ("similarity", "outputs=nope", "nan=always"),
    ("similarity", "row_noise+seed", "noise_rows"), ("outputs=full", "row_scale", "row_noise"), ("outputs=full", "nan=sometimes", "row_scale=short"),
    ("row_scale=short", "row_noise", "noise_rows"), ("row_scale", "row_noise+seed", "similarity"), ("nan=sometimes", "row_noise", "lengths=[5,0]"),
    ("row_scale", "lengths=[5,0]", "rows=[5,767]"), ("weight_sums", "row_noise+seed", "outputs=full"),
)


def _keywords(items, pick):
    kw = {}
    for n in pick:
        kw.update(items[n])
    return kw


def forward_cases():
    for tag, m, train, grad in configs():
        for pick in subsets(FORWARD_ITEMS, FORWARD_TRIPLES):
            def call(m=m, train=train, grad=grad, kw=_keywords(FORWARD_ITEMS, pick)):
                m.train(train)
                x = torch.zeros(1, 256, 768)
                return m(x.clone().requires_grad_(True) if grad else x, x, None, None, None, **kw)
            yield f"forward|{tag}|{'+'.join(pick)}", call


def forward_videos_cases():
    for tag, m, train, grad in configs():
        for pick in subsets(VIDEOS_ITEMS, VIDEOS_TRIPLES):
            def call(m=m, train=train, grad=grad, kw=_keywords(VIDEOS_ITEMS, pick)):
                m.train(train)
                kw = dict(kw)
                rows = kw.pop("_rows", torch.zeros(5, 768))
                lengths = kw.pop("_lengths", [5])
                return m.forward_videos(rows.clone().requires_grad_(True) if grad else rows, rows, lengths, **kw)
            yield f"forward_videos|{tag}|{'+'.join(pick)}", call


def forward_videos_host_cases():
    outputs = {"none": None, "full": "full", "fused": ("fused",), "nope": ("nope",)}
    inputs = {"f32": {}, "f64": dict(_dtype=torch.float64), "wire=f64": dict(wire_dtype=torch.float64), "wire=bf16": dict(wire_dtype=torch.bfloat16),
              "lengths=[0]": dict(_lengths=[0]), "D=767": dict(_width=767)}
    for train, noise, similarity, (oname, out), (iname, extra) in itertools.product(
            (False, True), ("StudentT", "Laplace"), (False, True), outputs.items(), inputs.items()):
        def call(train=train, noise=noise, similarity=similarity, out=out, extra=extra):
            m = model("f32", noise)
            m.train(train)
            kw = dict(extra)
            rows = torch.zeros(5, kw.pop("_width", 768), dtype=kw.pop("_dtype", torch.float32))
            return m.forward_videos_host([rows], [rows], kw.pop("_lengths", [5]), similarity=similarity, outputs=out, **kw)
        yield f"forward_videos_host|{'train' if train else 'eval'}|{noise}|similarity={similarity}|outputs={oname}|{iname}", call


LOADER_ITEMS = {
    "similarity=True": dict(similarity=True),
    "similarity=rows": dict(similarity="rows"),
    "similarity=cols": dict(similarity="cols"),
    "row_outputs": dict(row_outputs="full"),
    "attn_maps": dict(attn_maps=True),
    "attn_maps=False": dict(attn_maps=False),
    "attn_maps=[99]": dict(attn_maps=[99]),
    "trajectory": dict(trajectory=True),
    "variants": dict(fusion_variants=True),
    "steps": dict(steps=1),
    "ragged=False": dict(ragged=False),
    "ragged=True": dict(ragged=True),
    "host_list=False": dict(host_list=False),
    "batch_chunks": dict(batch_chunks=8),
}


class _ReachedTheWalk(Exception):
    """Raised in the place of the result collector of a `score_loader` call on "cuda": every refusal lies before it, and what follows
    would touch the device (and so differ between a machine with a GPU and one without)."""


class _NoSink:
    def __init__(self):
        raise _ReachedTheWalk("no refusal")


def score_loader_cases():
    m = model("f32").eval()
    for dev in ("cpu", "cuda"):
        for pick in subsets(LOADER_ITEMS, ()):
            def call(dev=dev, kw=_keywords(LOADER_ITEMS, pick)):
                m.eval()
                sink = harness._ScoreSink
                if dev == "cuda":
                    harness._ScoreSink = _NoSink
                try:
                    return harness.score_loader(m, [], 256, dev, **kw)
                finally:
                    harness._ScoreSink = sink
            yield f"score_loader|{dev}|{'+'.join(pick)}", call


GROUPS = {"forward": forward_cases, "forward_videos": forward_videos_cases, "forward_videos_host": forward_videos_host_cases,
          "score_loader": score_loader_cases}


def run(group):
    """[(case id, [exception type or "returned", message])] of one group, in the enumeration's order."""
    return [(cid, outcome(call)) for cid, call in GROUPS[group]()]
