"""The encoder's head-averaged attention maps on the device: `MMFMIL.forward(attn_maps=)` / `forward_videos(attn_maps=)`
(`iefvad_forward_attn`, `iefvad_forward_videos_attn`; `iefvad_attention_maps_kernel`, csrc/attention_maps.h) and
`harness.score_loader(attn_maps=)` on top of them.  `-m gpu`.

Accuracy is held against the reference's own captures (tests/golden/attn_*.npz, made by make_golden_attn.py): per layer and modality
|map - fp64 capture| <= 3 x attn_floor, where attn_floor is the reference's fp32-versus-fp64 difference on the same maps -- the
project's margin over a reference-side floor, nothing in the gate comes from the kernel.  bf16x6 and fp16x3 form the maps in fp32 from
their own q | k | v; their layer-1 inputs move inside the fp32 gates, so they are held to twice the gate (the precedent of
test_gpu_videos_full.py).  Everything else is exact: the same bits with and without the request, on replay, across batch
compositions, and between the valid-row route and the dense route on host-padded chunks."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth
from iefvad_amd import lib as L
from tests import attn_cases as A
from tests import helpers as H

pytestmark = pytest.mark.gpu

T = 256
# the query-block skip (1, 37: the second half of the queries is padding; 128 / 129: on either side of it), the pad-key columns
# (every length < 256), a full chunk (256: the all-zero chunk of the padded route is not built here) and two-chunk videos (257, 300)
LENGTHS = [1, 37, 128, 129, 255, 256, 257, 300]
N = sum(LENGTHS)
SCORE_KEYS = ("logits", "w_i_mean", "w_e_mean")
SENTINEL = -7.0


@functools.lru_cache(maxsize=None)
def fixture_model(name, compute="f32", **kw):
    g, cfg, sd, _, _ = A.load_fixture(name)
    m = iefvad_amd.MMFMIL(14, cfg["D"], 256, cfg["D"], 8, cfg["L"], 8, 10, 10, "cuda", A.model_args(cfg["L"], cfg["K"]), compute=compute, **kw)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


@functools.lru_cache(maxsize=None)
def edge_model(compute="f32", D=768, micro_batch=0, dense_encoder=False, outputs="full"):
    """`dense_encoder` only keys the cache: IEFVAD_DENSE_ENCODER is read when the handle is created, i.e. on the model's first call."""
    sd = synth.sharpen_qk(synth.make_state_dict(41, D, 2, 2), (8, 4))
    m = iefvad_amd.MMFMIL(14, D, 256, D, 8, 2, 8, 10, 10, "cuda", A.model_args(2, 2), compute=compute, micro_batch=micro_batch, outputs=outputs)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


@functools.lru_cache(maxsize=None)
def videos(dtype=np.float32, D=768, nan_video=-1):
    vids = [synth.make_video(6, i, int(n), D=D, dtype=dtype) for i, n in enumerate(LENGTHS)]
    if nan_video >= 0:
        vids = H.with_nan(vids, nan_video, 7, 5)
    return tuple(vids)


def pack(vids):
    return (torch.from_numpy(np.concatenate([v[0] for v in vids])).cuda(), torch.from_numpy(np.concatenate([v[1] for v in vids])).cuda())


def pad(vids):
    """Host-side chunker: ([C, 256, D] image, event) on the device and the index of the `[0:len]` rows."""
    D = vids[0][0].shape[1]
    ci = [harness.process_split(v[0], T)[0].reshape(-1, T, D) for v in vids]
    ce = [harness.process_split(v[1], T)[0].reshape(-1, T, D) for v in vids]
    index, off = [], 0
    for c, v in zip(ci, vids):
        index.append(np.arange(off * T, off * T + v[0].shape[0], dtype=np.int64))
        off += c.shape[0]
    return torch.from_numpy(np.concatenate(ci)).cuda(), torch.from_numpy(np.concatenate(ce)).cuda(), torch.from_numpy(np.concatenate(index)).cuda()


def dense(model, img, ev, **kw):
    with torch.no_grad():
        out = model(img, ev, None, None, None, **kw)
    torch.cuda.synchronize()
    return out


def rows(model, vids, lengths=LENGTHS, **kw):
    img, ev = pack(vids)
    with torch.no_grad():
        out = model.forward_videos(img, ev, lengths, **kw)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def padded_reference(dtype=np.float32, D=768, nan_video=-1):
    """The dense route on host-padded chunks (the host applies test.py:90-95 to the NaN video), `[0:len]` rows: computed once per
    configuration and left unchanged."""
    vids = videos(dtype, D, nan_video)
    if nan_video >= 0:
        vids = [tuple(np.nan_to_num(x, nan=0.0) if np.isnan(x).any() else x for x in v) for v in vids]
    img, ev, index = pad(vids)
    out = dense(edge_model(D=D), img, ev, attn_maps=True)
    ref = {k: out[k].reshape(2, -1, T)[:, index].clone() for k in ("image_attn", "event_attn")}
    ref["logits"] = out["logits"].reshape(-1)[index].clone()
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    return ref


def check_against_fixture(name, out, gate_factor, tag, copies=1):
    """Every copy of the fixture's chunks in `out` against the capture; returns the worst |d| / floor."""
    g, cfg, _, _, _ = A.load_fixture(name)
    B, worst = cfg["B"], 0.0
    assert out["attn_layers"] == tuple(range(cfg["L"]))
    for m, mod in enumerate(A.MODALITIES):
        got = out[f"{mod}_attn"]
        assert got.dtype == torch.float32 and tuple(got.shape) == (cfg["L"], B * copies, T, T)
        got = got.double().cpu().numpy()
        for l in range(cfg["L"]):
            for c in range(copies):
                d = np.abs(A.fixture_rows(g, got[l, c * B:(c + 1) * B], m, l) - g[mod][l]).max()
                ratio = d / g["attn_floor"][m, l]
                worst = max(worst, ratio)
                print(f"{tag} {name} {mod} layer {l} copy {c}: max |d| = {d:.3e}, floor = {g['attn_floor'][m, l]:.3e}, ratio = {ratio:.3f}")
                assert d <= gate_factor * g["attn_floor"][m, l], (tag, name, mod, l, d, g["attn_floor"][m, l])
    print(f"{tag} {name}: worst |d| / floor = {worst:.3f} (gate {gate_factor})")
    return worst


def assert_rows_sum_to_one(t):
    s = t.double().sum(-1)
    d = float((s - 1).abs().max())
    assert d <= 2.0 ** -16, d          # 256 roundings of terms that sum to one: loose on purpose


@pytest.mark.parametrize("name", A.FIXTURES)
def test_f32_maps_match_the_reference_within_three_floors(name):
    _, _, _, img, ev = A.load_fixture(name)
    out = dense(fixture_model(name), torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda(), attn_maps=True)
    check_against_fixture(name, out, 3.0, "f32")
    for k in ("image_attn", "event_attn"):
        assert_rows_sum_to_one(out[k])


@pytest.mark.parametrize("compute", ["bf16x6", "fp16x3"])
@pytest.mark.parametrize("name", ["attn_flat_k3", "attn_sharp_k3"])
def test_split_arithmetics_are_held_to_twice_the_gate_at_b8(name, compute):
    """B = 8: the fixture's two chunks four times (chunks are independent batch rows)."""
    _, _, _, img, ev = A.load_fixture(name)
    img8, ev8 = (torch.from_numpy(np.concatenate([x] * 4)).cuda() for x in (img, ev))
    out = dense(fixture_model(name, compute), img8, ev8, attn_maps=True)
    check_against_fixture(name, out, 6.0, compute, copies=4)
    for k in ("image_attn", "event_attn"):
        assert_rows_sum_to_one(out[k])


@pytest.mark.parametrize("compute", ["f32", "bf16x6"])
def test_asking_changes_no_other_result(compute):
    _, _, _, img, ev = A.load_fixture("attn_sharp_k3")
    di, de = torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()
    model = fixture_model("attn_sharp_k3", compute)
    plain = dense(model, di, de)
    asked = dense(model, di, de, attn_maps=True)
    assert set(asked) == set(iefvad_amd.OUTPUT_KEYS) | {"image_attn", "event_attn", "attn_layers"}
    for k in iefvad_amd.OUTPUT_KEYS:
        assert torch.equal(plain[k], asked[k]), k
    # the valid-row entry: scores and the two row means
    vids = videos()
    emodel = edge_model(compute, outputs="scores")
    a, b = rows(emodel, vids), rows(emodel, vids, attn_maps=[1])
    assert set(b) == set(SCORE_KEYS) | {"image_attn", "event_attn", "attn_layers"} and b["attn_layers"] == (1,)
    for k in SCORE_KEYS:
        assert torch.equal(a[k], b[k]), k


def test_graph_replay_is_intact_around_a_maps_call():
    """B = 1 replays a captured graph; the maps call launches directly on the same handle and workspace."""
    _, _, _, img, ev = A.load_fixture("attn_sharp_k3")
    di, de = torch.from_numpy(img[:1]).cuda(), torch.from_numpy(ev[:1]).cuda()
    model = fixture_model("attn_sharp_k3")
    first = dense(model, di, de)               # captures
    m1 = dense(model, di, de, attn_maps=True)
    again = dense(model, di, de)               # replays
    m2 = dense(model, di, de, attn_maps=True)
    for k in iefvad_amd.OUTPUT_KEYS:
        assert torch.equal(first[k], again[k]) and torch.equal(first[k], m1[k]) and torch.equal(first[k], m2[k]), k
    for k in ("image_attn", "event_attn"):
        assert torch.equal(m1[k], m2[k]), k


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def c_dense(model, img, ev, maps):
    lib = L.load_library()
    B = img.shape[0]
    logits = torch.empty(B * T, device="cuda")
    o = L.Outputs()
    o.logits = logits.data_ptr()
    ws = torch.empty(lib.iefvad_workspace_bytes(model._handle, B), dtype=torch.uint8, device="cuda")
    rc = lib.iefvad_forward_attn(model._handle, _p(img), _p(ev), L.IN_F32, B, _p(ws), ws.numel(), C.byref(o), C.byref(maps),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, L.last_error(), logits


def test_unrequested_layers_and_modalities_are_left_alone():
    _, _, _, img, ev = A.load_fixture("attn_sharp_k3")
    di, de = torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()
    model = fixture_model("attn_sharp_k3")
    full = dense(model, di, de, attn_maps=True)
    assert torch.equal(dense(model, di, de, attn_maps=[1])["image_attn"][0], full["image_attn"][1])
    # one buffer of three maps, only the middle one handed over (image, layer 1): its neighbours keep the sentinel
    buf = torch.full((3, 2 * T, T), SENTINEL, device="cuda")
    maps = L.AttnMaps()
    maps.image[1] = buf[1].data_ptr()
    rc, msg, logits = c_dense(model, di, de, maps)
    assert rc == 0, msg
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[2] == SENTINEL).all())
    assert torch.equal(buf[1].reshape(2, T, T), full["image_attn"][1])
    assert torch.equal(logits, full["logits"].reshape(-1))
    # event, layer 0 alone
    buf.fill_(SENTINEL)
    maps = L.AttnMaps()
    maps.event[0] = buf[1].data_ptr()
    rc, msg, _ = c_dense(model, di, de, maps)
    assert rc == 0, msg
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[2] == SENTINEL).all())
    assert torch.equal(buf[1].reshape(2, T, T), full["event_attn"][0])


def assert_rows_equal_padding(got, ref, tag):
    assert got["attn_layers"] == (0, 1)
    for k in ("image_attn", "event_attn"):
        assert got[k].dtype == torch.float32 and tuple(got[k].shape) == (2, N, T), (tag, k, got[k].shape)
        d = float((got[k] - ref[k]).abs().max())
        print(tag, k, "max |rows - padded| =", d)
        assert torch.equal(got[k], ref[k]), (tag, k, d)
        assert_rows_sum_to_one(got[k])
    assert torch.equal(got["logits"], ref["logits"]), tag


@pytest.mark.parametrize("micro_batch", [0, 3])
def test_valid_rows_equal_padding_bit_for_bit(micro_batch):
    """micro_batch = 3: passes of three chunks; the two-chunk video of 257 rows straddles passes 2 and 3."""
    ref = padded_reference()
    got = rows(edge_model(micro_batch=micro_batch), videos(), attn_maps=True)
    assert_rows_equal_padding(got, ref, f"micro_batch={micro_batch}")
    # the pad-key columns hold the pad key's weight: all equal within a row, and not zero (the reference attends to its zero rows)
    r0 = LENGTHS[0]                        # video 1 (37 rows) starts at packed row 1
    row = got["image_attn"][0, r0]
    assert bool((row[LENGTHS[1]:] == row[LENGTHS[1]]).all()) and float(row[LENGTHS[1]]) > 0


def test_valid_rows_equal_padding_fp16_rows():
    ref = padded_reference(np.float16)
    assert_rows_equal_padding(rows(edge_model(), videos(np.float16), attn_maps=True), ref, "fp16 rows")


def test_valid_rows_equal_padding_dense_encoder(monkeypatch):
    """IEFVAD_DENSE_ENCODER=1 (read when the handle is created): whole chunks in the encoder, the dense kernel reads and the chunk
    table decides what is written."""
    ref = padded_reference()
    monkeypatch.setenv("IEFVAD_DENSE_ENCODER", "1")
    model = edge_model(dense_encoder=True)
    got = rows(model, videos(), attn_maps=True)
    monkeypatch.delenv("IEFVAD_DENSE_ENCODER")
    assert_rows_equal_padding(got, ref, "dense encoder")


def test_valid_rows_equal_padding_d512():
    ref = padded_reference(np.float32, 512)
    assert_rows_equal_padding(rows(edge_model(D=512), videos(np.float32, 512), attn_maps=True), ref, "D=512")


def test_valid_rows_equal_padding_nan_rule():
    """One NaN in the image rows of video 1: the device applies test.py:90-95 to that video, the host did for the reference."""
    ref = padded_reference(np.float32, 768, 1)
    got = rows(edge_model(), videos(np.float32, 768, 1), attn_maps=True)
    assert_rows_equal_padding(got, ref, "NaN rule")


def test_batch_composition_does_not_move_the_bits():
    _, _, _, img, ev = A.load_fixture("attn_sharp_k3")
    model = fixture_model("attn_sharp_k3")
    one = dense(model, torch.from_numpy(img[1:2]).cuda(), torch.from_numpy(ev[1:2]).cuda(), attn_maps=True)
    i3 = np.concatenate([img[0:1], img[1:2], img[0:1]])
    e3 = np.concatenate([ev[0:1], ev[1:2], ev[0:1]])
    three = dense(model, torch.from_numpy(i3).cuda(), torch.from_numpy(e3).cuda(), attn_maps=True)
    for k in ("image_attn", "event_attn"):
        assert torch.equal(one[k][:, 0], three[k][:, 1]), k
        assert torch.equal(three[k][:, 0], three[k][:, 2]), k


def test_refusals_on_the_device():
    _, cfg, _, img, ev = A.load_fixture("attn_sharp_k3")
    di, de = torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()
    model = fixture_model("attn_sharp_k3")
    dense(model, di, de)                                           # creates the handle
    buf = torch.full((2 * T, T), SENTINEL, device="cuda")
    maps = L.AttnMaps()
    maps.image[cfg["L"]] = buf.data_ptr()                          # layer index L: the model has layers 0 .. L - 1
    rc, msg, _ = c_dense(model, di, de, maps)
    assert rc != 0 and msg.startswith("iefvad_forward_attn:") and f"layer {cfg['L']}" in msg, msg
    maps = L.AttnMaps()
    maps.event[0] = buf.data_ptr() + 4
    rc, msg, _ = c_dense(model, di, de, maps)
    assert rc != 0 and "16-byte aligned" in msg, msg
    rc, msg, _ = c_dense(model, di, de, L.AttnMaps())
    assert rc != 0 and "every map is null" in msg, msg
    # compute = BF16: refused by name by the library (the Python layer refuses earlier, so the handle is called directly)
    bmodel = fixture_model("attn_sharp_k3", "bf16")
    dense(bmodel, di, de)
    maps = L.AttnMaps()
    maps.image[0] = buf.data_ptr()
    rc, msg, _ = c_dense(bmodel, di, de, maps)
    assert rc != 0 and "compute = BF16" in msg, msg
    lib = L.load_library()
    lens = (C.c_int32 * 1)(T)
    ws = torch.empty(lib.iefvad_videos_workspace_bytes(bmodel._handle, lens, 1), dtype=torch.uint8, device="cuda")
    vec = torch.empty(T, device="cuda")
    rc = lib.iefvad_forward_videos_attn(bmodel._handle, _p(di), _p(de), L.IN_F32, lens, 1, 1, _p(ws), ws.numel(), _p(vec), None, None,
                                        C.byref(maps), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0 and L.last_error().startswith("iefvad_forward_videos_attn:") and "compute = BF16" in L.last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())                           # nothing was launched
    with pytest.raises(RuntimeError, match='compute="bf16"'):
        dense(bmodel, di, de, attn_maps=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(torch.from_numpy(img), torch.from_numpy(ev), None, None, None, attn_maps=True)


LIST_LENGTHS = [37, 300, 256, 1, 129, 257]


def list_items(lengths=LIST_LENGTHS, classes=("Normal", "Abuse", "Normal", "Arson", "Normal", "Abuse")):
    vids = [synth.make_video(9, i, n) for i, n in enumerate(lengths)]
    items = [(torch.from_numpy(v[0])[None], torch.from_numpy(v[1])[None], (c,), torch.tensor([n])) for v, n, c in zip(vids, lengths, classes)]
    return vids, items


def test_score_loader_attn_maps_matches_per_video_forward_videos():
    lengths = LIST_LENGTHS
    vids, items = list_items()
    model = edge_model()
    plain = harness.score_loader(model, items, T, "cuda:0", "ucfcrime", batch_chunks=3)
    got = harness.score_loader(model, items, T, "cuda:0", "ucfcrime", batch_chunks=3, attn_maps=[1])
    assert len(got) == len(plain) == 4
    for a, b in zip(plain[0], got[0]):
        assert np.array_equal(a, b)
    res = harness.score_loader.last_result["attn_maps"]
    assert res["layers"] == (1,) and res["row_offsets"].tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist()
    assert tuple(res["image"].shape) == tuple(res["event"].shape) == (1, sum(lengths), T) and res["image"].is_cuda
    for i, (v, n) in enumerate(zip(vids, lengths)):
        one = rows(model, [v], [n], attn_maps=[1])
        lo, hi = res["row_offsets"][i], res["row_offsets"][i + 1]
        assert torch.equal(res["image"][:, lo:hi], one["image_attn"]), i
        assert torch.equal(res["event"][:, lo:hi], one["event_attn"]), i


def test_test_functions_surface_the_maps_and_keep_their_results():
    """`attn_maps=` lands in `last_result`; the returned tuple is the one without it, and `attn=True` keeps the reference's empty list."""
    import argparse
    lengths = LIST_LENGTHS + [20, 64, 100, 12, 8, 50, 90, 130]       # one video per UCF class key: the metric tail concatenates every class
    assert len(lengths) == len(synth.UCF_CLASSES)
    _, items = list_items(lengths, synth.UCF_CLASSES)
    n = sum(lengths)
    args = argparse.Namespace(dataset="ucfcrime", exp_name="t")
    gt = synth.make_gt(9, n)
    model = edge_model()
    plain = harness.test(args, model, items, T, None, gt, "cuda:0")
    assert "attn_maps" not in harness.test.last_result
    got = harness.test(args, model, items, T, None, gt, "cuda:0", attn_maps=True)
    assert got == plain
    res = harness.test.last_result
    for a, b in zip(res["scores"], harness.score_loader(model, items, T, "cuda:0", "ucfcrime", batch_chunks=64)[0]):
        assert np.array_equal(a, b)
    maps = res["attn_maps"]
    assert maps["layers"] == (0, 1) and tuple(maps["image"].shape) == tuple(maps["event"].shape) == (2, n, T) and maps["event"].is_cuda
    assert_rows_sum_to_one(maps["image"])
    ret = harness.ucf_test(args, model, items, T, None, gt, "cuda:0", True, attn_maps=[1])
    assert len(ret) == 4 and ret[2] == [] and ret[:2] == plain
    assert harness.ucf_test.last_result["attn_maps"]["layers"] == (1,)
    assert torch.equal(harness.ucf_test.last_result["attn_maps"]["event"][0], maps["event"][1])
    with pytest.raises(ValueError, match="attn_maps does not combine with similarity"):
        harness.test(args, model, items, T, None, gt, "cuda:0", vis=True, attn_maps=True)
