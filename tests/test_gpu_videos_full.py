"""The full output dict on the valid-row routes: `MMFMIL.forward_videos(outputs=...)` / `forward_videos_host(outputs=...)`
(`iefvad_forward_videos_full`, `iefvad_forward_videos_host_full`, `iefvad_videos_full_workspace_bytes`; `iefvad_rows_out_wide_kernel`,
csrc/ragged.h) and `harness.score_loader(row_outputs=...)` on top of them.  `-m gpu`.

The reference throughout is the padded route as it was: an outputs="full" model of the same weights on `harness.process_split` chunks,
every tensor sliced `[0:len]` per video.  The model's padded call returns no row means beside its full dict, so the two means of the
reference come from the same handle's `iefvad_forward` with all ten pointers of `iefvad_outputs` set (the padded full route with the
means the C struct offers).  In f32, bf16 and fp16x3 the valid-row route performs every product and sum of the padded one and the new
kernel only copies rows, so equality is bit for bit; bf16x6 picks its kernels by batch size and each route is held to `H.TOL_BIG` /
`H.TOL_LOGIT` against the reference model by the suite's own gates, hence 2 x those between the two routes."""
import argparse
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth
from iefvad_amd import lib as L
from iefvad_amd.model import WIDE_KEYS
from tests import helpers as H

pytestmark = pytest.mark.gpu

EDGE = [37, 255, 256, 257, 512, 1500, 1, 300]      # 3,118 rows, 16 chunks: a one-row chunk, a len % 256 == 0 video, a six-chunk video
N = sum(EDGE)
T = 256
SCORE_KEYS = ("logits", "w_i_mean", "w_e_mean")
ALL_KEYS = SCORE_KEYS + WIDE_KEYS
IN_CODES = {torch.float32: L.IN_F32, torch.float16: L.IN_F16}


def make_model(compute, D=768, L_=2, K=3, **kw):
    sd = synth.make_state_dict(41, D, L_, K)
    args = argparse.Namespace(visual_layers=L_, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, D, 256, D, 8, L_, 8, 10, 10, "cuda", args, compute=compute, **kw)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


@functools.lru_cache(maxsize=None)
def videos(dtype, D=768):
    return tuple(synth.make_video(6, i, int(n), D=D, dtype=dtype) for i, n in enumerate(EDGE))


def pack(vids):
    return (torch.from_numpy(np.concatenate([v[0] for v in vids])).cuda(), torch.from_numpy(np.concatenate([v[1] for v in vids])).cuda())


def pad(vids):
    """Host-side chunker: ([C, 256, D] image, event) on the device and the index of the `[0:len]` slices."""
    D = vids[0][0].shape[1]
    ci = [harness.process_split(v[0], T)[0].reshape(-1, T, D) for v in vids]
    ce = [harness.process_split(v[1], T)[0].reshape(-1, T, D) for v in vids]
    index, off = [], 0
    for c, v in zip(ci, vids):
        index.append(np.arange(off * T, off * T + v[0].shape[0], dtype=np.int64))
        off += c.shape[0]
    return torch.from_numpy(np.concatenate(ci)).cuda(), torch.from_numpy(np.concatenate(ce)).cuda(), torch.from_numpy(np.concatenate(index)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def padded_full(model, img, ev, index):
    """The padded route of an outputs="full" model, valid rows only: logits and the seven [n, D] tensors from `model(img, ev)`, the two
    row means from `iefvad_forward` on the model's handle with every pointer of `iefvad_outputs` set."""
    D = img.shape[-1]
    with torch.no_grad():
        out = model(img, ev, None, None, None)
    ref = {k: out[k].reshape(-1, D)[index].clone() for k in WIDE_KEYS}
    ref["logits"] = out["logits"].reshape(-1)[index].clone()
    lib = L.load_library()
    B = img.shape[0]
    f32 = dict(dtype=torch.float32, device="cuda")
    bufs = {k: torch.empty(B * T, D, **f32) for k in WIDE_KEYS}
    bufs.update({k: torch.empty(B * T, **f32) for k in SCORE_KEYS})
    o = L.Outputs()
    for k, t in bufs.items():
        setattr(o, k, t.data_ptr())
    ws = torch.empty(lib.iefvad_workspace_bytes(model._handle, B), dtype=torch.uint8, device="cuda")
    rc = lib.iefvad_forward(model._handle, _p(img), _p(ev), IN_CODES[img.dtype], B, _p(ws), ws.numel(), C.byref(o),
                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    assert torch.equal(bufs["logits"][index], ref["logits"])          # the same route: the model's call and the handle's
    ref["w_i_mean"], ref["w_e_mean"] = bufs["w_i_mean"][index].clone(), bufs["w_e_mean"][index].clone()
    return ref


@functools.lru_cache(maxsize=None)
def reference(compute, dtype, micro_batch=0, D=768):
    """The padded route, computed once per configuration and left unchanged: key -> the valid rows ([N, D] or [N])."""
    model = make_model(compute, D=D, outputs="full", micro_batch=micro_batch)
    ref = padded_full(model, *pad(videos(dtype, D)))
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    return ref


def rows_call(model, dtype, D=768, **kw):
    rows = pack(videos(dtype, D))
    with torch.no_grad():
        return model.forward_videos(rows[0], rows[1], EDGE, **kw)


def assert_all_equal(got, want, tag, keys=ALL_KEYS):
    assert set(got) == set(keys), (tag, sorted(got))
    D = want["fused"].shape[1]
    for k in keys:
        assert got[k].dtype == torch.float32 and got[k].shape == ((N,) if k in SCORE_KEYS else (N, D)), (tag, k, got[k].shape)
        d = float((got[k] - want[k]).abs().max())
        print(tag, k, "max |rows - padded| =", d)
        assert torch.equal(got[k], want[k]), (tag, k, d)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("compute,micro_batch", [("f32", 0), ("f32", 3), ("bf16", 0), ("bf16", 3), ("fp16x3", 0)])
def test_full_dict_equals_the_padded_route_bit_for_bit(compute, micro_batch, dtype):
    """1. A scores-only model: the library keeps what the caller asked for.  micro_batch = 3: the six-chunk video straddles passes, so
    a pass writes at its own row offset."""
    model = make_model(compute, outputs="scores", micro_batch=micro_batch)
    got = rows_call(model, dtype, outputs="full")
    assert_all_equal(got, reference(compute, dtype, micro_batch), (compute, micro_batch, dtype.__name__))


@pytest.mark.parametrize("built_with", ["full", "weights"])
def test_full_dict_whatever_the_model_was_built_with(built_with):
    """1. `outputs=` of the constructor selects the padded call's dict; the valid-row call's keyword decides on its own."""
    got = rows_call(make_model("f32", outputs=built_with), np.float32, outputs="full")
    assert_all_equal(got, reference("f32", np.float32), built_with)


def test_full_dict_on_the_compacted_row_set(monkeypatch):
    """2. IEFVAD_DENSE_ENCODER=1 (read when the handle is created): the tail runs on the gathered valid rows in packed order, the map
    is the identity over 256-row slabs and there is no table."""
    want = reference("f32", np.float32)
    monkeypatch.setenv("IEFVAD_DENSE_ENCODER", "1")
    got = rows_call(make_model("f32", outputs="scores"), np.float32, outputs="full")
    assert_all_equal(got, want, "dense encoder")


def test_full_dict_d512():
    """3. ViT-B/16 width, f32."""
    got = rows_call(make_model("f32", D=512, outputs="scores"), np.float32, D=512, outputs="full")
    assert_all_equal(got, reference("f32", np.float32, 0, 512), "D=512")


def test_full_dict_bf16x6_within_twice_the_suites_gates():
    """4. bf16x6 picks its kernels by batch size: no exactness.  Each route is within TOL_BIG (TOL_LOGIT) of the reference model by the
    suite's gates, so the two routes are within twice that of each other."""
    want = reference("bf16x6", np.float32)
    got = rows_call(make_model("bf16x6", outputs="scores"), np.float32, outputs="full")
    assert set(got) == set(ALL_KEYS)
    worst = {k: float((got[k] - want[k]).abs().max()) / (2 * H.TOL_BIG) for k in WIDE_KEYS}
    worst["logits"] = float((got["logits"] - want["logits"]).abs().max()) / (2 * H.TOL_LOGIT)
    print("bf16x6 worst |rows - padded| in units of the cap:", worst)
    for k, v in worst.items():
        assert bool(torch.isfinite(got[k]).all()) and v <= 1.0, (k, v)


@pytest.mark.parametrize("compute", ["f32", "bf16", "bf16x6"])
def test_existing_results_keep_their_bits(compute):
    """5. Keeping the wide tensors changes no score (bf16x6: the scorer fold's keep-`fused` branch): the same call with and without
    `outputs`."""
    model = make_model(compute, outputs="scores")
    plain = rows_call(model, np.float32)
    full = rows_call(model, np.float32, outputs="full")
    again = rows_call(model, np.float32)
    assert set(plain) == set(SCORE_KEYS)
    for k in SCORE_KEYS:
        assert torch.equal(full[k], plain[k]), (compute, k, float((full[k] - plain[k]).abs().max()))
        assert torch.equal(again[k], plain[k]), (compute, k)


def test_subsets_return_only_their_keys_with_the_full_calls_bits():
    """6. Any subset is a valid request; "logits" may be named, it is returned anyway."""
    model = make_model("f32", outputs="scores")
    full = rows_call(model, np.float32, outputs="full")
    for names in (("image_logvar", "w_e"), ["w_i"], ("fused", "logits"), "event_mu"):
        wide = [names] if isinstance(names, str) else [k for k in names if k != "logits"]
        got = rows_call(model, np.float32, outputs=names)
        assert set(got) == set(SCORE_KEYS) | set(wide), (names, sorted(got))
        for k in got:
            assert torch.equal(got[k], full[k]), (names, k)
    assert set(rows_call(model, np.float32, outputs=())) == set(SCORE_KEYS)


def test_null_destinations_are_skipped_and_neighbours_stay_untouched():
    """6. A direct C call with only image_logvar and w_e set (and logits): each destination is the middle third of a sentinel-filled
    buffer, and the thirds next to it keep the sentinel -- the kernel writes the asked-for tensors' valid rows and nothing else."""
    model = make_model("f32", outputs="scores")
    full = rows_call(model, np.float32, outputs="full")
    rows = pack(videos(np.float32))
    lib = L.load_library()
    lens = (C.c_int32 * len(EDGE))(*EDGE)
    sentinel = -12345.0
    guard = {k: torch.full((3, N, 768), sentinel, device="cuda") for k in ("image_logvar", "w_e")}
    logits = torch.full((3, N), sentinel, device="cuda")
    o = L.Outputs()
    o.logits = logits[1].data_ptr()
    for k, t in guard.items():
        setattr(o, k, t[1].data_ptr())
    need = lib.iefvad_videos_full_workspace_bytes(model._handle, lens, len(EDGE), C.byref(o))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = lib.iefvad_forward_videos_full(model._handle, _p(rows[0]), _p(rows[1]), L.IN_F32, lens, len(EDGE), 1, _p(ws), need, C.byref(o),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    for k, t in guard.items():
        assert torch.equal(t[1], full[k]), k
        assert bool((t[0] == sentinel).all()) and bool((t[2] == sentinel).all()), k
    assert torch.equal(logits[1], full["logits"])
    assert bool((logits[0] == sentinel).all()) and bool((logits[2] == sentinel).all())


def assert_scores_as_the_plain_entries(got, want, compute):
    """The host-list entry against the device entry as tests/test_gpu_videos.py holds the plain pair: bit for bit, except the bf16
    mode's weight means, whose row sums the ring and the row-block heads kernels add in different orders (<= 1e-6 there)."""
    for k in SCORE_KEYS:
        if compute == "bf16" and k != "logits":
            assert float((got[k] - want[k]).abs().max()) <= 1e-6, k
        else:
            assert torch.equal(got[k], want[k]), (compute, k)


def host_call(model, vids, **kw):
    with torch.no_grad():
        return model.forward_videos_host([torch.from_numpy(v[0]) for v in vids], [torch.from_numpy(v[1]) for v in vids], EDGE, **kw)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_host_list_entry_equals_the_device_entry(compute):
    """7. batch_chunks = 3: several passes on both internal lanes, each with its own home for the weights behind its workspace, each
    writing at its own row offset of the list's tensors."""
    model = make_model(compute, outputs="scores")
    want = rows_call(model, np.float32, outputs="full")
    got = host_call(model, videos(np.float32), batch_chunks=3, outputs="full")
    assert set(got) == set(want) == set(ALL_KEYS)
    for k in WIDE_KEYS:
        assert got[k].shape == (N, 768) and torch.equal(got[k], want[k]), (compute, k, float((got[k] - want[k]).abs().max()))
    assert_scores_as_the_plain_entries(got, want, compute)
    sub = host_call(model, videos(np.float32), batch_chunks=3, outputs=("event_logvar",))
    assert set(sub) == set(SCORE_KEYS) | {"event_logvar"} and torch.equal(sub["event_logvar"], want["event_logvar"])
    assert set(host_call(model, videos(np.float32), batch_chunks=3)) == set(SCORE_KEYS)


@pytest.mark.parametrize("plant_nan", [False, True])
def test_host_passes_cut_into_micro_batches_write_at_the_composed_offset(plant_nan):
    """7. micro_batch = 2 under batch_chunks = 3: the 1,500-row video starts at a non-zero row of the list and spans three micro-batch
    passes of its host pass, so every destination is written at (list offset of the host pass) + (offset of the micro-batch pass in
    it), both above zero.  f32 is bit-identical across pass sizes (`micro_batch=3` above), so the device entry of a
    default-micro-batch model is the reference.  With a NaN planted, the per-video flag (scanned pass by pass) must reach every pass
    of the video; `torch.equal` is false on a NaN that got through."""
    vids = videos(np.float32)
    if plant_nan:          # in the image rows of the 1,500-row video's third chunk
        vids = H.with_nan(vids, EDGE.index(1500), 2 * T + 88, 11)
    rows = pack(vids)
    with torch.no_grad():
        want = make_model("f32", outputs="scores").forward_videos(rows[0], rows[1], EDGE, nan_to_num=True, outputs="full")
    got = host_call(make_model("f32", outputs="scores", micro_batch=2), vids, nan_to_num=True, batch_chunks=3, outputs="full")
    assert set(got) == set(want) == set(ALL_KEYS)
    for k in ALL_KEYS:
        assert torch.equal(got[k], want[k]), (plant_nan, k, float((got[k] - want[k]).abs().max()))


def test_nan_rule_precedes_the_wide_outputs():
    """8. An fp16 video with a NaN and both infinities in its image rows (and clean event rows) among clean videos: test.py:90-95
    replaces in the whole image tensor of that video only (NaN -> 0, +-inf -> +-65504) -- on the host for the padded route, on the
    device for the valid-row one."""
    lengths = [100, 300, 50]
    vids = [list(synth.make_video(9, i, n, dtype=np.float16)) for i, n in enumerate(lengths)]
    vids[1][0][7, 5] = np.nan
    vids[1][0][260, 11] = np.inf
    vids[1][0][299, 700] = -np.inf
    fixed = []
    for img, ev in vids:                                # the rule of test.py:90-95, per modality on the video's whole tensor
        ti, te = torch.from_numpy(img), torch.from_numpy(ev)
        ti = torch.nan_to_num(ti, nan=0.0) if bool(torch.isnan(ti).any()) else ti
        te = torch.nan_to_num(te, nan=0.0) if bool(torch.isnan(te).any()) else te
        fixed.append((ti.numpy(), te.numpy()))
    want = padded_full(make_model("f32", outputs="full"), *pad(fixed))
    rows = pack(vids)
    with torch.no_grad():
        got = make_model("f32", outputs="scores").forward_videos(rows[0], rows[1], lengths, outputs="full")
    for k in ALL_KEYS:
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k], want[k]), (k, float((got[k] - want[k]).abs().max()))


def test_workspace_query_and_a_too_small_workspace():
    """9. The w_i / w_e rows of a pass live behind the base workspace: the query says so, and a call with less is refused by name
    before anything is launched (its destinations keep their sentinel)."""
    model = make_model("f32", outputs="scores")
    rows = pack(videos(np.float32))
    rows_call(model, np.float32)                                             # creates the handle and sets the weights
    lib = L.load_library()
    lens = (C.c_int32 * len(EDGE))(*EDGE)
    nv = len(EDGE)
    base = lib.iefvad_videos_workspace_bytes(model._handle, lens, nv)
    sentinel = -7.0
    logits = torch.full((N,), sentinel, device="cuda")
    w_i = torch.full((N, 768), sentinel, device="cuda")
    fused = torch.full((N, 768), sentinel, device="cuda")
    o_w, o_f, o_s = L.Outputs(), L.Outputs(), L.Outputs()
    o_w.logits, o_w.w_i = logits.data_ptr(), w_i.data_ptr()
    o_f.logits, o_f.fused = logits.data_ptr(), fused.data_ptr()
    o_s.logits = logits.data_ptr()
    wb = lib.iefvad_videos_full_workspace_bytes
    assert base > 0
    for o in (o_w, o_f, o_s):
        assert wb(model._handle, lens, nv, C.byref(o)) >= base
    assert wb(model._handle, lens, nv, None) == base and wb(model._handle, lens, nv, C.byref(o_f)) == base
    assert wb(model._handle, lens, nv, C.byref(o_w)) == base + 2 * 16 * 256 * 768 * 4     # [2, R, D] floats, R = the 16 chunks' rows
    assert wb(model._handle, None, nv, C.byref(o_w)) == 0 and wb(model._handle, lens, 0, C.byref(o_w)) == 0
    full = wb(model._handle, lens, nv, C.byref(o_w))
    ws = torch.empty(full, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(o, wsb):
        rc = lib.iefvad_forward_videos_full(model._handle, _p(rows[0]), _p(rows[1]), L.IN_F32, lens, nv, 1, _p(ws), wsb, C.byref(o), stream)
        return rc, L.last_error()

    rc, msg = call(o_w, base)
    assert rc != 0 and msg.startswith("iefvad_forward_videos_full:") and "workspace too small" in msg, msg
    rc, msg = call(o_w, full - 1)
    assert rc != 0 and msg.startswith("iefvad_forward_videos_full:") and "workspace too small" in msg, msg
    torch.cuda.synchronize()
    assert bool((logits == sentinel).all()) and bool((w_i == sentinel).all())       # nothing was launched
    assert call(o_f, base)[0] == 0                                                  # without the weights the base workspace is enough
    assert call(o_w, full)[0] == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(w_i).all()) and bool((w_i > 0).all()) and bool((w_i < 1).all()) and bool((fused != sentinel).any())


# ------------------------------------------------------------------------------------------------
# 10. the harness on the config-1 set
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def config1(tmp_path_factory, golden_dir):
    return H.write_config1_set(tmp_path_factory.mktemp("cfg1full"), golden_dir)


def config1_model(sd, **kw):
    a = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=10, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, "cuda", a, **kw)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


def test_score_loader_row_outputs_on_the_config1_set(config1):
    """10. Both valid-row routes (the host-list walk and the `forward_videos` loop) against the padded route video by video: the
    full-dict model on the chunks `score_loader` itself would feed it (`_unpack_item`: one NaN element, one fp16 file), sliced [0:len].
    The scores are those of the call without `row_outputs`."""
    g, args, gt, sd = config1
    names = ("image_logvar", "event_logvar")
    lengths = [int(n) for n in g["lengths"]]
    full = config1_model(sd, outputs="full")
    want = {k: [] for k in names}
    with torch.no_grad():
        for item in harness.get_test_loader(args):
            img, ev, _, n = harness._unpack_item(item, 256, "ucfcrime", None)
            out = full(img.cuda(), ev.cuda(), None, None, None)
            for k in names:
                want[k].append(out[k].reshape(-1, 768)[:n].clone())
    assert [w.shape[0] for w in want[names[0]]] == lengths
    model = config1_model(sd, outputs="scores")
    for host_list in (True, False):
        plain = harness.score_loader(model, harness.get_test_loader(args), 256, "cuda:0", "ucfcrime", batch_chunks=4, host_list=host_list)
        got = harness.score_loader(model, harness.get_test_loader(args), 256, "cuda:0", "ucfcrime", batch_chunks=4, host_list=host_list,
                                   row_outputs=names)
        assert len(got) == len(plain) == 4 and got[1] == plain[1]
        for j in (0, 2, 3):
            for a, b in zip(got[j], plain[j]):
                assert np.array_equal(a, b), (host_list, j)
        last = harness.score_loader.last_result
        assert set(last) == {"row_outputs", "row_offsets"} and set(last["row_outputs"]) == set(names)
        offs = last["row_offsets"]
        assert offs.dtype == np.int64 and list(np.diff(offs)) == lengths and offs[0] == 0
        for k in names:
            t = last["row_outputs"][k]
            assert t.is_cuda and t.dtype == torch.float32 and t.shape == (sum(lengths), 768)
            for i, w in enumerate(want[k]):
                assert torch.equal(t[offs[i]:offs[i + 1]], w), (host_list, k, i)
