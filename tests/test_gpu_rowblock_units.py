"""Per-kernel parity of the bf16 mode's row-block kernels at fp32-ACCUMULATION tolerance (round-4 verdict, weak point 6).

The whole-pipeline tests of tests/test_gpu_bf16.py compare the mode with an fp64 evaluation of its data flow and have to allow for
cascades: one operand element whose fp32 value sits on a bf16 rounding boundary flips, and the flip travels through twenty
projections.  Here every stage runs ALONE -- `iefvad_rowblock_unit` (include/iefvad.h) launches the production kernel symbol the
forward launches, on rows the test supplies -- against an fp64 host evaluation of that stage on the same bf16-rounded operands
(a product of two bf16 values is exact in fp32, so what separates the two is the fp32 accumulation order, ~1e-6).  Where a stage
rounds to bf16 itself, the test computes WHICH elements lie within `tol` of a rounding boundary: only those may differ, only by
one bf16 step, and their effect downstream is bounded element by element.  A wrong fragment map, a swapped bias or a mis-ordered
k index costs >= 1e-3 and fails everywhere.

Reference lines: /root/reference/model/imf_vad.py:115-117,121-123 (encoder), :125-144 (heads, fusion), :146-150 (refinement, scorer).
`-m gpu`; the C ABI through ctypes."""
import argparse
import ctypes as C
import math

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, lib as L, synth

pytestmark = pytest.mark.gpu
D = 768
# 64-row blocks: 32 -> the one-block-per-workgroup kernels; 257 -> the persistent ones (>= 2 blocks per workgroup), uneven walk
ROWS = [2048, 16448]
TOL_ACC = 3e-6          # |fp32-accumulated value - fp64 value| allowed before a bf16 rounding is called "on the boundary"
GATE = 2e-5             # the fp32 gate of SURVEY 8c for 768-d outputs


def bf(x64: torch.Tensor) -> torch.Tensor:
    """fp64 -> nearest bf16 -> fp64"""
    return x64.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def bf_ulp(x64: torch.Tensor) -> torch.Tensor:
    """spacing of the bf16 grid at |x| (8 significant bits)"""
    e = torch.floor(torch.log2(x64.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def handle(L_, K, seed):
    sd = synth.make_state_dict(seed, D, L_, K)
    a = argparse.Namespace(visual_layers=L_, visual_head=8, num_refinement_steps=K, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m = iefvad_amd.MMFMIL(14, D, 256, D, 8, L_, 8, 10, 10, "cuda", a, compute="bf16", outputs="full")
    m.load_state_dict(sd)
    m = m.to("cuda:0").eval()
    with torch.cuda.device(0):
        m._ensure_handle(torch.device("cuda:0"))
        m._ensure_weights(torch.device("cuda:0"), torch.cuda.current_stream().cuda_stream)
    return m, {k: v.double() for k, v in sd.items()}


def run(model, stage, layer, rows, **ptrs):
    io = L.UnitIO()
    for name, val in ptrs.items():
        if isinstance(val, (list, tuple)):
            arr = getattr(io, name)
            for i, t in enumerate(val):
                arr[i] = t.data_ptr() if t is not None else None
        else:
            setattr(io, name, val.data_ptr() if val is not None else None)
    rc = L.load_library().iefvad_rowblock_unit(model._handle, stage, layer, rows, C.byref(io), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()


def check_bf16_output(got: torch.Tensor, ref64: torch.Tensor, tol: float, what: str):
    """`got` (bf16 from the kernel) against the fp64 value: equal to bf16(ref) wherever ref is further than `tol` from a rounding
    boundary; on a boundary either neighbour.  Returns the fraction of boundary elements (values large enough that one bf16 step
    exceeds 2 tol; smaller ones are trivially "on a boundary" and do not count)."""
    g = got.to(torch.float64).cpu()
    lo, hi = bf(ref64 - tol), bf(ref64 + tol)
    fragile = lo != hi
    exact = bf(ref64)
    assert torch.equal(g[~fragile], exact[~fragile]), (what, float((g - exact)[~fragile].abs().max()))
    assert bool(((g >= lo) & (g <= hi))[fragile].all()), what        # one of the two neighbours (for tiny values, whose bf16 step is below `tol`, anything between)
    frac = float((fragile & (bf_ulp(ref64) > 2 * tol)).double().mean())
    assert frac < 0.08, (what, frac)
    return frac


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("layer", [0, 1])
def test_inproj_kernel_alone(rows, layer):
    """iefvad_inproj_chain_{f32in,bf16}_kernel: q | k | v = x W_in^T + b_in, q pre-scaled, stored as bf16 head-major."""
    torch.set_num_threads(harness.host_cpu_share())
    model, W = handle(2, 1, 61)
    g = torch.Generator().manual_seed(rows + layer)
    x = [torch.randn(rows, D, generator=g) * 0.7 for _ in range(2)]
    if layer > 0:
        x = [t.to(torch.bfloat16) for t in x]
    xd = [t.cuda() for t in x]
    y = [torch.empty(3, 8, rows, 96, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    run(model, L.UNIT_INPROJ, layer, rows, x=xd, y=y)
    alpha = float(np.float32(np.float32(1.0) / np.sqrt(np.float32(96.0))) * np.float32(1.4426950408889634))
    for m, name in enumerate(("image", "event")):
        p = f"temporal.{name}_attn_layers.{layer}."
        ref = bf(x[m].double()) @ bf(W[p + "in_proj_weight"]).t() + W[p + "in_proj_bias"]
        ref[:, :D] *= alpha
        ref = ref.reshape(rows, 3, 8, 96).permute(1, 2, 0, 3).contiguous()          # [3][8 heads][rows][96]
        frac = check_bf16_output(y[m], ref, TOL_ACC, f"in_proj {name} layer {layer}")
        print(f"in_proj {name} layer {layer} rows {rows}: {frac:.2e} of the outputs on a bf16 rounding boundary")


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("layer", [0, 1])
def test_outproj_layernorm_kernel_alone(rows, layer):
    """iefvad_outproj_ln_{chain,pchain}_bf16_kernel: LayerNorm(resid + att W_o^T + b_o), plus the whitening LayerNorm behind the last
    layer (layer 1 of 2); fp32 rows and their bf16 copy."""
    torch.set_num_threads(harness.host_cpu_share())
    model, W = handle(2, 1, 62)
    g = torch.Generator().manual_seed(7 * rows + layer)
    att = [(torch.randn(rows, D, generator=g) * 0.5).to(torch.bfloat16) for _ in range(2)]
    res = [torch.randn(rows, D, generator=g) * 0.8 for _ in range(2)]
    y = [torch.empty(rows, D, device="cuda") for _ in range(2)]
    yb = [torch.empty(rows, D, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    run(model, L.UNIT_OUTPROJ_LN, layer, rows, x=[t.cuda() for t in att], resid=[t.cuda() for t in res], y=y, yb=yb)

    def ln(v, gk, bk):
        c = v - v.mean(-1, keepdim=True)
        return c / torch.sqrt((c * c).mean(-1, keepdim=True) + 1e-5) * W[gk] + W[bk]

    for m, name in enumerate(("image", "event")):
        p = f"temporal.{name}_attn_layers.{layer}."
        v = res[m].double() + att[m].double() @ bf(W[p + "out_proj.weight"]).t() + W[p + "out_proj.bias"]
        v = ln(v, f"temporal.{name}_norms.{layer}.weight", f"temporal.{name}_norms.{layer}.bias")
        if layer == 1:
            v = ln(v, f"temporal.whiten_{name}.weight", f"temporal.whiten_{name}.bias")
        err = float((y[m].cpu().double() - v).abs().max())
        print(f"out_proj + LN {name} layer {layer} rows {rows}: max |y - fp64| = {err:.2e}")
        assert err <= GATE, (name, err)
        check_bf16_output(yb[m], v, 1e-5, f"out_proj + LN {name} bf16 copy")      # two LayerNorms in fp32 sit between the sums and the rounding


@pytest.mark.parametrize("rows", ROWS)
def test_heads_fusion_kernel_alone(rows):
    """iefvad_heads_{chain,pchain}_bf16_kernel: the four heads, Student-t precision weights, normalised inverse-variance fusion."""
    torch.set_num_threads(harness.host_cpu_share())
    model, W = handle(2, 1, 63)
    g = torch.Generator().manual_seed(rows)
    x = [(torch.randn(rows, D, generator=g)).to(torch.bfloat16) for _ in range(2)]
    f32 = dict(device="cuda", dtype=torch.float32)
    mu = [torch.empty(rows, D, **f32) for _ in range(2)]
    lv = [torch.empty(rows, D, **f32) for _ in range(2)]
    w = [torch.empty(rows, D, **f32) for _ in range(2)]
    z = torch.empty(rows, D, **f32)
    run(model, L.UNIT_HEADS, 0, rows, x=[t.cuda() for t in x], mu=mu, logvar=lv, w=w, z=z)
    r = {}
    for m, name in enumerate(("image", "event")):
        r[f"mu{m}"] = x[m].double() @ bf(W[f"temporal.{name}_mu.weight"]).t() + W[f"temporal.{name}_mu.bias"]
        r[f"lv{m}"] = x[m].double() @ bf(W[f"temporal.{name}_logvar.weight"]).t() + W[f"temporal.{name}_logvar.bias"]
    f = 9.0 / 8.0
    wi, we = f * torch.exp(-r["lv0"]), f * torch.exp(-r["lv1"])
    den = wi + we + 1e-8
    r["n0"], r["n1"] = wi / den, we / den
    r["z"] = r["n0"] * r["mu0"] + r["n1"] * r["mu1"]
    got = {"mu0": mu[0], "mu1": mu[1], "lv0": lv[0], "lv1": lv[1], "n0": w[0], "n1": w[1], "z": z}
    errs = {k: float((got[k].cpu().double() - r[k]).abs().max()) for k in got}
    print(f"heads + fusion rows {rows}: max |out - fp64| =", {k: f"{v:.1e}" for k, v in errs.items()})
    for k, e in errs.items():
        assert e <= GATE, (k, e)
    # only z asked for: the optional stores must not be what makes z right
    z2 = torch.empty(rows, D, **f32)
    run(model, L.UNIT_HEADS, 0, rows, x=[t.cuda() for t in x], z=z2)
    assert torch.equal(z, z2)


@pytest.mark.parametrize("rows", ROWS)
def test_refinement_chain_kernel_alone_one_step(rows):
    """iefvad_refine_chain_bf16_kernel with K = 1 from a given z_0: z_1 = z_0 - lambda (W2 bf16(relu(W1 bf16(z_0) + b1)) + b2), logit = z_1 w_c + b_c.
    ONE internal rounding site, the hidden activation h: elements of h within TOL_ACC of a bf16 boundary may round the other way,
    which moves z_1[r, n] by at most lambda ulp(h[r, j]) |W2[n, j]| -- summed over the boundary elements of the row, that is the
    per-element allowance on top of the fp32 gate (1e-5 .. 2e-4: an order below what a mis-mapped fragment costs); the MEAN error is held to
    2e-6, fp32-accumulation level, because flips are rare."""
    torch.set_num_threads(harness.host_cpu_share())
    model, W = handle(1, 1, 64)
    lam = 0.5
    g = torch.Generator().manual_seed(3 * rows)
    z0 = torch.randn(rows, D, generator=g) * 0.5
    z1 = torch.empty(rows, D, device="cuda")
    lg = torch.empty(rows, device="cuda")
    run(model, L.UNIT_REFINE, 0, rows, x=[z0.cuda(), None], z=z1, logits=lg)
    p = "temporal.refinement_blocks.0."
    W2 = bf(W[p + "2.weight"])
    h = torch.relu(bf(z0.double()) @ bf(W[p + "0.weight"]).t() + W[p + "0.bias"])
    fragile = (bf(h - TOL_ACC) != bf(h + TOL_ACC)).double()
    allow = lam * (fragile * bf_ulp(h)) @ W2.abs().t()                                       # [rows, 768]
    ref = z0.double() - lam * (bf(h) @ W2.t() + W[p + "2.bias"])
    wc = W["temporal.classifier.weight"].reshape(-1)
    ref_lg = ref @ wc + W["temporal.classifier.bias"]
    d = (z1.cpu().double() - ref).abs()
    dl = (lg.cpu().double() - ref_lg).abs()
    assert bool((d <= GATE + allow).all()), float((d - allow).max())
    assert bool((dl <= GATE + allow @ wc.abs()).all()), float((dl - allow @ wc.abs()).max())
    # flips are rare: the MEAN error stays at fp32-accumulation level whatever the allowances (a systematic error of 1e-3 would sit in it)
    print(f"refinement chain K=1 rows {rows}: max error {float(d.max()):.2e} (largest allowance {float(allow.max()):.2e}, median row allowance "
          f"{float(allow.max(dim=1).values.median()):.2e}); mean error {float(d.mean()):.2e}; {float(fragile.mean()):.2e} of h on a rounding boundary")
    assert float(d.mean()) <= 2e-6 and float(dl.mean()) <= 5e-6
    assert float(allow.max(dim=1).values.median()) <= 2e-4
    # in place (z aliases z_0), as the forward runs it: same bits
    zin = z0.cuda()
    run(model, L.UNIT_REFINE, 0, rows, x=[zin, None], z=zin, logits=lg)
    assert torch.equal(zin, z1)


# ---- attention alone ----------------------------------------------------------------------------------------------------------------
ATT_KINDS = ["flat", "std5", "std20", "dominant", "ties", "extreme"]      # chunk c of a modality is of kind (c + modality) % 6
ATT_DOMINANT = [0, 255, 127, 128, 15, 16, 143, 144]                         # first / last key, the lane-pair split of a softmax row, 16-key tile edges
U32 = 2.0 ** -24                                                            # unit roundoff of fp32


def attention_case(nchunks, mod, seed):
    """bf16 q (log2 units, as in_proj stores it), k, v [nchunks, 8, 256, 96], made here and not by in_proj, so the test controls the scores
    s = q k^T.  Per chunk kind, different per head (seeded per head; the dominant positions rotate with the head) so a head mix-up shows:
      flat / std5 / std20   q, k normal with std(s) = 0.3 / 5 / 20
      dominant              query i of head h: key ATT_DOMINANT[(i + h) % 8] leads by ~12 (P ~ 0.9, the other keys share the rest)
      ties                  queries 0..63: q = 0, every score equal, P = 1/256 exactly; the others: two identical key rows (j, j + 1 of the
                            dominant list) tied for the maximum
      extreme               coordinate 0 of every k is 1, of every q -120; coordinate 1 of k is 1 for key j only.  Queries 0..127: q[1] =
                            240, so key j sits near +120 and the rest near -120 (exp2 underflows to exact zeros, P_j = 1); queries 128..255:
                            q[1] = 0, every score near -120 (only the max subtraction brings them back).  Odd heads: 140 instead of 120 --
                            2^120 and 2^-120 are still fp32 numbers, 2^140 and 2^-140 are not, so without the max subtraction these
                            heads return NaN
    v is asymmetric in key and column with a positive mean per column (gain 2^(c % 5 - 2)): no symmetric fragment permutation cancels, and
    the output does not cancel to a value whose bf16 step is smaller than the effect of one probability's rounding."""
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros(nchunks, 8, 256, 96, dtype=torch.float64)
    k = torch.randn(nchunks, 8, 256, 96, generator=g, dtype=torch.float64)
    gain = torch.exp2((torch.arange(96) % 5 - 2).double())
    v = gain * (1.0 + 0.5 * torch.randn(nchunks, 8, 256, 96, generator=g, dtype=torch.float64))
    qi = torch.arange(256)
    for c in range(nchunks):
        kind = ATT_KINDS[(c + mod) % len(ATT_KINDS)]
        noise = torch.randn(8, 256, 96, generator=g, dtype=torch.float64)
        if kind in ("flat", "std5", "std20"):
            q[c] = noise * ({"flat": 0.3, "std5": 5.0, "std20": 20.0}[kind] / math.sqrt(96.0))
            continue
        for h in range(8):
            j = torch.tensor(ATT_DOMINANT)[(qi + h + c) % 8]                  # the leading key of each query
            if kind == "extreme":
                k[c, h, :, 0] = 1.0
                k[c, h, :, 1] = 0.0
                jj = ATT_DOMINANT[(h + c) % 8]
                k[c, h, jj, 1] = 1.0
                q[c, h] = noise[h] * 0.05
                big = 120.0 if h % 2 == 0 else 140.0
                q[c, h, :, 0] = -big
                q[c, h, :, 1] = torch.where(qi < 128, 2 * big, 0.0).double()
                continue
            if kind == "ties":
                for a in range(0, 8, 2):                                      # keys (0, 255), (127, 128), (15, 16), (143, 144) become identical rows
                    k[c, h, ATT_DOMINANT[a + 1]] = k[c, h, ATT_DOMINANT[a]]
            kb = bf(k[c, h])
            lead = kb[j]                                                      # [256, 96]
            q[c, h] = 0.1 * noise[h] + 12.0 * lead / (lead * lead).sum(-1, keepdim=True)
            if kind == "ties":
                q[c, h, :64] = 0.0
    return bf(q), bf(k), bf(v)


def attention_model(q, k, v):
    """fp64 softmax2(q k^T) v on the same bf16 q, k, v, the normalised probability rounded to bf16 where the kernels round it (csrc/
    attention_bf16.h, attention_pbf16.h: `(bf16)(p * inv)` -- AFTER the normalisation, the sum taken over the unrounded p), and the
    allowance per output element: the kernel's probability before its rounding is p (1 +- eps) with
        eps = ln 2 (12 u sum_d |q_d k_d| + u |s - max|)      the score: six fp32 MFMA accumulations of 16-product blocks, each block's own
                                                             sum counted as another six; the subtraction's rounding
            + 2 u + 130 u + 3 u                              v_exp_f32 (1 ulp), the row sum (128 sequential fp32 additions of positive
                                                             terms + the lane-pair exchange, worst case), 1 / sum and the product
    so its bf16 value lies between P_lo = bf16(p (1 - eps)) and P_hi = bf16(p (1 + eps)), as does the model's; P V accumulates exact
    products in fp32 over 16 MFMA steps (20 u sum |P v|).  tol = (P_hi - P_lo) |v| + 20 u P |v|: nothing in it comes from a kernel run."""
    s = q @ k.transpose(-1, -2)
    sm = s - s.amax(-1, keepdim=True)
    p = torch.exp2(sm)
    p = p / p.sum(-1, keepdim=True)
    eps = math.log(2.0) * (12 * U32 * (q.abs() @ k.abs().transpose(-1, -2)) + U32 * sm.abs()) + 135 * U32
    P, spread = bf(p), bf(p * (1 + eps)) - bf(p * (1 - eps))
    ref = P @ v
    tol = spread @ v.abs() + 20 * U32 * (P @ v.abs()) + 1e-30      # 1e-30: a probability below 2^-126 may be flushed to zero
    return ref, tol, P


def attention_rows(rows):
    return -(-rows // 256) * 256          # the file's ROWS rounded up to whole chunks: 2048 (8 chunks), 16640 (65 chunks)


@pytest.mark.parametrize("rows", [attention_rows(r) for r in ROWS])
def test_attention_kernel_alone(rows):
    """iefvad_attention_bf16_kernel (rows = 2048: 128 items, below two per compute unit) and iefvad_attention_pbf16_kernel (rows = 16640:
    1,040 items): softmax2(q k^T) v per chunk and head on q, k, v the test designs (attention_case), against the fp64 model with the
    probability rounded where the kernels round it (attention_model).  Besides the boundary check, finite everywhere and exact where the
    arithmetic is exact: a query with P = 1/256 returns the fp32-accumulated column mean, a query whose other keys underflow returns v[j]."""
    torch.set_num_threads(harness.host_cpu_share())
    model, _ = handle(1, 1, 66)
    nchunks = rows // 256
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    import os
    persistent = os.environ.get("IEFVAD_PERSIST", "1") != "0" and 2 * nchunks * 8 >= 2 * cus       # launch_attention_bf16's own rule
    assert persistent == (rows > 4096), (rows, cus)          # 2048 rows -> the one-block kernel, 16640 -> the persistent one, on any CDNA part
    data = [attention_case(nchunks, m, 1000 * rows + m) for m in range(2)]
    x = [torch.stack([t.permute(1, 0, 2, 3).reshape(8, rows, 96) for t in d]).to(torch.bfloat16).contiguous().cuda() for d in data]
    yb = [torch.full((rows, D), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    run(model, L.UNIT_ATTENTION, 0, rows, x=x, yb=yb)
    for m, (q, k, v) in enumerate(data):
        worst, ndiff = 0.0, 0
        got = yb[m].cpu().reshape(nchunks, 256, 8, 96).permute(0, 2, 1, 3)          # [chunk, head, query, 96]
        assert bool(torch.isfinite(got.float()).all()), m
        fracs = []
        for c0 in range(0, nchunks, 6):                                            # six chunks (one of each kind) at a time: memory
            sl = slice(c0, min(c0 + 6, nchunks))
            ref, tol, P = attention_model(q[sl], k[sl], v[sl])
            fracs.append((check_bf16_output(got[sl], ref, tol, f"attention modality {m} chunks {c0}.."), ref.numel()))
            differ = got[sl].double() != bf(ref)
            ndiff += int(differ.sum())
            worst = max(worst, float(((got[sl].double() - ref).abs() / (tol + bf_ulp(ref))).max()))
            for c in range(sl.start, sl.stop):
                kind = ATT_KINDS[(c + m) % len(ATT_KINDS)]
                if kind == "extreme":      # queries 0..127 of every head: P is one-hot, the output IS v[j]
                    for h in range(8):
                        jj = ATT_DOMINANT[(h + c) % 8]
                        assert torch.equal(got[c, h, :128].double(), v[c, h, jj].expand(128, 96)), (m, c, h)
                if kind == "ties":         # queries 0..63: P = 2^-8 exactly
                    assert bool((P[c - sl.start, :, :64] == 2.0 ** -8).all())
        frac = sum(f * n for f, n in fracs) / sum(n for _, n in fracs)
        print(f"attention rows {rows} modality {m} ({'persistent' if persistent else 'one-block'} kernel): {ndiff / got.numel():.2e} of the outputs differ from bf16(fp64 model), "
              f"max |y - model| / (allowance + one bf16 step) = {worst:.2f}, {frac:.2e} of the outputs on a bf16 rounding boundary")


def test_unit_entry_rejects_what_it_cannot_run():
    model, _ = handle(2, 0, 65)          # K = 0: no refinement chain on this handle
    lib = L.load_library()
    io = L.UnitIO()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.iefvad_rowblock_unit(model._handle, L.UNIT_REFINE, 0, 64, C.byref(io), st) != 0 and "K >= 1" in L.last_error()
    assert lib.iefvad_rowblock_unit(model._handle, L.UNIT_INPROJ, 0, 100, C.byref(io), st) != 0 and "multiple of 64" in L.last_error()
    assert lib.iefvad_rowblock_unit(model._handle, L.UNIT_INPROJ, 5, 64, C.byref(io), st) != 0 and "layer" in L.last_error()
    assert lib.iefvad_rowblock_unit(model._handle, L.UNIT_HEADS, 0, 64, C.byref(io), st) != 0
    assert lib.iefvad_rowblock_unit(model._handle, 9, 0, 64, C.byref(io), st) != 0 and "unknown stage" in L.last_error()
    assert lib.iefvad_rowblock_unit(model._handle, L.UNIT_ATTENTION, 0, 320, C.byref(io), st) != 0 and "multiple of 256" in L.last_error()
    assert lib.iefvad_rowblock_unit(model._handle, L.UNIT_ATTENTION, 0, 256, C.byref(io), st) != 0 and "ATTENTION needs" in L.last_error()
    buf = torch.zeros(3 * 8 * 256 * 96 + 8, dtype=torch.bfloat16, device="cuda")
    for m in range(2):
        io.x[m], io.yb[m] = buf.data_ptr() + 2, buf.data_ptr()                 # x not 16-byte aligned
    assert lib.iefvad_rowblock_unit(model._handle, L.UNIT_ATTENTION, 0, 256, C.byref(io), st) != 0 and "aligned" in L.last_error()
    io = L.UnitIO()
    a = argparse.Namespace(visual_layers=1, visual_head=8, num_refinement_steps=1, lambda_ref=0.5, noise_model="StudentT", nu=8)
    m32 = iefvad_amd.MMFMIL(14, D, 256, D, 8, 1, 8, 10, 10, "cuda", a).to("cuda:0").eval()
    with torch.cuda.device(0):
        m32._ensure_handle(torch.device("cuda:0"))
        m32._ensure_weights(torch.device("cuda:0"), torch.cuda.current_stream().cuda_stream)
    assert lib.iefvad_rowblock_unit(m32._handle, L.UNIT_HEADS, 0, 64, C.byref(io), st) != 0 and "BF16" in L.last_error()
