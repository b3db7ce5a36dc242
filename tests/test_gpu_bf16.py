"""Throughput mode (bf16 operands / fp32 accumulation in the dense projections, everything else fp32 --
BASELINE config 3) against the golden vectors of the fp32 reference and, for AUC, against the CPU oracle.
Tolerances are the bf16-operand noise floor measured in SURVEY.md 8c: <= 1.1e-2 on the 768-d outputs,
<= 4.3e-3 on logits, <= 1.1e-3 on sigmoid(logit); gates sit ~3x above."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth
from oracle import iefvad_oracle as orc
from tests import helpers as H

pytestmark = pytest.mark.gpu

TOL_BIG_BF16 = 4e-2
TOL_LOGIT_BF16 = 1.5e-2
TOL_SIGMOID_BF16 = 4e-3


def make_model(L, K, lam, noise, nu, sd, **kw):
    args = argparse.Namespace(visual_layers=L, visual_head=8, num_refinement_steps=K, lambda_ref=lam,
                              noise_model=noise, nu=nu)
    m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, L, 8, 10, 10, "cuda", args, compute="bf16", **kw)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


def test_bf16_gemm_kernel_matches_fp64_of_rounded_operands():
    """The kernel must be exact up to fp32 accumulation once the operands are bf16: compare with an fp64 product
    of the SAME bf16-rounded operands (asymmetric data catches a transposed fragment or accumulator map)."""
    lib = iefvad_amd.lib.load_library()
    g = torch.Generator().manual_seed(0)
    for (M, N, K) in [(128, 128, 64), (256, 768, 768), (512, 2304, 768)]:
        A = torch.randn(M, K, generator=g).to(torch.bfloat16)
        W = torch.randn(N, K, generator=g).to(torch.bfloat16)
        b = torch.randn(N, generator=g)
        dA, dW, db = A.cuda(), W.cuda(), b.cuda()
        dC = torch.empty(M, N, device="cuda")
        rc = lib.iefvad_gemm_bias(dA.data_ptr(), dW.data_ptr(), db.data_ptr(), dC.data_ptr(), M, N, K, 1,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, iefvad_amd.lib.last_error()
        torch.cuda.synchronize()
        ref = A.double() @ W.double().t() + b.double()
        err = (dC.cpu().double() - ref).abs().max().item()
        assert err < 2e-4, (M, N, K, err)


@pytest.mark.parametrize("M,N", [(32768, 768), (16384, 2304)])
def test_bf16_w256_gemm_kernel_matches_fp64_and_the_pipe_kernel(M, N):
    """`iefvad_gemm_bf16_w256_kernel` (256 x 256 tiles, 8 waves) carries in_proj, out_proj and the heads of every full-size
    micro-batch; `iefvad_gemm_bias` selects it once (M / 256)(N / 256) >= 256.  Against an fp64 product of the same
    bf16-rounded operands on sampled rows, and BIT-IDENTICAL to the 128 x 256 pipe kernel (what a 512-row problem runs on:
    the "two bit-identical tilings" of plan_gemm_bf16, csrc/launch_rules.h) on the first and last 512 rows."""
    lib = iefvad_amd.lib.load_library()
    g = torch.Generator().manual_seed(5)
    K = 768
    A = torch.randn(M, K, generator=g).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    b = torch.randn(N, generator=g)
    dA, dW, db = A.cuda(), W.cuda(), b.cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def gemm(a_rows):
        out = torch.empty(a_rows.shape[0], N, device="cuda")
        rc = lib.iefvad_gemm_bias(a_rows.data_ptr(), dW.data_ptr(), db.data_ptr(), out.data_ptr(), a_rows.shape[0], N, K, 1, st)
        assert rc == 0, iefvad_amd.lib.last_error()
        return out

    big = gemm(dA)
    torch.cuda.synchronize()
    rows = torch.cat([torch.arange(0, 300), torch.arange(M // 2 - 130, M // 2 + 130), torch.arange(M - 300, M)])
    ref = A[rows].double() @ W.double().t() + b.double()
    err = (big[rows.cuda()].cpu().double() - ref).abs().max().item()
    assert err < 2e-4, err
    for lo in (0, M - 512):
        small = gemm(dA[lo:lo + 512].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(small, big[lo:lo + 512]), lo


BF16_REGIMES = ("flat", "sharp")      # not "over": the mode's own rounding noise there (fixture field bf16_floor_big) is the size of the gate


@pytest.mark.parametrize("name", H.golden_cases(regimes=BF16_REGIMES) + H.golden_cases(big=True, regimes=BF16_REGIMES))
def test_bf16_forward_within_bf16_noise_of_reference(name):
    """The sharp cases (peaked attention) keep these gates as long as the mode's own rounding noise fits under them with the usual
    3x margin: the fixtures record the distance of the mode's fp64 emulation (bf16_mode_emulation, computed on the CPU by the
    generator) and H.case_gates raises a gate to 3x that distance where it is larger (sharp_k3_student8: 768-d 1.53e-2 -> 4.6e-2)."""
    g, cfg, sd, img, ev = H.load_case(name)
    model = make_model(cfg["L"], cfg["K"], cfg["lam"], cfg["noise"], cfg["nu"], sd)
    with torch.no_grad():
        out = model(torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda(), None, None, None)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    gates = H.case_gates(g, (TOL_BIG_BF16, TOL_LOGIT_BF16, TOL_SIGMOID_BF16), ("bf16_floor_big", "bf16_floor_logit", "bf16_floor_sigmoid"))
    errs = H.compare_outputs(out, g, *gates)
    print(name, errs, "gates", gates)


def test_bf16_scores_mode_and_microbatch_bit_identical():
    sd = synth.make_state_dict(31, 768, 2, 3)
    img, ev = synth.make_inputs(32, 5)
    ti, te = torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()
    with torch.no_grad():
        a = make_model(2, 3, 0.5, "StudentT", 8, sd)(ti, te, None, None, None)
        b = make_model(2, 3, 0.5, "StudentT", 8, sd, micro_batch=2, outputs="scores")(ti, te, None, None, None)
    assert torch.equal(a["logits"], b["logits"])
    assert (b["w_i_mean"] - a["w_i"].mean(-1)).abs().max().item() < 1e-6


@pytest.mark.parametrize("outputs,overflow,L", [("full", False, 2), ("scores", False, 2), ("full", True, 2), ("full", False, 3)])
def test_fused_heads_kernel_equals_heads_projection_plus_fusion_kernel(monkeypatch, outputs, overflow, L):
    """bf16 mode runs the heads of both modalities and the fusion as ONE kernel once a micro-batch fills the chip
    (csrc/heads_chain_bf16.h from 11 chunks on), and out_proj + residual + LayerNorm(s) as one row-owning kernel (from 16 chunks:
    csrc/outproj_ln_chain_bf16.h, 64-row blocks on the refinement chain's structure).  Same k order, same LayerNorm / fusion
    code: every output must equal the unfused path bit for bit (IEFVAD_ROWBLOCK_OFF=6 at model creation: GEMM + LayerNorm kernel,
    GEMM + fusion kernel), the row means of the
    weights to fp32 rounding (their partial sums are combined in another order).  `overflow`: a log-variance column that
    overflows the literal formula (inf / inf = NaN, imf_vad.py:135-142), without refinement steps so that the NaN stays in
    its column.  L = 3: the middle layer's fused kernel reads its residual rows from the buffer it writes its output rows
    to (in place, row by row)."""
    K = 0 if overflow else 3
    sd = synth.make_state_dict(7, 768, L, K)
    if overflow:
        sd["temporal.image_logvar.bias"] = sd["temporal.image_logvar.bias"].clone()
        sd["temporal.image_logvar.bias"][5] = -95.0
        sd["temporal.event_logvar.bias"] = sd["temporal.event_logvar.bias"].clone()
        sd["temporal.event_logvar.bias"][5] = -95.0
    img, ev = synth.make_inputs(33, 64)
    ti, te = torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()
    with torch.no_grad():
        fused = make_model(L, K, 0.5, "StudentT", 8, sd, outputs=outputs)(ti, te, None, None, None)
        monkeypatch.setenv("IEFVAD_ROWBLOCK_OFF", "6")
        plain = make_model(L, K, 0.5, "StudentT", 8, sd, outputs=outputs)(ti, te, None, None, None)
    assert set(fused) == set(plain)
    for k in fused:
        a, b = fused[k].float(), plain[k].float()
        assert torch.equal(torch.isnan(a), torch.isnan(b)), k
        if k in ("w_i_mean", "w_e_mean"):
            assert torch.allclose(a, b, rtol=0, atol=1e-6, equal_nan=True), k
        else:
            assert torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)), k
    if overflow:
        assert torch.isnan(fused["fused"][..., 5]).all() and torch.isfinite(fused["fused"][..., :5]).all()


@pytest.mark.parametrize("K,lam,outputs,B", [(1, 0.5, "full", 64), (3, 0.3, "full", 64), (10, 0.5, "scores", 64),
                                             (5, 0.5, "scores", 192), (10, 0.5, "full", 128)])
def test_refinement_chain_kernel_equals_the_2k_launch_path(monkeypatch, K, lam, outputs, B):
    """bf16 mode runs the K refinement steps AND the scorer (imf_vad.py:146-150) as ONE kernel with the state on chip once a
    micro-batch is a whole chunk or more (csrc/refine_chain_bf16.h; the tests below use full grids): fp32 z in registers, one aliased bf16 z / h image in
    LDS, per-wave LDS-DMA weight streams.  Same products in the same k order, same epilogue arithmetic, the scorer kernel's
    own reduction: `fused` and `logits` must equal the 2K-launch path bit for bit (IEFVAD_ROWBLOCK_OFF=8 at model creation).
    B = 192 with micro_batch = 128 exercises a second, smaller pass (64 chunks) through the same handle."""
    sd = synth.make_state_dict(11, 768, 2, K)
    img, ev = synth.make_inputs(34, B)
    ti, te = torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()
    kw = dict(outputs=outputs, micro_batch=128)
    with torch.no_grad():
        chain = make_model(2, K, lam, "StudentT", 8, sd, **kw)(ti, te, None, None, None)
        monkeypatch.setenv("IEFVAD_ROWBLOCK_OFF", "8")
        plain = make_model(2, K, lam, "StudentT", 8, sd, **kw)(ti, te, None, None, None)
    assert set(chain) == set(plain)
    assert torch.isfinite(plain["logits"]).all()
    for k in chain:
        assert torch.equal(chain[k], plain[k]), (k, (chain[k].float() - plain[k].float()).abs().max().item())


@pytest.mark.parametrize("outputs,overflow,B", [("full", False, 64), ("scores", False, 40), ("full", True, 64)])
def test_heads_row_block_kernel_equals_the_ring_kernel(monkeypatch, outputs, overflow, B):
    """bf16 mode, >= 11 chunks (128 workgroups): heads + fusion run on the row-block kernel (csrc/heads_chain_bf16.h): 64 rows resident as an
    LDS image (x_i, then x_e), a wave streams the four head matrices of its 32 columns and fuses in registers.  Same products
    in the same k order and the same fusion code as the ring GEMM + the fusion kernel (IEFVAD_ROWBLOCK_OFF=4 at model creation:
    only this stage off its row-block kernel): every output bit for bit, the row means of the weights to fp32 rounding.
    `overflow`: the literal formula's inf / inf = NaN column (imf_vad.py:135-142) must come out the same."""
    K = 0 if overflow else 3
    sd = synth.make_state_dict(14, 768, 2, K)
    if overflow:
        for k in ("temporal.image_logvar.bias", "temporal.event_logvar.bias"):
            sd[k] = sd[k].clone()
            sd[k][5] = -95.0
    img, ev = synth.make_inputs(37, B)
    ti, te = torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()
    with torch.no_grad():
        rows = make_model(2, K, 0.5, "StudentT", 8, sd, outputs=outputs)(ti, te, None, None, None)
        monkeypatch.setenv("IEFVAD_ROWBLOCK_OFF", "4")
        ring = make_model(2, K, 0.5, "StudentT", 8, sd, outputs=outputs)(ti, te, None, None, None)
    assert set(rows) == set(ring)
    for k in rows:
        a, b = rows[k].float(), ring[k].float()
        assert torch.equal(torch.isnan(a), torch.isnan(b)), k
        if k in ("w_i_mean", "w_e_mean"):
            assert torch.allclose(a, b, rtol=0, atol=1e-6, equal_nan=True), k
        else:
            assert torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)), (k, (a - b).abs().max().item())
    if overflow:
        assert torch.isnan(rows["fused"][..., 5]).all() and torch.isfinite(rows["fused"][..., :5]).all()


@pytest.mark.parametrize("L,in_dtype,B", [(2, np.float32, 64), (3, np.float16, 64), (2, np.float32, 96)])
def test_inproj_row_block_kernel_equals_the_ring_kernel(monkeypatch, L, in_dtype, B):
    """bf16 mode, >= 16 chunks (128 workgroups): in_proj runs on the row-block kernel (csrc/inproj_chain_bf16.h): a workgroup keeps 64 rows as
    one LDS image, every wave streams its own 96 columns of q, k and v; the first layer reads the fp32 rows and rounds them to
    bf16 itself (no cast kernel, no bf16 copy of the inputs).  Same products in the same k order, the ring kernel's epilogue:
    every output must equal the ring-kernel path (IEFVAD_ROWBLOCK_OFF=1 at model creation) bit for bit.  NaN / inf rows
    included; fp16 inputs take the widening cast first; B = 96 with micro_batch = 64 runs a second, smaller pass (32 chunks)
    through the same handle."""
    sd = synth.make_state_dict(13, 768, L, 3)
    img, ev = synth.make_inputs(36, B)
    img[2, 100, 9] = np.nan
    ev[5, 0, 0] = np.inf
    ti, te = torch.from_numpy(img.astype(in_dtype)).cuda(), torch.from_numpy(ev.astype(in_dtype)).cuda()
    kw = dict(outputs="full", micro_batch=64)
    with torch.no_grad():
        rowblock = make_model(L, 3, 0.5, "StudentT", 8, sd, **kw)(ti, te, None, None, None)
        monkeypatch.setenv("IEFVAD_ROWBLOCK_OFF", "1")
        ring = make_model(L, 3, 0.5, "StudentT", 8, sd, **kw)(ti, te, None, None, None)
    assert set(rowblock) == set(ring)
    for k in rowblock:
        a, b = rowblock[k].float(), ring[k].float()
        assert torch.equal(torch.isnan(a), torch.isnan(b)), k
        assert torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)), (k, (a - b).abs().max().item())
    bad = (~torch.isfinite(rowblock["logits"])).reshape(B, 256).any(dim=1).cpu().numpy()
    assert bad[2] and bad[5] and bad.sum() == 2


@pytest.mark.parametrize("B", [1, 3, 12, 20])
def test_row_block_kernels_on_partially_filled_grids_equal_the_ring_kernels(monkeypatch, B):
    """The row-block kernels take a projection from 128 workgroups on and the refinement chain from one chunk (4 blocks): B = 1, 3
    run the chain beside ring-kernel projections, B = 12 adds the heads kernel, B = 20 all of them, on grids that fill a
    fraction of the chip.  Against the same model with both thresholds out of reach (IEFVAD_ROWBLOCK_MIN_WGS,
    IEFVAD_CHAIN_MIN_BLOCKS at model creation: ring kernels, 2K launches): every output bit for bit, the row means of the
    fusion weights to fp32 rounding."""
    sd = synth.make_state_dict(15, 768, 2, 4)
    img, ev = synth.make_inputs(38, B)
    ti, te = torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()
    kw = dict(outputs="full", graph_chunks=-1)
    with torch.no_grad():
        new = make_model(2, 4, 0.5, "StudentT", 8, sd, **kw)(ti, te, None, None, None)
        monkeypatch.setenv("IEFVAD_ROWBLOCK_MIN_WGS", "1000000")
        monkeypatch.setenv("IEFVAD_CHAIN_MIN_BLOCKS", "1000000")
        old = make_model(2, 4, 0.5, "StudentT", 8, sd, **kw)(ti, te, None, None, None)
    assert set(new) == set(old)
    for k in new:
        a, b = new[k].float(), old[k].float()
        if k in ("w_i_mean", "w_e_mean"):
            assert torch.allclose(a, b, rtol=0, atol=1e-6), k
        else:
            assert torch.equal(a, b), (k, (a - b).abs().max().item())


def test_refinement_chain_kernel_propagates_non_finite_rows(monkeypatch):
    """A NaN / inf in one snippet's fused state must stay in that row through the chain kernel exactly as through the
    projection launches (rows are independent in imf_vad.py:146-150)."""
    sd = synth.make_state_dict(12, 768, 2, 4)
    img, ev = synth.make_inputs(35, 64)
    img[3, 17, 5] = np.nan          # poisons chunk 3 through the unmasked attention
    ev[9, 200, 700] = np.inf
    ti, te = torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()
    with torch.no_grad():
        chain = make_model(2, 4, 0.5, "StudentT", 8, sd)(ti, te, None, None, None)
        monkeypatch.setenv("IEFVAD_ROWBLOCK_OFF", "8")
        plain = make_model(2, 4, 0.5, "StudentT", 8, sd)(ti, te, None, None, None)
    for k in ("logits", "fused"):
        a, b = chain[k].float(), plain[k].float()
        assert torch.equal(torch.isnan(a), torch.isnan(b)), k
        assert torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)), k
    bad = (~torch.isfinite(chain["logits"])).reshape(64, 256).any(dim=1).cpu().numpy()
    assert bad[3] and bad[9] and bad.sum() == 2


def test_xd_shaped_set_auc_and_ap_parity_bf16():
    """BASELINE config 3: XD-Violence-sized synthetic set (753 videos, ~145 k snippets), bf16 projections,
    AUC and AP (XD selects by AP, xd_train.py:114) equal to 4 d.p. against the fp32 CPU oracle."""
    seed = 2
    lengths = synth.lognormal_lengths(seed, 753, 145000)
    keys = harness.CLASS_KEYS['xd']
    classes = [keys[i % len(keys)] for i in range(753)]
    total = int(lengths.sum())
    gt = synth.make_gt(seed, total)
    sd = synth.make_state_dict(17)

    def items():
        for i, (n, c) in enumerate(zip(lengths, classes)):
            img, ev = synth.make_video(seed, i, int(n))
            ci, _ = harness.process_split(img, 256)
            ce, _ = harness.process_split(ev, 256)
            yield torch.tensor(ci).unsqueeze(0), torch.tensor(ce).unsqueeze(0), (c,), torch.tensor([int(n)])

    model = make_model(2, 10, 0.5, "StudentT", 8, sd, outputs="scores")
    s_gpu, _, _, _ = harness.score_loader(model, items(), 256, "cuda:0", "xd", batch_chunks=512)
    torch.set_num_threads(16)
    oracle = orc.OracleMMFMIL(sd, orc.OracleConfig())
    s_cpu, _, _, _ = harness.score_loader(oracle, items(), 256, "cpu", "xd", batch_chunks=8)
    a, b = np.concatenate(s_gpu), np.concatenate(s_cpu)
    assert a.shape == b.shape == (total,)
    dmax = float(np.abs(a - b).max())
    assert dmax <= TOL_SIGMOID_BF16, dmax
    r_gpu = harness.evaluate_scores(s_gpu, classes, gt, "xd", verbose=False, normal_keys=('normal',))
    r_cpu = harness.evaluate_scores(s_cpu, classes, gt, "xd", verbose=False, normal_keys=('normal',))
    for k in ("roc", "ap", "ano_auc"):
        assert abs(r_gpu[k] - r_cpu[k]) < 1e-4, (k, r_gpu[k], r_cpu[k])
    print("config-3 shape: snippets", total, "max|dscore|", dmax, "AUC", r_gpu["roc"], r_cpu["roc"], "AP", r_gpu["ap"], r_cpu["ap"])


def test_config5_k5_shang_msad_real_gt_bf16(golden_dir):
    """BASELINE config 5: K=5 refinement steps, the ShanghaiTech + MSAD test lists (197 + 241 videos, 8,723 + 9,009 =
    17,732 snippets) with the reference's REAL frame-level ground truth and label order (tests/golden/config5_gt.npz =
    /root/reference/list/{shang,msad}/rgb/vitl/{gt.npy,test.csv}; features and hence video lengths are synthetic, summing
    to each gt exactly), bf16 projections; per-dataset and combined AUC / AP vs the fp32 oracle."""
    lists = synth.config5_lists(golden_dir)
    assert sum(int(v[0].sum()) for v in lists.values()) == 17732
    sd = synth.make_state_dict(19, 768, 2, 5)
    model = make_model(2, 5, 0.5, "StudentT", 8, sd, outputs="scores")
    torch.set_num_threads(harness.host_cpu_share())
    oracle = orc.OracleMMFMIL(sd, orc.OracleConfig(num_refinement_steps=5))
    all_gpu, all_cpu, all_gt = [], [], []
    for seed, d in ((51, "shang"), (52, "msad")):
        lengths, classes, gt = lists[d]

        def items():
            for i, (n, c) in enumerate(zip(lengths, classes)):
                img, ev = synth.make_video(seed, i, int(n))
                ci, _ = harness.process_split(img, 256)
                ce, _ = harness.process_split(ev, 256)
                yield torch.tensor(ci).unsqueeze(0), torch.tensor(ce).unsqueeze(0), (c,), torch.tensor([int(n)])

        s_gpu, c_gpu, _, _ = harness.score_loader(model, items(), 256, "cuda:0", d, batch_chunks=128)
        s_cpu, _, _, _ = harness.score_loader(oracle, items(), 256, "cpu", d, batch_chunks=8)
        assert c_gpu == classes
        a, b = np.concatenate(s_gpu), np.concatenate(s_cpu)
        assert a.shape == b.shape == (len(gt) // 16,)
        assert float(np.abs(a - b).max()) <= TOL_SIGMOID_BF16
        nk = ('normal',) if d == "shang" else ('Normal',)
        r_gpu = harness.evaluate_scores(s_gpu, classes, gt, d, verbose=False, normal_keys=nk)
        r_cpu = harness.evaluate_scores(s_cpu, classes, gt, d, verbose=False, normal_keys=nk)
        for k in ("roc", "ap", "ano_auc"):
            assert abs(r_gpu[k] - r_cpu[k]) < 1e-4, (d, k, r_gpu[k], r_cpu[k])
        all_gpu.append(a); all_cpu.append(b); all_gt.append(gt)
    from sklearn.metrics import average_precision_score, roc_auc_score
    g = np.concatenate(all_gt)
    for f in (roc_auc_score, average_precision_score):
        assert abs(f(g, np.repeat(np.concatenate(all_gpu), 16)) - f(g, np.repeat(np.concatenate(all_cpu), 16))) < 1e-4


# ----------------------------------------------------------------------------------------------------------------------------------
# oracle-side checks of the row-block kernels: an fp64 evaluation of the SAME bf16-rounded operands
# ----------------------------------------------------------------------------------------------------------------------------------
def _r(x):
    """round to bf16 (nearest even) where a kernel rounds an MFMA operand or a stored activation; fp64 in, fp64 out"""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _ln(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    xc = x - mu
    return xc / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps) * g + b


def bf16_mode_emulation(sd, img, ev, L, K, lam, nu, stop_at_fusion=False):
    """The bf16 mode's data flow restated in fp64 with a bf16 rounding exactly where the kernels round: projection operands
    (inputs, LayerNorm outputs, attention outputs, the refinement state and hidden activation), q | k | v as stored (q pre-scaled by
    log2(e)/sqrt(96), softmax in base 2), the normalised probabilities before P V, every weight matrix; biases, LayerNorm, the
    residual stream, fusion, the refinement state and the scorer stay unrounded.  Products of bf16 values are exact in fp32, so
    what is left between this and the kernels is fp32 accumulation order -- and the rare operand whose fp32 value sits on a bf16
    rounding boundary."""
    W = {k: v.double() for k, v in sd.items()}
    Wb = {k: _r(v.double()) for k, v in sd.items() if v.dim() == 2 and v.shape[0] > 1}
    B = img.shape[0]
    enc = {}
    for m, x0 in (("image", img), ("event", ev)):
        x = x0.double()                       # fp32 residual stream
        a = _r(x)                             # the projection's bf16 operand
        for l in range(L):
            p = f"temporal.{m}_attn_layers.{l}."
            qkv = a @ Wb[p + "in_proj_weight"].t() + W[p + "in_proj_bias"]
            q, k, v = qkv.split(768, dim=-1)
            q = _r(q * (1.4426950408889634 / math.sqrt(96.0)))
            k, v = _r(k), _r(v)
            hd = lambda t: t.reshape(B, 256, 8, 96).transpose(1, 2)
            s = hd(q) @ hd(k).transpose(-1, -2)
            pr = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
            pr = _r(pr / pr.sum(dim=-1, keepdim=True))
            att = _r((pr @ hd(v)).transpose(1, 2).reshape(B, 256, 768))
            y = att @ Wb[p + "out_proj.weight"].t() + W[p + "out_proj.bias"] + x
            x = _ln(y, W[f"temporal.{m}_norms.{l}.weight"], W[f"temporal.{m}_norms.{l}.bias"])
            if l == L - 1:
                x = _ln(x, W[f"temporal.whiten_{m}.weight"], W[f"temporal.whiten_{m}.bias"])
            a = _r(x)
        enc[m] = a
    out = {}
    for m in ("image", "event"):
        out[f"{m}_mu"] = enc[m] @ Wb[f"temporal.{m}_mu.weight"].t() + W[f"temporal.{m}_mu.bias"]
        out[f"{m}_logvar"] = enc[m] @ Wb[f"temporal.{m}_logvar.weight"].t() + W[f"temporal.{m}_logvar.bias"]
    f = (nu + 1) / nu
    wi, we = f * torch.exp(-out["image_logvar"]), f * torch.exp(-out["event_logvar"])
    den = wi + we + 1e-8
    out["w_i"], out["w_e"] = wi / den, we / den
    z = out["w_i"] * out["image_mu"] + out["w_e"] * out["event_mu"]
    out["z0"] = z
    if not stop_at_fusion:
        out["fused"], out["logits"] = refinement_emulation(sd, z, K, lam)
    return out


def refinement_emulation(sd, z, K, lam):
    W = {k: v.double() for k, v in sd.items()}
    z = z.double()
    for k in range(K):
        p = f"temporal.refinement_blocks.{k}."
        h = _r(torch.relu(_r(z) @ _r(W[p + "0.weight"]).t() + W[p + "0.bias"]))
        z = z - lam * (h @ _r(W[p + "2.weight"]).t() + W[p + "2.bias"])
    return z, z @ W["temporal.classifier.weight"].t() + W["temporal.classifier.bias"]


import math  # noqa: E402


def test_refinement_chain_kernel_against_fp64_of_the_same_rounded_operands():
    """`iefvad_refine_chain_bf16_kernel` on its own: its input z_0 is recomputed EXACTLY from the forward's outputs (z_0 = n_i mu_i +
    n_e mu_e in the fusion kernel's fp32 operations), the K = 10 steps and the scorer are evaluated in fp64 on the same bf16-rounded
    operands.  Error = fp32 accumulation plus the occasional activation on a bf16 rounding boundary (one bf16 ulp of one operand
    element): an order below the bf16-vs-fp32 gate (4e-2) on the maximum, three orders on the mean."""
    K, lam = 10, 0.5
    sd = synth.make_state_dict(19, 768, 2, K)
    img, ev = synth.make_inputs(39, 16)
    with torch.no_grad():
        out = make_model(2, K, lam, "StudentT", 8, sd)(torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda(), None, None, None)
        z0 = out["w_i"] * out["image_mu"] + out["w_e"] * out["event_mu"]              # fmul, fmul, fadd: fuse_elem's own operations
    fused, logits = refinement_emulation(sd, z0.cpu(), K, lam)
    d_f, d_l = (out["fused"].cpu().double() - fused).abs(), (out["logits"].cpu().double() - logits).abs()
    e_f, e_l, m_f, m_l = float(d_f.max()), float(d_l.max()), float(d_f.mean()), float(d_l.mean())
    print("chain vs fp64 of rounded operands (max, mean):", e_f, e_l, m_f, m_l)
    # observed on MI355X: max 1.6e-3 / 5e-4 (flips compound over 20 projections), mean 2-4e-5; the bf16-vs-fp32 gate is 4e-2 / 1.5e-2
    assert e_f <= 5e-3 and e_l <= 2e-3 and m_f <= 1e-4 and m_l <= 1e-4, (e_f, e_l, m_f, m_l)


def test_row_block_encoder_and_heads_against_fp64_of_the_same_rounded_operands():
    """in_proj, attention, out_proj + LayerNorm and heads + fusion at a batch size where every one of them runs on its row-block
    kernel (B = 16: 128 workgroups), against the fp64 evaluation of the bf16 mode's own data flow (bf16_mode_emulation).  A rounding
    flip early in the encoder travels through two attention layers (and makes further flips likelier), so what is gated is "a few
    bf16 ulps of single operand elements": 7x below the bf16-vs-fp32 gate on the maximum, 60x on the mean."""
    L, K, lam, nu = 2, 2, 0.5, 8
    sd = synth.make_state_dict(20, 768, L, K)
    img, ev = synth.make_inputs(40, 16)
    with torch.no_grad():
        out = make_model(L, K, lam, "StudentT", nu, sd)(torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda(), None, None, None)
    torch.set_num_threads(harness.host_cpu_share())
    ref = bf16_mode_emulation(sd, torch.from_numpy(img), torch.from_numpy(ev), L, K, lam, nu)
    worst = {}
    for k in ("image_mu", "event_mu", "image_logvar", "event_logvar", "w_i", "w_e", "fused", "logits"):
        d = (out[k].cpu().double() - ref[k].reshape(out[k].shape)).abs()
        worst[k] = (float(d.max()), float(d.mean()))
    print("row-block kernels vs fp64 of rounded operands (max, mean):", worst)
    # observed on MI355X: max <= 1.9e-3, mean 0.5-1.9e-4 -- one bf16 ulp of one operand element is 1.4e-4 on every output of its row,
    # and such flips cascade through the two attention layers; the bf16-vs-fp32 gates are 4e-2 (768-d) and 1.5e-2 (logits)
    for k, (mx, mean) in worst.items():
        assert mx <= 6e-3 and mean <= 6e-4, (k, mx, mean)


def test_persistent_kernels_equal_the_one_block_kernels(tmp_path):
    _persistent_equals_one_block(tmp_path, None)


def test_persistent_kernels_equal_the_one_block_kernels_with_peaked_attention(tmp_path):
    """The same with the q / k rows sharpened (synth.sharpen_qk (8, 4)): both sides share the flat regime otherwise, where a
    wrong key order or a wrong running maximum in one of the two attention kernels moves nothing."""
    _persistent_equals_one_block(tmp_path, (8, 4))


def _persistent_equals_one_block(tmp_path, factors):
    """The three persistent kernels of the bf16 mode (out_proj + LayerNorm, heads + fusion, attention: one workgroup per CU walking
    blocks / items, the next image by LDS-DMA) against the kernels they replace from two blocks per CU on -- IEFVAD_PERSIST=0, read
    when the library handle is created; one child process per value.  B = 96 chunks (384 row blocks, 1,536 attention items: every persistent kernel
    runs), dense and as a list of videos (the row-compressed attention variant): every output bit for bit, the row means of the
    fusion weights to fp32 rounding (their summation order belongs to the kernel)."""
    import os
    import subprocess
    import sys
    script = (
        "import argparse, sys, numpy as np, torch\n"
        "sys.path.insert(0, %r)\n"
        "import iefvad_amd\n"
        "from iefvad_amd import synth\n"
        "sd = synth.make_state_dict(14, 768, 2, 3)\n"
        "factors = %r\n"
        "sd = synth.sharpen_qk(sd, factors) if factors else sd\n"
        "a = argparse.Namespace(visual_layers=2, visual_head=8, num_refinement_steps=3, lambda_ref=0.5, noise_model='StudentT', nu=8)\n"
        "m = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 2, 8, 10, 10, 'cuda', a, compute='bf16')\n"
        "m.load_state_dict(sd); m = m.to('cuda:0').eval()\n"
        "img, ev = synth.make_inputs(37, 96)\n"
        "ti, te = torch.from_numpy(img).cuda(), torch.from_numpy(ev).cuda()\n"
        "with torch.no_grad():\n"
        "    out = m(ti, te, None, None, None)\n"
        "    lens = [200 + (37 * i) %% 56 for i in range(96)]\n"
        "    rows_i = torch.cat([ti[i, :n] for i, n in enumerate(lens)]); rows_e = torch.cat([te[i, :n] for i, n in enumerate(lens)])\n"
        "    vid = m.forward_videos(rows_i, rows_e, lens)\n"
        "np.savez(sys.argv[1], **{k: v.float().cpu().numpy() for k, v in out.items()}, **{'vid_' + k: v.cpu().numpy() for k, v in vid.items()})\n"
    ) % (os.path.dirname(H.GOLDEN.rstrip('/').rsplit('/', 1)[0]), factors)
    res = {}
    for flag in ("1", "0"):
        env = dict(os.environ, IEFVAD_PERSIST=flag)
        path = str(tmp_path / f"persist{flag}.npz")
        r = subprocess.run([sys.executable, "-c", script, path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res[flag] = np.load(path)
    assert set(res["1"].files) == set(res["0"].files) and "vid_logits" in res["1"].files
    for k in res["1"].files:
        a, b = res["1"][k], res["0"][k]
        if k.endswith("w_i_mean") or k.endswith("w_e_mean"):
            assert np.allclose(a, b, rtol=0, atol=1e-6), k
        else:
            assert np.array_equal(a, b), (k, float(np.abs(a - b).max()))
