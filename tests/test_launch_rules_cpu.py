"""Kernel selection at its thresholds, without a GPU: tests/cabi/launch_rules.cpp (g++, -Wall -Werror) includes
ief-vad_amd/csrc/launch_rules.h -- the header libiefvad.so takes every kernel choice from -- and prints the plan for each query.

The expected values below are worked out by hand from the rules (rows = 256 B, D = K = 768, 256 CUs), not printed by the code:
  fp32      32x32 while (M/64)(N/64) nz < 320 (and K % 64 == 0); else 128x256 from (M/128)(N/256) nz >= 1536; else 64x64 while
            (M/128)(N/128) nz < 1024; else 128x128
  split     eligible from (M/128)(N/128) nz >= 72; the 128x256 tiling from (M/128)(N/256) nz >= 1536, bf16x6 and N % 256 == 0 only
  bf16 ring 256x256 from (M/256)(N/256) nz >= 256, never with the refine epilogue; 128x256 for M % 128 == N % 256 == 0; else 128x128 v1
  row-block in_proj and out_proj + LN from 2 (rows/64) >= 128, heads from 3 (rows/64) >= 128, the chain from rows/64 >= 4; rows % 64 == 0
  persist   out_proj + LN from rows/64 >= 2 (256/2), attention from 16 B >= 2 x 256, heads from rows/64 >= 2 (256/3 = 85)
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, BF16X6, FP16X3 = 0, 1, 2, 3                      # IEFVAD_COMPUTE_*
TILE = {"f32_tiny": (32, 32), "f32_small": (64, 64), "f32_128": (128, 128), "f32_t256": (128, 256),
        "bf16_v1": (128, 128), "bf16_pipe": (128, 256), "bf16_w256": (256, 256),
        "split_n128": (128, 128), "split_f16_n128": (128, 128), "split_n128x2": (128, 256)}


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("g++ / make not available")
    out = tmp_path_factory.mktemp("launch_rules")
    exe = os.path.join(str(out), "launch_rules")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cabi"), f"OUT={out}", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]

    def ask(queries):
        """answers to the queries, one per line; a `policy` line has no answer"""
        r = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        got = r.stdout.splitlines()
        assert len(got) == sum(not q.startswith("policy") for q in queries)
        return got
    return ask


def gemm(kernel, M, N):
    bm, bn = TILE[kernel]
    return f"{kernel} {(M // bm) * (N // bn)}"


def test_fp32_tilings_at_every_edge(ask):
    # (N, K, nz): the last B of 32x32, the last B of 64x64, the last B of 128x128; the 128x256 tiling from the next B on
    edges = {(768, 768, 1): (6, 85, 255), (2304, 768, 2): (1, 14, 42), (1536, 768, 2): (1, 21, 63), (512, 512, 1): (9, 127, 383)}
    q, want = [], []
    for (N, K, nz), (tiny, small, mid) in edges.items():
        for B, kernel in ((1, "f32_tiny"), (tiny, "f32_tiny"), (tiny + 1, "f32_small"), (small, "f32_small"), (small + 1, "f32_128"),
                          (mid, "f32_128"), (mid + 1, "f32_t256"), (1024, "f32_t256")):
            q.append(f"f32 {256 * B} {N} {K} {nz}")
            want.append(gemm(kernel, 256 * B, N))
    q += ["f32 64 768 768 1", "f32 256 768 48 1", "f32 256 832 768 1"]
    want += ["reject shape"] * 3
    # N % 256 != 0 never takes the 128x256 tiling; K % 64 != 0 never the 32x32 one
    q += ["f32 262144 896 768 1", "f32 256 768 96 1"]
    want += [gemm("f32_128", 262144, 896), gemm("f32_small", 256, 768)]
    assert ask(q) == want
    assert want[1] == "f32_tiny 1152" and want[2] == "f32_small 336"       # the grids, once by hand: 48 x 24 and 28 x 12


def test_split_tilings_and_the_forced_tile(ask):
    assert ask(["eligible 1280 768 768 1", "eligible 1536 768 768 1", "eligible 1536 768 32 1", "eligible 1536 832 768 1",
                "eligible 768 768 768 2"]) == ["0", "1", "0", "0", "1"]
    q, want = [], []
    for N, nz, B in ((768, 1, 256), (768, 2, 128), (1536, 2, 64), (2304, 2, 43)):           # the first B of the wide tiling
        q += [f"split {256 * (B - 1)} {N} 768 {nz} 0 0 0 0", f"split {256 * B} {N} 768 {nz} 0 0 0 0"]
        want += [gemm("split_n128", 256 * (B - 1), N), gemm("split_n128x2", 256 * B, N)]
    assert ask(q) == want
    assert want[:2] == ["split_n128 3060", "split_n128x2 1536"]
    M = 256 * 1024
    assert ask([f"split {M} 896 768 1 0 0 0 0",                   # N % 256 != 0 and fp16x3 have the narrow tiling only
                f"split {M} 768 768 1 1 0 0 0",
                "split 1536 768 768 1 0 256 0 0",                 # forced tiles, either way of the rule
                f"split {M} 768 768 1 0 128 0 0",
                f"split {M} 768 768 1 1 256 0 0",                 # a forced 256 is refused for fp16x3 and for N = 896
                f"split {M} 896 768 1 0 256 0 0",
                f"split {M} 768 768 1 0 64 0 0",
                "split 192 768 768 1 0 0 0 0", "split 256 768 32 1 0 0 0 0",
                "split 1536 768 768 1 0 0 1 1",                   # the dot-product epilogue: one bf16x6 problem with both operands
                "split 1536 768 768 1 0 0 1 0", "split 1536 768 768 2 0 0 1 1", "split 1536 768 768 1 1 0 1 1"]) == [
        gemm("split_n128", M, 896), gemm("split_f16_n128", M, 768), gemm("split_n128x2", 1536, 768), gemm("split_n128", M, 768),
        "reject no_wide_tiling", "reject no_wide_tiling", "reject tile_n", "reject shape", "reject shape",
        gemm("split_n128", 1536, 768), "reject dot_epilogue", "reject dot_epilogue", "reject dot_epilogue"]
    # IEFVAD_SPLIT_TILE=256 is a preference in launch_proj: N = 896 is forced to 128, fp16x3 goes by the rule (its narrow tiling)
    assert ask(["prefer 256 896 0", "prefer 256 768 1", "prefer 256 768 0", "prefer 128 768 0", "prefer 128 768 1", "prefer 0 768 0"]) == [
        "128", "0", "256", "128", "0", "0"]
    assert ask([f"split {M} 896 768 1 0 128 0 0", f"split {M} 768 768 1 1 0 0 0"]) == [gemm("split_n128", M, 896), gemm("split_f16_n128", M, 768)]


def test_bf16_ring_tilings(ask):
    q, want = [], []
    for N, nz, B in ((768, 1, 86), (2304, 2, 15)):                # the first B of the 256 x 256 tiling
        for refine in (0, 1):
            q += [f"bf16 {256 * (B - 1)} {N} 768 {nz} {refine}", f"bf16 {256 * B} {N} 768 {nz} {refine}"]
            want += [gemm("bf16_pipe", 256 * (B - 1), N), gemm("bf16_pipe" if refine else "bf16_w256", 256 * B, N)]
    # M = 128 is a whole 128 x 256 tile (never 256 x 256: M % 256 != 0, however many problems); N = 384 is not: the 128 x 128 v1 kernel
    q += ["bf16 128 768 768 1 0", "bf16 128 768 768 2 0", "bf16 65664 768 768 1 0", "bf16 256 384 768 1 0", "bf16 256 768 32 1 0",
          "bf16 64 768 768 1 0", "bf16 256 384 96 1 0"]
    want += [gemm("bf16_pipe", 128, 768), gemm("bf16_pipe", 128, 768), gemm("bf16_pipe", 65664, 768), gemm("bf16_v1", 256, 384),
             "reject shape", "reject shape", "reject shape"]
    assert ask(q) == want
    assert want[1] == "bf16_w256 258"


def flags(**on):
    return " ".join(f"{k}={int(v)}" for k, v in on.items())


def test_rowblock_flags_of_the_bf16_mode(ask):
    def passf(ip, ln):
        return flags(ip_chain=ip, need_xb0=not ip, splitmb=0, f16mb=0, ln_fused=ln)

    def tail(heads, chain):
        return flags(tail_split=0, heads_rows=heads, chain=chain, fold=0)
    assert ask([f"pass {BF16} {256 * 15}", f"pass {BF16} {256 * 16}", f"pass {BF16} 1000", f"pass {BF16} 262144", f"pass {F32} 262144",
                f"tail {BF16} {256 * 10} 10 0 0 1 1", f"tail {BF16} {256 * 11} 10 0 0 1 1",       # heads from B = 11
                f"tail {BF16} 192 1 0 0 1 1", f"tail {BF16} 256 1 0 0 1 1", f"tail {BF16} 262144 0 0 0 1 0",   # the chain from B = 1, K >= 1
                f"tail {BF16} 1000 10 0 0 1 1", f"tail {BF16} 262144 10 0 0 0 0", f"tail {F32} 262144 10 0 0 1 1"]) == [
        passf(0, 0), passf(1, 1), passf(0, 0), passf(1, 1), flags(ip_chain=0, need_xb0=0, splitmb=0, f16mb=0, ln_fused=0),
        tail(0, 1), tail(1, 1), tail(0, 0), tail(0, 1), tail(1, 0), tail(0, 0), tail(0, 0), tail(0, 0)]
    # each bit of IEFVAD_ROWBLOCK_OFF takes its stage off the row-block kernel, and only its stage
    for bit, (ip, ln, heads, chain) in {1: (0, 1, 1, 1), 2: (1, 0, 1, 1), 4: (1, 1, 0, 1), 8: (1, 1, 1, 0), 15: (0, 0, 0, 0)}.items():
        assert ask([f"policy {bit} 0 0 1 0 0", f"pass {BF16} 262144", f"tail {BF16} 262144 10 0 0 1 1"]) == [passf(ip, ln), tail(heads, chain)]
    # IEFVAD_ROWBLOCK_MIN_WGS / IEFVAD_CHAIN_MIN_BLOCKS move the thresholds; non-positive values keep 128 and 4
    assert ask(["policy 0 8 5 1 0 0", f"pass {BF16} 256", f"tail {BF16} 256 1 0 0 1 1", f"tail {BF16} 320 1 0 0 1 1",
                "policy 0 -3 -1 1 0 0", f"pass {BF16} {256 * 16}", f"tail {BF16} 256 1 0 0 1 1"]) == [
        passf(1, 1), tail(1, 0), tail(1, 1), passf(1, 1), tail(0, 1)]


def test_split_flags_of_a_pass_and_its_tail(ask):
    def passf(split, f16):
        return flags(ip_chain=0, need_xb0=0, splitmb=split, f16mb=f16, ln_fused=0)
    assert ask([f"pass {BF16X6} {256 * 5}", f"pass {BF16X6} {256 * 6}", f"pass {FP16X3} {256 * 5}", f"pass {FP16X3} {256 * 6}",
                f"pass {BF16X6} 1600", f"pass {BF16} {256 * 6}"]) == [
        passf(0, 0), passf(1, 0), passf(0, 0), passf(1, 1), passf(0, 0), flags(ip_chain=0, need_xb0=1, splitmb=0, f16mb=0, ln_fused=0)]

    def tail(split, fold):
        return flags(tail_split=split, heads_rows=0, chain=0, fold=fold)
    assert ask([f"tail {BF16X6} 1536 10 1 0 0 0",                 # an uncompacted split micro-batch
                f"tail {BF16X6} 1536 10 1 1 0 0",                 # a compacted set of 1,536 rows is still eligible ...
                f"tail {BF16X6} 1280 10 1 1 0 0",                 # ... below that it runs on the fp32 kernels
                f"tail {BF16X6} 1280 10 0 0 0 0",
                f"tail {BF16X6} 1536 0 1 0 0 0",                  # the folded scorer needs K >= 1 and the bf16x6 arithmetic
                f"tail {FP16X3} 1536 10 1 0 0 0"]) == [tail(1, 1), tail(1, 1), tail(0, 0), tail(0, 0), tail(1, 0), tail(1, 0)]


def test_persistent_kernels_from_two_blocks_per_cu(ask):
    q = ["outln 256 {} 1".format(256 * 63), "outln 256 {} 1".format(256 * 64), "outln 256 {} 0".format(256 * 64),
         "attn 256 31 0", "attn 256 32 0", "attn 256 31 1", "attn 256 32 1",
         "heads 256 {}".format(256 * 42), "heads 256 {}".format(256 * 43)]
    assert ask(q) == ["outln_chain 252 2 1", "outln_pchain 128 2 1", "outln_chain 256 2 1",
                      "attn_bf16 8 2 62", "attn_pbf16 256 1 1", "attn_bf16_rows 8 2 62", "attn_pbf16_rows 256 1 1",
                      "heads_chain 168 3 1", "heads_pchain 85 3 1"]
    # IEFVAD_PERSIST=0: the one-block kernels at any size
    assert ask(["policy 0 0 0 0 0 0"] + q) == ["outln_chain 252 2 1", "outln_chain 256 2 1", "outln_chain 256 2 1",
                                               "attn_bf16 8 2 62", "attn_bf16 8 2 64", "attn_bf16_rows 8 2 62", "attn_bf16_rows 8 2 64",
                                               "heads_chain 168 3 1", "heads_chain 172 3 1"]
    # the thresholds follow the device's CU count
    assert ask(["outln 64 4096 1", "outln 64 4032 1", "attn 64 8 0", "attn 64 7 0", "heads 64 2688", "heads 64 2624"]) == [
        "outln_pchain 32 2 1", "outln_chain 63 2 1", "attn_pbf16 64 1 1", "attn_bf16 8 2 14", "heads_pchain 21 3 1", "heads_chain 41 3 1"]
