"""The batch-invariant part of kernel selection, without a GPU: tests/cabi/launch_rules_invariant.cpp (g++ -std=c++17 -Wall -Werror,
compiled here) includes ief-vad_amd/csrc/launch_rules.h -- the header libiefvad.so takes every kernel choice from -- and answers one
query per line.

The expected values are worked out by hand from the rules (rows = 256 B, D = K = 768):
  default      bf16x6 / fp16x3 passes are split from (rows/128)(768/128) >= 72, i.e. rows >= 1536; a compacted tail below that is not
  split_always a bf16x6 pass is split at every row count, its tail too, compacted or not, so fold = (K >= 1); f32, bf16 and fp16x3
               answer as in the default policy
  small plan   grid (M/32)(N/128) for M % 32 == N % 128 == K % 64 == 0, K >= 64, nz in {1, 2}; the dot epilogue takes one problem
               with both operands; in the invariant mode it takes a projection up to (M/128)(N/128) nz = 128, one round of the
               chip's 512 workgroup slots for its own grid (kSplitSmallMaxWgs, measured: profiles/batch_invariant_probe.log)
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, BF16X6, FP16X3 = 0, 1, 2, 3                      # IEFVAD_COMPUTE_*


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("launch_rules_invariant")), "launch_rules_invariant")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cabi", "launch_rules_invariant.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]

    def ask(queries):
        """answers to the queries, one per line; an `always` line has no answer"""
        r = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        got = r.stdout.splitlines()
        assert len(got) == sum(not q.startswith("always") for q in queries)
        return got
    return ask


def flags(**on):
    return " ".join(f"{k}={int(v)}" for k, v in on.items())


def passf(split, f16=0, need_xb0=0):
    return flags(ip_chain=0, need_xb0=need_xb0, splitmb=split, f16mb=f16, ln_fused=0)


def tail(split, fold):
    return flags(tail_split=split, heads_rows=0, chain=0, fold=fold)


PASS_QUERIES = [f"pass {BF16X6} 256", f"pass {BF16X6} 1280", f"pass {BF16X6} 1536", f"pass {F32} 256", f"pass {F32} 1536",
                f"pass {BF16} 256", f"pass {BF16} 1536", f"pass {FP16X3} 256", f"pass {FP16X3} 1280", f"pass {FP16X3} 1536"]
TAIL_QUERIES = [f"tail {BF16X6} 256 10 1 1 0 0",                 # a compacted 256-row set behind a split encoder
                f"tail {BF16X6} 256 0 1 1 0 0",                  # ... without refinement steps: nothing to fold
                f"tail {BF16X6} 256 10 0 0 0 0",                 # what a default pass of one chunk hands to its tail
                f"tail {BF16X6} 1536 10 1 0 0 0",
                f"tail {F32} 256 10 0 0 0 0", f"tail {BF16} 256 10 0 0 0 0",
                f"tail {FP16X3} 256 10 0 0 0 0", f"tail {FP16X3} 1280 10 1 1 0 0", f"tail {FP16X3} 1536 10 1 0 0 0"]


def test_split_always_splits_every_bf16x6_pass_and_tail(ask):
    assert ask(["always 1"] + PASS_QUERIES) == [
        passf(1), passf(1), passf(1), passf(0), passf(0), passf(0, need_xb0=1), passf(0, need_xb0=1),
        passf(0), passf(0), passf(1, f16=1)]                      # fp16x3 keeps its rule: split from 1,536 rows on
    assert ask(["always 1"] + TAIL_QUERIES) == [
        tail(1, 1), tail(1, 0), tail(1, 1), tail(1, 1), tail(0, 0), tail(0, 0),
        tail(0, 0), tail(0, 0), tail(1, 0)]


def test_default_policy_answers_as_before(ask):
    want_pass = [passf(0), passf(0), passf(1), passf(0), passf(0), passf(0, need_xb0=1), passf(0, need_xb0=1),
                 passf(0), passf(0), passf(1, f16=1)]
    want_tail = [tail(0, 0), tail(0, 0), tail(0, 0), tail(1, 1), tail(0, 0), tail(0, 0), tail(0, 0), tail(0, 0), tail(1, 0)]
    assert ask(PASS_QUERIES) == want_pass
    assert ask(TAIL_QUERIES) == want_tail
    assert ask(["always 1", "always 0"] + PASS_QUERIES + TAIL_QUERIES) == want_pass + want_tail      # switched off again


def test_small_plan_grid_and_refusals(ask):
    assert ask(["small 256 768 768 1 0 0", "small 256 2304 768 2 0 0", "small 1280 1536 768 1 0 0", "small 32 128 64 1 0 0",
                "small 256 768 768 1 1 1"]) == ["small 48", "small 144", "small 480", "small 1", "small 48"]      # 8 x 6, 8 x 18, 40 x 12
    assert ask(["small 48 768 768 1 0 0", "small 256 192 768 1 0 0", "small 256 768 32 1 0 0", "small 256 768 96 1 0 0",
                "small 0 768 768 1 0 0", "small 256 768 768 3 0 0",
                "small 256 768 768 1 1 0", "small 256 768 768 2 1 1"]) == ["reject shape"] * 6 + ["reject dot_epilogue"] * 2


def test_small_tiling_takes_a_projection_while_its_grid_fits_one_round_of_the_chip(ask):
    # up to 128 workgroups of 128 x 128 (512 of 32 x 128).  768-wide, one problem: 12 per chunk -- 1,536 rows are 72 (the default mode's
    # crossover to the split kernels, still small here), 2,560 rows 120, 2,816 rows 132.  in_proj (N = 2304, two problems): 72 per chunk;
    # out_proj (N = 768, two problems): 24 per chunk, 5 chunks 120, 6 chunks 144; the heads (N = 1536, two problems): 48 per chunk.
    # A row count that is no multiple of 128 has no 128 x 128 plan at all.
    assert ask(["prefer_small 256 768 768 1", "prefer_small 1536 768 768 1", "prefer_small 2560 768 768 1", "prefer_small 2816 768 768 1",
                "prefer_small 256 2304 768 2", "prefer_small 512 2304 768 2",
                "prefer_small 1280 768 768 2", "prefer_small 1536 768 768 2",
                "prefer_small 512 1536 768 2", "prefer_small 768 1536 768 2",
                "prefer_small 96 768 768 1"]) == ["1", "1", "1", "0", "1", "0", "1", "0", "1", "0", "1"]
