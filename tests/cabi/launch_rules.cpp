// CPU-only driver for the kernel-selection rules (ief-vad_amd/csrc/launch_rules.h, the very header libiefvad.so is built from),
// built by tests/cabi/Makefile with g++ -std=c++17 -Wall -Werror.  Reads one query per line from stdin and prints the plan the
// launch code would execute; tests/test_launch_rules_cpu.py holds the expected answers.  Queries (all numbers decimal):
//   policy OFF MIN_WGS CHAIN_MIN PERSIST SPLIT_TILE DENSE   the switches of the queries that follow (0 = unset; PERSIST 0 / 1)
//   f32 M N K NZ                         -> <kernel> <wgs> | reject
//   bf16 M N K NZ REFINE                 -> <kernel> <wgs> | reject
//   split M N K NZ F16 TILE DOT DOT_OPS  -> <kernel> <wgs> | reject <reason>
//   prefer TILE N F16                    -> the forced tile launch_proj passes on
//   eligible M N K NZ                    -> 0 | 1
//   outln CUS ROWS UNIFORM | attn CUS NB ROWS_MODE | heads CUS ROWS   -> <kernel> <gx> <gy> <gz>
//   pass COMPUTE ROWS                    -> ip_chain need_xb0 splitmb f16mb ln_fused
//   tail COMPUTE ROWS K SPLITMB COMPACTED HEADS_PACKED CHAIN_PACKED   -> tail_split heads_rows chain fold
#include <stdio.h>
#include <string.h>

#include "../../ief-vad_amd/csrc/launch_rules.h"

static const char* gemm_name(GemmKernel k) {
    switch (k) {
    case GEMM_NONE: return "none";
    case GEMM_F32_TINY: return "f32_tiny";
    case GEMM_F32_SMALL: return "f32_small";
    case GEMM_F32_128: return "f32_128";
    case GEMM_F32_T256: return "f32_t256";
    case GEMM_BF16_V1: return "bf16_v1";
    case GEMM_BF16_PIPE: return "bf16_pipe";
    case GEMM_BF16_W256: return "bf16_w256";
    case GEMM_SPLIT_N128: return "split_n128";
    case GEMM_SPLIT_N128X2: return "split_n128x2";
    case GEMM_SPLIT_F16_N128: return "split_f16_n128";
    }
    return "?";
}
static const char* reject_name(GemmReject r) {
    switch (r) {
    case GEMM_OK: return "ok";
    case GEMM_BAD_SHAPE: return "shape";
    case GEMM_BAD_TILE_N: return "tile_n";
    case GEMM_NO_WIDE_TILING: return "no_wide_tiling";
    case GEMM_BAD_DOT_EPILOGUE: return "dot_epilogue";
    }
    return "?";
}
static const char* stage_name(StageKernel k) {
    switch (k) {
    case STAGE_OUTLN_CHAIN: return "outln_chain";
    case STAGE_OUTLN_PCHAIN: return "outln_pchain";
    case STAGE_ATTN_BF16: return "attn_bf16";
    case STAGE_ATTN_BF16_ROWS: return "attn_bf16_rows";
    case STAGE_ATTN_PBF16: return "attn_pbf16";
    case STAGE_ATTN_PBF16_ROWS: return "attn_pbf16_rows";
    case STAGE_HEADS_CHAIN: return "heads_chain";
    case STAGE_HEADS_PCHAIN: return "heads_pchain";
    }
    return "?";
}
static void print(const GemmPlan& p) {
    if (p.reject) printf("reject %s\n", reject_name(p.reject));
    else printf("%s %d\n", gemm_name(p.kernel), p.wgs);
}
static void print(const StagePlan& p) { printf("%s %d %d %d\n", stage_name(p.kernel), p.gx, p.gy, p.gz); }

int main() {
    LaunchPolicy policy = launch_policy(0, 0, 0, true, 0, false);
    char line[256], op[32];
    while (fgets(line, sizeof(line), stdin)) {
        int a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int n = sscanf(line, "%31s %d %d %d %d %d %d %d %d", op, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6], &a[7]) - 1;
        if (n < 0) continue;
        auto is = [&](const char* name, int args) { return !strcmp(op, name) && n == args; };
        if (is("policy", 6)) policy = launch_policy(a[0], a[1], a[2], a[3] != 0, a[4], a[5] != 0);
        else if (is("f32", 4)) print(plan_gemm_f32(a[0], a[1], a[2], a[3]));
        else if (is("bf16", 5)) print(plan_gemm_bf16(a[0], a[1], a[2], a[3], a[4] != 0));
        else if (is("split", 8)) print(plan_gemm_split(a[0], a[1], a[2], a[3], a[4] != 0, a[5], a[6] != 0, a[7] != 0));
        else if (is("prefer", 3)) printf("%d\n", split_tile_for(a[0], a[1], a[2] != 0));
        else if (is("eligible", 4)) printf("%d\n", (int)split_eligible(a[0], a[1], a[2], a[3]));
        else if (is("outln", 3)) print(plan_outproj_ln(policy, a[0], a[1], a[2] != 0));
        else if (is("attn", 3)) print(plan_attention_bf16(policy, a[0], a[1], a[2] != 0));
        else if (is("heads", 2)) print(plan_heads(policy, a[0], a[1]));
        else if (is("pass", 2)) {
            const PassFlags f = plan_pass(policy, a[0], a[1]);
            printf("ip_chain=%d need_xb0=%d splitmb=%d f16mb=%d ln_fused=%d\n", f.ip_chain, f.need_xb0, f.splitmb, f.f16mb, f.ln_fused);
        } else if (is("tail", 7)) {
            const TailFlags f = plan_tail(policy, a[0], a[1], a[2], a[3] != 0, a[4] != 0, a[5] != 0, a[6] != 0);
            printf("tail_split=%d heads_rows=%d chain=%d fold=%d\n", f.tail_split, f.heads_rows, f.chain, f.fold);
        } else {
            fprintf(stderr, "launch_rules: bad query: %s", line);
            return 2;
        }
    }
    return 0;
}
