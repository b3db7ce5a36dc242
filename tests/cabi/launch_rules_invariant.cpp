// CPU-only driver for the batch-invariant part of the kernel-selection rules (ief-vad_amd/csrc/launch_rules.h): LaunchPolicy::split_always
// and plan_gemm_split_small.  Built by tests/test_launch_rules_invariant_cpu.py with g++ -std=c++17 -Wall -Werror.  Reads one query per
// line from stdin; the test holds the expected answers.  Queries (all numbers decimal):
//   always ON                            LaunchPolicy::split_always of the queries that follow (the other switches at their defaults)
//   pass COMPUTE ROWS                    -> ip_chain need_xb0 splitmb f16mb ln_fused
//   tail COMPUTE ROWS K SPLITMB COMPACTED HEADS_PACKED CHAIN_PACKED   -> tail_split heads_rows chain fold
//   small M N K NZ DOT DOT_OPS           -> small <wgs> | reject <reason>
//   prefer_small M N K NZ                -> 0 | 1: the small tiling takes the projection in the invariant mode
#include <stdio.h>
#include <string.h>

#include "../../ief-vad_amd/csrc/launch_rules.h"

int main() {
    LaunchPolicy policy = launch_policy(0, 0, 0, true, 0, false);
    char line[256], op[32];
    while (fgets(line, sizeof(line), stdin)) {
        int a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int n = sscanf(line, "%31s %d %d %d %d %d %d %d %d", op, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6], &a[7]) - 1;
        if (n < 0) continue;
        auto is = [&](const char* name, int args) { return !strcmp(op, name) && n == args; };
        if (is("always", 1)) policy.split_always = a[0] != 0;
        else if (is("pass", 2)) {
            const PassFlags f = plan_pass(policy, a[0], a[1]);
            printf("ip_chain=%d need_xb0=%d splitmb=%d f16mb=%d ln_fused=%d\n", f.ip_chain, f.need_xb0, f.splitmb, f.f16mb, f.ln_fused);
        } else if (is("tail", 7)) {
            const TailFlags f = plan_tail(policy, a[0], a[1], a[2], a[3] != 0, a[4] != 0, a[5] != 0, a[6] != 0);
            printf("tail_split=%d heads_rows=%d chain=%d fold=%d\n", f.tail_split, f.heads_rows, f.chain, f.fold);
        } else if (is("small", 6)) {
            const GemmSmallPlan p = plan_gemm_split_small(a[0], a[1], a[2], a[3], a[4] != 0, a[5] != 0);
            if (p.ok) printf("small %d\n", p.wgs);
            else printf("reject %s\n", p.why == GEMM_BAD_SHAPE ? "shape" : p.why == GEMM_BAD_DOT_EPILOGUE ? "dot_epilogue" : "?");
        } else if (is("prefer_small", 4)) printf("%d\n", (int)split_small_preferred(a[0], a[1], a[2], a[3]));
        else {
            fprintf(stderr, "launch_rules_invariant: bad query: %s", line);
            return 2;
        }
    }
    return 0;
}
