// CPU-only driver for the layout behind the base workspace (ief-vad_amd/csrc/workspace_tail.h, the very header libiefvad.so is built
// from), built by tests/cabi/Makefile with g++ -std=c++17 -Wall -Werror.  Reads one query per line from stdin,
//   BASE NB D W_ROWS COLSUM TRAJ VARIANTS SAMPLES        (all numbers decimal; the flags 0 / 1, VARIANTS the count)
// and prints the byte offsets `w_rows colsum z_prev var smp total`; tests/test_workspace_tail_cpu.py holds the expected answers.
#include <stdio.h>

#include "../../ief-vad_amd/csrc/workspace_tail.h"

int main() {
    char line[256];
    while (fgets(line, sizeof(line), stdin)) {
        unsigned long long base, nb;
        int D, w_rows, colsum, traj, variants, samples;
        const int n = sscanf(line, "%llu %llu %d %d %d %d %d %d", &base, &nb, &D, &w_rows, &colsum, &traj, &variants, &samples);
        if (n <= 0) continue;
        if (n != 8) {
            fprintf(stderr, "workspace_tail: bad query: %s", line);
            return 2;
        }
        const WorkspaceTail t = workspace_tail((size_t)base, (size_t)nb, D, TailWants{w_rows != 0, colsum != 0, traj != 0, variants, samples != 0});
        printf("%zu %zu %zu %zu %zu %zu\n", t.w_rows, t.colsum, t.z_prev, t.var, t.smp, t.total);
    }
    return 0;
}
