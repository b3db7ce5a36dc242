// Prints the window plan of an online call as ief-vad_amd/csrc/window_plan.h lays it out (tests/test_online_cpu.py compiles this with
// g++ and compares the lines with harness.online_windows).  Usage: online_plan STRIDE HISTORY MICRO_BATCH LEN...
//   ok 0|1                                  online_params_ok
//   w VIDEO START END READ0                 one line per window, in packed rows of the call
//   r SKIP COUNT DST                        its read-out map (OnlineRead), dst relative to its pass
//   p FIRST COUNT SRC_BASE OUT_BASE OUT_ROWS   one line per pass
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "window_plan.h"

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const int stride = atoi(argv[1]), history = atoi(argv[2]), mb = atoi(argv[3]);
    std::vector<int32_t> lens;
    for (int i = 4; i < argc; ++i) lens.push_back(atoi(argv[i]));
    printf("ok %d\n", online_params_ok(stride, history) ? 1 : 0);
    if (!online_params_ok(stride, history)) return 0;
    const long long W = online_call_windows(lens.data(), (int)lens.size(), stride);
    printf("n %lld\n", W);
    if (W <= 0) return 0;
    std::vector<OnlineWindow> win((size_t)W);
    online_fill_windows(lens.data(), (int)lens.size(), stride, history, win.data());
    for (long long c0 = 0; c0 < W; c0 += mb) {
        const OnlinePass p = online_pass(win.data(), W, mb, c0);
        printf("p %lld %d %lld %lld %d\n", p.first, p.count, p.src_base, p.out_base, p.out_rows);
        for (int j = 0; j < p.count; ++j) {
            const OnlineWindow& w = win[c0 + j];
            const OnlineRead r = online_read(w, p);
            printf("w %d %lld %lld %lld\n", w.video, w.start, w.end, w.read0);
            printf("r %d %d %d\n", r.skip, r.count, r.dst);
        }
    }
    return 0;
}
