// Which kernel sehip_resample_frac (resample.hip) runs for a reduced ratio old -> new and a width, and with what tiling.  Host-only
// arithmetic, shared with resample_stream.hip: a streamed sample has the bits of the offline one only if it is summed in the order of
// the kernel that serves its ratio offline, so both files ask the same function.
#pragma once
#include <cstddef>

constexpr size_t RS_LDS_MAX = 160 * 1024;
constexpr int RS_WAVES = 16;         // phase kernel: 1024 threads, 4 waves per SIMD behind the scalar loads' latency
constexpr int RS_DT = 8;             // decim kernel: consecutive outputs per thread
constexpr int RS_DF = 256 * RS_DT;   //               outputs per tile

enum rs_kind { RS_DECIM = 0, RS_PHASE = 1, RS_DIRECT = 2 };

struct rs_plan {
    rs_kind kind;
    long K;          // taps, 2 * width + old
    size_t lds;      // dynamic LDS bytes (decim, phase)
    int os, P, wf;   // phase: LDS row stride in words, phases per lane, waves along frames
};

inline rs_plan rs_make_plan(int old_sr, int new_sr, int width) {
    rs_plan pl = {RS_DIRECT, 2L * width + old_sr, 0, 0, 0, 0};
    const long K = pl.K, J = (K + old_sr - 1) / old_sr;
    if (new_sr == 1) {
        const long W = (long)(RS_DF - 1) * old_sr + K;
        const size_t lds = (size_t)(W + ((W / old_sr) >> 3) + 8) * sizeof(float);
        if (lds <= RS_LDS_MAX) {
            pl.kind = RS_DECIM;
            pl.lds = lds;
            return pl;
        }
    }
    int os = (old_sr + 3) & ~3;                                   // LDS row stride: a multiple of 4 words that is 4 (mod 8)
    if ((os & 7) == 0) os += 4;
    // P phases per lane and wf of the 16 waves along frames (the rest along phase groups): the pair with the least estimated
    // wave-time per frame, rounds * (P + 2) / wf -- P pairs of FMAs per tap quad plus ~2 for the LDS read, the scalar loads' issue
    // and the loop; a tie goes to the larger P.  (An estimate: measured at 441 -> 160 only)
    int P = 0, wf = 0;
    long best = 0;
    for (int p = 8; p >= 1; p >>= 1) {
        if (p > 1 && p / 2 >= new_sr) continue;                   // more than half of the phases would be padding
        const int groups = (new_sr + p - 1) / p;
        int w = RS_WAVES;
        while (w > 1 && (RS_WAVES / w < groups || (size_t)(64 * w + J) * os * sizeof(float) > RS_LDS_MAX)) w >>= 1;
        const long rounds = (groups + RS_WAVES / w - 1) / (RS_WAVES / w), cost = rounds * (p + 2) * RS_WAVES / w;
        if (!P || cost < best) { P = p; wf = w; best = cost; }
    }
    const size_t lds = (size_t)(64 * wf + J) * os * sizeof(float);
    if (lds <= RS_LDS_MAX) {
        pl.kind = RS_PHASE;
        pl.lds = lds;
        pl.os = os;
        pl.P = P;
        pl.wf = wf;
    }
    return pl;
}
