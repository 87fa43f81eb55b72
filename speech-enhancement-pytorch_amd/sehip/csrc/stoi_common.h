// What the STOI metric (stoi.hip) and its backward pass (stoi_loss.hip) share: the constants of the published algorithm, the analysis
// window, the one-third-octave band table and the gather of one hop of a row's compacted signal.
#pragma once
#include "fft512.h"

namespace {
constexpr int ST_FRAME = 256, ST_HOP = 128, ST_BANDS = 15, ST_N = 30;
constexpr int ST_SEG = 16, ST_SEG_EXT = 8;      // segments per block of the two correlation kernels
constexpr float ST_EPS = 2.220446049250313e-16f;
constexpr float ST_DYN = 40.f;
constexpr float ST_CLIP = 6.623413251903491f;   // 1 + 10^(15 / 20)
constexpr float ST_FEW = 1e-5f;
constexpr int ST_MAX_P = 128, ST_MAX_Q = 1024;
constexpr long ST_MAX_LEN = 1L << 30;
constexpr int ST_MAX_ROWS = 32767;   // 2 rows per pair in the resampler's grid.y

// hanning(258)[1:-1] = 0.5 - 0.5 cos(2 pi (u + 1) / 257), evaluated at compile time in double and rounded once
struct StWin { float w[ST_FRAME]; };
constexpr StWin st_make_win() {
    StWin t{};
    for (int u = 0; u < ST_FRAME; ++u) {
        double c = 0, s = 0;
        fft_detail::cossin_frac(u + 1, ST_FRAME + 1, c, s);
        t.w[u] = (float)(0.5 - 0.5 * c);
    }
    return t;
}
__device__ const StWin g_st_win = st_make_win();
// one-third-octave bands of thirdoct(10000, 512, 15, 150): bins [lo[b], lo[b + 1])
__device__ const int g_st_band[ST_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

// sample u of hop j of a row's compacted signal: the first half of kept frame j plus the second half of kept frame j - 1
__device__ __forceinline__ float st_hop(const float* __restrict__ x, int prev, int cur, int u) {
    float v = cur >= 0 ? g_st_win.w[u] * x[(size_t)cur * ST_HOP + u] : 0.f;
    if (prev >= 0) v += g_st_win.w[u + ST_HOP] * x[(size_t)prev * ST_HOP + ST_HOP + u];
    return v;
}

// the frames [m0, m0 + SEG + 29) of a row's 15 clean and 15 estimate bands, zero past the row's T
template <int SEG>
__device__ __forceinline__ void st_stage(const float* __restrict__ tob, int rows, int row, int F, int T, int m0, float (*xt)[SEG + ST_N],
                                         float (*yt)[SEG + ST_N]) {
    constexpr int W = SEG + ST_N;
    for (int i = threadIdx.x; i < 2 * ST_BANDS * W; i += 256) {
        const int sig = i / (ST_BANDS * W), rem = i - sig * ST_BANDS * W, b = rem / W, c = rem - b * W;
        const float v = m0 + c < T ? tob[((size_t)(sig * rows + row) * ST_BANDS + b) * (F - 1) + m0 + c] : 0.f;
        (sig ? yt : xt)[b][c] = v;
    }
}
}  // namespace
