// STOI / ESTOI (Taal et al. 2011, Jensen & Taal 2016; the `stoi(..., extended=False)` that src/metric.py:126-144 calls per utterance) on
// the device, for rows of clean / estimate pairs:
//   resample : polyphase FIR to 10 kHz, out[m] = p sum_k x[k] w[L + m q - k p] with zeros outside x (resample_poly, not the replicate
//              padding of resample.hip), from a phase-major table tab[r][i] = p w[r + i p]
//   levels   : e_f = 20 log10(||win * frame_f|| + eps) of the clean rows' frames (256 samples, hop 128)
//   select   : row maximum, keep mask (within 40 dB of the loudest frame), exclusive scan -> kept[row], src[row][j]
//   bands    : frame t of the COMPACTED signal (the kept windowed frames overlap-added at hop 128) is gathered through src, windowed
//              again, clean in the real and estimate in the imaginary part of one 512-point transform (an all-zero frame of either is
//              kept exactly zero); the 15 third-octave band magnitudes of both are all that is stored
//   segments : the sliding 30-frame correlation (plain: scale, clip, centre, normalise per band; extended: normalise along time, then
//              along the bands), a fixed-order partial sum per block, then d[row] and the mean over rows
// The number of kept frames K is data-dependent per row and never leaves the device: every grid is sized by the upper bound (F frames)
// and the workgroups past a row's own count exit.  fp32, no atomics, every output element stored once, every sum in a fixed order.
#include "stoi_common.h"

namespace {
__global__ __launch_bounds__(256) void stoi_resample_kernel(const float* __restrict__ clean, const float* __restrict__ est, int rows, long n,
                                                            const float* __restrict__ table, int p, int q, int L, int kt, long n_out,
                                                            float* __restrict__ out) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= n_out) return;
    const int row = blockIdx.y;
    const float* x = row < rows ? clean + (size_t)row * n : est + (size_t)(row - rows) * n;
    const long base = m * q + L, k = base / p;
    const float* t = table + (size_t)(base - k * p) * kt;
    const long lo = k - (n - 1) > 0 ? k - (n - 1) : 0;           // taps i with 0 <= k - i < n
    const long hi = k < kt - 1 ? k : kt - 1;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;                // four chains, always combined in the same order
    long i = lo;
    for (; i + 3 <= hi; i += 4) {
        a0 = fmaf(t[i], x[k - i], a0);
        a1 = fmaf(t[i + 1], x[k - i - 1], a1);
        a2 = fmaf(t[i + 2], x[k - i - 2], a2);
        a3 = fmaf(t[i + 3], x[k - i - 3], a3);
    }
    for (; i <= hi; ++i) a0 = fmaf(t[i], x[k - i], a0);
    out[(size_t)row * n_out + m] = (a0 + a1) + (a2 + a3);
}

__global__ __launch_bounds__(256) void stoi_levels_kernel(const float* __restrict__ clean, long len, int F, float* __restrict__ level) {
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= F) return;                                          // (wave-uniform)
    const int row = blockIdx.y;
    const float* x = clean + (size_t)row * len + (size_t)f * ST_HOP;
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float v = g_st_win.w[lane + 64 * r] * x[lane + 64 * r];
        s = fmaf(v, v, s);
    }
    s = wave_sum(s);
    if (lane == 0) level[(size_t)row * F + f] = 20.f * log10f(sqrtf(s) + ST_EPS);
}

__global__ __launch_bounds__(256) void stoi_select_kernel(const float* __restrict__ level, int F, int* __restrict__ kept,
                                                          int* __restrict__ src) {
    __shared__ float red[4];
    __shared__ int cnt[4];
    const int row = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* e = level + (size_t)row * F;
    int* s = src + (size_t)row * F;
    float mx = -INFINITY;
    for (int f = threadIdx.x; f < F; f += 256) mx = fmaxf(mx, e[f]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) red[w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    int running = 0;
    for (int base = 0; base < F; base += 256) {
        const int f = base + threadIdx.x;
        const bool keep = f < F && (mx - ST_DYN - e[f]) < 0.f;
        const unsigned long long b = __ballot(keep);
        __syncthreads();                                         // the previous round's counts are read
        if (lane == 0) cnt[w] = __popcll(b);
        __syncthreads();
        int off = running;
        for (int i = 0; i < w; ++i) off += cnt[i];
        if (keep) s[off + __popcll(b & ((1ull << lane) - 1ull))] = f;
        running += cnt[0] + cnt[1] + cnt[2] + cnt[3];
    }
    if (threadIdx.x == 0) kept[row] = running;
}

__global__ __launch_bounds__(64) void stoi_bands_kernel(const float* __restrict__ clean, const float* __restrict__ est, int rows, long len,
                                                        int F, const int* __restrict__ kept, const int* __restrict__ src,
                                                        float* __restrict__ tob) {
    __shared__ float pw[2][256];
    const int row = blockIdx.y, t = blockIdx.x, lane = threadIdx.x;
    if (t >= kept[row] - 1) return;                              // T = K - 1 frames (the whole block is one wave)
    const int* s = src + (size_t)row * F;
    const int ja = t > 0 ? s[t - 1] : -1, jb = s[t], jc = s[t + 1];
    const float* x = clean + (size_t)row * len;
    const float* y = est + (size_t)row * len;
    float re[8], im[8];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int u = lane + 64 * r;
        const float w0 = g_st_win.w[u], w1 = g_st_win.w[u + ST_HOP];
        re[r] = w0 * st_hop(x, ja, jb, u);
        im[r] = w0 * st_hop(y, ja, jb, u);
        re[2 + r] = w1 * st_hop(x, jb, jc, u);
        im[2 + r] = w1 * st_hop(y, jb, jc, u);
    }
#pragma unroll
    for (int r = 4; r < 8; ++r) re[r] = im[r] = 0.f;
    // The split of the pair leaves rounding residue of one signal in the other (~1e-8 of its magnitude): nothing against a signal, but
    // an all-zero frame has the spectrum zero exactly, and a silent clean row must give 0.0 and not the correlation of that residue.
    const bool xzero = __ballot(re[0] != 0.f || re[1] != 0.f || re[2] != 0.f || re[3] != 0.f) == 0ull;
    const bool yzero = __ballot(im[0] != 0.f || im[1] != 0.f || im[2] != 0.f || im[3] != 0.f) == 0ull;
    FftTw tw;
    fft_twiddles<-1>(tw, lane);
    fft512_wave<-1>(re, im, tw, lane);
    float ar[8], ai[8], br[8], bi[8];
    fft_pair_split(re, im, lane, ar, ai, br, bi);
    constexpr int brev3[8] = {0, 4, 2, 6, 1, 5, 3, 7};
    const int k0 = 8 * brev6(lane);
    if (k0 < 256) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            pw[0][k0 + brev3[j]] = xzero ? 0.f : ar[j] * ar[j] + ai[j] * ai[j];
            pw[1][k0 + brev3[j]] = yzero ? 0.f : br[j] * br[j] + bi[j] * bi[j];
        }
    }
    __syncthreads();
    if (lane < 2 * ST_BANDS) {
        const int sig = lane / ST_BANDS, b = lane - sig * ST_BANDS;
        float a = 0.f;
        for (int k = g_st_band[b]; k < g_st_band[b + 1]; ++k) a += pw[sig][k];
        tob[((size_t)(sig * rows + row) * ST_BANDS + b) * (F - 1) + t] = sqrtf(a);
    }
}

__global__ __launch_bounds__(256) void stoi_segments_kernel(const float* __restrict__ tob, const int* __restrict__ kept, int rows, int F,
                                                            int nblk, float* __restrict__ partial) {
    __shared__ float xt[ST_BANDS][ST_SEG + ST_N], yt[ST_BANDS][ST_SEG + ST_N], red[4];
    const int row = blockIdx.y, T = kept[row] - 1, M = T - (ST_N - 1), m0 = blockIdx.x * ST_SEG;
    if (m0 >= M) return;                                         // (block-uniform)
    st_stage<ST_SEG>(tob, rows, row, F, T, m0, xt, yt);
    __syncthreads();
    const int sl = threadIdx.x / ST_BANDS, b = threadIdx.x - sl * ST_BANDS;
    float corr = 0.f;
    if (sl < ST_SEG && m0 + sl < M) {
        float xv[ST_N], yv[ST_N], sx = 0.f, sy = 0.f;
#pragma unroll
        for (int i = 0; i < ST_N; ++i) {
            xv[i] = xt[b][sl + i];
            yv[i] = yt[b][sl + i];
            sx = fmaf(xv[i], xv[i], sx);
            sy = fmaf(yv[i], yv[i], sy);
        }
        const float c = sqrtf(sx) / (sqrtf(sy) + ST_EPS);
        float mx = 0.f, my = 0.f;
#pragma unroll
        for (int i = 0; i < ST_N; ++i) {
            yv[i] = fminf(yv[i] * c, xv[i] * ST_CLIP);
            mx += xv[i];
            my += yv[i];
        }
        mx /= (float)ST_N;
        my /= (float)ST_N;
        sx = sy = 0.f;
#pragma unroll
        for (int i = 0; i < ST_N; ++i) {
            xv[i] -= mx;
            yv[i] -= my;
            sx = fmaf(xv[i], xv[i], sx);
            sy = fmaf(yv[i], yv[i], sy);
        }
        const float nx = sqrtf(sx) + ST_EPS, ny = sqrtf(sy) + ST_EPS;
#pragma unroll
        for (int i = 0; i < ST_N; ++i) corr += (yv[i] / ny) * (xv[i] / nx);
    }
    const float tot = block_sum<4>(corr, red);
    if (threadIdx.x == 0) partial[(size_t)row * nblk + blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void stoi_segments_ext_kernel(const float* __restrict__ tob, const int* __restrict__ kept, int rows, int F,
                                                                int nblk, float* __restrict__ partial) {
    __shared__ float xt[ST_BANDS][ST_SEG_EXT + ST_N], yt[ST_BANDS][ST_SEG_EXT + ST_N], red[4];
    __shared__ float xn[ST_SEG_EXT][ST_BANDS][ST_N], yn[ST_SEG_EXT][ST_BANDS][ST_N];
    const int row = blockIdx.y, T = kept[row] - 1, M = T - (ST_N - 1), m0 = blockIdx.x * ST_SEG_EXT;
    if (m0 >= M) return;
    st_stage<ST_SEG_EXT>(tob, rows, row, F, T, m0, xt, yt);
    __syncthreads();
    {   // along time: subtract the mean, divide by the norm + eps
        const int sl = threadIdx.x / ST_BANDS, b = threadIdx.x - sl * ST_BANDS;
        if (sl < ST_SEG_EXT) {
            float xv[ST_N], yv[ST_N], mx = 0.f, my = 0.f, sx = 0.f, sy = 0.f;
#pragma unroll
            for (int i = 0; i < ST_N; ++i) {
                xv[i] = xt[b][sl + i];
                yv[i] = yt[b][sl + i];
                mx += xv[i];
                my += yv[i];
            }
            mx /= (float)ST_N;
            my /= (float)ST_N;
#pragma unroll
            for (int i = 0; i < ST_N; ++i) {
                xv[i] -= mx;
                yv[i] -= my;
                sx = fmaf(xv[i], xv[i], sx);
                sy = fmaf(yv[i], yv[i], sy);
            }
            const float nx = sqrtf(sx) + ST_EPS, ny = sqrtf(sy) + ST_EPS;
#pragma unroll
            for (int i = 0; i < ST_N; ++i) {
                xn[sl][b][i] = xv[i] / nx;
                yn[sl][b][i] = yv[i] / ny;
            }
        }
    }
    __syncthreads();
    float corr = 0.f;
    {   // along the bands, then the correlation of the column
        const int sl = threadIdx.x / ST_N, i = threadIdx.x - sl * ST_N;
        if (sl < ST_SEG_EXT && m0 + sl < M) {
            float xv[ST_BANDS], yv[ST_BANDS], mx = 0.f, my = 0.f, sx = 0.f, sy = 0.f;
#pragma unroll
            for (int b = 0; b < ST_BANDS; ++b) {
                xv[b] = xn[sl][b][i];
                yv[b] = yn[sl][b][i];
                mx += xv[b];
                my += yv[b];
            }
            mx /= (float)ST_BANDS;
            my /= (float)ST_BANDS;
#pragma unroll
            for (int b = 0; b < ST_BANDS; ++b) {
                xv[b] -= mx;
                yv[b] -= my;
                sx = fmaf(xv[b], xv[b], sx);
                sy = fmaf(yv[b], yv[b], sy);
            }
            const float nx = sqrtf(sx) + ST_EPS, ny = sqrtf(sy) + ST_EPS;
#pragma unroll
            for (int b = 0; b < ST_BANDS; ++b) corr += (xv[b] / nx) * (yv[b] / ny);
        }
    }
    const float tot = block_sum<4>(corr, red);
    if (threadIdx.x == 0) partial[(size_t)row * nblk + blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void stoi_finalize_kernel(const float* __restrict__ partial, const int* __restrict__ kept, int rows, int nblk,
                                                            int seg, int div, float* __restrict__ d, float* __restrict__ out) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int row = threadIdx.x; row < rows; row += 256) {
        const int M = kept[row] - ST_N;                          // T - 29 with T = K - 1
        float v = ST_FEW;
        if (M >= 1) {
            const int nb = (M + seg - 1) / seg;
            float s = 0.f;
            for (int i = 0; i < nb; ++i) s += partial[(size_t)row * nblk + i];
            v = s / (float)(div * M);
        }
        d[row] = v;
        acc += v;
    }
    const float tot = block_sum<4>(acc, red);
    if (threadIdx.x == 0) out[0] = tot / (float)rows;
}

long st_gcd(long a, long b) {
    while (b) { const long t = a % b; a = b; b = t; }
    return a;
}
}  // namespace

extern "C" long sehip_stoi_out_len(long n, int sr) {
    if (n < 0 || n > ST_MAX_LEN || sr <= 0) return -1;
    const long g = st_gcd(10000, sr), p = 10000 / g, q = sr / g;
    return (n * p + q - 1) / q;
}

extern "C" int sehip_stoi_frames(long len) { return len < ST_FRAME || len > ST_MAX_LEN ? 0 : (int)((len - ST_FRAME) / ST_HOP + 1); }

extern "C" int sehip_stoi_segment_blocks(int F, int extended) {
    const int m = F - ST_N, seg = extended ? ST_SEG_EXT : ST_SEG;
    return m < 1 ? 1 : (m + seg - 1) / seg;
}

extern "C" int sehip_stoi_resample(const float* clean, const float* est, int rows, long n, const float* table, int p, int q, int L,
                                   float* out, void* stream) {
    SEHIP_REQUIRE(rows > 0 && rows <= ST_MAX_ROWS, "stoi_resample: rows=%d outside [1, %d]", rows, ST_MAX_ROWS);
    SEHIP_REQUIRE(p > 0 && q > 0 && p <= ST_MAX_P && q <= ST_MAX_Q, "stoi_resample: ratio %d / %d outside p <= %d, q <= %d", p, q, ST_MAX_P,
                  ST_MAX_Q);
    SEHIP_REQUIRE(st_gcd(p, q) == 1 && p != q, "stoi_resample: ratio %d / %d is not reduced (or is 1 / 1: nothing to do)", p, q);
    SEHIP_REQUIRE(L > 0 && L <= (1 << 20), "stoi_resample: half length L=%d outside [1, 2^20]", L);
    SEHIP_REQUIRE(n > 0 && n <= ST_MAX_LEN, "stoi_resample: n=%ld outside [1, 2^30]", n);
    SEHIP_REQUIRE(clean && est && table && out, "stoi_resample: null pointer");
    const long n_out = (n * p + q - 1) / q;
    SEHIP_REQUIRE(n_out <= ST_MAX_LEN, "stoi_resample: %ld output samples are more than 2^30", n_out);
    const int kt = 2 * L / p + 1;
    stoi_resample_kernel<<<dim3(cdiv(n_out, 256), 2 * rows), 256, 0, (hipStream_t)stream>>>(clean, est, rows, n, table, p, q, L, kt, n_out,
                                                                                             out);
    SEHIP_CHECK_LAUNCH("stoi_resample");
    sehip_note_kernel("stoi_resample p=%d q=%d L=%d kt=%d", p, q, L, kt);
    return 0;
}

#define ST_REQUIRE_ROWS_LEN(who)                                                                                   \
    SEHIP_REQUIRE(rows > 0 && rows <= ST_MAX_ROWS, who ": rows=%d outside [1, %d]", rows, ST_MAX_ROWS);            \
    SEHIP_REQUIRE(len >= ST_FRAME && len <= ST_MAX_LEN, who ": len=%ld outside [256, 2^30] samples at 10 kHz", len)

extern "C" int sehip_stoi_levels(const float* clean, int rows, long len, float* level, void* stream) {
    ST_REQUIRE_ROWS_LEN("stoi_levels");
    SEHIP_REQUIRE(clean && level, "stoi_levels: null pointer");
    const int F = sehip_stoi_frames(len);
    stoi_levels_kernel<<<dim3(cdiv(F, 4), rows), 256, 0, (hipStream_t)stream>>>(clean, len, F, level);
    SEHIP_CHECK_LAUNCH("stoi_levels");
    sehip_note_kernel("stoi_levels F=%d", F);
    return 0;
}

extern "C" int sehip_stoi_select(const float* level, int rows, int F, int* kept, int* src, void* stream) {
    SEHIP_REQUIRE(rows > 0 && rows <= ST_MAX_ROWS, "stoi_select: rows=%d outside [1, %d]", rows, ST_MAX_ROWS);
    SEHIP_REQUIRE(F > 0, "stoi_select: F=%d frames, need at least one", F);
    SEHIP_REQUIRE(level && kept && src, "stoi_select: null pointer");
    stoi_select_kernel<<<rows, 256, 0, (hipStream_t)stream>>>(level, F, kept, src);
    SEHIP_CHECK_LAUNCH("stoi_select");
    sehip_note_kernel("stoi_select F=%d", F);
    return 0;
}

extern "C" int sehip_stoi_bands(const float* clean, const float* est, int rows, long len, const int* kept, const int* src, float* tob,
                                void* stream) {
    ST_REQUIRE_ROWS_LEN("stoi_bands");
    SEHIP_REQUIRE(clean && est && kept && src && tob, "stoi_bands: null pointer");
    const int F = sehip_stoi_frames(len);
    if (F > 1) {                                                 // one frame: no row has a spectrum (T = K - 1 = 0)
        stoi_bands_kernel<<<dim3(F - 1, rows), 64, 0, (hipStream_t)stream>>>(clean, est, rows, len, F, kept, src, tob);
        SEHIP_CHECK_LAUNCH("stoi_bands");
    }
    sehip_note_kernel("stoi_bands F=%d", F);
    return 0;
}

extern "C" int sehip_stoi_segments(const float* tob, const int* kept, int rows, int F, int extended, float* partial, float* d, float* out,
                                   void* stream) {
    SEHIP_REQUIRE(rows > 0 && rows <= ST_MAX_ROWS, "stoi_segments: rows=%d outside [1, %d]", rows, ST_MAX_ROWS);
    SEHIP_REQUIRE(F > 0, "stoi_segments: F=%d frames, need at least one", F);
    SEHIP_REQUIRE(extended == 0 || extended == 1, "stoi_segments: extended=%d is neither 0 nor 1", extended);
    SEHIP_REQUIRE(tob && kept && partial && d && out, "stoi_segments: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = sehip_stoi_segment_blocks(F, extended);
    if (F > ST_N) {                                              // else every row has T < 30
        if (extended) stoi_segments_ext_kernel<<<dim3(nblk, rows), 256, 0, st>>>(tob, kept, rows, F, nblk, partial);
        else stoi_segments_kernel<<<dim3(nblk, rows), 256, 0, st>>>(tob, kept, rows, F, nblk, partial);
        SEHIP_CHECK_LAUNCH("stoi_segments");
    }
    stoi_finalize_kernel<<<1, 256, 0, st>>>(partial, kept, rows, nblk, extended ? ST_SEG_EXT : ST_SEG, extended ? ST_N : ST_BANDS, d, out);
    SEHIP_CHECK_LAUNCH("stoi_segments (finalize)");
    sehip_note_kernel("stoi_segments%s F=%d blocks=%d", extended ? "_ext" : "", F, nblk);
    return 0;
}
