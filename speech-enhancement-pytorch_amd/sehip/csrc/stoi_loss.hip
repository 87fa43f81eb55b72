// The backward pass of STOI / ESTOI as a training loss (sehip.loss.stoi_loss): d(-mean_rows d) / d(estimate) behind the forward launches of
// stoi.hip, whose kept / src / tob (and, off 10 kHz, the resampled estimate) it reads.  Gather form throughout: every output element is
// stored once by the thread that owns it, every sum runs in a fixed order, no atomics, nothing is read back.
//   segments : per segment m and band b the derivative of that segment's correlation term with respect to its 30 estimate cells
//              (plain: through c = ||x|| / (||y|| + eps), the clip, the mean removal and the (norm + eps) division; extended: through the
//              row-then-column normalisation), written to seg[row][m][b][30]; then dtob[row][b][t] = the sum over the at most 30 segments
//              that contain frame t in ascending order, scaled by -g / (div M)
//   bands    : one wave per (row, spectrum t): the estimate's frame t of the compacted signal is rebuilt through src and transformed,
//              bin k of band b is weighted by dtob / tob (0 where tob is 0), the adjoint of the zero-padded real transform (an
//              inverse-direction fft512_wave, first 256 outputs) is windowed: fgrad[row][t][256]
//   compact  : inv[row][f] = compacted index of original frame f or -1 (binary search in src); then the gradient of 10 kHz sample n from
//              the at most two kept frames that contain it, each through the at most two spectra that cover its compacted position
//   resample : the adjoint of stoi_resample, dy[k] = sum_m g[m] table[j % p][j / p] with j = L + m q - k p in [0, 2 L]
// Conventions: the kept-frame set is a constant; sqrt at exactly 0 has derivative 0; min passes the gradient to the branch the forward
// took (c y on a tie); a row with fewer than 30 spectra has gradient exactly zero.
#include "stoi_common.h"

namespace {
constexpr int STL_CELLS = ST_BANDS * ST_N;      // floats per segment of the segment-gradient scratch

struct StlBinBand { signed char b[ST_FRAME]; };
constexpr StlBinBand stl_make_binband() {
    constexpr int edge[ST_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
    StlBinBand t{};
    for (int k = 0; k < ST_FRAME; ++k) {
        t.b[k] = -1;
        for (int b = 0; b < ST_BANDS; ++b)
            if (k >= edge[b] && k < edge[b + 1]) t.b[k] = (signed char)b;
    }
    return t;
}
__device__ const StlBinBand g_stl_binband = stl_make_binband();   // band of bin k < 256, -1 outside 7 .. 218

// plain variant: thread (segment, band) as in stoi_segments_kernel
__global__ __launch_bounds__(256) void stoil_segments_kernel(const float* __restrict__ tob, const int* __restrict__ kept, int rows, int F,
                                                             float* __restrict__ seg) {
    __shared__ float xt[ST_BANDS][ST_SEG + ST_N], yt[ST_BANDS][ST_SEG + ST_N];
    const int row = blockIdx.y, T = kept[row] - 1, M = T - (ST_N - 1), m0 = blockIdx.x * ST_SEG;
    if (m0 >= M) return;                                         // (block-uniform)
    st_stage<ST_SEG>(tob, rows, row, F, T, m0, xt, yt);
    __syncthreads();
    const int sl = threadIdx.x / ST_BANDS, b = threadIdx.x - sl * ST_BANDS;
    if (sl >= ST_SEG || m0 + sl >= M) return;
    float xn[ST_N], zc[ST_N], sx = 0.f, sy = 0.f;
#pragma unroll
    for (int i = 0; i < ST_N; ++i) {
        const float x = xt[b][sl + i], y = yt[b][sl + i];
        sx = fmaf(x, x, sx);
        sy = fmaf(y, y, sy);
    }
    const float nys = sqrtf(sy), c = sqrtf(sx) / (nys + ST_EPS);
    float mx = 0.f, mz = 0.f;
#pragma unroll
    for (int i = 0; i < ST_N; ++i) {
        const float x = xt[b][sl + i], cy = yt[b][sl + i] * c, cx = x * ST_CLIP;
        xn[i] = x;
        zc[i] = cy <= cx ? cy : cx;
        mx += xn[i];
        mz += zc[i];
    }
    mx /= (float)ST_N;
    mz /= (float)ST_N;
    sx = sy = 0.f;
#pragma unroll
    for (int i = 0; i < ST_N; ++i) {
        xn[i] -= mx;
        zc[i] -= mz;
        sx = fmaf(xn[i], xn[i], sx);
        sy = fmaf(zc[i], zc[i], sy);
    }
    const float nx = sqrtf(sx) + ST_EPS, nzs = sqrtf(sy), nz = nzs + ST_EPS;
    float corr = 0.f;
#pragma unroll
    for (int i = 0; i < ST_N; ++i) {
        xn[i] /= nx;
        corr += (zc[i] / nz) * xn[i];
    }
    // d corr / d zc = (xn - corr zc / ||zc||) / (||zc|| + eps), the second term 0 at ||zc|| = 0; then the mean removal's adjoint
    const float k1 = nzs > 0.f ? corr / nzs : 0.f;
    float mg = 0.f;
#pragma unroll
    for (int i = 0; i < ST_N; ++i) {
        zc[i] = (xn[i] - k1 * zc[i]) / nz;
        mg += zc[i];
    }
    mg /= (float)ST_N;
    // the clip passes the gradient where the forward took c y; d c / d y = -c / (||y|| + eps) y / ||y||, 0 at ||y|| = 0
    float dc = 0.f;
#pragma unroll
    for (int i = 0; i < ST_N; ++i) {
        const float y = yt[b][sl + i];
        zc[i] = y * c <= xt[b][sl + i] * ST_CLIP ? zc[i] - mg : 0.f;
        dc = fmaf(zc[i], y, dc);
    }
    const float k2 = nys > 0.f ? -dc * c / ((nys + ST_EPS) * nys) : 0.f;
    float* o = seg + (((size_t)row * (F - ST_N) + m0 + sl) * ST_BANDS + b) * ST_N;
#pragma unroll
    for (int i = 0; i < ST_N; ++i) o[i] = fmaf(k2, yt[b][sl + i], c * zc[i]);
}

// the adjoint of o = (v - mean v) / (||v - mean v|| + eps) for one vector of LEN: given go and o (and n = ||v - mean v||), go becomes d / d v
template <int LEN>
__device__ __forceinline__ void stl_norm_bwd(float (&go)[LEN], const float (&o)[LEN], float n) {
    float s = 0.f, mg = 0.f;
#pragma unroll
    for (int i = 0; i < LEN; ++i) s = fmaf(go[i], o[i], s);
    const float k = n > 0.f ? s * (n + ST_EPS) / n : 0.f;
#pragma unroll
    for (int i = 0; i < LEN; ++i) {
        go[i] = (go[i] - k * o[i]) / (n + ST_EPS);
        mg += go[i];
    }
    mg /= (float)LEN;
#pragma unroll
    for (int i = 0; i < LEN; ++i) go[i] -= mg;
}

// extended variant: the forward's two phases, then the column and the row normalisation backwards
__global__ __launch_bounds__(256) void stoil_segments_ext_kernel(const float* __restrict__ tob, const int* __restrict__ kept, int rows, int F,
                                                                 float* __restrict__ seg) {
    __shared__ float xt[ST_BANDS][ST_SEG_EXT + ST_N], yt[ST_BANDS][ST_SEG_EXT + ST_N];
    __shared__ float xn[ST_SEG_EXT][ST_BANDS][ST_N], yn[ST_SEG_EXT][ST_BANDS][ST_N], ny[ST_SEG_EXT][ST_BANDS];
    const int row = blockIdx.y, T = kept[row] - 1, M = T - (ST_N - 1), m0 = blockIdx.x * ST_SEG_EXT;
    if (m0 >= M) return;                                         // (block-uniform)
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
            const float nx = sqrtf(sx) + ST_EPS, nys = sqrtf(sy);
#pragma unroll
            for (int i = 0; i < ST_N; ++i) {
                xn[sl][b][i] = xv[i] / nx;
                yn[sl][b][i] = yv[i] / (nys + ST_EPS);
            }
            ny[sl][b] = nys;
        }
    }
    __syncthreads();
    {   // along the bands: the correlation's gradient with respect to the estimate's column is the clean column; back through the
        // column's normalisation, stored over the clean cell (this thread is its only reader)
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
            const float nx = sqrtf(sx) + ST_EPS, nys = sqrtf(sy);
#pragma unroll
            for (int b = 0; b < ST_BANDS; ++b) {
                xv[b] /= nx;
                yv[b] /= nys + ST_EPS;
            }
            stl_norm_bwd<ST_BANDS>(xv, yv, nys);
#pragma unroll
            for (int b = 0; b < ST_BANDS; ++b) xn[sl][b][i] = xv[b];
        }
    }
    __syncthreads();
    {   // back through the normalisation along time
        const int sl = threadIdx.x / ST_BANDS, b = threadIdx.x - sl * ST_BANDS;
        if (sl < ST_SEG_EXT && m0 + sl < M) {
            float go[ST_N], o[ST_N];
#pragma unroll
            for (int i = 0; i < ST_N; ++i) {
                go[i] = xn[sl][b][i];
                o[i] = yn[sl][b][i];
            }
            stl_norm_bwd<ST_N>(go, o, ny[sl][b]);
            float* out = seg + (((size_t)row * (F - ST_N) + m0 + sl) * ST_BANDS + b) * ST_N;
#pragma unroll
            for (int i = 0; i < ST_N; ++i) out[i] = go[i];
        }
    }
}

// dtob[row][b][t]: the segments m in [t - 29, t] that exist, ascending; zero past the row's T and for a row without a segment
__global__ __launch_bounds__(256) void stoil_gather_kernel(const float* __restrict__ seg, const int* __restrict__ kept, int F, int div,
                                                           const float* __restrict__ gout, int gstride, float scale,
                                                           float* __restrict__ dtob) {
    const int idx = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (idx >= ST_BANDS * (F - 1)) return;
    const int b = idx / (F - 1), t = idx - b * (F - 1), M = kept[row] - ST_N;
    float v = 0.f;
    if (M >= 1 && t < M + ST_N - 1) {
        const int lo = t - (ST_N - 1) > 0 ? t - (ST_N - 1) : 0, hi = t < M - 1 ? t : M - 1;
        float a = 0.f;
        for (int m = lo; m <= hi; ++m) a += seg[(((size_t)row * (F - ST_N) + m) * ST_BANDS + b) * ST_N + (t - m)];
        v = a * (-(gout[(size_t)row * gstride] * scale) / (float)(div * M));
    }
    dtob[((size_t)row * ST_BANDS + b) * (F - 1) + t] = v;
}

__global__ __launch_bounds__(64) void stoil_bands_kernel(const float* __restrict__ est, long len, int rows, int F, const int* __restrict__ kept,
                                                         const int* __restrict__ src, const float* __restrict__ tob,
                                                         const float* __restrict__ dtob, float* __restrict__ fgrad) {
    __shared__ float gr[ST_FRAME], gi[ST_FRAME], wb[ST_BANDS];
    const int row = blockIdx.y, t = blockIdx.x, lane = threadIdx.x, K = kept[row];
    if (K < ST_N + 1 || t >= K - 1) return;                      // no segment in this row, or past its T = K - 1 (the block is one wave)
    const int* s = src + (size_t)row * F;
    const int ja = t > 0 ? s[t - 1] : -1, jb = s[t], jc = s[t + 1];
    const float* y = est + (size_t)row * len;
    float re[8], im[8];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int u = lane + 64 * r;
        re[r] = g_st_win.w[u] * st_hop(y, ja, jb, u);
        re[2 + r] = g_st_win.w[u + ST_HOP] * st_hop(y, jb, jc, u);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        im[r] = 0.f;
        if (r >= 4) re[r] = 0.f;
    }
    FftTw tw;
    fft_twiddles<-1>(tw, lane);
    fft512_wave<-1>(re, im, tw, lane);
    if (lane < ST_BANDS) {
        const float mag = tob[((size_t)(rows + row) * ST_BANDS + lane) * (F - 1) + t];
        const float d = dtob[((size_t)row * ST_BANDS + lane) * (F - 1) + t];
        wb[lane] = mag != 0.f ? d / mag : 0.f;
    }
    __syncthreads();
    constexpr int brev3[8] = {0, 4, 2, 6, 1, 5, 3, 7};
    const int k0 = 8 * brev6(lane);
    if (k0 < ST_FRAME) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + brev3[j], b = g_stl_binband.b[k];
            const float w = b >= 0 ? wb[b] : 0.f;
            gr[k] = w * re[j];
            gi[k] = w * im[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        re[r] = r < 4 ? gr[lane + 64 * r] : 0.f;
        im[r] = r < 4 ? gi[lane + 64 * r] : 0.f;
    }
    fft_twiddles<1>(tw, lane);
    fft512_wave<1>(re, im, tw, lane);
    if (k0 < ST_FRAME) {
        float* o = fgrad + ((size_t)row * (F - 1) + t) * ST_FRAME;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[k0 + brev3[j]] = g_st_win.w[k0 + brev3[j]] * re[j];
    }
}

__global__ __launch_bounds__(256) void stoil_inverse_kernel(const int* __restrict__ kept, const int* __restrict__ src, int F,
                                                            int* __restrict__ inv) {
    const int f = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (f >= F) return;
    const int* s = src + (size_t)row * F;
    int lo = 0, hi = kept[row];                                  // src is ascending: the first j with s[j] >= f
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s[mid] < f) lo = mid + 1;
        else hi = mid;
    }
    inv[(size_t)row * F + f] = lo < kept[row] && s[lo] == f ? lo : -1;
}

// the gradient of compacted sample v of kept frame j (position j 128 + v) from the spectra t = h and t = h - 1 that cover it
__device__ __forceinline__ float stl_compacted(const float* __restrict__ fg, int T, int j, int v) {
    const int h = j + (v >> 7), u = v & (ST_HOP - 1);
    float g = 0.f;
    if (h - 1 >= 0 && h - 1 < T) g = fg[(size_t)(h - 1) * ST_FRAME + u + ST_HOP];
    if (h < T) g += fg[(size_t)h * ST_FRAME + u];
    return g;
}

__global__ __launch_bounds__(256) void stoil_compact_kernel(const float* __restrict__ fgrad, const int* __restrict__ kept,
                                                            const int* __restrict__ inv, long len, int F, float* __restrict__ out) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= len) return;
    const int row = blockIdx.y, K = kept[row], T = K - 1;
    float acc = 0.f;
    if (K >= ST_N + 1) {
        const float* fg = fgrad + (size_t)row * (F - 1) * ST_FRAME;
        const int* iv = inv + (size_t)row * F;
        const long f = n >> 7;
        const int v = (int)(n & (ST_HOP - 1));
        if (f - 1 >= 0 && f - 1 < F) {
            const int j = iv[f - 1];
            if (j >= 0) acc = g_st_win.w[v + ST_HOP] * stl_compacted(fg, T, j, v + ST_HOP);
        }
        if (f < F) {
            const int j = iv[f];
            if (j >= 0) acc = fmaf(g_st_win.w[v], stl_compacted(fg, T, j, v), acc);
        }
    }
    out[(size_t)row * len + n] = acc;
}

__global__ __launch_bounds__(256) void stoil_resample_adj_kernel(const float* __restrict__ g, long n, const float* __restrict__ table, int p,
                                                                 int q, int L, int kt, long n_out, float* __restrict__ out) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int row = blockIdx.y;
    const float* gr = g + (size_t)row * n_out;
    const long c = k * p;
    const long lo = c - L > 0 ? (c - L + q - 1) / q : 0;            // outputs m with 0 <= L + m q - k p <= 2 L
    const long hi = (c + L) / q < n_out - 1 ? (c + L) / q : n_out - 1;
    const long j0 = L + lo * q - c;
    int r = (int)(j0 % p), i = (int)(j0 / p);
    const int dr = q % p, di = q / p;
    float a = 0.f;                                                  // about 2 L / q + 1 terms, ascending m
    for (long m = lo; m <= hi; ++m) {
        a = fmaf(table[(size_t)r * kt + i], gr[m], a);
        r += dr;
        i += di;
        if (r >= p) { r -= p; ++i; }
    }
    out[(size_t)row * n + k] = a;
}
}  // namespace

extern "C" long sehip_stoil_segment_floats(int rows, int F) {
    if (rows <= 0 || F <= 0) return -1;
    return (long)rows * (F > ST_N ? F - ST_N : 1) * STL_CELLS;
}

extern "C" int sehip_stoil_segments(const float* tob, const int* kept, int rows, int F, int extended, const float* gout, int gstride,
                                    float scale, float* seg, float* dtob, void* stream) {
    SEHIP_REQUIRE(rows > 0 && rows <= ST_MAX_ROWS, "stoil_segments: rows=%d outside [1, %d]", rows, ST_MAX_ROWS);
    SEHIP_REQUIRE(F > 0, "stoil_segments: F=%d frames, need at least one", F);
    SEHIP_REQUIRE(extended == 0 || extended == 1, "stoil_segments: extended=%d is neither 0 nor 1", extended);
    SEHIP_REQUIRE(gstride == 0 || gstride == 1, "stoil_segments: gstride=%d is neither 0 (one gradient) nor 1 (one per row)", gstride);
    SEHIP_REQUIRE(tob && kept && gout && seg && dtob, "stoil_segments: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (F > ST_N) {                                              // else every row has T < 30
        const int m = F - ST_N;
        if (extended) stoil_segments_ext_kernel<<<dim3(cdiv(m, ST_SEG_EXT), rows), 256, 0, st>>>(tob, kept, rows, F, seg);
        else stoil_segments_kernel<<<dim3(cdiv(m, ST_SEG), rows), 256, 0, st>>>(tob, kept, rows, F, seg);
        SEHIP_CHECK_LAUNCH("stoil_segments");
    }
    if (F > 1) {
        stoil_gather_kernel<<<dim3(cdiv((long)ST_BANDS * (F - 1), 256), rows), 256, 0, st>>>(seg, kept, F, extended ? ST_N : ST_BANDS, gout,
                                                                                              gstride, scale, dtob);
        SEHIP_CHECK_LAUNCH("stoil_segments (gather)");
    }
    sehip_note_kernel("stoil_segments%s F=%d", extended ? "_ext" : "", F);
    return 0;
}

#define STL_REQUIRE_ROWS_LEN(who)                                                                                  \
    SEHIP_REQUIRE(rows > 0 && rows <= ST_MAX_ROWS, who ": rows=%d outside [1, %d]", rows, ST_MAX_ROWS);            \
    SEHIP_REQUIRE(len >= ST_FRAME && len <= ST_MAX_LEN, who ": len=%ld outside [256, 2^30] samples at 10 kHz", len)

extern "C" int sehip_stoil_bands(const float* est, int rows, long len, const int* kept, const int* src, const float* tob, const float* dtob,
                                 float* fgrad, void* stream) {
    STL_REQUIRE_ROWS_LEN("stoil_bands");
    SEHIP_REQUIRE(est && kept && src && tob && dtob && fgrad, "stoil_bands: null pointer");
    const int F = (int)((len - ST_FRAME) / ST_HOP + 1);
    if (F > 1) {
        stoil_bands_kernel<<<dim3(F - 1, rows), 64, 0, (hipStream_t)stream>>>(est, len, rows, F, kept, src, tob, dtob, fgrad);
        SEHIP_CHECK_LAUNCH("stoil_bands");
    }
    sehip_note_kernel("stoil_bands F=%d", F);
    return 0;
}

extern "C" int sehip_stoil_compact(const float* fgrad, const int* kept, const int* src, int rows, long len, int* inv, float* out,
                                   void* stream) {
    STL_REQUIRE_ROWS_LEN("stoil_compact");
    SEHIP_REQUIRE(fgrad && kept && src && inv && out, "stoil_compact: null pointer");
    const int F = (int)((len - ST_FRAME) / ST_HOP + 1);
    hipStream_t st = (hipStream_t)stream;
    stoil_inverse_kernel<<<dim3(cdiv(F, 256), rows), 256, 0, st>>>(kept, src, F, inv);
    SEHIP_CHECK_LAUNCH("stoil_compact (inverse)");
    stoil_compact_kernel<<<dim3(cdiv(len, 256), rows), 256, 0, st>>>(fgrad, kept, inv, len, F, out);
    SEHIP_CHECK_LAUNCH("stoil_compact");
    sehip_note_kernel("stoil_compact F=%d", F);
    return 0;
}

extern "C" int sehip_stoil_resample_adj(const float* g, int rows, long n, const float* table, int p, int q, int L, float* out, void* stream) {
    SEHIP_REQUIRE(rows > 0 && rows <= ST_MAX_ROWS, "stoil_resample_adj: rows=%d outside [1, %d]", rows, ST_MAX_ROWS);
    SEHIP_REQUIRE(p > 0 && q > 0 && p <= ST_MAX_P && q <= ST_MAX_Q, "stoil_resample_adj: ratio %d / %d outside p <= %d, q <= %d", p, q,
                  ST_MAX_P, ST_MAX_Q);
    SEHIP_REQUIRE(p != q, "stoil_resample_adj: ratio %d / %d is 1 / 1: nothing to do", p, q);
    SEHIP_REQUIRE(L > 0 && L <= (1 << 20), "stoil_resample_adj: half length L=%d outside [1, 2^20]", L);
    SEHIP_REQUIRE(n > 0 && n <= ST_MAX_LEN, "stoil_resample_adj: n=%ld outside [1, 2^30]", n);
    SEHIP_REQUIRE(g && table && out, "stoil_resample_adj: null pointer");
    const long n_out = (n * p + q - 1) / q;
    SEHIP_REQUIRE(n_out <= ST_MAX_LEN, "stoil_resample_adj: %ld samples at 10 kHz are more than 2^30", n_out);
    const int kt = 2 * L / p + 1;
    stoil_resample_adj_kernel<<<dim3(cdiv(n, 256), rows), 256, 0, (hipStream_t)stream>>>(g, n, table, p, q, L, kt, n_out, out);
    SEHIP_CHECK_LAUNCH("stoil_resample_adj");
    sehip_note_kernel("stoil_resample_adj p=%d q=%d L=%d kt=%d", p, q, L, kt);
    return 0;
}
