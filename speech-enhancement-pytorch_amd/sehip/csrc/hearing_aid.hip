// The hearing-aid back end of the Clarity path (src/audio.py:33-61 amplify_torch): NAL-R FIR (src/ha/amplifier.py:206-215), the
// compressor (src/ha/compressor.py:73-109) and tanh, all on the device.
//
// FIR (ha_fir_kernel<ADJ>): rows [R][n] fp32, F tap sets [F][K] (K = nfir + 1 <= 1025), a per-row index picks the set.
//     forward  out[r][m] = sum_k h[k] x[r][m - k],  m in [0, n + K - 1), zero outside the row
//     adjoint  dx[r][i]  = sum_k h[k] dout[r][i + k],  i in [0, n)
//   A block of 256 threads takes a tile of HA_FT = 2048 outputs, 8 consecutive outputs per thread.  The tile's inputs and the halo
//   (K - 1 rounded up to 8) are staged in LDS with the zero padding applied while staging, sample i at i + (i >> 3): a lane's 8
//   samples are 9 words from the next lane's, an odd stride, so the lanes' reads are conflict-free.  The taps sit in LDS as well
//   (every lane reads the same word).  A thread keeps a register window of 8 samples; one tap costs one new LDS sample, one tap
//   read and 8 FMAs.  Every output is one fmaf chain over k = 0 .. K - 1 starting from 0: its bits do not depend on the tile, the
//   grid or the other rows.
//
// Compressor: with W = int(rms_buffer_size * fs),
//     lv_i = sqrt((sum of z^2 over the W samples ending at i, zeros before the row) / W + 1e-8)
//     (a, b)_i = lv_i > threshold ? (1 - attack, attack * (lv_i * attenuation + (1 - attenuation) * threshold)) : (1 - release, release)
//     c_i = a_i c_{i-1} + b_i,  c_{-1} = 1;   gain_i = fp32(c_i);   out_i = z_i * gain_i  (tanh of it with soft_clip)
//   c -> a c + b are affine maps and compose associatively: (a2, b2) o (a1, b1) = (a2 a1, a2 b1 + b2).  Both the window sum (a
//   difference of two prefix sums of z^2: the same scan with a = 1) and the recurrence are reduce-then-scan over tiles of
//   HA_CT = 1024 samples, in float64 (a is within 2e-3 of 1: an fp32 scan drifts to 1e-4 relative at 44 320 samples, the float64 one
//   stays at 3e-13 and rounds to the sample-by-sample loop's fp32 value).  Six ordinary launches on one
//   stream, each reading only what an EARLIER launch wrote -- no workgroup ever waits on another, no atomics, nothing synchronises
//   or reads back:
//     1 ha_sq_kernel<false>     per tile: sum of z^2                                   -> tsum [R][T]
//     2 ha_row_scan_kernel      one workgroup per row: exclusive prefix of tsum        -> tpre [R][T]
//     3 ha_sq_kernel<true>      per tile: rescan with the carry-in                     -> P [R][n] (inclusive prefix of z^2)
//     4 ha_comp_kernel<false>   per tile: levels from P, composition of the tile       -> aggA, aggB [R][T]
//     5 ha_row_scan_kernel      one workgroup per row: c at the start of every tile    -> cin [R][T]
//     6 ha_comp_kernel<true>    per tile: rescan with the carry-in, writes gain and out
//   A thread takes 4 consecutive samples, composes them, the 256 thread maps are scanned (Hillis-Steele by __shfl_up inside a wave,
//   the 4 wave totals through LDS), and in the last pass the thread walks its 4 samples from its own carry exactly as the loop does.
//
// Backward of compressor + clip (ha_comp_bwd_kernel): the reference rebuilds the gain from a detached array, so it is a constant:
//     dz = dout * (1 - out^2) * gain   (dout * gain without soft_clip).
#include "common.h"
#include "ha_scan.h"                              // Aff, ha_comb, ha_block_scan, ha_comp_params, HA_THREADS, HA_KMAX, HA_CPT, HA_CT

namespace {
constexpr int HA_FPT = 8;                         // FIR: consecutive outputs per thread
constexpr int HA_FT = HA_THREADS * HA_FPT;        //      outputs per tile
constexpr long HA_NMAX = 1L << 30;

__device__ __forceinline__ int ha_pad(int i) { return i + (i >> 3); }

template <bool ADJ>
__global__ __launch_bounds__(HA_THREADS) void ha_fir_kernel(const float* __restrict__ x, long n_in, long n_out, const float* __restrict__ taps,
                                                            int F, int K, const int* __restrict__ row_set, float* __restrict__ out) {
    // window sample j (j < HA_FT + HP) at ha_pad(j); forward: j <-> x[t0 - HP + j], adjoint: j <-> dout[t0 + j]
    __shared__ float xs[HA_FT + 1024 + (HA_FT + 1024) / 8 + 8];
    __shared__ float hs[HA_KMAX + 7];
    const int HP = (K - 1 + 7) & ~7;
    const long r = blockIdx.y;
    int f = row_set ? row_set[r] : 0;
    f = f < 0 ? 0 : (f >= F ? F - 1 : f);
    const float* h = taps + (long)f * K;
    const float* xr = x + r * n_in;
    float* yr = out + r * n_out;
    const long t0 = (long)blockIdx.x * HA_FT;
    const long base = ADJ ? t0 : t0 - HP;
    for (int j = threadIdx.x; j < HA_FT + HP; j += HA_THREADS) {
        const long i = base + j;
        xs[ha_pad(j)] = (i >= 0 && i < n_in) ? xr[i] : 0.f;
    }
    for (int k = threadIdx.x; k < K; k += HA_THREADS) hs[k] = h[k];
    __syncthreads();
    const int o0 = threadIdx.x * HA_FPT;
    float acc[HA_FPT], w[HA_FPT];
#pragma unroll
    for (int t = 0; t < HA_FPT; ++t) acc[t] = 0.f;
    if (!ADJ) {
        // tap k reads x[m - k] = window[o + HP - k]; window[o0 + HP - k + t] sits in w[(t - k) & 7]
#pragma unroll
        for (int t = 1; t < HA_FPT; ++t) w[t] = xs[ha_pad(o0 + HP + t)];
        for (int k0 = 0; k0 < K; k0 += HA_FPT) {
#pragma unroll
            for (int u = 0; u < HA_FPT; ++u) {
                const int k = k0 + u;
                if (k < K) {                                      // (block-uniform)
                    w[(HA_FPT - u) & (HA_FPT - 1)] = xs[ha_pad(o0 + HP - k)];
                    const float hk = hs[k];
#pragma unroll
                    for (int t = 0; t < HA_FPT; ++t) acc[t] = fmaf(hk, w[(t - u + HA_FPT) & (HA_FPT - 1)], acc[t]);
                }
            }
        }
    } else {
        // tap k reads dout[i + k] = window[o + k]; window[o0 + k + t] sits in w[(t + k) & 7]
#pragma unroll
        for (int t = 0; t < HA_FPT - 1; ++t) w[t] = xs[ha_pad(o0 + t)];
        for (int k0 = 0; k0 < K; k0 += HA_FPT) {
#pragma unroll
            for (int u = 0; u < HA_FPT; ++u) {
                const int k = k0 + u;
                if (k < K) {
                    w[(u + HA_FPT - 1) & (HA_FPT - 1)] = xs[ha_pad(o0 + k + HA_FPT - 1)];
                    const float hk = hs[k];
#pragma unroll
                    for (int t = 0; t < HA_FPT; ++t) acc[t] = fmaf(hk, w[(t + u) & (HA_FPT - 1)], acc[t]);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < HA_FPT; ++t) {
        const long m = t0 + o0 + t;
        if (m < n_out) yr[m] = acc[t];
    }
}

// WRITE = false: tsum[r][t] = sum of z^2 over the tile.  WRITE = true: P[r][i] = tpre[r][t] + (sum of z^2 over the tile up to i).
template <bool WRITE>
__global__ __launch_bounds__(HA_THREADS) void ha_sq_kernel(const float* __restrict__ z, long n, int T, const double* __restrict__ tpre,
                                                           double* __restrict__ dst) {
    __shared__ Aff sh[HA_THREADS / 64];
    const long r = blockIdx.y;
    const int t = blockIdx.x;
    const float* zr = z + r * n;
    const long i0 = (long)t * HA_CT + threadIdx.x * HA_CPT;
    double s[HA_CPT], sum = 0.0;
#pragma unroll
    for (int q = 0; q < HA_CPT; ++q) {
        const double v = i0 + q < n ? (double)zr[i0 + q] : 0.0;
        s[q] = v * v;
        sum += s[q];
    }
    Aff tot;
    const Aff ex = ha_block_scan(Aff{1.0, sum}, sh, &tot);
    if (!WRITE) {
        if (threadIdx.x == 0) dst[r * T + t] = tot.b;
    } else {
        double p = tpre[r * T + t] + ex.b;
#pragma unroll
        for (int q = 0; q < HA_CPT; ++q) {
            p += s[q];
            if (i0 + q < n) dst[r * n + i0 + q] = p;
        }
    }
}

// One workgroup per row: cin[r][0] = init, cin[r][t + 1] = A[r][t] * cin[r][t] + B[r][t]  (A == NULL: all ones, a prefix sum).
__global__ __launch_bounds__(HA_THREADS) void ha_row_scan_kernel(const double* __restrict__ A, const double* __restrict__ B, int T, double init,
                                                                 double* __restrict__ cin) {
    __shared__ Aff sh[HA_THREADS / 64];
    const long r = blockIdx.x;
    double carry = init;                                          // the same value in every thread
    for (int t0 = 0; t0 < T; t0 += HA_THREADS) {
        const int t = t0 + threadIdx.x;
        Aff v = {1.0, 0.0};
        if (t < T) v = Aff{A ? A[r * T + t] : 1.0, B[r * T + t]};
        Aff tot;
        const Aff ex = ha_block_scan(v, sh, &tot);
        if (t < T) cin[r * T + t] = fma(ex.a, carry, ex.b);
        carry = fma(tot.a, carry, tot.b);
    }
}

// FINAL = false: the tile's composition -> aggA / aggB.  FINAL = true: rescan from cin, write gain and out.
template <bool FINAL>
__global__ __launch_bounds__(HA_THREADS) void ha_comp_kernel(const float* __restrict__ z, long n, int T, int W, ha_comp_params p,
                                                             const double* __restrict__ P, double* __restrict__ aggA, double* __restrict__ aggB,
                                                             const double* __restrict__ cin, int soft_clip, float* __restrict__ gain,
                                                             float* __restrict__ out) {
    __shared__ Aff sh[HA_THREADS / 64];
    const long r = blockIdx.y;
    const int t = blockIdx.x;
    const double* Pr = P + r * n;
    const long i0 = (long)t * HA_CT + threadIdx.x * HA_CPT;
    Aff m[HA_CPT], mine = {1.0, 0.0};
#pragma unroll
    for (int q = 0; q < HA_CPT; ++q) {
        const long i = i0 + q;
        m[q] = Aff{1.0, 0.0};
        if (i < n) {
            double ss = Pr[i] - (i >= W ? Pr[i - W] : 0.0);
            ss = ss < 0.0 ? 0.0 : ss;
            const double lv = sqrt(ss * p.inv_w + 1e-8);
            m[q] = lv > p.thr ? Aff{p.a_att, p.attack * fma(lv, p.atten, p.hold)} : Aff{p.a_rel, p.b_rel};
        }
        mine = ha_comb(mine, m[q]);
    }
    Aff tot;
    const Aff ex = ha_block_scan(mine, sh, &tot);
    if (!FINAL) {
        if (threadIdx.x == 0) {
            aggA[r * T + t] = tot.a;
            aggB[r * T + t] = tot.b;
        }
    } else {
        double c = fma(ex.a, cin[r * T + t], ex.b);
        const float* zr = z + r * n;
#pragma unroll
        for (int q = 0; q < HA_CPT; ++q) {
            const long i = i0 + q;
            if (i < n) {
                c = fma(m[q].a, c, m[q].b);
                const float g = (float)c;
                const float y = zr[i] * g;
                gain[r * n + i] = g;
                out[r * n + i] = soft_clip ? tanhf(y) : y;
            }
        }
    }
}

__global__ __launch_bounds__(HA_THREADS) void ha_comp_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                                 const float* __restrict__ gain, long count, int soft_clip,
                                                                 float* __restrict__ dz) {
    for (long i = (long)blockIdx.x * HA_THREADS + threadIdx.x; i < count; i += (long)gridDim.x * HA_THREADS) {
        const float y = out[i];
        const float d = soft_clip ? dout[i] * (1.f - y * y) : dout[i];
        dz[i] = d * gain[i];
    }
}

bool ha_shape_ok(long rows, long n) { return rows >= 1 && rows <= 65535 && n >= 1 && n <= HA_NMAX; }

int ha_fir(bool adj, const float* x, long rows, long n, const float* taps, int F, int K, const int* row_set, float* out, void* stream) {
    const char* name = adj ? "ha_fir_adj" : "ha_fir_fwd";
    SEHIP_REQUIRE(K >= 1 && K <= HA_KMAX, "%s: K=%d outside [1, %d]", name, K, HA_KMAX);
    SEHIP_REQUIRE(F >= 1 && F <= 65535, "%s: F=%d tap sets outside [1, 65535]", name, F);
    SEHIP_REQUIRE(ha_shape_ok(rows, n), "%s: empty or oversized input: rows=%ld (1 .. 65535), n=%ld (1 .. 2^30)", name, rows, n);
    SEHIP_REQUIRE(x && taps && out, "%s: null pointer", name);
    const long n_long = n + K - 1;                                // forward: n -> n + K - 1; adjoint: n + K - 1 -> n
    const long n_in = adj ? n_long : n, n_out = adj ? n : n_long;
    const dim3 grid((unsigned)((n_out + HA_FT - 1) / HA_FT), (unsigned)rows);
    if (adj) ha_fir_kernel<true><<<grid, HA_THREADS, 0, (hipStream_t)stream>>>(x, n_in, n_out, taps, F, K, row_set, out);
    else ha_fir_kernel<false><<<grid, HA_THREADS, 0, (hipStream_t)stream>>>(x, n_in, n_out, taps, F, K, row_set, out);
    SEHIP_CHECK_LAUNCH(name);
    sehip_note_kernel("%s tile=%d K=%d F=%d tiles=%u", name, HA_FT, K, F, grid.x);
    return 0;
}
}  // namespace

extern "C" int sehip_ha_fir_fwd(const float* x, long rows, long n, const float* taps, int F, int K, const int* row_set, float* out, void* stream) {
    return ha_fir(false, x, rows, n, taps, F, K, row_set, out, stream);
}

extern "C" int sehip_ha_fir_adj(const float* dout, long rows, long n, const float* taps, int F, int K, const int* row_set, float* dx,
                                void* stream) {
    return ha_fir(true, dout, rows, n, taps, F, K, row_set, dx, stream);
}

extern "C" long sehip_ha_compressor_ws_doubles(long rows, long n, int W) {
    if (!ha_shape_ok(rows, n) || W < 1) return 0;
    const long T = (n + HA_CT - 1) / HA_CT;
    return rows * n + 5 * rows * T;
}

extern "C" int sehip_ha_compressor_fwd(const float* z, long rows, long n, int W, double threshold, double attack, double release,
                                       double attenuation, int soft_clip, double* ws, float* gain, float* out, void* stream) {
    SEHIP_REQUIRE(ha_shape_ok(rows, n), "ha_compressor_fwd: empty or oversized input: rows=%ld (1 .. 65535), n=%ld (1 .. 2^30)", rows, n);
    SEHIP_REQUIRE(W >= 1, "ha_compressor_fwd: window W=%d < 1 (rms_buffer_size * fs)", W);
    SEHIP_REQUIRE(threshold == threshold && attack == attack && release == release && attenuation == attenuation,
                  "ha_compressor_fwd: a NaN setting");
    SEHIP_REQUIRE(z && ws && gain && out, "ha_compressor_fwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int T = (int)((n + HA_CT - 1) / HA_CT);
    double* P = ws;
    double* tsum = P + rows * n;
    double* tpre = tsum + rows * T;
    double* aggA = tpre + rows * T;
    double* aggB = aggA + rows * T;
    double* cin = aggB + rows * T;
    ha_comp_params p;
    p.thr = threshold;
    p.a_att = 1.0 - attack;
    p.a_rel = 1.0 - release;
    p.b_rel = release;
    p.attack = attack;
    p.atten = attenuation;
    p.hold = (1.0 - attenuation) * threshold;
    p.inv_w = 1.0 / (double)W;
    const dim3 grid((unsigned)T, (unsigned)rows);
    ha_sq_kernel<false><<<grid, HA_THREADS, 0, st>>>(z, n, T, nullptr, tsum);
    SEHIP_CHECK_LAUNCH("ha_compressor_fwd (tile sums)");
    ha_row_scan_kernel<<<(unsigned)rows, HA_THREADS, 0, st>>>(nullptr, tsum, T, 0.0, tpre);
    SEHIP_CHECK_LAUNCH("ha_compressor_fwd (row scan of the sums)");
    ha_sq_kernel<true><<<grid, HA_THREADS, 0, st>>>(z, n, T, tpre, P);
    SEHIP_CHECK_LAUNCH("ha_compressor_fwd (prefix)");
    ha_comp_kernel<false><<<grid, HA_THREADS, 0, st>>>(z, n, T, W, p, P, aggA, aggB, nullptr, soft_clip, nullptr, nullptr);
    SEHIP_CHECK_LAUNCH("ha_compressor_fwd (tile maps)");
    ha_row_scan_kernel<<<(unsigned)rows, HA_THREADS, 0, st>>>(aggA, aggB, T, 1.0, cin);
    SEHIP_CHECK_LAUNCH("ha_compressor_fwd (row scan of the maps)");
    ha_comp_kernel<true><<<grid, HA_THREADS, 0, st>>>(z, n, T, W, p, P, nullptr, nullptr, cin, soft_clip, gain, out);
    SEHIP_CHECK_LAUNCH("ha_compressor_fwd (rescan)");
    sehip_note_kernel("ha_compressor tile=%d W=%d tiles=%d rows=%ld clip=%d", HA_CT, W, T, rows, soft_clip ? 1 : 0);
    return 0;
}

extern "C" int sehip_ha_compressor_bwd(const float* dout, const float* out, const float* gain, long count, int soft_clip, float* dz,
                                       void* stream) {
    SEHIP_REQUIRE(count >= 1, "ha_compressor_bwd: empty input (count=%ld)", count);
    SEHIP_REQUIRE(dout && out && gain && dz, "ha_compressor_bwd: null pointer");
    long blocks = (count + HA_THREADS - 1) / HA_THREADS;
    blocks = blocks > 4096 ? 4096 : blocks;
    ha_comp_bwd_kernel<<<(unsigned)blocks, HA_THREADS, 0, (hipStream_t)stream>>>(dout, out, gain, count, soft_clip, dz);
    SEHIP_CHECK_LAUNCH("ha_compressor_bwd");
    sehip_note_kernel("ha_compressor_bwd blocks=%ld clip=%d", blocks, soft_clip ? 1 : 0);
    return 0;
}
