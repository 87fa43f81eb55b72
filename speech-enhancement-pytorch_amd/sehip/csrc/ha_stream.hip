// The hearing-aid back end (hearing_aid.hip: NAL-R FIR, compressor, tanh) chunk by chunk, for rows that resume from carried state.
//
// State of a row, all on the device:
//     pos   int64   samples fed since the row was fresh (reset: pos = 0)
//     xring fp32 [LX], LX = K - 1 + C   input sample a sits at slot a mod LX
//     zring fp32 [LZ], LZ = W - 1 + C   filtered sample a sits at slot a mod LZ
//     c     float64                     the compressor's gain after sample pos - 1 (reset: c = 1)
//   C = chunk_samples is the largest chunk; a chunk has 1 <= n <= C samples.  A sample index below 0 reads as zero, so a reset
//   clears nothing.  A ring is as long as its history plus one chunk: the n slots a chunk writes (samples pos .. pos + n - 1) are never
//   the slots it reads as history (samples pos - (K - 1) .. pos - 1, pos - (W - 1) .. pos - 1), and nothing is copied to "shift".
//
// A chunk is three launches with the same arguments every time (the position is read on the device: capturable):
//   1 has_fir_kernel    grid (tiles of 2048 outputs, rows): out[m] = sum_k h[k] x[pos + m - k] over [xring history | xin], the same
//                       single fmaf chain over k = 0 .. K - 1 from 0 as ha_fir_kernel: the bits of offline fir_apply on the whole
//                       input.  Writes the chunk into xring, the result into zring and into filt.  Reads xin and xring's history.
//   2 has_comp_kernel   one workgroup per row, walks the chunk in segments of len = min(1024, W, rest) samples.  For sample j0 + l
//                       of a segment starting at chunk sample j0, with V = [W - 1 filtered history | chunk] (chunk sample j is V[W - 1 + j])
//                       the window is V[j0 + l .. j0 + l + W - 1]:
//                           ss = (sum V[j0 + l .. j0 + len - 1]) + (sum V[j0 + len .. j0 + W - 1]) + (sum V[j0 + W .. j0 + l + W - 1])
//                                 suffix scan of the segment      one reduction (mid)              prefix scan of the segment's
//                                 of OUTGOING samples                                              INCOMING samples (the chunk's own)
//                       float64, formed afresh from the stored fp32 samples in a fixed order.  NOTHING but c is accumulated across
//                       chunks: there is no running sum, so the error does not grow with the stream, and every term is >= 0 -- no
//                       difference is taken, a window of exact zeros gives exactly sqrt(1e-8).  Then the affine-map scan of
//                       hearing_aid.hip from the carried c, each thread walking its 4 samples as the reference's loop does.
//                       Reads zring, pos, c; writes gain, out and c_next.
//   3 has_advance_kernel  pos += n, c = c_next (each thread its own words).
// No launch writes an address that it, or a workgroup running beside it, reads (the advance's own words excepted, as the other
// streamers' counters).  No atomics; every sum has one owner and a fixed order: the same bits from run to run.
#include "common.h"
#include "ha_scan.h"

namespace {
constexpr int HAS_FPT = 8;                        // FIR: consecutive outputs per thread (as hearing_aid.hip)
constexpr int HAS_FT = HA_THREADS * HAS_FPT;
constexpr int HAS_WMAX = 1 << 20;
constexpr int HAS_CMAX = 1 << 16;

__device__ __forceinline__ int has_pad(int i) { return i + (i >> 3); }

// slot of sample pos + d in a ring of length L whose slot of sample pos is b0; -L < d < L
__device__ __forceinline__ long has_slot(long b0, long d, long L) {
    long s = b0 + d;
    s = s < 0 ? s + L : s;
    return s >= L ? s - L : s;
}

__global__ __launch_bounds__(HA_THREADS) void has_fir_kernel(const float* __restrict__ xin, int n, int C, const float* __restrict__ taps, int F,
                                                             int K, int W, const int* __restrict__ row_set, const long* __restrict__ pos,
                                                             float* __restrict__ xring, float* __restrict__ zring, float* __restrict__ filt) {
    // window sample j (j < HAS_FT + HP) at has_pad(j), j <-> chunk index t0 - HP + j (negative: history)
    __shared__ float xs[HAS_FT + 1024 + (HAS_FT + 1024) / 8 + 8];
    __shared__ float hs[HA_KMAX + 7];
    const int HP = (K - 1 + 7) & ~7;
    const long r = blockIdx.y;
    int f = row_set ? row_set[r] : 0;
    f = f < 0 ? 0 : (f >= F ? F - 1 : f);
    const float* h = taps + (long)f * K;
    const long LX = K - 1 + C, LZ = W - 1 + C;
    const long p0 = pos[r];
    const long bx = p0 % LX, bz = p0 % LZ;
    const float* xr = xin + r * C;
    float* xg = xring + r * LX;
    const int t0 = blockIdx.x * HAS_FT;
    const int tn = n - t0 < HAS_FT ? n - t0 : HAS_FT;             // outputs of this tile
    for (int j = threadIdx.x; j < tn + HP; j += HA_THREADS) {
        const int i = t0 - HP + j;
        float v = 0.f;
        if (i >= 0) v = xr[i];                                    // (i < t0 + tn <= n)
        else if (-i <= K - 1 && p0 + i >= 0) v = xg[has_slot(bx, i, LX)];
        xs[has_pad(j)] = v;
    }
    for (int j = tn + HP + threadIdx.x; j < tn + HP + HAS_FPT; j += HA_THREADS) xs[has_pad(j)] = 0.f;   // the last thread's register window
    for (int k = threadIdx.x; k < K; k += HA_THREADS) hs[k] = h[k];
    __syncthreads();
    const int o0 = threadIdx.x * HAS_FPT;
    if (o0 >= tn) return;
    float acc[HAS_FPT], w[HAS_FPT];
#pragma unroll
    for (int t = 0; t < HAS_FPT; ++t) acc[t] = 0.f;
    // tap k reads x[m - k] = window[o + HP - k]; window[o0 + HP - k + t] sits in w[(t - k) & 7]
#pragma unroll
    for (int t = 1; t < HAS_FPT; ++t) w[t] = xs[has_pad(o0 + HP + t)];
    for (int k0 = 0; k0 < K; k0 += HAS_FPT) {
#pragma unroll
        for (int u = 0; u < HAS_FPT; ++u) {
            const int k = k0 + u;
            if (k < K) {                                          // (block-uniform)
                w[(HAS_FPT - u) & (HAS_FPT - 1)] = xs[has_pad(o0 + HP - k)];
                const float hk = hs[k];
#pragma unroll
                for (int t = 0; t < HAS_FPT; ++t) acc[t] = fmaf(hk, w[(t - u + HAS_FPT) & (HAS_FPT - 1)], acc[t]);
            }
        }
    }
    float* zg = zring + r * LZ;
#pragma unroll
    for (int t = 0; t < HAS_FPT; ++t) {
        const int m = t0 + o0 + t;
        if (m < n) {
            filt[r * C + m] = acc[t];
            zg[has_slot(bz, m, LZ)] = acc[t];
            xg[has_slot(bx, m, LX)] = xr[m];
        }
    }
}

__global__ __launch_bounds__(HA_THREADS) void has_comp_kernel(const float* __restrict__ zring, int n, int C, int W, const long* __restrict__ pos,
                                                              const double* __restrict__ c_in, ha_comp_params p, int soft_clip,
                                                              double* __restrict__ c_next, float* __restrict__ gain, float* __restrict__ out) {
    __shared__ Aff sh[HA_THREADS / 64];
    __shared__ double suf[HA_CT];
    const long r = blockIdx.x;
    const long LZ = W - 1 + C;
    const float* zr = zring + r * LZ;
    const long p0 = pos[r];
    const long bz = p0 % LZ;
    // z^2 of V[i], i in [0, W - 1 + n): sample p0 - (W - 1) + i
    auto sq = [&](long i) -> double {
        const long d = i - (W - 1);
        if (p0 + d < 0) return 0.0;
        const double z = (double)zr[has_slot(bz, d, LZ)];
        return z * z;
    };
    double carry = c_in[r];                                       // the same value in every thread
    Aff tot;
    for (int j0 = 0; j0 < n;) {
        int len = n - j0 < HA_CT ? n - j0 : HA_CT;
        len = len < W ? len : W;
        // mid: V[j0 + len .. j0 + W - 1], each thread a strided share in rising order, the shares in thread order
        double part = 0.0;
        for (long i = (long)j0 + len + threadIdx.x; i < (long)j0 + W; i += HA_THREADS) part += sq(i);
        ha_block_scan(Aff{1.0, part}, sh, &tot);
        const double mid = tot.b;
        // suffix sums of the outgoing samples V[j0 + l], l < len: a prefix scan in falling l
        {
            double s[HA_CPT], sum = 0.0;
#pragma unroll
            for (int q = 0; q < HA_CPT; ++q) {
                const int l = len - 1 - (threadIdx.x * HA_CPT + q);
                s[q] = l >= 0 ? sq((long)j0 + l) : 0.0;
                sum += s[q];
            }
            double run = ha_block_scan(Aff{1.0, sum}, sh, &tot).b;
#pragma unroll
            for (int q = 0; q < HA_CPT; ++q) {
                const int l = len - 1 - (threadIdx.x * HA_CPT + q);
                run += s[q];
                if (l >= 0) suf[l] = run;
            }
        }
        // prefix sums of the incoming samples V[j0 + W + l - 1], 1 <= l < len (the chunk's samples j0 + 1 .. j0 + l)
        const int l0 = threadIdx.x * HA_CPT;
        double inc[HA_CPT];
        {
            double sum = 0.0;
#pragma unroll
            for (int q = 0; q < HA_CPT; ++q) {
                const int l = l0 + q;
                inc[q] = (l >= 1 && l < len) ? sq((long)j0 + W + l - 1) : 0.0;
                sum += inc[q];
            }
            double run = ha_block_scan(Aff{1.0, sum}, sh, &tot).b;   // (its barriers also publish suf)
#pragma unroll
            for (int q = 0; q < HA_CPT; ++q) {
                run += inc[q];
                inc[q] = run;
            }
        }
        // levels, maps, the scan from the carried c
        Aff m[HA_CPT], mine = {1.0, 0.0};
#pragma unroll
        for (int q = 0; q < HA_CPT; ++q) {
            const int l = l0 + q;
            m[q] = Aff{1.0, 0.0};
            if (l < len) {
                const double ss = (suf[l] + mid) + inc[q];
                const double lv = sqrt(ss * p.inv_w + 1e-8);
                m[q] = lv > p.thr ? Aff{p.a_att, p.attack * fma(lv, p.atten, p.hold)} : Aff{p.a_rel, p.b_rel};
            }
            mine = ha_comb(mine, m[q]);
        }
        const Aff ex = ha_block_scan(mine, sh, &tot);
        double c = fma(ex.a, carry, ex.b);
#pragma unroll
        for (int q = 0; q < HA_CPT; ++q) {
            const int l = l0 + q;
            if (l < len) {
                c = fma(m[q].a, c, m[q].b);
                const float g = (float)c;
                const float y = zr[has_slot(bz, j0 + l, LZ)] * g;
                gain[r * C + j0 + l] = g;
                out[r * C + j0 + l] = soft_clip ? tanhf(y) : y;
            }
        }
        carry = fma(tot.a, carry, tot.b);
        j0 += len;
    }
    if (threadIdx.x == 0) c_next[r] = carry;
}

__global__ __launch_bounds__(HA_THREADS) void has_advance_kernel(long* __restrict__ pos, double* __restrict__ c, const double* __restrict__ c_next,
                                                                 long rows, int n) {
    const long r = (long)blockIdx.x * HA_THREADS + threadIdx.x;
    if (r < rows) {
        pos[r] += n;
        c[r] = c_next[r];
    }
}

int has_check(const char* who, long rows, int n, int C, int K, int W) {
    SEHIP_REQUIRE(rows >= 1 && rows <= 65535, "%s: rows=%ld outside [1, 65535]", who, rows);
    SEHIP_REQUIRE(C >= 1 && C <= HAS_CMAX, "%s: chunk_samples C=%d outside [1, %d]", who, C, HAS_CMAX);
    SEHIP_REQUIRE(n >= 1 && n <= C, "%s: n=%d samples outside [1, chunk_samples = %d]", who, n, C);
    SEHIP_REQUIRE(K >= 1 && K <= HA_KMAX, "%s: K=%d outside [1, %d]", who, K, HA_KMAX);
    SEHIP_REQUIRE(W >= 1 && W <= HAS_WMAX, "%s: window W=%d outside [1, %d]", who, W, HAS_WMAX);
    return 0;
}
}  // namespace

extern "C" long sehip_has_state_bytes(long rows, int K, int W, int C) {
    if (rows < 1 || rows > 65535 || C < 1 || C > HAS_CMAX || K < 1 || K > HA_KMAX || W < 1 || W > HAS_WMAX) return 0;
    return rows * (4L * (K - 1 + C) + 4L * (W - 1 + C) + 8 + 8);
}

extern "C" int sehip_has_fir(const float* xin, long rows, int n, int C, const float* taps, int F, int K, int W, const int* row_set,
                             const long* pos, float* xring, float* zring, float* filt, void* stream) {
    if (int e = has_check("has_fir", rows, n, C, K, W)) return e;
    SEHIP_REQUIRE(F >= 1 && F <= 65535, "has_fir: F=%d tap sets outside [1, 65535]", F);
    SEHIP_REQUIRE(xin && taps && pos && xring && zring && filt, "has_fir: null pointer");
    const dim3 grid((unsigned)((n + HAS_FT - 1) / HAS_FT), (unsigned)rows);
    has_fir_kernel<<<grid, HA_THREADS, 0, (hipStream_t)stream>>>(xin, n, C, taps, F, K, W, row_set, pos, xring, zring, filt);
    SEHIP_CHECK_LAUNCH("has_fir");
    sehip_note_kernel("has_fir tile=%d K=%d F=%d tiles=%u", HAS_FT, K, F, grid.x);
    return 0;
}

extern "C" int sehip_has_compress(const float* zring, long rows, int n, int C, int W, const long* pos, const double* c, double threshold,
                                  double attack, double release, double attenuation, int soft_clip, double* c_next, float* gain, float* out,
                                  void* stream) {
    if (int e = has_check("has_compress", rows, n, C, 1, W)) return e;
    SEHIP_REQUIRE(threshold == threshold && attack == attack && release == release && attenuation == attenuation,
                  "has_compress: a NaN setting");
    SEHIP_REQUIRE(zring && pos && c && c_next && gain && out, "has_compress: null pointer");
    ha_comp_params p;
    p.thr = threshold;
    p.a_att = 1.0 - attack;
    p.a_rel = 1.0 - release;
    p.b_rel = release;
    p.attack = attack;
    p.atten = attenuation;
    p.hold = (1.0 - attenuation) * threshold;
    p.inv_w = 1.0 / (double)W;
    has_comp_kernel<<<(unsigned)rows, HA_THREADS, 0, (hipStream_t)stream>>>(zring, n, C, W, pos, c, p, soft_clip, c_next, gain, out);
    SEHIP_CHECK_LAUNCH("has_compress");
    const int seg = HA_CT < W ? HA_CT : W;
    sehip_note_kernel("has_compress tile=%d W=%d tiles=%d rows=%ld clip=%d", seg, W, (n + seg - 1) / seg, rows, soft_clip ? 1 : 0);
    return 0;
}

extern "C" int sehip_has_advance(long* pos, double* c, const double* c_next, long rows, int n, void* stream) {
    SEHIP_REQUIRE(rows >= 1 && rows <= 65535, "has_advance: rows=%ld outside [1, 65535]", rows);
    SEHIP_REQUIRE(n >= 1 && n <= HAS_CMAX, "has_advance: n=%d samples outside [1, %d]", n, HAS_CMAX);
    SEHIP_REQUIRE(pos && c && c_next, "has_advance: null pointer");
    has_advance_kernel<<<(unsigned)((rows + HA_THREADS - 1) / HA_THREADS), HA_THREADS, 0, (hipStream_t)stream>>>(pos, c, c_next, rows, n);
    SEHIP_CHECK_LAUNCH("has_advance");
    return 0;
}
