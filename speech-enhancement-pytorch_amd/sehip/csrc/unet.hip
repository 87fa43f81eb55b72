// U-Net on the power spectrogram (src/model/unet.py:9-146; `unet` of the registry): everything around the convolutions' products, on
// channels-last bf16 activations [R][T_l][F_l][C] (frames T, rows per frame F, both halved by floor per level); the spectrum, the
// network output and the incoming gradient stay fp32 [R][uc][F][T][2].
//   features     amp = re^2 + im^2 as bf16 [R][T][F][Cp] (Cp = uc rounded up to 8, padding channels exact zeros): the (F, T)
//                transposition through an LDS tile
//   bn_finalize  sehip_wun_bn_finalize (the same kernel, csrc/clbn.h) for a tensor whose last C - Cr channels are padding: their
//                records are zero (z = 0, dy = 0) and no parameter / running statistic beyond Cr is touched
//   bn_act       z = drop(LeakyReLU_0.01(scale y + shift)) at full resolution
//   bn_act_pool  the same followed by MaxPool2d(2) in one pass: the activated full-resolution tensor is never stored.  Writes the
//                pooled z and a 2-bit argmax code per output (8 channels = one 16-bit word): code = 2 (F offset) + (T offset), ties to
//                the first element in the reference's scan order (F offset outer, T offset inner).  An odd last row / column belongs to
//                no window.
//   bn_bwd_*     BatchNorm + LeakyReLU + dropout backward; the incoming gradient is full-resolution dz, or (pooled form) dpool with
//                the argmax code: the coded element takes the gradient, the other three and an odd last row / column exact zero
//   mask_fwd     out = spec * LeakyReLU_0.01(BN(y_head)), transposed back to [F][T]
//   mask_bwd     dm = dout_re spec_re + dout_im spec_im as bf16 [R][T][F][Cp]
// The streaming kernels have csrc/wavunet.hip's form: thread t of a 256-thread workgroup owns the 16-byte piece t % (C / 8) of row
// t / (C / 8) of the workgroup's rows, its channels' coefficients stay in registers.  Sums: clbn_block_partials' fixed order (csrc/clbn.h), one row
// of partials per workgroup, added by sehip_wun_bn_bwd_finalize.  No atomics.  Dropout: csrc/drop.h, the keep decision is recomputed
// from the element's index in the full-resolution tensor, forward and backward.
#include <stdlib.h>
#include "common.h"
#include "rbn.h"
#include "clbn.h"
#include "drop.h"

#define UNET_SLOPE 0.01f
#define UNET_TILE 32

namespace {

__device__ __forceinline__ float unet_lrelu(float v) { return v > 0.f ? v : UNET_SLOPE * v; }

// ---- spectrum -> channels-last bf16 ----------------------------------------------------------------------------------------------------
// MODE 0: re^2 + im^2 of spec; MODE 1: dout_re spec_re + dout_im spec_im.  grid (T tiles, F tiles, R * Cp / 8): one group of 8 channels
template <int MODE>
__global__ __launch_bounds__(256) void unet_gather_kernel(const float2* __restrict__ spec, const float2* __restrict__ dout, int uc, int F, int T,
                                                          int Cp, bf16_raw* __restrict__ dst) {
    __shared__ float tile[8][UNET_TILE][UNET_TILE + 1];
    const int ng = Cp >> 3;
    const int r = blockIdx.z / ng, c0 = (blockIdx.z - r * ng) * 8;
    const int t0 = blockIdx.x * UNET_TILE, f0 = blockIdx.y * UNET_TILE;
    const int a = threadIdx.x & 31, b = threadIdx.x >> 5;
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = f0 + b + 8 * i, t = t0 + a;
            float v = 0.f;
            if (c0 + c < uc && f < F && t < T) {
                const size_t o = (((size_t)r * uc + c0 + c) * F + f) * T + t;
                const float2 z = spec[o];
                if (MODE == 0) v = z.x * z.x + z.y * z.y;
                else { const float2 g = dout[o]; v = g.x * z.x + g.y * z.y; }
            }
            tile[c][b + 8 * i][a] = v;
        }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = threadIdx.x + 256 * i;
        const int tt = p >> 5, ff = p & 31;
        const int t = t0 + tt, f = f0 + ff;
        if (t < T && f < F) {
            float o[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) o[c] = tile[c][ff][tt];
            *reinterpret_cast<uint4*>(dst + (((size_t)r * T + t) * F + f) * Cp + c0) = r_pack8(o);
        }
    }
}

// out[r][c][f][t] = spec[r][c][f][t] * LeakyReLU(scale_c y[r][t][f][c] + shift_c)
__global__ __launch_bounds__(256) void unet_mask_fwd_kernel(const bf16_raw* __restrict__ y, const float4* __restrict__ coef,
                                                            const float2* __restrict__ spec, int uc, int F, int T, int Cp, float2* __restrict__ out) {
    __shared__ float tile[8][UNET_TILE][UNET_TILE + 1];
    const int ng = Cp >> 3;
    const int r = blockIdx.z / ng, c0 = (blockIdx.z - r * ng) * 8;
    const int t0 = blockIdx.x * UNET_TILE, f0 = blockIdx.y * UNET_TILE;
    const int a = threadIdx.x & 31, b = threadIdx.x >> 5;
    float sc[8], sh[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { const float4 k = coef[c0 + c]; sc[c] = k.x; sh[c] = k.y; }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = threadIdx.x + 256 * i;
        const int tt = p >> 5, ff = p & 31;
        const int t = t0 + tt, f = f0 + ff;
        if (t < T && f < F) {
            const RChunk8 v = r_unpack8(*reinterpret_cast<const uint4*>(y + (((size_t)r * T + t) * F + f) * Cp + c0));
#pragma unroll
            for (int c = 0; c < 8; ++c) tile[c][ff][tt] = unet_lrelu(sc[c] * v.v[c] + sh[c]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = f0 + b + 8 * i, t = t0 + a;
            if (c0 + c < uc && f < F && t < T) {
                const size_t o = (((size_t)r * uc + c0 + c) * F + f) * T + t;
                const float2 z = spec[o];
                const float m = tile[c][b + 8 * i][a];
                out[o] = make_float2(z.x * m, z.y * m);
            }
        }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float unet_drop(float v, unsigned key, unsigned idx, const RsmDrop& dp) {
    return rsm_keep(key, idx, dp.thresh) ? v * dp.scale : 0.f;
}

__global__ __launch_bounds__(256) void unet_bn_act_kernel(const bf16_raw* __restrict__ y, const float4* __restrict__ coef, unsigned rows, int C,
                                                          RsmDrop dp, bf16_raw* __restrict__ z) {
    const int nq = C >> 3, rpb = 256 / nq;
    const int q = threadIdx.x % nq, rl = threadIdx.x / nq;
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float4 k = coef[q * 8 + j]; sc[j] = k.x; sh[j] = k.y; }
    const unsigned key = dp.thresh ? rsm_key(dp) : 0u;
    const unsigned stride = gridDim.x * rpb;
    for (unsigned r = blockIdx.x * rpb + rl; r < rows; r += stride) {
        const size_t o = (size_t)r * C + q * 8;
        const RChunk8 a = r_unpack8(*reinterpret_cast<const uint4*>(y + o));
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[j] = unet_lrelu(sc[j] * a.v[j] + sh[j]);
            if (dp.thresh) v[j] = unet_drop(v[j], key, (unsigned)o + j, dp);
        }
        *reinterpret_cast<uint4*>(z + o) = r_pack8(v);
    }
}

// rows2 = R T2 F2 output rows.  Candidate k = 2 df + dt of output (n, t2, f2) is full-resolution row (n T + 2 t2 + dt) F + 2 f2 + df.
// a later candidate replaces the best only when it is strictly greater; where two kept candidates round to the same fp32 value the
// order of their y decides (the map y -> z is monotone with the sign of scale), so the code is the exact arithmetic's.
__global__ __launch_bounds__(256) void unet_bn_act_pool_kernel(const bf16_raw* __restrict__ y, const float4* __restrict__ coef, unsigned rows2, int T,
                                                               int F, int C, RsmDrop dp, bf16_raw* __restrict__ zp, unsigned short* __restrict__ code) {
    const int nq = C >> 3, rpb = 256 / nq;
    const int q = threadIdx.x % nq, rl = threadIdx.x / nq;
    const unsigned T2 = (unsigned)T >> 1, F2 = (unsigned)F >> 1;
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float4 k = coef[q * 8 + j]; sc[j] = k.x; sh[j] = k.y; }
    const unsigned key = dp.thresh ? rsm_key(dp) : 0u;
    const unsigned stride = gridDim.x * rpb;
    for (unsigned ro = blockIdx.x * rpb + rl; ro < rows2; ro += stride) {
        const unsigned f2 = ro % F2, nt = ro / F2;
        const unsigned t2 = nt % T2, n = nt / T2;
        const unsigned base = (n * (unsigned)T + 2u * t2) * (unsigned)F + 2u * f2;
        float best[8], by[8];
        bool bk[8];
        unsigned cd = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned row = base + (k & 1) * (unsigned)F + (k >> 1);
            const size_t o = (size_t)row * C + q * 8;
            const RChunk8 a = r_unpack8(*reinterpret_cast<const uint4*>(y + o));
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float v = unet_lrelu(sc[j] * a.v[j] + sh[j]);
                bool keep = true;
                if (dp.thresh) { keep = rsm_keep(key, (unsigned)o + j, dp.thresh); v = keep ? v * dp.scale : 0.f; }
                if (k == 0) { best[j] = v; by[j] = a.v[j]; bk[j] = keep; }
                else {
                    const bool ybeats = sc[j] > 0.f ? a.v[j] > by[j] : (sc[j] < 0.f ? a.v[j] < by[j] : false);
                    if (v > best[j] || (v == best[j] && keep && bk[j] && ybeats)) {
                        best[j] = v; by[j] = a.v[j]; bk[j] = keep;
                        cd = (cd & ~(3u << (2 * j))) | ((unsigned)k << (2 * j));
                    }
                }
            }
        }
        *reinterpret_cast<uint4*>(zp + (size_t)ro * C + q * 8) = r_pack8(best);
        code[(size_t)ro * nq + q] = (unsigned short)cd;
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------
// gradient that arrives at the activation's output in full-resolution row r, before dropout: dz[r], or the pooled gradient routed by
// the argmax code
__device__ __forceinline__ RChunk8 unet_dz(const bf16_raw* __restrict__ dz, const unsigned short* __restrict__ code, unsigned r, int T, int F, int C,
                                           int nq, int q) {
    if (!code) return r_unpack8(*reinterpret_cast<const uint4*>(dz + (size_t)r * C + q * 8));
    const unsigned f = r % (unsigned)F, nt = r / (unsigned)F;
    const unsigned t = nt % (unsigned)T, n = nt / (unsigned)T;
    const unsigned T2 = (unsigned)T >> 1, F2 = (unsigned)F >> 1;
    RChunk8 g;
    if ((t >> 1) >= T2 || (f >> 1) >= F2) {
#pragma unroll
        for (int j = 0; j < 8; ++j) g.v[j] = 0.f;
        return g;
    }
    const size_t ro = ((size_t)n * T2 + (t >> 1)) * F2 + (f >> 1);
    g = r_unpack8(*reinterpret_cast<const uint4*>(dz + ro * C + q * 8));
    const unsigned cd = code[ro * nq + q], mine = 2u * (f & 1u) + (t & 1u);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (((cd >> (2 * j)) & 3u) != mine) g.v[j] = 0.f;
    return g;
}

// pass 1: g = drop'(dz) LeakyReLU'(scale y + shift); per channel sum g, sum g xh
__global__ __launch_bounds__(256) void unet_bn_bwd_reduce_kernel(const bf16_raw* __restrict__ dz, const unsigned short* __restrict__ code,
                                                                 const bf16_raw* __restrict__ y, const float4* __restrict__ coef, unsigned rows, int T,
                                                                 int F, int C, RsmDrop dp, float* __restrict__ part) {
    __shared__ float lds[256 * 8];
    const int nq = C >> 3, rpb = 256 / nq;
    const int q = threadIdx.x % nq, rl = threadIdx.x / nq;
    float s[2][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s[0][j] = 0.f; s[1][j] = 0.f; }
    float4 k[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) k[j] = coef[q * 8 + j];
    const unsigned key = dp.thresh ? rsm_key(dp) : 0u;
    const unsigned stride = gridDim.x * rpb;
    for (unsigned r = blockIdx.x * rpb + rl; r < rows; r += stride) {
        const size_t o = (size_t)r * C + q * 8;
        const RChunk8 a = r_unpack8(*reinterpret_cast<const uint4*>(y + o));
        const RChunk8 g = unet_dz(dz, code, r, T, F, C, nq, q);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float gg = g.v[j];
            if (dp.thresh) gg = unet_drop(gg, key, (unsigned)o + j, dp);
            if (!(k[j].x * a.v[j] + k[j].y > 0.f)) gg *= UNET_SLOPE;
            s[0][j] += gg;
            s[1][j] += gg * (a.v[j] - k[j].z) * k[j].w;
        }
    }
    clbn_block_partials<2>(s, nq, rpb, C, part + (size_t)blockIdx.x * 2 * C, lds);
}

// pass 2: dy = gamma rstd (g - mean(g) - xh mean(g xh))
__global__ __launch_bounds__(256) void unet_bn_bwd_apply_kernel(const bf16_raw* __restrict__ dz, const unsigned short* __restrict__ code,
                                                                const bf16_raw* __restrict__ y, const float4* __restrict__ coef,
                                                                const float4* __restrict__ bcoef, unsigned rows, int T, int F, int C, RsmDrop dp,
                                                                bf16_raw* __restrict__ dy) {
    const int nq = C >> 3, rpb = 256 / nq;
    const int q = threadIdx.x % nq, rl = threadIdx.x / nq;
    float4 k[8], kb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { k[j] = coef[q * 8 + j]; kb[j] = bcoef[q * 8 + j]; }
    const unsigned key = dp.thresh ? rsm_key(dp) : 0u;
    const unsigned stride = gridDim.x * rpb;
    for (unsigned r = blockIdx.x * rpb + rl; r < rows; r += stride) {
        const size_t o = (size_t)r * C + q * 8;
        const RChunk8 a = r_unpack8(*reinterpret_cast<const uint4*>(y + o));
        const RChunk8 g = unet_dz(dz, code, r, T, F, C, nq, q);
        float out[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float gg = g.v[j];
            if (dp.thresh) gg = unet_drop(gg, key, (unsigned)o + j, dp);
            if (!(k[j].x * a.v[j] + k[j].y > 0.f)) gg *= UNET_SLOPE;
            const float xh = (a.v[j] - k[j].z) * k[j].w;
            out[j] = kb[j].x * (gg - kb[j].y - xh * kb[j].z);
        }
        *reinterpret_cast<uint4*>(dy + o) = r_pack8(out);
    }
}

RsmDrop unet_make_drop(unsigned seed_lo, unsigned seed_hi, const void* ctr, int layer, unsigned thresh, float scale) {
    RsmDrop d;
    d.seed_lo = seed_lo; d.seed_hi = seed_hi; d.ctr = (const unsigned*)ctr; d.layer = layer; d.thresh = thresh; d.scale = scale;
    return d;
}

}  // namespace

// C a power-of-two multiple of 8 (every thread of a workgroup owns one piece column), at most 2^32 elements (the dropout index)
static int check_unet(const char* who, long R, int T, int F, int C) {
    SEHIP_REQUIRE(C >= 8 && C <= 2048 && (C & (C - 1)) == 0, "%s: C=%d must be a power of two in [8, 2048]", who, C);
    SEHIP_REQUIRE(R >= 1 && T >= 1 && F >= 1, "%s: R=%ld T=%d F=%d must be positive", who, R, T, F);
    SEHIP_REQUIRE((double)R * T * F * C <= 4294967296.0, "%s: a tensor of R=%ld x T=%d x F=%d x C=%d has more than 2^32 elements", who, R, T, F, C);
    return 0;
}
static int check_spec(const char* who, int R, int uc, int F, int T, int Cp) {
    SEHIP_REQUIRE(R >= 1 && uc >= 1 && F >= 1 && T >= 1, "%s: R=%d uc=%d F=%d T=%d must be positive", who, R, uc, F, T);
    SEHIP_REQUIRE(Cp % 8 == 0 && Cp >= uc && Cp - uc < 8, "%s: Cp=%d must be uc=%d rounded up to a multiple of 8", who, Cp, uc);
    SEHIP_REQUIRE((long)R * (Cp / 8) <= 65535 && (F + UNET_TILE - 1) / UNET_TILE <= 65535, "%s: R=%d F=%d exceed the grid", who, R, F);
    SEHIP_REQUIRE((double)R * T * F * Cp <= 4294967296.0, "%s: more than 2^32 elements", who);
    return 0;
}
static int check_drop(const char* who, const void* ctr, unsigned thresh) {
    SEHIP_REQUIRE(thresh <= (1u << 24), "%s: dropout threshold %u above 2^24", who, thresh);
    SEHIP_REQUIRE(!thresh || ctr, "%s: dropout needs the step counter", who);
    return 0;
}

extern "C" int sehip_unet_features(const float* spec, int R, int uc, int F, int T, int Cp, void* amp, void* stream) {
    if (int e = check_spec("unet_features", R, uc, F, T, Cp)) return e;
    SEHIP_REQUIRE(spec && amp, "unet_features: null pointer");
    unet_gather_kernel<0><<<dim3(cdiv(T, UNET_TILE), cdiv(F, UNET_TILE), R * (Cp / 8)), 256, 0, (hipStream_t)stream>>>(
        (const float2*)spec, nullptr, uc, F, T, Cp, (bf16_raw*)amp);
    SEHIP_CHECK_LAUNCH("unet_features");
    return 0;
}

extern "C" int sehip_unet_mask_bwd(const float* dout, const float* spec, int R, int uc, int F, int T, int Cp, void* dm, void* stream) {
    if (int e = check_spec("unet_mask_bwd", R, uc, F, T, Cp)) return e;
    SEHIP_REQUIRE(dout && spec && dm, "unet_mask_bwd: null pointer");
    unet_gather_kernel<1><<<dim3(cdiv(T, UNET_TILE), cdiv(F, UNET_TILE), R * (Cp / 8)), 256, 0, (hipStream_t)stream>>>(
        (const float2*)spec, (const float2*)dout, uc, F, T, Cp, (bf16_raw*)dm);
    SEHIP_CHECK_LAUNCH("unet_mask_bwd");
    return 0;
}

extern "C" int sehip_unet_mask_fwd(const void* y, const float* coef, const float* spec, int R, int uc, int F, int T, int Cp, float* out,
                                   void* stream) {
    if (int e = check_spec("unet_mask_fwd", R, uc, F, T, Cp)) return e;
    SEHIP_REQUIRE(y && coef && spec && out, "unet_mask_fwd: null pointer");
    unet_mask_fwd_kernel<<<dim3(cdiv(T, UNET_TILE), cdiv(F, UNET_TILE), R * (Cp / 8)), 256, 0, (hipStream_t)stream>>>(
        (const bf16_raw*)y, (const float4*)coef, (const float2*)spec, uc, F, T, Cp, (float2*)out);
    SEHIP_CHECK_LAUNCH("unet_mask_fwd");
    return 0;
}

extern "C" int sehip_unet_bn_finalize(const float* part, const void* y, const float* gamma, const float* beta, float* running_mean,
                                      float* running_var, long* num_batches_tracked, long rows, int C, int Cr, float eps, float momentum,
                                      int training, float* coef, void* stream) {
    if (int e = check_unet("unet_bn_finalize", rows, 1, 1, C)) return e;
    SEHIP_REQUIRE(Cr >= 1 && Cr <= C, "unet_bn_finalize: Cr=%d must be in [1, C=%d]", Cr, C);
    SEHIP_REQUIRE(gamma && beta && running_mean && running_var && coef, "unet_bn_finalize: null pointer");
    SEHIP_REQUIRE(!training || (part && y && rows > 1), "unet_bn_finalize: training needs the partial sums, y and more than one row");
    const int nblk = clbn_sum_blocks(rows, C);      // the rows sehip_wun_bn_stats wrote
    clbn_bn_finalize_kernel<<<C, 64, 0, (hipStream_t)stream>>>(part, nblk, (const bf16_raw*)y, gamma, beta, running_mean, running_var,
                                                             num_batches_tracked, rows, C, Cr, eps, momentum, training, (float4*)coef);
    SEHIP_CHECK_LAUNCH("unet_bn_finalize");
    return 0;
}

extern "C" int sehip_unet_bn_act(const void* y, const float* coef, long rows, int C, unsigned seed_lo, unsigned seed_hi, const void* ctr, int layer,
                                 unsigned thresh, float scale, void* z, void* stream) {
    if (int e = check_unet("unet_bn_act", rows, 1, 1, C)) return e;
    if (int e = check_drop("unet_bn_act", ctr, thresh)) return e;
    SEHIP_REQUIRE(y && coef && z, "unet_bn_act: null pointer");
    unet_bn_act_kernel<<<clbn_blocks(rows, C, 4, 4096), 256, 0, (hipStream_t)stream>>>(
        (const bf16_raw*)y, (const float4*)coef, (unsigned)rows, C, unet_make_drop(seed_lo, seed_hi, ctr, layer, thresh, scale), (bf16_raw*)z);
    SEHIP_CHECK_LAUNCH("unet_bn_act");
    return 0;
}

extern "C" int sehip_unet_bn_act_pool(const void* y, const float* coef, int R, int T, int F, int C, unsigned seed_lo, unsigned seed_hi,
                                      const void* ctr, int layer, unsigned thresh, float scale, void* zp, void* code, void* stream) {
    if (int e = check_unet("unet_bn_act_pool", R, T, F, C)) return e;
    if (int e = check_drop("unet_bn_act_pool", ctr, thresh)) return e;
    SEHIP_REQUIRE(T >= 2 && F >= 2, "unet_bn_act_pool: T=%d and F=%d must be at least 2 (one pooling window)", T, F);
    SEHIP_REQUIRE(y && coef && zp && code, "unet_bn_act_pool: null pointer");
    const long rows2 = (long)R * (T / 2) * (F / 2);
    unet_bn_act_pool_kernel<<<clbn_blocks(rows2, C, 2, 4096), 256, 0, (hipStream_t)stream>>>(
        (const bf16_raw*)y, (const float4*)coef, (unsigned)rows2, T, F, C, unet_make_drop(seed_lo, seed_hi, ctr, layer, thresh, scale),
        (bf16_raw*)zp, (unsigned short*)code);
    SEHIP_CHECK_LAUNCH("unet_bn_act_pool");
    return 0;
}

// dz: full-resolution [R][T][F][C] (code == NULL) or pooled [R][T/2][F/2][C] with code [R][T/2][F/2][C/8] 16-bit words.
// part: sehip_wun_bn_scratch_floats(R T F, C) floats, read by sehip_wun_bn_bwd_finalize(part, coef, R T F, C, ...)
extern "C" int sehip_unet_bn_bwd_reduce(const void* dz, const void* code, const void* y, const float* coef, int R, int T, int F, int C,
                                        unsigned seed_lo, unsigned seed_hi, const void* ctr, int layer, unsigned thresh, float scale, float* part,
                                        void* stream) {
    if (int e = check_unet("unet_bn_bwd_reduce", R, T, F, C)) return e;
    if (int e = check_drop("unet_bn_bwd_reduce", ctr, thresh)) return e;
    SEHIP_REQUIRE(!code || (T >= 2 && F >= 2), "unet_bn_bwd_reduce: the pooled form needs T=%d and F=%d of at least 2", T, F);
    SEHIP_REQUIRE(dz && y && coef && part, "unet_bn_bwd_reduce: null pointer");
    const long rows = (long)R * T * F;
    const int nblk = clbn_sum_blocks(rows, C);
    unet_bn_bwd_reduce_kernel<<<nblk, 256, 0, (hipStream_t)stream>>>((const bf16_raw*)dz, (const unsigned short*)code, (const bf16_raw*)y,
                                                                   (const float4*)coef, (unsigned)rows, T, F, C,
                                                                   unet_make_drop(seed_lo, seed_hi, ctr, layer, thresh, scale), part);
    SEHIP_CHECK_LAUNCH("unet_bn_bwd_reduce");
    return 0;
}

extern "C" int sehip_unet_bn_bwd_apply(const void* dz, const void* code, const void* y, const float* coef, const float* bcoef, int R, int T, int F,
                                       int C, unsigned seed_lo, unsigned seed_hi, const void* ctr, int layer, unsigned thresh, float scale, void* dy,
                                       void* stream) {
    if (int e = check_unet("unet_bn_bwd_apply", R, T, F, C)) return e;
    if (int e = check_drop("unet_bn_bwd_apply", ctr, thresh)) return e;
    SEHIP_REQUIRE(!code || (T >= 2 && F >= 2), "unet_bn_bwd_apply: the pooled form needs T=%d and F=%d of at least 2", T, F);
    SEHIP_REQUIRE(dz && y && coef && bcoef && dy, "unet_bn_bwd_apply: null pointer");
    const long rows = (long)R * T * F;
    unet_bn_bwd_apply_kernel<<<clbn_blocks(rows, C, 4, 4096), 256, 0, (hipStream_t)stream>>>(
        (const bf16_raw*)dz, (const unsigned short*)code, (const bf16_raw*)y, (const float4*)coef, (const float4*)bcoef, (unsigned)rows, T, F, C,
        unet_make_drop(seed_lo, seed_hi, ctr, layer, thresh, scale), (bf16_raw*)dy);
    SEHIP_CHECK_LAUNCH("unet_bn_bwd_apply");
    return 0;
}
