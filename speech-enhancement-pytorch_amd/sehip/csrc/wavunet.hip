// Wave-U-Net (src/model/wav_unet.py:8-110): everything around the convolutions' products, on channels-last bf16 activations
// [B][T_l][C_l] (T_l = T / 2^l); the waveform and the network output stay fp32.
//   enc0      Conv1d(1 -> C0, k = 15, pad 7) + bias straight from the fp32 waveform, and its weight / bias gradient
//   bn_*      per-channel BatchNorm1d (batch statistics, biased variance, eps) + LeakyReLU(0.1), forward and backward; the
//             backward's incoming gradient is dz_full[t] + (t even ? dz_even[t / 2] : 0): the `[::2]` decimation's adjoint
//   up2       F.interpolate(scale_factor=2, mode="linear", align_corners=True) fused with the affine + LeakyReLU in front of
//             it (the activated tensor is never stored), and its adjoint as a gather
//   out       tanh(1x1 convolution of cat([o, input])) and its backward
// All of them stream 16-byte pieces (8 bf16 channels per lane): thread t of a 256-thread workgroup owns piece t % (C/8) of row
// t / (C/8) of the workgroup's rows, so a wave reads consecutive addresses and a thread's channels (its coefficients) are fixed.
// Sums: in-thread, then over the workgroup's rows in row order through LDS, one row of partials per workgroup, added by a
// finalize launch (one wave per output: lane-strided in double + the fixed shuffle tree): csrc/clbn.h, shared with csrc/unet.hip.
// No atomics: run-to-run identical.
#include <stdlib.h>
#include "common.h"
#include "rbn.h"
#include "clbn.h"

#define WUN_SLOPE 0.1f
#define WUN_TAPS 15

__device__ __forceinline__ float wun_lrelu(float v) { return v > 0.f ? v : WUN_SLOPE * v; }

// ---------------------------------------------------------------------------------------------------------------------------
// first encoder layer: y0[b][t][c] = bias[c] + sum_k W[c][k] x[b][t + k - 7]
__global__ __launch_bounds__(256) void wun_enc0_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                           const float* __restrict__ bias, int T, int C, bf16_raw* __restrict__ y) {
    const int nq = C >> 3, rpb = 256 / nq;
    const int q = threadIdx.x % nq, rl = threadIdx.x / nq;
    if (rl >= rpb) return;
    float w[WUN_TAPS][8], bs[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        bs[j] = bias[q * 8 + j];
#pragma unroll
        for (int k = 0; k < WUN_TAPS; ++k) w[k][j] = W[(q * 8 + j) * WUN_TAPS + k];
    }
    const float* xb = x + (size_t)blockIdx.y * T;
    bf16_raw* yb = y + (size_t)blockIdx.y * T * C;
    for (int t = blockIdx.x * rpb + rl; t < T; t += gridDim.x * rpb) {
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = bs[j];
#pragma unroll
        for (int k = 0; k < WUN_TAPS; ++k) {
            const int u = t + k - WUN_TAPS / 2;
            const float xv = (u >= 0 && u < T) ? xb[u] : 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] += w[k][j] * xv;
        }
        *reinterpret_cast<uint4*>(yb + (size_t)t * C + q * 8) = r_pack8(o);
    }
}

// partial rows [gridDim.y * gridDim.x][16][C]: k < 15 the taps' sums, k = 15 the bias's
__global__ __launch_bounds__(256) void wun_enc0_wgrad_kernel(const bf16_raw* __restrict__ dy, const float* __restrict__ x, int T, int C,
                                                             float* __restrict__ part) {
    __shared__ float lds[256 * 8];
    const int nq = C >> 3, rpb = 256 / nq;
    const int q = threadIdx.x % nq, rl = threadIdx.x / nq;
    float s[WUN_TAPS + 1][8];
#pragma unroll
    for (int k = 0; k <= WUN_TAPS; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) s[k][j] = 0.f;
    const float* xb = x + (size_t)blockIdx.y * T;
    const bf16_raw* gb = dy + (size_t)blockIdx.y * T * C;
    if (rl < rpb)
        for (int t = blockIdx.x * rpb + rl; t < T; t += gridDim.x * rpb) {
            const RChunk8 g = r_unpack8(*reinterpret_cast<const uint4*>(gb + (size_t)t * C + q * 8));
#pragma unroll
            for (int k = 0; k < WUN_TAPS; ++k) {
                const int u = t + k - WUN_TAPS / 2;
                const float xv = (u >= 0 && u < T) ? xb[u] : 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) s[k][j] += g.v[j] * xv;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) s[WUN_TAPS][j] += g.v[j];
        }
    const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    clbn_block_partials<WUN_TAPS + 1>(s, nq, rpb, C, part + blk * (WUN_TAPS + 1) * C, lds);
}

// one wave per (k, c): dW[c][k] (k < 15), db[c] (k = 15)
__global__ void wun_enc0_wgrad_finalize_kernel(const float* __restrict__ part, int nblk, int C, float* __restrict__ dW, float* __restrict__ db) {
    const int k = blockIdx.x / C, c = blockIdx.x - k * C;
    const double a = clbn_wave_total(part, nblk, (size_t)(WUN_TAPS + 1) * C, (size_t)k * C + c);
    if (threadIdx.x != 0) return;
    if (k < WUN_TAPS) dW[c * WUN_TAPS + k] = (float)a;
    else db[c] = (float)a;
}

// ---------------------------------------------------------------------------------------------------------------------------
// batch moments about a pivot (the channel's value in row 0, which every workgroup reads): sum (y - p), sum (y - p)^2.  A channel
// whose mean is far above its deviation keeps its variance: the sums are of deviations as large as the deviation itself.
__global__ __launch_bounds__(256) void wun_bn_stats_kernel(const bf16_raw* __restrict__ y, long rows, int C, float* __restrict__ part) {
    __shared__ float lds[256 * 8];
    const int nq = C >> 3, rpb = 256 / nq;
    const int q = threadIdx.x % nq, rl = threadIdx.x / nq;
    float s[2][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s[0][j] = 0.f; s[1][j] = 0.f; }
    if (rl < rpb) {
        const RChunk8 p = r_unpack8(*reinterpret_cast<const uint4*>(y + q * 8));
        const long stride = (long)gridDim.x * rpb;
#pragma unroll 4
        for (long r = (long)blockIdx.x * rpb + rl; r < rows; r += stride) {
            const RChunk8 a = r_unpack8(*reinterpret_cast<const uint4*>(y + r * C + q * 8));
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = a.v[j] - p.v[j];
                s[0][j] += d; s[1][j] += d * d;
            }
        }
    }
    clbn_block_partials<2>(s, nq, rpb, C, part + (size_t)blockIdx.x * 2 * C, lds);
}

__global__ __launch_bounds__(256) void wun_bn_apply_kernel(const bf16_raw* __restrict__ y, const float4* __restrict__ coef, long rows, int C,
                                                           bf16_raw* __restrict__ z) {
    const int nq = C >> 3, rpb = 256 / nq;
    const int q = threadIdx.x % nq, rl = threadIdx.x / nq;
    if (rl >= rpb) return;
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float4 k = coef[q * 8 + j]; sc[j] = k.x; sh[j] = k.y; }
    const long stride = (long)gridDim.x * rpb;
#pragma unroll 4
    for (long r = (long)blockIdx.x * rpb + rl; r < rows; r += stride) {
        const RChunk8 a = r_unpack8(*reinterpret_cast<const uint4*>(y + r * C + q * 8));
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = wun_lrelu(sc[j] * a.v[j] + sh[j]);
        *reinterpret_cast<uint4*>(z + r * C + q * 8) = r_pack8(o);
    }
}

// source frame and weight of output position p of the align-corners x2 interpolation, in integers:
// p (Tin - 1) = i0 (2 Tin - 1) + rem, weight of the right neighbour rem / (2 Tin - 1)
__device__ __forceinline__ void wun_up2_src(int p, int Tin, bool small, int& i0, float& w) {
    const unsigned den = 2u * (unsigned)Tin - 1u;
    unsigned rem;
    if (small) {
        const unsigned num = (unsigned)p * (unsigned)(Tin - 1);
        i0 = (int)(num / den); rem = num - (unsigned)i0 * den;
    } else {
        const unsigned long long num = (unsigned long long)p * (unsigned long long)(Tin - 1);
        i0 = (int)(num / den); rem = (unsigned)(num - (unsigned long long)i0 * den);
    }
    w = (float)rem / (float)den;
}

// up[b][p][c] = (1 - w) z[i0] + w z[min(i0 + 1, Tin - 1)],  z = LeakyReLU(scale y + shift) in fp32
__global__ __launch_bounds__(256) void wun_bn_apply_up2_kernel(const bf16_raw* __restrict__ y, const float4* __restrict__ coef, int Tin, int C,
                                                               bf16_raw* __restrict__ up) {
    const int nq = C >> 3, rpb = 256 / nq;
    const int q = threadIdx.x % nq, rl = threadIdx.x / nq;
    if (rl >= rpb) return;
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float4 k = coef[q * 8 + j]; sc[j] = k.x; sh[j] = k.y; }
    const bool small = (unsigned long long)(2 * (long)Tin) * (unsigned long long)(Tin - 1) < (1ull << 32);
    const bf16_raw* yb = y + (size_t)blockIdx.y * Tin * C + q * 8;
    bf16_raw* ub = up + (size_t)blockIdx.y * 2 * Tin * C + q * 8;
    for (int p = blockIdx.x * rpb + rl; p < 2 * Tin; p += gridDim.x * rpb) {
        int i0; float w;
        wun_up2_src(p, Tin, small, i0, w);
        const int i1 = i0 + 1 < Tin ? i0 + 1 : Tin - 1;
        const RChunk8 a = r_unpack8(*reinterpret_cast<const uint4*>(yb + (size_t)i0 * C));
        const RChunk8 b = r_unpack8(*reinterpret_cast<const uint4*>(yb + (size_t)i1 * C));
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            o[j] = (1.f - w) * wun_lrelu(sc[j] * a.v[j] + sh[j]) + w * wun_lrelu(sc[j] * b.v[j] + sh[j]);
        *reinterpret_cast<uint4*>(ub + (size_t)p * C) = r_pack8(o);
    }
}

// adjoint as a gather: source frame i is touched by output positions 2 i - 2 .. 2 i + 2 only (p / 2 - 1 / 2 <= p (Tin - 1) / (2 Tin - 1) <= p / 2)
__global__ __launch_bounds__(256) void wun_up2_bwd_kernel(const bf16_raw* __restrict__ dup, int Tin, int C, bf16_raw* __restrict__ dz) {
    const int nq = C >> 3, rpb = 256 / nq;
    const int q = threadIdx.x % nq, rl = threadIdx.x / nq;
    if (rl >= rpb) return;
    const bool small = (unsigned long long)(2 * (long)Tin) * (unsigned long long)(Tin - 1) < (1ull << 32);
    const bf16_raw* gb = dup + (size_t)blockIdx.y * 2 * Tin * C + q * 8;
    bf16_raw* ob = dz + (size_t)blockIdx.y * Tin * C + q * 8;
    for (int i = blockIdx.x * rpb + rl; i < Tin; i += gridDim.x * rpb) {
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = 0.f;
#pragma unroll
        for (int d = -2; d <= 2; ++d) {
            const int p = 2 * i + d;
            if (p < 0 || p >= 2 * Tin) continue;
            int i0; float w;
            wun_up2_src(p, Tin, small, i0, w);
            const int i1 = i0 + 1 < Tin ? i0 + 1 : Tin - 1;
            float wt = 0.f;
            if (i0 == i) wt += 1.f - w;
            if (i1 == i) wt += w;
            if (wt == 0.f) continue;
            const RChunk8 g = r_unpack8(*reinterpret_cast<const uint4*>(gb + (size_t)p * C));
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] += wt * g.v[j];
        }
        *reinterpret_cast<uint4*>(ob + (size_t)i * C) = r_pack8(o);
    }
}

// incoming gradient of row r: dz_full[r] + (r even ? dz_even[r / 2] : 0) (every utterance has an even number of frames when
// dz_even is given, so the parity of the row is the parity of the frame and row r / 2 is frame t / 2 of the same utterance)
__device__ __forceinline__ RChunk8 wun_dz(const bf16_raw* __restrict__ dzf, const bf16_raw* __restrict__ dze, long r, int C, int q) {
    RChunk8 g = r_unpack8(*reinterpret_cast<const uint4*>(dzf + r * C + q * 8));
    if (dze && !(r & 1)) {
        const RChunk8 e = r_unpack8(*reinterpret_cast<const uint4*>(dze + (r >> 1) * C + q * 8));
#pragma unroll
        for (int j = 0; j < 8; ++j) g.v[j] += e.v[j];
    }
    return g;
}

// backward pass 1: g = dz * LeakyReLU'(scale y + shift); per channel sum g, sum g xh (xh = (y - mean) rstd)
__global__ __launch_bounds__(256) void wun_bn_bwd_reduce_kernel(const bf16_raw* __restrict__ dzf, const bf16_raw* __restrict__ dze,
                                                                const bf16_raw* __restrict__ y, const float4* __restrict__ coef, long rows,
                                                                int C, float* __restrict__ part) {
    __shared__ float lds[256 * 8];
    const int nq = C >> 3, rpb = 256 / nq;
    const int q = threadIdx.x % nq, rl = threadIdx.x / nq;
    float s[2][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s[0][j] = 0.f; s[1][j] = 0.f; }
    if (rl < rpb) {
        float4 k[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) k[j] = coef[q * 8 + j];
        const long stride = (long)gridDim.x * rpb;
#pragma unroll 2
        for (long r = (long)blockIdx.x * rpb + rl; r < rows; r += stride) {
            const RChunk8 a = r_unpack8(*reinterpret_cast<const uint4*>(y + r * C + q * 8));
            const RChunk8 g = wun_dz(dzf, dze, r, C, q);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float o = k[j].x * a.v[j] + k[j].y;
                const float gg = o > 0.f ? g.v[j] : WUN_SLOPE * g.v[j];
                s[0][j] += gg;
                s[1][j] += gg * (a.v[j] - k[j].z) * k[j].w;
            }
        }
    }
    clbn_block_partials<2>(s, nq, rpb, C, part + (size_t)blockIdx.x * 2 * C, lds);
}

// bcoef record per channel: gamma rstd, mean(g), mean(g xh)
__global__ void wun_bn_bwd_finalize_kernel(const float* __restrict__ part, int nblk, const float4* __restrict__ coef, long rows, int C,
                                           float* __restrict__ dgamma, float* __restrict__ dbeta, float4* __restrict__ bcoef) {
    const int c = blockIdx.x;
    const double a0 = clbn_wave_total(part, nblk, (size_t)2 * C, c);
    const double a1 = clbn_wave_total(part, nblk, (size_t)2 * C, (size_t)C + c);
    if (threadIdx.x != 0) return;
    dbeta[c] = (float)a0;
    dgamma[c] = (float)a1;
    const double n = (double)rows;
    bcoef[c] = make_float4(coef[c].x, (float)(a0 / n), (float)(a1 / n), 0.f);
}

// backward pass 2: dy = gamma rstd (g - mean(g) - xh mean(g xh))
__global__ __launch_bounds__(256) void wun_bn_bwd_apply_kernel(const bf16_raw* __restrict__ dzf, const bf16_raw* __restrict__ dze,
                                                               const bf16_raw* __restrict__ y, const float4* __restrict__ coef,
                                                               const float4* __restrict__ bcoef, long rows, int C, bf16_raw* __restrict__ dy) {
    const int nq = C >> 3, rpb = 256 / nq;
    const int q = threadIdx.x % nq, rl = threadIdx.x / nq;
    if (rl >= rpb) return;
    float4 k[8], kb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { k[j] = coef[q * 8 + j]; kb[j] = bcoef[q * 8 + j]; }
    const long stride = (long)gridDim.x * rpb;
#pragma unroll 2
    for (long r = (long)blockIdx.x * rpb + rl; r < rows; r += stride) {
        const RChunk8 a = r_unpack8(*reinterpret_cast<const uint4*>(y + r * C + q * 8));
        const RChunk8 g = wun_dz(dzf, dze, r, C, q);
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = k[j].x * a.v[j] + k[j].y;
            const float gg = v > 0.f ? g.v[j] : WUN_SLOPE * g.v[j];
            const float xh = (a.v[j] - k[j].z) * k[j].w;
            o[j] = kb[j].x * (gg - kb[j].y - xh * kb[j].z);
        }
        *reinterpret_cast<uint4*>(dy + r * C + q * 8) = r_pack8(o);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// head: out[r] = tanh(sum_c W[c] z[r][c] + W[C] x[r] + b); one thread per row (the weights are wave-uniform loads)
__global__ __launch_bounds__(256) void wun_out_fwd_kernel(const bf16_raw* __restrict__ z, const float* __restrict__ x, const float* __restrict__ W,
                                                          const float* __restrict__ bias, long rows, int C, float* __restrict__ out) {
    const int nq = C >> 3;
    const long stride = (long)gridDim.x * 256;
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < rows; r += stride) {
        float a = bias[0] + W[C] * x[r];
        for (int q = 0; q < nq; ++q) {
            const RChunk8 v = r_unpack8(*reinterpret_cast<const uint4*>(z + r * C + q * 8));
#pragma unroll
            for (int j = 0; j < 8; ++j) a += W[q * 8 + j] * v.v[j];
        }
        out[r] = tanhf(a);
    }
}

// dpre = dout (1 - out^2); dz[r][c] = dpre W[c]; partial rows [nblk][2][C]: slot 0 sum dpre z[r][c], slot 1 [0] sum dpre x[r], [1] sum dpre
__global__ __launch_bounds__(256) void wun_out_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ out, const bf16_raw* __restrict__ z,
                                                          const float* __restrict__ x, const float* __restrict__ W, long rows, int C,
                                                          bf16_raw* __restrict__ dz, float* __restrict__ part) {
    __shared__ float lds[256 * 8];
    const int nq = C >> 3, rpb = 256 / nq;
    const int q = threadIdx.x % nq, rl = threadIdx.x / nq;
    float s[2][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s[0][j] = 0.f; s[1][j] = 0.f; }
    if (rl < rpb) {
        float w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = W[q * 8 + j];
        const long stride = (long)gridDim.x * rpb;
#pragma unroll 2
        for (long r = (long)blockIdx.x * rpb + rl; r < rows; r += stride) {
            const float o = out[r];
            const float dp = dout[r] * (1.f - o * o);
            const RChunk8 v = r_unpack8(*reinterpret_cast<const uint4*>(z + r * C + q * 8));
            float g[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { g[j] = dp * w[j]; s[0][j] += dp * v.v[j]; }
            *reinterpret_cast<uint4*>(dz + r * C + q * 8) = r_pack8(g);
            if (q == 0) { s[1][0] += dp * x[r]; s[1][1] += dp; }
        }
    }
    clbn_block_partials<2>(s, nq, rpb, C, part + (size_t)blockIdx.x * 2 * C, lds);
}

// one wave per output: dW[0 .. C) | dW[C] (the waveform's weight) | db
__global__ void wun_out_bwd_finalize_kernel(const float* __restrict__ part, int nblk, int C, float* __restrict__ dW, float* __restrict__ db) {
    const int c = blockIdx.x;
    const size_t off = c < C ? (size_t)c : (size_t)C + (c - C);
    const double a = clbn_wave_total(part, nblk, (size_t)2 * C, off);
    if (threadIdx.x != 0) return;
    if (c <= C) dW[c] = (float)a;
    else db[0] = (float)a;
}

// ---------------------------------------------------------------------------------------------------------------------------
static int check_wun(const char* who, long rows, int C) {
    SEHIP_REQUIRE(C >= 8 && C <= 2048 && C % 8 == 0, "%s: C=%d must be a multiple of 8 in [8, 2048]", who, C);
    SEHIP_REQUIRE(rows >= 1 && rows < (1L << 40), "%s: rows=%ld out of range", who, rows);
    return 0;
}
static int check_bt(const char* who, int B, int T) {
    SEHIP_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d must be in [1, 65535]", who, B);
    SEHIP_REQUIRE(T >= 1 && T <= (1 << 28), "%s: T=%d out of range", who, T);
    return 0;
}

extern "C" long sehip_wun_bn_scratch_floats(long rows, int C) {
    if (C < 8 || C > 2048 || C % 8 || rows < 1) return 0;
    return (long)clbn_sum_blocks(rows, C) * 2L * C;
}
static inline int wun_enc0_wg_blocks(int T, int C) { return clbn_blocks(T, C, 16, 16); }
extern "C" long sehip_wun_enc0_wgrad_scratch_floats(int B, int T, int C0) {
    if (C0 < 8 || C0 > 2048 || C0 % 8 || B < 1 || T < 1) return 0;
    return (long)B * wun_enc0_wg_blocks(T, C0) * (WUN_TAPS + 1L) * C0;
}
extern "C" long sehip_wun_out_bwd_scratch_floats(long rows, int C0) { return sehip_wun_bn_scratch_floats(rows, C0); }

extern "C" int sehip_wun_enc0_fwd(const float* x, const float* W, const float* bias, int B, int T, int C0, void* y0, void* stream) {
    if (int e = check_wun("wun_enc0_fwd", (long)B * T, C0)) return e;
    if (int e = check_bt("wun_enc0_fwd", B, T)) return e;
    SEHIP_REQUIRE(x && W && bias && y0, "wun_enc0_fwd: null pointer");
    wun_enc0_fwd_kernel<<<dim3(clbn_blocks(T, C0, 4, 2048), B), 256, 0, (hipStream_t)stream>>>(x, W, bias, T, C0, (bf16_raw*)y0);
    SEHIP_CHECK_LAUNCH("wun_enc0_fwd");
    return 0;
}

extern "C" int sehip_wun_enc0_wgrad(const void* dy0, const float* x, int B, int T, int C0, float* dW, float* db, float* scratch, void* stream) {
    if (int e = check_wun("wun_enc0_wgrad", (long)B * T, C0)) return e;
    if (int e = check_bt("wun_enc0_wgrad", B, T)) return e;
    SEHIP_REQUIRE(dy0 && x && dW && db && scratch, "wun_enc0_wgrad: null pointer");
    const int nbx = wun_enc0_wg_blocks(T, C0);
    wun_enc0_wgrad_kernel<<<dim3(nbx, B), 256, 0, (hipStream_t)stream>>>((const bf16_raw*)dy0, x, T, C0, scratch);
    SEHIP_CHECK_LAUNCH("wun_enc0_wgrad");
    wun_enc0_wgrad_finalize_kernel<<<(WUN_TAPS + 1) * C0, 64, 0, (hipStream_t)stream>>>(scratch, nbx * B, C0, dW, db);
    SEHIP_CHECK_LAUNCH("wun_enc0_wgrad_finalize");
    return 0;
}

extern "C" int sehip_wun_bn_stats(const void* y, long rows, int C, float* part, void* stream) {
    if (int e = check_wun("wun_bn_stats", rows, C)) return e;
    SEHIP_REQUIRE(rows > 1, "wun_bn_stats: BatchNorm needs more than one value per channel (rows=%ld)", rows);
    SEHIP_REQUIRE(y && part, "wun_bn_stats: null pointer");
    wun_bn_stats_kernel<<<clbn_sum_blocks(rows, C), 256, 0, (hipStream_t)stream>>>((const bf16_raw*)y, rows, C, part);
    SEHIP_CHECK_LAUNCH("wun_bn_stats");
    return 0;
}

extern "C" int sehip_wun_bn_finalize(const float* part, const void* y, const float* gamma, const float* beta, float* running_mean,
                                     float* running_var, long* num_batches_tracked, long rows, int C, float eps, float momentum,
                                     int training, float* coef, void* stream) {
    if (int e = check_wun("wun_bn_finalize", rows, C)) return e;
    SEHIP_REQUIRE(gamma && beta && running_mean && running_var && coef, "wun_bn_finalize: null pointer");
    SEHIP_REQUIRE(!training || (part && y && rows > 1), "wun_bn_finalize: training needs the partial sums, y and more than one row");
    clbn_bn_finalize_kernel<<<C, 64, 0, (hipStream_t)stream>>>(part, clbn_sum_blocks(rows, C), (const bf16_raw*)y, gamma, beta, running_mean,
                                                             running_var, num_batches_tracked, rows, C, C, eps, momentum, training, (float4*)coef);
    SEHIP_CHECK_LAUNCH("wun_bn_finalize");
    return 0;
}

extern "C" int sehip_wun_bn_apply(const void* y, const float* coef, long rows, int C, void* z, void* stream) {
    if (int e = check_wun("wun_bn_apply", rows, C)) return e;
    SEHIP_REQUIRE(y && coef && z, "wun_bn_apply: null pointer");
    wun_bn_apply_kernel<<<clbn_blocks(rows, C, 4, 4096), 256, 0, (hipStream_t)stream>>>((const bf16_raw*)y, (const float4*)coef, rows, C, (bf16_raw*)z);
    SEHIP_CHECK_LAUNCH("wun_bn_apply");
    return 0;
}

extern "C" int sehip_wun_bn_apply_up2(const void* y, const float* coef, int B, int Tin, int C, void* up, void* stream) {
    if (int e = check_wun("wun_bn_apply_up2", (long)B * Tin, C)) return e;
    if (int e = check_bt("wun_bn_apply_up2", B, Tin)) return e;
    SEHIP_REQUIRE(Tin >= 2, "wun_bn_apply_up2: the interpolation needs at least two source frames (Tin=%d)", Tin);
    SEHIP_REQUIRE(y && coef && up, "wun_bn_apply_up2: null pointer");
    wun_bn_apply_up2_kernel<<<dim3(clbn_blocks(2L * Tin, C, 4, 2048), B), 256, 0, (hipStream_t)stream>>>((const bf16_raw*)y, (const float4*)coef, Tin,
                                                                                                      C, (bf16_raw*)up);
    SEHIP_CHECK_LAUNCH("wun_bn_apply_up2");
    return 0;
}

extern "C" int sehip_wun_up2_bwd(const void* dup, int B, int Tin, int C, void* dz, void* stream) {
    if (int e = check_wun("wun_up2_bwd", (long)B * Tin, C)) return e;
    if (int e = check_bt("wun_up2_bwd", B, Tin)) return e;
    SEHIP_REQUIRE(Tin >= 2, "wun_up2_bwd: the interpolation needs at least two source frames (Tin=%d)", Tin);
    SEHIP_REQUIRE(dup && dz, "wun_up2_bwd: null pointer");
    wun_up2_bwd_kernel<<<dim3(clbn_blocks(Tin, C, 4, 2048), B), 256, 0, (hipStream_t)stream>>>((const bf16_raw*)dup, Tin, C, (bf16_raw*)dz);
    SEHIP_CHECK_LAUNCH("wun_up2_bwd");
    return 0;
}

extern "C" int sehip_wun_bn_bwd_reduce(const void* dz_full, const void* dz_even, const void* y, const float* coef, long rows, int C,
                                       float* part, void* stream) {
    if (int e = check_wun("wun_bn_bwd_reduce", rows, C)) return e;
    SEHIP_REQUIRE(dz_full && y && coef && part, "wun_bn_bwd_reduce: null pointer");
    SEHIP_REQUIRE(!dz_even || rows % 2 == 0, "wun_bn_bwd_reduce: dz_even needs an even number of frames per utterance (rows=%ld)", rows);
    wun_bn_bwd_reduce_kernel<<<clbn_sum_blocks(rows, C), 256, 0, (hipStream_t)stream>>>((const bf16_raw*)dz_full, (const bf16_raw*)dz_even,
                                                                                     (const bf16_raw*)y, (const float4*)coef, rows, C, part);
    SEHIP_CHECK_LAUNCH("wun_bn_bwd_reduce");
    return 0;
}

extern "C" int sehip_wun_bn_bwd_finalize(const float* part, const float* coef, long rows, int C, float* dgamma, float* dbeta, float* bcoef,
                                         void* stream) {
    if (int e = check_wun("wun_bn_bwd_finalize", rows, C)) return e;
    SEHIP_REQUIRE(part && coef && dgamma && dbeta && bcoef, "wun_bn_bwd_finalize: null pointer");
    wun_bn_bwd_finalize_kernel<<<C, 64, 0, (hipStream_t)stream>>>(part, clbn_sum_blocks(rows, C), (const float4*)coef, rows, C, dgamma, dbeta,
                                                                (float4*)bcoef);
    SEHIP_CHECK_LAUNCH("wun_bn_bwd_finalize");
    return 0;
}

extern "C" int sehip_wun_bn_bwd_apply(const void* dz_full, const void* dz_even, const void* y, const float* coef, const float* bcoef, long rows,
                                      int C, void* dy, void* stream) {
    if (int e = check_wun("wun_bn_bwd_apply", rows, C)) return e;
    SEHIP_REQUIRE(dz_full && y && coef && bcoef && dy, "wun_bn_bwd_apply: null pointer");
    SEHIP_REQUIRE(!dz_even || rows % 2 == 0, "wun_bn_bwd_apply: dz_even needs an even number of frames per utterance (rows=%ld)", rows);
    wun_bn_bwd_apply_kernel<<<clbn_blocks(rows, C, 4, 4096), 256, 0, (hipStream_t)stream>>>(
        (const bf16_raw*)dz_full, (const bf16_raw*)dz_even, (const bf16_raw*)y, (const float4*)coef, (const float4*)bcoef, rows, C, (bf16_raw*)dy);
    SEHIP_CHECK_LAUNCH("wun_bn_bwd_apply");
    return 0;
}

extern "C" int sehip_wun_out_fwd(const void* z, const float* x, const float* W, const float* bias, long rows, int C0, float* out, void* stream) {
    if (int e = check_wun("wun_out_fwd", rows, C0)) return e;
    SEHIP_REQUIRE(z && x && W && bias && out, "wun_out_fwd: null pointer");
    long g = (rows + 255) / 256;
    if (g > 8192) g = 8192;
    wun_out_fwd_kernel<<<(int)g, 256, 0, (hipStream_t)stream>>>((const bf16_raw*)z, x, W, bias, rows, C0, out);
    SEHIP_CHECK_LAUNCH("wun_out_fwd");
    return 0;
}

extern "C" int sehip_wun_out_bwd(const float* dout, const float* out, const void* z, const float* x, const float* W, long rows, int C0, void* dz,
                                 float* dW, float* db, float* scratch, void* stream) {
    if (int e = check_wun("wun_out_bwd", rows, C0)) return e;
    SEHIP_REQUIRE(dout && out && z && x && W && dz && dW && db && scratch, "wun_out_bwd: null pointer");
    const int nblk = clbn_sum_blocks(rows, C0);
    wun_out_bwd_kernel<<<nblk, 256, 0, (hipStream_t)stream>>>(dout, out, (const bf16_raw*)z, x, W, rows, C0, (bf16_raw*)dz, scratch);
    SEHIP_CHECK_LAUNCH("wun_out_bwd");
    wun_out_bwd_finalize_kernel<<<C0 + 2, 64, 0, (hipStream_t)stream>>>(scratch, nblk, C0, dW, db);
    SEHIP_CHECK_LAUNCH("wun_out_bwd_finalize");
    return 0;
}
