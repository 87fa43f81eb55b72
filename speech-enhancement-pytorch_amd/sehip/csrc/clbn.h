// Shared by csrc/wavunet.hip and csrc/unet.hip: the sums of the streaming channels-last kernels and the BatchNorm records made from them.
// A streaming kernel gives thread t of a 256-thread workgroup the 16-byte piece t % (C / 8) of row t / (C / 8) of the workgroup's rows; it
// adds in-thread, clbn_block_partials adds the workgroup's rows in row order through LDS into one row of partials per workgroup, and a
// finalize launch adds the workgroups' rows with one wave per output (clbn_wave_total: lane-strided in double + the fixed shuffle tree).
// No atomics: run-to-run identical.  rbn.h (DCUnet) adds in another order (shuffle tree first) and is therefore not folded in here.
//
// Deliberately NOT here: the streaming kernels themselves (wun_bn_apply / unet_bn_act, the two bwd_reduce, the two bwd_apply).  They
// differ in slope, dropout, where the incoming gradient comes from (wun_dz / unet_dz), index width and unroll pragmas; one template over
// all of that is more machinery than it removes and would change the code generated for the kernels that carry the step time.
#pragma once
#include "common.h"

#define CLBN_MAX_BLOCKS 512

static inline int clbn_rpb(int C) { return 256 / (C >> 3); }
static inline int clbn_blocks(long rows, int C, int per, int cap) {
    long g = (rows + (long)clbn_rpb(C) * per - 1) / ((long)clbn_rpb(C) * per);
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}
// workgroups of a kernel that ends in clbn_block_partials = rows of partials its finalize launch reads
static inline int clbn_sum_blocks(long rows, int C) { return clbn_blocks(rows, C, 8, CLBN_MAX_BLOCKS); }

// the workgroup's rows added in row order: out[k * C + c], k < NS.  lds: 256 * 8 floats.  Threads beyond rpb * nq (C / 8 no divisor of
// 256) hold zeros and are not read.
template <int NS>
__device__ __forceinline__ void clbn_block_partials(const float (&s)[NS][8], int nq, int rpb, int C, float* __restrict__ out, float* lds) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) lds[threadIdx.x * 8 + j] = s[k][j];
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) {
            const int q = c >> 3, j = c & 7;
            float a = 0.f;
            for (int rl = 0; rl < rpb; ++rl) a += lds[(rl * nq + q) * 8 + j];
            out[(size_t)k * C + c] = a;
        }
    }
}

// one wave: sum over the workgroups' rows of part[b * stride + off]
__device__ __forceinline__ double clbn_wave_total(const float* __restrict__ part, int nblk, size_t stride, size_t off) {
    double a = 0.0;
    for (int b = threadIdx.x & 63; b < nblk; b += 64) a += (double)part[(size_t)b * stride + off];
    return wave_sum_d(a);
}

// coef record per channel: scale (gamma rstd), shift (beta - mean scale), mean, rstd.  One wave per channel; part: the two moments about
// the pivot y[c] (the channel's value in row 0).  Channels c >= Cr are padding: their records are zero (z = 0, dy = 0) and no parameter /
// running statistic beyond Cr is touched.
static __global__ void clbn_bn_finalize_kernel(const float* __restrict__ part, int nblk, const bf16_raw* __restrict__ y, const float* __restrict__ gamma,
                                               const float* __restrict__ beta, float* __restrict__ rm, float* __restrict__ rv, long* __restrict__ nbt,
                                               long rows, int C, int Cr, float eps, float momentum, int training, float4* __restrict__ coef) {
    const int c = blockIdx.x;
    if (c >= Cr) {
        if (threadIdx.x == 0) coef[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    double mean, var;
    if (training) {
        const double a0 = clbn_wave_total(part, nblk, (size_t)2 * C, c);
        const double a1 = clbn_wave_total(part, nblk, (size_t)2 * C, (size_t)C + c);
        if (threadIdx.x != 0) return;
        const double n = (double)rows, md = a0 / n;
        var = a1 / n - md * md;
        if (var < 0.0) var = 0.0;
        mean = (double)bf2f(y[c]) + md;
        rm[c] = (float)((1.0 - (double)momentum) * (double)rm[c] + (double)momentum * mean);
        rv[c] = (float)((1.0 - (double)momentum) * (double)rv[c] + (double)momentum * (var * n / (n - 1.0)));   // nn.BatchNorm: UNBIASED
        if (c == 0 && nbt) nbt[0] += 1;
    } else {
        if (threadIdx.x != 0) return;
        mean = (double)rm[c]; var = (double)rv[c];
    }
    const double rstd = 1.0 / sqrt(var + (double)eps);
    const double sc = (double)gamma[c] * rstd;
    coef[c] = make_float4((float)sc, (float)((double)beta[c] - mean * sc), (float)mean, (float)rstd);
}
