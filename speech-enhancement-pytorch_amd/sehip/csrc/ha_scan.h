// What the whole-row compressor (hearing_aid.hip) and the chunked one (ha_stream.hip) share: the float64 affine maps c -> a c + b, their
// composition, the scan of one workgroup's maps and the compressor's settings as the kernels take them.
#pragma once
#include "common.h"

constexpr int HA_THREADS = 256;
constexpr int HA_KMAX = 1025;
constexpr int HA_CPT = 4;                         // compressor: consecutive samples per thread
constexpr int HA_CT = HA_THREADS * HA_CPT;        //             samples per tile

// ---- affine maps c -> a c + b in float64 --------------------------------------------------------------------------------------------
struct Aff {
    double a, b;
};
// g after f
__device__ __forceinline__ Aff ha_comb(Aff f, Aff g) { return Aff{g.a * f.a, fma(g.a, f.b, g.b)}; }

// Scan of the 256 threads' maps in thread order.  Returns the composition of all EARLIER threads (the identity for thread 0); *tot
// gets the composition of all 256.  sh: 4 maps of LDS.
__device__ __forceinline__ Aff ha_block_scan(Aff v, Aff* sh, Aff* tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Aff inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const Aff p = {__shfl_up(inc.a, o, 64), __shfl_up(inc.b, o, 64)};
        if (lane >= o) inc = ha_comb(p, inc);
    }
    Aff ex = {__shfl_up(inc.a, 1, 64), __shfl_up(inc.b, 1, 64)};
    if (lane == 0) ex = Aff{1.0, 0.0};
    __syncthreads();                                              // an earlier scan's readers of sh are done
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    Aff before = {1.0, 0.0}, all = {1.0, 0.0};
#pragma unroll
    for (int q = 0; q < HA_THREADS / 64; ++q) {
        const Aff s = sh[q];
        if (q < wave) before = ha_comb(before, s);
        all = ha_comb(all, s);
    }
    *tot = all;
    return ha_comb(before, ex);
}

struct ha_comp_params {
    double thr, a_att, a_rel, b_rel, attack, atten, hold, inv_w;   // hold = (1 - attenuation) * threshold
};
