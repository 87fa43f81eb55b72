// Counter-based dropout shared by rnn-stft-mask / mel-rnn (csrc/rnnmask.hip) and the U-Net (csrc/unet.hip):
// bits = mix(mix(index ^ key) + golden), key from (seed, step counter, layer).  No mask is stored: forward and backward recompute the
// keep decision from the element's index.  The Python twin is sehip/plan_rnnmask.py (drop_keep_mask).
#pragma once

struct RsmDrop {
    unsigned seed_lo, seed_hi;
    const unsigned* ctr;      // the step counter this forward pass took (device memory; never read on the host)
    int layer;
    unsigned thresh;          // round(p 2^24); an element is kept when its top 24 bits are >= thresh; 0 = no dropout here
    float scale;              // 1 / (1 - p), 0 for p = 1
};
__device__ __forceinline__ unsigned rsm_mix(unsigned x) {
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ unsigned rsm_key(const RsmDrop& d) {
    return rsm_mix(d.seed_lo ^ rsm_mix(d.seed_hi ^ rsm_mix(d.ctr[0] * 0x9e3779b9u + (unsigned)d.layer)));
}
__device__ __forceinline__ bool rsm_keep(unsigned key, unsigned idx, unsigned thresh) {
    return (rsm_mix(rsm_mix(idx ^ key) + 0x9e3779b9u) >> 8) >= thresh;
}
