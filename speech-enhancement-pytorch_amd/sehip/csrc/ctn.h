// ConvTasNet streaming kernels (csrc/tasnet.hip, csrc/tasnet_cln.hip): the 16-byte piece helpers, the thread layout and the launch
// grids they share.  Activations are channels-last bf16 [M][K][C]; a thread owns 8 channels = 16 bytes of a frame.
#pragma once
#include "common.h"

#define CTN_EPS 1e-8f

struct C8 { float v[8]; };
__device__ __forceinline__ C8 ld8(const bf16_raw* p) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    C8 c;
    c.v[0] = bf2f((bf16_raw)(u.x & 0xffff)); c.v[1] = bf2f((bf16_raw)(u.x >> 16));
    c.v[2] = bf2f((bf16_raw)(u.y & 0xffff)); c.v[3] = bf2f((bf16_raw)(u.y >> 16));
    c.v[4] = bf2f((bf16_raw)(u.z & 0xffff)); c.v[5] = bf2f((bf16_raw)(u.z >> 16));
    c.v[6] = bf2f((bf16_raw)(u.w & 0xffff)); c.v[7] = bf2f((bf16_raw)(u.w >> 16));
    return c;
}
__device__ __forceinline__ void st8(bf16_raw* p, const float* v) {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7]));
}
__device__ __forceinline__ uint4 ld8raw(const bf16_raw* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ C8 unpack8(const uint4 u) {
    C8 c;
    c.v[0] = bf2f((bf16_raw)(u.x & 0xffff)); c.v[1] = bf2f((bf16_raw)(u.x >> 16));
    c.v[2] = bf2f((bf16_raw)(u.y & 0xffff)); c.v[3] = bf2f((bf16_raw)(u.y >> 16));
    c.v[4] = bf2f((bf16_raw)(u.z & 0xffff)); c.v[5] = bf2f((bf16_raw)(u.z >> 16));
    c.v[6] = bf2f((bf16_raw)(u.w & 0xffff)); c.v[7] = bf2f((bf16_raw)(u.w >> 16));
    return c;
}
__device__ __forceinline__ C8 zero8() { C8 c; for (int j = 0; j < 8; ++j) c.v[j] = 0.f; return c; }
__device__ __forceinline__ float prelu(float h, float a) { return h > 0.f ? h : a * h; }

// Thread layout of the frame-streaming kernels below: a thread owns ONE piece of 8 channels (q = tid % nq) for all its
// frames, so gamma / beta / the depthwise taps of those channels are loaded once and stay in registers (fetched per piece
// they were 40 four-byte loads beside 3-8 sixteen-byte ones, and the kernels ran at the address unit's pace: 90-260 us for
// 26-MB tensors); rows t = bx*rpb + tid/nq, stepping by gridDim.x*rpb (rpb = 256/nq rows per block pass).
struct PieceMap { int q, c0, rsub, rpb; bool active; };
__device__ __forceinline__ PieceMap piece_map(int nq) {
    PieceMap p;
    p.rpb = 256 / nq;
    p.q = threadIdx.x % nq;
    p.rsub = threadIdx.x / nq;
    p.c0 = p.q * 8;
    p.active = p.rsub < p.rpb;
    return p;
}
__device__ __forceinline__ void ld8f(const float* __restrict__ p, float (&v)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// ---- per-frame (cLN) kernels: csrc/tasnet_cln.hip and the chunked streamer's csrc/tasnet_stream.hip share these, so a frame's
// arithmetic is the same code in both ----
// group of G lanes (a power of two <= 64, aligned) -> the sum over the group in every lane
__device__ __forceinline__ float group_sum(float v, int G) {
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ void group_sum2(float& a, float& b, int G) {
    for (int o = 1; o < G; o <<= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
}

// Thread layout: lane group of G per frame, thread owns piece q = tid % G (idle when q >= nq) of frames bx*rpb + tid/G, stepping by
// gridDim.x*rpb with rpb = 256/G.  The frame loop is uniform over the workgroup (the shuffles run with all lanes on).
struct FrameMap { int q, c0, rsub, rpb, G; bool act; };
__device__ __forceinline__ FrameMap frame_map(int nq) {
    FrameMap f;
    f.G = 1;
    while (f.G < nq) f.G <<= 1;
    f.rpb = 256 / f.G;
    f.q = threadIdx.x & (f.G - 1);
    f.rsub = threadIdx.x / f.G;
    f.act = f.q < nq;
    f.c0 = (f.act ? f.q : 0) * 8;
    return f;
}

// v = PReLU(x) -> centred values d = v - mean and 1/sigma of the frame (idle lanes: x = 0 in, d forced to 0)
__device__ __forceinline__ float cln_center(const C8& x, float a, bool act, int G, float invC, float (&d)[8]) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { d[j] = prelu(x.v[j], a); s += d[j]; }
    const float mean = group_sum(s, G) * invC;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { d[j] = act ? d[j] - mean : 0.f; q += d[j] * d[j]; }
    const float var = group_sum(q, G) * invC;
    return 1.f / sqrtf(var + CTN_EPS);
}

static int ctn_check(const char* who, int M, int K, int C) {
    SEHIP_REQUIRE(M > 0 && K > 0, "%s: empty input", who);
    SEHIP_REQUIRE(C >= 8 && C <= 512 && (C & 7) == 0, "%s: channels C=%d must be a multiple of 8 in [8, 512]", who, C);
    return 0;
}
static dim3 ctn_grid(int M, int K, int C) {
    long pieces = (long)K * (C >> 3);
    // 16-byte pieces per thread (C4 step, ms: 4: 3.82, 6: 3.77, 8: 3.78, 16: 3.82, 32: 4.16; 2: 5.6 -- every workgroup pays the
    // per-channel constants and, in the backward apply pass, its share of the column sums)
    static const int rows = getenv("SEHIP_CTN_ROWS") ? atoi(getenv("SEHIP_CTN_ROWS")) : 6;
    long g = (pieces + 256 * rows - 1) / (256 * rows);
    if (g < 1) g = 1;
    if (g > 64) g = 64;
    return dim3((unsigned)g, (unsigned)M);
}
