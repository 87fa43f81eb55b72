// ConvTasNet with causal=True, norm_type='cLN' run chunk by chunk (sehip/model/conv_tasnet_stream.py: ConvTasNetStreamer) -- the
// kernels that carry state from one chunk to the next.  S independent streams, Kc frames per call from Kc h new samples per stream
// (h = L/2); the 1x1 products, sehip_ctn_cln_apply and sehip_ctn_mask_softmax_fwd run as they are, on [S][Kc][C] buffers.
//
//   ctns_encoder   carry | chunk ((Kc + 1) h samples) -> mixture_w fp32 [S][Kc][N] and cLN(mixture_w) bf16, the new carry
//   ctns_dwconv    h2[i] = sum_j Wd[j] n1[i - (P - 1 - j) d],  n1 = cLN(PReLU(h1)) over history | chunk, the new history
//   ctns_decoder   mask * mixture_w, basis, overlap-add with the carried tail: Kc h samples per stream and source, the new tail
//   ctns_advance   pos[s] += Kc for every stream, phase ^= 1
//
// Frame indices.  pos[s] (int32, device) is the global index of the first frame of the coming call; it starts at -1: that frame is
// built from the zero carry, is computed like any other (shapes never change) and contributes nothing -- a depthwise tap whose global
// frame index is below 0 is ABSENT (as in ctn_cln_dwconv_fwd_kernel<P, true>, which skips taps before frame 0; it is not
// cLN(PReLU(0)) = beta), and the decoder adds nothing for a frame with a negative index.  A reset stream (pos = -1) therefore needs no
// clearing of its depthwise history: every row of it has a negative index.
//
// The history hazard, and what is done about it.  Frame i of a chunk reads the rows i - (P - 1 - j) d; the oldest of them is the row
// frame i RETIRES, and frames i' < i of the same launch still read it: an in-place ring of exactly (P - 1) d rows is a race, and so is
// any launch that moves the retained rows inside one buffer while other workgroups read them.  Chosen here: EVERY piece of state that
// a launch both reads and renews (input carry, depthwise history, decoder tail) exists twice, [2][...], and ONE int32 word in device
// memory, `phase`, says which half is current.  A launch reads half `phase` and the chunk, and writes half `phase ^ 1` -- no address is
// both read and written inside a launch, whatever the order of workgroups, so there is nothing to synchronise.  ctns_advance flips the
// word at the end of the chunk.  The halves are chosen on the device, so the launches of a chunk have the same arguments every time: a
// chunk is capturable, and the products write plain dense [S][Kc][H] rows (the dense-row kernels of the engine stay available) instead
// of a window of a longer buffer.  The new history is the last (P - 1) d rows of history | chunk, copied as raw 16-byte pieces.
//
// Arithmetic.  ctns_dwconv is ctn_cln_dwconv_fwd_kernel<P, true> (csrc/tasnet_cln.hip) frame by frame: the same lane groups, the
// moments of every tap row recomputed inside the group, the variance from centred values (cln_center, ctn.h) -- a frame's result does
// not depend on which workgroup or lane computes it, so it is the offline row bit for bit.  ctns_encoder is the wave-per-frame
// ctn_encoder_fwd_kernel (csrc/tasnet.hip) statement by statement; ctns_decoder its ctn_decoder_fwd_kernel's serial dot products,
// every output sample stored ONCE as upper half of frame i - 1 (or the tail) + lower half of frame i: no atomics, no clearing.  (At
// N = 128 with one audio channel the offline entry points take their split-bf16 MFMA kernels, ~2^-16 from these fp32 sums.)
#include "common.h"
#include "ctn.h"

#define CTNS_MAXC 8        // channels per lane of the wave-per-frame kernels: N <= 64 * 8

template <int MC>
__global__ __launch_bounds__(256) void ctns_encoder_kernel(const float* __restrict__ x /*[S][ac][Kc*h]*/, float* __restrict__ carry /*[2][S][ac][h]*/,
                                                           const int* __restrict__ phase, const float* __restrict__ U /*[N][ac*L]*/,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, int S, int ac,
                                                           int Kc, int N, int L, float* __restrict__ w, bf16_raw* __restrict__ cln) {
    extern __shared__ float sU[];                    // [ac*L][N]
    const int AL = ac * L;
    for (int i = threadIdx.x; i < N * AL; i += 256) { const int n = i / AL, l = i - n * AL; sU[l * N + n] = U[i]; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int step = L / 2, ph = phase[0] & 1;
    const float* cur = carry + (long)ph * S * ac * step;
    float* nxt = carry + (long)(ph ^ 1) * S * ac * step;
    const long frames = (long)S * Kc;
    for (long fr = (long)blockIdx.x * 4 + wave; fr < frames; fr += (long)gridDim.x * 4) {
        const int m = (int)(fr / Kc), k = (int)(fr - (long)m * Kc);
        float acc[MC];
#pragma unroll
        for (int i = 0; i < MC; ++i) acc[i] = 0.f;
        for (int a = 0; a < ac; ++a) {
            const float* xc = x + ((long)m * ac + a) * Kc * step;      // sample l of frame k is chunk sample (k - 1) step + l ...
            const float* xo = cur + ((long)m * ac + a) * step;         // ... or, for the first step samples of frame 0, the carry
            const long c0 = (long)(k - 1) * step;
            for (int l = 0; l < L; ++l) {
                const float xv = (k == 0 && l < step) ? xo[l] : xc[c0 + l];
#pragma unroll
                for (int i = 0; i < MC; ++i) {
                    const int n = lane + 64 * i;
                    if (n < N) acc[i] += xv * sU[(a * L + l) * N + n];
                }
            }
        }
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int i = 0; i < MC; ++i) {
            acc[i] = acc[i] > 0.f ? acc[i] : 0.f;
            if (lane + 64 * i < N) { s += acc[i]; q += acc[i] * acc[i]; }
        }
        s = wave_sum(s); q = wave_sum(q);
        const float mean = s / N;
        float var = q / N - mean * mean;
        var = var > 0.f ? var : 0.f;
        const float rs = 1.f / sqrtf(var + CTN_EPS);
#pragma unroll
        for (int i = 0; i < MC; ++i) {
            const int n = lane + 64 * i;
            if (n < N) {
                w[fr * N + n] = acc[i];
                cln[fr * N + n] = f2bf(gamma[n] * (acc[i] - mean) * rs + beta[n]);
            }
        }
        if (k == Kc - 1) {          // the last step samples of the chunk are the first half of the next call's frame 0
            for (int o = lane; o < ac * step; o += 64) {
                const int a = o / step, l = o - a * step;
                nxt[((long)m * ac + a) * step + l] = x[((long)m * ac + a) * Kc * step + (long)(Kc - 1) * step + l];
            }
        }
    }
}

template <int P>
__global__ __launch_bounds__(256) void ctns_dwconv_kernel(const bf16_raw* __restrict__ h1 /*[S][Kc][C]*/, bf16_raw* __restrict__ hist /*[2][S][(P-1)d][C]*/,
                                                          const int* __restrict__ phase, const int* __restrict__ pos,
                                                          const float* __restrict__ slope1, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const float* __restrict__ Wd /*[C][P]*/, int dil,
                                                          int Kc, int C, bf16_raw* __restrict__ h2 /*[S][Kc][C]*/) {
    const int m = blockIdx.y, S = gridDim.y, nq = C >> 3, HR = (P - 1) * dil;
    const FrameMap fm = frame_map(nq);
    const float a1 = slope1[0], invC = 1.f / (float)C;
    const int ph = phase[0] & 1, p0 = pos[m];
    const bf16_raw* cur = hist + ((long)ph * S + m) * HR * C + fm.c0;
    bf16_raw* nxt = hist + ((long)(ph ^ 1) * S + m) * HR * C + fm.c0;
    const bf16_raw* chunk = h1 + (long)m * Kc * C + fm.c0;
    bf16_raw* out = h2 + (long)m * Kc * C + fm.c0;
    float gm[8], bt[8], wd[P][8];
    ld8f(gamma + fm.c0, gm); ld8f(beta + fm.c0, bt);
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int p = 0; p < P; ++p) wd[p][j] = Wd[(fm.c0 + j) * P + p];
    for (int t0 = blockIdx.x * fm.rpb; t0 < Kc; t0 += gridDim.x * fm.rpb) {
        const int t = t0 + fm.rsub;
        const bool ok = fm.act && t < Kc;
        C8 x[P];
        bool tap[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {          // all loads in flight together
            const int r = t + p * dil;         // row of history | chunk: frame t is row HR + t, tap p lies (P - 1 - p) d before it
            tap[p] = p0 + t - (P - 1 - p) * dil >= 0;
            x[p] = (ok && tap[p]) ? ld8(r < HR ? cur + (long)r * C : chunk + (long)(r - HR) * C) : zero8();
        }
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = 0.f;
#pragma unroll
        for (int p = 0; p < P; ++p) {          // (the moments of every tap row, needed or not: the shuffles stay uniform)
            float d[8];
            const float rs = cln_center(x[p], a1, fm.act, fm.G, invC, d);
            if (tap[p]) {
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] += wd[p][j] * (gm[j] * (d[j] * rs) + bt[j]);
            }
        }
        if (ok) st8(out + (long)t * C, o);
    }
    // the other half's history: the last HR rows of history | chunk
    for (int j0 = blockIdx.x * fm.rpb; j0 < HR; j0 += gridDim.x * fm.rpb) {
        const int j = j0 + fm.rsub, r = Kc + j;
        if (fm.act && j < HR)
            *reinterpret_cast<uint4*>(nxt + (long)j * C) = ld8raw(r < HR ? cur + (long)r * C : chunk + (long)(r - HR) * C);
    }
}

// One wave per hop (s, i), i = 0 .. Kc: samples [i h, (i + 1) h) of the call = upper half of frame i - 1 (i = 0: the carried tail) +
// lower half of frame i; hop Kc is the new tail (upper half of frame Kc - 1 alone).  V^T in LDS ([AL][N + 1]); sw = w relu(mask) of
// the two frames in LDS per wave.
__global__ __launch_bounds__(256) void ctns_decoder_kernel(const float* __restrict__ w /*[S][Kc][N]*/, const bf16_raw* __restrict__ mask /*[S][Kc][Cs*N]*/,
                                                           const float* __restrict__ V /*[ac*L][N]*/, float* __restrict__ tail /*[2][S][Cs][ac][h]*/,
                                                           const int* __restrict__ phase, const int* __restrict__ pos, int S, int Kc, int N,
                                                           int L, int ac, int Cs, float* __restrict__ out /*[S][Cs][ac][Kc*h]*/) {
    extern __shared__ float smem[];
    const int AL = ac * L;
    float* sV = smem;                                  // [AL][N + 1]
    float* ssw = smem + (size_t)AL * (N + 1);          // per wave [2][N]
    for (int i = threadIdx.x; i < AL * N; i += 256) { const int l = i / N, n = i - l * N; sV[l * (N + 1) + n] = V[i]; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* swu = ssw + wave * 2 * N;                   // frame i - 1
    float* swl = swu + N;                              // frame i
    const int step = L / 2, ph = phase[0] & 1;
    const float* tcur = tail + (long)ph * S * Cs * ac * step;
    float* tnxt = tail + (long)(ph ^ 1) * S * Cs * ac * step;
    const long hops = (long)S * (Kc + 1);
    for (long hp = (long)blockIdx.x * 4 + wave; hp < hops; hp += (long)gridDim.x * 4) {
        const int m = (int)(hp / (Kc + 1)), i = (int)(hp - (long)m * (Kc + 1));
        const int p0 = pos[m];
        const bool up = i >= 1 && p0 + i - 1 >= 0, lo = i < Kc && p0 + i >= 0;      // (a frame with a negative index adds nothing)
        const long fu = (long)m * Kc + i - 1, fl = (long)m * Kc + i;
        for (int c = 0; c < Cs; ++c) {
            for (int n = lane; n < N; n += 64) {
                if (up) { const float ml = bf2f(mask[fu * ((long)Cs * N) + c * N + n]); swu[n] = w[fu * N + n] * (ml > 0.f ? ml : 0.f); }
                if (lo) { const float ml = bf2f(mask[fl * ((long)Cs * N) + c * N + n]); swl[n] = w[fl * N + n] * (ml > 0.f ? ml : 0.f); }
            }
            // the LDS queue of a wave is in order: a compiler-level barrier keeps the reads below behind the other lanes' stores
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int o = lane; o < ac * step; o += 64) {
                const int a = o / step, l = o - a * step;
                const long so = (((long)m * Cs + c) * ac + a) * step + l;
                float hi = i == 0 ? tcur[so] : 0.f, lw = 0.f;
                if (up) {
                    const float* v = sV + (a * L + step + l) * (N + 1);
                    float acc = 0.f;
                    for (int n = 0; n < N; ++n) acc += swu[n] * v[n];
                    hi = acc;
                }
                if (lo) {
                    const float* v = sV + (a * L + l) * (N + 1);
                    float acc = 0.f;
                    for (int n = 0; n < N; ++n) acc += swl[n] * v[n];
                    lw = acc;
                }
                if (i < Kc) out[(((long)m * Cs + c) * ac + a) * Kc * step + (long)i * step + l] = hi + lw;
                else tnxt[so] = hi;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
}

__global__ __launch_bounds__(256) void ctns_advance_kernel(int* __restrict__ pos, int* __restrict__ phase, int S, int Kc) {
    for (int s = threadIdx.x; s < S; s += 256) pos[s] += Kc;
    if (threadIdx.x == 0) phase[0] ^= 1;
}

// ------------------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------------------
static int ctns_check_chunk(const char* who, int S, int Kc) {
    SEHIP_REQUIRE(S >= 1, "%s: streams S=%d must be at least 1", who, S);
    SEHIP_REQUIRE(Kc >= 1, "%s: chunk_frames Kc=%d must be at least 1", who, Kc);
    SEHIP_REQUIRE((long)S * ((long)Kc + 1) < (1L << 30), "%s: S=%d streams of Kc=%d frames are too many rows", who, S, Kc);
    return 0;
}

extern "C" int sehip_ctns_encoder(const float* x, float* carry, const int* phase, const float* U, const float* gamma, const float* beta,
                                  int S, int ac, int Kc, int N, int L, float* w, void* cln_bf16, void* stream) {
    if (int e = ctns_check_chunk("ctns_encoder", S, Kc)) return e;
    SEHIP_REQUIRE(ac >= 1 && L >= 2 && (L & 1) == 0, "ctns_encoder: bad sizes (ac=%d L=%d: L must be even)", ac, L);
    SEHIP_REQUIRE(N >= 8 && N <= 64 * CTNS_MAXC && (N & 7) == 0, "ctns_encoder: N=%d must be a multiple of 8 up to %d", N, 64 * CTNS_MAXC);
    const size_t lds = (size_t)N * ac * L * sizeof(float);
    SEHIP_REQUIRE(lds <= 64 * 1024, "ctns_encoder: basis of %zu bytes does not fit the LDS budget", lds);
    SEHIP_REQUIRE(x && carry && phase && U && gamma && beta && w && cln_bf16, "ctns_encoder: null pointer argument");
    long g = ((long)S * Kc + 3) / 4;
    if (g > 2048) g = 2048;
    if (N <= 256) ctns_encoder_kernel<4><<<(int)g, 256, lds, (hipStream_t)stream>>>(x, carry, phase, U, gamma, beta, S, ac, Kc, N, L, w, (bf16_raw*)cln_bf16);
    else ctns_encoder_kernel<8><<<(int)g, 256, lds, (hipStream_t)stream>>>(x, carry, phase, U, gamma, beta, S, ac, Kc, N, L, w, (bf16_raw*)cln_bf16);
    SEHIP_CHECK_LAUNCH("ctns_encoder");
    return 0;
}

extern "C" int sehip_ctns_dwconv(const void* h1, void* hist, const int* phase, const int* pos, const float* slope1, const float* gamma,
                                 const float* beta, const float* Wd, int P, int dilation, int S, int Kc, int C, void* h2, void* stream) {
    if (int e = ctns_check_chunk("ctns_dwconv", S, Kc)) return e;
    SEHIP_REQUIRE(C >= 8 && C <= 512 && (C & 7) == 0, "ctns_dwconv: channels C=%d must be a multiple of 8 in [8, 512]", C);
    SEHIP_REQUIRE(P == 3 || P == 5 || P == 7, "ctns_dwconv: kernel size P must be 3, 5 or 7 (got %d)", P);
    SEHIP_REQUIRE(dilation >= 1 && dilation <= (1 << 20), "ctns_dwconv: dilation must be in [1, 2^20] (got %d)", dilation);
    SEHIP_REQUIRE(S <= 65535, "ctns_dwconv: S=%d streams exceed the grid's second dimension", S);
    SEHIP_REQUIRE(h1 && hist && phase && pos && slope1 && gamma && beta && Wd && h2, "ctns_dwconv: null pointer argument");
    // both loops of the kernel stride over the same grid.  A chunk is a few rows and the chain waits for this launch: one pass of
    // 256 / G rows per workgroup (ctn_grid's six pieces per thread are for tensors of 1e5 rows; at Kc = 32, C = 256 they made ONE
    // workgroup walk four dependent passes)
    const int rows = Kc > (P - 1) * dilation ? Kc : (P - 1) * dilation;
    int G = 1;
    while (G < (C >> 3)) G <<= 1;
    const int rpb = 256 / G;
    long gx = ((long)rows + rpb - 1) / rpb;
    if (gx > 256) gx = 256;
    const dim3 grid((unsigned)gx, (unsigned)S);
    bf16_raw* hs = (bf16_raw*)hist;
#define CTNS_DW(P_) ctns_dwconv_kernel<P_><<<grid, 256, 0, (hipStream_t)stream>>>((const bf16_raw*)h1, hs, phase, pos, slope1, gamma, beta, Wd, dilation, Kc, C, \
                                                                                  (bf16_raw*)h2)
    if (P == 3) CTNS_DW(3); else if (P == 5) CTNS_DW(5); else CTNS_DW(7);
#undef CTNS_DW
    SEHIP_CHECK_LAUNCH("ctns_dwconv");
    return 0;
}

extern "C" int sehip_ctns_decoder(const float* w, const void* mask_bf16, const float* V, float* tail, const int* phase, const int* pos, int S,
                                  int Kc, int N, int L, int ac, int Cs, float* out, void* stream) {
    if (int e = ctns_check_chunk("ctns_decoder", S, Kc)) return e;
    SEHIP_REQUIRE(ac >= 1 && Cs >= 1 && L >= 2 && (L & 1) == 0, "ctns_decoder: bad sizes (ac=%d Cs=%d L=%d: L must be even)", ac, Cs, L);
    SEHIP_REQUIRE(N >= 8 && N <= 64 * CTNS_MAXC && (N & 7) == 0, "ctns_decoder: N=%d must be a multiple of 8 up to %d", N, 64 * CTNS_MAXC);
    const size_t lds = ((size_t)ac * L * (N + 1) + 8 * (size_t)N) * sizeof(float);
    SEHIP_REQUIRE(lds <= 64 * 1024, "ctns_decoder: %zu bytes of LDS needed", lds);
    SEHIP_REQUIRE(w && mask_bf16 && V && tail && phase && pos && out, "ctns_decoder: null pointer argument");
    long g = ((long)S * (Kc + 1) + 3) / 4;
    if (g > 2048) g = 2048;
    ctns_decoder_kernel<<<(int)g, 256, lds, (hipStream_t)stream>>>(w, (const bf16_raw*)mask_bf16, V, tail, phase, pos, S, Kc, N, L, ac, Cs, out);
    SEHIP_CHECK_LAUNCH("ctns_decoder");
    return 0;
}

extern "C" int sehip_ctns_advance(int* pos, int* phase, int S, int Kc, void* stream) {
    if (int e = ctns_check_chunk("ctns_advance", S, Kc)) return e;
    SEHIP_REQUIRE(pos && phase, "ctns_advance: null pointer argument");
    ctns_advance_kernel<<<1, 256, 0, (hipStream_t)stream>>>(pos, phase, S, Kc);
    SEHIP_CHECK_LAUNCH("ctns_advance");
    return 0;
}
