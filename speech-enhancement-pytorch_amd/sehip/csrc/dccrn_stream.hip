// DCCRN run chunk by chunk (sehip/model/dccrn_stream.py: DCCRNStreamer) -- the kernels that carry state from one chunk to the next.
// S independent streams, Kc hops (Kc win_inc new samples per stream) per call.  The convolutions, the LSTM input products and the
// projections run as products of the implicit-GEMM engine on [history | chunk] buffers; the recurrence is sehip_lstm_fwd_chunk on
// buffers of Kc + 1 steps whose step 0 is the carried (h, c).
//
//   dcs_analysis    carry | chunk -> Kc spectra (fp32, and into the LA-deep ring) + the bf16 encoder input behind its history row
//   dcs_norm_hist   eval-mode BatchNorm + PReLU of a layer's Kc chunk rows behind its H history rows; the next call's history
//   dcs_lstm_carry  step Kc of the (h, c) records -> step 0
//   dcs_synthesis   mask x spectrum of the LAGGING frames pos - LA .. pos + Kc - LA - 1, inverse transform, window, overlap-add with the
//                   carried tail, 1 / window energy, clamp: Kc hops of output
//   dcs_mark_end    end[s] = pos[s] + extra (flush)          dcs_advance   pos[s] += Kc, phase ^= 1
//
// Frame indices.  pos[s] (int32, device) is the index of the first frame of the coming call, 0 on a fresh stream (a zero carry IS the
// reference's left pad: there is no phantom frame).  Every transposed convolution reads frames t and t + 1, so decoder j (and the
// buffers behind it) lags the encoder by j + 1 frames and the mask by LA = 6; output hop block q is the sum of frames q .. q + R - 1
// (R = win / hop), so the output lags by LA + R - 1 hops.  Frames with a negative index and output blocks with a negative index come
// out of zero histories; they feed only each other and the synthesis drops them.  end[s] ("infinite" = INT_MAX while the stream is open)
// is the number of frames of the clip: a frame >= end is ABSENT -- dcs_norm_hist stores it as a zero row (so it enters every decoder
// product as zeros, main input and skip; BatchNorm of a silent frame would not be zero) and dcs_synthesis adds nothing for it.
//
// State discipline (as csrc/tasnet_stream.hip): every piece of state that a launch both reads and renews exists twice, [2][...], and the
// device word `phase` names the current half; a launch reads half phase and writes half phase ^ 1, so no launch reads an address it
// writes, whatever the order of its workgroups, and a chunk has the same launch arguments every time (capturable).  dcs_lstm_carry
// reads step Kc and writes step 0 of the same buffer (Kc >= 1: different addresses).  No workgroup waits for another one.
#include "common.h"

#include "fft512.h"
#include "mask.h"

#define DCS_LA 6

static __device__ __forceinline__ int dcs_brev3(int j) { return ((j & 1) << 2) | (j & 2) | ((j >> 2) & 1); }

// ------------------------------------------------------------------------------------------------------------------
// analysis: one wave per frame (s, k); the transform, its window multiply and the LDS row are stft_fwd_kernel's (csrc/stft.hip)
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dcs_analysis_kernel(const float* __restrict__ x /*[S][Kc*hop]*/, float* __restrict__ carry /*[2][S][pad]*/,
                                                           const int* __restrict__ phase, const float* __restrict__ window, int S, int Kc,
                                                           int win, int hop, float2* __restrict__ spec /*[S][Kc][257]*/,
                                                           float2* __restrict__ ring /*[2][S][LA][257]*/, unsigned* __restrict__ enc /*[S][1+Kc][256]*/,
                                                           unsigned* __restrict__ ehist /*[2][S][256]*/) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long frame = (long)blockIdx.x * 4 + w;
    __shared__ float2 srow[4][264 + 33];
    __shared__ unsigned senc[4][256];
    if (frame >= (long)S * Kc) return;
    const int s = (int)(frame / Kc), k = (int)(frame - (long)s * Kc);
    const int pad = win - hop, ph = phase[0] & 1;
    const float* ccur = carry + ((long)ph * S + s) * pad;
    float* cnxt = carry + ((long)(ph ^ 1) * S + s) * pad;
    const float* xs = x + (long)s * Kc * hop;
    FftTw tw;
    fft_twiddles<-1>(tw, lane);
    float re[8], im[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int n = lane + 64 * r;
        float v = 0.f;
        if (n < win) {
            const int i = k * hop + n;                   // sample i of carry | chunk
            v = (i < pad ? ccur[i] : xs[i - pad]) * window[n];
        }
        re[r] = v; im[r] = 0.f;
    }
    fft512_wave<-1>(re, im, tw, lane);
    const int k0 = 8 * brev6(lane);
    if (k0 <= 256) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int b = k0 + dcs_brev3(j);
            if (b <= 256) {
                srow[w][b + (b >> 3)] = make_float2(re[j], im[j]);
                if (b >= 1) senc[w][b - 1] = pack_bf2(re[j], im[j]);
            }
        }
    }
    // (the row belongs to this wave alone and a wave's LDS operations complete in order: a compiler-level barrier is enough)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float2* rcur = ring + ((long)ph * S + s) * DCS_LA * NBIN;
    float2* rnxt = ring + ((long)(ph ^ 1) * S + s) * DCS_LA * NBIN;
    float2* so = spec + frame * NBIN;
    const int rr = DCS_LA - (Kc - k);                    // this frame's row of the next ring (the last LA rows of ring | chunk)
    float2* ro = rr >= 0 ? rnxt + (long)rr * NBIN : nullptr;
    for (int b = lane; b < NBIN; b += 64) {
        const float2 v = srow[w][b + (b >> 3)];
        so[b] = v;
        if (ro) ro[b] = v;
    }
    const uint4 ev = *reinterpret_cast<const uint4*>(&senc[w][4 * lane]);
    *reinterpret_cast<uint4*>(enc + ((long)s * (Kc + 1) + 1 + k) * 256 + 4 * lane) = ev;
    if (k == Kc - 1) {
        *reinterpret_cast<uint4*>(ehist + ((long)(ph ^ 1) * S + s) * 256 + 4 * lane) = ev;
        for (int m = lane; m < pad; m += 64) {           // the last pad samples of carry | chunk
            const int i = Kc * hop + m;
            cnxt[m] = i < pad ? ccur[i] : xs[i - pad];
        }
    }
    if (k == 0) {
        *reinterpret_cast<uint4*>(enc + (long)s * (Kc + 1) * 256 + 4 * lane) =
            *reinterpret_cast<const uint4*>(ehist + ((long)ph * S + s) * 256 + 4 * lane);
        for (int r = 0; r + Kc < DCS_LA; ++r)            // Kc < LA: the ring rows that stay move up
            for (int b = lane; b < NBIN; b += 64) rnxt[(long)r * NBIN + b] = rcur[(long)(r + Kc) * NBIN + b];
    }
}

// ------------------------------------------------------------------------------------------------------------------
// normalise + PReLU with history.  A frame is F rows of [Cr real | Cr imaginary] bf16; one thread per 4 complex channels of a row of
// z = history | chunk.  The arithmetic of a chunk element is cbn_apply_kernel's (csrc/cbn.hip), statement by statement.
// coef == nullptr: the chunk rows are copied (the LSTM projection has no BatchNorm behind it).
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dcs_norm_hist_kernel(const bf16_raw* __restrict__ y /*[S][Kc][F][2Cr]*/, const float* __restrict__ coef,
                                                            const float* __restrict__ slope, bf16_raw* __restrict__ hist /*[2][S][H][F][2Cr]*/,
                                                            const int* __restrict__ phase, const int* __restrict__ pos,
                                                            const int* __restrict__ end, int lag, int S, int Kc, int H, int F, int Cr,
                                                            bf16_raw* __restrict__ z /*[S][H+Kc][F][2Cr]*/) {
    const int nq = Cr >> 2, C = 2 * Cr, ph = phase[0] & 1;
    const long per_frame = (long)F * nq, total = (long)S * (H + Kc) * per_frame;
    const float a = coef ? slope[0] : 0.f;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long)gridDim.x * 256) {
        const long fr = it / per_frame;
        const int rem = (int)(it - fr * per_frame), f = rem / nq, q = rem - f * nq;
        const int s = (int)(fr / (H + Kc)), r = (int)(fr - (long)s * (H + Kc));
        const long eo = (long)f * C + 4 * q;             // element of the frame: real part; + Cr: imaginary part
        uint2 vr, vi;
        if (r < H) {
            const bf16_raw* hp = hist + (((long)ph * S + s) * H + r) * F * C + eo;
            vr = *reinterpret_cast<const uint2*>(hp);
            vi = *reinterpret_cast<const uint2*>(hp + Cr);
        } else if (pos[s] + (r - H) - lag >= end[s]) {
            vr = make_uint2(0u, 0u); vi = vr;            // an absent frame
        } else {
            const bf16_raw* yp = y + ((long)s * Kc + (r - H)) * F * C + eo;
            vr = *reinterpret_cast<const uint2*>(yp);
            vi = *reinterpret_cast<const uint2*>(yp + Cr);
            if (coef) {
                const bf16_raw* xr = reinterpret_cast<const bf16_raw*>(&vr);
                const bf16_raw* xi = reinterpret_cast<const bf16_raw*>(&vi);
                float orr[4], oii[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 zc = reinterpret_cast<const float4*>(coef)[(4 * q + j) * 4];
                    const float4 mb = reinterpret_cast<const float4*>(coef)[(4 * q + j) * 4 + 1];
                    const float cr = bf2f(xr[j]) - mb.x, ci = bf2f(xi[j]) - mb.y;
                    // (written with the one fused multiply-add per sum that cbn_apply_kernel's `zc.x * cr + zc.y * ci + mb.z` compiles
                    //  to -- the second product rounded, the first fused, the bias added last: left to the compiler, this kernel got
                    //  another contraction and one element in ~1e5 rounded to the neighbouring bf16 value)
                    const float ur = __builtin_fmaf(zc.x, cr, zc.y * ci) + mb.z;
                    const float ui = __builtin_fmaf(zc.z, cr, zc.w * ci) + mb.w;
                    orr[j] = ur > 0.f ? ur : a * ur;
                    oii[j] = ui > 0.f ? ui : a * ui;
                }
                vr = make_uint2(pack_bf2(orr[0], orr[1]), pack_bf2(orr[2], orr[3]));
                vi = make_uint2(pack_bf2(oii[0], oii[1]), pack_bf2(oii[2], oii[3]));
            }
        }
        bf16_raw* zp = z + ((long)s * (H + Kc) + r) * F * C + eo;
        *reinterpret_cast<uint2*>(zp) = vr;
        *reinterpret_cast<uint2*>(zp + Cr) = vi;
        if (r >= Kc) {                                    // the last H rows of history | chunk are the next call's history
            bf16_raw* np_ = hist + (((long)(ph ^ 1) * S + s) * H + (r - Kc)) * F * C + eo;
            *reinterpret_cast<uint2*>(np_) = vr;
            *reinterpret_cast<uint2*>(np_ + Cr) = vi;
        }
    }
}

// (h, c) of step Kc -> step 0: h bf16 [nh][Kc + 1][H], c fp32 [nc][Kc + 1][4 H] (the records of sehip_lstm_fwd_chunk)
__global__ __launch_bounds__(256) void dcs_lstm_carry_kernel(bf16_raw* __restrict__ h, float* __restrict__ c, int nh, int nc, int Kc, int H) {
    const long th = (long)nh * H, tc = (long)nc * 4 * H;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < th + tc; i += (long)gridDim.x * 256) {
        if (i < th) {
            const long b = i / H, u = i - b * H;
            h[b * (Kc + 1) * H + u] = h[(b * (Kc + 1) + Kc) * H + u];
        } else {
            const long j = i - th, b = j / (4 * H), u = j - b * 4 * H;
            c[b * (Kc + 1) * 4 * H + u] = c[(b * (Kc + 1) + Kc) * 4 * H + u];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// synthesis, first launch: one wave per lagging frame (s, k), frame index pos - LA + k: spectrum row k of ring | chunk, mask row k of
// the chunk -> windowed frame [win] (istft_frames_kernel's arithmetic, csrc/stft.hip); an absent frame is stored as zeros
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dcs_frames_kernel(const float2* __restrict__ spec /*[S][Kc][257]*/, const float2* __restrict__ ring /*[2][S][LA][257]*/,
                                                         const float2* __restrict__ mask /*[S][Kc][256]*/, const float* __restrict__ window,
                                                         const int* __restrict__ phase, const int* __restrict__ pos, const int* __restrict__ end,
                                                         int S, int Kc, int win, int mode, float* __restrict__ frames /*[S][Kc][win]*/) {
    const int lane = threadIdx.x & 63;
    const long frame = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (frame >= (long)S * Kc) return;
    const int s = (int)(frame / Kc), k = (int)(frame - (long)s * Kc);
    const int f = pos[s] - DCS_LA + k, ph = phase[0] & 1;
    float* fo = frames + frame * win;
    if (f < 0 || f >= end[s]) {
        for (int n = lane; n < win; n += 64) fo[n] = 0.f;
        return;
    }
    const float2* sp = k < DCS_LA ? ring + (((long)ph * S + s) * DCS_LA + k) * NBIN : spec + ((long)s * Kc + (k - DCS_LA)) * NBIN;
    const float2* mk = mask + frame * 256;
    FftTw tw;
    fft_twiddles<1>(tw, lane);
    float re[8], im[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int b = lane + 64 * r;
        float er = 0.f, ei = 0.f;
        if (b >= 1 && b <= 256) {  // DC: the mask row is zero padding -> estimate is exactly 0
            const float2 zz = sp[b];
            const float2 m = mk[b - 1];
            apply_mask(mode, zz.x, zz.y, m.x, m.y, er, ei);
        }
        re[r] = er; im[r] = ei;
    }
    fft512_wave<1>(re, im, tw, lane);
    const int n0 = 8 * brev6(lane);
    float u[8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int n = n0 + dcs_brev3(j);
        u[dcs_brev3(j)] = re[j];
        if (n < win) { s1 += re[j]; s2 += (n & 1) ? -re[j] : re[j]; }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    const float c = 1.0f / (float)(FFT_N + win);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int n = n0 + q;
        if (n < win) {
            const float corr = c * (s1 + ((n & 1) ? -s2 : s2));
            fo[n] = window[n] * (1.0f / 256.0f) * (u[q] - corr);
        }
    }
}

// second launch: position j of a stream counts from the first sample of hop block q0 = pos - LA - (R - 1).  j < Kc hop: an output
// sample, else the next tail.  Every sample is stored once: the carried tail, then the chunk's frames in ascending order.
__global__ __launch_bounds__(256) void dcs_ola_kernel(const float* __restrict__ frames, const float* __restrict__ inv_coff /*[hop]*/,
                                                      float* __restrict__ tail /*[2][S][pad]*/, const int* __restrict__ phase,
                                                      const int* __restrict__ pos, const int* __restrict__ end, int S, int Kc, int win, int hop,
                                                      float* __restrict__ out /*[S][Kc*hop]*/) {
    const int s = blockIdx.y, pad = win - hop, ph = phase[0] & 1, p0 = pos[s], e = end[s];
    const float* tcur = tail + ((long)ph * S + s) * pad;
    float* tnxt = tail + ((long)(ph ^ 1) * S + s) * pad;
    const int q0 = p0 - DCS_LA - (win / hop - 1);
    for (int j = blockIdx.x * 256 + threadIdx.x; j < Kc * hop + pad; j += gridDim.x * 256) {
        float acc = j < pad ? tcur[j] : 0.f;
        int k_lo = (j - win + hop) / hop, k_hi = j / hop;
        if (j - win + 1 <= 0) k_lo = 0;
        if (k_hi > Kc - 1) k_hi = Kc - 1;
        for (int k = k_lo; k <= k_hi; ++k) {
            const int f = p0 - DCS_LA + k;
            if (f >= 0 && f < e) acc += frames[((long)s * Kc + k) * win + (j - k * hop)];
        }
        if (j < Kc * hop) {
            const float v = acc * inv_coff[j % hop];
            out[(long)s * Kc * hop + j] = q0 + j / hop < 0 ? 0.f : fminf(1.f, fmaxf(-1.f, v));
        } else {
            tnxt[j - Kc * hop] = acc;
        }
    }
}

__global__ __launch_bounds__(256) void dcs_advance_kernel(int* __restrict__ pos, int* __restrict__ phase, int S, int Kc) {
    for (int s = threadIdx.x; s < S; s += 256) pos[s] += Kc;
    if (threadIdx.x == 0) phase[0] ^= 1;
}

__global__ __launch_bounds__(256) void dcs_mark_end_kernel(const int* __restrict__ pos, int* __restrict__ end, int S, int extra) {
    for (int s = blockIdx.x * 256 + threadIdx.x; s < S; s += gridDim.x * 256) end[s] = pos[s] + extra;
}

// ------------------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------------------
static int dcs_check_chunk(const char* who, int S, int Kc) {
    SEHIP_REQUIRE(S >= 1 && S <= 65535, "%s: streams S=%d must be in [1, 65535]", who, S);
    SEHIP_REQUIRE(Kc >= 1 && Kc <= 4096, "%s: chunk_frames Kc=%d must be in [1, 4096]", who, Kc);
    return 0;
}

static int dcs_check_frame(const char* who, int win, int hop) {
    SEHIP_REQUIRE(win > 0 && win <= FFT_N && (win % 2) == 0, "%s: win_len must be even and <= 512 (got %d)", who, win);
    SEHIP_REQUIRE(hop > 0 && hop <= win && win % hop == 0, "%s: win_len=%d must be a multiple of win_inc=%d", who, win, hop);
    return 0;
}

extern "C" int sehip_dcs_analysis(const float* x, float* carry, const int* phase, const float* window, int S, int Kc, int win, int hop,
                                  float* spec, float* ring, void* enc_bf16, void* enc_hist_bf16, void* stream) {
    if (int e = dcs_check_chunk("dcs_analysis", S, Kc)) return e;
    if (int e = dcs_check_frame("dcs_analysis", win, hop)) return e;
    SEHIP_REQUIRE(x && carry && phase && window && spec && ring && enc_bf16 && enc_hist_bf16, "dcs_analysis: null pointer argument");
    dcs_analysis_kernel<<<cdiv((long)S * Kc, 4), 256, 0, (hipStream_t)stream>>>(x, carry, phase, window, S, Kc, win, hop, (float2*)spec,
                                                                                 (float2*)ring, (unsigned*)enc_bf16, (unsigned*)enc_hist_bf16);
    SEHIP_CHECK_LAUNCH("dcs_analysis");
    return 0;
}

extern "C" int sehip_dcs_norm_hist(const void* y, const float* coef, const float* slope, void* hist, const int* phase, const int* pos,
                                   const int* end, int lag, int S, int Kc, int H, int F, int Cr, void* z, void* stream) {
    if (int e = dcs_check_chunk("dcs_norm_hist", S, Kc)) return e;
    SEHIP_REQUIRE(H >= 1 && H <= 64, "dcs_norm_hist: history rows H=%d must be in [1, 64]", H);
    SEHIP_REQUIRE(F >= 1 && F <= 65536, "dcs_norm_hist: rows per frame F=%d must be in [1, 65536]", F);
    SEHIP_REQUIRE(Cr >= 4 && Cr <= 4096 && (Cr & 3) == 0, "dcs_norm_hist: complex channels Cr=%d must be a multiple of 4 in [4, 4096]", Cr);
    SEHIP_REQUIRE(lag >= 0 && lag <= DCS_LA, "dcs_norm_hist: lag=%d must be in [0, %d]", lag, DCS_LA);
    SEHIP_REQUIRE(y && hist && phase && pos && end && z, "dcs_norm_hist: null pointer argument");
    SEHIP_REQUIRE(coef == nullptr || slope != nullptr, "dcs_norm_hist: coefficient records without a PReLU slope");
    const long total = (long)S * (H + Kc) * F * (Cr >> 2);
    long g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    dcs_norm_hist_kernel<<<(int)g, 256, 0, (hipStream_t)stream>>>((const bf16_raw*)y, coef, slope, (bf16_raw*)hist, phase, pos, end, lag, S, Kc,
                                                                  H, F, Cr, (bf16_raw*)z);
    SEHIP_CHECK_LAUNCH("dcs_norm_hist");
    return 0;
}

extern "C" int sehip_dcs_lstm_carry(void* h_bf16, float* c, int S, int Kc, int hidden, void* stream) {
    if (int e = dcs_check_chunk("dcs_lstm_carry", S, Kc)) return e;
    SEHIP_REQUIRE(hidden == 32 || hidden == 64 || hidden == 96 || hidden == 128, "dcs_lstm_carry: hidden=%d must be 32, 64, 96 or 128", hidden);
    SEHIP_REQUIRE(h_bf16 && c, "dcs_lstm_carry: null pointer argument");
    const int nh = 4 * S, nc = 4 * ((S + 3) / 4);
    const long total = (long)nh * hidden + (long)nc * 4 * hidden;
    dcs_lstm_carry_kernel<<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>((bf16_raw*)h_bf16, c, nh, nc, Kc, hidden);
    SEHIP_CHECK_LAUNCH("dcs_lstm_carry");
    return 0;
}

extern "C" int sehip_dcs_synthesis(const float* spec, const float* ring, const float* mask, const float* window, const float* inv_coff,
                                   float* tail, const int* phase, const int* pos, const int* end, int S, int Kc, int win, int hop, int mode,
                                   float* frames_ws, float* out, void* stream) {
    if (int e = dcs_check_chunk("dcs_synthesis", S, Kc)) return e;
    if (int e = dcs_check_frame("dcs_synthesis", win, hop)) return e;
    SEHIP_REQUIRE(mode >= 0 && mode <= 2, "dcs_synthesis: masking mode must be 0(E) 1(C) 2(R)");
    SEHIP_REQUIRE(spec && ring && mask && window && inv_coff && tail && phase && pos && end && frames_ws && out,
                  "dcs_synthesis: null pointer argument");
    hipStream_t st = (hipStream_t)stream;
    dcs_frames_kernel<<<cdiv((long)S * Kc, 4), 256, 0, st>>>((const float2*)spec, (const float2*)ring, (const float2*)mask, window, phase, pos,
                                                             end, S, Kc, win, mode, frames_ws);
    int gx = cdiv((long)Kc * hop + win - hop, 256);
    if (gx > 1024) gx = 1024;
    dcs_ola_kernel<<<dim3(gx, S), 256, 0, st>>>(frames_ws, inv_coff, tail, phase, pos, end, S, Kc, win, hop, out);
    SEHIP_CHECK_LAUNCH("dcs_synthesis");
    return 0;
}

extern "C" int sehip_dcs_mark_end(const int* pos, int* end, int S, int extra, void* stream) {
    SEHIP_REQUIRE(S >= 1, "dcs_mark_end: streams S=%d must be at least 1", S);
    SEHIP_REQUIRE(extra >= 0 && extra < 512, "dcs_mark_end: extra=%d frames must be in [0, 512)", extra);
    SEHIP_REQUIRE(pos && end, "dcs_mark_end: null pointer argument");
    dcs_mark_end_kernel<<<cdiv(S, 256), 256, 0, (hipStream_t)stream>>>(pos, end, S, extra);
    SEHIP_CHECK_LAUNCH("dcs_mark_end");
    return 0;
}

extern "C" int sehip_dcs_advance(int* pos, int* phase, int S, int Kc, void* stream) {
    if (int e = dcs_check_chunk("dcs_advance", S, Kc)) return e;
    SEHIP_REQUIRE(pos && phase, "dcs_advance: null pointer argument");
    dcs_advance_kernel<<<1, 256, 0, (hipStream_t)stream>>>(pos, phase, S, Kc);
    SEHIP_CHECK_LAUNCH("dcs_advance");
    return 0;
}
