// julius.resample_frac on the device (src/dataset.py:117-122, :354-359 resample every mixture and every source before the statistics,
// the normalisation and the crop): with the ratio reduced to old / new, width = ceil(24 * old / (0.945 * min(old, new))) and
// K = 2 * width + old taps, output sample m = q * new + p (frame q, phase p) of a row of len samples is
//     y[m] = sum_{k < K} kernels[p][k] * x[clamp(q * old + k - width, 0, len - 1)]
// (F.pad(..., (width, width + old), 'replicate') + conv1d(stride = old) + transpose + cut).  fp32 throughout, one ordinary launch
// per call, no atomics, every output sample summed by one thread in a fixed order: bit-identical from run to run.
//
// Rows live in one flat buffer as for wav_row_stats (row starts unaligned, so all global traffic is 4-byte accesses).  Every kernel
// stages the INPUT WINDOW of a tile of frames in LDS with the clamp applied while staging; the table never enters LDS:
//   phase kernel  (any new):   one lane per frame, P phases per lane in registers.  The phase group is wave-uniform, so the table
//                              values are scalar loads (the 360-640 KB tables of 441 -> 160 / 160 -> 441 / 441 -> 320 stay in L2 and the
//                              scalar cache) and one 16-byte LDS read feeds 4 * P FMAs (v_pk_fma_f32: taps pair up along k).  The
//                              16 waves of a block split into wf frame sub-tiles of 64 frames x 16 / wf phase groups; the window is
//                              stored as rows of `old` samples with a row stride that is 4 (mod 8) words, so the lanes' strided
//                              ds_read_b128 are aligned and conflict-free for every `old` (441, and the even 160 of 160 -> 441).
//   decim kernel  (new == 1):  48 kHz -> 16 kHz is 3 -> 1: one phase, 157 taps.  A lane takes 8 CONSECUTIVE outputs and walks the
//                              polyphase components r = k mod old of the input: for fixed r the taps j * old + r slide over
//                              x_r[q + j], so a register window of 8 samples takes one LDS read per 8 FMAs.  No phase tiling, no
//                              idle waves; results go back through LDS for coalesced stores.
//   direct kernel:             a window that does not fit the LDS (old > ~600, or a caller's own huge width): one thread per
//                              output sample straight from global memory.  Correct for every accepted argument, not tuned.
#include <mutex>
#include "common.h"
#include "resample_plan.h"

namespace {
typedef __attribute__((ext_vector_type(2))) float f32x2;
constexpr int RS_MAX_TERM = 1024;
constexpr int RS_MAX_WIDTH = 1 << 16;
constexpr int RS_MAX_DEVICES = 64;

__device__ __forceinline__ long rs_clamp(long i, long n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// what the row may write: the resampled length, and never more than the caller's out_off leaves room for
__device__ __forceinline__ long rs_row_out(const long* row_off, const long* out_off, int r, int old_sr, int new_sr) {
    const long n = row_off[r + 1] - row_off[r], room = out_off[r + 1] - out_off[r];
    const long n_out = n > 0 ? n * new_sr / old_sr : 0;
    return n_out < room ? n_out : room;
}

template <int P>
__global__ __launch_bounds__(64 * RS_WAVES) void resample_phase_kernel(const float* __restrict__ raw, const long* __restrict__ row_off,
                                                                       const float* __restrict__ table, int old_sr, int new_sr, int width,
                                                                       int os, int wf, float* __restrict__ out,
                                                                       const long* __restrict__ out_off) {
    extern __shared__ __attribute__((aligned(16))) float rs_x[];   // [F + ceil(K / old)][os]: window sample i at (i / old) * os + i % old
    const int K = 2 * width + old_sr, F = 64 * wf;
    const int r = blockIdx.y;
    const long lo = row_off[r], n = row_off[r + 1] - lo;
    const long n_out = rs_row_out(row_off, out_off, r, old_sr, new_sr);
    const long tiles = ((n_out + new_sr - 1) / new_sr + F - 1) / F;
    const float* x = raw + lo;
    float* y = out + out_off[r];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int fq = (wave % wf) * 64 + lane, g0 = wave / wf, gstep = RS_WAVES / wf;
    const int groups = (new_sr + P - 1) / P;
    const int W = (F - 1) * old_sr + K;
    const float* xw = rs_x + fq * os;                             // os = 4 (mod 8): 16-byte aligned rows, 16 lanes on 16 distinct slots
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long base = tile * F * old_sr - width;
        __syncthreads();                                          // the previous tile's readers are done
        for (int i = threadIdx.x; i < W; i += 64 * RS_WAVES) {
            const int a = i / old_sr;
            rs_x[a * os + (i - a * old_sr)] = x[rs_clamp(base + i, n)];
        }
        __syncthreads();
        const long m0 = (tile * F + fq) * new_sr;
        for (int g = g0; g < groups; g += gstep) {
            int pk[P];                                            // table row offsets (the last group repeats phase new - 1, not stored)
            f32x2 acc[P];                                         // taps of even / odd position in their row: two chains per output
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int p = g * P + i;
                pk[i] = (p < new_sr ? p : new_sr - 1) * K;
                acc[i] = f32x2{0.f, 0.f};
            }
            for (int k0 = 0, j = 0; k0 < K; k0 += old_sr, ++j) {
                const int cnt = K - k0 < old_sr ? K - k0 : old_sr;
                const float* xr = xw + j * os;
                const float* tk = table + k0;
                int c = 0;
                for (; c + 4 <= cnt; c += 4) {
                    const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + c);
                    const f32x2 x01 = {xv.x, xv.y}, x23 = {xv.z, xv.w};
#pragma unroll
                    for (int i = 0; i < P; ++i) {
                        const float* t = tk + pk[i] + c;          // wave-uniform: scalar loads
                        acc[i] = __builtin_elementwise_fma(f32x2{t[0], t[1]}, x01, acc[i]);
                        acc[i] = __builtin_elementwise_fma(f32x2{t[2], t[3]}, x23, acc[i]);
                    }
                }
                for (; c < cnt; ++c) {
                    const float x0 = xr[c];
#pragma unroll
                    for (int i = 0; i < P; ++i) acc[i].x = fmaf(tk[pk[i] + c], x0, acc[i].x);
                }
            }
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int p = g * P + i;
                if (p < new_sr && m0 + p < n_out) y[m0 + p] = acc[i].x + acc[i].y;
            }
        }
    }
}

__global__ __launch_bounds__(256) void resample_decim_kernel(const float* __restrict__ raw, const long* __restrict__ row_off,
                                                             const float* __restrict__ table, int old_sr, int width,
                                                             float* __restrict__ out, const long* __restrict__ out_off) {
    extern __shared__ __attribute__((aligned(16))) float rs_x[];   // window sample i at i + ((i / old) >> 3): a lane's 8 frames are
    const int K = 2 * width + old_sr;                            // 8 * old + 1 words from the next lane's -- an odd stride
    const int r = blockIdx.y;
    const long lo = row_off[r], n = row_off[r + 1] - lo;
    const long n_out = rs_row_out(row_off, out_off, r, old_sr, 1);
    const long tiles = (n_out + RS_DF - 1) / RS_DF;
    const float* x = raw + lo;
    float* y = out + out_off[r];
    const int W = (RS_DF - 1) * old_sr + K;
    const int q0 = threadIdx.x * RS_DT;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long base = tile * RS_DF * old_sr - width;
        __syncthreads();
        for (int i = threadIdx.x; i < W; i += 256) rs_x[i + ((i / old_sr) >> 3)] = x[rs_clamp(base + i, n)];
        __syncthreads();
        float acc[RS_DT];
#pragma unroll
        for (int t = 0; t < RS_DT; ++t) acc[t] = 0.f;
        for (int c = 0; c < old_sr; ++c) {                        // taps k = j * old + c, j < jn, read x_c[q + j] = window[(q + j) * old + c]
            const int jn = (K - c + old_sr - 1) / old_sr;
            float w[RS_DT];                                       // x_c[q0 + j + t] sits in w[(j + t) & 7]
#pragma unroll
            for (int t = 0; t < RS_DT - 1; ++t) {
                const int a = q0 + t;
                w[t] = rs_x[a * old_sr + c + (a >> 3)];
            }
            for (int j0 = 0; j0 < jn; j0 += RS_DT) {
#pragma unroll
                for (int u = 0; u < RS_DT; ++u) {
                    const int j = j0 + u;
                    if (j < jn) {                                 // (wave-uniform)
                        const int a = q0 + j + RS_DT - 1;
                        w[(u + RS_DT - 1) & (RS_DT - 1)] = rs_x[a * old_sr + c + (a >> 3)];
                        const float h = table[j * old_sr + c];
#pragma unroll
                        for (int t = 0; t < RS_DT; ++t) acc[t] = fmaf(h, w[(u + t) & (RS_DT - 1)], acc[t]);
                    }
                }
            }
        }
        __syncthreads();                                          // window consumed: the tile's outputs take its place
#pragma unroll
        for (int t = 0; t < RS_DT; ++t) rs_x[q0 + t + ((q0 + t) >> 3)] = acc[t];
        __syncthreads();
        for (int i = threadIdx.x; i < RS_DF; i += 256) {
            const long m = tile * RS_DF + i;
            if (m < n_out) y[m] = rs_x[i + (i >> 3)];
        }
    }
}

__global__ __launch_bounds__(256) void resample_direct_kernel(const float* __restrict__ raw, const long* __restrict__ row_off,
                                                              const float* __restrict__ table, int old_sr, int new_sr, int width,
                                                              float* __restrict__ out, const long* __restrict__ out_off) {
    const int K = 2 * width + old_sr;
    const int r = blockIdx.y;
    const long lo = row_off[r], n = row_off[r + 1] - lo;
    const long n_out = rs_row_out(row_off, out_off, r, old_sr, new_sr);
    const float* x = raw + lo;
    float* y = out + out_off[r];
    for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < n_out; m += (long)gridDim.x * 256) {
        const long q = m / new_sr;
        const float* t = table + (m - q * new_sr) * K;
        const long base = q * old_sr - width;
        float acc = 0.f;
        for (int k = 0; k < K; ++k) acc = fmaf(t[k], x[rs_clamp(base + k, n)], acc);
        y[m] = acc;
    }
}

long rs_gcd(long a, long b) {
    while (b) { const long t = a % b; a = b; b = t; }
    return a;
}

// the kernels' dynamic LDS may exceed the 64 KB default: the attribute is per device, so it is set once per device (under a lock:
// the first calls of two threads may race) and its result is checked
template <typename KernelT>
hipError_t rs_allow_lds(KernelT k) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RS_LDS_MAX);
}

hipError_t rs_prepare_device() {
    static std::mutex mu;
    static bool done[RS_MAX_DEVICES] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= RS_MAX_DEVICES) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(mu);
    if (done[dev]) return hipSuccess;
    if ((e = rs_allow_lds(&resample_phase_kernel<1>)) != hipSuccess) return e;
    if ((e = rs_allow_lds(&resample_phase_kernel<2>)) != hipSuccess) return e;
    if ((e = rs_allow_lds(&resample_phase_kernel<4>)) != hipSuccess) return e;
    if ((e = rs_allow_lds(&resample_phase_kernel<8>)) != hipSuccess) return e;
    if ((e = rs_allow_lds(&resample_decim_kernel)) != hipSuccess) return e;
    done[dev] = true;
    return hipSuccess;
}
}  // namespace

extern "C" long sehip_resample_out_len(long n, int old_sr, int new_sr) {
    if (n < 0 || old_sr <= 0 || new_sr <= 0) return -1;
    const long g = rs_gcd(old_sr, new_sr);
    return n * (new_sr / g) / (old_sr / g);
}

extern "C" int sehip_resample_frac(const float* raw, const long* row_off, int rows, const float* kernels, int old_sr, int new_sr, int width,
                                   float* out, const long* out_off, void* stream) {
    SEHIP_REQUIRE(rows > 0 && rows <= 65535, "resample_frac: rows=%d outside [1, 65535]", rows);
    SEHIP_REQUIRE(old_sr > 0 && new_sr > 0 && old_sr <= RS_MAX_TERM && new_sr <= RS_MAX_TERM,
                  "resample_frac: ratio %d -> %d has a term outside [1, %d]", old_sr, new_sr, RS_MAX_TERM);
    SEHIP_REQUIRE(rs_gcd(old_sr, new_sr) == 1 && old_sr != new_sr, "resample_frac: ratio %d -> %d is not reduced (or is 1 -> 1: nothing to do)",
                  old_sr, new_sr);
    SEHIP_REQUIRE(width > 0 && width <= RS_MAX_WIDTH, "resample_frac: width=%d outside [1, %d]", width, RS_MAX_WIDTH);
    SEHIP_REQUIRE(raw && row_off && kernels && out && out_off, "resample_frac: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const hipError_t prep = rs_prepare_device();
    if (prep != hipSuccess) return sehip_set_error(-2, "resample_frac: cannot raise the kernels' LDS limit: %s", hipGetErrorString(prep));
    const rs_plan pl = rs_make_plan(old_sr, new_sr, width);         // (resample_plan.h: the streamer follows the same decision)
    const long K = pl.K;
    int gx = 2048 / rows;                                         // blocks per row; a block strides over its row's tiles
    gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
    if (pl.kind == RS_DECIM) {
        resample_decim_kernel<<<dim3(gx, rows), 256, pl.lds, st>>>(raw, row_off, kernels, old_sr, width, out, out_off);
        SEHIP_CHECK_LAUNCH("resample_frac (decim)");
        sehip_note_kernel("resample_decim old=%d K=%ld lds=%zu", old_sr, K, pl.lds);
        return 0;
    }
    if (pl.kind == RS_PHASE) {
        const dim3 grid(gx, rows);
        const int os = pl.os, wf = pl.wf;
#define RS_LAUNCH(PP) resample_phase_kernel<PP><<<grid, 64 * RS_WAVES, pl.lds, st>>>(raw, row_off, kernels, old_sr, new_sr, width, os, wf, out, out_off)
        if (pl.P == 8) RS_LAUNCH(8);
        else if (pl.P == 4) RS_LAUNCH(4);
        else if (pl.P == 2) RS_LAUNCH(2);
        else RS_LAUNCH(1);
#undef RS_LAUNCH
        SEHIP_CHECK_LAUNCH("resample_frac (phase)");
        sehip_note_kernel("resample_phase P=%d wf=%d old=%d new=%d K=%ld lds=%zu", pl.P, wf, old_sr, new_sr, K, pl.lds);
        return 0;
    }
    resample_direct_kernel<<<dim3(gx, rows), 256, 0, st>>>(raw, row_off, kernels, old_sr, new_sr, width, out, out_off);
    SEHIP_CHECK_LAUNCH("resample_frac (direct)");
    sehip_note_kernel("resample_direct old=%d new=%d K=%ld", old_sr, new_sr, K);
    return 0;
}
