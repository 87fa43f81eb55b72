// The multi-resolution STFT loss (sehip.loss.mrstft_loss): per resolution (n_fft, hop, win_length) the spectral convergence
// ||Y - X||_F / ||Y||_F and the mean |log Y - log X| of the magnitudes M = sqrt(max(re^2 + im^2, 1e-7)) of torch.stft (periodic hann of
// win_length centred in n_fft, center=True, reflect padding, no division by win_length), forward and backward.  No spectrum is stored: the
// backward pass transforms both signals again.  No atomics, no readback, every sum in a fixed order.
//   frames<0> : one workgroup per (row, frame pair t0, t0 + 1).  The two frames of a signal are the real and the imaginary part of ONE
//               complex n_fft-point transform and come apart by Z[k] +- conj(Z[n_fft - k]); the clean and the enhanced pair run through
//               the same instructions on two LDS buffers, so equal inputs give equal bits (sc is then exactly 0, and so is its
//               gradient).  The transform is a radix-2 decimation in frequency in LDS, two stages per pass, natural order in,
//               bit-reversed out -- every use of the spectrum here is a sum over bins or a bin-wise product, so nothing is ever put
//               back in order.  Three partial sums per workgroup: sum (Y - X)^2, sum Y^2, sum |log Y - log X|.
//   finalize  : one workgroup adds the partials of every resolution in index order (double) and writes sc, mag, the weighted loss and
//               the two factors the backward pass needs.
//   frames<1> : the same transforms; bin gradient G[k] = (dL/dX / X) (re + i im) of the enhanced frames, extended to a Hermitian spectrum
//               (G / 2 and its conjugate; bins 0 and n_fft / 2 keep their real part) so that the adjoint of the real transform is a real
//               inverse transform; the pair goes back as H(t0) + i H(t0 + 1) through one decimation-in-time inverse (bit-reversed in,
//               natural out), is windowed, and the win_length samples of each frame are stored.
//   gather    : one thread per sample s adds, frames ascending, the stored frame gradients at padded positions s, -s and 2 (n - 1) - s
//               (the adjoint of the reflect padding).
//   frames<2> : the magnitudes of one signal written out, [rows][n_fft / 2 + 1][T] (sehip.ops.stft_magnitudes).
//   pair_*    : the same loss under permutation-invariant training (sehip.loss.pit_mrstft_loss), further down: a forward that transforms
//               each of the 2 S signals of a row group once and fills all S x S pairs, a select that adds the sums in finalize's order
//               and picks the permutation, and frames<1> with the row pairing read from that permutation.
// Conventions of the gradient: a cell the forward clamped (P < 1e-7) passes nothing; |.| at exactly 0 has derivative 0; ||Y - X|| = 0
// gives an exactly zero sc gradient.
#include <type_traits>   // std::integral_constant (mrl_dispatch)

#include "fft512.h"      // fft_detail::cossin_frac, the compile-time series behind g_fft_tw
#include "pit_perm.h"    // PIT_MAXS, pit_best_permutation

// The clean and the enhanced signal must come out of the same arithmetic (equal inputs -> equal bits -> sc exactly 0).  The compiler's
// own choice of which multiply to fuse into which add follows the uses of a value, and those differ between the two signals (the backward
// pass goes on with the enhanced spectrum): every fused multiply-add in this file is written out.
#pragma clang fp contract(off)

namespace {
constexpr int MRL_MAX_NFFT = 2048, MRL_MIN_NFFT = 64, MRL_THREADS = 256, MRL_MAX_RES = 8, MRL_MAX_ROWS = 65535;
constexpr long MRL_MAX_LEN = 1L << 30;
constexpr float MRL_CLAMP = 1e-7f;

// w[h + idx] = (cos, sin) (2 pi idx / (2 h)) for h = 1, 2, 4 .. 1024, idx < h: the twiddles of the stage of span 2 h, contiguous, and
// the same entries for every n_fft -- a transform of N points stages the prefix [0, N) in LDS (entry 0 is unused)
struct alignas(8) MrlCs { float c, s; };
struct MrlTw { MrlCs w[MRL_MAX_NFFT]; };
constexpr MrlTw mrl_make_tw() {
    MrlTw t{};
    for (int h = 1; h <= MRL_MAX_NFFT / 2; h <<= 1)
        for (int idx = 0; idx < h; ++idx) {
            double c = 0, sn = 0;
            fft_detail::cossin_frac(idx, 2 * h, c, sn);
            t.w[h + idx].c = (float)c;
            t.w[h + idx].s = (float)sn;
        }
    return t;
}
__device__ const MrlTw g_mrl_tw = mrl_make_tw();

struct MrlFrames {
    const float* enh;      // [rows][n]
    const float* src;      // [rows][n]
    const float* window;   // [n_fft]: the periodic hann of win_length, zero outside [lp, lp + win)
    long n;
    int T, n_fft, hop, win;
    float* partials;       // <0>: [rows][pairs][3]
    const float* stats;    // <1>: {1 / (||Y - X|| ||Y||) or 0, 1 / cells} of this resolution
    const float* gout;     // <1>: the upstream gradient, one float
    float ksc, kmag;       // <1>: sc_weight / R, mag_weight / R
    float* out;            // <1>: fgrad [rows][T][win]   <2>: magnitudes [rows][n_fft / 2 + 1][T]
};

__device__ __forceinline__ long mrl_reflect(long p, long n) { return p < 0 ? -p : (p >= n ? 2 * (n - 1) - p : p); }

// z[j] = window[j] (frame t0 [j] + i frame t0 + 1 [j]) of one row; a frame past T is zeros
template <int N>
__device__ __forceinline__ void mrl_load(const float* __restrict__ x, const MrlFrames& a, int t0, float2* z) {
    const long p0 = (long)t0 * a.hop - N / 2;
    const bool two = t0 + 1 < a.T;
#pragma unroll
    for (int j = threadIdx.x; j < N; j += MRL_THREADS) {
        const float w = a.window[j];
        const float u = w * x[mrl_reflect(p0 + j, a.n)];
        const float v = two ? w * x[mrl_reflect(p0 + a.hop + j, a.n)] : 0.f;
        z[j] = make_float2(u, v);
    }
}

// one radix-2 butterfly: decimation in frequency (p, q) -> (p + q, (p - q) (cos - i sin)); decimation in time, inverse direction,
// (p, q) -> (p + t, p - t) with t = q (cos + i sin)
__device__ __forceinline__ void mrl_dif2(float2& p, float2& q, MrlCs w) {
    const float dr = p.x - q.x, di = p.y - q.y;
    p = make_float2(p.x + q.x, p.y + q.y);
    q = make_float2(fmaf(dr, w.c, di * w.s), fmaf(di, w.c, -(dr * w.s)));
}
__device__ __forceinline__ void mrl_dit2(float2& p, float2& q, MrlCs w) {
    const float tr = fmaf(q.x, w.c, -(q.y * w.s)), ti = fmaf(q.x, w.s, q.y * w.c);
    q = make_float2(p.x - tr, p.y - ti);
    p = make_float2(p.x + tr, p.y + ti);
}

// one radix-2 stage of span 2 H over NB transforms of N points side by side (the odd stage of a size with an odd log2)
template <int N, int NB, int H, bool INVERSE>
__device__ __forceinline__ void mrl_stage2(float2* z, const MrlCs* tw) {
    constexpr int HALF = N / 2, WORK = NB * HALF, TRIPS = (WORK + MRL_THREADS - 1) / MRL_THREADS;
    float2 p[TRIPS], q[TRIPS];
    MrlCs w[TRIPS];
    int at[TRIPS];
    __syncthreads();
#pragma unroll
    for (int it = 0; it < TRIPS; ++it) {
        const int b = threadIdx.x + it * MRL_THREADS;
        const int bb = b & (HALF - 1), idx = bb & (H - 1);
        at[it] = ((bb - idx) << 1) + idx + (b - bb) * 2;
        if (WORK % MRL_THREADS == 0 || b < WORK) {
            p[it] = z[at[it]];
            q[it] = z[at[it] + H];
            w[it] = tw[H + idx];
        }
    }
#pragma unroll
    for (int it = 0; it < TRIPS; ++it) {
        if (WORK % MRL_THREADS == 0 || (int)threadIdx.x + it * MRL_THREADS < WORK) {
            if (INVERSE) mrl_dit2(p[it], q[it], w[it]);
            else mrl_dif2(p[it], q[it], w[it]);
            z[at[it]] = p[it];
            z[at[it] + H] = q[it];
        }
    }
}

// Two radix-2 stages in one pass over LDS: a thread holds the four points base + {0, Q, 2 Q, 3 Q} of a group of 4 Q.  Forward
// (decimation in frequency) the stage of span 4 Q pairs (0, 2 Q) and (Q, 3 Q), then the stage of span 2 Q pairs (0, Q) and (2 Q, 3 Q);
// the inverse (decimation in time) runs the spans in the other order.  The arithmetic is that of the two stages one after the other,
// bit for bit; the pass halves the barriers, the LDS traffic and the index arithmetic per point.
template <int N, int NB, int Q, bool INVERSE>
__device__ __forceinline__ void mrl_stage4(float2* z, const MrlCs* tw) {
    constexpr int QUART = N / 4, WORK = NB * QUART, TRIPS = (WORK + MRL_THREADS - 1) / MRL_THREADS;
    float2 v[TRIPS][4];
    MrlCs wa[TRIPS], wb[TRIPS], wc[TRIPS];
    int at[TRIPS];
    __syncthreads();
#pragma unroll
    for (int it = 0; it < TRIPS; ++it) {
        const int b = threadIdx.x + it * MRL_THREADS;
        const int bb = b & (QUART - 1), idx = bb & (Q - 1);
        at[it] = ((bb - idx) << 2) + idx + (b - bb) * 4;
        if (WORK % MRL_THREADS == 0 || b < WORK) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[it][j] = z[at[it] + j * Q];
            wa[it] = tw[2 * Q + idx];              // span 4 Q: the pair (0, 2 Q)
            wb[it] = tw[2 * Q + idx + Q];          //           the pair (Q, 3 Q)
            wc[it] = tw[Q + idx];                  // span 2 Q: both pairs
        }
    }
#pragma unroll
    for (int it = 0; it < TRIPS; ++it) {
        if (WORK % MRL_THREADS == 0 || (int)threadIdx.x + it * MRL_THREADS < WORK) {
            if (INVERSE) {
                mrl_dit2(v[it][0], v[it][1], wc[it]);
                mrl_dit2(v[it][2], v[it][3], wc[it]);
                mrl_dit2(v[it][0], v[it][2], wa[it]);
                mrl_dit2(v[it][1], v[it][3], wb[it]);
            } else {
                mrl_dif2(v[it][0], v[it][2], wa[it]);
                mrl_dif2(v[it][1], v[it][3], wb[it]);
                mrl_dif2(v[it][0], v[it][1], wc[it]);
                mrl_dif2(v[it][2], v[it][3], wc[it]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) z[at[it] + j * Q] = v[it][j];
        }
    }
}

template <int N, int NB, int Q, bool INVERSE>
struct MrlPasses {      // the passes of quarter Q, Q / 4 .. 1 forward; 1, 4 .. Q inverse
    static __device__ __forceinline__ void run(float2* z, const MrlCs* tw) {
        if (!INVERSE) mrl_stage4<N, NB, Q, false>(z, tw);
        if (Q >= 4) MrlPasses<N, NB, Q / 4, INVERSE>::run(z, tw);
        if (INVERSE) mrl_stage4<N, NB, Q, true>(z, tw);
    }
};
template <int N, int NB, bool INVERSE>
struct MrlPasses<N, NB, 0, INVERSE> {
    static __device__ __forceinline__ void run(float2*, const MrlCs*) {}
};

// NB transforms of N points side by side in z, forward, natural order in, bit-reversed out; ends with a barrier.  Every size is its own
// instantiation: a pass's points of one thread are loaded together, computed, and stored together (a loop with run-time bounds did one
// butterfly per trip, each behind its own twiddle load from global memory: 127 us per resolution at [32, 1, 32000]).  An odd log2 N
// takes its single radix-2 stage first (span N).
template <int N, int LG, int NB>
__device__ __forceinline__ void mrl_fft_dif(float2* z, const MrlCs* tw) {
    if (LG % 2) {
        mrl_stage2<N, NB, N / 2, false>(z, tw);
        MrlPasses<N, NB, N / 8, false>::run(z, tw);
    } else {
        MrlPasses<N, NB, N / 4, false>::run(z, tw);
    }
    __syncthreads();
}

// one unnormalised inverse transform of N points, bit-reversed in, natural order out; ends with a barrier: the forward's passes backwards
template <int N, int LG>
__device__ __forceinline__ void mrl_ifft_dit(float2* z, const MrlCs* tw) {
    if (LG % 2) {
        MrlPasses<N, 1, N / 8, true>::run(z, tw);
        mrl_stage2<N, 1, N / 2, true>(z, tw);
    } else {
        MrlPasses<N, 1, N / 4, true>::run(z, tw);
    }
    __syncthreads();
}

// the spectra of the two real frames packed in Z, at bin k: A from the real parts, B from the imaginary parts
__device__ __forceinline__ void mrl_split(float2 zk, float2 zm, float2& A, float2& B) {
    A = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
    B = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
}

__device__ __forceinline__ float mrl_mag(float2 v, float& P) {
    P = fmaf(v.x, v.x, v.y * v.y);
    return sqrtf(fmaxf(P, MRL_CLAMP));
}

extern __shared__ __align__(16) float2 mrl_lds[];

// The work of one workgroup of frames<MODE>: the enhanced frames of `row` against the clean frames of `src_row`, with the backward factors
// `stats` of that pairing (<1>); partial sums and gradients are stored under `row`.  frames<0 .. 2> pair a row with itself; the backward
// pass of the permutation-invariant loss reads the pairing from the permutation.
template <int MODE, int LG>
__device__ __forceinline__ void mrl_frames_body(const MrlFrames& a, int row, int src_row, const float* __restrict__ stats) {
    // twiddles [N]; <0>, <1>: enhanced pair [N], clean pair [N], 16 floats   <2>: one pair [N]
    constexpr int N = 1 << LG;
    const int t0 = 2 * blockIdx.x, tid = threadIdx.x;
    const bool two = t0 + 1 < a.T;
    MrlCs* tw = (MrlCs*)mrl_lds;
    float2* zx = mrl_lds + N;
    float2* zy = mrl_lds + 2 * N;
    for (int j = tid; j < N; j += MRL_THREADS) tw[j] = g_mrl_tw.w[j];
    mrl_load<N>(a.enh + (size_t)row * a.n, a, t0, zx);
    if (MODE != 2) mrl_load<N>(a.src + (size_t)src_row * a.n, a, t0, zy);
    mrl_fft_dif<N, LG, MODE == 2 ? 1 : 2>(zx, tw);

    float sA = 0.f, sB = 0.f, sC = 0.f, ksc = 0.f, kmag = 0.f;
    if (MODE == 1) {
        const float g = a.gout[0];
        ksc = g * a.ksc * stats[0];
        kmag = g * a.kmag * stats[1];
    }
    for (int k = tid; k <= N / 2; k += MRL_THREADS) {
        const int p = (int)(__brev((unsigned)k) >> (32 - LG)), q = (int)(__brev((unsigned)((N - k) & (N - 1))) >> (32 - LG));
        float2 X[2], Y[2];
        mrl_split(zx[p], zx[q], X[0], X[1]);
        if (MODE == 2) {
            float P;
            float* o = a.out + ((size_t)row * (N / 2 + 1) + k) * a.T + t0;
            o[0] = mrl_mag(X[0], P);
            if (two) o[1] = mrl_mag(X[1], P);
            continue;
        }
        mrl_split(zy[p], zy[q], Y[0], Y[1]);
        float2 H[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            float Px, Py;
            const float Mx = mrl_mag(X[f], Px), My = mrl_mag(Y[f], Py);
            const float d = My - Mx, l = logf(My) - logf(Mx);
            if (MODE == 0) {
                if (f == 0 || two) {
                    sA = fmaf(d, d, sA);
                    sB = fmaf(My, My, sB);
                    sC += fabsf(l);
                }
            } else {
                // dL / dX = ksc (X - Y) + kmag sign(log X - log Y) / X; through the clamp and the square root: (dL / dX) / X times (re, im)
                const float sg = l < 0.f ? 1.f : (l > 0.f ? -1.f : 0.f);
                const float dM = fmaf(ksc, -d, kmag * sg / Mx);
                const float c = Px >= MRL_CLAMP ? dM / Mx : 0.f;       // (a frame past T is zeros: clamped)
                const bool edge = k == 0 || k == N / 2;
                H[f] = edge ? make_float2(c * X[f].x, 0.f) : make_float2(0.5f * c * X[f].x, 0.5f * c * X[f].y);
            }
        }
        if (MODE == 1) {   // H(t0) + i H(t0 + 1) at bin k and, conjugated halves, at bin N - k; this thread is the only reader of p and q
            zx[p] = make_float2(H[0].x - H[1].y, H[0].y + H[1].x);
            if (q != p) zx[q] = make_float2(H[0].x + H[1].y, H[1].x - H[0].y);
        }
    }
    if (MODE == 0) {
        float* red = (float*)(mrl_lds + 3 * N);
        sA = wave_sum(sA);
        sB = wave_sum(sB);
        sC = wave_sum(sC);
        if ((tid & 63) == 0) {
            red[(tid >> 6) * 3 + 0] = sA;
            red[(tid >> 6) * 3 + 1] = sB;
            red[(tid >> 6) * 3 + 2] = sC;
        }
        __syncthreads();
        if (tid < 3) {
            float* o = a.partials + ((size_t)row * gridDim.x + blockIdx.x) * 3;
            o[tid] = ((red[tid] + red[3 + tid]) + red[6 + tid]) + red[9 + tid];
        }
    }
    if (MODE == 1) {
        mrl_ifft_dit<N, LG>(zx, tw);
        const int lp = (N - a.win) / 2;
        float* o = a.out + ((size_t)row * a.T + t0) * a.win;
        for (int u = tid; u < a.win; u += MRL_THREADS) {
            const float w = a.window[lp + u];
            const float2 v = zx[lp + u];
            o[u] = w * v.x;
            if (two) o[a.win + u] = w * v.y;
        }
    }
}

template <int MODE, int LG>
__global__ __launch_bounds__(MRL_THREADS) void mrl_frames_kernel(MrlFrames a) {
    mrl_frames_body<MODE, LG>(a, blockIdx.y, blockIdx.y, a.stats);
}

struct MrlFinal {
    int n_res;
    int off[MRL_MAX_RES], blocks[MRL_MAX_RES];     // partial triples of resolution r: [off, off + blocks)
    double cells[MRL_MAX_RES];                     // rows (n_fft / 2 + 1) T
    float scw, magw;
};

constexpr int MRL_FIN_THREADS = 1024;
__global__ __launch_bounds__(MRL_FIN_THREADS) void mrl_finalize_kernel(const float* __restrict__ partials, MrlFinal f,
                                                                       float* __restrict__ stats, float* __restrict__ terms,
                                                                       float* __restrict__ loss) {
    __shared__ double red[3][MRL_FIN_THREADS / 64];
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int r = 0; r < f.n_res; ++r) {
        const float* p = partials + (size_t)f.off[r] * 3;
        double s[3] = {0.0, 0.0, 0.0};
#pragma unroll 4
        for (int i = tid; i < f.blocks[r]; i += MRL_FIN_THREADS) {
            s[0] += (double)p[(size_t)i * 3];
            s[1] += (double)p[(size_t)i * 3 + 1];
            s[2] += (double)p[(size_t)i * 3 + 2];
        }
        __syncthreads();                           // (red of the previous resolution has been read)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            s[j] = wave_sum_d(s[j]);
            if ((tid & 63) == 0) red[j][tid >> 6] = s[j];
        }
        __syncthreads();
        if (tid == 0) {
            double v[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                v[j] = red[j][0];
                for (int w = 1; w < MRL_FIN_THREADS / 64; ++w) v[j] += red[j][w];
            }
            const double na = sqrt(v[0]), nb = sqrt(v[1]);
            const double sc = na / nb, mag = v[2] / f.cells[r];
            terms[2 * r] = (float)sc;
            terms[2 * r + 1] = (float)mag;
            stats[2 * r] = v[0] > 0.0 ? (float)(1.0 / (na * nb)) : 0.f;
            stats[2 * r + 1] = (float)(1.0 / f.cells[r]);
            total += (double)f.scw * sc + (double)f.magw * mag;
        }
    }
    if (tid == 0) loss[0] = (float)(total / f.n_res);
}

// grad[row][s] (+)= the frame gradients at the padded positions that read sample s: s itself and its mirror images -s and 2 (n - 1) - s
__global__ __launch_bounds__(256) void mrl_gather_kernel(const float* __restrict__ fgrad, long n, int T, int n_fft, int hop, int win,
                                                         int accumulate, float* __restrict__ grad) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const int row = blockIdx.y;
    const float* f = fgrad + (size_t)row * T * win;
    const long base = n_fft / 2 - (n_fft - win) / 2;             // padded position p is offset p + base of frame 0's window
    float acc = 0.f;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        if ((m == 1 && s == 0) || (m == 2 && s == n - 1)) continue;
        const long u = (m == 0 ? s : (m == 1 ? -s : 2 * (n - 1) - s)) + base;
        if (u < 0) continue;
        const long lo = u - win + 1 > 0 ? (u - win + hop) / hop : 0;      // frames t with 0 <= u - t hop < win, ascending
        const long hi = u / hop < T - 1 ? u / hop : T - 1;
        for (long t = lo; t <= hi; ++t) acc += f[(size_t)t * win + (u - t * hop)];
    }
    float* o = grad + (size_t)row * n + s;
    *o = accumulate ? *o + acc : acc;
}

int mrl_check(const char* who, int rows, long n, int n_fft, int hop, int win) {
    SEHIP_REQUIRE(n_fft >= MRL_MIN_NFFT && n_fft <= MRL_MAX_NFFT && (n_fft & (n_fft - 1)) == 0,
                  "%s: n_fft=%d is not a power of two in [%d, %d]", who, n_fft, MRL_MIN_NFFT, MRL_MAX_NFFT);
    SEHIP_REQUIRE(win >= 1 && win <= n_fft, "%s: win_length=%d outside [1, n_fft=%d]", who, win, n_fft);
    SEHIP_REQUIRE(hop >= 1 && hop <= win, "%s: hop=%d outside [1, win_length=%d]", who, hop, win);
    SEHIP_REQUIRE(n > n_fft / 2 && n <= MRL_MAX_LEN, "%s: n=%ld samples outside (n_fft / 2 = %d, 2^30]: the reflect padding needs more than n_fft / 2",
                  who, n, n_fft / 2);
    SEHIP_REQUIRE(rows >= 1 && rows <= MRL_MAX_ROWS, "%s: rows=%d outside [1, %d]", who, rows, MRL_MAX_ROWS);
    return 0;
}

// The one dispatch from n_fft to LG = log2(n_fft), a kernel's template argument: f is called with std::integral_constant<int, LG>, so
// every launch of this file has one instantiation per transform size (mrl_check has run: n_fft is a power of two in [64, 2048]).
template <class F>
auto mrl_dispatch(int n_fft, F&& f) {
    switch (n_fft) {
        case 64: return f(std::integral_constant<int, 6>{});
        case 128: return f(std::integral_constant<int, 7>{});
        case 256: return f(std::integral_constant<int, 8>{});
        case 512: return f(std::integral_constant<int, 9>{});
        case 1024: return f(std::integral_constant<int, 10>{});
        default: return f(std::integral_constant<int, 11>{});      // 2048
    }
}

template <int MODE>
void mrl_launch(const MrlFrames& a, int rows, hipStream_t st) {
    const dim3 grid((a.T + 1) / 2, rows);
    const size_t lds = (size_t)(MODE == 2 ? 2 : 3) * a.n_fft * sizeof(float2) + (MODE == 0 ? 16 * sizeof(float) : 0);
    mrl_dispatch(a.n_fft, [&](auto lg) { mrl_frames_kernel<MODE, decltype(lg)::value><<<grid, MRL_THREADS, lds, st>>>(a); });
}

MrlFrames mrl_args(const float* enh, const float* src, const float* window, long n, int n_fft, int hop, int win) {
    MrlFrames a{};
    a.enh = enh;
    a.src = src;
    a.window = window;
    a.n = n;
    a.T = (int)(1 + n / hop);
    a.n_fft = n_fft;
    a.hop = hop;
    a.win = win;
    return a;
}

// ---- the permutation-invariant form (sehip.loss.pit_mrstft_loss): enh / src [B][S][C][n], speakers on axis 1 -----------------------------
// Pair (i, j) is estimated speaker i against target speaker j, its norms and mean taken over the B C rows.  A pair needs the magnitudes of
// two signals out of 2 S, so a workgroup transforms each of them once and fills every pair from there.
struct MrlPair {
    MrlFrames f;           // f.enh / f.src: [B][S][C][n]; f.partials: the sums of one resolution, [2 S S + S][nblk]
    int S, C;
    long nblk;             // B C workgroups of frame pairs: index (b C + c) pairs + pair, the order of frames<0> on the slices
};
constexpr int MRLP_RED = 2 * PIT_MAXS;      // partial sums of one signal: sum (Y_j - X)^2 and sum |log Y_j - log X| for every target j

// the workgroup's sum of each of vals[v], v = t PIT_MAXS + j with j < S, in the order of frames<0> (wave_sum, then the four waves in
// index order), stored at out[(base[t] + j) nblk]
__device__ __forceinline__ void mrlp_reduce(const float (&vals)[MRLP_RED], int kinds, int S, float* red, float* out, int base0, int base1,
                                            long nblk) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int v = 0; v < MRLP_RED; ++v) {
        if (v / PIT_MAXS < kinds && v % PIT_MAXS < S) {
            const float x = wave_sum(vals[v]);
            if ((tid & 63) == 0) red[(tid >> 6) * MRLP_RED + v] = x;
        }
    }
    __syncthreads();
    if (tid < MRLP_RED && tid / PIT_MAXS < kinds && tid % PIT_MAXS < S) {
        const int at = (tid < PIT_MAXS ? base0 : base1) + tid % PIT_MAXS;
        out[(size_t)at * nblk] = ((red[tid] + red[MRLP_RED + tid]) + red[2 * MRLP_RED + tid]) + red[3 * MRLP_RED + tid];
    }
    __syncthreads();                                  // (red is written again by the next signal)
}

// signals per transform pass: two side by side where one alone would leave threads without a butterfly (n_fft / 4 < 256), one from 1024
// on -- the same arithmetic, and 8 n_fft bytes of LDS less, which is a workgroup more per CU at 1024 and at 2048 with two speakers
constexpr int mrlp_nb(int n_fft) { return n_fft >= 1024 ? 1 : 2; }

// One workgroup per (b, c, frame pair t0, t0 + 1).  The 2 S signals of that (b, c) -- targets first -- go through the transform of
// frames<0> mrlp_nb at a time.  A target leaves (Y(t0), Y(t0 + 1), log Y(t0), log Y(t0 + 1)) per bin in LDS and its sum Y^2; an estimate is
// taken against every target in LDS as it comes out of the transform.  Thread, bin and frame order of every sum are those of frames<0>
// on (enh[:, i], src[:, j]), so the partial sums carry the same bits.  A thread reads back only the bins it wrote itself.
// LDS: twiddles [N], the signals in the transform [mrlp_nb N] (float2), targets [S][N / 2 + 1] (float4), 4 x 12 floats: 131,360 B at
// N = 2048, S = 6; 65,760 B at N = 2048, S = 2.
template <int LG>
__global__ __launch_bounds__(MRL_THREADS) void mrl_pair_fwd_kernel(MrlPair a) {
    constexpr int N = 1 << LG, BINS = N / 2 + 1, NB = mrlp_nb(N);
    const MrlFrames& f = a.f;
    const int S = a.S, row = blockIdx.y, b = row / a.C, c = row - b * a.C, t0 = 2 * blockIdx.x, tid = threadIdx.x;
    const bool two = t0 + 1 < f.T;
    MrlCs* tw = (MrlCs*)mrl_lds;
    float2* z = mrl_lds + N;
    float4* ymag = (float4*)(mrl_lds + (1 + NB) * N);
    float* red = (float*)(ymag + (size_t)S * BINS);
    float* out = f.partials + (size_t)row * gridDim.x + blockIdx.x;
    for (int j = tid; j < N; j += MRL_THREADS) tw[j] = g_mrl_tw.w[j];
    for (int g0 = 0; g0 < 2 * S; g0 += NB) {
        if (g0) __syncthreads();                      // (every read of the signals before)
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            const int g = g0 + s, spk = g < S ? g : g - S;
            mrl_load<N>((g < S ? f.src : f.enh) + (((size_t)b * S + spk) * a.C + c) * f.n, f, t0, z + s * N);
        }
        mrl_fft_dif<N, LG, NB>(z, tw);
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            const int g = g0 + s;
            const float2* zs = z + s * N;
            float vals[MRLP_RED];
#pragma unroll
            for (int v = 0; v < MRLP_RED; ++v) vals[v] = 0.f;
            if (g < S) {
                float4* ym = ymag + (size_t)g * BINS;
                for (int k = tid; k <= N / 2; k += MRL_THREADS) {
                    const int p = (int)(__brev((unsigned)k) >> (32 - LG)), q = (int)(__brev((unsigned)((N - k) & (N - 1))) >> (32 - LG));
                    float2 Y[2];
                    float P;
                    mrl_split(zs[p], zs[q], Y[0], Y[1]);
                    const float M0 = mrl_mag(Y[0], P), M1 = mrl_mag(Y[1], P);
                    ym[k] = make_float4(M0, M1, logf(M0), logf(M1));
                    vals[0] = fmaf(M0, M0, vals[0]);
                    if (two) vals[0] = fmaf(M1, M1, vals[0]);
                }
                mrlp_reduce(vals, 1, 1, red, out, 2 * S * S + g, 0, a.nblk);
            } else {
                for (int k = tid; k <= N / 2; k += MRL_THREADS) {
                    const int p = (int)(__brev((unsigned)k) >> (32 - LG)), q = (int)(__brev((unsigned)((N - k) & (N - 1))) >> (32 - LG));
                    float2 X[2];
                    float P;
                    mrl_split(zs[p], zs[q], X[0], X[1]);
                    const float M0 = mrl_mag(X[0], P), M1 = mrl_mag(X[1], P);
                    const float L0 = logf(M0), L1 = logf(M1);
#pragma unroll
                    for (int j = 0; j < PIT_MAXS; ++j) {
                        if (j < S) {
                            const float4 y = ymag[(size_t)j * BINS + k];
                            const float d0 = y.x - M0, l0 = y.z - L0;
                            vals[j] = fmaf(d0, d0, vals[j]);
                            vals[PIT_MAXS + j] += fabsf(l0);
                            if (two) {
                                const float d1 = y.y - M1, l1 = y.w - L1;
                                vals[j] = fmaf(d1, d1, vals[j]);
                                vals[PIT_MAXS + j] += fabsf(l1);
                            }
                        }
                    }
                }
                mrlp_reduce(vals, 2, S, red, out, (g - S) * S, S * S + (g - S) * S, a.nblk);
            }
        }
    }
}

struct MrlPairFinal {
    int n_res, S;
    long off[MRL_MAX_RES];                         // floats in front of resolution r's sums
    int nblk[MRL_MAX_RES];
    double cells[MRL_MAX_RES];                     // B C (n_fft / 2 + 1) T
    float scw, magw, extra_weight;
};

// One workgroup.  Every sum is taken as finalize takes it -- thread q of 1024 adds the records q, q + 1024, .., the xor tree of a wave, the
// 16 waves in index order, all in double -- so sc, mag carry finalize's bits; a thread carries MRLP_VC sums at a time to keep that many
// loads of a trip in flight (one workgroup reads every record: the launch is bound by the latency of those loads).  Then
// matrix[i][j] = (1 / R) sum_r (scw sc + magw mag) (+ extra_weight extra[i][j]), the walk over the permutations, the loss
// (1 / S) sum_j matrix[perm[j]][j] in fp32 and, per (resolution, target j), the backward factors of the matched pair.
constexpr int MRLP_VC = 8;
__global__ __launch_bounds__(MRL_FIN_THREADS) void mrl_pair_select_kernel(const float* __restrict__ partials, MrlPairFinal f,
                                                                          const float* __restrict__ extra, float* __restrict__ terms,
                                                                          float* __restrict__ matrix, int* __restrict__ perm,
                                                                          float* __restrict__ loss, float* __restrict__ stats) {
    constexpr int SS_MAX = PIT_MAXS * PIT_MAXS, NV_MAX = 2 * SS_MAX + PIT_MAXS, WAVES = MRL_FIN_THREADS / 64;
    __shared__ double red[NV_MAX][WAVES];
    __shared__ double sums[NV_MAX];
    __shared__ float inv[MRL_MAX_RES][SS_MAX];
    __shared__ float m[SS_MAX];
    const int tid = threadIdx.x, S = f.S, SS = S * S, NV = 2 * SS + S;
    double total = 0.0;                            // thread i S + j: pair (i, j)
    for (int r = 0; r < f.n_res; ++r) {
        const int nblk = f.nblk[r];
        for (int v0 = 0; v0 < NV; v0 += MRLP_VC) {
            const float* p = partials + f.off[r] + (size_t)v0 * nblk;
            double acc[MRLP_VC];
#pragma unroll
            for (int u = 0; u < MRLP_VC; ++u) acc[u] = 0.0;
#pragma unroll 2
            for (int i = tid; i < nblk; i += MRL_FIN_THREADS) {
#pragma unroll
                for (int u = 0; u < MRLP_VC; ++u)
                    if (v0 + u < NV) acc[u] += (double)p[(size_t)u * nblk + i];
            }
#pragma unroll
            for (int u = 0; u < MRLP_VC; ++u) {
                if (v0 + u < NV) {
                    const double x = wave_sum_d(acc[u]);
                    if ((tid & 63) == 0) red[v0 + u][tid >> 6] = x;
                }
            }
        }
        __syncthreads();
        if (tid < NV) {
            double x = red[tid][0];
            for (int w = 1; w < WAVES; ++w) x += red[tid][w];
            sums[tid] = x;
        }
        __syncthreads();
        if (tid < SS) {
            const double v0 = sums[tid], v1 = sums[2 * SS + tid % S], v2 = sums[SS + tid];
            const double na = sqrt(v0), nb = sqrt(v1);
            const double sc = na / nb, mag = v2 / f.cells[r];
            terms[((size_t)r * SS + tid) * 2] = (float)sc;
            terms[((size_t)r * SS + tid) * 2 + 1] = (float)mag;
            inv[r][tid] = v0 > 0.0 ? (float)(1.0 / (na * nb)) : 0.f;
            total += (double)f.scw * sc + (double)f.magw * mag;
        }
        __syncthreads();                           // (sums is written again by the next resolution)
    }
    if (tid < SS) {
        float v = (float)(total / f.n_res);
        if (extra) v = v + f.extra_weight * extra[tid];
        m[tid] = v;
        matrix[tid] = v;
    }
    __syncthreads();
    if (tid != 0) return;
    int best[PIT_MAXS];
    pit_best_permutation(m, S, best);
    float tot = 0.f;
    for (int j = 0; j < S; ++j) {
        perm[j] = best[j];
        tot += m[best[j] * S + j];
    }
    loss[0] = tot / S;
    for (int r = 0; r < f.n_res; ++r)
        for (int j = 0; j < S; ++j) {
            stats[((size_t)r * S + j) * 2] = inv[r][best[j] * S + j];
            stats[((size_t)r * S + j) * 2 + 1] = (float)(1.0 / f.cells[r]);
        }
}

// frames<1> with the pairing read from the permutation: grid (frame pairs, B C, S); estimated speaker i = blockIdx.z goes against the
// target j with perm[j] == i and that target's factors stats[j][2]; fgrad in the order of the estimate's rows, (b S + i) C + c
template <int LG>
__global__ __launch_bounds__(MRL_THREADS) void mrl_pair_bwd_kernel(MrlFrames a, const int* __restrict__ perm, int S, int C) {
    const int i = blockIdx.z, b = blockIdx.y / C, c = blockIdx.y - b * C;
    int j = 0;
    for (int k = 0; k < S; ++k)
        if (perm[k] == i) j = k;
    mrl_frames_body<1, LG>(a, (b * S + i) * C + c, (b * S + j) * C + c, a.stats + 2 * j);
}

int mrl_pair_rows_check(const char* who, int B, int S, int C) {
    SEHIP_REQUIRE(S >= 1 && S <= PIT_MAXS, "%s: S=%d speakers outside [1, %d]", who, S, PIT_MAXS);
    SEHIP_REQUIRE(B >= 1 && C >= 1 && (long)B * C <= MRL_MAX_ROWS, "%s: rows=%ld (B=%d times C=%d) outside [1, %d]", who, (long)B * C, B, C,
                  MRL_MAX_ROWS);
    return 0;
}

int mrl_pair_check(const char* who, int B, int S, int C, long n, int n_fft, int hop, int win) {
    if (int e = mrl_pair_rows_check(who, B, S, C)) return e;
    return mrl_check(who, B * C, n, n_fft, hop, win);
}

size_t mrl_pair_lds(int S, int n_fft) {
    return (size_t)(1 + mrlp_nb(n_fft)) * n_fft * sizeof(float2) + (size_t)S * (n_fft / 2 + 1) * sizeof(float4) + 4 * MRLP_RED * sizeof(float);
}

template <int LG>
int mrl_pair_launch_fwd(const MrlPair& a, const dim3& grid, size_t lds, hipStream_t st) {
    static bool attr = false;                      // a workgroup with six targets at 2048 takes more than the 64 KB a launch gets unasked
    if (!attr) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mrl_pair_fwd_kernel<LG>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        SEHIP_REQUIRE(e == hipSuccess, "mrl_pair_forward: hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr = true;
    }
    mrl_pair_fwd_kernel<LG><<<grid, MRL_THREADS, lds, st>>>(a);
    return 0;
}
}  // namespace

extern "C" long sehip_mrl_frames(long n, int hop) { return hop >= 1 && n >= 1 ? 1 + n / hop : 0; }

extern "C" long sehip_mrl_blocks(long n, int hop) { return hop >= 1 && n >= 1 ? (1 + n / hop + 1) / 2 : 0; }

extern "C" int sehip_mrl_check(int n_res, const int* res, int rows, long n) {
    SEHIP_REQUIRE(n_res >= 1 && n_res <= MRL_MAX_RES, "mrl_check: resolutions=%d outside [1, %d]", n_res, MRL_MAX_RES);
    SEHIP_REQUIRE(res, "mrl_check: null pointer");
    for (int r = 0; r < n_res; ++r)
        if (int e = mrl_check("mrl_check", rows, n, res[3 * r], res[3 * r + 1], res[3 * r + 2])) return e;
    return 0;
}

extern "C" int sehip_mrl_forward(const float* enh, const float* src, int rows, long n, int n_fft, int hop, int win, const float* window,
                                 float* partials, void* stream) {
    if (int e = mrl_check("mrl_forward", rows, n, n_fft, hop, win)) return e;
    SEHIP_REQUIRE(enh && src && window && partials, "mrl_forward: null pointer");
    MrlFrames a = mrl_args(enh, src, window, n, n_fft, hop, win);
    a.partials = partials;
    mrl_launch<0>(a, rows, (hipStream_t)stream);
    SEHIP_CHECK_LAUNCH("mrl_forward");
    sehip_note_kernel("mrl_forward n_fft=%d T=%d", n_fft, a.T);
    return 0;
}

extern "C" int sehip_mrl_finalize(const float* partials, int n_res, const int* res, int rows, long n, float sc_weight, float mag_weight,
                                  float* stats, float* terms, float* loss, void* stream) {
    if (int e = sehip_mrl_check(n_res, res, rows, n)) return e;
    SEHIP_REQUIRE(partials && stats && terms && loss, "mrl_finalize: null pointer");
    MrlFinal f{};
    f.n_res = n_res;
    f.scw = sc_weight;
    f.magw = mag_weight;
    long off = 0;
    for (int r = 0; r < n_res; ++r) {
        const long blocks = (long)rows * sehip_mrl_blocks(n, res[3 * r + 1]);
        SEHIP_REQUIRE(off + blocks < (1L << 31), "mrl_finalize: %ld partial sums are more than 2^31", off + blocks);
        f.off[r] = (int)off;
        f.blocks[r] = (int)blocks;
        f.cells[r] = (double)rows * (res[3 * r] / 2 + 1) * (double)sehip_mrl_frames(n, res[3 * r + 1]);
        off += blocks;
    }
    mrl_finalize_kernel<<<1, MRL_FIN_THREADS, 0, (hipStream_t)stream>>>(partials, f, stats, terms, loss);
    SEHIP_CHECK_LAUNCH("mrl_finalize");
    return 0;
}

extern "C" int sehip_mrl_backward(const float* enh, const float* src, int rows, long n, int n_fft, int hop, int win, const float* window,
                                  const float* stats, const float* gout, float sc_scale, float mag_scale, float* fgrad, void* stream) {
    if (int e = mrl_check("mrl_backward", rows, n, n_fft, hop, win)) return e;
    SEHIP_REQUIRE(enh && src && window && stats && gout && fgrad, "mrl_backward: null pointer");
    MrlFrames a = mrl_args(enh, src, window, n, n_fft, hop, win);
    a.stats = stats;
    a.gout = gout;
    a.ksc = sc_scale;
    a.kmag = mag_scale;
    a.out = fgrad;
    mrl_launch<1>(a, rows, (hipStream_t)stream);
    SEHIP_CHECK_LAUNCH("mrl_backward");
    sehip_note_kernel("mrl_backward n_fft=%d T=%d", n_fft, a.T);
    return 0;
}

extern "C" int sehip_mrl_gather(const float* fgrad, int rows, long n, int n_fft, int hop, int win, int accumulate, float* grad,
                                void* stream) {
    if (int e = mrl_check("mrl_gather", rows, n, n_fft, hop, win)) return e;
    SEHIP_REQUIRE(accumulate == 0 || accumulate == 1, "mrl_gather: accumulate=%d is neither 0 nor 1", accumulate);
    SEHIP_REQUIRE(fgrad && grad, "mrl_gather: null pointer");
    mrl_gather_kernel<<<dim3(cdiv(n, 256), rows), 256, 0, (hipStream_t)stream>>>(fgrad, n, (int)(1 + n / hop), n_fft, hop, win, accumulate,
                                                                               grad);
    SEHIP_CHECK_LAUNCH("mrl_gather");
    return 0;
}

extern "C" int sehip_mrl_magnitudes(const float* x, int rows, long n, int n_fft, int hop, int win, const float* window, float* out,
                                    void* stream) {
    if (int e = mrl_check("mrl_magnitudes", rows, n, n_fft, hop, win)) return e;
    SEHIP_REQUIRE(x && window && out, "mrl_magnitudes: null pointer");
    MrlFrames a = mrl_args(x, x, window, n, n_fft, hop, win);
    a.out = out;
    mrl_launch<2>(a, rows, (hipStream_t)stream);
    SEHIP_CHECK_LAUNCH("mrl_magnitudes");
    sehip_note_kernel("mrl_magnitudes n_fft=%d T=%d", n_fft, a.T);
    return 0;
}

// ---- the permutation-invariant form -------------------------------------------------------------------------------------------------------
extern "C" long sehip_mrl_pair_blocks(int B, int S, int C, long n, int hop) {
    if (B < 1 || C < 1 || S < 1 || S > PIT_MAXS || (long)B * C > MRL_MAX_ROWS) return 0;
    return (long)(2 * S * S + S) * B * C * sehip_mrl_blocks(n, hop);
}

extern "C" int sehip_mrl_pair_forward(const float* enh, const float* src, int B, int S, int C, long n, int n_fft, int hop, int win,
                                      const float* window, float* partials, void* stream) {
    if (int e = mrl_pair_check("mrl_pair_forward", B, S, C, n, n_fft, hop, win)) return e;
    SEHIP_REQUIRE(enh && src && window && partials, "mrl_pair_forward: null pointer");
    MrlPair a{};
    a.f = mrl_args(enh, src, window, n, n_fft, hop, win);
    a.f.partials = partials;
    a.S = S;
    a.C = C;
    const dim3 grid((a.f.T + 1) / 2, B * C);
    a.nblk = (long)grid.x * grid.y;
    const size_t lds = mrl_pair_lds(S, n_fft);
    hipStream_t st = (hipStream_t)stream;
    if (int e = mrl_dispatch(n_fft, [&](auto lg) { return mrl_pair_launch_fwd<decltype(lg)::value>(a, grid, lds, st); })) return e;
    SEHIP_CHECK_LAUNCH("mrl_pair_forward");
    sehip_note_kernel("mrl_pair_forward n_fft=%d T=%d S=%d lds=%zu", n_fft, a.f.T, S, lds);
    return 0;
}

extern "C" int sehip_mrl_pair_select(const float* partials, int n_res, const int* res, int B, int S, int C, long n, float sc_weight,
                                     float mag_weight, const float* extra, float extra_weight, float* terms, float* matrix, int* perm,
                                     float* loss, float* stats, void* stream) {
    if (int e = mrl_pair_rows_check("mrl_pair_select", B, S, C)) return e;
    if (int e = sehip_mrl_check(n_res, res, B * C, n)) return e;
    SEHIP_REQUIRE(partials && terms && matrix && perm && loss && stats, "mrl_pair_select: null pointer");
    MrlPairFinal f{};
    f.n_res = n_res;
    f.S = S;
    f.scw = sc_weight;
    f.magw = mag_weight;
    f.extra_weight = extra_weight;
    long off = 0;
    for (int r = 0; r < n_res; ++r) {
        const long nblk = (long)B * C * sehip_mrl_blocks(n, res[3 * r + 1]);
        SEHIP_REQUIRE(nblk <= (1L << 30), "mrl_pair_select: %ld workgroups of one resolution are more than 2^30", nblk);
        f.off[r] = off;
        f.nblk[r] = (int)nblk;
        f.cells[r] = (double)B * C * (res[3 * r] / 2 + 1) * (double)sehip_mrl_frames(n, res[3 * r + 1]);
        off += (long)(2 * S * S + S) * nblk;
    }
    mrl_pair_select_kernel<<<1, MRL_FIN_THREADS, 0, (hipStream_t)stream>>>(partials, f, extra, terms, matrix, perm, loss, stats);
    SEHIP_CHECK_LAUNCH("mrl_pair_select");
    return 0;
}

extern "C" int sehip_mrl_pair_backward(const float* enh, const float* src, int B, int S, int C, long n, int n_fft, int hop, int win,
                                       const float* window, const float* stats, const int* perm, const float* gout, float sc_scale,
                                       float mag_scale, float* fgrad, void* stream) {
    if (int e = mrl_pair_check("mrl_pair_backward", B, S, C, n, n_fft, hop, win)) return e;
    SEHIP_REQUIRE(enh && src && window && stats && perm && gout && fgrad, "mrl_pair_backward: null pointer");
    MrlFrames a = mrl_args(enh, src, window, n, n_fft, hop, win);
    a.stats = stats;
    a.gout = gout;
    a.ksc = sc_scale;
    a.kmag = mag_scale;
    a.out = fgrad;
    const dim3 grid((a.T + 1) / 2, B * C, S);
    const size_t lds = (size_t)3 * n_fft * sizeof(float2);
    hipStream_t st = (hipStream_t)stream;
    mrl_dispatch(n_fft, [&](auto lg) { mrl_pair_bwd_kernel<decltype(lg)::value><<<grid, MRL_THREADS, lds, st>>>(a, perm, S, C); });
    SEHIP_CHECK_LAUNCH("mrl_pair_backward");
    sehip_note_kernel("mrl_pair_backward n_fft=%d T=%d S=%d", n_fft, a.T, S);
    return 0;
}
