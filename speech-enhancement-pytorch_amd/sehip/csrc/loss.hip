// SI-SNR loss forward/backward (reference: src/loss.py:14-29 -- l2_norm, si_snr, loss_sisdr).
//
//   s_t   = <x,s>/(<s,s>+eps) * s          (no zero-mean, as in the reference)
//   e     = x - s_t
//   l_row = 10*log10( |s_t|^2 / (|e|^2 + eps) + eps )
//   loss  = -mean_rows(l_row)
//
// HBM-bound: one 256-thread workgroup per utterance row; the row is read twice (dot products, then the
// exact residual energy -- the second read hits L2), the backward is one fused a*(x - alpha*s) + b*s pass whose three
// row coefficients were produced by the forward.
#include "common.h"
#include "pit_perm.h"      // PIT_MAXS, pit_best_permutation

#define EPS 1e-8f

// e = x - alpha*s, rounded as a product and a difference in EVERY kernel that forms it.  The backward's a*e cancels against the
// 2 q <e, s> / (<s, s> + eps) * s part of b*s whenever e is all but parallel to s (a one-sample row is the extreme), and it does so
// only if its e is bit for bit the e whose <e, s> the forward summed: no contraction to an fma here, in one kernel and not in another.
__device__ __forceinline__ float sisnr_residual(float x, float alpha, float s) {
    float t = alpha * s;
    asm volatile("" : "+v"(t));   // (-ffp-contract=fast overrides a contract(off) pragma; the product is pinned in a register instead)
    return x - t;
}

// rowstat[r] = {a, b, l_row, alpha}; d loss / d x_j = upstream * (a*(x_j - alpha*s_j) + b*s_j): the residual e = x - alpha s is formed
// per element, as the forward and the reference's autograd form it.  Folding alpha into the coefficient of s (a*x + (b - a*alpha)*s)
// is the same polynomial, but its two terms are each |a| |x| large and cancel down to |a| |e|: at 40 / 60 dB the rounding of the
// folded form is 3 x the reference's own fp32 deviation from float64, and a one-sample row loses its gradient altogether.
// (1024 threads: a row is two dependent passes of one workgroup, 32 rows per step -- latency, not bandwidth: 23.6 us with 256 threads)
__global__ __launch_bounds__(1024) void sisnr_fwd_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                                                        int n, int rows, float4* __restrict__ rowstat) {
    __shared__ float red[16];
    const int r = blockIdx.x;
    const float* x = est + (size_t)r * n;
    const float* s = ref + (size_t)r * n;
    float xs = 0.f, ss = 0.f;
    const int n4 = n >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const float4* s4 = reinterpret_cast<const float4*>(s);
    const bool vec = ((n & 3) == 0) && ((((uintptr_t)x | (uintptr_t)s) & 15) == 0);
    if (vec) {
        for (int i = threadIdx.x; i < n4; i += 1024) {
            float4 a = x4[i], b = s4[i];
            xs += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
            ss += b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w;
        }
    } else {
        for (int i = threadIdx.x; i < n; i += 1024) { xs += x[i] * s[i]; ss += s[i] * s[i]; }
    }
    xs = block_sum<16>(xs, red);
    ss = block_sum<16>(ss, red);
    const float alpha = xs / (ss + EPS);
    float et = 0.f, en = 0.f, es = 0.f;
    if (vec) {
        for (int i = threadIdx.x; i < n4; i += 1024) {
            float4 a = x4[i], b = s4[i];
            float t0 = alpha * b.x, t1 = alpha * b.y, t2 = alpha * b.z, t3 = alpha * b.w;
            float e0 = sisnr_residual(a.x, alpha, b.x), e1 = sisnr_residual(a.y, alpha, b.y), e2 = sisnr_residual(a.z, alpha, b.z),
                  e3 = sisnr_residual(a.w, alpha, b.w);
            et += t0 * t0 + t1 * t1 + t2 * t2 + t3 * t3;
            en += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
            es += e0 * b.x + e1 * b.y + e2 * b.z + e3 * b.w;
        }
    } else {
        for (int i = threadIdx.x; i < n; i += 1024) {
            float t = alpha * s[i], e = sisnr_residual(x[i], alpha, s[i]);
            et += t * t; en += e * e; es += e * s[i];
        }
    }
    et = block_sum<16>(et, red);
    en = block_sum<16>(en, red);
    es = block_sum<16>(es, red);
    if (threadIdx.x == 0) {
        const float ratio = et / (en + EPS);
        const float l = 10.f * log10f(ratio + EPS);
        // d l / d ratio, with the -1/rows of loss = -mean folded in
        const float c = -(1.0f / rows) * 10.f / (2.302585092994046f * (ratio + EPS));
        const float q = et / ((en + EPS) * (en + EPS));
        const float a = c * (-2.f * q);
        const float b = c * (2.f * alpha * ss / ((ss + EPS) * (en + EPS)) + 2.f * q * es / (ss + EPS));
        rowstat[r] = make_float4(a, b, l, alpha);
    }
}

__global__ void sisnr_finalize_kernel(const float4* __restrict__ rowstat, int rows, float* __restrict__ loss) {
    // single wave, deterministic order
    float acc = 0.f;
    for (int i = threadIdx.x; i < rows; i += 64) acc += rowstat[i].z;
    acc = wave_sum(acc);
    if (threadIdx.x == 0) loss[0] = -acc / rows;
}

__global__ __launch_bounds__(256) void sisnr_bwd_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                                                        const float4* __restrict__ rowstat, const float* __restrict__ upstream,
                                                        int n, float* __restrict__ dest) {
    const int r = blockIdx.y;
    const float4 st = rowstat[r];
    const float up = upstream ? upstream[0] : 1.f;
    const float a = st.x * up, b = st.y * up, alpha = st.w;
    const size_t base = (size_t)r * n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float s = ref[base + i];
        dest[base + i] = a * sisnr_residual(est[base + i], alpha, s) + b * s;
    }
}

// SI-SDR validation metric (src/metric.py:92-123, SI_SDR): per row alpha = <e,r> / (<r,r> + eps), ratio = |alpha r|^2 /
// (|e - alpha r|^2 + eps); result 10 log10(mean_rows(ratio) + eps) with eps = float32 machine epsilon (np.finfo of the
// reference's float32 arrays).  Same two-pass row kernel as the loss; ratios[rows] is scratch.
#define SDR_EPS 1.1920929e-07f
__global__ __launch_bounds__(256) void sisdr_metric_kernel(const float* __restrict__ ref, const float* __restrict__ est, int n,
                                                           float* __restrict__ ratios) {
    __shared__ float red[4];
    const int r = blockIdx.x;
    const float* s = ref + (size_t)r * n;
    const float* x = est + (size_t)r * n;
    float xs = 0.f, ss = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { xs += x[i] * s[i]; ss += s[i] * s[i]; }
    xs = block_sum<4>(xs, red);
    ss = block_sum<4>(ss, red);
    const float alpha = xs / (ss + SDR_EPS);
    float et = 0.f, en = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float t = alpha * s[i], e = x[i] - t;
        et += t * t; en += e * e;
    }
    et = block_sum<4>(et, red);
    en = block_sum<4>(en, red);
    if (threadIdx.x == 0) ratios[r] = et / (en + SDR_EPS);
}

__global__ void sisdr_metric_finalize_kernel(const float* __restrict__ ratios, int rows, float* __restrict__ out) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < rows; i += 64) acc += ratios[i];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) out[0] = 10.f * log10f(acc / rows + SDR_EPS);
}

extern "C" int sehip_sisdr_metric(const float* reference, const float* estimation, int rows, int n, float* ratios, float* out,
                                  void* stream) {
    SEHIP_REQUIRE(rows > 0 && n > 0, "sisdr_metric: empty input (rows=%d n=%d)", rows, n);
    hipStream_t st = (hipStream_t)stream;
    sisdr_metric_kernel<<<rows, 256, 0, st>>>(reference, estimation, n, ratios);
    sisdr_metric_finalize_kernel<<<1, 64, 0, st>>>(ratios, rows, out);
    SEHIP_CHECK_LAUNCH("sisdr_metric");
    return 0;
}

extern "C" int sehip_sisnr_fwd(const float* est, const float* ref, int rows, int n, float* rowstat, float* loss,
                               void* stream) {
    SEHIP_REQUIRE(rows > 0 && n > 0, "sisnr_fwd: empty input (rows=%d n=%d)", rows, n);
    hipStream_t st = (hipStream_t)stream;
    sisnr_fwd_kernel<<<rows, 1024, 0, st>>>(est, ref, n, rows, (float4*)rowstat);
    sisnr_finalize_kernel<<<1, 64, 0, st>>>((const float4*)rowstat, rows, loss);
    SEHIP_CHECK_LAUNCH("sisnr_fwd");
    return 0;
}

extern "C" int sehip_sisnr_bwd(const float* est, const float* ref, const float* rowstat, const float* upstream, int rows,
                               int n, float* dest, void* stream) {
    SEHIP_REQUIRE(rows > 0 && n > 0, "sisnr_bwd: empty input (rows=%d n=%d)", rows, n);
    dim3 grid(cdiv(n, 256 * 8), rows);
    sisnr_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(est, ref, (const float4*)rowstat, upstream, n, dest);
    SEHIP_CHECK_LAUNCH("sisnr_bwd");
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Permutation-invariant SI-SNR: src/loss.py:58-100 (UtterenceBaasedPermutationInvariantTraining with loss_function =
// loss_sisdr).  est / ref are [B][S][C][n] (speaker axis 1).  The reference fills an S x S matrix with the BATCH-mean loss of
// (estimated speaker i, target speaker j) (:70-71), takes the permutation with the smallest sum, walking
// itertools.permutations in its lexicographic order with a strict '<' (:73-86), and returns the mean of the chosen pairs'
// losses (:88-96).  One launch computes the S*S*B*C row records, one single-wave launch the matrix, the permutation and the
// loss; the backward pass reads the permutation from device memory (no host round trip).
//   rowstat [S*S][R] float4 (R = B*C rows per pair; pair index i*S + j), pairloss [S*S], perm [S] (perm[j] = estimated speaker
//   matched with target j), loss [1]
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sisnr_pit_rows_kernel(const float* __restrict__ est, const float* __restrict__ ref, int B, int S,
                                                             int C, int n, float4* __restrict__ rowstat) {
    __shared__ float red[4];
    const int R = B * C;
    const int r = blockIdx.x, pair = blockIdx.y;
    const int i = pair / S, j = pair - i * S;
    const int b = r / C, c = r - b * C;
    const float* x = est + (((size_t)b * S + i) * C + c) * n;
    const float* s = ref + (((size_t)b * S + j) * C + c) * n;
    float xs = 0.f, ss = 0.f;
    for (int k = threadIdx.x; k < n; k += 256) { xs += x[k] * s[k]; ss += s[k] * s[k]; }
    xs = block_sum<4>(xs, red);
    ss = block_sum<4>(ss, red);
    const float alpha = xs / (ss + EPS);
    float et = 0.f, en = 0.f, es = 0.f;
    for (int k = threadIdx.x; k < n; k += 256) {
        const float t = alpha * s[k], e = sisnr_residual(x[k], alpha, s[k]);
        et += t * t; en += e * e; es += e * s[k];
    }
    et = block_sum<4>(et, red);
    en = block_sum<4>(en, red);
    es = block_sum<4>(es, red);
    if (threadIdx.x == 0) {
        const float ratio = et / (en + EPS);
        const float l = 10.f * log10f(ratio + EPS);
        // loss = (1/S) sum over chosen pairs of -mean_rows(l): d loss / d l = -1 / (S R)
        const float cc = -(1.0f / ((float)S * (float)R)) * 10.f / (2.302585092994046f * (ratio + EPS));
        const float q = et / ((en + EPS) * (en + EPS));
        const float a = cc * (-2.f * q);
        const float bb = cc * (2.f * alpha * ss / ((ss + EPS) * (en + EPS)) + 2.f * q * es / (ss + EPS));
        rowstat[(size_t)pair * R + r] = make_float4(a, bb, l, alpha);
    }
}

__global__ void sisnr_pit_select_kernel(const float4* __restrict__ rowstat, int R, int S, float* __restrict__ pairloss,
                                        int* __restrict__ perm, float* __restrict__ loss) {
    __shared__ float m[PIT_MAXS * PIT_MAXS];
    for (int pair = 0; pair < S * S; ++pair) {            // single wave, fixed summation order
        float acc = 0.f;
        for (int r = threadIdx.x; r < R; r += 64) acc += rowstat[(size_t)pair * R + r].z;
        acc = wave_sum(acc);
        if (threadIdx.x == 0) { m[pair] = -acc / R; pairloss[pair] = -acc / R; }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int best[PIT_MAXS];
    pit_best_permutation(m, S, best);
    float tot = 0.f;
    for (int j = 0; j < S; ++j) { perm[j] = best[j]; tot += m[best[j] * S + j]; }
    loss[0] = tot / S;
}

__global__ __launch_bounds__(256) void sisnr_pit_bwd_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                                                            const float4* __restrict__ rowstat, const int* __restrict__ perm,
                                                            const float* __restrict__ upstream, int B, int S, int C, int n,
                                                            float* __restrict__ dest) {
    const int R = B * C;
    const int r = blockIdx.y, i = blockIdx.z;
    int j = 0;
    for (int k = 0; k < S; ++k)
        if (perm[k] == i) j = k;                           // the target this estimated speaker was matched with
    const int b = r / C, c = r - b * C;
    const float4 st = rowstat[(size_t)(i * S + j) * R + r];
    const float up = upstream ? upstream[0] : 1.f;
    const float a = st.x * up, bb = st.y * up, alpha = st.w;
    const size_t xb = (((size_t)b * S + i) * C + c) * n, sb = (((size_t)b * S + j) * C + c) * n;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
        const float s = ref[sb + k];
        dest[xb + k] = a * sisnr_residual(est[xb + k], alpha, s) + bb * s;       // the residual form of sisnr_bwd_kernel
    }
}

extern "C" int sehip_sisnr_pit_fwd(const float* est, const float* ref, int B, int S, int C, int n, float* rowstat, float* pairloss,
                                   int* perm, float* loss, void* stream) {
    SEHIP_REQUIRE(B > 0 && C > 0 && n > 0 && S >= 1 && S <= PIT_MAXS, "sisnr_pit_fwd: bad shape (B=%d S=%d C=%d n=%d; S <= %d)", B, S,
                  C, n, PIT_MAXS);
    hipStream_t st = (hipStream_t)stream;
    sisnr_pit_rows_kernel<<<dim3(B * C, S * S), 256, 0, st>>>(est, ref, B, S, C, n, (float4*)rowstat);
    sisnr_pit_select_kernel<<<1, 64, 0, st>>>((const float4*)rowstat, B * C, S, pairloss, perm, loss);
    SEHIP_CHECK_LAUNCH("sisnr_pit_fwd");
    return 0;
}

extern "C" int sehip_sisnr_pit_bwd(const float* est, const float* ref, const float* rowstat, const int* perm, const float* upstream,
                                   int B, int S, int C, int n, float* dest, void* stream) {
    SEHIP_REQUIRE(B > 0 && C > 0 && n > 0 && S >= 1 && S <= PIT_MAXS, "sisnr_pit_bwd: bad shape (B=%d S=%d C=%d n=%d)", B, S, C, n);
    dim3 grid(cdiv(n, 256 * 8), B * C, S);
    sisnr_pit_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(est, ref, (const float4*)rowstat, perm, upstream, B, S, C, n, dest);
    SEHIP_CHECK_LAUNCH("sisnr_pit_bwd");
    return 0;
}

// ------------------------------------------------------------------------------------------------
// l1 / mse (the reference uses torch.nn.functional.l1_loss / mse_loss with reduction 'mean', src/distrib.py:263-268)
// mode 0: mean |x - y|     mode 1: mean (x - y)^2
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pointwise_loss_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, long n,
                                                                 int mode, double* __restrict__ acc) {
    __shared__ float red[4];
    float a = 0.f;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        const float d = x[i] - y[i];
        a += mode == 0 ? fabsf(d) : d * d;
    }
    a = block_sum<4>(a, red);
    if (threadIdx.x == 0) atomicAdd(acc, (double)a);
}

__global__ void pointwise_loss_finalize_kernel(const double* __restrict__ acc, long n, float* __restrict__ loss) {
    loss[0] = (float)(acc[0] / (double)n);
}

__global__ __launch_bounds__(256) void pointwise_loss_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, long n,
                                                                 int mode, const float* __restrict__ upstream,
                                                                 float* __restrict__ dx) {
    const float up = (upstream ? upstream[0] : 1.f) / (float)n;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        const float d = x[i] - y[i];
        dx[i] = mode == 0 ? (d > 0.f ? up : (d < 0.f ? -up : 0.f)) : 2.f * d * up;
    }
}

// ------------------------------------------------------------------------------------------------
// phase-sensitive spectral approximation (src/loss.py:32-56, `optim.loss: psa`, STFT-domain models; the Solver hands the mixture's
// spectrum as the third argument, src/solver.py:480).  Per complex element (last axis = (real, imaginary)):
//   d = |E| - |T| cos(tanh(Ti / (Tr + 1e-9)) - tanh(Mi / (Mr + 1e-9)));   loss = mean d^2
// (sic: tanh of the ratio, not atan -- the reference's formula is restated, not corrected).  Backward w.r.t. the enhanced spectrum:
// dE = upstream * 2 d / n * E / |E|; an element with |E| = 0 gets 0 (torch's sqrt backward gives NaN there: 0 * inf).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float psa_residual(float2 e, float2 t, float2 m, float& ae) {
    const float am = tanhf(m.y / (m.x + 1e-9f)), at = tanhf(t.y / (t.x + 1e-9f));
    ae = sqrtf(e.y * e.y + e.x * e.x);
    return ae - sqrtf(t.y * t.y + t.x * t.x) * cosf(at - am);
}

__global__ __launch_bounds__(256) void psa_loss_fwd_kernel(const float2* __restrict__ enh, const float2* __restrict__ tgt,
                                                           const float2* __restrict__ mix, long n, double* __restrict__ acc) {
    __shared__ float red[4];
    float a = 0.f;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        float ae;
        const float d = psa_residual(enh[i], tgt[i], mix[i], ae);
        a += d * d;
    }
    a = block_sum<4>(a, red);
    if (threadIdx.x == 0) atomicAdd(acc, (double)a);
}

__global__ __launch_bounds__(256) void psa_loss_bwd_kernel(const float2* __restrict__ enh, const float2* __restrict__ tgt,
                                                           const float2* __restrict__ mix, long n, const float* __restrict__ upstream,
                                                           float2* __restrict__ denh) {
    const float up = 2.f * (upstream ? upstream[0] : 1.f) / (float)n;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        const float2 e = enh[i];
        float ae;
        const float d = psa_residual(e, tgt[i], mix[i], ae);
        const float k = ae > 0.f ? up * d / ae : 0.f;
        denh[i] = make_float2(k * e.x, k * e.y);
    }
}

extern "C" int sehip_psa_loss_fwd(const float* enh, const float* tgt, const float* mix, long ncomplex, double* acc, float* loss, void* stream) {
    SEHIP_REQUIRE(ncomplex > 0 && enh && tgt && mix, "psa_loss_fwd: bad arguments (n=%ld)", ncomplex);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(acc, 0, sizeof(double), st);
    SEHIP_REQUIRE(e == hipSuccess, "psa_loss_fwd: memset failed: %s", hipGetErrorString(e));
    int grid = cdiv(ncomplex, 256 * 8);
    if (grid > 1024) grid = 1024;
    if (sehip_deterministic()) grid = 1;
    psa_loss_fwd_kernel<<<grid, 256, 0, st>>>((const float2*)enh, (const float2*)tgt, (const float2*)mix, ncomplex, acc);
    pointwise_loss_finalize_kernel<<<1, 1, 0, st>>>(acc, ncomplex, loss);
    SEHIP_CHECK_LAUNCH("psa_loss_fwd");
    return 0;
}

extern "C" int sehip_psa_loss_bwd(const float* enh, const float* tgt, const float* mix, long ncomplex, const float* upstream, float* denh,
                                  void* stream) {
    SEHIP_REQUIRE(ncomplex > 0 && enh && tgt && mix && denh, "psa_loss_bwd: bad arguments (n=%ld)", ncomplex);
    int grid = cdiv(ncomplex, 256 * 4);
    if (grid > 2048) grid = 2048;
    psa_loss_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const float2*)enh, (const float2*)tgt, (const float2*)mix, ncomplex, upstream,
                                                             (float2*)denh);
    SEHIP_CHECK_LAUNCH("psa_loss_bwd");
    return 0;
}

extern "C" int sehip_pointwise_loss_fwd(const float* x, const float* y, long n, int mode, double* acc, float* loss,
                                        void* stream) {
    SEHIP_REQUIRE(n > 0 && (mode == 0 || mode == 1), "pointwise_loss_fwd: bad arguments (n=%ld mode=%d)", n, mode);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(acc, 0, sizeof(double), st);
    SEHIP_REQUIRE(e == hipSuccess, "pointwise_loss_fwd: memset failed: %s", hipGetErrorString(e));
    int grid = cdiv(n, 256 * 16);
    if (grid > 1024) grid = 1024;
    if (sehip_deterministic()) grid = 1;
    pointwise_loss_fwd_kernel<<<grid, 256, 0, st>>>(x, y, n, mode, acc);
    pointwise_loss_finalize_kernel<<<1, 1, 0, st>>>(acc, n, loss);
    SEHIP_CHECK_LAUNCH("pointwise_loss_fwd");
    return 0;
}

extern "C" int sehip_pointwise_loss_bwd(const float* x, const float* y, long n, int mode, const float* upstream, float* dx,
                                        void* stream) {
    SEHIP_REQUIRE(n > 0 && (mode == 0 || mode == 1), "pointwise_loss_bwd: bad arguments (n=%ld mode=%d)", n, mode);
    int grid = cdiv(n, 256 * 8);
    if (grid > 2048) grid = 2048;
    pointwise_loss_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(x, y, n, mode, upstream, dx);
    SEHIP_CHECK_LAUNCH("pointwise_loss_bwd");
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Permutation-invariant l1 / mse: src/loss.py:58-100 around torch.nn.functional.l1_loss / mse_loss (the reference's shipped
// `optim.loss: 'mse'`, `optim.pit: True`).  est / ref [B][S][C][n], speakers on axis 1; pair (i, j) is the mean over
// everything but the speaker of |e_i - t_j| or (e_i - t_j)^2.
//   pairs kernel : ONE pass over est and ref.  A workgroup owns `chunk` samples of one (b, c) row set, loads the S estimated and
//                  S target values of every sample once and keeps all S*S sums in registers (S, the mode and the load width are
//                  template parameters: 36 accumulators + 12 float4 at S = 6, no scratch); one record [S*S] per workgroup
//                  goes to partials[nblocks][S*S].  No atomics: the sums do not depend on arrival order, so nothing switches on
//                  sehip_deterministic().
//   select kernel: one wave adds the records in a fixed order in double, divides by B*C*n, walks the permutations
//                  (pit_best_permutation) and writes pairloss [S*S], perm [S], loss [1].
//   bwd kernel   : dest[b,i,c,k] = upstream / (S B C n) * g(e_i - t_j), j read from perm on the device; g as in
//                  pointwise_loss_bwd_kernel (sign with 0 at 0, or 2 d).
// Rows start at ((b*S + i)*C + c)*n floats: the float4 variants need n % 4 == 0 and 16-byte aligned bases (then every row and
// every chunk start is aligned: chunk is a multiple of 4), anything else takes the scalar variants (every n >= 1).
// ------------------------------------------------------------------------------------------------
#define PITPW_THREADS 256
#define PITPW_CHUNK 2048L           // samples of one row per workgroup (two float4 per thread), doubled while the grid exceeds ...
#define PITPW_MAXBLOCKS 1024L       // ... this many workgroups (the select kernel's single wave reads every record)
#define PITPW_MAXROWS (1L << 20)    // B*C: the grid's x extent
#define PITPW_MAXN (0x7fffffff - 64 * 4 * PITPW_THREADS)   // the loops' int sample index never wraps

static long pitpw_chunk(long rows, long n) {
    long chunk = PITPW_CHUNK;
    while (rows * ((n + chunk - 1) / chunk) > PITPW_MAXBLOCKS && chunk < n) chunk *= 2;
    return chunk;
}

extern "C" int sehip_pit_pointwise_blocks(int B, int S, int C, int n) {
    if (B <= 0 || C <= 0 || n <= 0 || S < 1 || S > PIT_MAXS || (long)B * C > PITPW_MAXROWS || n > PITPW_MAXN) return 0;
    const long rows = (long)B * C, chunk = pitpw_chunk(rows, n);
    return (int)(rows * ((n + chunk - 1) / chunk));
}

template <int MODE>
__device__ __forceinline__ float pitpw_term(float e, float t) {
    const float d = e - t;
    return MODE == 0 ? fabsf(d) : d * d;
}

template <int S, int MODE, bool VEC>
__global__ __launch_bounds__(PITPW_THREADS) void pit_pointwise_pairs_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                                                                            int C, int n, int chunk, float* __restrict__ partials) {
    __shared__ float red[PITPW_THREADS / 64][S * S];
    const int r = blockIdx.x, b = r / C, c = r - b * C;    // grid (x: b*C + c, y: chunk of the row)
    const size_t row0 = ((size_t)b * S * C + c) * n, sstride = (size_t)C * n;      // speaker i of this (b, c): row0 + i * sstride
    const int k0 = blockIdx.y * chunk;                                             // < n: gridDim.y = ceil(n / chunk)
    const int k1 = n - k0 < chunk ? n : k0 + chunk;
    float acc[S * S];
#pragma unroll
    for (int p = 0; p < S * S; ++p) acc[p] = 0.f;
    if (VEC) {
        for (int k = k0 + 4 * (int)threadIdx.x; k < k1; k += 4 * PITPW_THREADS) {
            float4 e[S], t[S];
#pragma unroll
            for (int i = 0; i < S; ++i) {
                e[i] = *reinterpret_cast<const float4*>(est + row0 + i * sstride + k);
                t[i] = *reinterpret_cast<const float4*>(ref + row0 + i * sstride + k);
            }
#pragma unroll
            for (int i = 0; i < S; ++i)
#pragma unroll
                for (int j = 0; j < S; ++j)
                    acc[i * S + j] += (pitpw_term<MODE>(e[i].x, t[j].x) + pitpw_term<MODE>(e[i].y, t[j].y)) +
                                      (pitpw_term<MODE>(e[i].z, t[j].z) + pitpw_term<MODE>(e[i].w, t[j].w));
        }
    } else {
        for (int k = k0 + (int)threadIdx.x; k < k1; k += PITPW_THREADS) {
            float e[S], t[S];
#pragma unroll
            for (int i = 0; i < S; ++i) {
                e[i] = est[row0 + i * sstride + k];
                t[i] = ref[row0 + i * sstride + k];
            }
#pragma unroll
            for (int i = 0; i < S; ++i)
#pragma unroll
                for (int j = 0; j < S; ++j) acc[i * S + j] += pitpw_term<MODE>(e[i], t[j]);
        }
    }
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int p = 0; p < S * S; ++p) {
        const float v = wave_sum(acc[p]);
        if ((threadIdx.x & 63) == 0) red[w][p] = v;
    }
    __syncthreads();
    if (threadIdx.x < S * S) {
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < PITPW_THREADS / 64; ++q) v += red[q][threadIdx.x];
        partials[((size_t)blockIdx.x * gridDim.y + blockIdx.y) * (S * S) + threadIdx.x] = v;
    }
}

template <int S>
__global__ __launch_bounds__(64) void pit_pointwise_select_kernel(const float* __restrict__ partials, int nblocks, double inv_count,
                                                                  float* __restrict__ pairloss, int* __restrict__ perm,
                                                                  float* __restrict__ loss) {
    __shared__ float m[S * S];
    double acc[S * S];                                     // single wave: lane l adds records l, l + 64, ... in that order, then the
#pragma unroll                                             // xor tree of wave_sum_d -- one fixed order whatever the schedule
    for (int p = 0; p < S * S; ++p) acc[p] = 0.0;
    for (int q = threadIdx.x; q < nblocks; q += 64) {
        const float* rec = partials + (size_t)q * (S * S);
#pragma unroll
        for (int p = 0; p < S * S; ++p) acc[p] += (double)rec[p];
    }
#pragma unroll
    for (int p = 0; p < S * S; ++p) {
        const double v = wave_sum_d(acc[p]);
        if (threadIdx.x == 0) { m[p] = (float)(v * inv_count); pairloss[p] = m[p]; }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int best[PIT_MAXS];
    pit_best_permutation(m, S, best);
    float tot = 0.f;
    for (int j = 0; j < S; ++j) { perm[j] = best[j]; tot += m[best[j] * S + j]; }
    loss[0] = tot / S;
}

template <int MODE>
__device__ __forceinline__ float pitpw_grad(float e, float t, float up) {
    const float d = e - t;
    return MODE == 0 ? (d > 0.f ? up : (d < 0.f ? -up : 0.f)) : 2.f * d * up;
}

// grid (x: b*C + c, y: strides over the row, z: estimated speaker i)
template <int MODE, bool VEC>
__global__ __launch_bounds__(PITPW_THREADS) void pit_pointwise_bwd_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                                                                          const int* __restrict__ perm, const float* __restrict__ upstream,
                                                                          int S, int C, int n, float scale, float* __restrict__ dest) {
    const int r = blockIdx.x, i = blockIdx.z, b = r / C, c = r - b * C;
    int j = 0;
    for (int k = 0; k < S; ++k)
        if (perm[k] == i) j = k;                           // the target this estimated speaker was matched with
    const float up = (upstream ? upstream[0] : 1.f) * scale;
    const size_t xb = (((size_t)b * S + i) * C + c) * n, sb = (((size_t)b * S + j) * C + c) * n;
    if (VEC) {
        const int n4 = n >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(est + xb);
        const float4* s4 = reinterpret_cast<const float4*>(ref + sb);
        float4* d4 = reinterpret_cast<float4*>(dest + xb);
        for (int k = blockIdx.y * PITPW_THREADS + threadIdx.x; k < n4; k += gridDim.y * PITPW_THREADS) {
            const float4 e = x4[k], t = s4[k];
            d4[k] = make_float4(pitpw_grad<MODE>(e.x, t.x, up), pitpw_grad<MODE>(e.y, t.y, up), pitpw_grad<MODE>(e.z, t.z, up),
                                pitpw_grad<MODE>(e.w, t.w, up));
        }
    } else {
        for (int k = blockIdx.y * PITPW_THREADS + threadIdx.x; k < n; k += gridDim.y * PITPW_THREADS)
            dest[xb + k] = pitpw_grad<MODE>(est[xb + k], ref[sb + k], up);
    }
}

static bool pitpw_vec(const void* a, const void* b, const void* c, int n) {
    return (n & 3) == 0 && ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0);
}

template <int S>
static void pitpw_launch_fwd(const float* est, const float* ref, int B, int C, int n, int mode, float* partials, float* pairloss,
                             int* perm, float* loss, hipStream_t st) {
    const long rows = (long)B * C, chunk = pitpw_chunk(rows, n);
    const dim3 grid((unsigned)rows, (unsigned)((n + chunk - 1) / chunk));
    const bool vec = pitpw_vec(est, ref, nullptr, n);
#define PITPW_PAIRS(MODE_, VEC_) \
    pit_pointwise_pairs_kernel<S, MODE_, VEC_><<<grid, PITPW_THREADS, 0, st>>>(est, ref, C, n, (int)chunk, partials)
    if (mode == 0) { if (vec) PITPW_PAIRS(0, true); else PITPW_PAIRS(0, false); }
    else           { if (vec) PITPW_PAIRS(1, true); else PITPW_PAIRS(1, false); }
#undef PITPW_PAIRS
    pit_pointwise_select_kernel<S><<<1, 64, 0, st>>>(partials, (int)(grid.x * grid.y), 1.0 / ((double)B * C * n), pairloss, perm, loss);
}

extern "C" int sehip_pit_pointwise_fwd(const float* est, const float* ref, int B, int S, int C, int n, int mode, float* partials,
                                       float* pairloss, int* perm, float* loss, void* stream) {
    SEHIP_REQUIRE(S >= 1 && S <= PIT_MAXS, "pit_pointwise_fwd: S=%d outside [1, %d]", S, PIT_MAXS);
    SEHIP_REQUIRE(mode == 0 || mode == 1, "pit_pointwise_fwd: mode=%d (0 = l1, 1 = mse)", mode);
    SEHIP_REQUIRE(B > 0 && C > 0 && n > 0, "pit_pointwise_fwd: empty input (B=%d C=%d n=%d)", B, C, n);
    SEHIP_REQUIRE((long)B * C <= PITPW_MAXROWS && n <= PITPW_MAXN, "pit_pointwise_fwd: shape too large (B*C=%ld n=%d)", (long)B * C, n);
    SEHIP_REQUIRE(est && ref && partials && pairloss && perm && loss, "pit_pointwise_fwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    switch (S) {
        case 1: pitpw_launch_fwd<1>(est, ref, B, C, n, mode, partials, pairloss, perm, loss, st); break;
        case 2: pitpw_launch_fwd<2>(est, ref, B, C, n, mode, partials, pairloss, perm, loss, st); break;
        case 3: pitpw_launch_fwd<3>(est, ref, B, C, n, mode, partials, pairloss, perm, loss, st); break;
        case 4: pitpw_launch_fwd<4>(est, ref, B, C, n, mode, partials, pairloss, perm, loss, st); break;
        case 5: pitpw_launch_fwd<5>(est, ref, B, C, n, mode, partials, pairloss, perm, loss, st); break;
        default: pitpw_launch_fwd<6>(est, ref, B, C, n, mode, partials, pairloss, perm, loss, st); break;
    }
    SEHIP_CHECK_LAUNCH("pit_pointwise_fwd");
    return 0;
}

extern "C" int sehip_pit_pointwise_bwd(const float* est, const float* ref, const int* perm, const float* upstream, int B, int S, int C,
                                       int n, int mode, float* dest, void* stream) {
    SEHIP_REQUIRE(S >= 1 && S <= PIT_MAXS, "pit_pointwise_bwd: S=%d outside [1, %d]", S, PIT_MAXS);
    SEHIP_REQUIRE(mode == 0 || mode == 1, "pit_pointwise_bwd: mode=%d (0 = l1, 1 = mse)", mode);
    SEHIP_REQUIRE(B > 0 && C > 0 && n > 0, "pit_pointwise_bwd: empty input (B=%d C=%d n=%d)", B, C, n);
    SEHIP_REQUIRE((long)B * C <= PITPW_MAXROWS && n <= PITPW_MAXN, "pit_pointwise_bwd: shape too large (B*C=%ld n=%d)", (long)B * C, n);
    SEHIP_REQUIRE(est && ref && perm && dest, "pit_pointwise_bwd: null pointer");
    const bool vec = pitpw_vec(est, ref, dest, n);
    int gy = cdiv(n, PITPW_THREADS * 8);
    if (gy > 64) gy = 64;
    const dim3 grid(B * C, gy, S);
    const float scale = (float)(1.0 / ((double)S * B * C * n));
    hipStream_t st = (hipStream_t)stream;
#define PITPW_BWD(MODE_, VEC_) \
    pit_pointwise_bwd_kernel<MODE_, VEC_><<<grid, PITPW_THREADS, 0, st>>>(est, ref, perm, upstream, S, C, n, scale, dest)
    if (mode == 0) { if (vec) PITPW_BWD(0, true); else PITPW_BWD(0, false); }
    else           { if (vec) PITPW_BWD(1, true); else PITPW_BWD(1, false); }
#undef PITPW_BWD
    SEHIP_CHECK_LAUNCH("pit_pointwise_bwd");
    return 0;
}
