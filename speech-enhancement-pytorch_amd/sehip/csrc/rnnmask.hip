// rnn-stft-mask (src/model/stft_rnn.py:5-119, RNNBaseSTFTMask): everything of the train step but the BatchNorm statistics
// (sehip_wun_bn_stats / _finalize of csrc/wavunet.hip fit [rows][C] as they are).
//
// Row space.  The reference hands [B C][T][F] to an nn.LSTM / nn.GRU with batch_first=False: the recurrence runs along the B C axis
// (L = B C steps) and the T frames are its independent rows.  Every activation here is therefore [T frames][L steps][channels],
// row r = n L + l, bf16 with the channel axis padded to a multiple of 8 by zeros; the gate pre-activations, the activated gates
// and the carried state (c of the LSTM, h of the GRU) are fp32.
//
// Products.  bf16 operands, fp32 accumulation in __builtin_amdgcn_mfma_f32_16x16x32_bf16, operands straight from global memory
// in the MFMA's own fragment layout (lane = (row & 15, k chunk of 8)), as dmx_lstm_step_fwd_kernel of csrc/demucs.hip does:
//   rsm_gemm_nt : C [M][N] = A [M][K] B [N][K]^T   (input projections, the head with bias + ReLU, both input gradients)
//   rsm_gemm_tn : dW [N][K] = sum_m A [m][N]^T X [m + shift][K]   (every weight gradient, written in the parameter's own layout
//                 with its own, unpadded row length; shift = -+1 inside a row's L steps gives dW_hh from dG(l) and h(l -+ 1))
// Every sum has one owner and a fixed order: no atomics, no split-K, two runs are bit-identical.
//
// Recurrence.  One launch per step, grid (H / 16, directions, ceil(rows / 16)): no persistent kernel, no hand-off, no spin.
//
// mel-rnn (src/model/mel_rnn.py:8-114, MelRNN at n_mels = 0) is the same pipeline with three more cells of arithmetic: the Elman
// recurrence (rsm_elman_step_*: one gate, so a workgroup's four waves take four 16-unit blocks, grid (ceil(H / 64), directions,
// ceil(rows / 16))), a head of Linear + ReLU + Linear + Sigmoid (two more epilogues of rsm_gemm_nt_kernel) and a mask backward that
// carries the sigmoid's derivative.
#include "common.h"
#include "drop.h"

namespace {

__device__ __forceinline__ float rsm_sigm(float x) { return 1.f / (1.f + __expf(-x)); }

// ---- dropout: counter-based (RsmDrop, rsm_mix / rsm_key / rsm_keep: csrc/drop.h, shared with csrc/unet.hip) ------------------------------
__global__ void rsm_counter_next_kernel(unsigned long long* ctr, unsigned* used) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const unsigned long long c = ctr[0];
        used[0] = (unsigned)c;
        ctr[0] = c + 1ull;
    }
}

// ---- features: x [RC][F][T][2] fp32 -> feat [T][RC][Fp] bf16 = | re^2 - im^2 |, the (F, T) transposition through an LDS tile ----------
__global__ __launch_bounds__(256) void rsm_features_kernel(const float2* __restrict__ x, int RC, int F, int T, int Fp, bf16_raw* __restrict__ feat) {
    __shared__ float tile[32][33];
    const int rc = blockIdx.z, t0 = blockIdx.x * 32, f0 = blockIdx.y * 32;
    const int a = threadIdx.x & 31, b = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int f = f0 + b + 8 * i, t = t0 + a;
        float v = 0.f;
        if (f < F && t < T) {
            const float2 z = x[((long)rc * F + f) * T + t];
            v = fabsf(z.x * z.x - z.y * z.y);
        }
        tile[b + 8 * i][a] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = t0 + b + 8 * i, f = f0 + a;
        if (t < T && f < Fp) feat[((long)t * RC + rc) * Fp + f] = f2bf(tile[a][b + 8 * i]);
    }
}

// ---- weights: fp32 [N][K] -> bf16 [N][ld] (zero beyond K) or, transposed, bf16 [K][ld] (zero beyond N) -----------------------------------
__global__ __launch_bounds__(256) void rsm_pack_w_kernel(const float* __restrict__ w, int N, int K, int transpose, int ld, bf16_raw* __restrict__ dst) {
    const int rows = transpose ? K : N, cols = transpose ? N : K;
    const int cpad = (cols + 7) & ~7;
    const long total = (long)rows * cpad;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % cpad);
        const long r = i / cpad;
        float v = 0.f;
        if (c < cols) v = transpose ? w[(long)c * K + r] : w[r * K + c];
        dst[r * ld + c] = f2bf(v);
    }
}

// ---- C = A B^T ------------------------------------------------------------------------------------------------------------------------
// A [M][lda], B [N][ldb] bf16, K a multiple of 8 (chunks beyond K read as zero), rows beyond M / N are neither read nor written.
// EPI 0: fp32 C; 1: bf16 C; 2: bf16 max(C + bias[n], 0); 3: bf16 sigmoid(C + bias[n]); 4: bf16 C where gate[m][n] > 0, else 0 (gate bf16
// [M][ldg]: a stored ReLU output).  Workgroup = 64 x 64 of C, wave w its rows 16 w .. 16 w + 15.
template <int EPI>
__global__ __launch_bounds__(256) void rsm_gemm_nt_kernel(const bf16_raw* __restrict__ A, int lda, const bf16_raw* __restrict__ B, int ldb, int M, int N,
                                                          int K, const float* __restrict__ bias, void* __restrict__ Cout, int ldc,
                                                          const bf16_raw* __restrict__ gate = nullptr, int ldg = 0) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, kg = lane >> 4;
    const int m0 = blockIdx.y * 64 + 16 * w, n0 = blockIdx.x * 64;
    if (m0 >= M) return;
    const int am = m0 + i;
    const bool aok = am < M;
    const bf16_raw* ap = A + (long)(aok ? am : M - 1) * lda + 8 * kg;
    const bf16_raw* bp[4];
    bool bok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int bn = n0 + 16 * j + i;
        bok[j] = bn < N;
        bp[j] = B + (long)(bok[j] ? bn : N - 1) * ldb + 8 * kg;
    }
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 32) {
        const bool kok = k0 + 8 * kg < K;
        uint4 av = make_uint4(0, 0, 0, 0);
        if (aok && kok) av = *reinterpret_cast<const uint4*>(ap + k0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint4 bv = make_uint4(0, 0, 0, 0);
            if (bok[j] && kok) bv = *reinterpret_cast<const uint4*>(bp[j] + k0);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), acc[j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + 16 * j + i;
        if (n >= N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 4 * kg + r;
            if (m >= M) continue;
            const long o = (long)m * ldc + n;
            if (EPI == 0) ((float*)Cout)[o] = acc[j][r];
            else if (EPI == 1) ((bf16_raw*)Cout)[o] = f2bf(acc[j][r]);
            else if (EPI == 2) ((bf16_raw*)Cout)[o] = f2bf(fmaxf(acc[j][r] + bias[n], 0.f));
            else if (EPI == 3) ((bf16_raw*)Cout)[o] = f2bf(rsm_sigm(acc[j][r] + bias[n]));
            else ((bf16_raw*)Cout)[o] = bf2f(gate[(long)m * ldg + n]) > 0.f ? f2bf(acc[j][r]) : (bf16_raw)0;
        }
    }
}

// ---- dW = A^T X -----------------------------------------------------------------------------------------------------------------------
// A [M][lda] (columns 0 .. N-1 of it), X [M][ldx] (columns 0 .. K-1) bf16; dW [N][ldw] fp32.  Row m of A meets row m + shift of X, and
// only while both lie in the same run of L rows (shift = 0: plain).  32 rows at a time are transposed through LDS into the MFMA's
// fragment layout; a workgroup owns 64 x 64 of dW and walks all M rows in order.
__global__ __launch_bounds__(256) void rsm_gemm_tn_kernel(const bf16_raw* __restrict__ A, int lda, const bf16_raw* __restrict__ X, int ldx, int M, int N,
                                                          int K, int L, int shift, float* __restrict__ dW, int ldw) {
    __shared__ __attribute__((aligned(16))) bf16_raw At[64][40];
    __shared__ __attribute__((aligned(16))) bf16_raw Xt[64][40];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, kg = lane >> 4;
    const int n0 = blockIdx.y * 64, k0 = blockIdx.x * 64;
    const int mr = threadIdx.x >> 3, c8 = (threadIdx.x & 7) * 8;
    const int n8 = (N + 7) & ~7, k8 = (K + 7) & ~7;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int m0 = 0; m0 < M; m0 += 32) {
        const int m = m0 + mr;
        uint4 av = make_uint4(0, 0, 0, 0), xv = make_uint4(0, 0, 0, 0);
        if (m < M) {
            const int l = m % L + shift;
            if (l >= 0 && l < L) {
                if (n0 + c8 < n8) av = *reinterpret_cast<const uint4*>(A + (long)m * lda + n0 + c8);
                if (k0 + c8 < k8) xv = *reinterpret_cast<const uint4*>(X + (long)(m + shift) * ldx + k0 + c8);
            }
        }
        __syncthreads();      // the previous round's fragments are read
        const bf16_raw* ae = reinterpret_cast<const bf16_raw*>(&av);
        const bf16_raw* xe = reinterpret_cast<const bf16_raw*>(&xv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            At[c8 + e][mr] = ae[e];
            Xt[c8 + e][mr] = xe[e];
        }
        __syncthreads();
        const uint4 af = *reinterpret_cast<const uint4*>(&At[16 * w + i][8 * kg]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint4 bf = *reinterpret_cast<const uint4*>(&Xt[16 * j + i][8 * kg]);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af), __builtin_bit_cast(bf16x8, bf), acc[j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = k0 + 16 * j + i;
        if (k >= K) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + 16 * w + 4 * kg + r;
            if (n < N) dW[(long)n * ldw + k] = acc[j][r];
        }
    }
}

// ---- LSTM, one step.  pre fp32 [Bn][L][D][4][H] = x W_ih^T (no bias in this model), whh bf16 [D][4H][H], gates fp32 [Bn][L][D][4][H]
// (activated i, f, g, o: kept for backward), hs bf16 [Bn][L][D H] (output and next step's operand), cs fp32 [Bn][L][D H],
// hd bf16 [Bn][L][D H] or NULL: the dropped-out copy the next layer reads.  Direction 1 walks the steps backwards. ----------------------
__global__ __launch_bounds__(256) void rsm_lstm_step_fwd_kernel(const float* __restrict__ pre, const bf16_raw* __restrict__ whh, float* __restrict__ gates,
                                                                bf16_raw* __restrict__ hs, float* __restrict__ cs, bf16_raw* __restrict__ hd, int Bn,
                                                                int L, int H, int D, int s, RsmDrop dp) {
    __shared__ float gl[4][16][17];
    const int dir = blockIdx.y, u0 = blockIdx.x * 16, bt = blockIdx.z * 16;
    const int t = dir ? L - 1 - s : s, tp = dir ? t + 1 : t - 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, m = lane & 15, ug = lane >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
        const int brow = bt + m;
        const bf16_raw* hp = hs + ((long)(brow < Bn ? brow : Bn - 1) * L + tp) * D * H + dir * H + 8 * ug;
        const bf16_raw* wp = whh + ((long)(dir * 4 + w) * H + u0 + m) * H + 8 * ug;
        for (int k0 = 0; k0 < H; k0 += 32) {
            uint4 av = *reinterpret_cast<const uint4*>(hp + k0);
            if (brow >= Bn) av = make_uint4(0, 0, 0, 0);
            const uint4 bv = *reinterpret_cast<const uint4*>(wp + k0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) gl[w][4 * ug + r][m] = acc[r];
    __syncthreads();
    const int row = threadIdx.x >> 4, u = threadIdx.x & 15, b = bt + row;
    if (b >= Bn) return;
    const long g0 = (((long)b * L + t) * D + dir) * 4 * H + u0 + u;
    const float gi = rsm_sigm(pre[g0] + gl[0][row][u]);
    const float gf = rsm_sigm(pre[g0 + H] + gl[1][row][u]);
    const float gg = tanhf(pre[g0 + 2 * H] + gl[2][row][u]);
    const float go = rsm_sigm(pre[g0 + 3 * H] + gl[3][row][u]);
    const long o = ((long)b * L + t) * D * H + dir * H + u0 + u;
    const float cp = s > 0 ? cs[((long)b * L + tp) * D * H + dir * H + u0 + u] : 0.f;
    const float c = gf * cp + gi * gg;
    cs[o] = c;
    const bf16_raw hb = f2bf(go * tanhf(c));
    hs[o] = hb;
    if (hd) hd[o] = rsm_keep(rsm_key(dp), (unsigned)o, dp.thresh) ? f2bf(bf2f(hb) * dp.scale) : (bf16_raw)0;
    gates[g0] = gi; gates[g0 + H] = gf; gates[g0 + 2 * H] = gg; gates[g0 + 3 * H] = go;
}

// Backward step: dh = mask(dhs[t]) + dG(next) W_hh (wave w reduces gate w's part of K), then the cell.  whhT bf16 [D][H][4H]; dhs bf16
// [Bn][L][D H] gradient of the layer's (dropped-out, when dp.thresh) output; dG bf16 [Bn][L][D][4][H]; dc fp32 [D][Bn][H] carried.
__global__ __launch_bounds__(256) void rsm_lstm_step_bwd_kernel(const float* __restrict__ gates, const bf16_raw* __restrict__ whhT,
                                                                const float* __restrict__ cs, const bf16_raw* __restrict__ dhs,
                                                                bf16_raw* __restrict__ dG, float* __restrict__ dc, int Bn, int L, int H, int D, int s,
                                                                RsmDrop dp) {
    __shared__ float pl[4][16][17];
    const int dir = blockIdx.y, u0 = blockIdx.x * 16, bt = blockIdx.z * 16;
    const int t = dir ? s : L - 1 - s;
    const int tn = dir ? t - 1 : t + 1;         // the step after t in forward order (the previous launch)
    const int tp = dir ? t + 1 : t - 1;         // the step before t in forward order
    const bool has_prev = dir ? (t < L - 1) : (t > 0);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, m = lane & 15, ug = lane >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
        const int brow = bt + m;
        const bf16_raw* ap = dG + (((long)(brow < Bn ? brow : Bn - 1) * L + tn) * D + dir) * 4 * H + w * H + 8 * ug;
        const bf16_raw* wp = whhT + ((long)dir * H + u0 + m) * 4 * H + w * H + 8 * ug;
        for (int k0 = 0; k0 < H; k0 += 32) {
            uint4 av = *reinterpret_cast<const uint4*>(ap + k0);
            if (brow >= Bn) av = make_uint4(0, 0, 0, 0);
            const uint4 bv = *reinterpret_cast<const uint4*>(wp + k0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) pl[w][4 * ug + r][m] = acc[r];
    __syncthreads();
    const int row = threadIdx.x >> 4, u = threadIdx.x & 15, b = bt + row;
    if (b >= Bn) return;
    const long o = ((long)b * L + t) * D * H + dir * H + u0 + u;
    float dout = bf2f(dhs[o]);
    if (dp.thresh) dout = rsm_keep(rsm_key(dp), (unsigned)o, dp.thresh) ? dout * dp.scale : 0.f;
    const float dh = dout + pl[0][row][u] + pl[1][row][u] + pl[2][row][u] + pl[3][row][u];
    const long g0 = (((long)b * L + t) * D + dir) * 4 * H + u0 + u;
    const float gi = gates[g0], gf = gates[g0 + H], gg = gates[g0 + 2 * H], go = gates[g0 + 3 * H];
    const float c = cs[o];
    const float cp = has_prev ? cs[((long)b * L + tp) * D * H + dir * H + u0 + u] : 0.f;
    float* dcp = dc + ((long)dir * Bn + b) * H + u0 + u;
    const float tc = tanhf(c);
    const float dcc = dh * go * (1.f - tc * tc) + (s > 0 ? *dcp : 0.f);
    *dcp = dcc * gf;
    dG[g0] = f2bf(dcc * gg * gi * (1.f - gi));
    dG[g0 + H] = f2bf(dcc * cp * gf * (1.f - gf));
    dG[g0 + 2 * H] = f2bf(dcc * gi * (1.f - gg * gg));
    dG[g0 + 3 * H] = f2bf(dh * tc * go * (1.f - go));
}

// ---- GRU, one step.  pre fp32 [Bn][L][D][3][H] = x W_ih^T (r, z, n), whh bf16 [D][3H][H]; with a = h(t-1) W_hh^T:
//   r = sigm(pre_r + a_r), z = sigm(pre_z + a_z), n = tanh(pre_n + r a_n), h = (1 - z) n + z h(t-1)
// gates fp32 [Bn][L][D][4][H] = (r, z, n, a_n); hf fp32 [Bn][L][D H] the carried h; hs its bf16 copy (output, next step's operand). --------
__global__ __launch_bounds__(256) void rsm_gru_step_fwd_kernel(const float* __restrict__ pre, const bf16_raw* __restrict__ whh, float* __restrict__ gates,
                                                               bf16_raw* __restrict__ hs, float* __restrict__ hf, bf16_raw* __restrict__ hd, int Bn,
                                                               int L, int H, int D, int s, RsmDrop dp) {
    __shared__ float gl[3][16][17];
    const int dir = blockIdx.y, u0 = blockIdx.x * 16, bt = blockIdx.z * 16;
    const int t = dir ? L - 1 - s : s, tp = dir ? t + 1 : t - 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, m = lane & 15, ug = lane >> 4;
    if (w < 3) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (s > 0) {
            const int brow = bt + m;
            const bf16_raw* hp = hs + ((long)(brow < Bn ? brow : Bn - 1) * L + tp) * D * H + dir * H + 8 * ug;
            const bf16_raw* wp = whh + ((long)(dir * 3 + w) * H + u0 + m) * H + 8 * ug;
            for (int k0 = 0; k0 < H; k0 += 32) {
                uint4 av = *reinterpret_cast<const uint4*>(hp + k0);
                if (brow >= Bn) av = make_uint4(0, 0, 0, 0);
                const uint4 bv = *reinterpret_cast<const uint4*>(wp + k0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) gl[w][4 * ug + r][m] = acc[r];
    }
    __syncthreads();
    const int row = threadIdx.x >> 4, u = threadIdx.x & 15, b = bt + row;
    if (b >= Bn) return;
    const long p0 = (((long)b * L + t) * D + dir) * 3 * H + u0 + u;
    const long g0 = (((long)b * L + t) * D + dir) * 4 * H + u0 + u;
    const float an = gl[2][row][u];
    const float gr = rsm_sigm(pre[p0] + gl[0][row][u]);
    const float gz = rsm_sigm(pre[p0 + H] + gl[1][row][u]);
    const float gn = tanhf(pre[p0 + 2 * H] + gr * an);
    const long o = ((long)b * L + t) * D * H + dir * H + u0 + u;
    const float hp = s > 0 ? hf[((long)b * L + tp) * D * H + dir * H + u0 + u] : 0.f;
    const float h = (1.f - gz) * gn + gz * hp;
    hf[o] = h;
    const bf16_raw hb = f2bf(h);
    hs[o] = hb;
    if (hd) hd[o] = rsm_keep(rsm_key(dp), (unsigned)o, dp.thresh) ? f2bf(bf2f(hb) * dp.scale) : (bf16_raw)0;
    gates[g0] = gr; gates[g0 + H] = gz; gates[g0 + 2 * H] = gn; gates[g0 + 3 * H] = an;
}

// Backward step.  dG bf16 [Bn][L][D][4][H] = (d pre_r, d pre_z, d pre_n, r d pre_n): blocks 0 .. 2 are the gradient of x W_ih^T, blocks
// 0, 1, 3 that of h(t-1) W_hh^T.  whhT bf16 [D][H][3H]; dhc fp32 [D][Bn][H] carries z dh, the direct path to h(t-1).
__global__ __launch_bounds__(256) void rsm_gru_step_bwd_kernel(const float* __restrict__ gates, const bf16_raw* __restrict__ whhT,
                                                               const float* __restrict__ hf, const bf16_raw* __restrict__ dhs,
                                                               bf16_raw* __restrict__ dG, float* __restrict__ dhc, int Bn, int L, int H, int D, int s,
                                                               RsmDrop dp) {
    __shared__ float pl[3][16][17];
    const int dir = blockIdx.y, u0 = blockIdx.x * 16, bt = blockIdx.z * 16;
    const int t = dir ? s : L - 1 - s;
    const int tn = dir ? t - 1 : t + 1;
    const int tp = dir ? t + 1 : t - 1;
    const bool has_prev = dir ? (t < L - 1) : (t > 0);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, m = lane & 15, ug = lane >> 4;
    if (w < 3) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (s > 0) {
            const int brow = bt + m;
            const int blk = w == 2 ? 3 : w;
            const bf16_raw* ap = dG + (((long)(brow < Bn ? brow : Bn - 1) * L + tn) * D + dir) * 4 * H + blk * H + 8 * ug;
            const bf16_raw* wp = whhT + ((long)dir * H + u0 + m) * 3 * H + w * H + 8 * ug;
            for (int k0 = 0; k0 < H; k0 += 32) {
                uint4 av = *reinterpret_cast<const uint4*>(ap + k0);
                if (brow >= Bn) av = make_uint4(0, 0, 0, 0);
                const uint4 bv = *reinterpret_cast<const uint4*>(wp + k0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) pl[w][4 * ug + r][m] = acc[r];
    }
    __syncthreads();
    const int row = threadIdx.x >> 4, u = threadIdx.x & 15, b = bt + row;
    if (b >= Bn) return;
    const long o = ((long)b * L + t) * D * H + dir * H + u0 + u;
    float dout = bf2f(dhs[o]);
    if (dp.thresh) dout = rsm_keep(rsm_key(dp), (unsigned)o, dp.thresh) ? dout * dp.scale : 0.f;
    float* dcp = dhc + ((long)dir * Bn + b) * H + u0 + u;
    const float dh = dout + pl[0][row][u] + pl[1][row][u] + pl[2][row][u] + (s > 0 ? *dcp : 0.f);
    const long g0 = (((long)b * L + t) * D + dir) * 4 * H + u0 + u;
    const float gr = gates[g0], gz = gates[g0 + H], gn = gates[g0 + 2 * H], an = gates[g0 + 3 * H];
    const float hp = has_prev ? hf[((long)b * L + tp) * D * H + dir * H + u0 + u] : 0.f;
    *dcp = dh * gz;
    const float dpn = dh * (1.f - gz) * (1.f - gn * gn);
    dG[g0] = f2bf(dpn * an * gr * (1.f - gr));
    dG[g0 + H] = f2bf(dh * (hp - gn) * gz * (1.f - gz));
    dG[g0 + 2 * H] = f2bf(dpn);
    dG[g0 + 3 * H] = f2bf(dpn * gr);
}

// ---- Elman cell, one step: h(t) = tanh(pre(t) + h(t-1) W_hh^T).  pre fp32 [Bn][L][D][H] = x W_ih^T (no bias), whh bf16 [D][H][H], hs bf16
// [Bn][L][D H] (output and next step's operand), hf fp32 [Bn][L][D H] the same h unrounded (backward reads it).  One gate: wave w of a
// workgroup owns the 16 hidden units 64 blockIdx.x + 16 w .. + 15 (waves beyond H leave: H = 32 and 96 end in a ragged block), takes
// all of K itself and writes its accumulator fragment (lane (m, ug): rows 4 ug .. 4 ug + 3 of unit m) straight out: no LDS, no barrier.
__global__ __launch_bounds__(256) void rsm_elman_step_fwd_kernel(const float* __restrict__ pre, const bf16_raw* __restrict__ whh, bf16_raw* __restrict__ hs,
                                                                 float* __restrict__ hf, int Bn, int L, int H, int D, int s) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, m = lane & 15, ug = lane >> 4;
    const int dir = blockIdx.y, u0 = blockIdx.x * 64 + 16 * w, bt = blockIdx.z * 16;
    if (u0 >= H) return;
    const int t = dir ? L - 1 - s : s, tp = dir ? t + 1 : t - 1;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
        const int brow = bt + m;
        const bf16_raw* hp = hs + ((long)(brow < Bn ? brow : Bn - 1) * L + tp) * D * H + dir * H + 8 * ug;
        const bf16_raw* wp = whh + ((long)dir * H + u0 + m) * H + 8 * ug;
        for (int k0 = 0; k0 < H; k0 += 32) {
            uint4 av = *reinterpret_cast<const uint4*>(hp + k0);
            if (brow >= Bn) av = make_uint4(0, 0, 0, 0);
            const uint4 bv = *reinterpret_cast<const uint4*>(wp + k0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = bt + 4 * ug + r;
        if (b >= Bn) continue;
        const long o = ((long)b * L + t) * D * H + dir * H + u0 + m;
        const float h = tanhf(pre[o] + acc[r]);
        hf[o] = h;
        hs[o] = f2bf(h);
    }
}

// Backward step: dpre(t) = (dhs(t) + dpre(t+1) W_hh) (1 - h(t)^2), dpre(t+1) read back as the bf16 dG the previous launch stored (nothing
// is carried beside it).  whhT bf16 [D][H][H] (W_hh transposed), dhs bf16 [Bn][L][D H], dG bf16 [Bn][L][D][H].
__global__ __launch_bounds__(256) void rsm_elman_step_bwd_kernel(const bf16_raw* __restrict__ whhT, const float* __restrict__ hf,
                                                                 const bf16_raw* __restrict__ dhs, bf16_raw* __restrict__ dG, int Bn, int L, int H, int D,
                                                                 int s) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, m = lane & 15, ug = lane >> 4;
    const int dir = blockIdx.y, u0 = blockIdx.x * 64 + 16 * w, bt = blockIdx.z * 16;
    if (u0 >= H) return;
    const int t = dir ? s : L - 1 - s;
    const int tn = dir ? t - 1 : t + 1;         // the step after t in forward order (the previous launch)
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
        const int brow = bt + m;
        const bf16_raw* ap = dG + ((long)(brow < Bn ? brow : Bn - 1) * L + tn) * D * H + dir * H + 8 * ug;
        const bf16_raw* wp = whhT + ((long)dir * H + u0 + m) * H + 8 * ug;
        for (int k0 = 0; k0 < H; k0 += 32) {
            uint4 av = *reinterpret_cast<const uint4*>(ap + k0);
            if (brow >= Bn) av = make_uint4(0, 0, 0, 0);
            const uint4 bv = *reinterpret_cast<const uint4*>(wp + k0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = bt + 4 * ug + r;
        if (b >= Bn) continue;
        const long o = ((long)b * L + t) * D * H + dir * H + u0 + m;
        const float h = hf[o];
        dG[o] = f2bf((bf2f(dhs[o]) + acc[r]) * (1.f - h * h));
    }
}

// ---- column sums over rows of [rows][C] bf16, two fixed-order stages.  Stage one: 256 rows per workgroup, 64 columns x 4 row lanes;
// part [chunks][2][C].  MODE 0: (sum a, 0);  MODE 1: (sum a, sum a xhat), xhat = (y - mean) rstd from coef [C][4] = (scale, shift, mean, rstd)
#define RSM_SUM_ROWS 256
template <int MODE>
__global__ __launch_bounds__(256) void rsm_colsum_kernel(const bf16_raw* __restrict__ a, const bf16_raw* __restrict__ y, const float4* __restrict__ coef,
                                                         long rows, int C, int lda, float* __restrict__ part) {
    __shared__ float red[2][4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
    const long r0 = (long)blockIdx.y * RSM_SUM_ROWS;
    float s0 = 0.f, s1 = 0.f;
    if (c < C) {
        float mean = 0.f, rstd = 0.f;
        if (MODE == 1) { const float4 k = coef[c]; mean = k.z; rstd = k.w; }
        for (int j = q; j < RSM_SUM_ROWS; j += 4) {
            const long r = r0 + j;
            if (r >= rows) break;
            const float v = bf2f(a[r * lda + c]);
            s0 += v;
            if (MODE == 1) s1 += v * ((bf2f(y[r * C + c]) - mean) * rstd);
        }
    }
    red[0][q][threadIdx.x & 63] = s0;
    red[1][q][threadIdx.x & 63] = s1;
    __syncthreads();
    if (q == 0 && c < C) {
        const int x = threadIdx.x;
        part[((long)blockIdx.y * 2) * C + c] = (red[0][0][x] + red[0][1][x]) + (red[0][2][x] + red[0][3][x]);
        part[((long)blockIdx.y * 2 + 1) * C + c] = (red[1][0][x] + red[1][1][x]) + (red[1][2][x] + red[1][3][x]);
    }
}
// stage two: the chunks in order, in double.  out0 = sum a (dbeta / a bias gradient), out1 = sum a xhat (dgamma, optional);
// bcoef [C][4] = (gamma rstd, out0 / rows, out1 / rows, 0) (optional)
__global__ __launch_bounds__(256) void rsm_colsum_finalize_kernel(const float* __restrict__ part, int chunks, long rows, int C, const float* __restrict__ gamma,
                                                                  const float4* __restrict__ coef, float* __restrict__ out0, float* __restrict__ out1,
                                                                  float4* __restrict__ bcoef) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s0 = 0.0, s1 = 0.0;
    for (int k = 0; k < chunks; ++k) {
        s0 += (double)part[((long)k * 2) * C + c];
        s1 += (double)part[((long)k * 2 + 1) * C + c];
    }
    out0[c] = (float)s0;
    if (out1) out1[c] = (float)s1;
    if (bcoef) bcoef[c] = make_float4(gamma[c] * coef[c].w, (float)(s0 / (double)rows), (float)(s1 / (double)rows), 0.f);
}

// z = scale y + shift (BatchNorm1d forward, no activation)
__global__ __launch_bounds__(256) void rsm_bn_apply_kernel(const bf16_raw* __restrict__ y, const float4* __restrict__ coef, long rows, int C,
                                                           bf16_raw* __restrict__ z) {
    const long total = rows * C;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const float4 k = coef[(int)(i % C)];
        z[i] = f2bf(bf2f(y[i]) * k.x + k.y);
    }
}
// dy = gamma rstd (dz - mean(dz) - xhat mean(dz xhat))
__global__ __launch_bounds__(256) void rsm_bn_bwd_apply_kernel(const bf16_raw* __restrict__ dz, const bf16_raw* __restrict__ y, const float4* __restrict__ coef,
                                                               const float4* __restrict__ bcoef, long rows, int C, bf16_raw* __restrict__ dy) {
    const long total = rows * C;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const float4 k = coef[c], bk = bcoef[c];
        const float xh = (bf2f(y[i]) - k.z) * k.w;
        dy[i] = f2bf(bk.x * (bf2f(dz[i]) - bk.y - xh * bk.z));
    }
}

// ---- mask application.  mask bf16 [T][RC][SFp] (row t RC + rc, column s F + f), x fp32 [RC = B C][F][T][2],
// out fp32 [B][S][C][F][T][2] = mask x; the (F, T) transposition through an LDS tile.  grid (ceil(T/32), ceil(F/32), RC S) ---------------
__global__ __launch_bounds__(256) void rsm_mask_fwd_kernel(const bf16_raw* __restrict__ mask, const float2* __restrict__ x, int Cn, int S, int F, int T,
                                                           int RC, int SFp, float2* __restrict__ out) {
    __shared__ float tile[32][33];      // [t][f]
    const int rc = blockIdx.z / S, sp = blockIdx.z % S, t0 = blockIdx.x * 32, f0 = blockIdx.y * 32;
    const int a = threadIdx.x & 31, b = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = t0 + b + 8 * i, f = f0 + a;
        tile[b + 8 * i][a] = (t < T && f < F) ? bf2f(mask[((long)t * RC + rc) * SFp + sp * F + f]) : 0.f;
    }
    __syncthreads();
    const int bb = rc / Cn, cc = rc % Cn;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int f = f0 + b + 8 * i, t = t0 + a;
        if (f < F && t < T) {
            const float2 z = x[((long)rc * F + f) * T + t];
            const float mk = tile[a][b + 8 * i];
            out[((((long)bb * S + sp) * Cn + cc) * F + f) * T + t] = make_float2(mk * z.x, mk * z.y);
        }
    }
}
// dpre bf16 [T][RC][SFp] = (mask > 0) (dout_re x_re + dout_im x_im): the gradient in front of the head's ReLU; padded columns untouched.
// SIGMOID: the head ends in a sigmoid instead, dpre = m (1 - m) (dout_re x_re + dout_im x_im) with m the stored bf16 mask.
template <bool SIGMOID>
__global__ __launch_bounds__(256) void rsm_mask_bwd_kernel(const float2* __restrict__ dout, const float2* __restrict__ x, const bf16_raw* __restrict__ mask,
                                                           int Cn, int S, int F, int T, int RC, int SFp, bf16_raw* __restrict__ dpre) {
    __shared__ float tile[32][33];      // [f][t]
    const int rc = blockIdx.z / S, sp = blockIdx.z % S, t0 = blockIdx.x * 32, f0 = blockIdx.y * 32;
    const int a = threadIdx.x & 31, b = threadIdx.x >> 5;
    const int bb = rc / Cn, cc = rc % Cn;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int f = f0 + b + 8 * i, t = t0 + a;
        float v = 0.f;
        if (f < F && t < T) {
            const float2 z = x[((long)rc * F + f) * T + t];
            const float2 g = dout[((((long)bb * S + sp) * Cn + cc) * F + f) * T + t];
            v = g.x * z.x + g.y * z.y;
        }
        tile[b + 8 * i][a] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = t0 + b + 8 * i, f = f0 + a;
        if (t < T && f < F) {
            const long o = ((long)t * RC + rc) * SFp + sp * F + f;
            const float mk = bf2f(mask[o]);
            if (SIGMOID) dpre[o] = f2bf(mk * (1.f - mk) * tile[a][b + 8 * i]);
            else dpre[o] = mk > 0.f ? f2bf(tile[a][b + 8 * i]) : (bf16_raw)0;
        }
    }
}

int check_rnn(const char* what, int Bn, int L, int H, int D) {
    SEHIP_REQUIRE(Bn >= 1 && L >= 1, "%s: rows=%d steps=%d must be positive", what, Bn, L);
    SEHIP_REQUIRE(H >= 32 && H <= 1024 && H % 32 == 0, "%s: hidden size %d must be a multiple of 32 in 32 .. 1024", what, H);
    SEHIP_REQUIRE(D == 1 || D == 2, "%s: %d directions", what, D);
    SEHIP_REQUIRE((long)Bn * L * D * 4 * H < (1L << 32), "%s: more than 2^32 gate elements", what);
    SEHIP_REQUIRE((Bn + 15) / 16 <= 65535, "%s: more than 65535 row tiles", what);
    return 0;
}
RsmDrop make_drop(unsigned seed_lo, unsigned seed_hi, const unsigned* ctr, int layer, unsigned thresh, float scale) {
    RsmDrop d;
    d.seed_lo = seed_lo; d.seed_hi = seed_hi; d.ctr = ctr; d.layer = layer; d.thresh = thresh; d.scale = scale;
    return d;
}
int grid1(long n) { const long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g)); }

}  // namespace

extern "C" long sehip_rsm_sum_scratch_floats(long rows, int C) {
    if (rows < 1 || C < 1) return 0;
    return ((rows + RSM_SUM_ROWS - 1) / RSM_SUM_ROWS) * 2L * C;
}

extern "C" int sehip_rsm_counter_next(void* counter, void* used, void* stream) {
    SEHIP_REQUIRE(counter && used, "rsm_counter_next: null pointer");
    rsm_counter_next_kernel<<<1, 64, 0, (hipStream_t)stream>>>((unsigned long long*)counter, (unsigned*)used);
    SEHIP_CHECK_LAUNCH("rsm_counter_next");
    return 0;
}

extern "C" int sehip_rsm_features(const float* x, int RC, int F, int T, int Fp, void* feat, void* stream) {
    SEHIP_REQUIRE(x && feat, "rsm_features: null pointer");
    SEHIP_REQUIRE(RC >= 1 && RC <= 65535 && F >= 1 && T >= 1 && Fp >= F && Fp % 8 == 0 && Fp - F < 8, "rsm_features: RC=%d F=%d T=%d Fp=%d", RC, F, T, Fp);
    rsm_features_kernel<<<dim3((T + 31) / 32, (Fp + 31) / 32, RC), 256, 0, (hipStream_t)stream>>>((const float2*)x, RC, F, T, Fp, (bf16_raw*)feat);
    SEHIP_CHECK_LAUNCH("rsm_features");
    return 0;
}

extern "C" int sehip_rsm_pack_w(const float* w, int N, int K, int transpose, int ld, void* dst, void* stream) {
    SEHIP_REQUIRE(w && dst, "rsm_pack_w: null pointer");
    SEHIP_REQUIRE(N >= 1 && K >= 1 && ld % 8 == 0 && ld >= (((transpose ? N : K) + 7) & ~7), "rsm_pack_w: N=%d K=%d ld=%d", N, K, ld);
    rsm_pack_w_kernel<<<grid1((long)N * K), 256, 0, (hipStream_t)stream>>>(w, N, K, transpose, ld, (bf16_raw*)dst);
    SEHIP_CHECK_LAUNCH("rsm_pack_w");
    return 0;
}

extern "C" int sehip_rsm_gemm_nt(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epilogue, const float* bias, void* C,
                                 int ldc, void* stream) {
    SEHIP_REQUIRE(A && B && C, "rsm_gemm_nt: null pointer");
    SEHIP_REQUIRE(M >= 1 && N >= 1 && K >= 8 && K % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && lda >= K && ldb >= K && ldc >= N,
                  "rsm_gemm_nt: M=%d N=%d K=%d lda=%d ldb=%d ldc=%d (K and the operand strides are multiples of 8)", M, N, K, lda, ldb, ldc);
    SEHIP_REQUIRE((M + 63) / 64 <= 65535, "rsm_gemm_nt: M=%d: more than 65535 row tiles", M);
    SEHIP_REQUIRE(epilogue >= 0 && epilogue <= 2 && (epilogue != 2 || bias), "rsm_gemm_nt: epilogue %d", epilogue);
    const dim3 grid((N + 63) / 64, (M + 63) / 64);
    const bf16_raw *a = (const bf16_raw*)A, *b = (const bf16_raw*)B;
    if (epilogue == 0) rsm_gemm_nt_kernel<0><<<grid, 256, 0, (hipStream_t)stream>>>(a, lda, b, ldb, M, N, K, bias, C, ldc);
    else if (epilogue == 1) rsm_gemm_nt_kernel<1><<<grid, 256, 0, (hipStream_t)stream>>>(a, lda, b, ldb, M, N, K, bias, C, ldc);
    else rsm_gemm_nt_kernel<2><<<grid, 256, 0, (hipStream_t)stream>>>(a, lda, b, ldb, M, N, K, bias, C, ldc);
    SEHIP_CHECK_LAUNCH("rsm_gemm_nt");
    return 0;
}

extern "C" int sehip_rsm_gemm_nt_head(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int epilogue, const float* bias,
                                      const void* gate, int ldg, void* C, int ldc, void* stream) {
    SEHIP_REQUIRE(A && B && C, "rsm_gemm_nt_head: null pointer");
    SEHIP_REQUIRE(M >= 1 && N >= 1 && K >= 8 && K % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && lda >= K && ldb >= K && ldc >= N,
                  "rsm_gemm_nt_head: M=%d N=%d K=%d lda=%d ldb=%d ldc=%d (K and the operand strides are multiples of 8)", M, N, K, lda, ldb, ldc);
    SEHIP_REQUIRE((M + 63) / 64 <= 65535, "rsm_gemm_nt_head: M=%d: more than 65535 row tiles", M);
    SEHIP_REQUIRE((epilogue == 3 && bias) || (epilogue == 4 && gate && ldg >= N),
                  "rsm_gemm_nt_head: epilogue %d (3: bias + sigmoid, needs bias; 4: gated by a stored ReLU output, needs gate and ldg=%d >= N)", epilogue, ldg);
    const dim3 grid((N + 63) / 64, (M + 63) / 64);
    const bf16_raw *a = (const bf16_raw*)A, *b = (const bf16_raw*)B;
    if (epilogue == 3) rsm_gemm_nt_kernel<3><<<grid, 256, 0, (hipStream_t)stream>>>(a, lda, b, ldb, M, N, K, bias, C, ldc, nullptr, 0);
    else rsm_gemm_nt_kernel<4><<<grid, 256, 0, (hipStream_t)stream>>>(a, lda, b, ldb, M, N, K, nullptr, C, ldc, (const bf16_raw*)gate, ldg);
    SEHIP_CHECK_LAUNCH("rsm_gemm_nt_head");
    return 0;
}

extern "C" int sehip_rsm_gemm_tn(const void* A, int lda, const void* X, int ldx, int M, int N, int K, int L, int shift, float* dW, int ldw,
                                 void* stream) {
    SEHIP_REQUIRE(A && X && dW, "rsm_gemm_tn: null pointer");
    SEHIP_REQUIRE(M >= 1 && N >= 1 && K >= 1 && L >= 1 && M % L == 0 && shift >= -1 && shift <= 1 && lda % 8 == 0 && ldx % 8 == 0
                  && lda >= ((N + 7) & ~7) && ldx >= ((K + 7) & ~7) && ldw >= K,
                  "rsm_gemm_tn: M=%d N=%d K=%d L=%d shift=%d lda=%d ldx=%d ldw=%d", M, N, K, L, shift, lda, ldx, ldw);
    SEHIP_REQUIRE((N + 63) / 64 <= 65535, "rsm_gemm_tn: N=%d: more than 65535 tiles", N);
    rsm_gemm_tn_kernel<<<dim3((K + 63) / 64, (N + 63) / 64), 256, 0, (hipStream_t)stream>>>((const bf16_raw*)A, lda, (const bf16_raw*)X, ldx, M, N, K, L,
                                                                                          shift, dW, ldw);
    SEHIP_CHECK_LAUNCH("rsm_gemm_tn");
    return 0;
}

extern "C" int sehip_rsm_rnn_fwd(int gru, const float* pre, const void* whh, float* gates, void* hs, float* state, void* hd, int Bn, int L, int H,
                                 int D, unsigned seed_lo, unsigned seed_hi, const void* ctr, int layer, unsigned thresh, float scale,
                                 void* stream) {
    if (int e = check_rnn("rsm_rnn_fwd", Bn, L, H, D)) return e;
    SEHIP_REQUIRE(pre && whh && gates && hs && state, "rsm_rnn_fwd: null pointer");
    SEHIP_REQUIRE(!hd || ctr, "rsm_rnn_fwd: dropout needs the step counter");
    const RsmDrop dp = make_drop(seed_lo, seed_hi, (const unsigned*)ctr, layer, thresh, scale);
    const dim3 grid(H / 16, D, (Bn + 15) / 16);
    for (int s = 0; s < L; ++s) {
        if (gru)
            rsm_gru_step_fwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(pre, (const bf16_raw*)whh, gates, (bf16_raw*)hs, state, (bf16_raw*)hd, Bn, L, H, D, s, dp);
        else
            rsm_lstm_step_fwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(pre, (const bf16_raw*)whh, gates, (bf16_raw*)hs, state, (bf16_raw*)hd, Bn, L, H, D, s, dp);
    }
    SEHIP_CHECK_LAUNCH("rsm_rnn_fwd");
    return 0;
}

extern "C" int sehip_rsm_rnn_bwd(int gru, const float* gates, const void* whhT, const float* state, const void* dhs, void* dG, float* carry, int Bn,
                                 int L, int H, int D, unsigned seed_lo, unsigned seed_hi, const void* ctr, int layer, unsigned thresh, float scale,
                                 void* stream) {
    if (int e = check_rnn("rsm_rnn_bwd", Bn, L, H, D)) return e;
    SEHIP_REQUIRE(gates && whhT && state && dhs && dG && carry, "rsm_rnn_bwd: null pointer");
    SEHIP_REQUIRE(!thresh || ctr, "rsm_rnn_bwd: dropout needs the step counter");
    const RsmDrop dp = make_drop(seed_lo, seed_hi, (const unsigned*)ctr, layer, thresh, scale);
    const dim3 grid(H / 16, D, (Bn + 15) / 16);
    for (int s = 0; s < L; ++s) {
        if (gru)
            rsm_gru_step_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(gates, (const bf16_raw*)whhT, state, (const bf16_raw*)dhs, (bf16_raw*)dG, carry, Bn, L, H, D, s, dp);
        else
            rsm_lstm_step_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(gates, (const bf16_raw*)whhT, state, (const bf16_raw*)dhs, (bf16_raw*)dG, carry, Bn, L, H, D, s, dp);
    }
    SEHIP_CHECK_LAUNCH("rsm_rnn_bwd");
    return 0;
}

extern "C" int sehip_rsm_elman_fwd(const float* pre, const void* whh, void* hs, float* state, int Bn, int L, int H, int D, void* stream) {
    if (int e = check_rnn("rsm_elman_fwd", Bn, L, H, D)) return e;
    SEHIP_REQUIRE(pre && whh && hs && state, "rsm_elman_fwd: null pointer");
    const dim3 grid((H + 63) / 64, D, (Bn + 15) / 16);
    for (int s = 0; s < L; ++s)
        rsm_elman_step_fwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(pre, (const bf16_raw*)whh, (bf16_raw*)hs, state, Bn, L, H, D, s);
    SEHIP_CHECK_LAUNCH("rsm_elman_fwd");
    return 0;
}

extern "C" int sehip_rsm_elman_bwd(const void* whhT, const float* state, const void* dhs, void* dG, int Bn, int L, int H, int D, void* stream) {
    if (int e = check_rnn("rsm_elman_bwd", Bn, L, H, D)) return e;
    SEHIP_REQUIRE(whhT && state && dhs && dG, "rsm_elman_bwd: null pointer");
    const dim3 grid((H + 63) / 64, D, (Bn + 15) / 16);
    for (int s = 0; s < L; ++s)
        rsm_elman_step_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const bf16_raw*)whhT, state, (const bf16_raw*)dhs, (bf16_raw*)dG, Bn, L, H, D, s);
    SEHIP_CHECK_LAUNCH("rsm_elman_bwd");
    return 0;
}

extern "C" int sehip_rsm_colsum(const void* a, int lda, const void* y, const float* coef, long rows, int C, float* part, void* stream) {
    SEHIP_REQUIRE(a && part && rows >= 1 && C >= 1 && lda >= C, "rsm_colsum: rows=%ld C=%d lda=%d", rows, C, lda);
    SEHIP_REQUIRE((y == nullptr) == (coef == nullptr), "rsm_colsum: y and coef come together");
    const long chunks = (rows + RSM_SUM_ROWS - 1) / RSM_SUM_ROWS;
    SEHIP_REQUIRE(chunks <= 65535, "rsm_colsum: rows=%ld: more than 65535 chunks", rows);
    const dim3 grid((C + 63) / 64, (unsigned)chunks);
    if (y) rsm_colsum_kernel<1><<<grid, 256, 0, (hipStream_t)stream>>>((const bf16_raw*)a, (const bf16_raw*)y, (const float4*)coef, rows, C, lda, part);
    else rsm_colsum_kernel<0><<<grid, 256, 0, (hipStream_t)stream>>>((const bf16_raw*)a, nullptr, nullptr, rows, C, lda, part);
    SEHIP_CHECK_LAUNCH("rsm_colsum");
    return 0;
}

extern "C" int sehip_rsm_colsum_finalize(const float* part, long rows, int C, const float* gamma, const float* coef, float* out0, float* out1,
                                         float* bcoef, void* stream) {
    SEHIP_REQUIRE(part && out0 && rows >= 1 && C >= 1, "rsm_colsum_finalize: rows=%ld C=%d", rows, C);
    SEHIP_REQUIRE(!bcoef || (gamma && coef), "rsm_colsum_finalize: bcoef needs gamma and coef");
    const int chunks = (int)((rows + RSM_SUM_ROWS - 1) / RSM_SUM_ROWS);
    rsm_colsum_finalize_kernel<<<(C + 255) / 256, 256, 0, (hipStream_t)stream>>>(part, chunks, rows, C, gamma, (const float4*)coef, out0, out1, (float4*)bcoef);
    SEHIP_CHECK_LAUNCH("rsm_colsum_finalize");
    return 0;
}

extern "C" int sehip_rsm_bn_apply(const void* y, const float* coef, long rows, int C, void* z, void* stream) {
    SEHIP_REQUIRE(y && coef && z && rows >= 1 && C >= 1, "rsm_bn_apply: rows=%ld C=%d", rows, C);
    rsm_bn_apply_kernel<<<grid1(rows * C), 256, 0, (hipStream_t)stream>>>((const bf16_raw*)y, (const float4*)coef, rows, C, (bf16_raw*)z);
    SEHIP_CHECK_LAUNCH("rsm_bn_apply");
    return 0;
}

extern "C" int sehip_rsm_bn_bwd_apply(const void* dz, const void* y, const float* coef, const float* bcoef, long rows, int C, void* dy, void* stream) {
    SEHIP_REQUIRE(dz && y && coef && bcoef && dy && rows >= 1 && C >= 1, "rsm_bn_bwd_apply: rows=%ld C=%d", rows, C);
    rsm_bn_bwd_apply_kernel<<<grid1(rows * C), 256, 0, (hipStream_t)stream>>>((const bf16_raw*)dz, (const bf16_raw*)y, (const float4*)coef,
                                                                             (const float4*)bcoef, rows, C, (bf16_raw*)dy);
    SEHIP_CHECK_LAUNCH("rsm_bn_bwd_apply");
    return 0;
}

static int check_mask(const char* what, int B, int Cn, int S, int F, int T, int SFp) {
    SEHIP_REQUIRE(B >= 1 && Cn >= 1 && S >= 1 && F >= 1 && T >= 1 && SFp >= S * F && SFp % 8 == 0, "%s: B=%d C=%d S=%d F=%d T=%d SFp=%d", what, B, Cn, S, F,
                  T, SFp);
    SEHIP_REQUIRE((long)B * Cn * S <= 65535, "%s: B C S = %ld exceeds 65535", what, (long)B * Cn * S);
    return 0;
}
extern "C" int sehip_rsm_mask_fwd(const void* mask, const float* x, int B, int Cn, int S, int F, int T, int SFp, float* out, void* stream) {
    if (int e = check_mask("rsm_mask_fwd", B, Cn, S, F, T, SFp)) return e;
    SEHIP_REQUIRE(mask && x && out, "rsm_mask_fwd: null pointer");
    rsm_mask_fwd_kernel<<<dim3((T + 31) / 32, (F + 31) / 32, B * Cn * S), 256, 0, (hipStream_t)stream>>>((const bf16_raw*)mask, (const float2*)x, Cn, S, F, T,
                                                                                                      B * Cn, SFp, (float2*)out);
    SEHIP_CHECK_LAUNCH("rsm_mask_fwd");
    return 0;
}
extern "C" int sehip_rsm_mask_bwd(const float* dout, const float* x, const void* mask, int B, int Cn, int S, int F, int T, int SFp, void* dpre,
                                  void* stream) {
    if (int e = check_mask("rsm_mask_bwd", B, Cn, S, F, T, SFp)) return e;
    SEHIP_REQUIRE(dout && x && mask && dpre, "rsm_mask_bwd: null pointer");
    rsm_mask_bwd_kernel<false><<<dim3((T + 31) / 32, (F + 31) / 32, B * Cn * S), 256, 0, (hipStream_t)stream>>>((const float2*)dout, (const float2*)x,
                                                                                                             (const bf16_raw*)mask, Cn, S, F, T, B * Cn,
                                                                                                             SFp, (bf16_raw*)dpre);
    SEHIP_CHECK_LAUNCH("rsm_mask_bwd");
    return 0;
}
extern "C" int sehip_rsm_mask_bwd_sigmoid(const float* dout, const float* x, const void* mask, int B, int Cn, int S, int F, int T, int SFp, void* dpre,
                                          void* stream) {
    if (int e = check_mask("rsm_mask_bwd_sigmoid", B, Cn, S, F, T, SFp)) return e;
    SEHIP_REQUIRE(dout && x && mask && dpre, "rsm_mask_bwd_sigmoid: null pointer");
    rsm_mask_bwd_kernel<true><<<dim3((T + 31) / 32, (F + 31) / 32, B * Cn * S), 256, 0, (hipStream_t)stream>>>((const float2*)dout, (const float2*)x,
                                                                                                            (const bf16_raw*)mask, Cn, S, F, T, B * Cn,
                                                                                                            SFp, (bf16_raw*)dpre);
    SEHIP_CHECK_LAUNCH("rsm_mask_bwd_sigmoid");
    return 0;
}
