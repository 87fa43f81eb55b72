// ConvTasNet with norm_type='cLN' (src/model/conv_tasnet.py:422-461: the channel-wise LayerNorm on BOTH norms of every temporal
// block), causal or not -- the counterparts of tasnet.hip's gLN kernels.
//
//   cLN:  y = gamma (v - mu_t) / sqrt(var_t + 1e-8) + beta,  mu_t / var_t (biased) over the C channels of ONE frame t;  v = PReLU(h; a)
//         dv = (gamma dy - mean_c(gamma dy) - xh mean_c(gamma dy xh)) / sigma_t;  dh = dv (h > 0 ? 1 : a);  da = sum dv h [h <= 0]
//
// Every sum of the normalisation is per frame, and a frame of C <= 512 bf16 channels is C/8 <= 64 sixteen-byte pieces: the
// lanes that hold a frame are a group of G = next power of two >= C/8 neighbouring lanes of ONE wave (C/8 = 12: groups of 16 with
// four idle lanes), and the sums meet by xor-shuffles inside the group -- no LDS, no statistics record, no second pass:
//
//   ctn_cln_apply        u = cLN(PReLU(h))
//   ctn_cln_dwconv_fwd   h2[t] = sum_j Wd[j] n1[t + (j - c) d],  n1 = cLN(PReLU(h1)),  c = P/2 or (causal) P - 1
//   ctn_cln_bwd          gradient of y = cLN(PReLU(h)), directly or behind the transposed depthwise conv, in ONE pass
//
// Moments of the P tap rows of the depthwise conv: RECOMPUTED.  The group that produces frame t loads the whole rows t + (j - c) d
// anyway (all C channels of each), so the moments of each tap row cost 2 log2(G) shuffles per row and no byte of traffic; a side
// array [M][K][2] would need a pass of its own over h1 to be written (the product's epilogue does not see whole frames).  The
// backward pass needs the moments of its own frame only.
// The variance is taken from the centred values in registers (sum (v - mu)^2), not from E[v^2] - mu^2.
// Every xor butterfly leaves the same bits in all lanes of the group (each level adds the same two operands on both sides), and
// a frame's result does not depend on which workgroup or lane computes it.
#include "common.h"
#include "det.h"
#include "ctn.h"

// (group_sum, FrameMap and cln_center -- the lane-group sums, the thread layout and a frame's moments -- are in ctn.h)

__global__ __launch_bounds__(256) void ctn_cln_apply_kernel(const bf16_raw* __restrict__ h, const float* __restrict__ slope,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, int K, int C,
                                                            bf16_raw* __restrict__ u) {
    const int m = blockIdx.y, nq = C >> 3;
    const FrameMap fm = frame_map(nq);
    const float a = slope[0], invC = 1.f / (float)C;
    const bf16_raw* base = h + (long)m * K * C + fm.c0;
    bf16_raw* out = u + (long)m * K * C + fm.c0;
    float gm[8], bt[8];
    ld8f(gamma + fm.c0, gm); ld8f(beta + fm.c0, bt);
    for (int t0 = blockIdx.x * fm.rpb; t0 < K; t0 += gridDim.x * fm.rpb) {
        const int t = t0 + fm.rsub;
        const bool ok = fm.act && t < K;
        const C8 x = ok ? ld8(base + (long)t * C) : zero8();
        float d[8];
        const float rs = cln_center(x, a, fm.act, fm.G, invC, d);
        if (ok) {
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = gm[j] * (d[j] * rs) + bt[j];
            st8(out + (long)t * C, o);
        }
    }
}

template <int P, bool CAUSAL>
__global__ __launch_bounds__(256) void ctn_cln_dwconv_fwd_kernel(const bf16_raw* __restrict__ h1, const float* __restrict__ slope1,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 const float* __restrict__ Wd /*[C][P]*/, int dil, int K, int C,
                                                                 bf16_raw* __restrict__ h2) {
    const int m = blockIdx.y, nq = C >> 3;
    const FrameMap fm = frame_map(nq);
    const float a1 = slope1[0], invC = 1.f / (float)C;
    const bf16_raw* base = h1 + (long)m * K * C + fm.c0;
    bf16_raw* out = h2 + (long)m * K * C + fm.c0;
    float gm[8], bt[8], wd[P][8];
    ld8f(gamma + fm.c0, gm); ld8f(beta + fm.c0, bt);
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int p = 0; p < P; ++p) wd[p][j] = Wd[(fm.c0 + j) * P + p];
    for (int t0 = blockIdx.x * fm.rpb; t0 < K; t0 += gridDim.x * fm.rpb) {
        const int t = t0 + fm.rsub;
        const bool ok = fm.act && t < K;
        C8 x[P];
        bool tap[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {          // all loads in flight together
            const int tt = t + (p - (CAUSAL ? P - 1 : P / 2)) * dil;
            tap[p] = tt >= 0 && tt < K;
            x[p] = (ok && tap[p]) ? ld8(base + (long)tt * C) : zero8();
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
}

// Backward of y = cLN(PReLU(h)) in one pass.  dy is read directly (DW = false: g = du) or is the transposed depthwise conv of g = dh2
// (DW = true):  dy[t] = sum_j Wd[j] dh2[t - (j - c) d],  dWd[j] += dh2[t - (j - c) d] n[t]  (n = y of frame t; c = P/2 or P - 1).
// S1 = mean_c(gamma dy) and S2 = mean_c(gamma dy xh) are sums over the frame's own group, so dh is stored right away.
// Per channel: dgamma += dy xh, dbeta += dy [, dWd]; per launch: dslope += dv h [h <= 0].  Every workgroup leaves ONE row
// (dgamma [C] | dbeta [C] | dWd [C][P] (DW only) | dslope) in `part`; ctn_cln_colsum_kernel adds the rows.
template <int P, bool DW, bool CAUSAL>
__global__ __launch_bounds__(256) void ctn_cln_bwd_kernel(const bf16_raw* __restrict__ g, const bf16_raw* __restrict__ h,
                                                          const float* __restrict__ slope, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const float* __restrict__ Wd, int dil, int K, int C,
                                                          bf16_raw* __restrict__ dh, float* __restrict__ part) {
    extern __shared__ float lds[];       // the row of the workgroup: [NV * C + 1]
    const int m = blockIdx.y, nq = C >> 3;
    const FrameMap fm = frame_map(nq);
    constexpr int NV = 2 + (DW ? P : 0), NP = DW ? P : 1;
    const int ncols = NV * C + 1;
    for (int i = threadIdx.x; i < ncols; i += 256) lds[i] = 0.f;
    __syncthreads();
    const float a = slope[0], invC = 1.f / (float)C;
    const bf16_raw* gb = g + (long)m * K * C + fm.c0;
    const bf16_raw* hb = h + (long)m * K * C + fm.c0;
    bf16_raw* out = dh + (long)m * K * C + fm.c0;
    float gm[8], bt[8], wd[NP][8], dg[8], db[8], dw[NP][8];
    float qs = 0.f;
    ld8f(gamma + fm.c0, gm); ld8f(beta + fm.c0, bt);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        dg[j] = 0.f; db[j] = 0.f;
#pragma unroll
        for (int p = 0; p < NP; ++p) { wd[p][j] = DW ? Wd[(fm.c0 + j) * P + p] : 0.f; dw[p][j] = 0.f; }
    }
    for (int t0 = blockIdx.x * fm.rpb; t0 < K; t0 += gridDim.x * fm.rpb) {
        const int t = t0 + fm.rsub;
        const bool ok = fm.act && t < K;
        const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
        const uint4 xr = ok ? ld8raw(hb + (long)t * C) : z4;
        uint4 gr[NP];
        bool tap[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int tt = DW ? t - (p - (CAUSAL ? P - 1 : P / 2)) * dil : t;
            tap[p] = tt >= 0 && tt < K;
            gr[p] = (ok && tap[p]) ? ld8raw(gb + (long)tt * C) : z4;
        }
        const C8 x = unpack8(xr);
        float d[8];
        const float rs = cln_center(x, a, fm.act, fm.G, invC, d);
        float dy[8];
        if (!DW) {
            const C8 g0 = unpack8(gr[0]);
#pragma unroll
            for (int j = 0; j < 8; ++j) dy[j] = g0.v[j];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) dy[j] = 0.f;
#pragma unroll
            for (int p = 0; p < NP; ++p) {          // (rows outside [0, K) were loaded as zeros)
                const C8 gp = unpack8(gr[p]);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    dy[j] += wd[p][j] * gp.v[j];
                    dw[p][j] += gp.v[j] * (gm[j] * (d[j] * rs) + bt[j]);      // (ok = false: gp = 0)
                }
            }
        }
        float s1 = 0.f, s2 = 0.f, xh[8], gd[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            xh[j] = d[j] * rs;
            gd[j] = gm[j] * dy[j];
            s1 += gd[j]; s2 += gd[j] * xh[j];
            dg[j] += dy[j] * xh[j]; db[j] += dy[j];
        }
        group_sum2(s1, s2, fm.G);
        s1 *= invC; s2 *= invC;
        if (ok) {
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float dv = (gd[j] - s1 - xh[j] * s2) * rs;
                const bool pos = x.v[j] > 0.f;
                o[j] = pos ? dv : a * dv;
                if (!pos) qs += dv * x.v[j];
            }
            st8(out + (long)t * C, o);
        }
    }
    // per-channel partials of the workgroup: the lanes of a wave that hold the same channels (G apart) meet by xor-shuffles, then the
    // four waves add their words one after the other with plain read-add-write (a fixed order; see ctn_gln_bwd_reduce_kernel)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        for (int o = fm.G; o < 64; o <<= 1) {
            dg[j] += __shfl_xor(dg[j], o, 64); db[j] += __shfl_xor(db[j], o, 64);
            if (DW) {
#pragma unroll
                for (int p = 0; p < NP; ++p) dw[p][j] += __shfl_xor(dw[p][j], o, 64);
            }
        }
    }
    qs = wave_sum(qs);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int turn = 0; turn < 4; ++turn) {
        if (wave == turn) {
            if (lane < nq) {          // (lane < G: q = lane)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    lds[fm.c0 + j] += dg[j];
                    lds[C + fm.c0 + j] += db[j];
                    if (DW) {
#pragma unroll
                        for (int p = 0; p < NP; ++p) lds[2 * C + (fm.c0 + j) * P + p] += dw[p][j];
                    }
                }
            }
            if (lane == 63) lds[NV * C] += qs;
        }
        __syncthreads();
    }
    float* row = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ncols;
    for (int i = threadIdx.x; i < ncols; i += 256) row[i] = lds[i];
}

// gch[c] += sum over rows of part[row][c] for the per-channel columns, dslope += the last column  (grid = (ceil(ncols / 256), row
// groups); one row group -- the deterministic schedule -- adds all rows in row order, one add per column; caller zeroes gch / dslope)
__global__ __launch_bounds__(256) void ctn_cln_colsum_kernel(const float* __restrict__ part, int nrows, int ncols, float* __restrict__ gch,
                                                             float* __restrict__ dslope) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols) return;
    float s = 0.f;
    for (int r = blockIdx.y; r < nrows; r += gridDim.y) s += part[(size_t)r * ncols + c];
    atomicAdd(c == ncols - 1 ? dslope : &gch[c], s);
}

// ------------------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------------------
// workgroups of the one-pass backward kernel (= rows of partials): each pays the per-channel constants, the LDS image and a partial row
static dim3 ctn_cln_bwd_grid(int M, int K, int C) {
    int G = 1;
    while (G < (C >> 3)) G <<= 1;
    const int rpb = 256 / G;
    static const int total = getenv("SEHIP_CTN_CLN_BLOCKS") ? atoi(getenv("SEHIP_CTN_CLN_BLOCKS")) : 1024;
    long g = (total + M - 1) / M;
    const long cap = ((long)K + rpb - 1) / rpb;
    if (g > cap) g = cap;
    if (g > 64) g = 64;
    if (g < 1) g = 1;
    return dim3((unsigned)g, (unsigned)M);
}

static int ctn_cln_check_p(const char* who, int P) {
    SEHIP_REQUIRE(P == 3 || P == 5 || P == 7, "%s: kernel size P must be 3, 5 or 7 (got %d)", who, P);
    return 0;
}

extern "C" int sehip_ctn_cln_apply(const void* h, const float* slope, const float* gamma, const float* beta, int M, int K, int C, void* u,
                                   void* stream) {
    if (int e = ctn_check("ctn_cln_apply", M, K, C)) return e;
    ctn_cln_apply_kernel<<<ctn_grid(M, K, C), 256, 0, (hipStream_t)stream>>>((const bf16_raw*)h, slope, gamma, beta, K, C, (bf16_raw*)u);
    SEHIP_CHECK_LAUNCH("ctn_cln_apply");
    return 0;
}

extern "C" int sehip_ctn_cln_dwconv_fwd(const void* h1, const float* slope1, const float* gamma, const float* beta, const float* Wd, int P,
                                        int dilation, int causal, int M, int K, int C, void* h2, void* stream) {
    if (int e = ctn_check("ctn_cln_dwconv_fwd", M, K, C)) return e;
    if (int e = ctn_cln_check_p("ctn_cln_dwconv_fwd", P)) return e;
    SEHIP_REQUIRE(dilation >= 1, "ctn_cln_dwconv_fwd: dilation must be positive (got %d)", dilation);
    const dim3 grid = ctn_grid(M, K, C);
#define CTN_CF(P_, CA_) ctn_cln_dwconv_fwd_kernel<P_, CA_><<<grid, 256, 0, (hipStream_t)stream>>>((const bf16_raw*)h1, slope1, gamma, beta, Wd, \
                                                                                                  dilation, K, C, (bf16_raw*)h2)
    if (causal) { if (P == 3) CTN_CF(3, true); else if (P == 5) CTN_CF(5, true); else CTN_CF(7, true); }
    else { if (P == 3) CTN_CF(3, false); else if (P == 5) CTN_CF(5, false); else CTN_CF(7, false); }
#undef CTN_CF
    SEHIP_CHECK_LAUNCH("ctn_cln_dwconv_fwd");
    return 0;
}

extern "C" long sehip_ctn_cln_bwd_scratch_floats(int M, int K, int C) {
    if (M <= 0 || K <= 0 || C < 8) return 0;
    const dim3 grid = ctn_cln_bwd_grid(M, K, C);
    return (long)grid.x * grid.y * (9L * C + 1);          // rows of 2 + P <= 9 values per channel + the slope-gradient sum
}

extern "C" int sehip_ctn_cln_bwd(const void* g, const void* h, const float* slope, const float* gamma, const float* beta, const float* Wd,
                                 int P, int dilation, int dw, int causal, int M, int K, int C, float* gch, void* dh, float* dslope,
                                 float* scratch, void* stream) {
    if (int e = ctn_check("ctn_cln_bwd", M, K, C)) return e;
    if (dw) {
        if (int e = ctn_cln_check_p("ctn_cln_bwd", P)) return e;
        SEHIP_REQUIRE(dilation >= 1, "ctn_cln_bwd: dilation must be positive (got %d)", dilation);
    }
    SEHIP_REQUIRE(scratch != nullptr, "ctn_cln_bwd: missing scratch buffer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid = ctn_cln_bwd_grid(M, K, C);
    const int ncols = (2 + (dw ? P : 0)) * C + 1, nrows = (int)(grid.x * grid.y);
    const size_t lds = (size_t)ncols * sizeof(float);
    bf16_raw* o = (bf16_raw*)dh;
    const bf16_raw *gi = (const bf16_raw*)g, *hi = (const bf16_raw*)h;
#define CTN_CB(P_, CA_) ctn_cln_bwd_kernel<P_, true, CA_><<<grid, 256, lds, st>>>(gi, hi, slope, gamma, beta, Wd, dilation, K, C, o, scratch)
    if (!dw) ctn_cln_bwd_kernel<3, false, false><<<grid, 256, lds, st>>>(gi, hi, slope, gamma, beta, Wd, 1, K, C, o, scratch);
    else if (causal) { if (P == 3) CTN_CB(3, true); else if (P == 5) CTN_CB(5, true); else CTN_CB(7, true); }
    else { if (P == 3) CTN_CB(3, false); else if (P == 5) CTN_CB(5, false); else CTN_CB(7, false); }
#undef CTN_CB
    int rg = nrows / 8;                      // >= 8 rows per thread, up to 64 row groups
    if (rg > 64) rg = 64;
    if (rg < 1 || sehip_deterministic()) rg = 1;
    ctn_cln_colsum_kernel<<<dim3((unsigned)((ncols + 255) / 256), (unsigned)rg), 256, 0, st>>>(scratch, nrows, ncols, gch, dslope);
    SEHIP_CHECK_LAUNCH("ctn_cln_bwd");
    return 0;
}
