// julius.resample_frac (resample.hip) chunk by chunk, for rows that resume from carried state (sehip.ResampleStreamer).
//
// With the ratio reduced to old / new, K = 2 * width + old, the offline output of a row of n samples is
//     y[q * new + p] = sum_{k < K} kernels[p][k] * x[clamp(q * old + k - width, 0, n - 1)],   q * new + p < floor(n * new / old)
// The `new` outputs with the same q are a frame; a frame consumes `old` input samples.  Frame q reads input up to sample
// q * old + width + old - 1, so after F input frames the frames q <= F - 1 - Dq are computable, Dq = ceil(width / old): a call that
// takes the input frames F .. F + f - 1 returns the output frames F - Dq .. F + f - 1 - Dq (zeros for q < 0), a fixed delay of
// Dq * new output samples.  Those frames read the samples F * old - H .. (F + f) * old - 1, H = Dq * old + width.
//
// State of a row, all on the device:
//     pos   int64                      input frames fed since the row was fresh (reset: pos = 0)
//     ring  fp32 [L], L = H + C * old  input sample a sits at slot a mod L
//   C = chunk_frames is the largest chunk.  The ring is one chunk longer than the history: the f * old slots a chunk writes (samples
//   pos * old ..) are never the H slots it reads, and nothing is copied.  A sample index below 0 reads sample 0 (replicate padding, as
//   offline; sample 0 is still in the ring, or in the chunk, whenever such an index can occur), so a reset clears nothing.
//   The end of a stream: a call with end >= 0 says that the row's last sample is chunk sample end - 1 (end = 0: the sample before the
//   chunk).  Chunk samples from `end` on read as that sample -- in the window AND in what goes into the ring, so the ring then holds the
//   replicate-padded stream and further calls with end = 0 continue it.  That is offline's right-hand clamp.
//
// A chunk is two launches with the same arguments every time (the position is read on the device: capturable):
//   1 rss_feed_kernel     grid (tiles of ft frames, rows), 256 threads.  A workgroup stages the window of its tile, (tn - 1) * old + K
//                         samples of [ring history | chunk] with both clamps applied, in LDS, then one thread per output sample
//                         (lane = phase within a frame: the lanes of a frame read the same LDS word -- a broadcast -- and consecutive
//                         words of the TRANSPOSED table [K][new]) sums its K products in the order of the offline kernel that serves
//                         the ratio (resample_plan.h), with explicit fused multiply-adds: the bits of the offline sample.
//                             phase  : two chains over segments of `old` taps; quads put taps c, c + 2 on chain x and c + 1, c + 3 on
//                                      chain y, the cnt % 4 leftovers go on x; x + y at the end (resample_phase_kernel)
//                             decim  : one chain, residue c = k mod old outer, j inner (resample_decim_kernel)
//                             direct : one chain over k (resample_direct_kernel)
//                         The workgroup also stores its tile's chunk samples into the ring.  A window that does not fit the LDS (K
//                         above ~16000: old near 1024 against new <= 3) is read straight from global memory, same order.
//   2 rss_advance_kernel  pos += f (each thread its own word).
// No launch reads an address that it writes (the advance's own words excepted, as the other streamers' counters); no workgroup waits
// on another; no atomics; every output has one owner and a fixed order: the same bits from run to run.
#include "common.h"
#include "resample_plan.h"

namespace {
typedef __attribute__((ext_vector_type(2))) float f32x2;
constexpr int RSS_MAX_TERM = 1024;
constexpr int RSS_MAX_WIDTH = 1 << 16;
constexpr int RSS_CMAX = 4096;                    // chunk_frames
constexpr int RSS_THREADS = 256;
constexpr size_t RSS_LDS_MAX = 64 * 1024;         // the default dynamic-LDS limit: no per-device attribute to set

// where a row's samples are, relative to the first sample of the chunk (index i: i >= 0 the chunk, i < 0 the ring's history)
struct rss_src {
    const float* xr;     // the row's chunk
    const float* rg;     // the row's ring
    long base;           // pos * old: the stream index of chunk sample 0
    long slot0;          // base mod L
    long L;
    int end;             // >= 0: chunk samples from `end` on read as sample end - 1
};

// sample i, -H <= i < frames * old, with both clamps
__device__ __forceinline__ float rss_sample(const rss_src& s, long i) {
    if (s.end >= 0 && i > s.end - 1) i = s.end - 1;
    if (s.base + i < 0) i = -s.base;                              // (then base < H: sample 0 has not been overwritten)
    if (i >= 0) return s.xr[i];
    long slot = s.slot0 + i;                                      // -L < i < 0
    slot = slot < 0 ? slot + s.L : slot;
    return s.rg[slot];
}

template <bool STAGED>
struct rss_window {
    const float* xs;     // STAGED: the frame's window in LDS
    const rss_src* src;  // otherwise: global memory,
    long i0;             //            the frame's first window sample
    __device__ __forceinline__ float operator()(int k) const {
        if (STAGED) return xs[k];
        return rss_sample(*src, i0 + k);
    }
};

template <int KIND, bool STAGED>
__global__ __launch_bounds__(RSS_THREADS) void rss_feed_kernel(const float* __restrict__ xin, int frames, int C, const float* __restrict__ table_t,
                                                               int old_sr, int new_sr, int width, int dq, int ft,
                                                               const long* __restrict__ pos, float* __restrict__ ring, long L, int end,
                                                               float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float rss_x[];  // window sample j <-> chunk index w0 + j
    const int K = 2 * width + old_sr;
    const long r = blockIdx.y;
    const long F = pos[r];
    rss_src src;
    src.xr = xin + r * (long)C * old_sr;
    src.rg = ring + r * L;
    src.base = F * old_sr;
    src.slot0 = src.base % L;
    src.L = L;
    src.end = end;
    const int f0 = blockIdx.x * ft;
    const int tn = frames - f0 < ft ? frames - f0 : ft;           // frames of this tile
    const long w0 = (long)(f0 - dq) * old_sr - width;             // >= -H; the last window sample is (f0 + tn - dq) * old + width - 1
    if (STAGED) {
        const int W = (tn - 1) * old_sr + K;
        for (int j = threadIdx.x; j < W; j += RSS_THREADS) rss_x[j] = rss_sample(src, w0 + j);
    }
    // the tile's share of the chunk goes into the ring (slots that no workgroup of this launch reads)
    float* rg = ring + r * L;
    for (int j = f0 * old_sr + threadIdx.x; j < (f0 + tn) * old_sr; j += RSS_THREADS) {
        long slot = src.slot0 + j;                                // j < C * old <= L
        slot = slot >= L ? slot - L : slot;
        rg[slot] = rss_sample(src, j);
    }
    if (STAGED) __syncthreads();
    float* y = out + r * (long)C * new_sr + (long)f0 * new_sr;
    for (int o = threadIdx.x; o < tn * new_sr; o += RSS_THREADS) {
        const int g = o / new_sr, p = o - g * new_sr;
        rss_window<STAGED> x = {rss_x + g * old_sr, &src, w0 + (long)g * old_sr};
        const float* t = table_t + p;                             // tap k of phase p at t[k * new]
        float res;
        if (KIND == RS_PHASE) {
            f32x2 acc = {0.f, 0.f};
            for (int k0 = 0; k0 < K; k0 += old_sr) {
                const int cnt = K - k0 < old_sr ? K - k0 : old_sr;
                int c = 0;
                for (; c + 4 <= cnt; c += 4) {
                    const int k = k0 + c;
                    const f32x2 t01 = {t[(long)k * new_sr], t[(long)(k + 1) * new_sr]}, t23 = {t[(long)(k + 2) * new_sr], t[(long)(k + 3) * new_sr]};
                    const f32x2 x01 = {x(k), x(k + 1)}, x23 = {x(k + 2), x(k + 3)};
                    acc = __builtin_elementwise_fma(t01, x01, acc);
                    acc = __builtin_elementwise_fma(t23, x23, acc);
                }
                for (; c < cnt; ++c) acc.x = fmaf(t[(long)(k0 + c) * new_sr], x(k0 + c), acc.x);
            }
            res = acc.x + acc.y;
        } else if (KIND == RS_DECIM) {
            float acc = 0.f;
            for (int c = 0; c < old_sr; ++c) {
                const int jn = (K - c + old_sr - 1) / old_sr;
                for (int j = 0; j < jn; ++j) {
                    const int k = j * old_sr + c;
                    acc = fmaf(t[(long)k * new_sr], x(k), acc);
                }
            }
            res = acc;
        } else {
            float acc = 0.f;
            for (int k = 0; k < K; ++k) acc = fmaf(t[(long)k * new_sr], x(k), acc);
            res = acc;
        }
        y[o] = F - dq + f0 + g < 0 ? 0.f : res;                   // a frame before the stream's first: the delay's zeros
    }
}

__global__ __launch_bounds__(RSS_THREADS) void rss_advance_kernel(long* __restrict__ pos, long rows, int frames) {
    const long r = (long)blockIdx.x * RSS_THREADS + threadIdx.x;
    if (r < rows) pos[r] += frames;
}

long rss_gcd(long a, long b) {
    while (b) { const long t = a % b; a = b; b = t; }
    return a;
}

bool rss_ratio_ok(int old_sr, int new_sr, int width) {
    return old_sr >= 1 && new_sr >= 1 && old_sr <= RSS_MAX_TERM && new_sr <= RSS_MAX_TERM && old_sr != new_sr && rss_gcd(old_sr, new_sr) == 1 &&
           width >= 1 && width <= RSS_MAX_WIDTH;
}

long rss_dq(int old_sr, int width) { return ((long)width + old_sr - 1) / old_sr; }
long rss_ring(int old_sr, int width, int C) { return rss_dq(old_sr, width) * old_sr + width + (long)C * old_sr; }
}  // namespace

extern "C" long sehip_rss_delay_frames(int old_sr, int new_sr, int width) {
    if (!rss_ratio_ok(old_sr, new_sr, width)) return -1;
    return rss_dq(old_sr, width);
}

extern "C" long sehip_rss_state_bytes(long rows, int old_sr, int new_sr, int width, int chunk_frames) {
    if (rows < 1 || rows > 65535 || !rss_ratio_ok(old_sr, new_sr, width) || chunk_frames < 1 || chunk_frames > RSS_CMAX) return 0;
    return rows * (8 + 4 * rss_ring(old_sr, width, chunk_frames));
}

extern "C" int sehip_rss_feed(const float* xin, long rows, int frames, int chunk_frames, const float* table_t, int old_sr, int new_sr, int width,
                              const long* pos, float* ring, long end_len, float* out, void* stream) {
    SEHIP_REQUIRE(rows >= 1 && rows <= 65535, "rss_feed: rows=%ld outside [1, 65535]", rows);
    SEHIP_REQUIRE(old_sr >= 1 && new_sr >= 1 && old_sr <= RSS_MAX_TERM && new_sr <= RSS_MAX_TERM,
                  "rss_feed: ratio %d -> %d has a term outside [1, %d]", old_sr, new_sr, RSS_MAX_TERM);
    SEHIP_REQUIRE(rss_gcd(old_sr, new_sr) == 1 && old_sr != new_sr, "rss_feed: ratio %d -> %d is not reduced (or is 1 -> 1: nothing to do)",
                  old_sr, new_sr);
    SEHIP_REQUIRE(width >= 1 && width <= RSS_MAX_WIDTH, "rss_feed: width=%d outside [1, %d]", width, RSS_MAX_WIDTH);
    SEHIP_REQUIRE(chunk_frames >= 1 && chunk_frames <= RSS_CMAX, "rss_feed: chunk_frames C=%d outside [1, %d]", chunk_frames, RSS_CMAX);
    SEHIP_REQUIRE(frames >= 1 && frames <= chunk_frames, "rss_feed: frames=%d outside [1, chunk_frames = %d]", frames, chunk_frames);
    SEHIP_REQUIRE(end_len <= (long)frames * old_sr, "rss_feed: end_len=%ld beyond the chunk's %ld samples", end_len, (long)frames * old_sr);
    SEHIP_REQUIRE(xin && table_t && pos && ring && out, "rss_feed: null pointer");
    const rs_plan pl = rs_make_plan(old_sr, new_sr, width);         // the order of the kernel that serves this ratio offline
    const int dq = (int)rss_dq(old_sr, width), end = end_len < 0 ? -1 : (int)end_len;
    const long K = pl.K, L = rss_ring(old_sr, width, chunk_frames);
    // ft frames per workgroup: about one output per thread, no more than the chunk has, a window that fits the LDS
    int ft = (RSS_THREADS + new_sr - 1) / new_sr;
    ft = ft < frames ? ft : frames;
    while (ft > 1 && (size_t)((long)(ft - 1) * old_sr + K) * sizeof(float) > RSS_LDS_MAX) ft >>= 1;
    const size_t lds = (size_t)((long)(ft - 1) * old_sr + K) * sizeof(float);
    const bool staged = lds <= RSS_LDS_MAX;
    const dim3 grid((unsigned)((frames + ft - 1) / ft), (unsigned)rows);
    hipStream_t st = (hipStream_t)stream;
#define RSS_LAUNCH(KIND)                                                                                                              \
    do {                                                                                                                              \
        if (staged)                                                                                                                   \
            rss_feed_kernel<KIND, true><<<grid, RSS_THREADS, lds, st>>>(xin, frames, chunk_frames, table_t, old_sr, new_sr, width, dq, ft, pos, \
                                                                        ring, L, end, out);                                           \
        else                                                                                                                          \
            rss_feed_kernel<KIND, false><<<grid, RSS_THREADS, 0, st>>>(xin, frames, chunk_frames, table_t, old_sr, new_sr, width, dq, ft, pos,  \
                                                                       ring, L, end, out);                                            \
    } while (0)
    if (pl.kind == RS_PHASE) RSS_LAUNCH(RS_PHASE);
    else if (pl.kind == RS_DECIM) RSS_LAUNCH(RS_DECIM);
    else RSS_LAUNCH(RS_DIRECT);
#undef RSS_LAUNCH
    SEHIP_CHECK_LAUNCH("rss_feed");
    sehip_note_kernel("resample_stream order=%s old=%d new=%d K=%ld ft=%d tiles=%u lds=%zu", pl.kind == RS_PHASE ? "phase" : pl.kind == RS_DECIM ? "decim" : "direct",
                      old_sr, new_sr, K, ft, grid.x, staged ? lds : (size_t)0);
    return 0;
}

extern "C" int sehip_rss_advance(long* pos, long rows, int frames, void* stream) {
    SEHIP_REQUIRE(rows >= 1 && rows <= 65535, "rss_advance: rows=%ld outside [1, 65535]", rows);
    SEHIP_REQUIRE(frames >= 1 && frames <= RSS_CMAX, "rss_advance: frames=%d outside [1, %d]", frames, RSS_CMAX);
    SEHIP_REQUIRE(pos, "rss_advance: null pointer");
    rss_advance_kernel<<<(unsigned)((rows + RSS_THREADS - 1) / RSS_THREADS), RSS_THREADS, 0, (hipStream_t)stream>>>(pos, rows, frames);
    SEHIP_CHECK_LAUNCH("rss_advance");
    return 0;
}
