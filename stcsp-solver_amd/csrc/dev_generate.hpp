// dev_generate.hpp -- counting, enumerating and sampling solution prefixes on the device.
//
// There is no reference counterpart. Contract: stcsp_engine.h, stcsp_engine_generate. The pass runs where dev_monitor.hpp
// runs, over the same structure-of-arrays edge list and the flags postprocess() left in HBM. It is the converse of the
// monitor: that one follows given rows through the automaton, this one chooses the rows.
//
// Build, once per (mask, horizon, flags):
//   k_q_reach     (dev_quotient.hpp) the live states.
//   k_g_degree    one lane per edge: live out-degree of every state (dead edges and edges of non-live states left out).
//   k_g_scan_*    exclusive scan of the degrees over the states: tile sums (kGenScanTile states per block), a one-block scan
//                 of the tile sums that walks them in chunks with a carry (any number of tiles), and the tiles again with
//                 their offsets. The scanned offsets are written twice: off[] stays, cur[] is the fill cursor.
//   k_g_fill      one lane per edge: seg[atomicAdd(&cur[src], 1)] = edge. The order inside a segment is the scheduler's.
//   k_g_order     one wavefront per state puts the segment into canonical order (full row, then edge index). Lanes take
//                 the edges of the segment in chunks of 64; a lane ranks its edge by counting the edges of the segment
//                 that come before it (the other edge's id and row are wave-uniform loads, a row compare stops at the first
//                 difference) and writes edge id and destination at that rank: O(d^2) compares per state over 64 lanes, no
//                 scratch, no LDS. A segment longer than kGenWaveSegment is heap-sorted in place by one lane instead,
//                 O(d log d): the order is a strict total order, so both roads give the same permutation.
//   k_g_level0    W_0.
//   k_g_weights   once per level, one lane per state: W_{t+1}(s) = the sequential sum of W_t(dst) over the ordered segment.
//                 The launches are the dependency between levels. The lane of the root also leaves count[t + 1].
// Generate:
//   k_g_generate  one lane per stream, both modes (template). Per step: W_r(s) (8 B, sample only), then 4 + 8 B per
//                 scanned edge (destination, its weight), then the chosen edge's id and its row of n_vars * 4 B; the
//                 projected row goes out by plain vector stores. `len` dependent look-ups: latency bound, like k_m_walk_det.
//
// Floating point: one add, one subtract, one multiply or one compare at a time, contraction off: see the contract.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_quotient.hpp"

namespace stcsp {
namespace dev {

constexpr uint32_t kGenWaveSegment = 4096;  // longest segment k_g_order ranks by counting; longer ones are sorted by one lane
constexpr int kGenScanItems = 4;            // states per lane in the scan
constexpr int kGenScanTile = 256 * kGenScanItems;
// the words the host reads
enum { G_MAXDEG = 0, G_ERROR = Q_ERROR, G_WORDS = 4 };
enum { G_ERR_NO_EDGE = 8 };

__device__ inline bool g_edge_live(uint32_t e, const long long *src, const long long *dst, const uint8_t *alive, const uint8_t *live) {
    return alive[e] && live[src[e]] && live[dst[e]];
}

__global__ void k_g_degree(uint32_t E, const long long *src, const long long *dst, const uint8_t *alive, const uint8_t *live, uint32_t *deg) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E || !g_edge_live(e, src, dst, alive, live)) return;
    atomicAdd(&deg[(uint32_t)src[e]], 1u);
}

// Exclusive scan of x over one block of 256 lanes; *total = the sum (valid in every lane). tmp: 4 words of LDS.
__device__ inline uint32_t g_block_scan(uint32_t x, uint32_t *tmp, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = x;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
    }
    __syncthreads();  // (tmp may still be read from the call before)
    if (lane == 63) tmp[wave] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (int w = 0; w < 4; w++) {
        if (w < wave) base += tmp[w];
        all += tmp[w];
    }
    *total = all;
    return base + incl - x;
}

// blocks of 256 lanes, tile b = states [b * kGenScanTile, (b + 1) * kGenScanTile)
__global__ __launch_bounds__(256) void k_g_scan_tiles(uint32_t S, const uint32_t *deg, uint32_t *tile_sum) {
    __shared__ uint32_t tmp[4];
    const uint32_t first = blockIdx.x * kGenScanTile + threadIdx.x * kGenScanItems;
    uint32_t x = 0, total;
    for (int i = 0; i < kGenScanItems; i++)
        if (first + i < S) x += deg[first + i];
    g_block_scan(x, tmp, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one block: tile_sum[0 .. n) -> its exclusive scan in place, tile_sum[n] = the total
__global__ __launch_bounds__(256) void k_g_scan_sums(uint32_t n, uint32_t *tile_sum) {
    __shared__ uint32_t tmp[4];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t x = i < n ? tile_sum[i] : 0u;
        uint32_t total;
        const uint32_t excl = g_block_scan(x, tmp, &total);
        if (i < n) tile_sum[i] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) tile_sum[n] = carry;
}

// deg may be cur: a lane reads its own items before it writes them
__global__ __launch_bounds__(256) void k_g_scan_write(uint32_t S, const uint32_t *deg, const uint32_t *tile_sum, uint32_t n_tiles,
                                                      uint32_t *off, uint32_t *cur) {
    __shared__ uint32_t tmp[4];
    const uint32_t first = blockIdx.x * kGenScanTile + threadIdx.x * kGenScanItems;
    uint32_t d[kGenScanItems], x = 0, total;
    for (int i = 0; i < kGenScanItems; i++) {
        d[i] = first + i < S ? deg[first + i] : 0u;
        x += d[i];
    }
    uint32_t at = tile_sum[blockIdx.x] + g_block_scan(x, tmp, &total);
    for (int i = 0; i < kGenScanItems; i++)
        if (first + i < S) {
            off[first + i] = at;
            cur[first + i] = at;
            at += d[i];
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) off[S] = tile_sum[n_tiles];
}

// seg has off[S] entries; a cursor stays inside its state's segment because k_g_degree counted with the same predicate
__global__ void k_g_fill(uint32_t E, const long long *src, const long long *dst, const uint8_t *alive, const uint8_t *live, uint32_t *cur,
                         uint32_t *seg) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E || !g_edge_live(e, src, dst, alive, live)) return;
    seg[atomicAdd(&cur[(uint32_t)src[e]], 1u)] = e;
}

// canonical order: row of a before row of b, or the same row and a < b
__device__ inline bool g_before(uint32_t a, uint32_t b, const int32_t *values, int N) {
    const int32_t *ra = values + (size_t)a * N, *rb = values + (size_t)b * N;
    for (int i = 0; i < N; i++) {
        const int32_t x = ra[i], y = rb[i];
        if (x != y) return x < y;
    }
    return a < b;
}

__device__ inline void g_sift_down(uint32_t *h, uint32_t root, uint32_t n, const int32_t *values, int N) {
    for (;;) {
        uint32_t child = 2 * root + 1;
        if (child >= n) return;
        if (child + 1 < n && g_before(h[child], h[child + 1], values, N)) child++;
        if (!g_before(h[root], h[child], values, N)) return;
        const uint32_t x = h[root];
        h[root] = h[child];
        h[child] = x;
        root = child;
    }
}

// One wavefront per state: blocks of 256 lanes take 4 states. seg: the segments as k_g_fill left them (sorted in place on
// the long road); eid / dstp: the ordered edge ids and their destinations.
__global__ __launch_bounds__(256) void k_g_order(uint32_t S, const uint32_t *off, uint32_t *seg, const long long *dst, const int32_t *values,
                                                 int N, uint32_t *eid, uint32_t *dstp, uint32_t *ctl) {
    const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= S) return;
    const uint32_t b = off[s], d = off[s + 1] - b;
    if (d == 0) return;
    if (lane == 0) atomicMax(&ctl[G_MAXDEG], d);
    if (d > kGenWaveSegment) {
        if (lane != 0) return;
        uint32_t *h = seg + b;
        for (uint32_t i = d / 2; i-- > 0;) g_sift_down(h, i, d, values, N);
        for (uint32_t n = d - 1; n > 0; n--) {
            const uint32_t x = h[0];
            h[0] = h[n];
            h[n] = x;
            g_sift_down(h, 0, n, values, N);
        }
        for (uint32_t i = 0; i < d; i++) {
            eid[b + i] = h[i];
            dstp[b + i] = (uint32_t)dst[h[i]];
        }
        return;
    }
    for (uint32_t c = 0; c < d; c += 64) {
        const uint32_t i = c + lane;
        if (i >= d) continue;  // (no wave-wide operation below)
        const uint32_t mine = seg[b + i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < d; j++) {
            const uint32_t other = seg[b + j];
            if (other != mine && g_before(other, mine, values, N)) rank++;
        }
        eid[b + rank] = mine;
        dstp[b + rank] = (uint32_t)dst[mine];
    }
}

__global__ void k_g_level0(uint32_t S, const uint8_t *live, const uint8_t *fin, int end_final, double *W, double *count) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const double w = live[s] && (!end_final || fin[s]) ? 1.0 : 0.0;
    W[s] = w;
    if (s == 0) count[0] = w;
}

// W_prev = level t, W_next = level t + 1, count_next = &count[t + 1]
__global__ void k_g_weights(uint32_t S, const uint32_t *off, const uint32_t *dstp, const double *W_prev, double *W_next, double *count_next) {
#pragma clang fp contract(off)
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    double acc = 0.0;
    for (uint32_t k = off[s], end = off[s + 1]; k < end; k++) acc = acc + W_prev[dstp[k]];
    W_next[s] = acc;
    if (s == 0) *count_next = acc;
}

__device__ inline double g_uniform(unsigned long long seed, unsigned long long stream, unsigned long long t) {
#pragma clang fp contract(off)
    const unsigned long long z = q_mix(q_mix(q_mix(seed + 0x9e3779b97f4a7c15ull) + stream) + t);
    return (double)(z >> 11) * 0x1.0p-53;
}

// The root is live and count[len] > 0 (the host answers the other cases itself); ranks are valid. out: [n_streams][len][n_obs].
template <bool UNRANK>
__global__ void k_g_generate(uint32_t n_streams, uint32_t len, unsigned long long seed, const unsigned long long *ranks, uint32_t S,
                             const double *W, const uint32_t *off, const uint32_t *dstp, const uint32_t *eid, const int32_t *values, int N,
                             const int32_t *obs, int n_obs, const uint8_t *fin, int32_t *out, uint8_t *end_final, uint32_t *ctl) {
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_streams) return;
    int32_t *rows = out + (size_t)i * len * n_obs;
    uint32_t s = 0;
    double tau = 0.0;
    if (UNRANK) tau = (double)ranks[i];
    for (uint32_t t = 0; t < len; t++) {
        const uint32_t r = len - t;
        const double *W_next = W + (size_t)(r - 1) * S;
        if (!UNRANK) tau = g_uniform(seed, i, t) * W[(size_t)r * S + s];
        double acc = 0.0, before = 0.0, before_last = 0.0;
        uint32_t pick = kQEmpty, last = kQEmpty;
        for (uint32_t k = off[s], end = off[s + 1]; k < end; k++) {
            const double w = W_next[dstp[k]];
            if (w > 0.0) {
                last = k;
                before_last = acc;
            }
            const double sum = acc + w;
            if (sum > tau) {
                pick = k;
                before = acc;
                break;
            }
            acc = sum;
        }
        if (pick == kQEmpty) {
            pick = last;
            before = before_last;
        }
        if (pick == kQEmpty) {  // no edge of non-zero weight: the tables contradict count[len] > 0; the host refuses the result
            atomicOr(&ctl[G_ERROR], (uint32_t)G_ERR_NO_EDGE);
            break;
        }
        if (UNRANK) tau = tau - before;
        const int32_t *row = values + (size_t)eid[pick] * N;
        for (int v = 0; v < n_obs; v++) rows[(size_t)t * n_obs + v] = row[obs[v]];
        s = dstp[pick];
    }
    end_final[i] = fin[s] ? 1 : 0;
}

}  // namespace dev
}  // namespace stcsp
