// dev_csr.hpp -- what the graph passes on the live automaton share on the device (components, optimisation, fair CTL;
// DESIGN.md section 4.10.1). There is no reference counterpart.
//   k_s_count / k_s_scan / k_s_fill   the edges that are alive and have both ends in a set of states (`live`: the live set, or
//                      the omega-live states for the worlds of CTL) as 32-bit CSR by source: off[S + 1], and per position
//                      source, destination and the edge's index in the export (12 B per edge)
//   walk_least_row     one step of a greedy walk by least full row, by one wavefront
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace stcsp {
namespace dev {

constexpr uint32_t kRowNone = 0xffffffffu;  // walk_least_row: the segment holds no candidate

// ctr += the number of lanes of the wavefront for which pred holds: one atomic per wavefront
__device__ inline void s_tally(bool pred, uint32_t *ctr) {
    const unsigned long long m = __ballot(pred);
    if (pred && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(ctr, (uint32_t)__popcll(m));
}

__device__ inline bool s_live_edge(uint32_t e, const long long *src, const long long *dst, const uint8_t *alive, const uint8_t *live) {
    return alive[e] && live[src[e]] && live[dst[e]];
}

__global__ void k_s_count(uint32_t E, const long long *src, const long long *dst, const uint8_t *alive, const uint8_t *live, uint32_t *deg) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E || !s_live_edge(e, src, dst, alive, live)) return;
    atomicAdd(&deg[src[e]], 1u);
}

// Exclusive scan of deg[0 .. S) by one workgroup of 256: lane t owns the states [t * chunk, (t + 1) * chunk). off[S] = the total.
__global__ void k_s_scan(uint32_t S, uint32_t chunk, const uint32_t *deg, uint32_t *off, uint32_t *cursor) {
    __shared__ uint32_t part[256];
    const uint32_t t = threadIdx.x;
    const unsigned long long base = (unsigned long long)t * chunk;
    uint32_t sum = 0;
    for (uint32_t i = 0; i < chunk; i++)
        if (base + i < S) sum += deg[base + i];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t x = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (uint32_t i = 0; i < chunk; i++)
        if (base + i < S) {
            off[base + i] = run;
            cursor[base + i] = run;
            run += deg[base + i];
        }
    if (t == 255) off[S] = part[255];
}

__global__ void k_s_fill(uint32_t E, const long long *src, const long long *dst, const uint8_t *alive, const uint8_t *live, uint32_t *cursor,
                         uint32_t L, uint32_t *csrc, uint32_t *cdst, uint32_t *ceid) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E || !s_live_edge(e, src, dst, alive, live)) return;
    const uint32_t u = (uint32_t)src[e], k = atomicAdd(&cursor[u], 1u);
    if (k >= L) return;  // (cannot happen: the counts are of the same edges)
    csrc[k] = u;
    cdst[k] = (uint32_t)dst[e];
    ceid[k] = e;
}

// true when the full row of export edge a is lexicographically below that of b; *equal when the rows are the same
__device__ inline bool row_less(const int32_t *val, int N, uint32_t a, uint32_t b, bool *equal) {
    const int32_t *x = val + (size_t)a * N, *y = val + (size_t)b * N;
    for (int i = 0; i < N; i++)
        if (x[i] != y[i]) return x[i] < y[i];
    *equal = true;
    return false;
}

// One step of a greedy walk, by a whole wavefront (every lane calls it with the same s): among the positions k of the CSR
// segment of state s for which candidate(k) holds, the one whose export edge ceid[k] carries the least full row, the same in
// every lane; kRowNone when there is none. *dup becomes true, in every lane, when two candidates carry the same row: an error
// of the automaton, for the caller to report. (Then the lower position wins, which keeps the lanes in step.)
template <typename Candidate>
__device__ inline uint32_t walk_least_row(const uint32_t *off, uint32_t s, int lane, const uint32_t *ceid, const int32_t *val, int N, Candidate candidate, bool *dup) {
    uint32_t best = kRowNone;  // a CSR position
    bool twice = false;
    for (uint32_t k = off[s] + lane; k < off[s + 1]; k += 64) {
        if (!candidate(k)) continue;
        if (best == kRowNone || row_less(val, N, ceid[k], ceid[best], &twice)) best = k;
    }
    for (int step = 32; step > 0; step >>= 1) {
        const uint32_t other = __shfl_xor(best, step);
        if (other == kRowNone || other == best) continue;
        if (best == kRowNone || row_less(val, N, ceid[other], ceid[best], &twice))
            best = other;
        else if (twice && other < best)
            best = other;  // (equal rows: an error anyway; keeps the lanes in step)
    }
    *dup = __any(twice);
    return best;
}

}  // namespace dev
}  // namespace stcsp
