// dev_optimise.hpp -- optimal solution streams on the device: the least cost of a solution prefix per length, its
// lexicographically least witness, and the minimum cycle mean of every cyclic component (contract: stcsp_engine.h,
// stcsp_engine_optimise).
//
// There is no reference counterpart. Everything is level-synchronous: one work item per live edge or per state, a launch
// per level, and the host does not look between the launches of a phase. The relaxations are 64-bit atomicMin into a row
// that an earlier launch set to kOptNone; min commutes, so the result depends on no scheduling. No workgroup waits for
// another: launch boundaries are the only ordering between workgroups. Every loop is bounded by a launch parameter.
// The kernels only ever minimise; the host negates the weights to maximise.
//
// The live edges come as 32-bit CSR by source (k_s_count / k_s_scan / k_s_fill of dev_csr.hpp, built for this call into the
// services' one CSR group): off[S + 1], and per position source, destination and the edge's index in the export.
//
//   k_opt_cost           per position: c = sum_v weights[v] * values[eid][v] in int64, once per call
//   k_opt_init           V_0[s] = 0 on the live states (the live final ones under END_FINAL), kOptNone elsewhere
//   k_opt_relax_back     level k: V_k[src] = min(V_k[src], c + V_{k-1}[dst]), skipping kOptNone
//   k_opt_clear          after level k: sets the row of level k + 1 to kOptNone and keeps best[k] = V_k[root]
//   k_opt_walk           one wavefront per requested length: the greedy walk over the rows V_0 .. V_L; the lanes stride over
//                      the state's CSR segment, walk_least_row (dev_csr.hpp) picks the least full row among the tight edges
//   k_opt_karp_init      all cyclic components at once (they are disjoint, so one pair of rows serves them all):
//                      D_0 = 0 at every component's least member, kOptNone elsewhere
//   k_opt_karp_fwd       level k: D_k[dst] = min(D_k[dst], D_{k-1}[src] + c) over the edges whose two ends share a component
//   k_opt_karp_keep      pass 1, after level k: keeps D_n[v] = D_k[v] where k == size(component(v)); clears the next row
//   k_opt_karp_ratio     pass 2, at level k: per state the greatest (D_n - D_k) / (n - k) over k < n as an exact pair,
//                      compared by cross-multiplication; clears the next row
//   k_opt_karp_min       per component the state with the least such pair (ties: the least state), by compare-and-swap
//                      on the state's index
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_csr.hpp"

namespace stcsp {
namespace dev {

constexpr long long kOptNone = 0x7fffffffffffffffll;  // STCSP_OPT_NONE: no path / not reached
constexpr uint32_t kOptIdxNone = 0xffffffffu;
enum { OPT_DUPLICATE = 0, OPT_STUCK = 1, OPT_WORDS = 4 };  // error words of k_opt_walk and k_opt_karp_min

__global__ void k_opt_cost(uint32_t L, int N, const uint32_t *ceid, const int32_t *val, const int32_t *weights, long long *cost) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L) return;
    const int32_t *row = val + (size_t)ceid[k] * N;
    long long c = 0;
    for (int x = 0; x < N; x++) c += (long long)weights[x] * (long long)row[x];
    cost[k] = c;
}

__global__ void k_opt_init(uint32_t S, const uint8_t *live, const uint8_t *fin, int end_final, long long *row) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    row[s] = live[s] && (!end_final || fin[s]) ? 0ll : kOptNone;
}

__global__ void k_opt_relax_back(uint32_t L, const uint32_t *csrc, const uint32_t *cdst, const long long *cost, const long long *prev, long long *cur) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L) return;
    const long long d = prev[cdst[k]];
    if (d == kOptNone) return;
    atomicMin(&cur[csrc[k]], cost[k] + d);
}

// next: the row of the level after `cur`'s (not `cur`, not the row `cur` was relaxed from while that launch ran)
__global__ void k_opt_clear(uint32_t S, long long *next, const long long *cur, long long *best_slot) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    if (next) next[s] = kOptNone;
    if (s == 0) *best_slot = cur[0];
}

// One wavefront per requested length: block j walks lengths[j] steps from the root over the rows V_0 .. V_L (rows[k * S + s])
// and writes the CSR positions' export edge indices to out_eid[woff[j] + t] and the entered states to out_state. A length
// whose best is kOptNone writes nothing (its witness is empty: woff[j + 1] == woff[j]).
__global__ void __launch_bounds__(64) k_opt_walk(uint32_t S, int N, int n_lengths, const int32_t *lengths, const long long *woff, const long long *rows,
                                               const uint32_t *off, const uint32_t *cdst, const uint32_t *ceid, const long long *cost,
                                               const int32_t *val, uint32_t *out_eid, uint32_t *out_state, uint32_t *ctl) {
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= n_lengths) return;
    const int len = lengths[j];
    if (woff[j + 1] - woff[j] != (long long)len) return;
    uint32_t s = 0;
    for (int left = len; left > 0; left--) {
        const long long want = rows[(size_t)left * S + s];
        const long long *below = rows + (size_t)(left - 1) * S;
        bool dup = false;
        const uint32_t best = walk_least_row(off, s, lane, ceid, val, N, [&](uint32_t k) {  // the tight edges
            const long long d = below[cdst[k]];
            return d != kOptNone && cost[k] + d == want;
        }, &dup);
        if (dup) {
            if (lane == 0) ctl[OPT_DUPLICATE] = 1u + s;
            return;
        }
        if (best == kRowNone) {  // (cannot happen: V_k[s] is the minimum over exactly these edges)
            if (lane == 0) ctl[OPT_STUCK] = 1u + s;
            return;
        }
        s = cdst[best];
        if (lane == 0) {
            out_eid[woff[j] + (len - left)] = ceid[best];
            out_state[woff[j] + (len - left)] = s;
        }
    }
}

// Karp, all cyclic components at once. n_of[v] = the size of v's component when that is cyclic, else 0; comp[v] = its number
// (kOptIdxNone outside the live automaton); least[c] = the least member of component c.
__global__ void k_opt_karp_init(uint32_t S, const uint32_t *n_of, const uint32_t *comp, const uint32_t *least, long long *d0, long long *d1,
                              long long *dn) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    d0[s] = n_of[s] && least[comp[s]] == s ? 0ll : kOptNone;
    d1[s] = kOptNone;
    if (dn) dn[s] = kOptNone;  // (pass 1)
}

__global__ void k_opt_karp_fwd(uint32_t L, const uint32_t *csrc, const uint32_t *cdst, const uint32_t *comp, const long long *cost, const long long *prev,
                             long long *cur) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L) return;
    const uint32_t u = csrc[k], v = cdst[k];
    if (comp[u] != comp[v]) return;
    const long long d = prev[u];
    if (d == kOptNone) return;
    atomicMin(&cur[v], d + cost[k]);
}

// cur = D_level (complete); next = the other row, which becomes D_(level + 1)
__global__ void k_opt_karp_keep(uint32_t S, uint32_t level, const uint32_t *n_of, const long long *cur, long long *next, long long *dn) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    if (n_of[s] == level) dn[s] = cur[s];
    next[s] = kOptNone;
}

// den[s] == 0: no pair yet. Every product stays below 2^63: |D_n - D_k| < 2 nmax cmax, the denominators are <= nmax, and the
// host has checked nmax^2 cmax <= 2^62.
__global__ void k_opt_karp_ratio(uint32_t S, uint32_t level, const uint32_t *n_of, const long long *cur, long long *next, const long long *dn,
                               long long *num, uint32_t *den) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    next[s] = kOptNone;
    const uint32_t n = n_of[s];
    if (level >= n || dn[s] == kOptNone || cur[s] == kOptNone) return;
    const long long a = dn[s] - cur[s], b = (long long)(n - level);
    if (den[s] == 0 || a * (long long)den[s] > num[s] * b) {
        num[s] = a;
        den[s] = (uint32_t)b;
    }
}

// arg[c] = the state of component c with the least pair (ties: the least state). A compare-and-swap that fails means that
// another state's pair went in, which is below the one read: a state retries at most size(c) times, bound = S.
__global__ void k_opt_karp_min(uint32_t S, uint32_t bound, const uint32_t *comp, const long long *num, const uint32_t *den, uint32_t *arg, uint32_t *ctl) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S || den[s] == 0) return;
    uint32_t *slot = &arg[comp[s]];
    uint32_t seen = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t tries = 0; tries <= bound; tries++) {
        if (seen != kOptIdxNone) {
            const long long mine = num[s] * (long long)den[seen], theirs = num[seen] * (long long)den[s];
            if (mine > theirs || (mine == theirs && seen < s)) return;
        }
        const uint32_t old = atomicCAS(slot, seen, s);
        if (old == seen) return;
        seen = old;
    }
    ctl[OPT_STUCK] = 1u + s;
}

}  // namespace dev
}  // namespace stcsp
