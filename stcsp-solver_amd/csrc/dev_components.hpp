// dev_components.hpp -- strongly connected components of the live automaton and the sweeps behind the lasso solutions, on
// the device (contract: stcsp_engine.h, stcsp_engine_components).
//
// There is no reference counterpart. Everything here is level-synchronous: one work item per live edge or per state, a
// launch per sweep, and the host reads one changed word (and the count of the states that have a component) between
// batches of sweeps. No workgroup waits for another: what one sweep writes the next launch reads, and within a launch
// a racing reader can only see a value that is already correct or the older one, which the next sweep mends. Every loop
// in a kernel is bounded by a launch parameter.
//
//   k_s_count / k_s_scan / k_s_fill   (dev_csr.hpp) once: the live edges (alive, both ends live) compacted into 32-bit CSR by
//                      source: off[S + 1], and per position source, destination and the edge's index in the export
//   trim round         k_s_deg marks the states that have an in-edge / an out-edge inside the remaining set (self-loops
//                      do not count), k_s_trim gives every other remaining state its own component
//   colouring round    (Orzan) k_s_colour_init colours the remaining states with their own index; k_s_colour_fwd sweeps
//                      propagate the least colour forward with atomicMin to a fixpoint; a state that kept its index is a
//                      root (k_s_roots) and the least member of its component; k_s_colour_back sweeps collect, inside
//                      one colour, the states that reach the root. The found components leave the remaining set.
//   k_s_bfs            depth[] by one forward breadth-first search, a launch per level
//   k_s_state_info / k_s_edge_info     size, least depth, least depth of a final member and the flags of every component
//                      by atomics, indexed by the component's least member
//   k_s_omega_init / k_s_omega_back    backward reachability from the accepting components
//   k_s_stem_init / k_s_stem_back      64 components per pass, one bit each in a 64-bit word per state: marked backward
//                      from the component's final states of least depth over the edges with depth[v] == depth[u] + 1
//   k_s_loop_init / k_s_loop_back      distance to the anchor over the edges inside a component, all anchors at once
//                      (components are disjoint, so one array serves them all)
// The host walks stems and loops greedily over the pinned export (least full row first).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_csr.hpp"

namespace stcsp {
namespace dev {

constexpr uint32_t kSNone = 0xffffffffu;  // no component yet / not in the remaining set / not reached
enum { S_CHANGED = 0, S_ASSIGNED = 1, S_WORDS = 4 };  // the words the host reads between batches of sweeps
enum { S_INFO_CYCLIC = 1, S_INFO_FINAL = 2, S_INFO_LEAVES = 4 };

// Trim. has_in / has_out are zeroed before the launch.
__global__ void k_s_deg(uint32_t L, const uint32_t *csrc, const uint32_t *cdst, const uint32_t *comp, uint32_t *has_in, uint32_t *has_out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L) return;
    const uint32_t u = csrc[k], v = cdst[k];
    if (u == v || comp[u] != kSNone || comp[v] != kSNone) return;
    has_out[u] = 1u;
    has_in[v] = 1u;
}
__global__ void k_s_trim(uint32_t S, const uint8_t *live, const uint32_t *has_in, const uint32_t *has_out, uint32_t *comp, uint32_t *ctl) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const bool alone = live[s] && comp[s] == kSNone && (!has_in[s] || !has_out[s]);
    if (alone) {
        comp[s] = s;
        ctl[S_CHANGED] = 1u;
    }
    s_tally(alone, &ctl[S_ASSIGNED]);
}

// Colouring. colour[s] != kSNone exactly on the remaining set of this round.
__global__ void k_s_colour_init(uint32_t S, const uint8_t *live, const uint32_t *comp, uint32_t *colour) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    colour[s] = live[s] && comp[s] == kSNone ? s : kSNone;
}
__global__ void k_s_colour_fwd(uint32_t L, const uint32_t *csrc, const uint32_t *cdst, uint32_t *colour, uint32_t *ctl) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L) return;
    const uint32_t u = csrc[k], v = cdst[k];
    const uint32_t cu = __hip_atomic_load(&colour[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t cv = __hip_atomic_load(&colour[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cu == kSNone || cv == kSNone || cu >= cv) return;
    atomicMin(&colour[v], cu);
    ctl[S_CHANGED] = 1u;
}
__global__ void k_s_roots(uint32_t S, const uint32_t *colour, uint32_t *comp, uint32_t *ctl) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const bool root = colour[s] == s;
    if (root) comp[s] = s;
    s_tally(root, &ctl[S_ASSIGNED]);
}
__global__ void k_s_colour_back(uint32_t L, const uint32_t *csrc, const uint32_t *cdst, const uint32_t *colour, uint32_t *comp, uint32_t *ctl) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L) return;
    const uint32_t u = csrc[k], v = cdst[k], c = colour[v];
    if (c == kSNone || colour[u] != c) return;
    if (__hip_atomic_load(&comp[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != c) return;
    if (atomicCAS(&comp[u], kSNone, c) != kSNone) return;
    ctl[S_CHANGED] = 1u;
    atomicAdd(&ctl[S_ASSIGNED], 1u);
}

// depth[] = kSNone but for the root before level 0
__global__ void k_s_bfs(uint32_t L, uint32_t level, const uint32_t *csrc, const uint32_t *cdst, uint32_t *depth, uint32_t *ctl) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L) return;
    const uint32_t v = cdst[k];
    if (depth[csrc[k]] != level || depth[v] != kSNone) return;
    depth[v] = level + 1;  // (every writer of this launch writes the same value)
    ctl[S_CHANGED] = 1u;
}

// Per component, indexed by its least member r: info[r] = size, info[S + r] = flags, info[2 S + r] = least depth,
// info[3 S + r] = least depth of a final member. Initialised to 0, 0, kSNone, kSNone.
__global__ void k_s_state_info(uint32_t S, const uint8_t *live, const uint8_t *fin, const uint32_t *comp, const uint32_t *depth, uint32_t *info) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S || !live[s]) return;
    const uint32_t r = comp[s];
    if (r >= S) return;
    atomicAdd(&info[r], 1u);
    atomicMin(&info[2 * (size_t)S + r], depth[s]);
    if (fin[s]) {
        atomicOr(&info[(size_t)S + r], (uint32_t)S_INFO_FINAL);
        atomicMin(&info[3 * (size_t)S + r], depth[s]);
    }
}
__global__ void k_s_edge_info(uint32_t L, uint32_t S, const uint32_t *csrc, const uint32_t *cdst, const uint32_t *comp, uint32_t *info) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L) return;
    const uint32_t a = comp[csrc[k]], b = comp[cdst[k]];
    if (a >= S) return;
    const uint32_t bit = a == b ? S_INFO_CYCLIC : S_INFO_LEAVES;
    if (!(info[(size_t)S + a] & bit)) atomicOr(&info[(size_t)S + a], bit);
}

__global__ void k_s_omega_init(uint32_t S, const uint8_t *live, const uint32_t *comp, const uint32_t *info, uint8_t *omega) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const uint32_t r = live[s] ? comp[s] : kSNone, want = S_INFO_CYCLIC | S_INFO_FINAL;
    omega[s] = r < S && (info[(size_t)S + r] & want) == want;
}
__global__ void k_s_omega_back(uint32_t L, const uint32_t *csrc, const uint32_t *cdst, uint8_t *omega, uint32_t *ctl) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L) return;
    const uint32_t u = csrc[k];
    if (!omega[cdst[k]] || omega[u]) return;
    omega[u] = 1;
    ctl[S_CHANGED] = 1u;
}

// Stems: sel[0 .. n_sel) are the least members of the components of this pass (n_sel <= 64); bit j of mark[s] = s lies on
// a shortest path from the root to a final state of least depth of component sel[j].
__global__ void k_s_stem_init(uint32_t S, int n_sel, const uint32_t *sel, const uint8_t *live, const uint8_t *fin, const uint32_t *comp,
                              const uint32_t *depth, const uint32_t *info, unsigned long long *mark) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    unsigned long long m = 0;
    if (live[s] && fin[s]) {
        const uint32_t r = comp[s];
        if (r < S && depth[s] == info[3 * (size_t)S + r])
            for (int j = 0; j < n_sel; j++)
                if (sel[j] == r) m |= 1ull << j;
    }
    mark[s] = m;
}
__global__ void k_s_stem_back(uint32_t L, uint32_t level, const uint32_t *csrc, const uint32_t *cdst, const uint32_t *depth, unsigned long long *mark) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L) return;
    const uint32_t u = csrc[k], v = cdst[k];
    if (depth[u] != level || depth[v] != level + 1) return;
    const unsigned long long m = mark[v];  // (level + 1 is complete: the launch before this one wrote it)
    if (m) atomicOr(&mark[u], m);
}

// Loops: dist[] = kSNone but 0 at the anchors
__global__ void k_s_loop_init(uint32_t n, uint32_t S, const uint32_t *anchors, uint32_t *dist) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || anchors[i] >= S) return;
    dist[anchors[i]] = 0u;
}
__global__ void k_s_loop_back(uint32_t L, uint32_t level, const uint32_t *csrc, const uint32_t *cdst, const uint32_t *comp, uint32_t *dist,
                              uint32_t *ctl) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L) return;
    const uint32_t u = csrc[k], v = cdst[k];
    if (comp[u] != comp[v] || dist[v] != level || dist[u] != kSNone) return;
    dist[u] = level + 1;  // (every writer of this launch writes the same value)
    ctl[S_CHANGED] = 1u;
}

}  // namespace dev
}  // namespace stcsp
