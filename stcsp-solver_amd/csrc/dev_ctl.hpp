// dev_ctl.hpp -- fair CTL over the infinite solutions on the device (contract: stcsp_engine.h, stcsp_engine_ctl; DESIGN.md
// section 4.23). There is no reference counterpart.
//
// The worlds (live edges into omega-live states) are the positions of a CSR by source built by k_s_count / k_s_scan /
// k_s_fill (dev_csr.hpp) into the services' one CSR group, for this call. A set of worlds is a bit set over the positions: the wavefront
// of the lanes [64 j, 64 j + 64) owns word j and writes it whole from __ballot, so no set word is ever written by two
// wavefronts and none needs an atomic; a lane past n_worlds votes 0, which keeps the tail bits of the last word 0.
// Everything is level-synchronous: launch boundaries are the only ordering, no workgroup waits for another, and every loop
// in a kernel is bounded by a launch parameter.
//
//   k_ctl_pred      a maximal temporal-free subformula in one pass over the rows: the lane interprets the postfix slice with
//                   its boolean stack in one 64-bit register
//   k_ctl_fin       Fin(e) = final[dst(e)]
//   k_ctl_bool      NOT / AND / OR / COPY on whole set words
//   k_ctl_mark      EX, first launch: a world in Z stores 1 into some[src] (plain stores of the same value)
//   k_ctl_pre       EX, second launch: pre = some[dst], fused with the & f / | Z of the enclosing fixpoint, the changed word
//                   and, for the witness, the level at which a world joined. It also clears the OTHER some[] for the sweep
//                   after this one: the two buffers alternate, so a sweep is two launches and no memset.
//   k_ctl_dist_init the distances of an EU that keeps them, before its first level
//   k_ctl_walk      the witness: one wavefront, lanes striding over a state's CSR segment, the least full row among the
//                   candidates of the distance wanted, a __shfl_xor butterfly for the least of 64 (walk_least_row of dev_csr.hpp)
//   k_ctl_scatter   the final set to bytes by export index, and the tallies of the initial worlds
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_csr.hpp"
#include "stcsp_engine.h"

namespace stcsp {
namespace dev {

enum { CTL_CHANGED = 0, CTL_INITIAL = 1, CTL_INITIAL_SAT = 2, CTL_DUPLICATE = 3, CTL_STUCK = 4, CTL_WITNESS_LEN = 5, CTL_WORDS = 8 };
enum { CTL_B_NOT = 0, CTL_B_AND = 1, CTL_B_OR = 2, CTL_B_COPY = 3 };
constexpr uint32_t kCtlNone = 0xffffffffu;  // dist[]: not in the set

__device__ inline bool ctl_compare(int32_t op, int32_t x, int32_t y) {
    return op == STCSP_CTL_OP_EQ ? x == y : op == STCSP_CTL_OP_NE ? x != y : op == STCSP_CTL_OP_LT ? x < y : op == STCSP_CTL_OP_LE ? x <= y
         : op == STCSP_CTL_OP_GT ? x > y : x >= y;
}
__device__ inline bool ctl_bit(const unsigned long long *set, uint32_t k) { return (set[k >> 6] >> (k & 63)) & 1ull; }

// out = the worlds whose full row satisfies prog[0 .. len): the stack is the bits of `st`, the top in bit 0 (depth <= 64: the host checks)
__global__ void k_ctl_pred(uint32_t W, int N, const uint32_t *ceid, const int32_t *val, const int32_t *prog, int len, unsigned long long *out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t *row = val + (size_t)(k < W ? ceid[k] : 0u) * N;
    unsigned long long st = 0;
    if (k < W)
        for (int i = 0; i < len; i++) {
            const int32_t t = prog[i];
            if (t == STCSP_CTL_TRUE || t == STCSP_CTL_FALSE) {
                st = (st << 1) | (t == STCSP_CTL_TRUE ? 1ull : 0ull);
            } else if (t == STCSP_CTL_CMP_CONST || t == STCSP_CTL_CMP_VAR) {
                const int32_t x = row[prog[i + 1]], y = t == STCSP_CTL_CMP_CONST ? prog[i + 3] : row[prog[i + 3]];
                st = (st << 1) | (ctl_compare(prog[i + 2], x, y) ? 1ull : 0ull);
                i += 3;
            } else if (t == STCSP_CTL_NOT) {
                st ^= 1ull;
            } else {  // AND, OR
                const unsigned long long a = st & 1ull;
                st >>= 1;
                st = t == STCSP_CTL_AND ? (st & (~1ull | a)) : (st | a);
            }
        }
    const unsigned long long word = __ballot(k < W && (st & 1ull));
    if ((threadIdx.x & 63) == 0 && (k >> 6) < ((W + 63) >> 6)) out[k >> 6] = word;
}

__global__ void k_ctl_fin(uint32_t W, const uint32_t *cdst, const uint8_t *fin, unsigned long long *out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long word = __ballot(k < W && fin[cdst[k < W ? k : 0u]]);
    if ((threadIdx.x & 63) == 0 && (k >> 6) < ((W + 63) >> 6)) out[k >> 6] = word;
}

// one lane per set word; the bits past W stay 0 under NOT
__global__ void k_ctl_bool(uint32_t W, int op, const unsigned long long *a, const unsigned long long *b, unsigned long long *out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, words = (W + 63) >> 6;
    if (j >= words) return;
    const unsigned long long tail = (j == words - 1 && (W & 63)) ? (1ull << (W & 63)) - 1 : ~0ull;
    out[j] = op == CTL_B_NOT ? ~a[j] & tail : op == CTL_B_AND ? a[j] & b[j] : op == CTL_B_OR ? a[j] | b[j] : a[j];
}

// dist[] before the first level of an EU that keeps its distances: 0 on sat(g), kCtlNone elsewhere
__global__ void k_ctl_dist_init(uint32_t W, const unsigned long long *z, uint32_t *dist) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < W) dist[k] = ctl_bit(z, k) ? 0u : kCtlNone;
}

// some[] is all 0 before the launch: the k_ctl_pre two launches back cleared it
__global__ void k_ctl_mark(uint32_t W, const uint32_t *csrc, const unsigned long long *z, uint8_t *some) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < W && ctl_bit(z, k)) some[csrc[k]] = 1;
}

// z = (f ? f & pre : pre) | (or_old ? z : 0) with pre(k) = some[dst(k)]; ctl[CTL_CHANGED] when a word of z changes; dist (may be
// null): a world that joins z gets `level`. clear: the some[] of the next sweep (every state a world leaves).
__global__ void k_ctl_pre(uint32_t W, const uint32_t *csrc, const uint32_t *cdst, const uint8_t *some, uint8_t *clear, const unsigned long long *f,
                          int or_old, unsigned long long *z, uint32_t *dist, uint32_t level, uint32_t *ctl) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x, j = k >> 6, words = (W + 63) >> 6;
    const bool in = k < W;
    bool old = false, now = false;
    if (in) {
        clear[csrc[k]] = 0;
        old = ctl_bit(z, k);
        now = some[cdst[k]] && (!f || ctl_bit(f, k));
        now = now || (or_old && old);
        if (dist && now && !old) dist[k] = level;
    }
    const unsigned long long word = __ballot(now), before = __ballot(old);
    if ((threadIdx.x & 63) == 0 && j < words && word != before) {
        z[j] = word;
        ctl[CTL_CHANGED] = 1u;
    }
}

// The witness walk, one wavefront. With dist (EU): the candidates of a step with `rem` worlds to go are the worlds of the
// segment with dist == rem - 1; len = 1 + the least dist among the initial worlds (found here). Without (EX): set_a at
// rem == 2 and set_b at rem == 1; len = 2 when an initial world is in set_a. Writes the export edges to out_eid[0 .. len)
// and len to ctl[CTL_WITNESS_LEN] (0: no initial world qualifies). max_len bounds every loop.
__global__ void __launch_bounds__(64) k_ctl_walk(uint32_t W, int N, uint32_t max_len, const uint32_t *off, const uint32_t *cdst, const uint32_t *ceid, const uint32_t *dist,
                                               const unsigned long long *set_a, const unsigned long long *set_b, const int32_t *val, uint32_t *out_eid,
                                               uint32_t *ctl) {
    const int lane = threadIdx.x;
    uint32_t len = kCtlNone;
    for (uint32_t k = off[0] + lane; k < off[1]; k += 64) {
        if (dist ? dist[k] != kCtlNone : ctl_bit(set_a, k)) len = min(len, dist ? dist[k] + 1 : 2u);
    }
    for (int step = 32; step > 0; step >>= 1) len = min(len, (uint32_t)__shfl_xor((int)len, step));
    if (len == kCtlNone || len > max_len) {
        if (lane == 0) ctl[CTL_WITNESS_LEN] = 0u;
        return;
    }
    uint32_t s = 0;
    for (uint32_t rem = len; rem > 0; rem--) {
        bool dup = false;
        const uint32_t best = walk_least_row(off, s, lane, ceid, val, N, [&](uint32_t k) {  // the worlds of the distance, or the set, wanted
            return dist ? dist[k] == rem - 1 : ctl_bit(rem == 2 ? set_a : set_b, k);
        }, &dup);
        if (dup) {
            if (lane == 0) ctl[CTL_DUPLICATE] = 1u + s;
            return;
        }
        if (best == kRowNone || best >= W) {  // (cannot happen: a world of distance d > 0 has a successor of distance d - 1)
            if (lane == 0) ctl[CTL_STUCK] = 1u + s;
            return;
        }
        if (lane == 0) out_eid[len - rem] = ceid[best];
        s = cdst[best];
    }
    if (lane == 0) ctl[CTL_WITNESS_LEN] = len;
}

// edge_world / edge_sat are zeroed before the launch
__global__ void k_ctl_scatter(uint32_t W, const uint32_t *csrc, const uint32_t *ceid, const unsigned long long *z, uint8_t *edge_world, uint8_t *edge_sat,
                              uint32_t *ctl) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = k < W, sat = in && ctl_bit(z, k), initial = in && csrc[k] == 0u;
    if (in) {
        edge_world[ceid[k]] = 1;
        edge_sat[ceid[k]] = sat;
    }
    s_tally(initial, &ctl[CTL_INITIAL]);
    s_tally(initial && sat, &ctl[CTL_INITIAL_SAT]);
}

}  // namespace dev
}  // namespace stcsp
