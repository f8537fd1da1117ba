// dev_monitor.hpp -- checking observed streams against the live automaton, on the device.
//
// There is no reference counterpart. Contract: stcsp_engine.h, stcsp_engine_monitor_check. The pass runs where
// dev_quotient.hpp runs, over the same structure-of-arrays edge list and the flags postprocess() left in HBM, and takes
// its two patterns from there: exact ids for the projected labels by lookup-or-insert with a full-key compare, and the
// edge as the unit of parallelism. What it adds is a per-state transition look-up.
//
// Build, once per mask:
//   k_q_reach    (dev_quotient.hpp) the live states.
//   k_m_build    one lane per edge. Dead edges and edges of non-live states are left out. The projected label gets its id
//                as in k_q_labels (the index of the first edge that carried it; the table is KEPT). Then the pair
//                (source, label id) is looked up or inserted in a second table with a full-key compare (one 64-bit CAS),
//                and the edge is pushed on the chain the slot heads: next[e] = atomicExch(&head[slot], e). No sort, no scan.
//   k_m_finish   one lane per slot: drops from the chain the edges whose destination an earlier entry already has (two
//                edges that differ only in hidden variables), leaves the first destination beside the key (dst0), and
//                reports the largest number of distinct destinations of a pair: 1 = deterministic under this mask.
// Check:
//   k_m_steps    one lane per step: the row of n_obs values -> label id, or kQEmpty where no live edge carries the row.
//                A pure stream of 4 * n_obs bytes read and 4 bytes written per step.
//   k_m_walk_det one lane per stream, `len` dependent look-ups (key probe, then dst0): the throughput path, taken while no
//                pair has two destinations (always so with every variable observable).
//   k_m_walk_sets one wavefront per stream. The current and the next state set are open-addressing sets in LDS
//                (kMonSetSlots words each); a lane takes the states of its slots and walks their chains; inserting into
//                the next set de-duplicates. A set may hold kMonSetCap states. A stream that outgrows it is marked
//                (accepted_len = -1) and finished by the host twin: never an approximate answer.
//
// Tables: EMPTY = all ones, linear probing, capacity a power of two of at least twice the number of edges.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_quotient.hpp"

namespace stcsp {
namespace dev {

constexpr unsigned long long kMEmptyKey = ~0ull;
constexpr int kMonSetCap = 256;    // states a stream's set may hold on the device
constexpr int kMonSetSlots = 512;  // LDS words per set (load factor <= 1/2)
// the words the host reads; M_ERROR sits where the quotient's tables expect it (word 3 is free)
enum { M_LABELS = 0, M_PAIRS = 1, M_ERROR = Q_ERROR, M_MAXDST = 4, M_EDGES = 5, M_OVERFLOW = 6, M_WORDS = 8 };

__device__ inline unsigned long long m_row_hash(const int32_t *row, int n_obs) {
    unsigned long long h = 0x9e3779b97f4a7c15ull;
    for (int i = 0; i < n_obs; i++) h = q_mix(h ^ (uint32_t)row[i]);
    return h;
}

__device__ inline uint32_t m_wave_sum(uint32_t x) {
    for (int d = 32; d; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

// slot of the pair (s, l), or kQEmpty
__device__ inline uint32_t m_find(const unsigned long long *keys, uint32_t mask, uint32_t s, uint32_t l) {
    const unsigned long long key = ((unsigned long long)s << 32) | l;
    uint32_t slot = (uint32_t)q_mix(key) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
        const unsigned long long k = keys[slot];
        if (k == key) return slot;
        if (k == kMEmptyKey) break;
    }
    return kQEmpty;
}

// obs[0 .. n_obs) are the observable variables in increasing order.
__global__ void k_m_build(uint32_t E, const long long *src, const long long *dst, const int32_t *values, int N, const int32_t *obs,
                          int n_obs, const uint8_t *alive, const uint8_t *live, uint32_t *ltab, unsigned long long *keys, uint32_t *head,
                          uint32_t mask, uint32_t *dst32, uint32_t *next, uint32_t *ctl) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const uint32_t u = (uint32_t)src[e], v = (uint32_t)dst[e];
    dst32[e] = v;
    next[e] = kQEmpty;
    if (!alive[e] || !live[u] || !live[v]) return;
    const int32_t *row = values + (size_t)e * N;
    unsigned long long h = 0x9e3779b97f4a7c15ull;
    for (int i = 0; i < n_obs; i++) h = q_mix(h ^ (uint32_t)row[obs[i]]);
    uint32_t slot = (uint32_t)h & mask, l = kQEmpty;
    for (uint32_t probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
        uint32_t o = atomicCAS(&ltab[slot], kQEmpty, e);
        if (o == kQEmpty) {
            atomicAdd(&ctl[M_LABELS], 1u);
            o = e;
        }
        if (o != e) {
            const int32_t *other = values + (size_t)o * N;
            bool same = true;
            for (int i = 0; i < n_obs && same; i++) same = row[obs[i]] == other[obs[i]];
            if (!same) continue;
        }
        l = o;
        break;
    }
    if (l == kQEmpty) {
        atomicOr(&ctl[M_ERROR], (uint32_t)Q_ERR_TABLE_FULL);
        return;
    }
    const unsigned long long key = ((unsigned long long)u << 32) | l;
    slot = (uint32_t)q_mix(key) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
        const unsigned long long o = atomicCAS(&keys[slot], kMEmptyKey, key);
        if (o == kMEmptyKey || o == key) {
            next[e] = atomicExch(&head[slot], e);
            return;
        }
    }
    atomicOr(&ctl[M_ERROR], (uint32_t)Q_ERR_TABLE_FULL);
}

// One lane per slot, which owns its chain: plain stores.
__global__ void k_m_finish(uint32_t cap, const unsigned long long *keys, const uint32_t *head, uint32_t *next, const uint32_t *dst32,
                           uint32_t *dst0, uint32_t *ctl) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t edges = 0, distinct = 0;
    if (slot < cap && keys[slot] != kMEmptyKey) {
        const uint32_t h = head[slot];
        dst0[slot] = dst32[h];
        uint32_t prev = kQEmpty;
        for (uint32_t e = h; e != kQEmpty;) {
            const uint32_t d = dst32[e], n = next[e];
            bool dup = false;
            for (uint32_t f = h; f != e && !dup; f = next[f]) dup = dst32[f] == d;
            if (dup) {
                next[prev] = n;  // (the head is never a duplicate: prev is an edge here)
            } else {
                prev = e;
                distinct++;
            }
            edges++;
            e = n;
        }
        if (distinct > 1) atomicMax(&ctl[M_MAXDST], distinct);  // (the host takes 1 where there is a pair at all)
    }
    const uint32_t pairs = m_wave_sum(distinct ? 1u : 0u), all = m_wave_sum(edges);
    if ((threadIdx.x & 63) == 0 && all) {
        atomicAdd(&ctl[M_PAIRS], pairs);
        atomicAdd(&ctl[M_EDGES], all);
    }
}

__global__ void k_m_steps(uint32_t n_steps, const int32_t *rows, int n_obs, const int32_t *values, int N, const int32_t *obs,
                          const uint32_t *ltab, uint32_t mask, uint32_t *step_lid) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_steps) return;
    const int32_t *row = rows + (size_t)t * n_obs;
    uint32_t slot = (uint32_t)m_row_hash(row, n_obs) & mask, l = kQEmpty;
    for (uint32_t probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
        const uint32_t o = ltab[slot];
        if (o == kQEmpty) break;
        const int32_t *other = values + (size_t)o * N;
        bool same = true;
        for (int i = 0; i < n_obs && same; i++) same = row[i] == other[obs[i]];
        if (same) {
            l = o;
            break;
        }
    }
    step_lid[t] = l;
}

// The root is live (the host answers the other case itself).
__global__ void k_m_walk_det(uint32_t n_streams, const long long *offsets, const uint32_t *step_lid, const unsigned long long *keys,
                             const uint32_t *dst0, uint32_t mask, const uint8_t *fin, int32_t *accepted, int32_t *n_end, uint8_t *end_final) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_streams) return;
    const long long off = offsets[i];
    const uint32_t len = (uint32_t)(offsets[i + 1] - off);
    uint32_t s = 0, t = 0;
    for (; t < len; t++) {
        const uint32_t l = step_lid[off + t];
        if (l == kQEmpty) break;
        const uint32_t slot = m_find(keys, mask, s, l);
        if (slot == kQEmpty) break;
        s = dst0[slot];
    }
    accepted[i] = (int32_t)t;
    n_end[i] = 1;
    end_final[i] = fin[s] ? 1 : 0;
}

__device__ inline uint32_t m_set_hash(uint32_t s) { return (s * 0x9e3779b1u) >> 16; }

// One wavefront (= one block of 64 lanes) per stream; the root is live.
__global__ __launch_bounds__(64) void k_m_walk_sets(uint32_t n_streams, const long long *offsets, const uint32_t *step_lid,
                                                    const unsigned long long *keys, const uint32_t *head, const uint32_t *next,
                                                    const uint32_t *dst32, uint32_t mask, const uint8_t *fin, int32_t *accepted,
                                                    int32_t *n_end, uint8_t *end_final, uint32_t *ctl) {
    __shared__ uint32_t set[2][kMonSetSlots];
    __shared__ uint32_t count, overflow;
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n_streams) return;
    const long long off = offsets[i];
    const uint32_t len = (uint32_t)(offsets[i + 1] - off);
    for (int k = lane; k < kMonSetSlots; k += 64) set[0][k] = kQEmpty;
    if (lane == 0) overflow = 0u;
    __syncthreads();
    if (lane == 0) set[0][m_set_hash(0u) & (kMonSetSlots - 1)] = 0u;
    __syncthreads();
    int cur = 0;
    uint32_t n = 1, t = 0;
    for (; t < len; t++) {
        const uint32_t l = step_lid[off + t];
        if (l == kQEmpty) break;
        uint32_t *nxt = set[1 - cur];
        for (int k = lane; k < kMonSetSlots; k += 64) nxt[k] = kQEmpty;
        if (lane == 0) count = 0u;
        __syncthreads();
        for (int k = lane; k < kMonSetSlots; k += 64) {
            const uint32_t s = set[cur][k];
            if (s == kQEmpty) continue;
            const uint32_t slot = m_find(keys, mask, s, l);
            if (slot == kQEmpty) continue;
            for (uint32_t e = head[slot]; e != kQEmpty; e = next[e]) {
                const uint32_t d = dst32[e];
                uint32_t h = m_set_hash(d) & (kMonSetSlots - 1);
                int probe = 0;
                for (; probe < kMonSetSlots; probe++, h = (h + 1) & (kMonSetSlots - 1)) {
                    const uint32_t o = atomicCAS(&nxt[h], kQEmpty, d);
                    if (o == kQEmpty) atomicAdd(&count, 1u);
                    if (o == kQEmpty || o == d) break;
                }
                if (probe == kMonSetSlots) overflow = 1u;
            }
        }
        __syncthreads();
        const uint32_t c = count, full = overflow;
        __syncthreads();  // (lane 0 resets `count` at the top of the next step)
        if (full || c > (uint32_t)kMonSetCap) {
            if (lane == 0) {
                accepted[i] = -1;  // the host twin finishes this stream
                n_end[i] = 0;
                end_final[i] = 0;
                atomicAdd(&ctl[M_OVERFLOW], 1u);
            }
            return;
        }
        if (c == 0) break;
        cur = 1 - cur;
        n = c;
    }
    int f = 0;
    for (int k = lane; k < kMonSetSlots; k += 64) {
        const uint32_t s = set[cur][k];
        if (s != kQEmpty && fin[s]) f = 1;
    }
    f = __syncthreads_or(f);
    if (lane == 0) {
        accepted[i] = (int32_t)t;
        n_end[i] = (int32_t)n;
        end_final[i] = f ? 1 : 0;
    }
}

}  // namespace dev
}  // namespace stcsp
