// dev_compare.hpp -- the synchronous product of two deterministic automata on the device: inclusion of their languages and the
// shortest witnesses.
//
// There is no reference counterpart. Contract: stcsp_engine.h, stcsp_engine_compare. Both operands lie in HBM as CSR by source
// (off / lab / dst): lab is the rank of the edge's row among the rows of both operands (the host merges them), ascending
// within a state, so one lane finds the other side's edge of a row by binary search. The sink of an operand is the index
// n: off has n + 2 entries and the sink's segment is empty, fin has n + 1 entries and the sink's is 0. A pair (l, r) is its
// own exact 64-bit key (l << 32 | r): the table needs no verification. Pairs are numbered canonically level by level, so a
// frontier is a range of pair numbers and the record of a pair (key, parent, label) lies at its number.
//
// Once:
//   k_c_init      the root pair into the table, as the one new pair of level 0.
// Per level:
//   k_c_collect   one lane per new pair: its min-key (the least (parent number << 32 | label rank) over the edges that found
//                 it) to where the host reads it, and the out-degrees of its components into the bound of the next level.
//                 The host sorts the keys of the level: the rank of a key is the pair's number within the level.
//   k_c_number    one lane per new pair: key, parent and label to its number; the four predicates, each with a 32-bit
//                 atomicMin on the pair number (after a reduction over the wavefront).
//   k_c_expand<LANES>  LANES lanes per frontier pair (8 or 64; the host chooses by the mean out-degree of the frontier). The
//                 lanes stride over the items of the pair: the edges of l, then the edges of r. An edge of l looks its row up
//                 in r's segment; an edge of r whose row l has too is dropped (the edge of l stands for both). The successor
//                 key is looked up or inserted with one 64-bit CAS per probed slot; the winner appends the slot to the list
//                 of the new pairs; every item lowers the slot's min-key with a 64-bit atomicMin. Edges are counted per
//                 lane, summed over the wavefront and added once.
//   k_c_rehash    the table into a larger one, between levels (every pair is numbered then: the min-keys start afresh).
//
// Nothing waits inside a launch. What a workgroup writes with a plain store (the list of new slots, the records) is read
// in a later launch only; within a launch the table, the min-keys and the counters are touched through atomics alone.
// Every loop is bounded by a launch parameter or by a size one bounds (a segment's length, the slots of the table).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_quotient.hpp"

namespace stcsp {
namespace dev {

constexpr unsigned long long kCmpEmpty = ~0ull;  // free slot, and a min-key no edge has lowered
constexpr uint32_t kCmpNone = 0xffffffffu;
// the words the host reads; C_EDGES and C_DEG are 64-bit counters (two words, 8-byte aligned)
enum { C_NEW = 0, C_ERROR = 1, C_EDGES = 2, C_DEG = 4, C_VERDICT = 6, C_WORDS = 10 };
enum { C_ERR_TABLE_FULL = 1, C_ERR_NEW_FULL = 2 };

struct CmpSide {
    const uint32_t *off, *lab, *dst;  // [n + 2], [off[n]], [off[n]]
    const uint8_t *fin;               // [n + 1]
    uint32_t n;                       // states; the index of the sink
};

__device__ inline uint32_t c_slot(unsigned long long key, uint32_t smask) { return (uint32_t)q_mix(key) & smask; }

// the position of `rank` in lab[a, b) (ascending, distinct), or kCmpNone
__device__ inline uint32_t c_find(const uint32_t *lab, uint32_t a, uint32_t b, uint32_t rank) {
    const uint32_t end = b;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (lab[mid] < rank)
            a = mid + 1;
        else
            b = mid;
    }
    return a < end && lab[a] == rank ? a : kCmpNone;
}

__global__ void k_c_init(unsigned long long root, unsigned long long *tab, unsigned long long *minkey, uint32_t smask, uint32_t *newslot, uint32_t *ctl) {
    if (blockIdx.x || threadIdx.x) return;
    const uint32_t slot = c_slot(root, smask);
    tab[slot] = root;
    minkey[slot] = 0ull;
    newslot[0] = slot;
    ctl[C_NEW] = 1;
}

__global__ void k_c_rehash(uint32_t old_slots, const unsigned long long *old_tab, unsigned long long *tab, uint32_t smask, uint32_t *ctl) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= old_slots) return;
    const unsigned long long key = old_tab[i];
    if (key == kCmpEmpty) return;
    uint32_t slot = c_slot(key, smask);
    for (uint32_t probe = 0; probe <= smask; probe++, slot = (slot + 1) & smask)
        if (atomicCAS(&tab[slot], kCmpEmpty, key) == kCmpEmpty) return;
    atomicOr(&ctl[C_ERROR], (uint32_t)C_ERR_TABLE_FULL);
}

__global__ __launch_bounds__(256) void k_c_collect(uint32_t n_new, const uint32_t *newslot, const unsigned long long *tab, const unsigned long long *minkey,
                                                   const uint32_t *loff, const uint32_t *roff, unsigned long long *keys, uint32_t *ctl) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    unsigned long long deg = 0;
    if (i < n_new) {
        const uint32_t slot = newslot[i];
        const unsigned long long key = tab[slot];
        const uint32_t l = (uint32_t)(key >> 32), r = (uint32_t)key;
        keys[i] = minkey[slot];
        deg = (unsigned long long)(loff[l + 1] - loff[l]) + (roff[r + 1] - roff[r]);
    }
    for (int d = 32; d; d >>= 1) deg += __shfl_down(deg, d);
    if ((threadIdx.x & 63) == 0 && deg) atomicAdd((unsigned long long *)(ctl + C_DEG), deg);
}

// rank[i] = the place of new pair i among the new pairs of the level; its number is base + rank[i]
__global__ __launch_bounds__(256) void k_c_number(uint32_t n_new, uint32_t base, const uint32_t *newslot, const uint32_t *rank, const unsigned long long *tab,
                                                  const unsigned long long *keys, const uint8_t *lfin, const uint8_t *rfin, uint32_t nl, uint32_t nr,
                                                  unsigned long long *pkey, uint32_t *parent, uint32_t *plabel, uint32_t *ctl) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t v[4] = {kCmpNone, kCmpNone, kCmpNone, kCmpNone};
    if (i < n_new) {
        const uint32_t num = base + rank[i];
        const unsigned long long key = tab[newslot[i]], mk = keys[i];
        const uint32_t l = (uint32_t)(key >> 32), r = (uint32_t)key;
        pkey[num] = key;
        parent[num] = (uint32_t)(mk >> 32);
        plabel[num] = (uint32_t)mk;
        const bool fl = lfin[l] != 0, fr = rfin[r] != 0;  // (the sinks are not final)
        if (l != nl && r == nr) v[0] = num;
        if (r != nr && l == nl) v[1] = num;
        if (fl && !fr) v[2] = num;
        if (fr && !fl) v[3] = num;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t m = v[k];
        for (int d = 32; d; d >>= 1) m = min(m, (uint32_t)__shfl_down(m, d));
        if ((threadIdx.x & 63) == 0 && m != kCmpNone) atomicMin(&ctl[C_VERDICT + k], m);
    }
}

// the frontier is the pairs [f0, f1); newslot has room for cap_new slots
template <int kLanes>
__global__ __launch_bounds__(256) void k_c_expand(uint32_t f0, uint32_t f1, const unsigned long long *pkey, CmpSide L, CmpSide R, unsigned long long *tab,
                                                  unsigned long long *minkey, uint32_t smask, uint32_t *newslot, uint32_t cap_new, uint32_t *ctl) {
    constexpr uint32_t kGroups = 256 / kLanes;
    const uint32_t sub = threadIdx.x % kLanes;
    uint32_t edges = 0;
    for (unsigned long long f = (unsigned long long)f0 + blockIdx.x * kGroups + threadIdx.x / kLanes; f < f1; f += (unsigned long long)gridDim.x * kGroups) {
        const unsigned long long key = pkey[f];
        const uint32_t l = (uint32_t)(key >> 32), r = (uint32_t)key;
        const uint32_t la = L.off[l], dl = L.off[l + 1] - la, ra = R.off[r], dr = R.off[r + 1] - ra;
        for (uint32_t i = sub; i < dl + dr; i += kLanes) {
            uint32_t rank, l2, r2;
            if (i < dl) {
                rank = L.lab[la + i];
                l2 = L.dst[la + i];
                const uint32_t j = c_find(R.lab, ra, ra + dr, rank);
                r2 = j == kCmpNone ? R.n : R.dst[j];
            } else {
                const uint32_t j = ra + (i - dl);
                rank = R.lab[j];
                if (c_find(L.lab, la, la + dl, rank) != kCmpNone) continue;  // the edge of l has taken this row
                l2 = L.n;
                r2 = R.dst[j];
            }
            edges++;
            const unsigned long long succ = ((unsigned long long)l2 << 32) | r2;
            uint32_t slot = c_slot(succ, smask), probe = 0;
            bool won = false;
            for (; probe <= smask; probe++, slot = (slot + 1) & smask) {
                const unsigned long long o = atomicCAS(&tab[slot], kCmpEmpty, succ);
                won = o == kCmpEmpty;
                if (won || o == succ) break;
            }
            if (probe > smask) {
                atomicOr(&ctl[C_ERROR], (uint32_t)C_ERR_TABLE_FULL);
                continue;
            }
            if (won) {
                const uint32_t at = atomicAdd(&ctl[C_NEW], 1u);
                if (at < cap_new)
                    newslot[at] = slot;
                else
                    atomicOr(&ctl[C_ERROR], (uint32_t)C_ERR_NEW_FULL);
            }
            atomicMin(&minkey[slot], (f << 32) | rank);
        }
    }
    for (int d = 32; d; d >>= 1) edges += __shfl_down(edges, d);
    if ((threadIdx.x & 63) == 0 && edges) atomicAdd((unsigned long long *)(ctl + C_EDGES), (unsigned long long)edges);
}

}  // namespace dev
}  // namespace stcsp
