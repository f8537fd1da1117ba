// dev_observer.hpp -- the observer (subset construction) of the live automaton under a mask, on the device.
//
// There is no reference counterpart. Contract: stcsp_engine.h, stcsp_engine_observer. The pass runs over the CSR of the last
// generator_build() (dev_generate.hpp: off / dstp, live states only) and the dense label ids of repair_labels() (dev_repair.hpp).
// An observer state is a set of automaton states, kept as an ascending list of state indices in one pool; a record names its
// list, and a table keyed by a 64-bit hash of the set names its record. Nothing waits for anything inside a launch: what one
// workgroup writes is read by another only in a later launch, so the launch boundaries are the only visibility the pass needs.
//
// Build, once per generator_build():
//   k_o_order     one wavefront per state: its out-edges as keys (label rank << 32 | destination), ranked by counting the keys
//                 of the segment that come before (the way of k_g_order), written in that order. The label rank is the
//                 lexicographic rank of the projected row (the host sorts the n_labels rows), so label order is row order and
//                 one member finds the run of a label by binary search. Duplicate keys stay: a bitset swallows them.
// Per level (a frontier of observer states, cut into chunks when the items would not fit the budget):
//   k_o_items     one workgroup per frontier set, lanes over its members: every first key of a run of one label claims the
//                 pair (set, label) with one 64-bit CAS; the winner appends the work item.
//   k_o_succ<INTERN>  one workgroup per item: the members' runs of the label OR their destinations into a bitset over the
//                 states (LDS up to kObsLdsWords words, else a slice of global scratch per workgroup); the touched word range
//                 is scanned for the size, a 64-bit hash and the final flag, and cleared. Lane 0 looks the hash up with one
//                 CAS per probed slot; the winner takes the next state number and reserves its room in the pool.
//                 The host reads the counters here: both limits are checked before a list is written.
//   k_o_succ<WRITE>   the winners build their bitset again and write the ascending member list into the room they reserved.
//   k_o_succ<VERIFY>  every item logs its edge (source set, label rank, destination set); every other item builds its bitset
//                 again and compares it, member by member, with the list of the record its hash found: a difference is a
//                 collision of the hash and sets the error word.
// Numbering, after the last level:
//   k_o_keys      per level, one lane per edge logged there: key of a state new at that level = min (canonical number of the
//                 source << 32 | label rank). The host sorts the keys of the level.
//   k_o_renumber  one lane per edge: state numbers -> canonical numbers.
//   k_o_gather    one workgroup per state: its member list to its place in canonical order.
//
// Every loop is bounded by a launch parameter or by a size a launch parameter bounds (a record's n <= S, a segment's length,
// 32 bits of a word, the slots of a table). A full table sets the error word and the lane returns.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_generate.hpp"

namespace stcsp {
namespace dev {

constexpr unsigned long long kObsEmpty = ~0ull;  // free slot of both tables
constexpr uint32_t kObsLdsWords = 8192;          // a bitset of up to 32 * 8192 states lives in LDS (32 KiB)
constexpr uint32_t kObsWin = 0x80000000u;        // item_slot: this item inserted the slot (tables have at most 2^31 slots)
// the words the host reads; O_POOL is one 64-bit counter (two words, 8-byte aligned)
enum { O_ITEMS = 0, O_STATES = 1, O_ERROR = 2, O_MAXDEG = 3, O_POOL = 4, O_WORDS = 8 };
enum { O_ERR_TABLE_FULL = 1, O_ERR_COLLISION = 2, O_ERR_ITEMS_FULL = 4 };
enum { O_INTERN = 0, O_WRITE = 1, O_VERIFY = 2 };

struct ObsRec {
    unsigned long long off;  // first member in the pool
    uint32_t n;              // members
    uint32_t fin;            // some member is final
};

__device__ inline unsigned long long o_member_hash(uint32_t s) { return q_mix((unsigned long long)s ^ 0x243f6a8885a308d3ull); }
// the hash of a set from the sum of its members' hashes and its size; never kObsEmpty
__device__ inline unsigned long long o_set_hash(unsigned long long sum, uint32_t n) {
    const unsigned long long h = q_mix2(sum + (unsigned long long)n * 0x9e3779b97f4a7c15ull);
    return h == kObsEmpty ? 0ull : h;
}

// okey has off[S] entries; lrank[label id] = rank of the label's projected row
__global__ __launch_bounds__(256) void k_o_order(uint32_t S, const uint32_t *off, const uint32_t *lid, const uint32_t *dstp, const uint32_t *lrank,
                                                 unsigned long long *okey, uint32_t *ctl) {
    const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= S) return;
    const uint32_t b = off[s], d = off[s + 1] - b;
    if (lane == 0 && d) atomicMax(&ctl[O_MAXDEG], d);
    for (uint32_t i = lane; i < d; i += 64) {
        const unsigned long long ki = ((unsigned long long)lrank[lid[b + i]] << 32) | dstp[b + i];
        uint32_t r = 0;
        for (uint32_t j = 0; j < d; j++) {
            const unsigned long long kj = ((unsigned long long)lrank[lid[b + j]] << 32) | dstp[b + j];
            r += (kj < ki || (kj == ki && j < i)) ? 1u : 0u;
        }
        okey[b + r] = ki;
    }
}

// the root's set {0}: state 0, one member
__global__ void k_o_init(const uint8_t *fin, ObsRec *rec, uint32_t *pool, unsigned long long *stab, uint32_t *ssid, uint32_t smask, uint32_t *ctl) {
    if (blockIdx.x || threadIdx.x) return;
    const unsigned long long h = o_set_hash(o_member_hash(0), 1);
    const uint32_t slot = (uint32_t)h & smask;
    stab[slot] = h;
    ssid[slot] = 0;
    pool[0] = 0;
    rec[0] = ObsRec{0ull, 1u, fin[0]};
    ctl[O_STATES] = 1;
    *(unsigned long long *)(ctl + O_POOL) = 1ull;
}

// the state table into a larger one; a hash is in the old table once
__global__ void k_o_rehash(uint32_t old_slots, const unsigned long long *old_tab, const uint32_t *old_sid, unsigned long long *stab, uint32_t *ssid,
                           uint32_t smask, uint32_t *ctl) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= old_slots) return;
    const unsigned long long h = old_tab[i];
    if (h == kObsEmpty) return;
    uint32_t slot = (uint32_t)h & smask;
    for (uint32_t probe = 0; probe <= smask; probe++, slot = (slot + 1) & smask)
        if (atomicCAS(&stab[slot], kObsEmpty, h) == kObsEmpty) {
            ssid[slot] = old_sid[i];
            return;
        }
    atomicOr(&ctl[O_ERROR], (uint32_t)O_ERR_TABLE_FULL);
}

// frontier sets [c0, c1); items[i] = (set - c0) << 32 | label rank
__global__ __launch_bounds__(256) void k_o_items(uint32_t c0, uint32_t c1, const ObsRec *rec, const uint32_t *pool, const uint32_t *off,
                                                 const unsigned long long *okey, unsigned long long *itab, uint32_t imask, unsigned long long *items,
                                                 uint32_t cap_items, uint32_t *ctl) {
    for (uint32_t f = c0 + blockIdx.x; f < c1; f += gridDim.x) {
        const ObsRec r = rec[f];
        for (uint32_t m = threadIdx.x; m < r.n; m += 256) {
            const uint32_t s = pool[r.off + m];
            uint32_t prev = 0xffffffffu;
            for (uint32_t k = off[s]; k < off[s + 1]; k++) {
                const uint32_t l = (uint32_t)(okey[k] >> 32);
                if (l == prev) continue;
                prev = l;
                const unsigned long long key = ((unsigned long long)(f - c0) << 32) | l;
                uint32_t slot = (uint32_t)q_mix(key) & imask, probe = 0;
                for (; probe <= imask; probe++, slot = (slot + 1) & imask) {
                    const unsigned long long o = atomicCAS(&itab[slot], kObsEmpty, key);
                    if (o == kObsEmpty) {
                        const uint32_t at = atomicAdd(&ctl[O_ITEMS], 1u);
                        if (at < cap_items)
                            items[at] = key;
                        else
                            atomicOr(&ctl[O_ERROR], (uint32_t)O_ERR_ITEMS_FULL);
                        break;
                    }
                    if (o == key) break;
                }
                if (probe > imask) atomicOr(&ctl[O_ERROR], (uint32_t)O_ERR_TABLE_FULL);
            }
        }
    }
}

// The bitset of one workgroup. In global scratch every access goes to L2 (atomics, agent-scope loads and stores): the words an
// atomic changed are not in this CU's L1.
template <bool kGlobal>
__device__ inline void o_bit_set(uint32_t *bits, uint32_t s) { atomicOr(&bits[s >> 5], 1u << (s & 31)); }
template <bool kGlobal>
__device__ inline uint32_t o_word(uint32_t *bits, uint32_t i) {
    return kGlobal ? __hip_atomic_load(&bits[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : bits[i];
}
template <bool kGlobal>
__device__ inline void o_clear(uint32_t *bits, uint32_t i) {
    if (kGlobal)
        __hip_atomic_store(&bits[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        bits[i] = 0u;
}

// delta(set r, label l) into bits (all zero before); range[0..1] = the touched words (0xffffffff, 0 when there is none)
template <bool kGlobal>
__device__ inline void o_expand(uint32_t *bits, const ObsRec r, uint32_t l, const uint32_t *pool, const uint32_t *off, const unsigned long long *okey,
                                uint32_t *range) {
    if (threadIdx.x == 0) {
        range[0] = 0xffffffffu;
        range[1] = 0u;
    }
    __syncthreads();
    uint32_t lo = 0xffffffffu, hi = 0u;
    const unsigned long long want = (unsigned long long)l << 32;
    for (uint32_t m = threadIdx.x; m < r.n; m += 256) {
        const uint32_t s = pool[r.off + m], end = off[s + 1];
        uint32_t a = off[s], b = end;
        while (a < b) {  // the first key of the segment that is not below the label's run
            const uint32_t mid = a + (b - a) / 2;
            if (okey[mid] < want)
                a = mid + 1;
            else
                b = mid;
        }
        for (uint32_t k = a; k < end; k++) {
            const unsigned long long key = okey[k];
            if ((uint32_t)(key >> 32) != l) break;
            const uint32_t d = (uint32_t)key;
            o_bit_set<kGlobal>(bits, d);
            lo = min(lo, d >> 5);
            hi = max(hi, d >> 5);
        }
    }
    if (lo <= hi) {
        atomicMin(&range[0], lo);
        atomicMax(&range[1], hi);
    }
    __syncthreads();
}

// items [0, n_items) of the chunk that starts at frontier set c0; W = bitset words, scratch = gridDim.x slices of W words (kGlobal).
// INTERN writes rec / ssid / item_slot; WRITE writes the pool; VERIFY writes the edge log at e_base + item.
template <bool kGlobal, int kMode>
__global__ __launch_bounds__(256) void k_o_succ(uint32_t n_items, uint32_t c0, const unsigned long long *items, ObsRec *rec, uint32_t *pool,
                                                const uint32_t *off, const unsigned long long *okey, const uint8_t *fin, uint32_t W, uint32_t *scratch,
                                                unsigned long long *stab, uint32_t *ssid, uint32_t smask, uint32_t *item_slot, uint32_t e_base,
                                                uint32_t *esrc, uint32_t *elab, uint32_t *edst, uint32_t *ctl) {
    __shared__ uint32_t lds[kGlobal ? 1 : kObsLdsWords];
    __shared__ uint32_t range[2], tmp[4], red_f[4];
    __shared__ unsigned long long red_h[4];
    uint32_t *bits = kGlobal ? scratch + (size_t)blockIdx.x * W : lds;
    for (uint32_t i = threadIdx.x; i < W; i += 256) o_clear<kGlobal>(bits, i);
    __syncthreads();
    for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const unsigned long long item = items[it];
        const uint32_t f = c0 + (uint32_t)(item >> 32), l = (uint32_t)item;
        ObsRec t{0ull, 0u, 0u};  // the record the item's hash found
        if (kMode != O_INTERN) {
            const uint32_t sw = item_slot[it];  // (the same in every lane: the branches below are taken by the whole workgroup)
            const uint32_t sid = ssid[sw & ~kObsWin];
            if (kMode == O_WRITE && !(sw & kObsWin)) continue;
            if (kMode == O_VERIFY) {
                if (threadIdx.x == 0) {
                    esrc[e_base + it] = f;
                    elab[e_base + it] = l;
                    edst[e_base + it] = sid;
                }
                if (sw & kObsWin) continue;
            }
            t = rec[sid];
        }
        o_expand<kGlobal>(bits, rec[f], l, pool, off, okey, range);
        const uint32_t lo = range[0], hi = range[1];
        uint32_t count = 0, any_fin = 0, bad = 0;
        unsigned long long sum = 0;
        if (lo != 0xffffffffu)
            for (uint32_t base = lo; base <= hi; base += 256) {
                const uint32_t wi = base + threadIdx.x;
                uint32_t w = wi <= hi ? o_word<kGlobal>(bits, wi) : 0u, total;
                uint32_t at = count + g_block_scan((uint32_t)__popc(w), tmp, &total);
                if (w) o_clear<kGlobal>(bits, wi);
                while (w) {
                    const uint32_t s = wi * 32 + (uint32_t)(__ffs(w) - 1);
                    w &= w - 1;
                    if (kMode == O_INTERN) {
                        sum += o_member_hash(s);
                        any_fin |= fin[s];
                    }
                    if (kMode == O_WRITE) pool[t.off + at] = s;  // (at < t.n: the same bitset gave t.n)
                    if (kMode == O_VERIFY) bad |= (at >= t.n || pool[t.off + at] != s) ? 1u : 0u;
                    at++;
                }
                count += total;
            }
        if (kMode == O_VERIFY && (bad || count != t.n)) atomicOr(&ctl[O_ERROR], (uint32_t)O_ERR_COLLISION);
        if (kMode == O_INTERN) {
            for (int d = 32; d; d >>= 1) {
                sum += __shfl_down(sum, d);
                any_fin |= __shfl_down(any_fin, d);
            }
            if ((threadIdx.x & 63) == 0) {
                red_h[threadIdx.x >> 6] = sum;
                red_f[threadIdx.x >> 6] = any_fin;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                const unsigned long long h = o_set_hash(red_h[0] + red_h[1] + red_h[2] + red_h[3], count);
                const uint32_t final_flag = (red_f[0] | red_f[1] | red_f[2] | red_f[3]) ? 1u : 0u;
                uint32_t slot = (uint32_t)h & smask, probe = 0, found = 0;
                for (; probe <= smask; probe++, slot = (slot + 1) & smask) {
                    const unsigned long long o = atomicCAS(&stab[slot], kObsEmpty, h);
                    if (o == kObsEmpty) {  // a new state: its number, its room in the pool (written by the WRITE launch)
                        const uint32_t sid = atomicAdd(&ctl[O_STATES], 1u);
                        const unsigned long long at = atomicAdd((unsigned long long *)(ctl + O_POOL), (unsigned long long)count);
                        rec[sid] = ObsRec{at, count, final_flag};
                        ssid[slot] = sid;
                        found = slot | kObsWin;
                        break;
                    }
                    if (o == h) {
                        found = slot;
                        break;
                    }
                }
                if (probe > smask) atomicOr(&ctl[O_ERROR], (uint32_t)O_ERR_TABLE_FULL);
                item_slot[it] = found;
            }
        }
    }
}

// edges [e0, e1) were logged while the states from s0 on were new: their keys
__global__ void k_o_keys(uint32_t e0, uint32_t e1, const uint32_t *esrc, const uint32_t *elab, const uint32_t *edst, uint32_t s0, const uint32_t *canon,
                         unsigned long long *keys) {
    const uint32_t e = e0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= e1) return;
    const uint32_t d = edst[e];
    if (d >= s0) atomicMin(&keys[d], ((unsigned long long)canon[esrc[e]] << 32) | elab[e]);
}

__global__ void k_o_renumber(uint32_t E, uint32_t *esrc, uint32_t *edst, const uint32_t *canon) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    esrc[e] = canon[esrc[e]];
    edst[e] = canon[edst[e]];
}

// where[sid] = the first entry of the state's list in `out` (canonical order)
__global__ __launch_bounds__(256) void k_o_gather(uint32_t n_states, const ObsRec *rec, const unsigned long long *where, const uint32_t *pool,
                                                  int32_t *out) {
    for (uint32_t s = blockIdx.x; s < n_states; s += gridDim.x) {
        const ObsRec r = rec[s];
        for (uint32_t m = threadIdx.x; m < r.n; m += 256) out[where[s] + m] = (int32_t)pool[r.off + m];
    }
}

}  // namespace dev
}  // namespace stcsp
