// dev_quotient.hpp -- bisimulation quotient of the live automaton, on the device.
//
// There is no reference counterpart: the reference prints the automaton as the search left it, one state per
// (constraint set, signature). This pass folds the states that accept the same language. It runs where
// dev_postproc.hpp ran, over the same structure-of-arrays edge list and the flags the post-search passes left in HBM.
//
// Input: the live automaton = the states that are `valid` and reachable from the root over `alive` edges (what
// write_dot prints), and the alive edges between them. Labels are projected on the observable variables.
// Result: the coarsest partition in which two states share a class only if they have the same `final` flag and their
// live out-edges give the same SET of pairs (projected label, class of the destination): the largest bisimulation. With
// every variable observable the automaton is deterministic and the quotient is its minimal form; under a projecting mask
// the automaton is nondeterministic and the quotient keeps the language but need not be the smallest such automaton.
//
// Design (b) of the two the issue allows -- a commutative 128-bit signature per state, verified exactly at the end:
//   k_q_labels   once: every live edge's projected label gets an exact id by lookup-or-insert with a full-key compare
//                (the id is the index of the first edge that carried the label). The only sweep that reads the 4 N-byte
//                label rows. It also leaves 4-byte copies of src / dst, so a round reads 12 B per edge.
//   one round:   k_q_state_init   acc[s] = f(final[s])                                      (20 B written per state)
//                k_q_edges        acc[src] += mixA / mixB (label id, class[dst])            (12 B read per edge, one 4 B
//                                 gather, two 8 B atomic adds; duplicates of a pair within one state are dropped first by an
//                                 exact set of (src, label id, class[dst]) triples -- only while some state HAS two
//                                 edges with one projected label, which round 1 finds out)
//                k_q_number       class'[s] = first state seen with the same (class[s], acc[s]): lookup-or-insert with a
//                                 full-key compare; the class id is that state's index       (24 B read per state)
//   The host reads the class count between rounds and stops when it no longer grows. A class never merges with another
//   (the old class is part of the key), and sums of equal sets are equal, so bisimilar states are never separated; a
//   128-bit collision could only leave two different states together. That is what the last sweep excludes:
//   k_q_verify_* compare every state with its class representative pair by pair -- every pair of the state is looked up
//   in the representative's exact pair set, and the numbers of distinct pairs must agree. A mismatch is reported to the
//   host, which returns STCSP_E_INTERNAL: never a silently wrong partition.
//
// All tables hold 4-byte indices into arrays that do not change while the kernel that fills the table runs (edge index,
// state index), EMPTY = 0xffffffff, linear probing, capacity a power of two of at least twice the number of keys.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace stcsp {
namespace dev {

constexpr uint32_t kQEmpty = 0xffffffffu;  // free table slot; label id of an edge outside the live automaton
enum { Q_CLASSES = 0, Q_DUPS = 1, Q_ERROR = 2, Q_CHANGED = 3, Q_WORDS = 4 };  // the words the host reads between rounds
enum { Q_ERR_TABLE_FULL = 1, Q_ERR_PAIR = 2, Q_ERR_STATE = 4 };

__device__ inline unsigned long long q_mix(unsigned long long x) {  // splitmix64 finaliser
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
__device__ inline unsigned long long q_mix2(unsigned long long x) {  // murmur3 finaliser: the second, independent mixer
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    return x ^ (x >> 33);
}

// live[s] = reachable from a valid root over alive edges into valid states: flags read live, like k_trav_back.
__global__ void k_q_reach(uint32_t E, const long long *src, const long long *dst, const uint8_t *alive, const uint8_t *valid,
                          uint8_t *live, uint32_t *ctl) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E || !alive[e]) return;
    const long long u = src[e], v = dst[e];
    if (live[u] && valid[v] && !live[v]) {
        live[v] = 1;
        ctl[Q_CHANGED] = 1u;
    }
}

// Label ids. obs[0 .. n_obs) are the observable variables in increasing order.
__global__ void k_q_labels(uint32_t E, const long long *src, const long long *dst, const int32_t *values, int N, const int32_t *obs,
                           int n_obs, const uint8_t *alive, const uint8_t *live, uint32_t *table, uint32_t mask, uint32_t *src32,
                           uint32_t *dst32, uint32_t *lid, uint32_t *ctl) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const uint32_t u = (uint32_t)src[e], v = (uint32_t)dst[e];
    src32[e] = u;
    dst32[e] = v;
    if (!alive[e] || !live[u] || !live[v]) {
        lid[e] = kQEmpty;
        return;
    }
    const int32_t *row = values + (size_t)e * N;
    unsigned long long h = 0x9e3779b97f4a7c15ull;
    for (int i = 0; i < n_obs; i++) h = q_mix(h ^ (uint32_t)row[obs[i]]);
    uint32_t slot = (uint32_t)h & mask;
    for (uint32_t probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
        uint32_t o = atomicCAS(&table[slot], kQEmpty, e);
        if (o == kQEmpty) o = e;
        if (o != e) {
            const int32_t *other = values + (size_t)o * N;
            bool same = true;
            for (int i = 0; i < n_obs && same; i++) same = row[obs[i]] == other[obs[i]];
            if (!same) continue;
        }
        lid[e] = o;
        return;
    }
    lid[e] = kQEmpty;
    atomicOr(&ctl[Q_ERROR], (uint32_t)Q_ERR_TABLE_FULL);
}

__global__ void k_q_state_init(uint32_t S, const uint8_t *fin, unsigned long long *accA, unsigned long long *accB, uint32_t *cnt) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    accA[s] = fin[s] ? 0x6a09e667f3bcc909ull : 0ull;
    accB[s] = fin[s] ? 0xbb67ae8584caa73bull : 0ull;
    cnt[s] = 0u;
}

__device__ inline uint32_t q_triple_hash(uint32_t s, uint32_t l, uint32_t c) {
    return (uint32_t)q_mix((((unsigned long long)s << 32) | l) ^ ((unsigned long long)c * 0x9e3779b97f4a7c15ull));
}

// One refinement sweep over the edges. dedup: drop the second and later edges of one state that carry the same
// (label id, class of destination) -- the sum below must count a pair once. cnt[s] = distinct pairs (with dedup).
__global__ void k_q_edges(uint32_t E, const uint32_t *src32, const uint32_t *dst32, const uint32_t *lid, const uint32_t *cls, int dedup,
                          uint32_t *table, uint32_t mask, unsigned long long *accA, unsigned long long *accB, uint32_t *cnt,
                          uint32_t *ctl) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const uint32_t l = lid[e];
    if (l == kQEmpty) return;
    const uint32_t s = src32[e], c = cls[dst32[e]];
    if (dedup) {
        uint32_t slot = q_triple_hash(s, l, c) & mask;
        uint32_t probe = 0;
        for (; probe <= mask; probe++, slot = (slot + 1) & mask) {
            const uint32_t o = atomicCAS(&table[slot], kQEmpty, e);
            if (o == kQEmpty) break;  // first edge with this triple
            if (src32[o] == s && lid[o] == l && cls[dst32[o]] == c) {
                atomicAdd(&ctl[Q_DUPS], 1u);
                return;
            }
        }
        if (probe > mask) {
            atomicOr(&ctl[Q_ERROR], (uint32_t)Q_ERR_TABLE_FULL);
            return;
        }
        atomicAdd(&cnt[s], 1u);
    }
    const unsigned long long key = ((unsigned long long)l << 32) | c;
    atomicAdd(&accA[s], q_mix(key ^ 0x243f6a8885a308d3ull));
    atomicAdd(&accB[s], q_mix2(key + 0x13198a2e03707344ull));
}

// New classes: states with the same (old class, signature) share the index of the first of them to arrive.
__global__ void k_q_number(uint32_t S, const uint8_t *live, const uint32_t *cls, const unsigned long long *accA,
                           const unsigned long long *accB, uint32_t *table, uint32_t mask, uint32_t *cls_new, uint32_t *ctl) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    if (!live[s]) {
        cls_new[s] = kQEmpty;
        return;
    }
    const uint32_t c = cls[s];
    const unsigned long long a = accA[s], b = accB[s];
    uint32_t slot = (uint32_t)q_mix(a ^ q_mix2(b + c)) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
        const uint32_t o = atomicCAS(&table[slot], kQEmpty, s);
        if (o == kQEmpty) {
            cls_new[s] = s;
            atomicAdd(&ctl[Q_CLASSES], 1u);
            return;
        }
        if (cls[o] == c && accA[o] == a && accB[o] == b) {
            cls_new[s] = o;
            return;
        }
    }
    cls_new[s] = s;
    atomicOr(&ctl[Q_ERROR], (uint32_t)Q_ERR_TABLE_FULL);
}

// Exact verification, after a k_q_edges sweep with dedup over the final classes (table = every state's exact pair set):
// each pair of a state must be a pair of its class representative ...
__global__ void k_q_verify_edges(uint32_t E, const uint32_t *src32, const uint32_t *dst32, const uint32_t *lid, const uint32_t *cls,
                                 const uint32_t *table, uint32_t mask, uint32_t *ctl) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const uint32_t l = lid[e];
    if (l == kQEmpty) return;
    const uint32_t s = src32[e], r = cls[s], c = cls[dst32[e]];
    if (r == s) return;
    uint32_t slot = q_triple_hash(r, l, c) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
        const uint32_t o = table[slot];
        if (o == kQEmpty) break;
        if (src32[o] == r && lid[o] == l && cls[dst32[o]] == c) return;
    }
    atomicOr(&ctl[Q_ERROR], (uint32_t)Q_ERR_PAIR);
}
// ... and have as many distinct pairs and the same final flag; a representative represents itself.
__global__ void k_q_verify_states(uint32_t S, const uint8_t *live, const uint8_t *fin, const uint32_t *cls, const uint32_t *cnt,
                                  uint32_t *ctl) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S || !live[s]) return;
    const uint32_t r = cls[s];
    if (r >= S || !live[r] || cls[r] != r || fin[r] != fin[s] || cnt[r] != cnt[s]) atomicOr(&ctl[Q_ERROR], (uint32_t)Q_ERR_STATE);
}

}  // namespace dev
}  // namespace stcsp
