// dev_align.hpp -- aligning an observed stream with the solution language, on the device.
//
// There is no reference counterpart. Contract: stcsp_engine.h, stcsp_engine_align. The repair's shortest path over
// (time x automaton) (dev_repair.hpp) with two more arcs: a skip keeps the state and consumes a step, an insert follows an
// edge and consumes none. The inserts make every level a shortest-path problem of its own, the closure
//   G(s) = min(B(s), gap + min over the live out-edges of G(dst)),
// whose least fixpoint is unique because gap >= 1, so sweeps in any order, Jacobi or in place, reach it. Label ids, long
// list, cost table and stream records are the repair's (k_r_labels .. k_r_cost, BatchStream); rows are counted in steps
// remaining, r = len - t, as there.
//
// Two roads to the same table [stream of the batch][len + 1][S]:
//   k_a_fused     one workgroup per stream, every level in one launch. The rows r - 1 and r sit in LDS (2 x 4 B x S of
//                 dynamic shared memory). Per level: B from the LDS row, 4 B lid + 4 B dst streamed and 4 B cost gathered
//                 per edge; closure sweeps over the LDS row, 4 B dst streamed per edge and sweep, in place, between
//                 workgroup barriers until a sweep stores nothing (__syncthreads_or); then the row goes to HBM, coalesced.
//                 No grid barrier, no atomics on the table, no host round trip. States on the long list (more than
//                 `wave_segment` live out-edges) are taken by whole wavefronts of the workgroup in turn, lanes striding the
//                 segment, as k_r_relax_long does.
//   k_a_base      level r of every stream with len >= r, blockIdx.y = stream: k_r_relax plus the skip term;
//   k_a_base_long the wavefront variant for the long list;
//   k_a_sweep     one closure sweep of level r over (state, stream), in place: 4 B dst streamed and 4 B G gathered per edge;
//   k_a_sweep_long  a state that stores raises ctl[A_CHANGED]; the host reads the word once per group of sweeps.
// Then, on either road:
//   k_a_distance  one lane per stream: G_len(root).
//   k_a_walk      one lane per stream: the four rules of the contract; rows and ops go out by plain vector stores into
//                 room for len + distance / gap of each, which the host sized from k_a_distance's answer.
//
// Everything is uint32 arithmetic; kRepInf is "no alignment". The host refuses requests whose finite values, those in
// the middle of a closure included, could reach it (align_host.hpp: align_request_ok).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_repair.hpp"

namespace stcsp {
namespace dev {

// The fused road holds two rows of S uint32 in LDS. A CU has 160 KiB; __syncthreads_or keeps a few words of its own,
// for which 1 KiB is set aside: S <= (160 KiB - 1 KiB) / 8 B.
constexpr uint32_t kAlnLdsBytes = 160u << 10;
constexpr uint32_t kAlnLdsReserve = 1u << 10;
constexpr uint32_t kAlnFusedStates = (kAlnLdsBytes - kAlnLdsReserve) / (2 * sizeof(uint32_t));  // 20,352
constexpr uint32_t kAlnFusedThreads = 1024;
constexpr uint32_t kAlnSweepGroup = 4;  // closure sweeps of the general road per read of the changed word
enum { A_CHANGED = 0, A_ERROR = 1, A_WORDS = 4 };
enum { A_ERR_NO_RULE = 1, A_ERR_NO_ROOM = 2, A_ERR_SWEEPS = 4 };
enum { A_OP_MATCH = 0, A_OP_SKIP = 1, A_OP_INSERT = 2 };

// gap + the least G over the positions [k, end) at a stride; a destination without an alignment stays out. The row is the one
// the sweeps store to in place while others read it: every access is volatile, one whole 4-byte load or store each.
__device__ inline uint32_t a_gap_min(uint32_t k, uint32_t end, uint32_t stride, const uint32_t *dstp, const volatile uint32_t *row, uint32_t gap) {
    uint32_t best = kRepInf;
    for (; k < end; k += stride) {
        const uint32_t g = row[dstp[k]];
        const uint32_t sum = gap + g;  // (g finite: no wrap, see the contract's bound)
        if (g != kRepInf && sum < best) best = sum;
    }
    return best;
}

__device__ inline uint32_t a_wave_min(uint32_t best) {
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t other = __shfl_xor(best, d);
        if (other < best) best = other;
    }
    return best;
}

// B(s) from the matches (over the segment, already reduced) and the skip
__device__ inline uint32_t a_with_skip(uint32_t matched, uint32_t below, uint32_t skip) {
    const uint32_t sum = skip + below;
    return below != kRepInf && sum < matched ? sum : matched;
}

// The closure of one LDS row by the whole workgroup, in place. Every thread of the block calls it.
__device__ inline void a_close_row(uint32_t S, volatile uint32_t *row, const uint32_t *off, const uint32_t *dstp, uint32_t wave_segment, uint32_t n_long,
                                   const uint32_t *long_states, uint32_t gap, uint32_t *ctl) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    for (uint32_t sweeps = 0;; sweeps++) {
        int changed = 0;
        for (uint32_t s = threadIdx.x; s < S; s += blockDim.x) {
            const uint32_t b = off[s], end = off[s + 1];
            if (end - b > wave_segment) continue;
            const uint32_t best = a_gap_min(b, end, 1, dstp, row, gap);
            if (best < row[s]) {
                row[s] = best;
                changed = 1;
            }
        }
        for (uint32_t i = wave; i < n_long; i += waves) {  // (wave-uniform)
            const uint32_t s = long_states[i];
            const uint32_t best = a_wave_min(a_gap_min(off[s] + lane, off[s + 1], 64, dstp, row, gap));
            if (lane == 0 && best < row[s]) {
                row[s] = best;
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
        if (sweeps > S) {  // a shortest path has fewer than S edges: unreachable (block-uniform)
            if (threadIdx.x == 0) atomicOr(&ctl[A_ERROR], (uint32_t)A_ERR_SWEEPS);
            break;
        }
    }
}

// One workgroup per stream of the batch, every level: dynamic shared memory = 2 * S * 4 bytes.
__global__ __launch_bounds__(kAlnFusedThreads) void k_a_fused(uint32_t S, const BatchStream *streams, const uint32_t *off, const uint32_t *lid,
                                                             const uint32_t *dstp, uint32_t n_labels, const uint32_t *cost, uint32_t wave_segment,
                                                             uint32_t n_long, const uint32_t *long_states, const uint8_t *live, const uint8_t *fin,
                                                             int end_final, uint32_t skip, uint32_t gap, uint32_t *G, uint32_t *ctl) {
    extern __shared__ uint32_t a_rows[];
    const BatchStream st = streams[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    uint32_t *below = a_rows, *row = a_rows + S;
    uint32_t *T = G + st.table;
    for (uint32_t s = threadIdx.x; s < S; s += blockDim.x) below[s] = live[s] && (!end_final || fin[s]) ? 0u : kRepInf;
    __syncthreads();
    if (end_final) a_close_row(S, below, off, dstp, wave_segment, n_long, long_states, gap, ctl);
    for (uint32_t s = threadIdx.x; s < S; s += blockDim.x) T[s] = below[s];
    for (uint32_t r = 1; r <= st.len; r++) {
        // (the row written here was last read before the barriers of the level before)
        const uint32_t *c = cost + (st.step + (st.len - r)) * n_labels;
        for (uint32_t s = threadIdx.x; s < S; s += blockDim.x) {
            const uint32_t b = off[s], end = off[s + 1];
            if (end - b > wave_segment) continue;
            row[s] = a_with_skip(r_segment_min(b, end, 1, lid, dstp, c, below), below[s], skip);
        }
        for (uint32_t i = wave; i < n_long; i += waves) {
            const uint32_t s = long_states[i];
            const uint32_t best = a_wave_min(r_segment_min(off[s] + lane, off[s + 1], 64, lid, dstp, c, below));
            if (lane == 0) row[s] = a_with_skip(best, below[s], skip);
        }
        __syncthreads();
        a_close_row(S, row, off, dstp, wave_segment, n_long, long_states, gap, ctl);
        for (uint32_t s = threadIdx.x; s < S; s += blockDim.x) T[(size_t)r * S + s] = row[s];
        uint32_t *swap = below;
        below = row;
        row = swap;
    }
}

// Level r without the closure: B_r(s) for every stream of the batch with len >= r. blockIdx.y = stream.
__global__ __launch_bounds__(256) void k_a_base(uint32_t S, uint32_t r, const BatchStream *streams, const uint32_t *off, const uint32_t *lid,
                                                const uint32_t *dstp, uint32_t n_labels, const uint32_t *cost, uint32_t wave_segment, uint32_t skip,
                                                uint32_t *G) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const BatchStream st = streams[blockIdx.y];
    if (s >= S || r > st.len) return;
    const uint32_t b = off[s], end = off[s + 1];
    if (end - b > wave_segment) return;  // k_a_base_long's
    const uint32_t *below = G + st.table + (size_t)(r - 1) * S;
    const uint32_t *c = cost + (st.step + (st.len - r)) * n_labels;
    G[st.table + (size_t)r * S + s] = a_with_skip(r_segment_min(b, end, 1, lid, dstp, c, below), below[s], skip);
}

// One wavefront per (long state, stream): blocks of 256 lanes take 4 long states. blockIdx.y = stream.
__global__ __launch_bounds__(256) void k_a_base_long(uint32_t n_long, const uint32_t *long_states, uint32_t S, uint32_t r, const BatchStream *streams,
                                                     const uint32_t *off, const uint32_t *lid, const uint32_t *dstp, uint32_t n_labels,
                                                     const uint32_t *cost, uint32_t skip, uint32_t *G) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const BatchStream st = streams[blockIdx.y];
    if (i >= n_long || r > st.len) return;  // (wave-uniform)
    const uint32_t s = long_states[i];
    const uint32_t *below = G + st.table + (size_t)(r - 1) * S;
    const uint32_t *c = cost + (st.step + (st.len - r)) * n_labels;
    const uint32_t best = a_wave_min(r_segment_min(off[s] + lane, off[s + 1], 64, lid, dstp, c, below));
    if (lane == 0) G[st.table + (size_t)r * S + s] = a_with_skip(best, below[s], skip);
}

// One closure sweep of level r, in place: a 4-byte value another lane stores meanwhile is an upper bound of the fixpoint
// either way, and a sweep in which nobody stores has read the fixpoint. blockIdx.y = stream.
__global__ __launch_bounds__(256) void k_a_sweep(uint32_t S, uint32_t r, const BatchStream *streams, const uint32_t *off, const uint32_t *dstp,
                                                 uint32_t wave_segment, uint32_t gap, uint32_t *G, uint32_t *ctl) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const BatchStream st = streams[blockIdx.y];
    if (s >= S || r > st.len) return;
    const uint32_t b = off[s], end = off[s + 1];
    if (end - b > wave_segment) return;  // k_a_sweep_long's
    volatile uint32_t *row = G + st.table + (size_t)r * S;
    const uint32_t best = a_gap_min(b, end, 1, dstp, row, gap);
    if (best < row[s]) {
        row[s] = best;
        ctl[A_CHANGED] = 1;
    }
}

__global__ __launch_bounds__(256) void k_a_sweep_long(uint32_t n_long, const uint32_t *long_states, uint32_t S, uint32_t r, const BatchStream *streams,
                                                      const uint32_t *off, const uint32_t *dstp, uint32_t gap, uint32_t *G, uint32_t *ctl) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const BatchStream st = streams[blockIdx.y];
    if (i >= n_long || r > st.len) return;  // (wave-uniform)
    const uint32_t s = long_states[i];
    volatile uint32_t *row = G + st.table + (size_t)r * S;
    const uint32_t best = a_wave_min(a_gap_min(off[s] + lane, off[s + 1], 64, dstp, row, gap));
    if (lane == 0 && best < row[s]) {
        row[s] = best;
        ctl[A_CHANGED] = 1;
    }
}

// One lane per stream of the batch: G_len(root) as the contract's distance
__global__ void k_a_distance(uint32_t n, const BatchStream *streams, uint32_t S, const uint32_t *G, int32_t *distance) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BatchStream st = streams[i];
    const uint32_t total = G[st.table + (size_t)st.len * S];
    distance[i] = total == kRepInf ? -1 : (int32_t)total;
}

// One lane per stream of the batch. rows: [steps of the batch][n_obs]. room: [n + 1], stream i owns the entries
// room[i] .. room[i + 1] of ops and, times n_obs, of out: len + distance / gap of them, which no walk exceeds.
__global__ void k_a_walk(uint32_t n, const BatchStream *streams, uint32_t S, const uint32_t *G, const uint32_t *off, const uint32_t *lid,
                         const uint32_t *dstp, const uint32_t *eid, uint32_t n_labels, const uint32_t *cost, const int32_t *values, int N,
                         const int32_t *obs, int n_obs, const uint8_t *fin, const int32_t *rows, uint32_t skip, uint32_t gap,
                         const long long *room, const int32_t *distance, int32_t *out, uint8_t *ops, int32_t *n_rows, int32_t *n_ops,
                         uint8_t *end_final, int32_t *n_changed, int32_t *n_skipped, int32_t *n_inserted, uint32_t *ctl) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BatchStream st = streams[i];
    const uint32_t *T = G + st.table;
    uint32_t s = 0, t = 0, changed = 0, skipped = 0, inserted = 0, emitted = 0, done = 0;
    if (distance[i] >= 0) {
        const uint32_t cap = (uint32_t)(room[i + 1] - room[i]);
        int32_t *y = out + (size_t)room[i] * n_obs;
        uint8_t *o = ops + room[i];
        for (;;) {
            const uint32_t r = st.len - t;
            const uint32_t want = T[(size_t)r * S + s];
            if (r == 0 && want == 0) break;  // rule 1: base(s) is 0 or infinite, and `want` is finite
            uint32_t pick = kQEmpty, op = A_OP_INSERT;
            if (r > 0) {
                const uint32_t *below = T + (size_t)(r - 1) * S;
                const uint32_t *c = cost + (st.step + t) * n_labels;
                for (uint32_t k = off[s], end = off[s + 1]; k < end; k++) {  // rule 2
                    const uint32_t g = below[dstp[k]];
                    if (g != kRepInf && c[lid[k]] + g == want) {
                        pick = k;
                        op = A_OP_MATCH;
                        break;
                    }
                }
                if (pick == kQEmpty && below[s] != kRepInf && skip + below[s] == want) op = A_OP_SKIP;  // rule 3
            }
            if (op == A_OP_INSERT) {  // rule 4
                const uint32_t *row = T + (size_t)r * S;
                for (uint32_t k = off[s], end = off[s + 1]; k < end; k++) {
                    const uint32_t g = row[dstp[k]];
                    if (g != kRepInf && gap + g == want) {
                        pick = k;
                        break;
                    }
                }
                if (pick == kQEmpty) {  // the table contradicts itself; the host refuses the result
                    atomicOr(&ctl[A_ERROR], (uint32_t)A_ERR_NO_RULE);
                    break;
                }
            }
            if (done == cap || (op != A_OP_SKIP && emitted == cap)) {
                atomicOr(&ctl[A_ERROR], (uint32_t)A_ERR_NO_ROOM);
                break;
            }
            o[done++] = (uint8_t)op;
            if (op == A_OP_SKIP) {
                skipped++;
                t++;
                continue;
            }
            const int32_t *row = values + (size_t)eid[pick] * N;
            const int32_t *x = rows + (st.step + t) * n_obs;  // (read by a match only)
            int32_t *yr = y + (size_t)emitted * n_obs;
            for (int v = 0; v < n_obs; v++) {
                const int32_t p = row[obs[v]];
                yr[v] = p;
                if (op == A_OP_MATCH) changed += x[v] != kRepMissing && x[v] != p;
            }
            emitted++;
            s = dstp[pick];
            if (op == A_OP_MATCH) t++;
            else inserted++;
        }
    }
    n_rows[i] = (int32_t)emitted;
    n_ops[i] = (int32_t)done;
    end_final[i] = distance[i] >= 0 && fin[s] ? 1 : 0;
    n_changed[i] = (int32_t)changed;
    n_skipped[i] = (int32_t)skipped;
    n_inserted[i] = (int32_t)inserted;
}

}  // namespace dev
}  // namespace stcsp
