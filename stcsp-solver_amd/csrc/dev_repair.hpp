// dev_repair.hpp -- the nearest solution prefix of an observed stream, on the device.
//
// There is no reference counterpart. Contract: stcsp_engine.h, stcsp_engine_repair. The pass runs over the canonical CSR
// of the last generator_build() (dev_generate.hpp: off / eid / dstp, live states only) and is the tropical twin of its
// weight table: W_{t+1}(s) = sum W_t(dst) there, G_{r+1}(s) = min (cost + G_r(dst)) here, and the walk from the root takes
// the first edge that attains the minimum where k_g_generate takes the first edge whose running sum passes the target.
//
// Once per generator_build(), on the first repair:
//   k_r_labels    one lane per CSR position: the exact id of the edge's projected label by lookup-or-insert with a full-key
//                 compare (the pattern of k_q_labels); lid[k] = the slot that holds the label.
//   k_r_number    one lane per slot: a taken slot gets the next dense id and names its edge as the label's representative.
//   k_r_remap     one lane per CSR position: lid[k] = dense id. The ids depend on the scheduler; no output does.
//   k_r_long      one lane per state: the states with more than `wave_segment` live out-edges, as a list.
// Per batch of streams:
//   k_r_cost      one lane per (step of the batch, label): cost[step][label] from the representative's row and the observed
//                 row, n_obs compares; written once, coalesced.
//   k_r_level0    G_0.
//   k_r_relax     once per level r = 1 .. the longest stream of the batch, blockIdx.y = stream, one lane per state: pulls
//                 over the segment, 4 B lid + 4 B dst streamed, 4 B cost and 4 B G_{r-1}(dst) gathered per edge, one 4 B
//                 store per state. No atomics; the launches are the dependency. A stream takes part while r <= len.
//                 States on the long list are left to
//   k_r_relax_long  one wavefront per (long state, stream): lanes stride the segment, a wave-wide min, lane 0 stores.
//   k_r_walk      one lane per stream: per step the first edge of the segment with cost + G_{r-1}(dst) == G_r(s); its
//                 projected row goes out by plain vector stores.
//
// Everything is uint32 arithmetic; kRepInf = 0xffffffff is "no path". The host refuses requests whose finite values could
// reach it. The table is [stream of the batch][len + 1][S], streams packed one after the other.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_generate.hpp"

namespace stcsp {
namespace dev {

constexpr uint32_t kRepInf = 0xffffffffu;
constexpr int32_t kRepMissing = INT32_MIN;  // STCSP_REPAIR_MISSING
// a state with more live out-edges than this is relaxed by a wavefront (k_r_relax_long); STCSP_REPAIR_WAVE_SEGMENT overrides
constexpr uint32_t kRepWaveSegment = 128;
enum { R_LABELS = 0, R_LONG = 1, R_ERROR = 2, R_WORDS = 4 };
enum { R_ERR_TABLE_FULL = 1, R_ERR_NO_EDGE = 8 };

// what the kernels of repair, inference and posterior need to know of one stream of the batch
struct BatchStream {
    unsigned long long table;  // first entry of its [len + 1][S] tables
    unsigned long long step;   // its first step among the steps of the batch
    uint32_t len;
    uint32_t index;            // its place in the batch
};

__global__ void k_r_labels(uint32_t total, const uint32_t *eid, const int32_t *values, int N, const int32_t *obs, int n_obs, uint32_t *table,
                           uint32_t mask, uint32_t *lid, uint32_t *ctl) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= total) return;
    const uint32_t e = eid[k];
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
        lid[k] = slot;
        return;
    }
    lid[k] = 0;
    atomicOr(&ctl[R_ERROR], (uint32_t)R_ERR_TABLE_FULL);
}

// table[slot]: the representative edge -> the dense id; rep[id] = the edge
__global__ void k_r_number(uint32_t slots, uint32_t *table, uint32_t *rep, uint32_t *ctl) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= slots) return;
    const uint32_t e = table[slot];
    if (e == kQEmpty) return;
    const uint32_t id = atomicAdd(&ctl[R_LABELS], 1u);
    rep[id] = e;
    table[slot] = id;
}

__global__ void k_r_remap(uint32_t total, const uint32_t *table, uint32_t *lid) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= total) return;
    lid[k] = table[lid[k]];
}

// long_states has room for S entries
__global__ void k_r_long(uint32_t S, const uint32_t *off, uint32_t wave_segment, uint32_t *long_states, uint32_t *ctl) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    if (off[s + 1] - off[s] > wave_segment) long_states[atomicAdd(&ctl[R_LONG], 1u)] = s;
}

// rows: the observed steps of the batch, [steps][n_obs]; cost: [steps][n_labels]. blockIdx.y strides the steps.
__global__ void k_r_cost(uint32_t n_labels, uint32_t steps, const uint32_t *rep, const int32_t *values, int N, const int32_t *obs, int n_obs,
                         const int32_t *weights, const int32_t *rows, uint32_t *cost) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_labels) return;
    const int32_t *row = values + (size_t)rep[l] * N;
    for (size_t step = blockIdx.y; step < steps; step += gridDim.y) {
        const int32_t *x = rows + step * n_obs;
        uint32_t c = 0;
        for (int v = 0; v < n_obs; v++) {
            const int32_t xv = x[v];
            if (xv != kRepMissing && row[obs[v]] != xv) c += (uint32_t)weights[v];
        }
        cost[step * n_labels + l] = c;
    }
}

// blockIdx.y = stream of the batch
__global__ void k_r_level0(uint32_t S, const BatchStream *streams, const uint8_t *live, const uint8_t *fin, int end_final, uint32_t *G) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    G[streams[blockIdx.y].table + s] = live[s] && (!end_final || fin[s]) ? 0u : kRepInf;
}

// min over positions [k, end) at a stride: the term of an edge whose destination has no path stays out
__device__ inline uint32_t r_segment_min(uint32_t k, uint32_t end, uint32_t stride, const uint32_t *lid, const uint32_t *dstp,
                                         const uint32_t *cost, const uint32_t *G_prev) {
    uint32_t best = kRepInf;
    for (; k < end; k += stride) {
        const uint32_t g = G_prev[dstp[k]];
        const uint32_t c = cost[lid[k]];
        const uint32_t sum = c + g;  // (g finite: no wrap, see the contract's bound)
        if (g != kRepInf && sum < best) best = sum;
    }
    return best;
}

// Level r: G_r(s) for every stream of the batch with len >= r. blockIdx.y = stream.
__global__ __launch_bounds__(256) void k_r_relax(uint32_t S, uint32_t r, const BatchStream *streams, const uint32_t *off, const uint32_t *lid,
                                                 const uint32_t *dstp, uint32_t n_labels, const uint32_t *cost, uint32_t wave_segment,
                                                 uint32_t *G) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const BatchStream st = streams[blockIdx.y];
    if (s >= S || r > st.len) return;
    const uint32_t b = off[s], end = off[s + 1];
    if (end - b > wave_segment) return;  // k_r_relax_long's
    const uint32_t *G_prev = G + st.table + (size_t)(r - 1) * S;
    const uint32_t *c = cost + (st.step + (st.len - r)) * n_labels;
    G[st.table + (size_t)r * S + s] = r_segment_min(b, end, 1, lid, dstp, c, G_prev);
}

// One wavefront per (long state, stream): blocks of 256 lanes take 4 long states. blockIdx.y = stream.
__global__ __launch_bounds__(256) void k_r_relax_long(uint32_t n_long, const uint32_t *long_states, uint32_t S, uint32_t r,
                                                      const BatchStream *streams, const uint32_t *off, const uint32_t *lid, const uint32_t *dstp,
                                                      uint32_t n_labels, const uint32_t *cost, uint32_t *G) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const BatchStream st = streams[blockIdx.y];
    if (i >= n_long || r > st.len) return;  // (wave-uniform)
    const uint32_t s = long_states[i];
    const uint32_t *G_prev = G + st.table + (size_t)(r - 1) * S;
    const uint32_t *c = cost + (st.step + (st.len - r)) * n_labels;
    uint32_t best = r_segment_min(off[s] + lane, off[s + 1], 64, lid, dstp, c, G_prev);
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t other = __shfl_xor(best, d);
        if (other < best) best = other;
    }
    if (lane == 0) G[st.table + (size_t)r * S + s] = best;
}

// One lane per stream of the batch. rows / out: [steps of the batch][n_obs], out zeroed by the host beforehand.
__global__ void k_r_walk(uint32_t n, const BatchStream *streams, uint32_t S, const uint32_t *G, const uint32_t *off, const uint32_t *lid,
                         const uint32_t *dstp, const uint32_t *eid, uint32_t n_labels, const uint32_t *cost, const int32_t *values, int N,
                         const int32_t *obs, int n_obs, const uint8_t *fin, const int32_t *rows, int32_t *out, int32_t *distance,
                         uint8_t *end_final, int32_t *n_changed, uint32_t *ctl) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BatchStream st = streams[i];
    const uint32_t *T = G + st.table;
    const uint32_t total = T[(size_t)st.len * S];  // G_len(root)
    if (total == kRepInf) {
        distance[i] = -1;
        end_final[i] = 0;
        n_changed[i] = 0;
        return;
    }
    uint32_t s = 0, changed = 0;
    for (uint32_t t = 0; t < st.len; t++) {
        const uint32_t r = st.len - t;
        const uint32_t want = T[(size_t)r * S + s];
        const uint32_t *G_next = T + (size_t)(r - 1) * S;
        const uint32_t *c = cost + (st.step + t) * n_labels;
        uint32_t pick = kQEmpty;
        for (uint32_t k = off[s], end = off[s + 1]; k < end; k++) {
            const uint32_t g = G_next[dstp[k]];
            if (g != kRepInf && c[lid[k]] + g == want) {
                pick = k;
                break;
            }
        }
        if (pick == kQEmpty) {  // the table contradicts itself; the host refuses the result
            atomicOr(&ctl[R_ERROR], (uint32_t)R_ERR_NO_EDGE);
            break;
        }
        const int32_t *row = values + (size_t)eid[pick] * N;
        const int32_t *x = rows + (st.step + t) * n_obs;
        int32_t *y = out + (st.step + t) * n_obs;
        for (int v = 0; v < n_obs; v++) {
            const int32_t p = row[obs[v]], xv = x[v];
            y[v] = p;
            changed += xv != kRepMissing && xv != p;
        }
        s = dstp[pick];
    }
    distance[i] = (int32_t)total;
    end_final[i] = fin[s] ? 1 : 0;
    n_changed[i] = (int32_t)changed;
}

}  // namespace dev
}  // namespace stcsp
