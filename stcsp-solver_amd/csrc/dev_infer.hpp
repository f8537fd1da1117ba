// dev_infer.hpp -- what the unobserved entries of a partially observed stream can be, on the device.
//
// There is no reference counterpart. Contract: stcsp_engine.h, stcsp_engine_infer. The pass is the forward-backward sweep
// over (time x automaton) and the third member of a family: dev_generate.hpp sums the weights of all edges, dev_repair.hpp
// takes minima of costs, this one sums over the edges that MATCH the stream's step and then sweeps forward. It runs over
// the canonical CSR of the last generator_build() (off / eid / dstp, live states only) and the label ids of dev_repair.hpp
// (lid / rep, built once for both calls), one dev_repair.hpp BatchStream per stream of the batch.
//
// Once per generator_build(), on the first infer:
//   k_i_rows      one lane per (label, observable variable): the representative's value, for the host to build the sorted
//                 dictionaries of the values each variable carries and vidx[label][v], the index into them.
// Per batch of streams:
//   k_i_match     one lane per (step of the batch, label): match[step][label] = 1 iff the representative's row agrees with
//                 every observed entry of the step; one byte, written once, coalesced (the pattern of k_r_cost).
//   k_i_level0    B_0.
//   k_i_backward  once per level r = 1 .. the longest stream of the batch, blockIdx.y = stream, one lane per state: pulls over
//                 the segment IN ORDER, 4 B lid + 4 B dst streamed, 1 B match gathered, 8 B B_{r-1}(dst) gathered for a
//                 matching edge, one 8 B store per state. The order of the sum is the contract, so there is no wave-wide
//                 reduction here, not even for a long segment (k_g_weights does the same). <true>: dev_posterior.hpp's, with
//                 one 8 B gather of w[lid] per matching edge, one multiply and one add per term.
//   k_i_root      one lane per stream: count = B_len(root), F_0[root] = count > 0.
//   k_i_forward   once per level t = 0 .. longest - 1, one lane per (state, stream): for s in F_t every matching edge whose
//                 destination has weight to go marks F_{t+1}[dst] and feas[step][lid], by plain vector byte stores of the
//                 value 1 (every writer writes the same byte). The launches are the dependency. Booleans have no order, so
//                 states on dev_repair.hpp's long list go to
//   k_i_forward_long  one wavefront per (long state, stream), lanes stride the segment.
//   k_i_count     |F_t| for every level of every stream: a wave-wide ballot per level, one vector atomic per wavefront.
//   k_i_support   one lane per (step, label) with feas set: ORs bit vidx[label][v] into the step's bitmap of variable v with a
//                 vector atomic. Sorted dictionaries make bit order value order; the host expands the bitmaps.
//   k_i_walk      one lane per (stream, draw), both modes (template): k_g_generate over the matching edges and the stream's
//                 own B.
//
// Floating point: one add, one subtract, one multiply or one compare at a time, contraction off: see the contract.
// The tables are [stream of the batch][len + 1][S], streams packed one after the other: doubles for B, bytes for F.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_repair.hpp"

namespace stcsp {
namespace dev {

constexpr int32_t kInfMissing = INT32_MIN;  // STCSP_INFER_MISSING
enum { I_ERROR = 0, I_WORDS = 4 };
enum { I_ERR_NO_EDGE = 8 };

// out: [n_labels][n_obs]
__global__ void k_i_rows(uint32_t n_labels, const uint32_t *rep, const int32_t *values, int N, const int32_t *obs, int n_obs, int32_t *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_labels * n_obs) return;
    const uint32_t l = (uint32_t)(i / n_obs);
    const int v = (int)(i % n_obs);
    out[i] = values[(size_t)rep[l] * N + obs[v]];
}

// rows: the observed steps of the batch, [steps][n_obs]; match: [steps][n_labels]. blockIdx.y strides the steps.
__global__ void k_i_match(uint32_t n_labels, uint32_t steps, const uint32_t *rep, const int32_t *values, int N, const int32_t *obs, int n_obs,
                          const int32_t *rows, uint8_t *match) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_labels) return;
    const int32_t *row = values + (size_t)rep[l] * N;
    for (size_t step = blockIdx.y; step < steps; step += gridDim.y) {
        const int32_t *x = rows + step * n_obs;
        bool ok = true;
        for (int v = 0; v < n_obs && ok; v++) {
            const int32_t xv = x[v];
            ok = xv == kInfMissing || row[obs[v]] == xv;
        }
        match[step * n_labels + l] = ok ? 1 : 0;
    }
}

// blockIdx.y = stream of the batch
__global__ void k_i_level0(uint32_t S, const BatchStream *streams, const uint8_t *live, const uint8_t *fin, int end_final, double *B) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    B[streams[blockIdx.y].table + s] = live[s] && (!end_final || fin[s]) ? 1.0 : 0.0;
}

// Level r: B_r(s) for every stream of the batch with len >= r. blockIdx.y = stream. <true, const double *> (dev_posterior.hpp)
// takes w, [n_labels], after match: every term times w[label], terms that are not positive left out. <false> has no such argument.
// W is a pack so that <false> keeps k_i_backward's argument list, and with it the kernarg layout and registers, of before the merge.
template <bool WEIGHTED, typename... W>
__global__ __launch_bounds__(256) void k_i_backward(uint32_t S, uint32_t r, const BatchStream *streams, const uint32_t *off, const uint32_t *lid,
                                                    const uint32_t *dstp, uint32_t n_labels, const uint8_t *match, W... w, double *B) {
#pragma clang fp contract(off)
    static_assert(sizeof...(W) == (WEIGHTED ? 1 : 0), "k_i_backward<false> or k_i_backward<true, const double *>");
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const BatchStream st = streams[blockIdx.y];
    if (s >= S || r > st.len) return;
    const double *B_prev = B + st.table + (size_t)(r - 1) * S;
    const uint8_t *m = match + (st.step + (st.len - r)) * n_labels;
    double acc = 0.0;
    for (uint32_t k = off[s], end = off[s + 1]; k < end; k++) {
        if constexpr (!WEIGHTED) {
            if (m[lid[k]]) acc = acc + B_prev[dstp[k]];
        } else {
            const uint32_t l = lid[k];
            if (!m[l]) continue;
            const double wl = (w, ...)[l];
            if (!(wl > 0.0)) continue;
            const double b = B_prev[dstp[k]];
            if (!(b > 0.0)) continue;
            const double term = wl * b;
            acc = acc + term;
        }
    }
    B[st.table + (size_t)r * S + s] = acc;
}

// One lane per stream of the batch: the count and F_0. A root that is not live has B == 0 on every level.
__global__ void k_i_root(uint32_t n, const BatchStream *streams, uint32_t S, const double *B, uint8_t *F, double *count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BatchStream st = streams[i];
    const double c = B[st.table + (size_t)st.len * S];
    count[i] = c;
    if (c > 0.0) F[st.table] = 1;
}

// the edges at positions [k, end) at a stride that are feasible at this step: mark their destination and their label
__device__ inline void i_segment_mark(uint32_t k, uint32_t end, uint32_t stride, const uint32_t *lid, const uint32_t *dstp, const uint8_t *m,
                                      const double *B_next, uint8_t *F_next, uint8_t *feas) {
    for (; k < end; k += stride) {
        const uint32_t l = lid[k];
        if (!m[l]) continue;
        const uint32_t d = dstp[k];
        if (B_next[d] > 0.0) {
            F_next[d] = 1;
            feas[l] = 1;
        }
    }
}

// Level t: F_{t+1} and the feasible labels of step t for every stream of the batch with len > t. blockIdx.y = stream.
__global__ __launch_bounds__(256) void k_i_forward(uint32_t S, uint32_t t, const BatchStream *streams, const uint32_t *off, const uint32_t *lid,
                                                   const uint32_t *dstp, uint32_t n_labels, const uint8_t *match, const double *B,
                                                   uint32_t wave_segment, uint8_t *F, uint8_t *feas) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const BatchStream st = streams[blockIdx.y];
    if (s >= S || t >= st.len) return;
    if (!F[st.table + (size_t)t * S + s]) return;
    const uint32_t b = off[s], end = off[s + 1];
    if (end - b > wave_segment) return;  // k_i_forward_long's
    const size_t step = st.step + t;
    i_segment_mark(b, end, 1, lid, dstp, match + step * n_labels, B + st.table + (size_t)(st.len - t - 1) * S,
                   F + st.table + (size_t)(t + 1) * S, feas + step * n_labels);
}

// One wavefront per (long state, stream): blocks of 256 lanes take 4 long states. blockIdx.y = stream.
__global__ __launch_bounds__(256) void k_i_forward_long(uint32_t n_long, const uint32_t *long_states, uint32_t S, uint32_t t,
                                                        const BatchStream *streams, const uint32_t *off, const uint32_t *lid, const uint32_t *dstp,
                                                        uint32_t n_labels, const uint8_t *match, const double *B, uint8_t *F, uint8_t *feas) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const BatchStream st = streams[blockIdx.y];
    if (i >= n_long || t >= st.len) return;
    const uint32_t s = long_states[i];
    if (!F[st.table + (size_t)t * S + s]) return;
    const size_t step = st.step + t;
    i_segment_mark(off[s] + lane, off[s + 1], 64, lid, dstp, match + step * n_labels, B + st.table + (size_t)(st.len - t - 1) * S,
                   F + st.table + (size_t)(t + 1) * S, feas + step * n_labels);
}

// |F_t| for t = 0 .. len of every stream: blockIdx.y = stream, one lane per state; n_states zeroed by the host beforehand.
// Every lane of a wavefront stays to the end (the ballot is wave-wide); a lane past S counts nothing.
__global__ __launch_bounds__(256) void k_i_count(uint32_t S, const BatchStream *streams, const uint8_t *F, int32_t *n_states) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const BatchStream st = streams[blockIdx.y];
    const uint8_t *T = F + st.table;
    int32_t *out = n_states + st.step + st.index;
    for (uint32_t t = 0; t <= st.len; t++) {
        const bool in = s < S && T[(size_t)t * S + s];
        const unsigned long long mask = __ballot(in);
        if (lane == 0 && mask) atomicAdd(&out[t], (int32_t)__popcll(mask));
    }
}

// feas: [steps][n_labels]; vidx: [n_labels][n_obs]; word_off: [n_obs] first bitmap word of a variable; bits: [steps][words],
// zeroed by the host beforehand. blockIdx.y strides the steps.
__global__ void k_i_support(uint32_t n_labels, uint32_t steps, const uint8_t *feas, const uint32_t *vidx, const uint32_t *word_off, int n_obs,
                            uint32_t words, uint32_t *bits) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_labels) return;
    for (size_t step = blockIdx.y; step < steps; step += gridDim.y) {
        if (!feas[step * n_labels + l]) continue;
        uint32_t *row = bits + step * words;
        for (int v = 0; v < n_obs; v++) {
            const uint32_t i = vidx[(size_t)l * n_obs + v];
            atomicOr(&row[word_off[v] + (i >> 5)], 1u << (i & 31));
        }
    }
}

// One lane per (stream of the batch, draw). q0: the index of the batch's first draw in the request. ranks: the batch's, valid.
// out: the batch's draws, [stream][draw][len][n_obs], filled with MISSING by the host beforehand; end_final zeroed.
template <bool UNRANK>
__global__ void k_i_walk(uint32_t n_q, uint32_t draws, unsigned long long q0, unsigned long long seed, const unsigned long long *ranks,
                         const BatchStream *streams, uint32_t S, const double *B, const uint32_t *off, const uint32_t *lid, const uint32_t *dstp,
                         const uint32_t *eid, uint32_t n_labels, const uint8_t *match, const int32_t *values, int N, const int32_t *obs, int n_obs,
                         const uint8_t *fin, int32_t *out, uint8_t *end_final, uint32_t *ctl) {
#pragma clang fp contract(off)
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_q) return;
    const BatchStream st = streams[q / draws];
    const double *T = B + st.table;
    if (!(T[(size_t)st.len * S] > 0.0)) return;  // infeasible: rows of MISSING, end_final 0
    int32_t *rows = out + (st.step * draws + (size_t)(q % draws) * st.len) * n_obs;
    uint32_t s = 0;
    double tau = 0.0;
    if (UNRANK) tau = (double)ranks[q];
    for (uint32_t t = 0; t < st.len; t++) {
        const uint32_t r = st.len - t;
        const double *B_next = T + (size_t)(r - 1) * S;
        const uint8_t *m = match + (st.step + t) * n_labels;
        if (!UNRANK) tau = g_uniform(seed, q0 + q, t) * T[(size_t)r * S + s];
        double acc = 0.0, before = 0.0, before_last = 0.0;
        uint32_t pick = kQEmpty, last = kQEmpty;
        for (uint32_t k = off[s], end = off[s + 1]; k < end; k++) {
            if (!m[lid[k]]) continue;
            const double w = B_next[dstp[k]];
            if (w > 0.0) {
                last = k;
                before_last = acc;
            }
            const double sum = acc + w;
            if (sum > tau) {
                pick = k;
                before = acc;
                break;
            }
            acc = sum;
        }
        if (pick == kQEmpty) {
            pick = last;
            before = before_last;
        }
        if (pick == kQEmpty) {  // no matching edge of non-zero weight: the table contradicts B_r(s) > 0; the host refuses the result
            atomicOr(&ctl[I_ERROR], (uint32_t)I_ERR_NO_EDGE);
            return;
        }
        if (UNRANK) tau = tau - before;
        const int32_t *row = values + (size_t)eid[pick] * N;
        for (int v = 0; v < n_obs; v++) rows[(size_t)t * n_obs + v] = row[obs[v]];
        s = dstp[pick];
    }
    end_final[q] = fin[s] ? 1 : 0;
}

}  // namespace dev
}  // namespace stcsp
