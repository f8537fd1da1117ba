// dev_posterior.hpp -- how many solutions give each value of an unobserved stream entry, under value weights, on the device
// (DESIGN.md section 4.20).
//
// There is no reference counterpart. Contract: stcsp_engine.h, stcsp_engine_posterior. The pass is dev_infer.hpp's
// forward-backward sweep with numbers in the place of bits: a weighted backward table of doubles in the contract's order,
// a forward sweep of uint64 (exact streams only: every quantity is an integer below 2^53, so integer atomics in any order
// give the one answer), and a scatter of the per-edge products A * w * B into per-(step, variable, value) bins. It runs
// over the canonical CSR of the last generator_build(), the label ids of dev_repair.hpp and the dictionaries of
// dev_infer.hpp. From dev_infer.hpp it takes k_i_match, k_i_rows, k_i_level0 and k_i_backward<true, const double *> as they are, from
// dev_repair.hpp BatchStream and the long-state list.
//
// Per call:
//   k_p_label_weight  one lane per label: w(l) = the product, in variable order, of the weights of its dictionary entries.
// Per batch of streams:
//   k_i_match, k_i_level0, k_i_backward<true, ...>  (dev_infer.hpp) the weighted B, in canonical order.
//   k_p_root          one lane per stream: mass, exact, A_0[root] = 1 for an exact feasible stream.
//   k_p_forward_long  one wavefront per (long state, stream), lanes stride the segment; launched BEFORE
//   k_p_forward       of the same level: one lane per (state, stream) with A_t > 0. Per feasible edge one 64-bit atomicAdd
//                     of A_t(src) * w into A_{t+1}[dst] and one of A_t(src) * w * B into the step's per-label accumulator.
//                     A has two rolling rows per stream; the lane clears its own A_t(s) after reading it, long states
//                     included, since that row is the target of level t + 1. A stream that has ended keeps A_len.
//   k_p_final         final_mass: a wave-wide sum of A_len over the final states, one vector atomic per wavefront.
//   k_p_bins          one lane per (step, label) of non-zero mass: adds it into bins[step][bin_off[v] + vidx[label][v]] for
//                     every observable v (k_i_support with 64-bit adds in the place of the ORs).
//
// Floating point: one multiply, one add or one compare at a time, contraction off: see the contract.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_infer.hpp"

namespace stcsp {
namespace dev {

typedef unsigned long long p_u64;

// wbin: [bins] the weight of every dictionary entry; vidx: [n_labels][n_obs]; bin_off: [n_obs]
__global__ void k_p_label_weight(uint32_t n_labels, const uint32_t *vidx, const uint32_t *bin_off, int n_obs, const double *wbin, double *w) {
#pragma clang fp contract(off)
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_labels) return;
    double acc = 1.0;
    for (int v = 0; v < n_obs; v++) acc = acc * wbin[bin_off[v] + vidx[(size_t)l * n_obs + v]];
    w[l] = acc;
}

// One lane per stream of the batch. A: [stream][2][S], zeroed by the host beforehand.
__global__ void k_p_root(uint32_t n, const BatchStream *streams, uint32_t S, const double *B, p_u64 *A, double *mass, uint8_t *exact) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BatchStream st = streams[i];
    const double c = B[st.table + (size_t)st.len * S];
    const bool ex = c < 0x1.0p53;
    mass[i] = c;
    exact[i] = ex ? 1 : 0;
    if (ex && c > 0.0) A[(size_t)st.index * 2 * S] = 1;
}

// the edges at positions [k, end) at a stride that are feasible at this step, out of a state of forward mass a. Only a
// feasible edge of an exact stream converts its doubles: there both are integers below 2^53.
__device__ inline void p_segment_add(uint32_t k, uint32_t end, uint32_t stride, const uint32_t *lid, const uint32_t *dstp, const uint8_t *m,
                                     const double *w, const double *B_next, p_u64 a, p_u64 *A_next, p_u64 *lab) {
    for (; k < end; k += stride) {
        const uint32_t l = lid[k];
        if (!m[l]) continue;
        const double wl = w[l];
        if (!(wl > 0.0)) continue;
        const uint32_t d = dstp[k];
        const double b = B_next[d];
        if (!(b > 0.0)) continue;
        const p_u64 aw = a * (p_u64)wl;
        atomicAdd(&A_next[d], aw);
        atomicAdd(&lab[l], aw * (p_u64)b);
    }
}

// Level t: A_{t+1} and the per-label masses of step t for every stream of the batch with len > t. blockIdx.y = stream.
// Launched after k_p_forward_long of the level: it clears A_t(s) for every state, which is then level t + 1's target.
__global__ __launch_bounds__(256) void k_p_forward(uint32_t S, uint32_t t, const BatchStream *streams, const uint32_t *off, const uint32_t *lid,
                                                   const uint32_t *dstp, uint32_t n_labels, const uint8_t *match, const double *w, const double *B,
                                                   uint32_t wave_segment, p_u64 *A, p_u64 *lab) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const BatchStream st = streams[blockIdx.y];
    if (s >= S || t >= st.len) return;
    p_u64 *A_cur = A + ((size_t)st.index * 2 + (t & 1)) * S;
    const p_u64 a = A_cur[s];
    if (!a) return;
    A_cur[s] = 0;
    const uint32_t b = off[s], end = off[s + 1];
    if (end - b > wave_segment) return;  // k_p_forward_long's
    const size_t step = st.step + t;
    p_segment_add(b, end, 1, lid, dstp, match + step * n_labels, w, B + st.table + (size_t)(st.len - t - 1) * S, a,
                  A + ((size_t)st.index * 2 + ((t + 1) & 1)) * S, lab + step * n_labels);
}

// One wavefront per (long state, stream): blocks of 256 lanes take 4 long states. blockIdx.y = stream. Integer sums have no
// order, so the lanes may stride the segment. Reads A_t only: k_p_forward clears it afterwards.
__global__ __launch_bounds__(256) void k_p_forward_long(uint32_t n_long, const uint32_t *long_states, uint32_t S, uint32_t t,
                                                        const BatchStream *streams, const uint32_t *off, const uint32_t *lid, const uint32_t *dstp,
                                                        uint32_t n_labels, const uint8_t *match, const double *w, const double *B, p_u64 *A,
                                                        p_u64 *lab) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const BatchStream st = streams[blockIdx.y];
    if (i >= n_long || t >= st.len) return;
    const uint32_t s = long_states[i];
    const p_u64 a = A[((size_t)st.index * 2 + (t & 1)) * S + s];
    if (!a) return;
    const size_t step = st.step + t;
    p_segment_add(off[s] + lane, off[s + 1], 64, lid, dstp, match + step * n_labels, w, B + st.table + (size_t)(st.len - t - 1) * S, a,
                  A + ((size_t)st.index * 2 + ((t + 1) & 1)) * S, lab + step * n_labels);
}

// final_mass[stream] = the sum of A_len(s) over the final states: blockIdx.y = stream, one lane per state; final_mass zeroed
// by the host beforehand. Every lane of a wavefront stays to the end (the shuffles are wave-wide).
__global__ __launch_bounds__(256) void k_p_final(uint32_t S, const BatchStream *streams, const uint8_t *fin, const p_u64 *A, p_u64 *final_mass) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const BatchStream st = streams[blockIdx.y];
    p_u64 x = s < S && fin[s] ? A[((size_t)st.index * 2 + (st.len & 1)) * S + s] : 0;
    for (int d = 32; d; d >>= 1) x += __shfl_xor(x, d, 64);
    if (lane == 0 && x) atomicAdd(&final_mass[blockIdx.y], x);
}

// lab: [steps][n_labels]; vidx: [n_labels][n_obs]; bin_off: [n_obs] first bin of a variable; bins: [steps][n_bins], zeroed
// by the host beforehand. blockIdx.y strides the steps.
__global__ void k_p_bins(uint32_t n_labels, uint32_t steps, const p_u64 *lab, const uint32_t *vidx, const uint32_t *bin_off, int n_obs,
                         uint32_t n_bins, p_u64 *bins) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_labels) return;
    for (size_t step = blockIdx.y; step < steps; step += gridDim.y) {
        const p_u64 m = lab[step * n_labels + l];
        if (!m) continue;
        p_u64 *row = bins + step * n_bins;
        for (int v = 0; v < n_obs; v++) atomicAdd(&row[bin_off[v] + vidx[(size_t)l * n_obs + v]], m);
    }
}

}  // namespace dev
}  // namespace stcsp
