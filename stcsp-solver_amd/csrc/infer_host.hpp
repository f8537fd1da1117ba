// infer_host.hpp -- the host twin of the device stream inference (dev_infer.hpp; definition: stcsp_engine.h,
// stcsp_engine_infer), written plainly: the sorted edge lists of generate_host.hpp, one vector of
// doubles per level, the match taken from the rows themselves.
//
// One implementation, used by libstcsp_host.so (stcsp_automaton_infer_streams: the checker of the device pass in the
// tests, and the path for automata whose flags live on the host) and compiled into libstcsp_hip.so, which shares the
// request checks.
//
// Every floating-point step is one add, one subtract, one multiply or one compare, as in generate_host.hpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "generate_host.hpp"
#include "monitor_host.hpp"

#if !defined(__clang__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace stcsp {

constexpr int kInferEndFinal = 1;                                       // STCSP_INFER_END_FINAL
constexpr int32_t kInferMissing = std::numeric_limits<int32_t>::min();  // STCSP_INFER_MISSING

// Offsets as the monitor takes them and draws >= 0. Shared by the engine and the host twin.
inline bool infer_request_ok(int64_t n_streams, const int64_t *offsets, int32_t draws) { return draws >= 0 && monitor_offsets_ok(n_streams, offsets); }

// The draws of one feasible stream: 0 = fine, 1 = its count is not finite (STCSP_E_UNSUPPORTED), 2 = an unrank against a
// count of 2^53 or more or a rank that is not below the count (STCSP_E_INVALID). ranks: the stream's, or NULL.
inline int infer_draws_ok(double count, int32_t draws, const uint64_t *ranks) {
    if (draws <= 0 || !(count > 0.0)) return 0;
    if (!std::isfinite(count)) return 1;
    if (ranks) {
        if (!(count < 0x1.0p53)) return 2;
        for (int32_t j = 0; j < draws; j++)
            if (ranks[j] >= (1ull << 53) || !((double)ranks[j] < count)) return 2;
    }
    return 0;
}

struct HostInfer {
    HostGenerator gen;  // horizon 0: the canonical order, and weight[0][s] = 1 exactly for the live states

    void build(const MonitorView &a, const uint8_t *mask) { gen.build(a, mask, 0, 0); }

    bool matches(const int32_t *row, const int32_t *x) const {
        for (int i = 0; i < gen.n_obs; i++)
            if (x[i] != kInferMissing && row[gen.obs[(size_t)i]] != x[i]) return false;
        return true;
    }

    // One stream, the first half: B[r][s] for r = 0 .. len, and the count.
    double backward(const int32_t *rows, int64_t len, int flags, std::vector<std::vector<double>> &B) const {
        STCSP_GEN_NO_CONTRACT
        const size_t S = gen.fin.size();
        const int n_obs = gen.n_obs, N = gen.n_vars;
        B.assign((size_t)len + 1, std::vector<double>(S, 0.0));
        for (size_t s = 0; s < S; s++)
            if (gen.weight[0][s] > 0.0 && (!(flags & kInferEndFinal) || gen.fin[s])) B[0][s] = 1.0;
        for (int64_t r = 1; r <= len; r++) {
            const int32_t *x = rows + (len - r) * n_obs;
            const std::vector<double> &prev = B[(size_t)r - 1];
            for (size_t s = 0; s < S; s++) {
                double acc = 0.0;
                for (int64_t k = gen.off[s]; k < gen.off[s + 1]; k++)
                    if (matches(gen.values + gen.edge[(size_t)k] * N, x)) acc = acc + prev[(size_t)gen.dest[(size_t)k]];
                B[(size_t)r][s] = acc;
            }
        }
        return gen.root_live ? B[(size_t)len][0] : 0.0;
    }

    // The second half: support[t * n_obs + v] = the sorted distinct values, n_states[0 .. len] = |F_t|.
    void forward(const int32_t *rows, int64_t len, const std::vector<std::vector<double>> &B, double count,
                 std::vector<std::vector<int32_t>> &support, int32_t *n_states) const {
        const size_t S = gen.fin.size();
        const int n_obs = gen.n_obs, N = gen.n_vars;
        support.assign((size_t)len * (size_t)n_obs, std::vector<int32_t>());
        std::vector<uint8_t> F(S, 0), next(S, 0);
        if (count > 0.0) F[0] = 1;
        for (int64_t t = 0; t <= len; t++) {
            int32_t n = 0;
            for (size_t s = 0; s < S; s++) n += F[s];
            n_states[t] = n;
            if (t == len) break;
            std::fill(next.begin(), next.end(), 0);
            const int32_t *x = rows + t * n_obs;
            const std::vector<double> &togo = B[(size_t)(len - t - 1)];
            for (size_t s = 0; s < S; s++) {
                if (!F[s]) continue;
                for (int64_t k = gen.off[s]; k < gen.off[s + 1]; k++) {
                    const int32_t *row = gen.values + gen.edge[(size_t)k] * N;
                    const size_t d = (size_t)gen.dest[(size_t)k];
                    if (!matches(row, x) || !(togo[d] > 0.0)) continue;
                    next[d] = 1;
                    for (int i = 0; i < n_obs; i++) support[(size_t)t * n_obs + i].push_back(row[gen.obs[(size_t)i]]);
                }
            }
            for (int i = 0; i < n_obs; i++) {
                std::vector<int32_t> &v = support[(size_t)t * n_obs + i];
                std::sort(v.begin(), v.end());
                v.erase(std::unique(v.begin(), v.end()), v.end());
            }
            F.swap(next);
        }
    }

    // One draw of a feasible stream of finite count: out = [len * n_obs]. With `rank` the rank-th consistent path, else the
    // sample of (seed, q). false: a state with weight to go and no matching edge of non-zero weight (unreachable).
    bool walk(const int32_t *rows, int64_t len, const std::vector<std::vector<double>> &B, uint64_t seed, uint64_t q, const uint64_t *rank,
              int32_t *out, uint8_t *end_final) const {
        STCSP_GEN_NO_CONTRACT
        const int n_obs = gen.n_obs, N = gen.n_vars;
        int64_t s = 0;
        double tau = rank ? (double)*rank : 0.0;
        for (int64_t t = 0; t < len; t++) {
            const int64_t r = len - t;
            const std::vector<double> &next = B[(size_t)r - 1];
            const int32_t *x = rows + t * n_obs;
            if (!rank) tau = gen_uniform(seed, q, (uint64_t)t) * B[(size_t)r][(size_t)s];
            double acc = 0.0, before = 0.0, before_last = 0.0;
            int64_t pick = -1, last = -1;
            for (int64_t k = gen.off[(size_t)s]; k < gen.off[(size_t)s + 1]; k++) {
                if (!matches(gen.values + gen.edge[(size_t)k] * N, x)) continue;
                const double w = next[(size_t)gen.dest[(size_t)k]];
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
            if (pick < 0) {
                pick = last;
                before = before_last;
            }
            if (pick < 0) return false;
            if (rank) tau = tau - before;
            const int32_t *row = gen.values + gen.edge[(size_t)pick] * N;
            for (int i = 0; i < n_obs; i++) out[t * n_obs + i] = row[gen.obs[(size_t)i]];
            s = gen.dest[(size_t)pick];
        }
        *end_final = gen.fin[(size_t)s] ? 1 : 0;
        return true;
    }
};

}  // namespace stcsp

#if !defined(__clang__)
#pragma GCC pop_options
#endif
