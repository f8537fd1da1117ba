// posterior_host.hpp -- the host twin of the device posterior marginals (dev_posterior.hpp; definition: stcsp_engine.h,
// stcsp_engine_posterior), written plainly: the sorted edge lists of generate_host.hpp, one weight
// per edge, one vector of doubles per backward level, a vector of uint64 forward, the match taken from the rows themselves.
//
// One implementation, used by libstcsp_host.so (stcsp_automaton_posterior_streams: the checker of the device pass in the
// tests, and the path for automata whose flags live on the host) and compiled into libstcsp_hip.so, which shares the
// request checks.
//
// Every floating-point step is one multiply, one add or one compare, as in generate_host.hpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "infer_host.hpp"

#if !defined(__clang__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace stcsp {

constexpr int kPosteriorEndFinal = 1;  // STCSP_POSTERIOR_END_FINAL

// Offsets as the monitor takes them; the weights all absent, or a CSR over the n_obs variables with values strictly
// increasing inside a variable and no negative weight. Shared by the engine and the host twin.
inline bool posterior_request_ok(int64_t n_streams, const int64_t *offsets, int n_obs, const int64_t *weight_off, const int32_t *weight_val,
                                 const int32_t *weight_w) {
    if (!monitor_offsets_ok(n_streams, offsets)) return false;
    if (!weight_off) return !weight_val && !weight_w;
    if (weight_off[0] != 0) return false;
    for (int v = 0; v < n_obs; v++)
        if (weight_off[v + 1] < weight_off[v]) return false;
    if (weight_off[n_obs] > 0 && (!weight_val || !weight_w)) return false;
    for (int v = 0; v < n_obs; v++)
        for (int64_t k = weight_off[v]; k < weight_off[v + 1]; k++) {
            if (weight_w[k] < 0) return false;
            if (k > weight_off[v] && weight_val[k] <= weight_val[k - 1]) return false;
        }
    return true;
}

// The weight of value x of observable variable v: the listed one, else 1.
inline double posterior_value_weight(int v, int32_t x, const int64_t *weight_off, const int32_t *weight_val, const int32_t *weight_w) {
    if (!weight_off) return 1.0;
    const int32_t *b = weight_val + weight_off[v], *e = weight_val + weight_off[v + 1];
    const int32_t *p = std::lower_bound(b, e, x);
    return p != e && *p == x ? (double)weight_w[p - weight_val] : 1.0;
}

struct HostPosterior {
    HostInfer inf;
    std::vector<double> w;  // per position of the sorted edge lists

    void build(const MonitorView &a, const uint8_t *mask, const int64_t *weight_off, const int32_t *weight_val, const int32_t *weight_w) {
        STCSP_GEN_NO_CONTRACT
        inf.build(a, mask);
        const HostGenerator &g = inf.gen;
        w.assign(g.edge.size(), 1.0);
        for (size_t k = 0; k < g.edge.size(); k++) {
            const int32_t *row = g.values + g.edge[k] * g.n_vars;
            double acc = 1.0;
            for (int i = 0; i < g.n_obs; i++) acc = acc * posterior_value_weight(i, row[g.obs[(size_t)i]], weight_off, weight_val, weight_w);
            w[k] = acc;
        }
    }

    // One stream, the first half: B[r][s] for r = 0 .. len, and the mass.
    double backward(const int32_t *rows, int64_t len, int flags, std::vector<std::vector<double>> &B) const {
        STCSP_GEN_NO_CONTRACT
        const HostGenerator &g = inf.gen;
        const size_t S = g.fin.size();
        const int n_obs = g.n_obs, N = g.n_vars;
        B.assign((size_t)len + 1, std::vector<double>(S, 0.0));
        for (size_t s = 0; s < S; s++)
            if (g.weight[0][s] > 0.0 && (!(flags & kPosteriorEndFinal) || g.fin[s])) B[0][s] = 1.0;
        for (int64_t r = 1; r <= len; r++) {
            const int32_t *x = rows + (len - r) * n_obs;
            const std::vector<double> &prev = B[(size_t)r - 1];
            for (size_t s = 0; s < S; s++) {
                double acc = 0.0;
                for (int64_t k = g.off[s]; k < g.off[s + 1]; k++) {
                    if (!inf.matches(g.values + g.edge[(size_t)k] * N, x)) continue;
                    const double wk = w[(size_t)k], b = prev[(size_t)g.dest[(size_t)k]];
                    if (!(wk > 0.0) || !(b > 0.0)) continue;
                    const double term = wk * b;
                    acc = acc + term;
                }
                B[(size_t)r][s] = acc;
            }
        }
        return g.root_live ? B[(size_t)len][0] : 0.0;
    }

    // The second half, for an exact stream (mass < 2^53): marg[t * n_obs + v] = the sorted (value, mass) pairs; returns
    // final_mass. Everything is an integer below 2^53.
    uint64_t forward(const int32_t *rows, int64_t len, const std::vector<std::vector<double>> &B, double mass,
                     std::vector<std::vector<std::pair<int32_t, uint64_t>>> &marg) const {
        const HostGenerator &g = inf.gen;
        const size_t S = g.fin.size();
        const int n_obs = g.n_obs, N = g.n_vars;
        marg.assign((size_t)len * (size_t)n_obs, std::vector<std::pair<int32_t, uint64_t>>());
        std::vector<uint64_t> A(S, 0), next(S, 0);
        if (mass > 0.0) A[0] = 1;
        for (int64_t t = 0; t < len; t++) {
            std::fill(next.begin(), next.end(), 0);
            const int32_t *x = rows + t * n_obs;
            const std::vector<double> &togo = B[(size_t)(len - t - 1)];
            for (size_t s = 0; s < S; s++) {
                if (!A[s]) continue;
                for (int64_t k = g.off[s]; k < g.off[s + 1]; k++) {
                    const int32_t *row = g.values + g.edge[(size_t)k] * N;
                    const size_t d = (size_t)g.dest[(size_t)k];
                    if (!inf.matches(row, x) || !(w[(size_t)k] > 0.0) || !(togo[d] > 0.0)) continue;
                    const uint64_t aw = A[s] * (uint64_t)w[(size_t)k];
                    next[d] += aw;
                    const uint64_t m = aw * (uint64_t)togo[d];
                    for (int i = 0; i < n_obs; i++) marg[(size_t)t * n_obs + i].push_back({row[g.obs[(size_t)i]], m});
                }
            }
            for (int i = 0; i < n_obs; i++) {
                std::vector<std::pair<int32_t, uint64_t>> &v = marg[(size_t)t * n_obs + i];
                std::sort(v.begin(), v.end());
                size_t n = 0;
                for (size_t k = 0; k < v.size(); k++)
                    if (n && v[n - 1].first == v[k].first)
                        v[n - 1].second += v[k].second;
                    else
                        v[n++] = v[k];
                v.resize(n);
            }
            A.swap(next);
        }
        uint64_t fm = 0;
        for (size_t s = 0; s < S; s++)
            if (g.fin[s]) fm += A[s];
        return fm;
    }
};

}  // namespace stcsp

#if !defined(__clang__)
#pragma GCC pop_options
#endif
