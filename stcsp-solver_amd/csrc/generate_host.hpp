// generate_host.hpp -- the host twin of the device stream generator (dev_generate.hpp; definition: stcsp_engine.h,
// stcsp_engine_generate), written plainly: sorted edge lists and vectors of doubles.
//
// One implementation, used by libstcsp_host.so (stcsp_automaton_generate / stcsp_automaton_count_streams: the checker of
// the device pass in the tests, and the path for automata whose flags live on the host) and compiled into
// libstcsp_hip.so beside monitor_host.hpp.
//
// Every floating-point step is one add, one subtract, one multiply or one compare, as the contract has it; there is no
// expression of the shape a * b + c, and contraction is switched off on top of that.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "monitor_host.hpp"

#if defined(__clang__)
#define STCSP_GEN_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define STCSP_GEN_NO_CONTRACT
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace stcsp {

constexpr int kGenEndFinal = 1;  // STCSP_GEN_END_FINAL

inline uint64_t gen_mix(uint64_t x) {  // splitmix64 finaliser
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
inline double gen_uniform(uint64_t seed, uint64_t stream, uint64_t t) {
    STCSP_GEN_NO_CONTRACT
    const uint64_t z = gen_mix(gen_mix(gen_mix(seed + 0x9e3779b97f4a7c15ull) + stream) + t);
    return (double)(z >> 11) * 0x1.0p-53;
}

// A request against count[0 .. horizon]: 0 <= len <= horizon, count[len] > 0, and for an unrank count[len] < 2^53 and every
// rank below it. Shared by the engine and the host twin.
inline bool generate_request_ok(const std::vector<double> &count, int64_t n_streams, int len, const uint64_t *ranks) {
    if (n_streams < 0 || len < 0 || (size_t)len >= count.size() || !(count[(size_t)len] > 0.0)) return false;
    if (ranks) {
        if (!(count[(size_t)len] < 0x1.0p53)) return false;
        for (int64_t i = 0; i < n_streams; i++)
            if (ranks[i] >= (1ull << 53) || !((double)ranks[i] < count[(size_t)len])) return false;
    }
    return true;
}

struct HostGenerator {
    int n_vars = 0, n_obs = 0, horizon = 0;
    bool root_live = false;
    std::vector<int> obs;
    std::vector<uint8_t> fin;
    const int32_t *values = nullptr;
    std::vector<int64_t> off, edge, dest;        // live edges by source in canonical order: off[s] .. off[s + 1]
    std::vector<std::vector<double>> weight;     // [horizon + 1][n_states]
    std::vector<double> count;                   // [horizon + 1]
    int64_t n_live = 0, max_out_degree = 0;

    // mask: [n_vars], nonzero = observable. false if a count is not finite.
    bool build(const MonitorView &a, const uint8_t *mask, int horizon_, int flags) {
        STCSP_GEN_NO_CONTRACT
        n_vars = a.n_vars;
        horizon = horizon_;
        values = a.values;
        obs.clear();
        for (int v = 0; v < a.n_vars; v++)
            if (mask[v]) obs.push_back(v);
        n_obs = (int)obs.size();
        fin.assign(a.final_, a.final_ + a.n_states);
        const size_t S = (size_t)a.n_states;
        // the live automaton: valid states the (valid) root reaches over alive edges
        std::vector<uint8_t> live(S, 0);
        root_live = a.n_states > 0 && a.valid[0];
        std::vector<std::vector<int64_t>> by_src(S);
        for (int64_t e = 0; e < a.n_edges; e++)
            if (a.alive[e] && a.valid[a.dst[e]]) by_src[(size_t)a.src[e]].push_back(e);
        if (root_live) {
            std::vector<int64_t> stack{0};
            live[0] = 1;
            while (!stack.empty()) {
                const int64_t u = stack.back();
                stack.pop_back();
                for (int64_t e : by_src[(size_t)u])
                    if (!live[(size_t)a.dst[e]]) {
                        live[(size_t)a.dst[e]] = 1;
                        stack.push_back(a.dst[e]);
                    }
            }
        }
        const int N = a.n_vars;
        const int32_t *val = a.values;
        off.assign(S + 1, 0);
        edge.clear();
        dest.clear();
        n_live = max_out_degree = 0;
        for (size_t s = 0; s < S; s++) {
            if (live[s]) {
                n_live++;
                std::vector<int64_t> &seg = by_src[s];
                std::sort(seg.begin(), seg.end(), [&](int64_t x, int64_t y) {
                    const int32_t *rx = val + x * N, *ry = val + y * N;
                    if (std::lexicographical_compare(rx, rx + N, ry, ry + N)) return true;
                    if (std::lexicographical_compare(ry, ry + N, rx, rx + N)) return false;
                    return x < y;
                });
                for (int64_t e : seg) {
                    edge.push_back(e);
                    dest.push_back(a.dst[e]);
                }
                max_out_degree = std::max<int64_t>(max_out_degree, (int64_t)seg.size());
            }
            off[s + 1] = (int64_t)edge.size();
        }
        weight.assign((size_t)horizon + 1, std::vector<double>(S, 0.0));
        for (size_t s = 0; s < S; s++)
            if (live[s]) weight[0][s] = (flags & kGenEndFinal) ? (fin[s] ? 1.0 : 0.0) : 1.0;
        for (int t = 0; t < horizon; t++)
            for (size_t s = 0; s < S; s++) {
                double acc = 0.0;
                for (int64_t k = off[s]; k < off[s + 1]; k++) acc = acc + weight[(size_t)t][(size_t)dest[(size_t)k]];
                weight[(size_t)t + 1][s] = acc;
            }
        count.assign((size_t)horizon + 1, 0.0);
        bool finite = true;
        for (int t = 0; t <= horizon; t++) {
            count[(size_t)t] = root_live ? weight[(size_t)t][0] : 0.0;
            finite = finite && std::isfinite(count[(size_t)t]);
        }
        return finite;
    }

    // One stream: rows = [len * n_obs]. With `rank` the rank-th path, else the sample of (seed, stream).
    void generate_one(int len, uint64_t seed, uint64_t stream, const uint64_t *rank, int32_t *rows, uint8_t *end_final) const {
        STCSP_GEN_NO_CONTRACT
        int64_t s = 0;
        double tau = rank ? (double)*rank : 0.0;
        for (int t = 0; t < len; t++) {
            const int r = len - t;
            const std::vector<double> &w_next = weight[(size_t)r - 1];
            if (!rank) tau = gen_uniform(seed, stream, (uint64_t)t) * weight[(size_t)r][(size_t)s];
            double acc = 0.0, before = 0.0, before_last = 0.0;
            int64_t pick = -1, last = -1;
            for (int64_t k = off[(size_t)s]; k < off[(size_t)s + 1]; k++) {
                const double w = w_next[(size_t)dest[(size_t)k]];
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
            if (pick < 0) break;  // (unreachable while count[len] > 0)
            if (rank) tau = tau - before;
            const int32_t *row = values + edge[(size_t)pick] * n_vars;
            for (int i = 0; i < n_obs; i++) rows[(size_t)t * n_obs + i] = row[obs[(size_t)i]];
            s = dest[(size_t)pick];
        }
        *end_final = fin[(size_t)s] ? 1 : 0;
    }
};

}  // namespace stcsp

#if !defined(__clang__)
#pragma GCC pop_options
#endif
