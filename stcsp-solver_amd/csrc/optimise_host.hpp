// optimise_host.hpp -- the host twin of the device optimisation pass (dev_optimise.hpp; definition: stcsp_engine.h,
// stcsp_engine_optimise), written plainly: the same dynamic programme over the live edges, the same
// greedy walk, and a textbook Karp per component with the full table. It shares nothing with the device pass but the
// result struct.
//
// Used by libstcsp_host.so (stcsp_automaton_optimise: the checker of the device pass in the tests, and the path for
// automata whose flags live on the host: merged sharded runs, host adversarial passes, read_binary, import_flags).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "components_host.hpp"
#include "monitor_host.hpp"
#include "stcsp_engine.h"

namespace stcsp {

struct HostOptimise {
    int n_vars = 0;
    int64_t n_live = 0, omega_num = 0, omega_den = 0;
    int32_t omega_component = -1, largest_cyclic = 0;
    std::vector<int64_t> best, state_best, witness_off{0}, comp_num, comp_den;
    std::vector<int32_t> witness_values, witness_states, state_component;

    // STCSP_OK or the error of the contract. lb / ub: [n_vars] the variables' bounds.
    int run(const MonitorView &a, const int *lb, const int *ub, const stcsp_optimise_request &rq) {
        const int64_t S = a.n_states, E = a.n_edges;
        const int N = n_vars = a.n_vars;
        const int32_t horizon = rq.horizon, flags = rq.flags;
        if (!rq.weights || horizon < 0 || rq.n_lengths < 0 || (rq.n_lengths > 0 && !rq.lengths)) return STCSP_E_INVALID;
        for (int32_t i = 0; i < rq.n_lengths; i++)
            if (rq.lengths[i] < 0 || rq.lengths[i] > horizon) return STCSP_E_INVALID;
        const __int128 limit = (__int128)1 << 62;
        __int128 cmax = 0;
        for (int x = 0; x < N; x++)
            cmax += (__int128)std::llabs((long long)rq.weights[x]) * std::max(std::llabs((long long)lb[x]), std::llabs((long long)ub[x]));
        if (cmax * std::max(horizon, 1) > limit) return STCSP_E_INVALID;
        const bool maximise = flags & STCSP_OPT_MAXIMISE;
        std::vector<int64_t> w(rq.weights, rq.weights + N);
        if (maximise)
            for (int64_t &x : w) x = -x;
        // the live automaton and its edges by source, each with its cost
        std::vector<uint8_t> live((size_t)S, 0);
        std::vector<int64_t> off((size_t)S + 1, 0), by_src((size_t)E), cost((size_t)E, 0);
        for (int64_t e = 0; e < E; e++) off[(size_t)a.src[e] + 1]++;
        for (int64_t s = 0; s < S; s++) off[(size_t)s + 1] += off[(size_t)s];
        {
            std::vector<int64_t> at(off.begin(), off.end() - 1);
            for (int64_t e = 0; e < E; e++) by_src[(size_t)at[(size_t)a.src[e]]++] = e;
        }
        if (S > 0 && a.valid[0]) {
            std::vector<int64_t> stack{0};
            live[0] = 1;
            while (!stack.empty()) {
                const int64_t u = stack.back();
                stack.pop_back();
                for (int64_t k = off[(size_t)u]; k < off[(size_t)u + 1]; k++) {
                    const int64_t e = by_src[(size_t)k], v = a.dst[e];
                    if (a.alive[e] && a.valid[v] && !live[(size_t)v]) {
                        live[(size_t)v] = 1;
                        stack.push_back(v);
                    }
                }
            }
        }
        n_live = std::count(live.begin(), live.end(), 1);
        auto live_edge = [&](int64_t e) { return a.alive[e] && live[(size_t)a.src[e]] && live[(size_t)a.dst[e]]; };
        for (int64_t e = 0; e < E; e++)
            for (int x = 0; x < N; x++) cost[(size_t)e] += w[(size_t)x] * (int64_t)a.values[e * N + x];
        // finite horizon: V[k][s] = the least cost of k live edges from s (to a final state under END_FINAL)
        const int64_t none = STCSP_OPT_NONE;
        const bool witnesses = rq.n_lengths > 0;
        std::vector<std::vector<int64_t>> V(witnesses ? (size_t)horizon + 1 : 2, std::vector<int64_t>((size_t)S, none));
        auto row = [&](int32_t k) -> std::vector<int64_t> & { return V[witnesses ? (size_t)k : (size_t)(k % 2)]; };
        best.assign((size_t)horizon + 1, none);
        for (int64_t s = 0; s < S; s++)
            if (live[(size_t)s] && (!(flags & STCSP_OPT_END_FINAL) || a.final_[s])) row(0)[(size_t)s] = 0;
        if (S > 0) best[0] = row(0)[0];
        for (int32_t k = 1; k <= horizon; k++) {
            std::vector<int64_t> &cur = row(k);
            const std::vector<int64_t> &prev = row(k - 1);
            std::fill(cur.begin(), cur.end(), none);
            for (int64_t e = 0; e < E; e++) {
                if (!live_edge(e) || prev[(size_t)a.dst[e]] == none) continue;
                cur[(size_t)a.src[e]] = std::min(cur[(size_t)a.src[e]], cost[(size_t)e] + prev[(size_t)a.dst[e]]);
            }
            best[(size_t)k] = cur[0];
        }
        if (flags & STCSP_OPT_STATE_BEST) state_best = row(horizon);
        // witnesses: the greedy walk, the least full row among the tight edges
        for (int32_t i = 0; i < rq.n_lengths; i++) {
            const int32_t len = rq.lengths[i];
            if (best[(size_t)len] == none) {
                witness_off.push_back(witness_off.back());
                continue;
            }
            int64_t u = 0;
            for (int32_t left = len; left > 0; left--) {
                int64_t pick = -1;
                for (int64_t k = off[(size_t)u]; k < off[(size_t)u + 1]; k++) {
                    const int64_t e = by_src[(size_t)k], below = row(left - 1)[(size_t)a.dst[e]];
                    if (!live_edge(e) || below == none || cost[(size_t)e] + below != row(left)[(size_t)u]) continue;
                    if (pick < 0) {
                        pick = e;
                        continue;
                    }
                    const int32_t *x = a.values + e * N, *y = a.values + pick * N;
                    if (std::equal(x, x + N, y)) return STCSP_E_INTERNAL;
                    if (std::lexicographical_compare(x, x + N, y, y + N)) pick = e;
                }
                if (pick < 0) return STCSP_E_INTERNAL;
                witness_values.insert(witness_values.end(), a.values + pick * N, a.values + (pick + 1) * N);
                u = a.dst[pick];
                witness_states.push_back((int32_t)u);
            }
            witness_off.push_back(witness_off.back() + len);
        }
        // long run: Karp's minimum cycle mean per cyclic component, with the full table
        if (flags & STCSP_OPT_MEAN) {
            HostComponents hc;
            if (!hc.run(a, 0, 0)) return STCSP_E_INTERNAL;
            state_component = hc.state_component;
            const size_t n_comp = hc.comp_size.size();
            comp_num.assign(n_comp, 0);
            comp_den.assign(n_comp, 0);
            std::vector<std::vector<int64_t>> members(n_comp);
            for (int64_t s = 0; s < S; s++)
                if (state_component[(size_t)s] >= 0) members[(size_t)state_component[(size_t)s]].push_back(s);
            for (size_t c = 0; c < n_comp; c++)
                if (hc.comp_flags[c] & STCSP_SCC_CYCLIC) largest_cyclic = std::max(largest_cyclic, hc.comp_size[c]);
            if ((__int128)largest_cyclic * largest_cyclic * cmax > limit) return STCSP_E_UNSUPPORTED;
            std::vector<int64_t> local((size_t)S, -1);
            for (size_t c = 0; c < n_comp; c++) {
                if (!(hc.comp_flags[c] & STCSP_SCC_CYCLIC)) continue;
                const std::vector<int64_t> &ms = members[c];
                const size_t n = ms.size();
                for (size_t i = 0; i < n; i++) local[(size_t)ms[i]] = (int64_t)i;
                std::vector<int64_t> D((n + 1) * n, none);  // D[k * n + i]: the least cost of k edges from the least member to member i
                D[0] = 0;
                for (size_t k = 1; k <= n; k++)
                    for (size_t i = 0; i < n; i++) {
                        if (D[(k - 1) * n + i] == none) continue;
                        const int64_t u = ms[i];
                        for (int64_t p = off[(size_t)u]; p < off[(size_t)u + 1]; p++) {
                            const int64_t e = by_src[(size_t)p], v = a.dst[e];
                            if (!live_edge(e) || state_component[(size_t)v] != (int32_t)c) continue;
                            int64_t &d = D[k * n + (size_t)local[(size_t)v]];
                            d = std::min(d, D[(k - 1) * n + i] + cost[(size_t)e]);
                        }
                    }
                bool have = false;
                int64_t bp = 0, bq = 1;
                for (size_t i = 0; i < n; i++) {
                    if (D[n * n + i] == none) continue;
                    bool any = false;
                    int64_t mp = 0, mq = 1;  // the greatest (D_n - D_k) / (n - k)
                    for (size_t k = 0; k < n; k++) {
                        if (D[k * n + i] == none) continue;
                        const int64_t p = D[n * n + i] - D[k * n + i], q = (int64_t)(n - k);
                        if (!any || (__int128)p * mq > (__int128)mp * q) mp = p, mq = q;
                        any = true;
                    }
                    if (any && (!have || (__int128)mp * bq < (__int128)bp * mq)) bp = mp, bq = mq;
                    have = have || any;
                }
                if (!have) return STCSP_E_INTERNAL;
                int64_t x = std::llabs(bp), y = bq;
                while (y) {
                    const int64_t r = x % y;
                    x = y;
                    y = r;
                }
                comp_num[c] = bp / x;
                comp_den[c] = bq / x;
            }
            for (size_t c = 0; c < n_comp; c++) {
                if (!(hc.comp_flags[c] & STCSP_SCC_ACCEPTING)) continue;
                if (omega_component < 0 || (__int128)comp_num[c] * omega_den < (__int128)omega_num * comp_den[c]) {
                    omega_num = comp_num[c];
                    omega_den = comp_den[c];
                    omega_component = (int32_t)c;
                }
            }
        }
        if (maximise) {
            for (int64_t &x : best)
                if (x != none) x = -x;
            for (int64_t &x : state_best)
                if (x != none) x = -x;
            for (int64_t &x : comp_num) x = -x;
            omega_num = -omega_num;
        }
        return STCSP_OK;
    }
};

}  // namespace stcsp
