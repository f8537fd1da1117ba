// components_host.hpp -- the host twin of the device component pass (dev_components.hpp; definition: stcsp_engine.h,
// stcsp_engine_components), written plainly: an iterative Tarjan, breadth-first searches and a
// greedy walk. It shares nothing with the device pass but the result struct.
//
// Used by libstcsp_host.so (stcsp_automaton_components: the checker of the device pass in the tests, and the path for
// automata whose flags live on the host: sharded runs, host adversarial passes, read_binary, import_flags).
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "monitor_host.hpp"
#include "stcsp_engine.h"

namespace stcsp {

struct HostComponents {
    int n_vars = 0;
    int64_t n_live = 0, n_cyclic = 0, n_accepting = 0, n_bottom = 0, n_omega = 0;
    int32_t root_omega = 0;
    std::vector<int32_t> state_component, comp_size, comp_depth, comp_flags, lasso_component, lasso_stem_len, lasso_values;
    std::vector<uint8_t> state_omega;
    std::vector<int64_t> lasso_off{0};

    // false: two live out-edges of one state carry the same full row (the automaton is not deterministic)
    bool run(const MonitorView &a, int64_t max_lassos, int32_t flags) {
        const int64_t S = a.n_states, E = a.n_edges;
        const int N = n_vars = a.n_vars;
        state_component.assign((size_t)S, -1);
        state_omega.assign((size_t)S, 0);
        if (S == 0 || !a.valid[0]) return true;
        // out-edges by source, then the live set and the depths by one breadth-first search from the root
        std::vector<int64_t> off((size_t)S + 1, 0), by_src((size_t)E);
        for (int64_t e = 0; e < E; e++) off[(size_t)a.src[e] + 1]++;
        for (int64_t s = 0; s < S; s++) off[(size_t)s + 1] += off[(size_t)s];
        {
            std::vector<int64_t> at(off.begin(), off.end() - 1);
            for (int64_t e = 0; e < E; e++) by_src[(size_t)at[(size_t)a.src[e]]++] = e;
        }
        std::vector<int32_t> depth((size_t)S, -1);
        std::vector<int64_t> order{0};
        depth[0] = 0;
        for (size_t q = 0; q < order.size(); q++) {
            const int64_t u = order[q];
            for (int64_t k = off[(size_t)u]; k < off[(size_t)u + 1]; k++) {
                const int64_t e = by_src[(size_t)k], v = a.dst[e];
                if (a.alive[e] && a.valid[v] && depth[(size_t)v] < 0) {
                    depth[(size_t)v] = depth[(size_t)u] + 1;
                    order.push_back(v);
                }
            }
        }
        n_live = (int64_t)order.size();
        auto live_edge = [&](int64_t e) { return a.alive[e] && depth[(size_t)a.src[e]] >= 0 && depth[(size_t)a.dst[e]] >= 0; };
        // in-edges by destination, live ones only
        std::vector<int64_t> roff((size_t)S + 1, 0), by_dst;
        for (int64_t e = 0; e < E; e++)
            if (live_edge(e)) roff[(size_t)a.dst[e] + 1]++;
        for (int64_t s = 0; s < S; s++) roff[(size_t)s + 1] += roff[(size_t)s];
        by_dst.resize((size_t)roff[(size_t)S]);
        {
            std::vector<int64_t> at(roff.begin(), roff.end() - 1);
            for (int64_t e = 0; e < E; e++)
                if (live_edge(e)) by_dst[(size_t)at[(size_t)a.dst[e]]++] = e;
        }
        // Tarjan, iterative; raw[s] = a member of s's component
        std::vector<int64_t> index((size_t)S, -1), low((size_t)S, 0), raw((size_t)S, -1), stack;
        std::vector<uint8_t> on_stack((size_t)S, 0);
        std::vector<std::pair<int64_t, int64_t>> call;  // (state, next position among its out-edges)
        int64_t counter = 0;
        for (int64_t start : order) {
            if (index[(size_t)start] >= 0) continue;
            call.push_back({start, off[(size_t)start]});
            index[(size_t)start] = low[(size_t)start] = counter++;
            stack.push_back(start);
            on_stack[(size_t)start] = 1;
            while (!call.empty()) {
                const int64_t u = call.back().first;
                int64_t &k = call.back().second;
                bool descended = false;
                while (k < off[(size_t)u + 1]) {
                    const int64_t e = by_src[(size_t)k++];
                    if (!live_edge(e)) continue;
                    const int64_t v = a.dst[e];
                    if (index[(size_t)v] < 0) {
                        index[(size_t)v] = low[(size_t)v] = counter++;
                        stack.push_back(v);
                        on_stack[(size_t)v] = 1;
                        call.push_back({v, off[(size_t)v]});
                        descended = true;
                        break;
                    }
                    if (on_stack[(size_t)v]) low[(size_t)u] = std::min(low[(size_t)u], index[(size_t)v]);
                }
                if (descended) continue;
                if (low[(size_t)u] == index[(size_t)u])
                    for (;;) {
                        const int64_t w = stack.back();
                        stack.pop_back();
                        on_stack[(size_t)w] = 0;
                        raw[(size_t)w] = u;
                        if (w == u) break;
                    }
                call.pop_back();
                if (!call.empty()) low[(size_t)call.back().first] = std::min(low[(size_t)call.back().first], low[(size_t)u]);
            }
        }
        // numbers by least member, then sizes, depths and flags
        std::vector<int32_t> number((size_t)S, -1);
        for (int64_t s = 0; s < S; s++) {
            if (depth[(size_t)s] < 0) continue;
            int32_t &c = number[(size_t)raw[(size_t)s]];
            if (c < 0) {
                c = (int32_t)comp_size.size();
                comp_size.push_back(0);
                comp_depth.push_back(depth[(size_t)s]);
                comp_flags.push_back(STCSP_SCC_BOTTOM);
            }
            state_component[(size_t)s] = c;
            comp_size[(size_t)c]++;
            comp_depth[(size_t)c] = std::min(comp_depth[(size_t)c], depth[(size_t)s]);
            if (a.final_[s]) comp_flags[(size_t)c] |= STCSP_SCC_FINAL;
        }
        for (int64_t e = 0; e < E; e++) {
            if (!live_edge(e)) continue;
            const int32_t cu = state_component[(size_t)a.src[e]], cv = state_component[(size_t)a.dst[e]];
            if (cu == cv)
                comp_flags[(size_t)cu] |= STCSP_SCC_CYCLIC;
            else
                comp_flags[(size_t)cu] &= ~STCSP_SCC_BOTTOM;
        }
        const int32_t accepting = STCSP_SCC_CYCLIC | STCSP_SCC_FINAL;
        for (int32_t &f : comp_flags) {
            if ((f & accepting) == accepting) f |= STCSP_SCC_ACCEPTING;
            n_cyclic += (f & STCSP_SCC_CYCLIC) != 0;
            n_accepting += (f & STCSP_SCC_ACCEPTING) != 0;
            n_bottom += (f & STCSP_SCC_BOTTOM) != 0;
        }
        // omega: backward from the members of the accepting components
        std::vector<int64_t> work;
        for (int64_t s : order)
            if (comp_flags[(size_t)state_component[(size_t)s]] & STCSP_SCC_ACCEPTING) {
                state_omega[(size_t)s] = 1;
                work.push_back(s);
            }
        while (!work.empty()) {
            const int64_t v = work.back();
            work.pop_back();
            for (int64_t k = roff[(size_t)v]; k < roff[(size_t)v + 1]; k++) {
                const int64_t u = a.src[by_dst[(size_t)k]];
                if (!state_omega[(size_t)u]) {
                    state_omega[(size_t)u] = 1;
                    work.push_back(u);
                }
            }
        }
        for (int64_t s : order) n_omega += state_omega[(size_t)s];
        root_omega = state_omega[0];
        if (max_lassos == 0) return true;
        // lassos: the accepting components by (depth, number)
        std::vector<int32_t> wanted;
        for (int32_t c = 0; c < (int32_t)comp_flags.size(); c++)
            if ((comp_flags[(size_t)c] & STCSP_SCC_ACCEPTING) && (!(flags & STCSP_SCC_LASSO_BOTTOM) || (comp_flags[(size_t)c] & STCSP_SCC_BOTTOM)))
                wanted.push_back(c);
        std::stable_sort(wanted.begin(), wanted.end(), [&](int32_t x, int32_t y) { return comp_depth[(size_t)x] < comp_depth[(size_t)y]; });
        if (max_lassos > 0 && (int64_t)wanted.size() > max_lassos) wanted.resize((size_t)max_lassos);
        std::vector<std::vector<int64_t>> members(comp_size.size());
        for (int32_t c : wanted) members[(size_t)c].reserve((size_t)comp_size[(size_t)c]);
        {
            std::vector<uint8_t> is_wanted(comp_size.size(), 0);
            for (int32_t c : wanted) is_wanted[(size_t)c] = 1;
            for (int64_t s = 0; s < S; s++)
                if (state_component[(size_t)s] >= 0 && is_wanted[(size_t)state_component[(size_t)s]]) members[(size_t)state_component[(size_t)s]].push_back(s);
        }
        std::vector<int64_t> stamp((size_t)S, -1), dist((size_t)S, 0);
        int64_t tick = 0;
        bool deterministic = true;
        // the live out-edge of u with the least full row among those whose destination `ok` admits; -1 when there is none
        auto least_edge = [&](int64_t u, auto &&ok) {
            int64_t best = -1;
            for (int64_t k = off[(size_t)u]; k < off[(size_t)u + 1]; k++) {
                const int64_t e = by_src[(size_t)k];
                if (!live_edge(e) || !ok(a.dst[e])) continue;
                if (best < 0) {
                    best = e;
                    continue;
                }
                const int32_t *x = a.values + e * N, *y = a.values + best * N;
                if (std::equal(x, x + N, y)) deterministic = false;
                if (std::lexicographical_compare(x, x + N, y, y + N)) best = e;
            }
            return best;
        };
        for (int32_t c : wanted) {
            // stem: the states on a shortest path from the root to a final member of least depth
            int32_t len = -1;
            for (int64_t s : members[(size_t)c])
                if (a.final_[s] && (len < 0 || depth[(size_t)s] < len)) len = depth[(size_t)s];
            tick++;
            work.clear();
            for (int64_t s : members[(size_t)c])
                if (a.final_[s] && depth[(size_t)s] == len) {
                    stamp[(size_t)s] = tick;
                    work.push_back(s);
                }
            while (!work.empty()) {
                const int64_t v = work.back();
                work.pop_back();
                for (int64_t k = roff[(size_t)v]; k < roff[(size_t)v + 1]; k++) {
                    const int64_t u = a.src[by_dst[(size_t)k]];
                    if (depth[(size_t)u] + 1 == depth[(size_t)v] && stamp[(size_t)u] != tick) {
                        stamp[(size_t)u] = tick;
                        work.push_back(u);
                    }
                }
            }
            int64_t u = 0;
            for (int32_t t = 0; t < len; t++) {
                const int64_t e = least_edge(u, [&](int64_t v) { return depth[(size_t)v] == t + 1 && stamp[(size_t)v] == tick; });
                if (e < 0 || !deterministic) return false;
                lasso_values.insert(lasso_values.end(), a.values + e * N, a.values + (e + 1) * N);
                u = a.dst[e];
            }
            const int64_t anchor = u;
            // loop: distances to the anchor inside the component, breadth-first and backward
            tick++;
            std::vector<int64_t> queue{anchor};
            stamp[(size_t)anchor] = tick;
            dist[(size_t)anchor] = 0;
            for (size_t q = 0; q < queue.size(); q++) {
                const int64_t v = queue[q];
                for (int64_t k = roff[(size_t)v]; k < roff[(size_t)v + 1]; k++) {
                    const int64_t w = a.src[by_dst[(size_t)k]];
                    if (state_component[(size_t)w] == c && stamp[(size_t)w] != tick) {
                        stamp[(size_t)w] = tick;
                        dist[(size_t)w] = dist[(size_t)v] + 1;
                        queue.push_back(w);
                    }
                }
            }
            int64_t loop_len = -1;
            for (int64_t k = off[(size_t)anchor]; k < off[(size_t)anchor + 1]; k++) {
                const int64_t e = by_src[(size_t)k], v = a.dst[e];
                if (live_edge(e) && state_component[(size_t)v] == c && (loop_len < 0 || dist[(size_t)v] + 1 < loop_len)) loop_len = dist[(size_t)v] + 1;
            }
            if (loop_len < 1) return false;  // (an accepting component is cyclic)
            for (int64_t rem = loop_len; rem > 0; rem--) {
                const int64_t e = least_edge(u, [&](int64_t v) { return state_component[(size_t)v] == c && dist[(size_t)v] == rem - 1; });
                if (e < 0 || !deterministic) return false;
                lasso_values.insert(lasso_values.end(), a.values + e * N, a.values + (e + 1) * N);
                u = a.dst[e];
            }
            if (u != anchor) return false;
            lasso_component.push_back(c);
            lasso_stem_len.push_back(len);
            lasso_off.push_back(lasso_off.back() + len + loop_len);
        }
        return true;
    }
};

}  // namespace stcsp
