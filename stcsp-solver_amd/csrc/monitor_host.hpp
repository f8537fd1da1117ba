// monitor_host.hpp -- the host twin of the device stream monitor (dev_monitor.hpp; definition: stcsp_engine.h,
// stcsp_engine_monitor_check), written plainly with ordered containers.
//
// One implementation, used by libstcsp_host.so (stcsp_automaton_check_streams: the checker of the device pass in the
// tests, and the path for automata whose flags live on the host) and by libstcsp_hip.so (the streams whose state set
// outgrows the kernel's capacity are finished here, so the API result is always exact).
#pragma once
#include <cstdint>
#include <map>
#include <set>
#include <utility>
#include <vector>

namespace stcsp {

// The automaton as flat arrays: state 0 is the root; flags as graphTraverse / the adversarial passes left them.
struct MonitorView {
    int n_vars = 0;
    int64_t n_states = 0, n_edges = 0;
    const int64_t *src = nullptr, *dst = nullptr;
    const int32_t *values = nullptr;  // [n_edges * n_vars]
    const uint8_t *valid = nullptr, *final_ = nullptr, *alive = nullptr;
};

struct HostMonitor {
    int n_obs = 0;
    bool root_live = false;
    std::vector<uint8_t> fin;
    std::map<std::vector<int32_t>, int32_t> label_ids;                   // projected label -> id
    std::map<std::pair<int64_t, int32_t>, std::set<int64_t>> transition;  // (state, label id) -> destinations

    // mask: [n_vars], nonzero = observable
    void build(const MonitorView &a, const uint8_t *mask) {
        label_ids.clear();
        transition.clear();
        std::vector<int> obs;
        for (int v = 0; v < a.n_vars; v++)
            if (mask[v]) obs.push_back(v);
        n_obs = (int)obs.size();
        fin.assign(a.final_, a.final_ + a.n_states);
        // the live automaton: valid states the (valid) root reaches over alive edges
        std::vector<uint8_t> live((size_t)a.n_states, 0);
        root_live = a.n_states > 0 && a.valid[0];
        if (!root_live) return;
        std::vector<int64_t> off((size_t)a.n_states + 1, 0), by_src((size_t)a.n_edges);
        for (int64_t e = 0; e < a.n_edges; e++) off[(size_t)a.src[e] + 1]++;
        for (int64_t s = 0; s < a.n_states; s++) off[(size_t)s + 1] += off[(size_t)s];
        {
            std::vector<int64_t> at(off.begin(), off.end() - 1);
            for (int64_t e = 0; e < a.n_edges; e++) by_src[(size_t)at[(size_t)a.src[e]]++] = e;
        }
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
        std::vector<int32_t> proj;
        for (int64_t e = 0; e < a.n_edges; e++) {
            if (!a.alive[e] || !live[(size_t)a.src[e]] || !live[(size_t)a.dst[e]]) continue;
            proj.clear();
            for (int v : obs) proj.push_back(a.values[e * a.n_vars + v]);
            const int32_t l = label_ids.emplace(proj, (int32_t)label_ids.size()).first->second;
            transition[{a.src[e], l}].insert(a.dst[e]);
        }
    }

    // One stream of `len` rows of n_obs values. Returns the largest |S_t| met.
    int64_t check_one(const int32_t *rows, int64_t len, int32_t *accepted_len, int32_t *n_end, uint8_t *end_final) const {
        std::set<int64_t> cur, next;
        if (root_live) cur.insert(0);
        int64_t t = 0, largest = (int64_t)cur.size();
        std::vector<int32_t> row((size_t)n_obs);
        for (; t < len && !cur.empty(); t++) {
            row.assign(rows + t * n_obs, rows + (t + 1) * n_obs);
            const auto l = label_ids.find(row);
            if (l == label_ids.end()) break;
            next.clear();
            for (int64_t s : cur) {
                const auto d = transition.find({s, l->second});
                if (d != transition.end()) next.insert(d->second.begin(), d->second.end());
            }
            if (next.empty()) break;
            cur.swap(next);
            if ((int64_t)cur.size() > largest) largest = (int64_t)cur.size();
        }
        *accepted_len = (int32_t)t;
        *n_end = (int32_t)cur.size();
        *end_final = 0;
        for (int64_t s : cur)
            if (fin[(size_t)s]) *end_final = 1;
        return largest;
    }
};

// offsets: [n_streams + 1], in steps, starting at 0 and not decreasing; every stream shorter than 2^31 steps.
inline bool monitor_offsets_ok(int64_t n_streams, const int64_t *offsets) {
    if (n_streams < 0) return false;
    if (n_streams == 0) return !offsets || offsets[0] == 0;
    if (!offsets || offsets[0] != 0) return false;
    for (int64_t i = 0; i < n_streams; i++)
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 0x7fffffffll) return false;
    return true;
}

}  // namespace stcsp
