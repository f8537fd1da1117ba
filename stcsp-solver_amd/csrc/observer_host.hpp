// observer_host.hpp -- the host twin of the device observer (dev_observer.hpp; definition: stcsp_engine.h,
// stcsp_engine_observer), written plainly with ordered containers.
//
// Used by libstcsp_host.so (stcsp_automaton_observer: the checker of the device pass in the tests, and the path for
// automata whose flags live on the host: sharded runs, host adversarial passes, read_binary).
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <set>
#include <vector>

#include "monitor_host.hpp"

namespace stcsp {

struct HostObserver {
    int n_obs = 0;
    int32_t levels = 0;
    int64_t n_labels = 0, max_set = 0;
    std::vector<int64_t> member_off{0};
    std::vector<int32_t> member, edge_src, edge_dst, edge_values;
    std::vector<uint8_t> state_final;

    int64_t n_states() const { return (int64_t)member_off.size() - 1; }
    int64_t n_edges() const { return (int64_t)edge_src.size(); }

    // mask: [n_vars], nonzero = observable. false: more than max_states sets (the members are then a partial result, not to be used).
    bool build(const MonitorView &a, const uint8_t *mask, int64_t max_states) {
        typedef std::vector<int32_t> Label;
        typedef std::vector<int64_t> Set;  // ascending
        HostMonitor mon;                   // the live automaton, the label ids and (state, label id) -> destinations
        mon.build(a, mask);
        n_obs = mon.n_obs;
        n_labels = (int64_t)mon.label_ids.size();
        if (!mon.root_live) return true;
        std::vector<const Label *> label_of((size_t)n_labels);
        for (const auto &kv : mon.label_ids) label_of[(size_t)kv.second] = &kv.first;
        std::map<int64_t, std::vector<std::pair<int32_t, const std::set<int64_t> *>>> out;  // state -> (label id, destinations)
        for (const auto &kv : mon.transition) out[kv.first.first].push_back({kv.first.second, &kv.second});
        std::map<Set, int32_t> number;
        std::vector<const Set *> order;
        std::vector<int32_t> depth;
        auto intern = [&](const Set &s, int32_t d) {
            const auto it = number.emplace(s, (int32_t)number.size());
            if (it.second) {
                order.push_back(&it.first->first);
                depth.push_back(d);
            }
            return it.first->second;
        };
        intern(Set{0}, 0);
        for (size_t q = 0; q < order.size(); q++) {  // breadth-first; the out-edges of a set in the order of their projected rows
            const Set &D = *order[q];
            std::map<Label, std::set<int64_t>> succ;
            for (int64_t s : D) {
                const auto o = out.find(s);
                if (o == out.end()) continue;
                for (const auto &ld : o->second) succ[*label_of[(size_t)ld.first]].insert(ld.second->begin(), ld.second->end());
            }
            for (const auto &kv : succ) {
                const int32_t d = intern(Set(kv.second.begin(), kv.second.end()), depth[q] + 1);
                if ((int64_t)number.size() > max_states) return false;
                edge_src.push_back((int32_t)q);
                edge_dst.push_back(d);
                edge_values.insert(edge_values.end(), kv.first.begin(), kv.first.end());
            }
        }
        for (size_t q = 0; q < order.size(); q++) {
            const Set &D = *order[q];
            uint8_t fin = 0;
            for (int64_t s : D) {
                member.push_back((int32_t)s);
                fin |= mon.fin[(size_t)s] ? 1 : 0;
            }
            member_off.push_back((int64_t)member.size());
            state_final.push_back(fin);
            max_set = std::max<int64_t>(max_set, (int64_t)D.size());
            levels = std::max(levels, depth[q] + 1);
        }
        return true;
    }
};

}  // namespace stcsp
