// compare_host.hpp -- comparing two observable languages on the host (definition: stcsp_engine.h, stcsp_engine_compare;
// DESIGN.md section 4.17).
//
// HostComparison is the host twin of the device pass (dev_compare.hpp), written plainly with ordered containers over two
// stcsp_observer_results: the checker of the device pass in the tests, and the road for sharded runs, host adversarial passes
// and automata read from binary files (libstcsp_host.so: stcsp_compare_observers). CompareOperand and merge_rows are what the
// device pass takes from the host: an operand as CSR by source over its sorted distinct rows, and the common ranks of two
// operands' rows. The twin uses neither.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "stcsp_engine.h"

namespace stcsp {

// What is wrong with a deterministic automaton given in the layout of stcsp_observer_result (n_states, n_edges, state_final,
// edge_src, edge_dst, edge_values, n_observable), or nullptr
inline const char *compare_operand_fault(const stcsp_observer_result &o) {
    if (o.n_states < 0 || o.n_edges < 0 || o.n_observable < 0) return "has a negative size";
    if (o.n_states > 0x7ffffffell || o.n_edges > 0x7ffffffell) return "has more than 2^31 - 2 states or edges";
    if (o.n_states && !o.state_final) return "has states and no state_final";
    if (o.n_edges && (!o.edge_src || !o.edge_dst || (o.n_observable && !o.edge_values))) return "has edges and no edge arrays";
    const size_t w = (size_t)o.n_observable;
    for (int64_t e = 0; e < o.n_edges; e++) {
        if (o.edge_src[e] < 0 || o.edge_src[e] >= o.n_states || o.edge_dst[e] < 0 || o.edge_dst[e] >= o.n_states) return "has an edge whose state index is out of range";
        if (!e) continue;
        if (o.edge_src[e - 1] > o.edge_src[e]) return "has edges that are not sorted by (source, row)";
        if (o.edge_src[e - 1] < o.edge_src[e]) continue;
        const int32_t *a = o.edge_values + (size_t)(e - 1) * w, *b = a + w;
        if (std::lexicographical_compare(b, b + w, a, a + w)) return "has edges that are not sorted by (source, row)";
        if (std::equal(a, a + w, b)) return "has two edges with one (source, row)";
    }
    return nullptr;
}

// A deterministic automaton as the device pass wants it: CSR by source with a sink behind the last state, labels as indices into
// its sorted distinct rows
struct CompareOperand {
    int n_obs = 0;
    uint32_t n_states = 0, n_rows = 0;
    std::vector<uint32_t> off{0, 0}, lab, dst;  // off: [n_states + 2], the sink's segment is empty
    std::vector<uint8_t> fin{0};                // [n_states + 1], the sink is not final
    std::vector<int32_t> rows;                  // [n_rows][n_obs], sorted

    void clear() { *this = CompareOperand(); }
    // states and edges sorted by (source, label); lab_of(e) = the edge's index into the rows given afterwards
    template <typename SrcFn, typename LabFn, typename DstFn>
    void set_graph(int n_observable, size_t states, const uint8_t *final_flags, size_t edges, SrcFn src_of, LabFn lab_of, DstFn dst_of) {
        n_obs = n_observable;
        n_states = (uint32_t)states;
        off.assign(states + 2, 0);
        fin.assign(states + 1, 0);
        std::copy(final_flags, final_flags + states, fin.begin());
        lab.resize(edges);
        dst.resize(edges);
        for (size_t e = 0; e < edges; e++) {
            off[(size_t)src_of(e) + 1]++;
            lab[e] = (uint32_t)lab_of(e);
            dst[e] = (uint32_t)dst_of(e);
        }
        for (size_t s = 0; s <= states; s++) off[s + 1] += off[s];
    }
    // from an automaton that compare_operand_fault() accepts
    void load(const stcsp_observer_result &o) {
        const size_t w = (size_t)o.n_observable, E = (size_t)o.n_edges;
        auto row = [&](size_t e) { return o.edge_values + e * w; };
        std::vector<uint32_t> order(E), rank(E);
        for (size_t e = 0; e < E; e++) order[e] = (uint32_t)e;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return std::lexicographical_compare(row(a), row(a) + w, row(b), row(b) + w); });
        rows.clear();
        n_rows = 0;
        for (size_t i = 0; i < E; i++) {
            if (!i || !std::equal(row(order[i]), row(order[i]) + w, row(order[i - 1]))) {
                rows.insert(rows.end(), row(order[i]), row(order[i]) + w);
                n_rows++;
            }
            rank[order[i]] = n_rows - 1;
        }
        set_graph(o.n_observable, (size_t)o.n_states, o.state_final, E, [&](size_t e) { return o.edge_src[e]; }, [&](size_t e) { return rank[e]; },
                  [&](size_t e) { return o.edge_dst[e]; });
    }
};

// The sorted distinct rows of a and b together ([..][w]; returns how many), and where each row of a and of b lies among them
inline uint32_t merge_rows(size_t w, const std::vector<int32_t> &a, size_t na, const std::vector<int32_t> &b, size_t nb, std::vector<int32_t> &common,
                       std::vector<uint32_t> &map_a, std::vector<uint32_t> &map_b) {
    common.clear();
    map_a.resize(na);
    map_b.resize(nb);
    uint32_t n = 0;
    for (size_t i = 0, j = 0; i < na || j < nb; n++) {
        const int32_t *ra = a.data() + i * w, *rb = b.data() + j * w;
        const bool take_a = j == nb || (i < na && !std::lexicographical_compare(rb, rb + w, ra, ra + w));  // a's row <= b's
        const bool take_b = i == na || (j < nb && !std::lexicographical_compare(ra, ra + w, rb, rb + w));  // b's row <= a's
        const int32_t *r = take_a ? ra : rb;
        common.insert(common.end(), r, r + w);
        if (take_a) map_a[i++] = n;
        if (take_b) map_b[j++] = n;
    }
    return n;
}

// The product of two deterministic automata completed with a sink each, numbered breadth-first with the out-edges of a pair in
// row order, and the four verdicts with their witnesses
struct HostComparison {
    int64_t n_pairs = 0, n_pair_edges = 0;
    int32_t levels = 0, n_obs = 0;
    int32_t witness_len[4] = {-1, -1, -1, -1}, witness_left[4] = {-1, -1, -1, -1}, witness_right[4] = {-1, -1, -1, -1};
    int64_t witness_off[5] = {0, 0, 0, 0, 0};  // in rows
    std::vector<int32_t> witness_values;

    // STCSP_OK; STCSP_E_INVALID: a malformed operand or two numbers of observable variables; STCSP_E_NOMEM: more than max_pairs pairs
    int run(const stcsp_observer_result &L, const stcsp_observer_result &R, int64_t max_pairs) {
        typedef std::vector<int32_t> Row;
        typedef std::pair<int64_t, int64_t> Pair;
        if (compare_operand_fault(L) || compare_operand_fault(R) || L.n_observable != R.n_observable) return STCSP_E_INVALID;
        n_obs = L.n_observable;
        const size_t w = (size_t)n_obs;
        auto out_edges = [&](const stcsp_observer_result &o) {  // state -> row -> destination; the last entry is the sink's
            std::vector<std::map<Row, int64_t>> out((size_t)o.n_states + 1);
            for (int64_t e = 0; e < o.n_edges; e++) out[(size_t)o.edge_src[e]][Row(o.edge_values + (size_t)e * w, o.edge_values + (size_t)(e + 1) * w)] = o.edge_dst[e];
            return out;
        };
        const std::vector<std::map<Row, int64_t>> out_l = out_edges(L), out_r = out_edges(R);
        const int64_t sink_l = L.n_states, sink_r = R.n_states;
        if (!sink_l && !sink_r) return STCSP_OK;  // two automata without states: no pair
        std::map<Pair, int64_t> number;
        std::vector<Pair> order;
        std::vector<int64_t> parent;
        std::vector<int32_t> depth;
        std::vector<Row> label;
        auto intern = [&](const Pair &p, int64_t from, int32_t d, const Row &row) {
            if (number.emplace(p, (int64_t)order.size()).second) {
                order.push_back(p);
                parent.push_back(from);
                depth.push_back(d);
                label.push_back(row);
            }
        };
        intern(Pair(0, 0), -1, 0, Row());  // (an automaton without states starts in its sink: index 0 == n_states)
        if (max_pairs < 1) return STCSP_E_NOMEM;
        for (size_t q = 0; q < order.size(); q++) {
            const Pair p = order[q];
            std::map<Row, Pair> succ;
            for (const auto &kv : out_l[(size_t)p.first]) succ[kv.first] = Pair(kv.second, sink_r);
            for (const auto &kv : out_r[(size_t)p.second]) {
                const auto it = succ.emplace(kv.first, Pair(sink_l, kv.second));
                if (!it.second) it.first->second.second = kv.second;
            }
            for (const auto &kv : succ) {
                intern(kv.second, (int64_t)q, depth[q] + 1, kv.first);
                if ((int64_t)order.size() > max_pairs) return STCSP_E_NOMEM;
                n_pair_edges++;
            }
        }
        n_pairs = (int64_t)order.size();
        for (size_t q = 0; q < order.size(); q++) {
            const int64_t l = order[q].first, r = order[q].second;
            const bool fl = l != sink_l && L.state_final[l], fr = r != sink_r && R.state_final[r];
            const bool hit[4] = {l != sink_l && r == sink_r, r != sink_r && l == sink_l, fl && !fr, fr && !fl};
            for (int k = 0; k < 4; k++)
                if (hit[k] && witness_len[k] < 0) {
                    witness_len[k] = depth[q];
                    witness_left[k] = l == sink_l ? -1 : (int32_t)l;
                    witness_right[k] = r == sink_r ? -1 : (int32_t)r;
                }
            levels = std::max(levels, depth[q] + 1);
        }
        for (int k = 0; k < 4; k++) {
            witness_off[k + 1] = witness_off[k] + std::max(witness_len[k], 0);
            if (witness_len[k] < 0) continue;
            const Pair at(witness_left[k] < 0 ? sink_l : witness_left[k], witness_right[k] < 0 ? sink_r : witness_right[k]);
            std::vector<const Row *> path;
            for (int64_t q = number[at]; parent[(size_t)q] >= 0; q = parent[(size_t)q]) path.push_back(&label[(size_t)q]);
            for (size_t i = path.size(); i-- > 0;) witness_values.insert(witness_values.end(), path[i]->begin(), path[i]->end());
        }
        return STCSP_OK;
    }
};

}  // namespace stcsp
