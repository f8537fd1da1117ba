// align_host.hpp -- the host twin of the device stream alignment (dev_align.hpp; definition: stcsp_engine.h,
// stcsp_engine_align), written from the contract: the sorted edge lists of generate_host.hpp, one
// vector of uint32 per level, and per level a worklist closure over the reversed edges (the least value first: every
// state is settled once).
//
// One implementation, used by libstcsp_host.so (stcsp_automaton_align_streams: the checker of the device pass in the
// tests, and the path for automata whose flags live on the host) and compiled into libstcsp_hip.so, which shares the
// request check.
#pragma once
#include <cstdint>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

#include "repair_host.hpp"

namespace stcsp {

constexpr int kAlignEndFinal = 1;  // STCSP_ALIGN_END_FINAL
enum : uint8_t { kAlignMatch = 0, kAlignSkip = 1, kAlignInsert = 2 };

// Offsets as the monitor takes them, no negative weight, skip and gap at least 1, and
//   max(sum of the weights, skip) * (the longest stream) + gap * n_states <= 2^31 - 2.
// A finite G_t(s) is the cost of some alignment of the rest of the stream from s: at most max(...) per step that is left
// and gap per insert, fewer than n_states of them after the last step. In the middle of a closure a value is the cost of
// an alignment that may carry up to n_states - 1 more inserts (a walk without a cycle to the state whose B it took), and a
// candidate adds one term to it: below 2 * (2^31 - 2) + 1 < 2^32 - 1, so no sum wraps and none is taken for infinity.
// weights may be NULL (all 1). Shared by the engine and the host twin.
inline bool align_request_ok(int64_t n_streams, const int64_t *offsets, const int32_t *weights, int n_obs, int32_t skip_cost, int32_t gap_cost,
                             int64_t n_states) {
    if (!monitor_offsets_ok(n_streams, offsets)) return false;
    if (skip_cost < 1 || gap_cost < 1 || n_states < 0) return false;
    int64_t sum = 0, longest = 0;
    for (int v = 0; v < n_obs; v++) {
        if (weights && weights[v] < 0) return false;
        sum += weights ? weights[v] : 1;
    }
    for (int64_t i = 0; i < n_streams; i++) longest = std::max<int64_t>(longest, offsets[i + 1] - offsets[i]);
    const int64_t limit = (1ll << 31) - 2, step = std::max<int64_t>(sum, skip_cost);
    if (longest > limit / step) return false;
    if (n_states > limit / gap_cost) return false;
    return step * longest + (int64_t)gap_cost * n_states <= limit;
}

struct AlignedStream {
    int32_t distance = -1, n_changed = 0, n_skipped = 0, n_inserted = 0;
    uint8_t end_final = 0;
    std::vector<int32_t> rows;  // [out_len * n_obs]
    std::vector<uint8_t> ops;
};

struct HostAlign {
    HostRepair rep;  // the canonical order, the live states and the step cost
    uint32_t skip = 1, gap = 1;
    std::vector<int64_t> roff, rsrc;  // the live edges by destination: roff[d] .. roff[d + 1] index rsrc

    void build(const MonitorView &a, const uint8_t *mask, const int32_t *w, int32_t skip_cost, int32_t gap_cost) {
        rep.build(a, mask, w);
        skip = (uint32_t)skip_cost;
        gap = (uint32_t)gap_cost;
        const HostGenerator &g = rep.gen;
        const size_t S = g.fin.size();
        roff.assign(S + 1, 0);
        for (int64_t d : g.dest) roff[(size_t)d + 1]++;
        for (size_t s = 0; s < S; s++) roff[s + 1] += roff[s];
        rsrc.assign(g.dest.size(), 0);
        std::vector<int64_t> at(roff.begin(), roff.end() - 1);
        for (size_t s = 0; s < S; s++)
            for (int64_t k = g.off[s]; k < g.off[s + 1]; k++) rsrc[(size_t)at[(size_t)g.dest[(size_t)k]]++] = (int64_t)s;
    }

    // The least fixpoint of G = min(G, gap + min over the out-edges of G(dst)), from the values G holds
    void close(std::vector<uint32_t> &G) const {
        typedef std::pair<uint32_t, int64_t> Item;
        std::priority_queue<Item, std::vector<Item>, std::greater<Item>> work;
        for (size_t s = 0; s < G.size(); s++)
            if (G[s] != kRepairInf) work.push(Item(G[s], (int64_t)s));
        while (!work.empty()) {
            const Item it = work.top();
            work.pop();
            if (it.first != G[(size_t)it.second]) continue;  // (settled at less since)
            for (int64_t k = roff[(size_t)it.second]; k < roff[(size_t)it.second + 1]; k++) {
                const int64_t p = rsrc[(size_t)k];
                if (gap + it.first < G[(size_t)p]) {
                    G[(size_t)p] = gap + it.first;
                    work.push(Item(G[(size_t)p], p));
                }
            }
        }
    }

    // One stream: rows = [len * n_obs]
    void align_one(const int32_t *rows, int64_t len, int flags, AlignedStream &out) const {
        const HostGenerator &g = rep.gen;
        const size_t S = g.fin.size(), m = (size_t)len;
        const int n_obs = g.n_obs, N = g.n_vars;
        out = AlignedStream();
        if (!g.root_live) return;
        std::vector<std::vector<uint32_t>> G(m + 1, std::vector<uint32_t>(S, kRepairInf));
        for (size_t s = 0; s < S; s++)
            if (g.weight[0][s] > 0.0 && (!(flags & kAlignEndFinal) || g.fin[s])) G[m][s] = 0;
        close(G[m]);
        for (size_t t = m; t-- > 0;) {
            const int32_t *x = rows + t * n_obs;
            const std::vector<uint32_t> &next = G[t + 1];
            for (size_t s = 0; s < S; s++) {
                if (g.weight[0][s] <= 0.0) continue;
                uint32_t best = next[s] == kRepairInf ? kRepairInf : skip + next[s];
                for (int64_t k = g.off[s]; k < g.off[s + 1]; k++) {
                    const uint32_t below = next[(size_t)g.dest[(size_t)k]];
                    if (below == kRepairInf) continue;
                    const uint32_t sum = rep.step_cost(g.values + g.edge[(size_t)k] * N, x) + below;
                    if (sum < best) best = sum;
                }
                G[t][s] = best;
            }
            close(G[t]);
        }
        if (G[0][0] == kRepairInf) return;
        out.distance = (int32_t)G[0][0];
        size_t s = 0, t = 0;
        for (;;) {
            const uint32_t want = G[t][s];
            if (t == m && want == 0) break;  // rule 1 (base is 0 or infinite, and `want` is finite)
            int64_t pick = -1;
            uint8_t op = kAlignInsert;
            if (t < m) {
                const int32_t *x = rows + t * n_obs;
                for (int64_t k = g.off[s]; k < g.off[s + 1] && pick < 0; k++) {  // rule 2
                    const uint32_t below = G[t + 1][(size_t)g.dest[(size_t)k]];
                    if (below != kRepairInf && rep.step_cost(g.values + g.edge[(size_t)k] * N, x) + below == want) pick = k;
                }
                if (pick >= 0) op = kAlignMatch;
                else if (G[t + 1][s] != kRepairInf && skip + G[t + 1][s] == want) op = kAlignSkip;  // rule 3
            }
            if (op == kAlignInsert) {  // rule 4
                for (int64_t k = g.off[s]; k < g.off[s + 1] && pick < 0; k++) {
                    const uint32_t beside = G[t][(size_t)g.dest[(size_t)k]];
                    if (beside != kRepairInf && gap + beside == want) pick = k;
                }
                if (pick < 0) break;  // (unreachable: a finite value is attained by one of the three)
            }
            out.ops.push_back(op);
            if (op == kAlignSkip) {
                out.n_skipped++;
                t++;
                continue;
            }
            const int32_t *row = g.values + g.edge[(size_t)pick] * N;
            for (int i = 0; i < n_obs; i++) {
                const int32_t p = row[g.obs[(size_t)i]];
                out.rows.push_back(p);
                if (op == kAlignMatch) {
                    const int32_t xv = rows[t * n_obs + i];
                    out.n_changed += xv != kRepairMissing && xv != p;
                }
            }
            s = (size_t)g.dest[(size_t)pick];
            if (op == kAlignMatch) t++;
            else out.n_inserted++;
        }
        out.end_final = g.fin[s] ? 1 : 0;
    }
};

}  // namespace stcsp
