// repair_host.hpp -- the host twin of the device stream repair (dev_repair.hpp; definition: stcsp_engine.h,
// stcsp_engine_repair), written plainly: the sorted edge lists of generate_host.hpp and one
// vector of uint32 per level.
//
// One implementation, used by libstcsp_host.so (stcsp_automaton_repair_streams: the checker of the device pass in the
// tests, and the path for automata whose flags live on the host) and compiled into libstcsp_hip.so, which shares the
// request check.
#pragma once
#include <cstdint>
#include <limits>
#include <vector>

#include "generate_host.hpp"
#include "monitor_host.hpp"

namespace stcsp {

constexpr int kRepairEndFinal = 1;                                        // STCSP_REPAIR_END_FINAL
constexpr int32_t kRepairMissing = std::numeric_limits<int32_t>::min();  // STCSP_REPAIR_MISSING
constexpr uint32_t kRepairInf = 0xffffffffu;

// Offsets as the monitor takes them, no negative weight, and (sum of the weights) * (the longest stream) <= 2^31 - 2: no
// finite cost reaches kRepairInf or leaves an int32. weights may be NULL (all 1). Shared by the engine and the host twin.
inline bool repair_request_ok(int64_t n_streams, const int64_t *offsets, const int32_t *weights, int n_obs) {
    if (!monitor_offsets_ok(n_streams, offsets)) return false;
    int64_t sum = 0, longest = 0;
    for (int v = 0; v < n_obs; v++) {
        if (weights && weights[v] < 0) return false;
        sum += weights ? weights[v] : 1;
    }
    for (int64_t i = 0; i < n_streams; i++) longest = std::max<int64_t>(longest, offsets[i + 1] - offsets[i]);
    return sum == 0 || longest <= ((1ll << 31) - 2) / sum;
}

struct HostRepair {
    HostGenerator gen;  // horizon 0: the canonical order, and weight[0][s] = 1 exactly for the live states
    std::vector<int32_t> weights;

    void build(const MonitorView &a, const uint8_t *mask, const int32_t *w) {
        gen.build(a, mask, 0, 0);
        weights.assign((size_t)gen.n_obs, 1);
        if (w) weights.assign(w, w + gen.n_obs);
    }

    uint32_t step_cost(const int32_t *row, const int32_t *x) const {
        uint32_t c = 0;
        for (int i = 0; i < gen.n_obs; i++)
            if (x[i] != kRepairMissing && row[gen.obs[(size_t)i]] != x[i]) c += (uint32_t)weights[(size_t)i];
        return c;
    }

    // One stream: rows / out = [len * n_obs]. out is written only when a repair exists, else left as it is.
    void repair_one(const int32_t *rows, int64_t len, int flags, int32_t *distance, int32_t *out, uint8_t *end_final, int32_t *n_changed) const {
        const size_t S = gen.fin.size();
        const int n_obs = gen.n_obs, N = gen.n_vars;
        *distance = -1;
        *end_final = 0;
        *n_changed = 0;
        if (!gen.root_live) return;
        std::vector<std::vector<uint32_t>> G((size_t)len + 1, std::vector<uint32_t>(S, kRepairInf));
        for (size_t s = 0; s < S; s++)
            if (gen.weight[0][s] > 0.0 && (!(flags & kRepairEndFinal) || gen.fin[s])) G[0][s] = 0;
        for (int64_t r = 1; r <= len; r++) {
            const int32_t *x = rows + (len - r) * n_obs;
            const std::vector<uint32_t> &prev = G[(size_t)r - 1];
            for (size_t s = 0; s < S; s++) {
                uint32_t best = kRepairInf;
                for (int64_t k = gen.off[s]; k < gen.off[s + 1]; k++) {
                    const uint32_t g = prev[(size_t)gen.dest[(size_t)k]];
                    if (g == kRepairInf) continue;
                    const uint32_t sum = step_cost(gen.values + gen.edge[(size_t)k] * N, x) + g;
                    if (sum < best) best = sum;
                }
                G[(size_t)r][s] = best;
            }
        }
        if (G[(size_t)len][0] == kRepairInf) return;
        *distance = (int32_t)G[(size_t)len][0];
        int64_t s = 0;
        int32_t changed = 0;
        for (int64_t t = 0; t < len; t++) {
            const int64_t r = len - t;
            const int32_t *x = rows + t * n_obs;
            const std::vector<uint32_t> &next = G[(size_t)r - 1];
            int64_t pick = -1;
            for (int64_t k = gen.off[(size_t)s]; k < gen.off[(size_t)s + 1] && pick < 0; k++) {
                const uint32_t g = next[(size_t)gen.dest[(size_t)k]];
                if (g != kRepairInf && step_cost(gen.values + gen.edge[(size_t)k] * N, x) + g == G[(size_t)r][(size_t)s]) pick = k;
            }
            if (pick < 0) break;  // (unreachable: a finite minimum is attained)
            const int32_t *row = gen.values + gen.edge[(size_t)pick] * N;
            for (int i = 0; i < n_obs; i++) {
                const int32_t p = row[gen.obs[(size_t)i]];
                out[t * n_obs + i] = p;
                changed += x[i] != kRepairMissing && x[i] != p;
            }
            s = gen.dest[(size_t)pick];
        }
        *end_final = gen.fin[(size_t)s] ? 1 : 0;
        *n_changed = changed;
    }
};

}  // namespace stcsp
