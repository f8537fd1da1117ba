// postproc.cpp -- host post-processing of the raw automaton and the solutions.dot writer.
//
// Behavioural mirror of
//   src/graph.cpp:357-418   graphTraverse      (final / valid flags, drop edges into invalid)
//   src/graph.cpp:304-355   adversarialTraverse  + checkVertexOutEdge  (167-189)
//   src/graph.cpp:247-302   adversarialTraverse2 + checkVertexOutEdge2 (193-244)
//   src/graph.cpp:420-442   renumberVertex
//   src/solveralgorithm.cpp:709-730 solverOut, src/graph.cpp:41-101,145-154 vertexOut/edgeOut
// on flat arrays (CSR) instead of hash_map<int, slist<Edge*>*> per vertex. All passes are
// monotone fixpoints, so the result does not depend on the reference's pointer-ordered
// std::set worklists. O(V+E), once per solve: host plumbing (SURVEY.md section 8f-2 lists the
// device version as a "next" row).
#include <algorithm>
#include <new>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "generate_host.hpp"
#include "monitor_host.hpp"
#include <chrono>
#include "repair_host.hpp"
#include "align_host.hpp"
#include "observer_host.hpp"
#include "components_host.hpp"
#include "optimise_host.hpp"
#include "ctl_host.hpp"
#include "compare_host.hpp"
#include "infer_host.hpp"
#include "posterior_host.hpp"
#include "okfix.hpp"
#include "stcsp_host.h"

namespace stcsp {

// Append-only text buffer with hand-rolled integer formatting: the reference prints one fprintf
// per edge (src/graph.cpp:92-101; 82 MB of text on partialorder_14), which dominates the wall
// time once the search itself takes milliseconds.
struct TextOut {
    std::vector<char> buf;
    size_t n = 0;
    FILE *fp = nullptr;  // nullptr: keep everything in memory
    explicit TextOut(FILE *f = nullptr, size_t cap = 1u << 22) : buf(cap), fp(f) {}
    void room(size_t need) {
        if (n + need <= buf.size()) return;
        if (fp) {
            fwrite(buf.data(), 1, n, fp);
            n = 0;
            if (need > buf.size()) buf.resize(need * 2);
        } else {
            buf.resize(std::max(buf.size() * 2, n + need));
        }
    }
    void str(const char *s, size_t len) {
        room(len);
        memcpy(buf.data() + n, s, len);
        n += len;
    }
    void str(const std::string &s) { str(s.data(), s.size()); }
    void lit(const char *s) { str(s, strlen(s)); }
    void ch(char c) {
        room(1);
        buf[n++] = c;
    }
    void num(long long v) {
        room(24);
        char tmp[24];
        int k = 0;
        unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
        do {
            tmp[k++] = (char)('0' + u % 10);
            u /= 10;
        } while (u);
        if (v < 0) buf[n++] = '-';
        while (k) buf[n++] = tmp[--k];
    }
    void flush() {
        if (fp && n) {
            fwrite(buf.data(), 1, n, fp);
            n = 0;
        }
    }
    std::string take() { return std::string(buf.data(), n); }
};

struct Automaton {
    int n_vars = 0, sig_len = 0, n_sig_vars = 0, n_until = 0;
    std::vector<std::string> names;
    std::vector<uint8_t> is_sig;
    std::vector<int> var_lb, var_ub;
    int64_t n_states = 0;
    int64_t table_states = -1;  // "# Number of nodes" when it differs from n_states (binary reload)
    std::vector<int32_t> cid, sig;
    std::vector<uint8_t> fail, valid, final_;
    std::vector<int64_t> id;  // printed vertex id (renumberVertex)
    std::vector<int32_t> cid_print;  // order_by_label(): constraint-set ids renumbered by first visit of renumber()
    std::vector<int64_t> esrc, edst;
    std::vector<int32_t> eval;
    std::vector<uint8_t> ealive;
    std::vector<int64_t> out_off, out_edge;  // CSR by src, edges sorted by (dst, insertion)
    std::vector<int64_t> in_off, in_edge;    // CSR by dst

    void build_csr() {
        int64_t E = (int64_t)esrc.size();
        out_off.assign(n_states + 1, 0);
        in_off.assign(n_states + 1, 0);
        for (int64_t e = 0; e < E; e++) {
            out_off[esrc[e] + 1]++;
            in_off[edst[e] + 1]++;
        }
        for (int64_t v = 0; v < n_states; v++) {
            out_off[v + 1] += out_off[v];
            in_off[v + 1] += in_off[v];
        }
        out_edge.resize(E);
        in_edge.resize(E);
        std::vector<int64_t> oc(out_off.begin(), out_off.end() - 1), ic(in_off.begin(), in_off.end() - 1);
        for (int64_t e = 0; e < E; e++) {
            out_edge[oc[esrc[e]]++] = e;
            in_edge[ic[edst[e]]++] = e;
        }
        for (int64_t v = 0; v < n_states; v++)
            std::stable_sort(out_edge.begin() + out_off[v], out_edge.begin() + out_off[v + 1],
                             [&](int64_t a, int64_t b) { return edst[a] < edst[b]; });
    }

    // State indices and the order of the edge arrays depend on the scheduling of the search, so the
    // (dst, insertion) order above differs from run to run. For output files the out-edges of every
    // state are re-ordered by content instead: destination buckets by their smallest label, edges
    // inside a bucket by label (a label determines its destination, so this is a total order) --
    // the same input then always gives the same solutions.dot / binary file.
    void order_by_label() {
        auto less = [&](int64_t a, int64_t b) {
            const int32_t *x = &eval[a * n_vars], *y = &eval[b * n_vars];
            for (int i = 0; i < n_vars; i++)
                if (x[i] != y[i]) return x[i] < y[i];
            return a < b;
        };
        std::vector<int64_t> rank(n_states, -1), touched;
        for (int64_t v = 0; v < n_states; v++) {
            auto b = out_edge.begin() + out_off[v], e = out_edge.begin() + out_off[v + 1];
            if (e - b < 2) continue;
            std::sort(b, e, less);
            int64_t next = 0;
            touched.clear();
            for (auto it = b; it != e; ++it)
                if (rank[edst[*it]] < 0) {
                    rank[edst[*it]] = next++;
                    touched.push_back(edst[*it]);
                }
            std::stable_sort(b, e, [&](int64_t x, int64_t y) { return rank[edst[x]] < rank[edst[y]]; });
            for (int64_t d : touched) rank[d] = -1;
        }
        label_ordered = true;
    }
    bool label_ordered = false;
    int32_t printed_cid(int64_t v) const {
        return (label_ordered && cid[v] >= 0 && (size_t)cid[v] < cid_print.size() && cid_print[cid[v]] >= 0) ? cid_print[cid[v]] : cid[v];
    }

    // graphTraverse (graph.cpp:357-418)
    void traverse(int root_final) {
        std::vector<int64_t> work;
        for (int64_t v = 0; v < n_states; v++) {
            if (v != 0) {
                bool fin = true;
                for (int c = n_sig_vars; fin && c < n_sig_vars + n_until; c++) fin = sig[v * sig_len + c] == 1;
                final_[v] = fin;
                valid[v] = fin;
                if (fin) work.push_back(v);
            } else {
                final_[v] = (uint8_t)root_final;
                valid[v] = final_[v];
            }
        }
        while (!work.empty()) {  // backward reachability over the parent map
            int64_t v = work.back();
            work.pop_back();
            for (int64_t i = in_off[v]; i < in_off[v + 1]; i++) {
                int64_t e = in_edge[i];
                if (!ealive[e]) continue;
                int64_t u = esrc[e];
                if (u != v && !valid[u]) {
                    valid[u] = 1;
                    work.push_back(u);
                }
            }
        }
        for (int64_t e = 0; e < (int64_t)esrc.size(); e++)
            if (ealive[e] && (valid[esrc[e]] || esrc[e] == 0) && !valid[edst[e]]) ealive[e] = 0;
    }

    // checkVertexOutEdge (graph.cpp:167-189)
    bool covers_all_values(int64_t v, int i) const {
        for (long long c = var_lb[i]; c <= var_ub[i]; c++) {  // (64-bit: a bound may be INT_MAX)
            bool exist = false;
            for (int64_t k = out_off[v]; k < out_off[v + 1] && !exist; k++) {
                int64_t e = out_edge[k];
                if (ealive[e] && eval[e * n_vars + i] == c && valid[edst[e]]) exist = true;
            }
            if (!exist) return false;
        }
        return true;
    }
    void requeue_valid_parents(int64_t v, std::set<int64_t> &todo) const {
        for (int64_t k = in_off[v]; k < in_off[v + 1]; k++) {
            int64_t e = in_edge[k];
            if (ealive[e] && esrc[e] != v && valid[esrc[e]]) todo.insert(esrc[e]);
        }
    }
    // adversarialTraverse (graph.cpp:304-355)
    int adversarial(int i) {
        if (i < 0 || i >= n_vars) return STCSP_E_INVALID;
        std::set<int64_t> todo;
        for (int64_t v = 0; v < n_states; v++) todo.insert(v);
        while (!todo.empty()) {
            int64_t v = *todo.begin();
            todo.erase(todo.begin());
            if (!covers_all_values(v, i)) {
                valid[v] = 0;
                requeue_valid_parents(v, todo);
            }
        }
        for (int64_t e = 0; e < (int64_t)esrc.size(); e++)
            if (ealive[e] && valid[esrc[e]] && !valid[edst[e]]) ealive[e] = 0;
        return valid[0];
    }
    // checkVertexOutEdge2 (graph.cpp:193-244)
    bool simultaneous_check(int64_t v, int op, int ava) {
        std::map<int, std::set<int>> seen;
        size_t op_nums = (size_t)((long long)var_ub[op] - var_lb[op] + 1);
        bool node_valid = false;
        for (int64_t k = out_off[v]; k < out_off[v + 1]; k++) {
            int64_t e = out_edge[k];
            if (!ealive[e] || !valid[edst[e]]) continue;
            std::set<int> &s = seen[eval[e * n_vars + ava]];
            s.insert(eval[e * n_vars + op]);
            if (s.size() == op_nums) node_valid = true;
        }
        if (node_valid)
            for (int64_t k = out_off[v]; k < out_off[v + 1]; k++) {
                int64_t e = out_edge[k];
                if (ealive[e] && valid[edst[e]] && seen[eval[e * n_vars + ava]].size() != op_nums) ealive[e] = 0;
            }
        return node_valid;
    }
    // adversarialTraverse2 (graph.cpp:247-302)
    int adversarial2(int op, int ava) {
        if (op < 0 || op >= n_vars || ava < 0 || ava >= n_vars) return STCSP_E_INVALID;
        std::vector<uint8_t> was_valid(valid);  // the parent map is built from valid vertices only
        std::set<int64_t> todo;
        for (int64_t v = 0; v < n_states; v++) todo.insert(v);
        while (!todo.empty()) {
            int64_t v = *todo.begin();
            todo.erase(todo.begin());
            if (!simultaneous_check(v, op, ava)) {
                valid[v] = 0;
                for (int64_t k = in_off[v]; k < in_off[v + 1]; k++) {
                    int64_t e = in_edge[k];
                    int64_t u = esrc[e];
                    if (u != v && was_valid[u] && valid[u]) todo.insert(u);
                }
            }
        }
        if (valid[0])
            for (int64_t e = 0; e < (int64_t)esrc.size(); e++)
                if (ealive[e] && valid[esrc[e]] && !valid[edst[e]]) ealive[e] = 0;
        return valid[0];
    }
    // renumberVertex (graph.cpp:420-442): stack-based walk from the root; unreachable
    // vertices keep their table id.
    void renumber() {
        std::vector<uint8_t> seen(n_states, 0);
        std::vector<int64_t> stack{0};
        int64_t next = 0;
        int32_t next_cid = 0;
        cid_print.clear();
        while (!stack.empty()) {
            int64_t v = stack.back();
            stack.pop_back();
            if (seen[v]) continue;
            seen[v] = 1;
            id[v] = next++;
            if (label_ordered && cid[v] >= 0) {  // set ids in the order this walk meets them (the search's
                if ((size_t)cid[v] >= cid_print.size()) cid_print.resize(cid[v] + 1, -1);  // discovery order is scheduling-dependent)
                if (cid_print[cid[v]] < 0) cid_print[cid[v]] = next_cid++;
            }
            int64_t last = -1;
            for (int64_t k = out_off[v]; k < out_off[v + 1]; k++) {
                int64_t e = out_edge[k];
                if (!ealive[e] || edst[e] == last) continue;
                last = edst[e];
                stack.push_back(last);
            }
        }
    }

    std::string name_line() const {
        std::string s = "#";
        for (auto &n : names) s += " " + n;
        return s;
    }
    std::string sig_name_line() const {
        std::string s = "#";
        for (int v = 0; v < n_vars; v++)
            if (is_sig[v]) s += " " + names[v];
        return s;
    }
    std::string sig_text(int64_t v, const char *sep) const {
        if (v == 0) return "S";
        std::string s;
        int n = n_sig_vars + n_until;
        for (int i = 0; i < n; i++) {
            s += std::to_string(sig[v * sig_len + i]);
            if (i != n - 1) s += sep;
        }
        return s;
    }

    // label text of one edge ("v0, v1, ..., vN-1"): per variable the text of every domain value
    // is formatted once, then an edge label is a run of short copies
    struct LabelTable {
        // Consecutive variables are grouped while the product of their domain sizes stays small
        // and the joint text fits 16 bytes; a group's text is one table lookup + one 16-byte copy
        // (partialorder_14: 31 values per label -> 8 copies).
        struct Piece {
            char text[16];
            uint32_t len;
        };
        struct Group {
            int first, count;  // variables [first, first + count)
            int base;          // index of the group's first piece
            int combos;
        };
        std::vector<Piece> piece;
        std::vector<Group> groups;
        const Automaton &a;
        const char *sep;
        LabelTable(const Automaton &au, const char *sep_) : a(au), sep(sep_) {
            const size_t seplen = strlen(sep);
            auto width = [&](int i) { return (long long)a.var_ub[i] - a.var_lb[i] + 1; };
            auto maxlen = [&](int i) {
                return std::max(std::to_string(a.var_lb[i]).size(), std::to_string(a.var_ub[i]).size()) + (i != a.n_vars - 1 ? seplen : 0);
            };
            for (int i = 0; i < a.n_vars;) {
                Group g{i, 0, (int)piece.size(), 1};
                size_t len = 0;
                while (i < a.n_vars && width(i) <= 4096 && (long long)g.combos * width(i) <= 4096 && len + maxlen(i) <= sizeof(Piece::text)) {
                    g.combos *= (int)width(i);
                    len += maxlen(i);
                    g.count++;
                    i++;
                }
                if (g.count == 0) {  // a variable that does not fit a table: formatted directly
                    g.count = -1;
                    i++;
                    groups.push_back(g);
                    continue;
                }
                for (int c = 0; c < g.combos; c++) {  // mixed radix, first variable most significant
                    std::string t;
                    int rem = c, div = g.combos;
                    for (int k = 0; k < g.count; k++) {
                        const int v = g.first + k;
                        div /= (int)width(v);
                        t += std::to_string(a.var_lb[v] + rem / div);
                        rem %= div;
                        if (v != a.n_vars - 1) t += sep;
                    }
                    Piece pc{};
                    memcpy(pc.text, t.data(), t.size());
                    pc.len = (uint32_t)t.size();
                    piece.push_back(pc);
                }
                groups.push_back(g);
            }
        }
        void put(TextOut &o, int64_t e) const {
            const int32_t *row = &a.eval[e * a.n_vars];
            o.room((size_t)a.n_vars * 16 + 32);
            char *w = o.buf.data() + o.n;
            for (const Group &g : groups) {
                bool direct = g.count < 0;
                int idx = 0;
                if (!direct)
                    for (int k = 0; k < g.count; k++) {
                        const int v = g.first + k;
                        const int d = row[v] - a.var_lb[v], wd = a.var_ub[v] - a.var_lb[v] + 1;
                        direct |= (d < 0) | (d >= wd);  // value outside the declared bounds
                        idx = idx * wd + d;
                    }
                if (!direct) {
                    const Piece &pc = piece[g.base + idx];
                    memcpy(w, pc.text, sizeof pc.text);
                    w += pc.len;
                    continue;
                }
                o.n = (size_t)(w - o.buf.data());
                const int cnt = g.count < 0 ? 1 : g.count;
                for (int k = 0; k < cnt; k++) {
                    o.num(row[g.first + k]);
                    if (g.first + k != a.n_vars - 1) o.lit(sep);
                }
                o.room((size_t)a.n_vars * 16 + 32);
                w = o.buf.data() + o.n;
            }
            o.n = (size_t)(w - o.buf.data());
        }
    };

    // solverOut / graphOut / vertexOut / edgeOut
    int write_dot(const char *path) const {
        FILE *fp = fopen(path, "w");
        if (!fp) return STCSP_E_INVALID;
        TextOut o(fp);
        o.lit("# Number of nodes = ");
        o.num(table_states >= 0 ? table_states : n_states);
        o.ch('\n');
        o.str(name_line());
        o.ch('\n');
        o.str(sig_name_line());
        o.lit("\ndigraph \"StCSP\" {\n");
        if (valid[0]) {
            LabelTable labels(*this, ", ");
            std::vector<uint8_t> seen(n_states, 0);
            // iterative version of the reference's recursive vertexOut
            struct Frame {
                int64_t v, k;
            };
            std::vector<Frame> st;
            auto open = [&](int64_t v) {
                seen[v] = 1;
                o.num(id[v]);
                o.lit(final_[v] ? " [shape=doublecircle, label=\"" : " [shape=circle, label=\"");
                o.num(printed_cid(v));
                o.lit(": ");
                o.str(sig_text(v, ", "));
                o.lit("\"];\n");
                st.push_back(Frame{v, out_off[v]});
            };
            open(0);
            while (!st.empty()) {
                Frame &f = st.back();
                while (f.k < out_off[f.v + 1] && !ealive[out_edge[f.k]]) f.k++;
                if (f.k >= out_off[f.v + 1]) {
                    st.pop_back();
                    continue;
                }
                int64_t d = edst[out_edge[f.k]];
                int64_t v = f.v;
                while (f.k < out_off[v + 1] && edst[out_edge[f.k]] == d) {  // one destination bucket
                    int64_t e = out_edge[f.k++];
                    if (f.k + 6 < out_off[v + 1]) {  // label rows are visited in CSR order, i.e. at random
                        const char *nx = (const char *)&eval[out_edge[f.k + 6] * n_vars];
                        __builtin_prefetch(nx);
                        __builtin_prefetch(nx + 64);
                    }
                    if (!ealive[e]) continue;
                    o.num(id[v]);
                    o.lit(" -> ");
                    o.num(id[d]);
                    o.lit(" [label=\"");
                    labels.put(o, e);
                    o.lit("\"];\n");
                }
                if (!seen[d]) open(d);  // invalidates f
            }
        }
        o.lit("}\n");
        o.flush();
        const bool bad = ferror(fp) != 0;
        return (fclose(fp) != 0 || bad) ? STCSP_E_INVALID : STCSP_OK;
    }

    // ---- compact binary form of the printed automaton ----------
    // Little-endian. Holds what solutions.dot holds -- the states reachable from a valid root over
    // kept edges, with their printed ids -- at ~(4 + n_vars) bytes per edge instead of ~120 of text.
    //   char  magic[8] = "STCSPAUT"; u32 version = 1; u32 n_vars, sig_len, n_sig_vars, n_until;
    //   u32 value_bytes (1: u8 offset from the variable's lb, 4: i32); u64 table_states; u64 n_states; u64 n_edges;
    //   per variable: i32 lb, i32 ub, u8 is_signature, u16 name_len, name
    //   u32 id[n_states]; i32 cid[n_states]; u8 final[n_states]; i32 sig[n_states*sig_len]; u32 out_degree[n_states];
    //   u32 dst[n_edges] (index into the state arrays, grouped by source in state order); values[n_edges*n_vars]
    static constexpr const char *kMagic = "STCSPAUT";
    int write_binary(const char *path) const {
        FILE *fp = fopen(path, "wb");
        if (!fp) return STCSP_E_INVALID;
        std::vector<int64_t> order;  // kept states in discovery order (index 0 = root)
        std::vector<int64_t> dense(n_states, -1);
        if (valid[0]) {
            dense[0] = 0;
            order.push_back(0);
            for (size_t q = 0; q < order.size(); q++)
                for (int64_t k = out_off[order[q]]; k < out_off[order[q] + 1]; k++) {
                    const int64_t e = out_edge[k];
                    if (ealive[e] && dense[edst[e]] < 0) {
                        dense[edst[e]] = (int64_t)order.size();
                        order.push_back(edst[e]);
                    }
                }
        }
        bool narrow = true;
        for (int i = 0; i < n_vars; i++) narrow = narrow && (long long)var_ub[i] - var_lb[i] < 256;
        std::vector<uint32_t> ids, outdeg, dsts;
        std::vector<int32_t> cids, sigs;
        std::vector<uint8_t> fins, vals8;
        std::vector<int32_t> vals32;
        for (int64_t v : order) {
            ids.push_back((uint32_t)id[v]);
            cids.push_back(printed_cid(v));
            fins.push_back(final_[v]);
            for (int c = 0; c < sig_len; c++) sigs.push_back(sig[v * sig_len + c]);
            uint32_t deg = 0;
            for (int64_t k = out_off[v]; k < out_off[v + 1]; k++) {
                const int64_t e = out_edge[k];
                if (!ealive[e]) continue;
                deg++;
                dsts.push_back((uint32_t)dense[edst[e]]);
                for (int i = 0; i < n_vars; i++) {
                    const int32_t x = eval[e * n_vars + i];
                    if (narrow && (x < var_lb[i] || x > var_ub[i])) {  // cannot happen for engine results
                        fclose(fp);
                        return STCSP_E_INVALID;
                    }
                    if (narrow) vals8.push_back((uint8_t)(x - var_lb[i]));
                    else vals32.push_back(x);
                }
            }
            outdeg.push_back(deg);
        }
        auto put = [&](const void *ptr, size_t bytes) { if (bytes) fwrite(ptr, 1, bytes, fp); };
        auto u32 = [&](uint32_t x) { put(&x, 4); };
        auto u64 = [&](uint64_t x) { put(&x, 8); };
        put(kMagic, 8);
        u32(1);
        u32((uint32_t)n_vars);
        u32((uint32_t)sig_len);
        u32((uint32_t)n_sig_vars);
        u32((uint32_t)n_until);
        u32(narrow ? 1 : 4);
        u64((uint64_t)n_states);
        u64(order.size());
        u64(dsts.size());
        for (int i = 0; i < n_vars; i++) {
            int32_t b[2] = {var_lb[i], var_ub[i]};
            put(b, 8);
            put(&is_sig[i], 1);
            uint16_t nl = (uint16_t)names[i].size();
            put(&nl, 2);
            put(names[i].data(), nl);
        }
        put(ids.data(), ids.size() * 4);
        put(cids.data(), cids.size() * 4);
        put(fins.data(), fins.size());
        put(sigs.data(), sigs.size() * 4);
        put(outdeg.data(), outdeg.size() * 4);
        put(dsts.data(), dsts.size() * 4);
        if (narrow) put(vals8.data(), vals8.size());
        else put(vals32.data(), vals32.size() * 4);
        const bool bad = ferror(fp) != 0;
        return (fclose(fp) != 0 || bad) ? STCSP_E_INVALID : STCSP_OK;
    }
    int read_binary(const char *path) {
        FILE *fp = fopen(path, "rb");
        if (!fp) return STCSP_E_INVALID;
        bool ok = true;
        auto get = [&](void *ptr, size_t bytes) { if (bytes && fread(ptr, 1, bytes, fp) != bytes) ok = false; };
        char magic[8] = {0};
        uint32_t h[6] = {0};
        uint64_t table = 0, ns = 0, ne = 0;
        get(magic, 8);
        get(h, sizeof h);
        get(&table, 8);
        get(&ns, 8);
        get(&ne, 8);
        if (!ok || memcmp(magic, kMagic, 8) != 0 || h[0] != 1 || (h[5] != 1 && h[5] != 4) || h[1] > (1u << 20) || h[2] > (1u << 20) ||
            ns > (1ull << 32) || ne > (1ull << 36)) {
            fclose(fp);
            return STCSP_E_INVALID;
        }
        // the counts must be covered by what is left of the file BEFORE anything is sized from them (a
        // truncated or hostile header would otherwise ask for hundreds of GB)
        {
            const long here = ftell(fp);
            long size = -1;
            if (here >= 0 && fseek(fp, 0, SEEK_END) == 0) size = ftell(fp);
            if (here < 0 || size < here || fseek(fp, here, SEEK_SET) != 0) {
                fclose(fp);
                return STCSP_E_INVALID;
            }
            const unsigned __int128 left = (unsigned __int128)(size - here);
            const unsigned __int128 need = (unsigned __int128)h[1] * 11                     // per variable: bounds, flag, name length
                                           + (unsigned __int128)ns * (4 + 4 + 1 + 4)        // ids, cids, final, outdeg
                                           + (unsigned __int128)ns * h[2] * 4               // signatures
                                           + (unsigned __int128)ne * 4                      // dsts
                                           + (unsigned __int128)ne * h[1] * (h[5] == 1 ? 1 : 4);  // labels
            if (need > left) {
                fclose(fp);
                return STCSP_E_INVALID;
            }
        }
        n_vars = (int)h[1];
        sig_len = (int)h[2];
        n_sig_vars = (int)h[3];
        n_until = (int)h[4];
        names.clear();
        var_lb.clear();
        var_ub.clear();
        is_sig.clear();
        for (int i = 0; i < n_vars && ok; i++) {
            int32_t b[2] = {0, 0};
            uint8_t sg = 0;
            uint16_t nl = 0;
            get(b, 8);
            get(&sg, 1);
            get(&nl, 2);
            std::string nm(nl, ' ');
            get(&nm[0], nl);
            var_lb.push_back(b[0]);
            var_ub.push_back(b[1]);
            is_sig.push_back(sg);
            names.push_back(nm);
        }
        table_states = (int64_t)table;
        n_states = (int64_t)std::max<uint64_t>(ns, 1);  // an EMPTY automaton keeps an invalid root
        std::vector<uint32_t> ids(ns), outdeg(ns), dsts(ne);
        cid.assign(n_states, 0);
        final_.assign(n_states, 0);
        sig.assign((size_t)n_states * sig_len, 0);
        get(ids.data(), ns * 4);
        get(cid.data(), ns * 4);
        get(final_.data(), ns);
        get(sig.data(), ns * sig_len * 4);
        get(outdeg.data(), ns * 4);
        get(dsts.data(), ne * 4);
        eval.assign((size_t)ne * n_vars, 0);
        if (h[5] == 1) {
            std::vector<uint8_t> v8((size_t)ne * n_vars);
            get(v8.data(), v8.size());
            for (size_t k = 0; k < v8.size(); k++) eval[k] = var_lb[k % n_vars] + v8[k];
        } else {
            get(eval.data(), eval.size() * 4);
        }
        fclose(fp);
        uint64_t sum = 0;
        for (uint32_t d : outdeg) sum += d;
        for (uint32_t d : dsts) ok = ok && d < ns;
        if (!ok || sum != ne) return STCSP_E_INVALID;
        id.assign(n_states, 0);
        for (uint64_t v = 0; v < ns; v++) id[v] = ids[v];
        fail.assign(n_states, 0);
        valid.assign(n_states, ns ? 1 : 0);
        esrc.clear();
        edst.assign(dsts.begin(), dsts.end());
        for (uint64_t v = 0; v < ns; v++) esrc.insert(esrc.end(), outdeg[v], (int64_t)v);
        ealive.assign(ne, 1);
        build_csr();
        return STCSP_OK;
    }

    // SURVEY.md Appendix A.7 (normative script: tests/canon.py)
    std::string canonical(int64_t *n_live_states, int64_t *n_live_edges, bool want_text = true) const {
        TextOut out(nullptr, want_text ? (1u << 22) : 4096);
        out.str(name_line());
        out.ch('\n');
        out.str(sig_name_line());
        out.ch('\n');
        int64_t ns = 0, ne = 0;
        if (!valid[0]) {
            out.lit("EMPTY\n");
        } else {
            std::vector<int64_t> num(n_states, -1), order;
            std::map<int, int> cidmap;
            std::vector<int64_t> sorted_edges, sorted_off{0};  // per state in `order`: live out-edges sorted by label
            auto sort_out = [&](int64_t u) {
                const size_t b = sorted_edges.size();
                for (int64_t k = out_off[u]; k < out_off[u + 1]; k++)
                    if (ealive[out_edge[k]]) sorted_edges.push_back(out_edge[k]);
                std::sort(sorted_edges.begin() + b, sorted_edges.end(), [&](int64_t a, int64_t b2) {
                    const int32_t *x = &eval[a * n_vars], *y = &eval[b2 * n_vars];
                    for (int i = 0; i < n_vars; i++)
                        if (x[i] != y[i]) return x[i] < y[i];
                    return a < b2;
                });
                sorted_off.push_back((int64_t)sorted_edges.size());
            };
            num[0] = 0;
            order.push_back(0);
            for (size_t q = 0; q < order.size(); q++) {
                sort_out(order[q]);
                for (int64_t k = sorted_off[q]; k < sorted_off[q + 1]; k++) {
                    int64_t v = edst[sorted_edges[k]];
                    if (num[v] < 0) {
                        num[v] = (int64_t)order.size();
                        order.push_back(v);
                    }
                }
            }
            ns = (int64_t)order.size();
            ne = (int64_t)sorted_edges.size();
            if (want_text) {
                LabelTable labels(*this, " ");
                for (size_t q = 0; q < order.size(); q++) {
                    const int64_t u = order[q];
                    if (!cidmap.count(cid[u])) {
                        int k = (int)cidmap.size();
                        cidmap[cid[u]] = k;
                    }
                    out.lit("S ");
                    out.num(num[u]);
                    out.ch(' ');
                    out.num(cidmap[cid[u]]);
                    out.ch(' ');
                    out.num((int)final_[u]);
                    out.ch(' ');
                    out.str(sig_text(u, " "));
                    out.ch('\n');
                    for (int64_t k = sorted_off[q]; k < sorted_off[q + 1]; k++) {
                        const int64_t e = sorted_edges[k];
                        out.lit("E ");
                        out.num(num[u]);
                        out.ch(' ');
                        out.num(num[edst[e]]);
                        out.ch(' ');
                        labels.put(out, e);
                        out.ch('\n');
                    }
                }
            }
        }
        if (n_live_states) *n_live_states = ns;
        if (n_live_edges) *n_live_edges = ne;
        return out.take();
    }

    // ---- bisimulation quotient (no reference counterpart; device twin: dev_quotient.hpp, definition: stcsp_engine.h) ----
    std::vector<uint8_t> observable;  // [n_vars], empty = the default mask (every variable whose name does not start with "_V")
    std::vector<uint8_t> observable_mask(const uint8_t *obs) const {
        std::vector<uint8_t> m((size_t)n_vars, 1);
        for (int v = 0; v < n_vars; v++) m[(size_t)v] = obs ? (uint8_t)(obs[v] != 0) : (uint8_t)(names[(size_t)v].compare(0, 2, "_V") != 0);
        return m;
    }
    // the live automaton: valid states the (valid) root reaches over alive edges
    std::vector<uint8_t> live_states() const {
        std::vector<uint8_t> live((size_t)n_states, 0);
        if (n_states == 0 || !valid[0]) return live;
        std::vector<int64_t> stack{0};
        live[0] = 1;
        while (!stack.empty()) {
            const int64_t u = stack.back();
            stack.pop_back();
            for (int64_t k = out_off[u]; k < out_off[u + 1]; k++) {
                const int64_t e = out_edge[k], v = edst[e];
                if (ealive[e] && valid[v] && !live[v]) {
                    live[v] = 1;
                    stack.push_back(v);
                }
            }
        }
        return live;
    }
    // tests/canon.py's numbering: breadth-first from the root, the live out-edges of a state in label order; -1 = not reached
    std::vector<int64_t> canonical_numbers() const {
        std::vector<int64_t> num((size_t)n_states, -1), order, edges;
        if (n_states == 0 || !valid[0]) return num;
        num[0] = 0;
        order.push_back(0);
        for (size_t q = 0; q < order.size(); q++) {
            const int64_t u = order[q];
            edges.clear();
            for (int64_t k = out_off[u]; k < out_off[u + 1]; k++)
                if (ealive[out_edge[k]]) edges.push_back(out_edge[k]);
            std::sort(edges.begin(), edges.end(), [&](int64_t a, int64_t b) {
                const int32_t *x = &eval[a * n_vars], *y = &eval[b * n_vars];
                for (int i = 0; i < n_vars; i++)
                    if (x[i] != y[i]) return x[i] < y[i];
                return a < b;
            });
            for (int64_t e : edges)
                if (num[(size_t)edst[e]] < 0) {
                    num[(size_t)edst[e]] = (int64_t)order.size();
                    order.push_back(edst[e]);
                }
        }
        return num;
    }
    // Plain partition refinement with ordered containers: every round keys each live state by (its class, its final
    // flag, the set of (projected label, class of destination) over its live out-edges) until the class count stops
    // growing; classes are then numbered by their least member. Returns the number of rounds.
    int bisimulation(const uint8_t *obs, int32_t *state_class, int64_t *n_classes) {
        observable = observable_mask(obs);
        const std::vector<uint8_t> live = live_states();
        std::map<std::vector<int32_t>, int32_t> label_ids;
        std::vector<int32_t> lid(esrc.size(), -1), proj;
        for (size_t e = 0; e < esrc.size(); e++) {
            if (!ealive[e] || !live[(size_t)esrc[e]] || !live[(size_t)edst[e]]) continue;
            proj.clear();
            for (int v = 0; v < n_vars; v++)
                if (observable[(size_t)v]) proj.push_back(eval[e * n_vars + v]);
            lid[e] = label_ids.emplace(proj, (int32_t)label_ids.size()).first->second;
        }
        std::vector<int32_t> cls((size_t)n_states, -1), next((size_t)n_states, -1);
        for (int64_t s = 0; s < n_states; s++)
            if (live[(size_t)s]) cls[(size_t)s] = 0;
        typedef std::set<std::pair<int32_t, int32_t>> Pairs;
        int rounds = 0;
        for (size_t prev = 0;;) {
            rounds++;
            std::map<std::pair<std::pair<int32_t, int>, Pairs>, int32_t> ids;  // ((class, final), pairs) -> new class
            for (int64_t s = 0; s < n_states; s++) {
                if (!live[(size_t)s]) continue;
                Pairs pairs;
                for (int64_t k = out_off[s]; k < out_off[s + 1]; k++) {
                    const int64_t e = out_edge[k];
                    if (lid[(size_t)e] >= 0) pairs.insert({lid[(size_t)e], cls[(size_t)edst[e]]});
                }
                next[(size_t)s] = ids.emplace(std::make_pair(std::make_pair(cls[(size_t)s], (int)final_[(size_t)s]), std::move(pairs)), (int32_t)ids.size()).first->second;
            }
            cls.swap(next);
            if (ids.size() == prev) break;
            prev = ids.size();
        }
        std::map<int32_t, int32_t> number;  // states are visited in index order: a class is numbered when its least member is met
        for (int64_t s = 0; s < n_states; s++) {
            if (!live[(size_t)s]) {
                state_class[s] = -1;
                continue;
            }
            state_class[s] = number.emplace(cls[(size_t)s], (int32_t)number.size()).first->second;
        }
        if (n_classes) *n_classes = (int64_t)number.size();
        return rounds;
    }
    // The quotient under a partition (state_class as bisimulation() or the device pass give it): one state per class,
    // printed with the constraint id and signature of the member the canonical numbering reaches first; one edge per distinct (source class, projected
    // label, destination class), carrying the lexicographically least full label among the edges that project on it.
    int quotient(const int32_t *state_class, int64_t n_classes, Automaton &q) const {
        if (n_classes < 0) return STCSP_E_INVALID;
        const std::vector<uint8_t> mask = observable.empty() ? observable_mask(nullptr) : observable;
        q.n_vars = n_vars;
        q.sig_len = sig_len;
        q.n_sig_vars = n_sig_vars;
        q.n_until = n_until;
        q.names = names;
        q.is_sig = is_sig;
        q.var_lb = var_lb;
        q.var_ub = var_ub;
        q.observable = observable;
        const bool empty = n_classes == 0 || n_states == 0 || state_class[0] != 0;  // no live root: the EMPTY automaton
        q.n_states = empty ? 1 : n_classes;
        q.cid.assign((size_t)q.n_states, 0);
        q.sig.assign((size_t)q.n_states * sig_len, 0);
        q.fail.assign((size_t)q.n_states, 0);
        q.valid.assign((size_t)q.n_states, empty ? 0 : 1);
        q.final_.assign((size_t)q.n_states, 0);
        q.id.resize((size_t)q.n_states);
        for (int64_t c = 0; c < q.n_states; c++) q.id[(size_t)c] = c;
        if (!empty) {
            // the member a class is printed as: the one the canonical numbering reaches first (state indices depend on the
            // search's scheduling, that numbering does not); the root for the root's class
            const std::vector<int64_t> num = canonical_numbers();
            std::vector<int64_t> rep((size_t)n_classes, -1);
            auto before = [&](int64_t a, int64_t b) { return num[(size_t)a] >= 0 && (num[(size_t)b] < 0 || num[(size_t)a] < num[(size_t)b]); };
            for (int64_t s = 0; s < n_states; s++) {
                const int32_t c = state_class[s];
                if (c < -1 || c >= n_classes) return STCSP_E_INVALID;
                if (c < 0) continue;
                int64_t &r = rep[(size_t)c];
                if (r < 0 || before(s, r)) r = s;
            }
            for (int64_t c = 0; c < n_classes; c++) {
                const int64_t s = rep[(size_t)c];
                if (s < 0) return STCSP_E_INVALID;  // a class without a member
                q.cid[(size_t)c] = cid[(size_t)s];
                q.final_[(size_t)c] = final_[(size_t)s];
                std::copy(sig.begin() + s * sig_len, sig.begin() + (s + 1) * sig_len, q.sig.begin() + c * sig_len);
            }
            typedef std::pair<std::pair<int32_t, int32_t>, std::vector<int32_t>> Key;  // ((source class, destination class), projected label)
            std::map<Key, int64_t> least;                                              // -> edge with the least full label
            Key key;
            for (size_t e = 0; e < esrc.size(); e++) {
                const int32_t cs = state_class[esrc[e]], cd = state_class[edst[e]];
                if (!ealive[e] || cs < 0 || cd < 0) continue;
                key.first = {cs, cd};
                key.second.clear();
                for (int v = 0; v < n_vars; v++)
                    if (mask[(size_t)v]) key.second.push_back(eval[e * n_vars + v]);
                auto it = least.emplace(key, (int64_t)e);
                if (!it.second && std::lexicographical_compare(eval.begin() + e * n_vars, eval.begin() + (e + 1) * n_vars,
                                                               eval.begin() + it.first->second * n_vars, eval.begin() + (it.first->second + 1) * n_vars))
                    it.first->second = (int64_t)e;
            }
            for (const auto &kv : least) {
                q.esrc.push_back(kv.first.first.first);
                q.edst.push_back(kv.first.first.second);
                q.eval.insert(q.eval.end(), eval.begin() + kv.second * n_vars, eval.begin() + (kv.second + 1) * n_vars);
            }
        }
        q.ealive.assign(q.esrc.size(), 1);
        q.build_csr();
        return STCSP_OK;
    }
    // The observer as an automaton (o: stcsp_engine_observer() or stcsp_automaton_observer() of this automaton under `obs`): one state
    // per set, printed with the constraint id and signature of its member of least canonical number; an edge carries the
    // lexicographically least full label among the live edges between members of its two sets that project on its row.
    int from_observer(const uint8_t *obs, const stcsp_observer_result &o, Automaton &q) const {
        const std::vector<uint8_t> mask = observable_mask(obs);
        int n_obs = 0;
        for (uint8_t m : mask) n_obs += m != 0;
        if (o.n_states < 0 || o.n_edges < 0 || o.n_observable != n_obs || (o.n_states == 0 && o.n_edges != 0)) return STCSP_E_INVALID;
        q.n_vars = n_vars;
        q.sig_len = sig_len;
        q.n_sig_vars = n_sig_vars;
        q.n_until = n_until;
        q.names = names;
        q.is_sig = is_sig;
        q.var_lb = var_lb;
        q.var_ub = var_ub;
        q.observable = mask;
        const bool empty = o.n_states == 0;  // no live root: the EMPTY automaton
        q.n_states = empty ? 1 : o.n_states;
        q.cid.assign((size_t)q.n_states, 0);
        q.sig.assign((size_t)q.n_states * sig_len, 0);
        q.fail.assign((size_t)q.n_states, 0);
        q.valid.assign((size_t)q.n_states, empty ? 0 : 1);
        q.final_.assign((size_t)q.n_states, 0);
        q.id.resize((size_t)q.n_states);
        for (int64_t c = 0; c < q.n_states; c++) q.id[(size_t)c] = c;
        if (!empty) {
            const std::vector<int64_t> num = canonical_numbers();
            if (o.member_off[0] != 0) return STCSP_E_INVALID;
            for (int64_t c = 0; c < o.n_states; c++) {
                int64_t rep = -1;
                if (o.member_off[c + 1] <= o.member_off[c]) return STCSP_E_INVALID;  // (a set is never empty)
                for (int64_t k = o.member_off[c]; k < o.member_off[c + 1]; k++) {
                    const int64_t s = o.member[k];
                    if (s < 0 || s >= n_states || num[(size_t)s] < 0) return STCSP_E_INVALID;  // not a live state
                    if (rep < 0 || num[(size_t)s] < num[(size_t)rep]) rep = s;
                }
                q.cid[(size_t)c] = cid[(size_t)rep];
                q.final_[(size_t)c] = o.state_final[c] ? 1 : 0;
                std::copy(sig.begin() + rep * sig_len, sig.begin() + (rep + 1) * sig_len, q.sig.begin() + c * sig_len);
            }
            std::map<std::vector<int32_t>, int64_t> least;  // of the source set in hand: projected row -> edge with the least full label
            int64_t in_hand = -1;
            std::vector<int32_t> row;
            for (int64_t i = 0; i < o.n_edges; i++) {
                const int64_t c = o.edge_src[i], d = o.edge_dst[i];
                if (c < 0 || c >= o.n_states || d < 0 || d >= o.n_states) return STCSP_E_INVALID;
                if (c != in_hand) {
                    least.clear();
                    in_hand = c;
                    for (int64_t k = o.member_off[c]; k < o.member_off[c + 1]; k++) {
                        const int64_t s = o.member[k];
                        for (int64_t j = out_off[s]; j < out_off[s + 1]; j++) {
                            const int64_t e = out_edge[j];
                            if (!ealive[e] || num[(size_t)edst[e]] < 0) continue;
                            row.clear();
                            for (int v = 0; v < n_vars; v++)
                                if (mask[(size_t)v]) row.push_back(eval[e * n_vars + v]);
                            auto it = least.emplace(row, e);
                            if (!it.second && std::lexicographical_compare(eval.begin() + e * n_vars, eval.begin() + (e + 1) * n_vars,
                                                                           eval.begin() + it.first->second * n_vars, eval.begin() + (it.first->second + 1) * n_vars))
                                it.first->second = e;
                        }
                    }
                }
                row.assign(o.edge_values + i * n_obs, o.edge_values + (i + 1) * n_obs);
                const auto it = least.find(row);
                if (it == least.end()) return STCSP_E_INVALID;  // no live edge of the set projects on this row
                q.esrc.push_back(c);
                q.edst.push_back(d);
                q.eval.insert(q.eval.end(), eval.begin() + it->second * n_vars, eval.begin() + (it->second + 1) * n_vars);
            }
        }
        q.ealive.assign(q.esrc.size(), 1);
        q.build_csr();
        return STCSP_OK;
    }
};

struct Merged {
    std::vector<int32_t> cid, sig, eval;
    std::vector<uint8_t> fail, issig;
    std::vector<int64_t> esrc, edst;
    stcsp_result res{};
};

}  // namespace stcsp

using stcsp::Automaton;

struct stcsp_automaton {
    Automaton a;
    int root_final;
};
struct stcsp_merged {
    stcsp::Merged m;
};
struct stcsp_observer {
    stcsp::HostObserver o;
    stcsp_observer_result res;
};
struct stcsp_comparison {
    stcsp::HostComparison c;
    stcsp_compare_result res;
};
struct stcsp_components {
    stcsp::HostComponents c;
    stcsp_components_result res;
};
struct stcsp_optimise {
    stcsp::HostOptimise o;
    stcsp_optimise_result res;
};
struct stcsp_ctl {
    stcsp::HostCtl c;
    stcsp_ctl_result res;
};

extern "C" {

int stcsp_automaton_build(const stcsp_problem *p, const stcsp_result *r, stcsp_automaton **out) {
    if (!p || !r || !out) return STCSP_E_INVALID;
    stcsp_automaton *h = new stcsp_automaton();
    Automaton &a = h->a;
    a.n_vars = r->n_vars;
    a.sig_len = r->sig_len;
    a.n_sig_vars = r->n_sig_vars;
    a.n_until = r->n_until;
    for (int v = 0; v < a.n_vars; v++) {
        a.names.push_back(p->var_names && p->var_names[v] ? p->var_names[v] : ("v" + std::to_string(v)));
        a.var_lb.push_back(p->var_lb[v]);
        a.var_ub.push_back(p->var_ub[v]);
    }
    a.is_sig.assign(r->var_is_signature, r->var_is_signature + a.n_vars);
    a.n_states = r->n_states;
    a.cid.assign(r->state_cid, r->state_cid + r->n_states);
    a.sig.assign(r->state_sig, r->state_sig + r->n_states * (int64_t)r->sig_len);
    a.fail.assign(r->state_fail, r->state_fail + r->n_states);
    a.valid.assign(r->n_states, 0);
    a.final_.assign(r->n_states, 0);
    a.id.resize(r->n_states);
    for (int64_t v = 0; v < r->n_states; v++) a.id[v] = v;
    a.esrc.assign(r->edge_src, r->edge_src + r->n_edges);
    a.edst.assign(r->edge_dst, r->edge_dst + r->n_edges);
    a.eval.assign(r->edge_values, r->edge_values + r->n_edges * (int64_t)r->n_vars);
    a.ealive.assign(r->n_edges, 1);
    for (int64_t e = 0; e < r->n_edges; e++)  // tolerate raw logs (STCSP_F_KEEP_RAW_EDGES)
        if (a.fail[a.edst[e]]) a.ealive[e] = 0;
    a.build_csr();
    h->root_final = r->root_final;
    *out = h;
    return STCSP_OK;
}

void stcsp_automaton_free(stcsp_automaton *a) { delete a; }

int stcsp_automaton_traverse(stcsp_automaton *a) {
    if (!a) return STCSP_E_INVALID;
    a->a.traverse(a->root_final);
    return STCSP_OK;
}
int stcsp_automaton_adversarial(stcsp_automaton *a, int var_index) { return a ? a->a.adversarial(var_index) : STCSP_E_INVALID; }
int stcsp_automaton_adversarial2(stcsp_automaton *a, int op, int ava) { return a ? a->a.adversarial2(op, ava) : STCSP_E_INVALID; }
int stcsp_automaton_import_flags(stcsp_automaton *a, const uint8_t *valid, const uint8_t *final_flags, const uint8_t *alive) {
    if (!a || !valid || !final_flags || (!alive && !a->a.esrc.empty())) return STCSP_E_INVALID;
    Automaton &g = a->a;
    g.valid.assign(valid, valid + g.n_states);
    g.final_.assign(final_flags, final_flags + g.n_states);
    for (size_t e = 0; e < g.esrc.size(); e++) g.ealive[e] = g.ealive[e] && alive[e];
    return STCSP_OK;
}
int stcsp_automaton_flags(const stcsp_automaton *a, uint8_t *valid, uint8_t *final_flags, uint8_t *alive) {
    if (!a) return STCSP_E_INVALID;
    const Automaton &g = a->a;
    if (valid) memcpy(valid, g.valid.data(), g.valid.size());
    if (final_flags) memcpy(final_flags, g.final_.data(), g.final_.size());
    if (alive) memcpy(alive, g.ealive.data(), g.ealive.size());
    return STCSP_OK;
}
int stcsp_automaton_order_by_label(stcsp_automaton *a) {
    if (!a) return STCSP_E_INVALID;
    a->a.order_by_label();
    return STCSP_OK;
}
int stcsp_automaton_renumber(stcsp_automaton *a) {
    if (!a) return STCSP_E_INVALID;
    a->a.renumber();
    return STCSP_OK;
}
int stcsp_automaton_write_dot(const stcsp_automaton *a, const char *path) { return a ? a->a.write_dot(path) : STCSP_E_INVALID; }
int stcsp_automaton_write_binary(const stcsp_automaton *a, const char *path) { return a && path ? a->a.write_binary(path) : STCSP_E_INVALID; }
int stcsp_automaton_read_binary(const char *path, stcsp_automaton **out) {
    if (!path || !out) return STCSP_E_INVALID;
    stcsp_automaton *h = nullptr;
    try {  // no exception may cross the C boundary
        h = new stcsp_automaton();
        h->root_final = 0;
        int rc = h->a.read_binary(path);
        if (rc != STCSP_OK) {
            delete h;
            return rc;
        }
    } catch (const std::bad_alloc &) {
        delete h;
        return STCSP_E_NOMEM;
    } catch (...) {
        delete h;
        return STCSP_E_INVALID;
    }
    *out = h;
    return STCSP_OK;
}

int stcsp_automaton_bisimulation(stcsp_automaton *a, const uint8_t *observable, int32_t *state_class_out, int64_t *n_classes) {
    if (!a || !state_class_out) return STCSP_E_INVALID;
    try {
        return a->a.bisimulation(observable, state_class_out, n_classes);
    } catch (const std::bad_alloc &) {
        return STCSP_E_NOMEM;
    }
}
int stcsp_automaton_check_streams(const stcsp_automaton *a, const uint8_t *observable, int64_t n_streams, const int64_t *offsets,
                                  const int32_t *values, int32_t *accepted_len, int32_t *n_end, uint8_t *end_final,
                                  int64_t *max_set_size) {
    if (!a || !stcsp::monitor_offsets_ok(n_streams, offsets)) return STCSP_E_INVALID;
    if (n_streams > 0 && (!accepted_len || !n_end || !end_final)) return STCSP_E_INVALID;
    try {
        const Automaton &g = a->a;
        stcsp::MonitorView v;
        v.n_vars = g.n_vars;
        v.n_states = g.n_states;
        v.n_edges = (int64_t)g.esrc.size();
        v.src = g.esrc.data();
        v.dst = g.edst.data();
        v.values = g.eval.data();
        v.valid = g.valid.data();
        v.final_ = g.final_.data();
        v.alive = g.ealive.data();
        stcsp::HostMonitor mon;
        mon.build(v, g.observable_mask(observable).data());
        if (n_streams > 0 && offsets[n_streams] > 0 && mon.n_obs > 0 && !values) return STCSP_E_INVALID;
        int64_t largest = mon.root_live ? 1 : 0;
        for (int64_t i = 0; i < n_streams; i++)
            largest = std::max(largest, mon.check_one(values + offsets[i] * mon.n_obs, offsets[i + 1] - offsets[i], &accepted_len[i], &n_end[i], &end_final[i]));
        if (max_set_size) *max_set_size = largest;
    } catch (const std::bad_alloc &) {
        return STCSP_E_NOMEM;
    }
    return STCSP_OK;
}
static stcsp::MonitorView generator_view(const Automaton &g) {
    stcsp::MonitorView v;
    v.n_vars = g.n_vars;
    v.n_states = g.n_states;
    v.n_edges = (int64_t)g.esrc.size();
    v.src = g.esrc.data();
    v.dst = g.edst.data();
    v.values = g.eval.data();
    v.valid = g.valid.data();
    v.final_ = g.final_.data();
    v.alive = g.ealive.data();
    return v;
}
int stcsp_automaton_generate(const stcsp_automaton *a, const uint8_t *observable, int32_t horizon, int32_t flags, int64_t n_streams,
                             int32_t len, uint64_t seed, const uint64_t *ranks, double *count, int32_t *values, uint8_t *end_final) {
    if (!a || horizon < 0 || n_streams < 0) return STCSP_E_INVALID;
    try {
        stcsp::HostGenerator gen;
        if (!gen.build(generator_view(a->a), a->a.observable_mask(observable).data(), horizon, flags)) return STCSP_E_UNSUPPORTED;
        if (count) std::copy(gen.count.begin(), gen.count.end(), count);
        if (!stcsp::generate_request_ok(gen.count, n_streams, len, ranks)) return STCSP_E_INVALID;
        if (n_streams > 0 && (!end_final || (!values && len > 0 && gen.n_obs > 0))) return STCSP_E_INVALID;
        for (int64_t i = 0; i < n_streams; i++)
            gen.generate_one(len, seed, (uint64_t)i, ranks ? &ranks[i] : nullptr, values + (size_t)i * (size_t)len * (size_t)gen.n_obs, &end_final[i]);
    } catch (const std::bad_alloc &) {
        return STCSP_E_NOMEM;
    }
    return STCSP_OK;
}
int stcsp_automaton_count_streams(const stcsp_automaton *a, int32_t horizon, int32_t flags, double *count) {
    if (!a || horizon < 0 || !count) return STCSP_E_INVALID;
    try {
        stcsp::HostGenerator gen;
        std::vector<uint8_t> none((size_t)a->a.n_vars, 0);
        if (!gen.build(generator_view(a->a), none.data(), horizon, flags)) return STCSP_E_UNSUPPORTED;
        std::copy(gen.count.begin(), gen.count.end(), count);
    } catch (const std::bad_alloc &) {
        return STCSP_E_NOMEM;
    }
    return STCSP_OK;
}
int stcsp_automaton_repair_streams(const stcsp_automaton *a, const uint8_t *observable, int32_t flags, const int32_t *weights, int64_t n_streams,
                                   const int64_t *offsets, const int32_t *values, int32_t *distance, int32_t *out_values, uint8_t *end_final,
                                   int32_t *n_changed) {
    if (!a) return STCSP_E_INVALID;
    try {
        stcsp::HostRepair rep;
        const std::vector<uint8_t> mask = a->a.observable_mask(observable);
        int n_obs = 0;
        for (uint8_t m : mask) n_obs += m != 0;
        if (!stcsp::repair_request_ok(n_streams, offsets, weights, n_obs)) return STCSP_E_INVALID;
        if (n_streams > 0 && (!distance || !end_final || !n_changed)) return STCSP_E_INVALID;
        const int64_t cells = n_streams > 0 ? offsets[n_streams] * n_obs : 0;
        if (cells > 0 && (!values || !out_values)) return STCSP_E_INVALID;
        rep.build(generator_view(a->a), mask.data(), weights);
        std::fill(out_values, out_values + cells, 0);
        for (int64_t i = 0; i < n_streams; i++)
            rep.repair_one(values + offsets[i] * n_obs, offsets[i + 1] - offsets[i], flags, &distance[i], out_values + offsets[i] * n_obs, &end_final[i],
                           &n_changed[i]);
    } catch (const std::bad_alloc &) {
        return STCSP_E_NOMEM;
    }
    return STCSP_OK;
}
int stcsp_automaton_align_streams(const stcsp_automaton *a, const uint8_t *observable, int32_t flags, const int32_t *weights, int32_t skip_cost,
                                  int32_t gap_cost, int64_t n_streams, const int64_t *offsets, const int32_t *values, int32_t *distance,
                                  int64_t *out_offsets, int32_t **out_values, int64_t *op_offsets, uint8_t **ops, uint8_t *end_final,
                                  int32_t *n_changed, int32_t *n_skipped, int32_t *n_inserted) {
    if (!a || !out_values || !ops) return STCSP_E_INVALID;
    *out_values = nullptr;
    *ops = nullptr;
    try {
        stcsp::HostAlign aln;
        const std::vector<uint8_t> mask = a->a.observable_mask(observable);
        int n_obs = 0;
        for (uint8_t m : mask) n_obs += m != 0;
        if (!stcsp::align_request_ok(n_streams, offsets, weights, n_obs, skip_cost, gap_cost, a->a.n_states)) return STCSP_E_INVALID;
        if (!out_offsets || !op_offsets) return STCSP_E_INVALID;
        if (n_streams > 0 && (!distance || !end_final || !n_changed || !n_skipped || !n_inserted)) return STCSP_E_INVALID;
        if (n_streams > 0 && offsets[n_streams] * n_obs > 0 && !values) return STCSP_E_INVALID;
        aln.build(generator_view(a->a), mask.data(), weights, skip_cost, gap_cost);
        std::vector<int32_t> rows;
        std::vector<uint8_t> all_ops;
        stcsp::AlignedStream one;
        out_offsets[0] = op_offsets[0] = 0;
        for (int64_t i = 0; i < n_streams; i++) {
            aln.align_one(values + offsets[i] * n_obs, offsets[i + 1] - offsets[i], flags, one);
            distance[i] = one.distance;
            end_final[i] = one.end_final;
            n_changed[i] = one.n_changed;
            n_skipped[i] = one.n_skipped;
            n_inserted[i] = one.n_inserted;
            rows.insert(rows.end(), one.rows.begin(), one.rows.end());
            all_ops.insert(all_ops.end(), one.ops.begin(), one.ops.end());
            op_offsets[i + 1] = (int64_t)all_ops.size();
            out_offsets[i + 1] = out_offsets[i] + (int64_t)one.ops.size() - one.n_skipped;
        }
        int32_t *vals = (int32_t *)malloc(std::max<size_t>(rows.size(), 1) * sizeof(int32_t));
        uint8_t *o = (uint8_t *)malloc(std::max<size_t>(all_ops.size(), 1));
        if (!vals || !o) {
            free(vals);
            free(o);
            return STCSP_E_NOMEM;
        }
        std::copy(rows.begin(), rows.end(), vals);
        std::copy(all_ops.begin(), all_ops.end(), o);
        *out_values = vals;
        *ops = o;
    } catch (const std::bad_alloc &) {
        return STCSP_E_NOMEM;
    }
    return STCSP_OK;
}
int stcsp_automaton_infer_streams(const stcsp_automaton *a, const uint8_t *observable, int32_t flags, int64_t n_streams, const int64_t *offsets,
                                  const int32_t *values, int32_t draws, const uint64_t *ranks, uint64_t seed, double *count, int64_t *support_off,
                                  int32_t **support_val, int32_t *n_states, int32_t *draw_values, uint8_t *end_final) {
    if (!a || !support_val) return STCSP_E_INVALID;
    *support_val = nullptr;
    try {
        stcsp::HostInfer inf;
        const std::vector<uint8_t> mask = a->a.observable_mask(observable);
        int n_obs = 0;
        for (uint8_t m : mask) n_obs += m != 0;
        if (!stcsp::infer_request_ok(n_streams, offsets, draws) || !support_off) return STCSP_E_INVALID;
        if (n_streams > 0 && (!count || !n_states || (draws > 0 && !end_final))) return STCSP_E_INVALID;
        const int64_t steps = n_streams > 0 ? offsets[n_streams] : 0;
        if (steps * n_obs > 0 && (!values || (draws > 0 && !draw_values))) return STCSP_E_INVALID;
        inf.build(generator_view(a->a), mask.data());
        std::vector<int32_t> all;
        std::vector<std::vector<double>> B;
        std::vector<std::vector<int32_t>> support;
        support_off[0] = 0;
        for (int64_t i = 0; i < n_streams; i++) {
            const int64_t len = offsets[i + 1] - offsets[i];
            const int32_t *rows = values + offsets[i] * n_obs;
            count[i] = inf.backward(rows, len, flags, B);
            inf.forward(rows, len, B, count[i], support, n_states + offsets[i] + i);
            for (size_t c = 0; c < support.size(); c++) {
                all.insert(all.end(), support[c].begin(), support[c].end());
                support_off[(size_t)offsets[i] * n_obs + c + 1] = (int64_t)all.size();
            }
            const uint64_t *rk = ranks ? ranks + i * draws : nullptr;
            const int bad = stcsp::infer_draws_ok(count[i], draws, rk);
            if (bad) return bad == 1 ? STCSP_E_UNSUPPORTED : STCSP_E_INVALID;
            for (int64_t j = 0; j < draws; j++) {
                const int64_t q = i * draws + j;
                int32_t *out = draw_values + (offsets[i] * draws + j * len) * n_obs;
                end_final[q] = 0;
                if (count[i] > 0.0) {
                    if (!inf.walk(rows, len, B, seed, (uint64_t)q, rk ? &rk[j] : nullptr, out, &end_final[q])) return STCSP_E_INTERNAL;
                } else {
                    std::fill(out, out + len * n_obs, stcsp::kInferMissing);
                }
            }
        }
        int32_t *vals = (int32_t *)malloc(std::max<size_t>(all.size(), 1) * sizeof(int32_t));
        if (!vals) return STCSP_E_NOMEM;
        std::copy(all.begin(), all.end(), vals);
        *support_val = vals;
    } catch (const std::bad_alloc &) {
        return STCSP_E_NOMEM;
    }
    return STCSP_OK;
}
int stcsp_automaton_posterior_streams(const stcsp_automaton *a, const uint8_t *observable, int32_t flags, int64_t n_streams, const int64_t *offsets,
                                      const int32_t *values, const int64_t *weight_off, const int32_t *weight_val, const int32_t *weight_w,
                                      double *mass, uint8_t *exact, uint64_t *final_mass, int64_t *marg_off, int32_t **marg_val, uint64_t **marg_mass) {
    if (!a || !marg_val || !marg_mass) return STCSP_E_INVALID;
    *marg_val = nullptr;
    *marg_mass = nullptr;
    try {
        stcsp::HostPosterior pos;
        const std::vector<uint8_t> mask = a->a.observable_mask(observable);
        int n_obs = 0;
        for (uint8_t m : mask) n_obs += m != 0;
        if (!stcsp::posterior_request_ok(n_streams, offsets, n_obs, weight_off, weight_val, weight_w) || !marg_off) return STCSP_E_INVALID;
        if (n_streams > 0 && (!mass || !exact || !final_mass)) return STCSP_E_INVALID;
        const int64_t steps = n_streams > 0 ? offsets[n_streams] : 0;
        if (steps * n_obs > 0 && !values) return STCSP_E_INVALID;
        pos.build(generator_view(a->a), mask.data(), weight_off, weight_val, weight_w);
        std::vector<int32_t> all_val;
        std::vector<uint64_t> all_mass;
        std::vector<std::vector<double>> B;
        std::vector<std::vector<std::pair<int32_t, uint64_t>>> marg;
        marg_off[0] = 0;
        for (int64_t i = 0; i < n_streams; i++) {
            const int64_t len = offsets[i + 1] - offsets[i];
            const int32_t *rows = values + offsets[i] * n_obs;
            mass[i] = pos.backward(rows, len, flags, B);
            exact[i] = mass[i] < 0x1.0p53;
            final_mass[i] = 0;
            if (exact[i])
                final_mass[i] = pos.forward(rows, len, B, mass[i], marg);
            else
                marg.assign((size_t)len * (size_t)n_obs, std::vector<std::pair<int32_t, uint64_t>>());
            for (size_t c = 0; c < marg.size(); c++) {
                for (const auto &vm : marg[c]) {
                    all_val.push_back(vm.first);
                    all_mass.push_back(vm.second);
                }
                marg_off[(size_t)offsets[i] * n_obs + c + 1] = (int64_t)all_val.size();
            }
        }
        int32_t *vals = (int32_t *)malloc(std::max<size_t>(all_val.size(), 1) * sizeof(int32_t));
        uint64_t *masses = (uint64_t *)malloc(std::max<size_t>(all_mass.size(), 1) * sizeof(uint64_t));
        if (!vals || !masses) {
            free(vals);
            free(masses);
            return STCSP_E_NOMEM;
        }
        std::copy(all_val.begin(), all_val.end(), vals);
        std::copy(all_mass.begin(), all_mass.end(), masses);
        *marg_val = vals;
        *marg_mass = masses;
    } catch (const std::bad_alloc &) {
        return STCSP_E_NOMEM;
    }
    return STCSP_OK;
}
int stcsp_automaton_num_observable(const stcsp_automaton *a, const uint8_t *observable) {
    if (!a) return STCSP_E_INVALID;
    int n = 0;
    for (uint8_t m : a->a.observable_mask(observable)) n += m;
    return n;
}
int stcsp_automaton_set_observable(stcsp_automaton *a, const uint8_t *observable) {
    if (!a) return STCSP_E_INVALID;
    a->a.observable = a->a.observable_mask(observable);
    return STCSP_OK;
}
int stcsp_automaton_quotient(const stcsp_automaton *a, const int32_t *state_class, int64_t n_classes, stcsp_automaton **out) {
    if (!a || !state_class || !out) return STCSP_E_INVALID;
    stcsp_automaton *h = nullptr;
    try {
        h = new stcsp_automaton();
        const int rc = a->a.quotient(state_class, n_classes, h->a);
        if (rc != STCSP_OK) {
            delete h;
            return rc;
        }
        h->root_final = h->a.final_[0];
    } catch (const std::bad_alloc &) {
        delete h;
        return STCSP_E_NOMEM;
    }
    *out = h;
    return STCSP_OK;
}

int stcsp_automaton_observer(const stcsp_automaton *a, const uint8_t *observable, int64_t max_states, stcsp_observer **out) {
    if (!a || !out || max_states < 0) return STCSP_E_INVALID;
    stcsp_observer *h = nullptr;
    try {
        h = new stcsp_observer();
        const auto t0 = std::chrono::steady_clock::now();
        if (!h->o.build(generator_view(a->a), a->a.observable_mask(observable).data(), max_states ? max_states : (int64_t)1 << 26)) {
            delete h;
            return STCSP_E_NOMEM;
        }
        stcsp::HostObserver &o = h->o;
        o.member.reserve(1);  // (empty vectors still give valid pointers)
        o.state_final.reserve(1);
        o.edge_src.reserve(1);
        o.edge_dst.reserve(1);
        o.edge_values.reserve(1);
        memset(&h->res, 0, sizeof h->res);
        h->res.n_states = o.n_states();
        h->res.n_edges = o.n_edges();
        h->res.member_off = o.member_off.data();
        h->res.member = o.member.data();
        h->res.state_final = o.state_final.data();
        h->res.edge_src = o.edge_src.data();
        h->res.edge_dst = o.edge_dst.data();
        h->res.edge_values = o.edge_values.data();
        h->res.n_labels = o.n_labels;
        h->res.max_set = o.max_set;
        h->res.n_observable = o.n_obs;
        h->res.levels = o.levels;
        h->res.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } catch (const std::bad_alloc &) {
        delete h;
        return STCSP_E_NOMEM;
    }
    *out = h;
    return STCSP_OK;
}
const stcsp_observer_result *stcsp_observer_get(const stcsp_observer *o) { return o ? &o->res : nullptr; }
void stcsp_observer_free(stcsp_observer *o) { delete o; }
int stcsp_automaton_from_observer(const stcsp_automaton *a, const uint8_t *observable, const stcsp_observer_result *observer, stcsp_automaton **out) {
    if (!a || !observer || !out) return STCSP_E_INVALID;
    stcsp_automaton *h = nullptr;
    try {
        h = new stcsp_automaton();
        const int rc = a->a.from_observer(observable, *observer, h->a);
        if (rc != STCSP_OK) {
            delete h;
            return rc;
        }
        h->root_final = h->a.final_[0];
    } catch (const std::bad_alloc &) {
        delete h;
        return STCSP_E_NOMEM;
    }
    *out = h;
    return STCSP_OK;
}

int stcsp_automaton_num_vars(const stcsp_automaton *a) { return a ? a->a.n_vars : STCSP_E_INVALID; }
const char *stcsp_automaton_var_name(const stcsp_automaton *a, int index) {
    return a && index >= 0 && index < a->a.n_vars && (size_t)index < a->a.names.size() ? a->a.names[(size_t)index].c_str() : nullptr;
}

int stcsp_compare_observers(const stcsp_observer_result *left, const stcsp_observer_result *right, int64_t max_pairs, stcsp_comparison **out) {
    if (!left || !right || !out || max_pairs < 0) return STCSP_E_INVALID;
    stcsp_comparison *h = nullptr;
    try {
        h = new stcsp_comparison();
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = h->c.run(*left, *right, max_pairs ? max_pairs : (int64_t)1 << 26);
        if (rc != STCSP_OK) {
            delete h;
            return rc;
        }
        stcsp::HostComparison &c = h->c;
        c.witness_values.reserve(1);  // (an empty vector still gives a valid pointer)
        memset(&h->res, 0, sizeof h->res);
        h->res.n_pairs = c.n_pairs;
        h->res.n_pair_edges = c.n_pair_edges;
        h->res.witness_values = c.witness_values.data();
        for (int k = 0; k < 4; k++) {
            h->res.witness_len[k] = c.witness_len[k];
            h->res.witness_left[k] = c.witness_left[k];
            h->res.witness_right[k] = c.witness_right[k];
        }
        std::copy(c.witness_off, c.witness_off + 5, h->res.witness_off);
        h->res.n_observable = c.n_obs;
        h->res.levels = c.levels;
        h->res.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } catch (const std::bad_alloc &) {
        delete h;
        return STCSP_E_NOMEM;
    }
    *out = h;
    return STCSP_OK;
}
const stcsp_compare_result *stcsp_comparison_get(const stcsp_comparison *c) { return c ? &c->res : nullptr; }
void stcsp_comparison_free(stcsp_comparison *c) { delete c; }

int stcsp_automaton_components(const stcsp_automaton *a, int64_t max_lassos, int32_t flags, stcsp_components **out) {
    if (!a || !out || max_lassos < -1) return STCSP_E_INVALID;
    stcsp_components *h = nullptr;
    try {
        h = new stcsp_components();
        const auto t0 = std::chrono::steady_clock::now();
        if (!h->c.run(generator_view(a->a), max_lassos, flags)) {
            delete h;
            return STCSP_E_INTERNAL;
        }
        stcsp::HostComponents &c = h->c;
        for (auto *v : {&c.state_component, &c.comp_size, &c.comp_depth, &c.comp_flags, &c.lasso_component, &c.lasso_stem_len, &c.lasso_values})
            v->reserve(1);  // (empty vectors still give valid pointers)
        c.state_omega.reserve(1);
        memset(&h->res, 0, sizeof h->res);
        h->res.n_states = c.n_live;
        h->res.n_components = (int64_t)c.comp_size.size();
        h->res.n_cyclic = c.n_cyclic;
        h->res.n_accepting = c.n_accepting;
        h->res.n_bottom = c.n_bottom;
        h->res.n_omega = c.n_omega;
        h->res.state_component = c.state_component.data();
        h->res.state_omega = c.state_omega.data();
        h->res.comp_size = c.comp_size.data();
        h->res.comp_depth = c.comp_depth.data();
        h->res.comp_flags = c.comp_flags.data();
        h->res.n_lassos = (int64_t)c.lasso_component.size();
        h->res.lasso_component = c.lasso_component.data();
        h->res.lasso_off = c.lasso_off.data();
        h->res.lasso_stem_len = c.lasso_stem_len.data();
        h->res.lasso_values = c.lasso_values.data();
        h->res.n_vars = c.n_vars;
        h->res.root_omega = c.root_omega;
        h->res.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } catch (const std::bad_alloc &) {
        delete h;
        return STCSP_E_NOMEM;
    }
    *out = h;
    return STCSP_OK;
}
const stcsp_components_result *stcsp_components_get(const stcsp_components *c) { return c ? &c->res : nullptr; }
void stcsp_components_free(stcsp_components *c) { delete c; }

int stcsp_automaton_optimise(const stcsp_automaton *a, const stcsp_optimise_request *request, stcsp_optimise **out) {
    if (!a || !request || !out) return STCSP_E_INVALID;
    stcsp_optimise *h = nullptr;
    try {
        h = new stcsp_optimise();
        const auto t0 = std::chrono::steady_clock::now();
        if (int rc = h->o.run(generator_view(a->a), a->a.var_lb.data(), a->a.var_ub.data(), *request)) {
            delete h;
            return rc;
        }
        stcsp::HostOptimise &o = h->o;
        for (auto *v : {&o.best, &o.state_best, &o.witness_off, &o.comp_num, &o.comp_den}) v->reserve(1);  // (empty vectors still give valid pointers)
        for (auto *v : {&o.witness_values, &o.witness_states, &o.state_component}) v->reserve(1);
        memset(&h->res, 0, sizeof h->res);
        h->res.n_states = o.n_live;
        h->res.best = o.best.data();
        h->res.state_best = (request->flags & STCSP_OPT_STATE_BEST) ? o.state_best.data() : nullptr;
        h->res.n_witnesses = request->n_lengths;
        h->res.witness_off = o.witness_off.data();
        h->res.witness_values = o.witness_values.data();
        h->res.witness_states = o.witness_states.data();
        h->res.n_components = (int64_t)o.comp_num.size();
        h->res.state_component = (request->flags & STCSP_OPT_MEAN) ? o.state_component.data() : nullptr;
        h->res.comp_mean_num = o.comp_num.data();
        h->res.comp_mean_den = o.comp_den.data();
        h->res.omega_mean_num = o.omega_num;
        h->res.omega_mean_den = o.omega_den;
        h->res.omega_component = o.omega_component;
        h->res.n_vars = o.n_vars;
        h->res.horizon = request->horizon;
        h->res.largest_cyclic = o.largest_cyclic;
        h->res.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } catch (const std::bad_alloc &) {
        delete h;
        return STCSP_E_NOMEM;
    }
    *out = h;
    return STCSP_OK;
}
const stcsp_optimise_result *stcsp_optimise_get(const stcsp_optimise *o) { return o ? &o->res : nullptr; }
void stcsp_optimise_free(stcsp_optimise *o) { delete o; }

int stcsp_ctl_parse(const char *text, const stcsp_problem *problem, int32_t **program, int32_t *n_words, int32_t *error_pos, char *message,
                    size_t message_len) {
    if (!text || !problem || !program || !n_words) return STCSP_E_INVALID;
    *program = nullptr;
    *n_words = 0;
    try {
        stcsp::CtlParser parser(text, problem->n_vars, problem->var_names);
        if (!parser.parse()) {
            if (error_pos) *error_pos = (int32_t)parser.error_pos;
            if (message && message_len) snprintf(message, message_len, "%s", parser.error.c_str());
            return STCSP_E_INVALID;
        }
        int32_t *w = (int32_t *)malloc(parser.out.size() * sizeof(int32_t));
        if (!w) return STCSP_E_NOMEM;
        memcpy(w, parser.out.data(), parser.out.size() * sizeof(int32_t));
        *program = w;
        *n_words = (int32_t)parser.out.size();
    } catch (const std::bad_alloc &) {
        return STCSP_E_NOMEM;
    }
    return STCSP_OK;
}

int stcsp_automaton_ctl(const stcsp_automaton *a, const stcsp_ctl_request *request, stcsp_ctl **out) {
    if (!a || !request || !out) return STCSP_E_INVALID;
    stcsp_ctl *h = nullptr;
    try {
        h = new stcsp_ctl();
        const auto t0 = std::chrono::steady_clock::now();
        stcsp::CtlProgram prog;
        int rc = prog.build(request->program, request->n_words, a->a.n_vars);
        if (rc == STCSP_OK) rc = h->c.run(generator_view(a->a), prog, request->flags);
        if (rc != STCSP_OK) {
            delete h;
            return rc;
        }
        stcsp::HostCtl &c = h->c;
        c.edge_world.reserve(1);  // (empty vectors still give valid pointers)
        c.edge_sat.reserve(1);
        c.witness_values.reserve(1);
        memset(&h->res, 0, sizeof h->res);
        h->res.n_worlds = c.n_worlds;
        h->res.n_initial = c.n_initial;
        h->res.n_initial_sat = c.n_initial_sat;
        h->res.n_edges = (int64_t)c.edge_world.size();
        h->res.edge_world = c.edge_world.data();
        h->res.edge_sat = c.edge_sat.data();
        h->res.witness_values = c.witness_values.data();
        h->res.witness_kind = c.witness_kind;
        h->res.witness_len = c.witness_len;
        h->res.n_vars = c.n_vars;
        h->res.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } catch (const std::bad_alloc &) {
        delete h;
        return STCSP_E_NOMEM;
    }
    *out = h;
    return STCSP_OK;
}
const stcsp_ctl_result *stcsp_ctl_get(const stcsp_ctl *c) { return c ? &c->res : nullptr; }
void stcsp_ctl_free(stcsp_ctl *c) { delete c; }

char *stcsp_automaton_canonical(const stcsp_automaton *a, size_t *len) {
    if (!a) return nullptr;
    std::string s = a->a.canonical(nullptr, nullptr);
    char *p = (char *)malloc(s.size() + 1);
    memcpy(p, s.c_str(), s.size() + 1);
    if (len) *len = s.size();
    return p;
}
int64_t stcsp_automaton_num_states(const stcsp_automaton *a) { return a->a.table_states >= 0 ? a->a.table_states : a->a.n_states; }
int64_t stcsp_automaton_num_live_states(const stcsp_automaton *a) {
    int64_t ns = 0;
    a->a.canonical(&ns, nullptr, false);
    return ns;
}
int64_t stcsp_automaton_num_live_edges(const stcsp_automaton *a) {
    int64_t ne = 0;
    a->a.canonical(nullptr, &ne, false);
    return ne;
}

// Sharded runs: shard r's result holds its local states (index = local id) and the raw edge
// log of the leaves it committed, with global ids (owner << STCSP_GID_SHIFT | local) in
// edge_src / edge_dst. The root is local state 0 of shard 0.
int stcsp_merge_shards(const stcsp_result *const *shards, int n, stcsp_merged **out) {
    if (!shards || n <= 0 || !out) return STCSP_E_INVALID;
    stcsp_merged *h = new stcsp_merged();
    stcsp::Merged &m = h->m;
    std::vector<int64_t> off(n + 1, 0);
    for (int r = 0; r < n; r++) off[r + 1] = off[r] + shards[r]->n_states;
    const stcsp_result *s0 = shards[0];
    int sl = s0->sig_len, nv = s0->n_vars;
    stcsp_counters ctr{};
    int truncated = 0, nsets = 0;
    for (int r = 0; r < n; r++) {
        const stcsp_result *s = shards[r];
        m.cid.insert(m.cid.end(), s->state_cid, s->state_cid + s->n_states);
        m.sig.insert(m.sig.end(), s->state_sig, s->state_sig + s->n_states * (int64_t)sl);
        for (int64_t e = 0; e < s->n_edges; e++) {
            int64_t gs = s->edge_src[e], gd = s->edge_dst[e];
            m.esrc.push_back(off[gs >> STCSP_GID_SHIFT] + (gs & (((int64_t)1 << STCSP_GID_SHIFT) - 1)));
            m.edst.push_back(off[gd >> STCSP_GID_SHIFT] + (gd & (((int64_t)1 << STCSP_GID_SHIFT) - 1)));
        }
        m.eval.insert(m.eval.end(), s->edge_values, s->edge_values + s->n_edges * (int64_t)nv);
        ctr.search_nodes += s->counters.search_nodes;
        ctr.gac_calls += s->counters.gac_calls;
        ctr.fails += s->counters.fails;
        ctr.leaves += s->counters.leaves;
        ctr.revisions += s->counters.revisions;
        ctr.evaluations += s->counters.evaluations;
        if (s->counters.levels > ctr.levels) ctr.levels = s->counters.levels;
        if (s->counters.seconds_search > ctr.seconds_search) ctr.seconds_search = s->counters.seconds_search;
        if (s->counters.seconds_export > ctr.seconds_export) ctr.seconds_export = s->counters.seconds_export;
        truncated |= s->truncated;
        if (s->n_constraint_sets > nsets) nsets = s->n_constraint_sets;
    }
    std::vector<uint8_t> alive;
    stcsp::ok_fixpoint(off[n], m.esrc, m.edst, m.fail, alive);
    size_t w = 0;
    for (size_t e = 0; e < alive.size(); e++)
        if (alive[e]) {
            m.esrc[w] = m.esrc[e];
            m.edst[w] = m.edst[e];
            std::copy(m.eval.begin() + e * nv, m.eval.begin() + (e + 1) * nv, m.eval.begin() + w * nv);
            w++;
        }
    m.esrc.resize(w);
    m.edst.resize(w);
    m.eval.resize(w * nv);
    int64_t ok_states = 0;
    for (int64_t v = 1; v < off[n]; v++) ok_states += !m.fail[v];
    ctr.dominance = (int64_t)w - ok_states;
    m.issig.assign(s0->var_is_signature, s0->var_is_signature + nv);
    m.res = *s0;
    m.res.n_states = off[n];
    m.res.state_cid = m.cid.data();
    m.res.state_sig = m.sig.data();
    m.res.state_fail = m.fail.data();
    m.res.n_edges = (int64_t)w;
    m.res.edge_src = m.esrc.data();
    m.res.edge_dst = m.edst.data();
    m.res.edge_values = m.eval.data();
    m.res.var_is_signature = m.issig.data();
    {
        // Solver::seenConstraints holds the initial set and every set some leaf translated to, i.e. the distinct
        // set ids of the table's states (a shard's own registry may hold more: sets it translated ahead of need)
        std::set<int32_t> used(m.cid.begin(), m.cid.end());
        used.insert(0);
        nsets = (int32_t)used.size();
    }
    m.res.n_constraint_sets = nsets;
    m.res.truncated = truncated;
    m.res.counters = ctr;
    *out = h;
    return STCSP_OK;
}
const stcsp_result *stcsp_merged_result(const stcsp_merged *m) { return m ? &m->m.res : nullptr; }
void stcsp_merged_free(stcsp_merged *m) { delete m; }

}  // extern "C"
