// ctl_host.hpp -- fair CTL over the infinite solutions, host side (contract: stcsp_engine.h, stcsp_engine_ctl; DESIGN.md
// section 4.23). Three parts:
//   CtlProgram   the request's postfix words checked, lowered to the basis {atoms, !, &, |, EX, EU, EG} and measured against
//                the limits. SHARED by the device pass (automaton.hip) and the twin: one lowering is the contract.
//   HostCtl      the host twin: the same fixpoints over one byte per world, the same witness rule. It shares the lowering and
//                the result struct with the device pass, nothing else.
//   ctl_parse    formula text -> postfix words (stcsp_ctl_parse of stcsp_host.h).
#pragma once
#include <algorithm>
#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "components_host.hpp"
#include "monitor_host.hpp"
#include "stcsp_engine.h"

namespace stcsp {

// a node of the lowered formula; kind is one of the basis tokens (TRUE, FALSE, CMP_CONST, CMP_VAR, NOT, AND, OR, EX, EU, EG)
struct CtlNode {
    int32_t kind = 0, a = -1, b = -1;  // children (a only for the unary ones)
    int32_t var = 0, op = 0, arg = 0;  // of a comparison
    bool temporal = false;             // an EX, EU or EG at or below this node
    int32_t slots = 1, depth = 1;      // sets held at once while this node is evaluated; stack depth of its postfix (temporal-free only)
};

struct CtlProgram {
    std::vector<CtlNode> nodes;
    int32_t root = -1;
    std::string error;

    static bool is_atom(int32_t k) { return k == STCSP_CTL_TRUE || k == STCSP_CTL_FALSE || k == STCSP_CTL_CMP_CONST || k == STCSP_CTL_CMP_VAR; }
    static bool compare(int32_t op, int32_t x, int32_t y) {
        switch (op) {
        case STCSP_CTL_OP_EQ: return x == y;
        case STCSP_CTL_OP_NE: return x != y;
        case STCSP_CTL_OP_LT: return x < y;
        case STCSP_CTL_OP_LE: return x <= y;
        case STCSP_CTL_OP_GT: return x > y;
        default: return x >= y;
        }
    }

    int fail(int code, const char *fmt, long long x = 0, long long y = 0) {
        char buf[256];
        snprintf(buf, sizeof buf, fmt, x, y);
        error = buf;
        return code;
    }
    // false: one node more than the limit
    bool push(int32_t kind, int32_t a = -1, int32_t b = -1, int32_t *out = nullptr) {
        if ((int)nodes.size() >= STCSP_CTL_MAX_NODES) return false;
        CtlNode n;
        n.kind = kind;
        n.a = a;
        n.b = b;
        nodes.push_back(n);
        if (out) *out = (int32_t)nodes.size() - 1;
        return true;
    }
    // a copy of the subtree at r (A[f U g] names g three times and f once more than written)
    bool clone(int32_t r, int32_t *out) {
        const CtlNode n = nodes[(size_t)r];
        int32_t a = -1, b = -1;
        if (n.a >= 0 && !clone(n.a, &a)) return false;
        if (n.b >= 0 && !clone(n.b, &b)) return false;
        if (!push(n.kind, a, b, out)) return false;
        nodes.back().var = n.var;
        nodes.back().op = n.op;
        nodes.back().arg = n.arg;
        return true;
    }

    // STCSP_OK, STCSP_E_INVALID (malformed) or STCSP_E_UNSUPPORTED (over a limit), with `error` set
    int build(const int32_t *w, int32_t n_words, int n_vars) {
        nodes.clear();
        root = -1;
        if (!w || n_words <= 0) return fail(STCSP_E_INVALID, "ctl: the program is empty");
        const char *too_many = "ctl: the lowered program has more than %lld atoms and operators";
        std::vector<int32_t> st;
        auto neg = [&](int32_t x, int32_t *out) { return push(STCSP_CTL_NOT, x, -1, out); };
        for (int32_t i = 0; i < n_words; i++) {
            const int32_t t = w[i];
            int32_t r = -1;
            bool ok = true;
            if (t == STCSP_CTL_TRUE || t == STCSP_CTL_FALSE) {
                ok = push(t, -1, -1, &r);
            } else if (t == STCSP_CTL_CMP_CONST || t == STCSP_CTL_CMP_VAR) {
                if (i + 3 >= n_words) return fail(STCSP_E_INVALID, "ctl: word %lld: an atom without its three operands", i);
                const int32_t var = w[i + 1], op = w[i + 2], arg = w[i + 3];
                if (var < 0 || var >= n_vars) return fail(STCSP_E_INVALID, "ctl: word %lld: variable index %lld is out of range", i + 1, var);
                if (op < STCSP_CTL_OP_EQ || op > STCSP_CTL_OP_GE) return fail(STCSP_E_INVALID, "ctl: word %lld: %lld is no comparison", i + 2, op);
                if (t == STCSP_CTL_CMP_VAR && (arg < 0 || arg >= n_vars))
                    return fail(STCSP_E_INVALID, "ctl: word %lld: variable index %lld is out of range", i + 3, arg);
                ok = push(t, -1, -1, &r);
                if (ok) {
                    nodes.back().var = var;
                    nodes.back().op = op;
                    nodes.back().arg = arg;
                }
                i += 3;
            } else if (t == STCSP_CTL_NOT || t == STCSP_CTL_EX || t == STCSP_CTL_EF || t == STCSP_CTL_EG || t == STCSP_CTL_AX || t == STCSP_CTL_AF ||
                       t == STCSP_CTL_AG) {
                if (st.empty()) return fail(STCSP_E_INVALID, "ctl: word %lld: stack underflow", i);
                const int32_t f = st.back();
                st.pop_back();
                int32_t x = -1, y = -1;
                switch (t) {
                case STCSP_CTL_NOT: ok = neg(f, &r); break;
                case STCSP_CTL_EX: ok = push(STCSP_CTL_EX, f, -1, &r); break;
                case STCSP_CTL_EG: ok = push(STCSP_CTL_EG, f, -1, &r); break;
                case STCSP_CTL_EF: ok = push(STCSP_CTL_TRUE, -1, -1, &x) && push(STCSP_CTL_EU, x, f, &r); break;
                case STCSP_CTL_AX: ok = neg(f, &x) && push(STCSP_CTL_EX, x, -1, &y) && neg(y, &r); break;
                case STCSP_CTL_AF: ok = neg(f, &x) && push(STCSP_CTL_EG, x, -1, &y) && neg(y, &r); break;
                default: {  // AG f = !E[true U !f]
                    int32_t tr = -1;
                    ok = neg(f, &x) && push(STCSP_CTL_TRUE, -1, -1, &tr) && push(STCSP_CTL_EU, tr, x, &y) && neg(y, &r);
                }
                }
            } else if (t == STCSP_CTL_AND || t == STCSP_CTL_OR || t == STCSP_CTL_IMPLIES || t == STCSP_CTL_EU || t == STCSP_CTL_AU) {
                if (st.size() < 2) return fail(STCSP_E_INVALID, "ctl: word %lld: stack underflow", i);
                const int32_t g = st.back(), f = st[st.size() - 2];
                st.resize(st.size() - 2);
                int32_t x = -1;
                if (t == STCSP_CTL_AND || t == STCSP_CTL_OR || t == STCSP_CTL_EU) {
                    ok = push(t, f, g, &r);
                } else if (t == STCSP_CTL_IMPLIES) {
                    ok = neg(f, &x) && push(STCSP_CTL_OR, x, g, &r);
                } else {  // A[f U g] = !E[!g U (!f & !g)] & !EG !g
                    int32_t g2 = -1, g3 = -1, ng = -1, nf = -1, ng2 = -1, both = -1, eu = -1, neu = -1, ng3 = -1, eg = -1, neg_eg = -1;
                    ok = clone(g, &g2) && clone(g, &g3) && neg(g, &ng) && neg(f, &nf) && neg(g2, &ng2) && push(STCSP_CTL_AND, nf, ng2, &both) &&
                         push(STCSP_CTL_EU, ng, both, &eu) && neg(eu, &neu) && neg(g3, &ng3) && push(STCSP_CTL_EG, ng3, -1, &eg) && neg(eg, &neg_eg) &&
                         push(STCSP_CTL_AND, neu, neg_eg, &r);
                }
            } else {
                return fail(STCSP_E_INVALID, "ctl: word %lld: unknown token %lld", i, t);
            }
            if (!ok) return fail(STCSP_E_UNSUPPORTED, too_many, STCSP_CTL_MAX_NODES);
            st.push_back(r);
        }
        if (st.size() != 1) return fail(STCSP_E_INVALID, "ctl: %lld operands are left over", (long long)st.size() - 1);
        root = st[0];
        return measure(root);
    }

    // temporal, slots and depth of every node below r, children first; the limits
    int measure(int32_t r) {
        CtlNode &n = nodes[(size_t)r];
        if (n.a >= 0)
            if (int rc = measure(n.a)) return rc;
        if (n.b >= 0)
            if (int rc = measure(n.b)) return rc;
        const CtlNode *a = n.a >= 0 ? &nodes[(size_t)n.a] : nullptr, *b = n.b >= 0 ? &nodes[(size_t)n.b] : nullptr;
        n.temporal = n.kind == STCSP_CTL_EX || n.kind == STCSP_CTL_EU || n.kind == STCSP_CTL_EG || (a && a->temporal) || (b && b->temporal);
        if (!n.temporal) {
            n.slots = 1;
            n.depth = !a ? 1 : !b ? a->depth : std::max(a->depth, b->depth + 1);
            if (n.depth > 64) return fail(STCSP_E_UNSUPPORTED, "ctl: a step predicate needs a stack of %lld, the limit is 64", n.depth);
            return STCSP_OK;
        }
        switch (n.kind) {
        case STCSP_CTL_NOT: n.slots = a->slots; break;
        case STCSP_CTL_EX: n.slots = std::max(a->slots, 2); break;  // (the witness keeps the operand)
        case STCSP_CTL_EG: n.slots = std::max(a->slots, 3); break;
        default: n.slots = std::max(a->slots, b->slots + 1);  // AND, OR, EU
        }
        if (n.slots > STCSP_CTL_MAX_SLOTS) return fail(STCSP_E_UNSUPPORTED, "ctl: the formula holds %lld sets of worlds at once, the limit is %lld", n.slots, STCSP_CTL_MAX_SLOTS);
        return STCSP_OK;
    }

    // the postfix slice of the temporal-free subtree at r, the words the step-predicate kernel interprets (tokens as in the request)
    void slice(int32_t r, std::vector<int32_t> &out) const {
        const CtlNode &n = nodes[(size_t)r];
        if (n.a >= 0) slice(n.a, out);
        if (n.b >= 0) slice(n.b, out);
        out.push_back(n.kind);
        if (n.kind == STCSP_CTL_CMP_CONST || n.kind == STCSP_CTL_CMP_VAR) {
            out.push_back(n.var);
            out.push_back(n.op);
            out.push_back(n.arg);
        }
    }
    // the temporal-free subtree at r on one full row
    bool holds(int32_t r, const int32_t *row) const {
        const CtlNode &n = nodes[(size_t)r];
        switch (n.kind) {
        case STCSP_CTL_TRUE: return true;
        case STCSP_CTL_FALSE: return false;
        case STCSP_CTL_CMP_CONST: return compare(n.op, row[n.var], n.arg);
        case STCSP_CTL_CMP_VAR: return compare(n.op, row[n.var], row[n.arg]);
        case STCSP_CTL_NOT: return !holds(n.a, row);
        case STCSP_CTL_AND: return holds(n.a, row) && holds(n.b, row);
        default: return holds(n.a, row) || holds(n.b, row);
        }
    }
    // where a witness comes from: the top node when it is EX or EU (*negated = false), its operand when the top is ! of one; -1: nowhere
    int32_t witness_node(bool *negated) const {
        const CtlNode &n = nodes[(size_t)root];
        *negated = false;
        if (n.kind == STCSP_CTL_EX || n.kind == STCSP_CTL_EU) return root;
        if (n.kind != STCSP_CTL_NOT) return -1;
        const int32_t k = nodes[(size_t)n.a].kind;
        *negated = true;
        return k == STCSP_CTL_EX || k == STCSP_CTL_EU ? n.a : -1;
    }
};

struct HostCtl {
    typedef std::vector<uint8_t> Set;
    int n_vars = 0;
    int64_t n_worlds = 0, n_initial = 0, n_initial_sat = 0;
    std::vector<uint8_t> edge_world, edge_sat;
    std::vector<int32_t> witness_values;
    int32_t witness_kind = STCSP_CTL_NONE, witness_len = 0;

    // the world graph: worlds in export order
    std::vector<int64_t> eid, first, last;  // the export edge of a world; the worlds out of dst(w) are [first[w], last[w]) of `by_src`
    std::vector<int64_t> by_src;
    std::vector<uint8_t> fin;
    const CtlProgram *prog = nullptr;
    const MonitorView *view = nullptr;
    int32_t wit = -1;                // the node whose fixpoint keeps its distances
    std::vector<int64_t> wit_dist;   // EU: the breadth-first distance to sat(g) inside sat(f), -1 outside the set
    Set wit_operand;                 // EX: sat(f)
    bool stuck = false;

    Set ex(const Set &z) const {
        Set r(z.size(), 0);
        for (size_t w = 0; w < z.size(); w++)
            for (int64_t k = first[w]; k < last[w] && !r[w]; k++) r[w] = z[(size_t)by_src[(size_t)k]];
        return r;
    }
    // the least fixpoint Z = g | (f & EX Z), level by level; dist (may be null) receives the level at which a world joined
    Set eu(const Set &f, const Set &g, std::vector<int64_t> *dist) {
        Set z = g;
        if (dist) {
            dist->assign(z.size(), -1);
            for (size_t w = 0; w < z.size(); w++)
                if (z[w]) (*dist)[w] = 0;
        }
        for (int64_t level = 1;; level++) {
            if (level > (int64_t)z.size() + 8) {
                stuck = true;
                return z;
            }
            const Set pre = ex(z);
            bool changed = false;
            for (size_t w = 0; w < z.size(); w++)
                if (!z[w] && f[w] && pre[w]) {
                    z[w] = 1;
                    changed = true;
                    if (dist) (*dist)[w] = level;
                }
            if (!changed) return z;
        }
    }
    Set eval(int32_t r) {
        const CtlNode &n = prog->nodes[(size_t)r];
        const size_t W = eid.size();
        if (!n.temporal) {
            Set s(W);
            for (size_t w = 0; w < W; w++) s[w] = prog->holds(r, view->values + eid[w] * n_vars);
            return s;
        }
        Set a = eval(n.a), b;
        if (n.b >= 0) b = eval(n.b);
        switch (n.kind) {
        case STCSP_CTL_NOT:
            for (auto &x : a) x = !x;
            return a;
        case STCSP_CTL_AND:
            for (size_t w = 0; w < W; w++) a[w] = a[w] && b[w];
            return a;
        case STCSP_CTL_OR:
            for (size_t w = 0; w < W; w++) a[w] = a[w] || b[w];
            return a;
        case STCSP_CTL_EX:
            if (r == wit) wit_operand = a;
            return ex(a);
        case STCSP_CTL_EU: return eu(a, b, r == wit ? &wit_dist : nullptr);
        default: {  // EG: Emerson-Lei
            Set z = a;
            for (int64_t round = 0;; round++) {
                if (round > (int64_t)W + 8) {
                    stuck = true;
                    return z;
                }
                Set t(W);
                for (size_t w = 0; w < W; w++) t[w] = z[w] && fin[w];
                const Set pre = ex(eu(a, t, nullptr));
                bool changed = false;
                for (size_t w = 0; w < W; w++) {
                    const uint8_t nz = a[w] && pre[w];
                    changed |= nz != z[w];
                    z[w] = nz;
                }
                if (!changed) return z;
            }
        }
        }
    }

    // STCSP_OK, or STCSP_E_INTERNAL (a fixpoint that did not converge; two equal full rows among the candidates of a witness step)
    int run(const MonitorView &a, const CtlProgram &p, int32_t flags) {
        const int64_t S = a.n_states, E = a.n_edges;
        const int N = n_vars = a.n_vars;
        prog = &p;
        view = &a;
        edge_world.assign((size_t)E, 0);
        edge_sat.assign((size_t)E, 0);
        HostComponents comp;
        if (!comp.run(a, 0, 0)) return STCSP_E_INTERNAL;
        const std::vector<uint8_t> &omega = comp.state_omega;
        // the worlds, and per state its out-worlds
        std::vector<int64_t> off((size_t)S + 1, 0);
        for (int64_t e = 0; e < E; e++)
            if (a.alive[e] && omega[(size_t)a.src[e]] && omega[(size_t)a.dst[e]]) {
                edge_world[(size_t)e] = 1;
                eid.push_back(e);
                off[(size_t)a.src[e] + 1]++;
            }
        const size_t W = eid.size();
        n_worlds = (int64_t)W;
        for (int64_t s = 0; s < S; s++) off[(size_t)s + 1] += off[(size_t)s];
        by_src.resize(W);
        {
            std::vector<int64_t> at(off.begin(), off.end() - 1);
            for (size_t w = 0; w < W; w++) by_src[(size_t)at[(size_t)a.src[eid[w]]]++] = (int64_t)w;
        }
        first.resize(W);
        last.resize(W);
        fin.resize(W);
        for (size_t w = 0; w < W; w++) {
            const int64_t v = a.dst[eid[w]];
            first[w] = off[(size_t)v];
            last[w] = off[(size_t)v + 1];
            fin[w] = a.final_[v];
        }
        bool negated = false;
        wit = (flags & STCSP_CTL_WITNESS) ? p.witness_node(&negated) : -1;
        const Set sat = eval(p.root);
        if (stuck) return STCSP_E_INTERNAL;
        for (size_t w = 0; w < W; w++) {
            edge_sat[(size_t)eid[w]] = sat[w];
            if (a.src[eid[w]] == 0) {
                n_initial++;
                n_initial_sat += sat[w];
            }
        }
        if (wit < 0 || W == 0) return STCSP_OK;
        // the walk: at every step the least full row among the candidates of the distance wanted
        const bool is_ex = p.nodes[(size_t)wit].kind == STCSP_CTL_EX;
        Set ex_set;
        if (is_ex) ex_set = ex(wit_operand);
        int64_t len = -1;  // in worlds
        for (int64_t k = off[0]; k < off[1]; k++) {
            const size_t w = (size_t)by_src[(size_t)k];
            if (is_ex ? ex_set[w] : wit_dist[w] >= 0) {
                const int64_t l = is_ex ? 2 : wit_dist[w] + 1;
                if (len < 0 || l < len) len = l;
            }
        }
        if (len < 0) return STCSP_OK;  // no initial world satisfies the EX / EU: neither witness nor counterexample
        int64_t lo = off[0], hi = off[1];
        for (int64_t rem = len; rem > 0; rem--) {
            int64_t best = -1;
            for (int64_t k = lo; k < hi; k++) {
                const size_t w = (size_t)by_src[(size_t)k];
                if (!(is_ex ? (rem == 2 ? ex_set[w] : wit_operand[w]) : wit_dist[w] == rem - 1)) continue;
                if (best < 0) {
                    best = (int64_t)w;
                    continue;
                }
                const int32_t *x = a.values + eid[w] * N, *y = a.values + eid[(size_t)best] * N;
                if (std::equal(x, x + N, y)) return STCSP_E_INTERNAL;
                if (std::lexicographical_compare(x, x + N, y, y + N)) best = (int64_t)w;
            }
            if (best < 0) return STCSP_E_INTERNAL;
            witness_values.insert(witness_values.end(), a.values + eid[(size_t)best] * N, a.values + (eid[(size_t)best] + 1) * N);
            lo = first[(size_t)best];
            hi = last[(size_t)best];
        }
        witness_len = (int32_t)len;
        witness_kind = negated ? STCSP_CTL_IS_COUNTEREXAMPLE : STCSP_CTL_IS_WITNESS;
        return STCSP_OK;
    }
};

// Formula text -> postfix words, by recursive descent (grammar: stcsp_host.h, stcsp_ctl_parse)
struct CtlParser {
    const char *s;
    size_t pos = 0;
    int n_vars;
    const char *const *names;
    std::vector<int32_t> out;
    std::string error;
    size_t error_pos = 0;

    CtlParser(const char *text, int n, const char *const *nm) : s(text), n_vars(n), names(nm) {}
    bool fail(size_t at, const std::string &what) {
        if (error.empty()) {
            error = what;
            error_pos = at;
        }
        return false;
    }
    void skip() {
        while (s[pos] && isspace((unsigned char)s[pos])) pos++;
    }
    static bool word_char(char c) { return isalnum((unsigned char)c) || c == '_'; }
    std::string peek_word() {
        skip();
        size_t e = pos;
        if (isalpha((unsigned char)s[e]) || s[e] == '_')
            while (word_char(s[e])) e++;
        return std::string(s + pos, e - pos);
    }
    bool eat(const char *lit) {
        skip();
        const size_t n = strlen(lit);
        if (strncmp(s + pos, lit, n) != 0) return false;
        pos += n;
        return true;
    }
    int find_var(const std::string &name) const {
        for (int v = 0; v < n_vars; v++)
            if (names && names[v] && name == names[v]) return v;
        return -1;
    }
    // -1: no comparison here
    int comparison() {
        skip();
        static const struct { const char *text; int op; } ops[] = {{"==", STCSP_CTL_OP_EQ}, {"!=", STCSP_CTL_OP_NE}, {"<=", STCSP_CTL_OP_LE},
                                                                   {">=", STCSP_CTL_OP_GE}, {"<", STCSP_CTL_OP_LT},  {">", STCSP_CTL_OP_GT}};
        for (const auto &o : ops)
            if (strncmp(s + pos, o.text, strlen(o.text)) == 0) {
                pos += strlen(o.text);
                return o.op;
            }
        return -1;
    }
    bool implies(int depth) {
        if (!disjunction(depth)) return false;
        skip();
        if (s[pos] == '-' && s[pos + 1] == '>') {
            pos += 2;
            if (!implies(depth)) return false;
            out.push_back(STCSP_CTL_IMPLIES);
        }
        return true;
    }
    bool disjunction(int depth) {
        if (!conjunction(depth)) return false;
        for (;;) {
            skip();
            if (s[pos] != '|') return true;
            pos++;
            if (!conjunction(depth)) return false;
            out.push_back(STCSP_CTL_OR);
        }
    }
    bool conjunction(int depth) {
        if (!unary(depth)) return false;
        for (;;) {
            skip();
            if (s[pos] != '&') return true;
            pos++;
            if (!unary(depth)) return false;
            out.push_back(STCSP_CTL_AND);
        }
    }
    bool until(int32_t token, int depth) {
        if (!implies(depth)) return false;
        const std::string w = peek_word();
        if (w != "U") return fail(pos, "expected U");
        pos += 1;
        if (!implies(depth)) return false;
        skip();
        if (s[pos] != ']') return fail(pos, "expected ]");
        pos++;
        out.push_back(token);
        return true;
    }
    bool unary(int depth) {
        if (depth > 200) return fail(pos, "the formula is nested too deeply");
        skip();
        const size_t at = pos;
        if (!s[pos]) return fail(pos, "the formula ends where an operand is expected");
        if (s[pos] == '!') {
            pos++;
            if (!unary(depth + 1)) return false;
            out.push_back(STCSP_CTL_NOT);
            return true;
        }
        if (s[pos] == '(') {
            pos++;
            if (!implies(depth + 1)) return false;
            skip();
            if (s[pos] != ')') return fail(pos, "expected )");
            pos++;
            return true;
        }
        const std::string w = peek_word();
        if (w.empty()) return fail(pos, std::string("unexpected '") + s[pos] + "'");
        pos += w.size();
        const size_t after = pos;
        const int op = comparison();
        if (op >= 0) {  // an atom: NAME op INT | NAME op NAME
            const int var = find_var(w);
            if (var < 0) return fail(at, "unknown variable '" + w + "'");
            skip();
            const size_t rhs = pos;
            const std::string w2 = peek_word();
            if (!w2.empty()) {
                const int var2 = find_var(w2);
                if (var2 < 0) return fail(rhs, "unknown variable '" + w2 + "'");
                pos += w2.size();
                out.insert(out.end(), {STCSP_CTL_CMP_VAR, var, op, var2});
                return true;
            }
            size_t e = pos;
            if (s[e] == '-' || s[e] == '+') e++;
            const size_t digits = e;
            long long value = 0;
            while (isdigit((unsigned char)s[e]) && e - digits < 12) value = value * 10 + (s[e++] - '0');
            if (e == digits) return fail(rhs, "expected an integer or a variable");
            if (isdigit((unsigned char)s[e])) return fail(rhs, "the integer is outside int32");
            if (s[pos] == '-') value = -value;
            if (value < INT32_MIN || value > INT32_MAX) return fail(rhs, "the integer is outside int32");
            pos = e;
            out.insert(out.end(), {STCSP_CTL_CMP_CONST, var, op, (int32_t)value});
            return true;
        }
        pos = after;
        if (w == "true" || w == "false") {
            out.push_back(w == "true" ? STCSP_CTL_TRUE : STCSP_CTL_FALSE);
            return true;
        }
        static const struct { const char *text; int32_t token; } prefix[] = {{"EX", STCSP_CTL_EX}, {"EF", STCSP_CTL_EF}, {"EG", STCSP_CTL_EG},
                                                                            {"AX", STCSP_CTL_AX}, {"AF", STCSP_CTL_AF}, {"AG", STCSP_CTL_AG}};
        for (const auto &p : prefix)
            if (w == p.text) {
                if (!unary(depth + 1)) return false;
                out.push_back(p.token);
                return true;
            }
        if (w == "E" || w == "A") {
            skip();
            if (s[pos] != '[') return fail(pos, "expected [ after " + w);
            pos++;
            return until(w == "E" ? STCSP_CTL_EU : STCSP_CTL_AU, depth + 1);
        }
        return fail(at, find_var(w) >= 0 ? "expected a comparison after '" + w + "'" : "unknown word '" + w + "'");
    }
    bool parse() {
        if (!implies(0)) return false;
        skip();
        if (s[pos]) return fail(pos, std::string("unexpected '") + s[pos] + "' after the formula");
        return true;
    }
};

}  // namespace stcsp
