"""The independent yardstick of the fair CTL service (tests only): plain Python on the explicit world graph of the CPU oracle's
automaton. It shares nothing with the host twin or the device pass: it has its own parser, and it does NOT use the lowering
of include/stcsp_engine.h -- every operator is evaluated from its path definition.

Definition (include/stcsp_engine.h, stcsp_engine_ctl). A world is a live edge into an omega-live state (omega-liveness: the
yardstick of tests/components_ref.py); its successors are the worlds that leave its destination; a solution is an infinite
path of worlds that passes Fin worlds (final destination) infinitely often; every world starts one.
  EX f      some successor in f
  E[f U g]  a finite path inside f to a world of g (backward search; any finite path extends to a solution)
  EG f      the world reaches, inside the f-worlds, a cyclic strongly connected component of the f-restricted world graph that
            holds a Fin world (own Tarjan): exactly then a solution stays in f for ever
  AX f      no successor outside f                        AG f   no path to a world outside f
  AF f      no solution stays outside f for ever           A[f U g]  no solution avoids g for ever, and no path inside !g
                                                                     reaches a world outside both f and g
"""
import re
from collections import deque

import numpy as np

import components_ref as R
import quotient_ref as Q

OPS = {"==": lambda x, y: x == y, "!=": lambda x, y: x != y, "<": lambda x, y: x < y, "<=": lambda x, y: x <= y,
       ">": lambda x, y: x > y, ">=": lambda x, y: x >= y}
OP_ORDER = ("==", "!=", "<", "<=", ">", ">=")
UNARY = ("EX", "EF", "EG", "AX", "AF", "AG")
# the program tokens of include/stcsp_engine.h (the parser comparison needs them; the evaluation does not)
TOKEN = {"true": 1, "false": 2, "cmpc": 3, "cmpv": 4, "!": 10, "&": 11, "|": 12, "->": 13, "EX": 20, "EF": 21, "EG": 22, "EU": 23,
         "AX": 24, "AF": 25, "AG": 26, "AU": 27}


class ParseError(ValueError):
    def __init__(self, position, message):
        super().__init__(f"{position}: {message}")
        self.position = position


# ---------------------------------------------------------------------------------------------------------------- the parser
_TOKEN_RE = re.compile(r"\s*(->|==|!=|<=|>=|[<>!&|()\[\]]|[A-Za-z_][A-Za-z0-9_]*|[-+]?\d+)")


def tokens(text):
    out, pos = [], 0
    while True:
        m = _TOKEN_RE.match(text, pos)
        if not m:
            rest = text[pos:].lstrip()
            if rest:
                raise ParseError(len(text) - len(rest), f"unexpected '{rest[0]}'")
            return out
        out.append((m.group(1), m.start(1)))
        pos = m.end()


def parse(text, names):
    """Formula text -> a tree of tuples: ("true",) ("false",) ("cmp", var, op, ("int", k) | ("var", v)) ("!", f) ("&", f, g)
    ("|", f, g) ("->", f, g) ("EX", f) .. ("AG", f) ("EU", f, g) ("AU", f, g). Variables are indices into `names`."""
    toks = tokens(text) + [(None, len(text))]
    at = [0]

    def peek():
        return toks[at[0]][0]

    def take():
        at[0] += 1
        return toks[at[0] - 1]

    def expect(t):
        if peek() != t:
            raise ParseError(toks[at[0]][1], f"expected {t}")
        take()

    def var(name, pos):
        if name not in names:
            raise ParseError(pos, f"unknown variable '{name}'")
        return names.index(name)

    def implies():
        f = disj()
        if peek() == "->":
            take()
            return ("->", f, implies())
        return f

    def disj():
        f = conj()
        while peek() == "|":
            take()
            f = ("|", f, conj())
        return f

    def conj():
        f = unary()
        while peek() == "&":
            take()
            f = ("&", f, unary())
        return f

    def unary():
        t, pos = take()
        if t is None:
            raise ParseError(pos, "the formula ends where an operand is expected")
        if t == "!":
            return ("!", unary())
        if t == "(":
            f = implies()
            expect(")")
            return f
        if re.fullmatch(r"[A-Za-z_]\w*", t):
            if peek() in OPS:
                op, _ = take()
                rhs, rpos = take()
                if rhs is not None and re.fullmatch(r"[-+]?\d+", rhs):
                    k = int(rhs)
                    if not -2 ** 31 <= k < 2 ** 31:
                        raise ParseError(rpos, "the integer is outside int32")
                    return ("cmp", var(t, pos), op, ("int", k))
                if rhs is not None and re.fullmatch(r"[A-Za-z_]\w*", rhs):
                    return ("cmp", var(t, pos), op, ("var", var(rhs, rpos)))
                raise ParseError(rpos, "expected an integer or a variable")
            if t in ("true", "false"):
                return (t,)
            if t in UNARY:
                return (t, unary())
            if t in ("E", "A"):
                expect("[")
                f = implies()
                expect("U")
                g = implies()
                expect("]")
                return (t + "U", f, g)
            raise ParseError(pos, f"unknown word '{t}'")
        raise ParseError(pos, f"unexpected '{t}'")
    f = implies()
    if peek() is not None:
        raise ParseError(toks[at[0]][1], f"unexpected '{peek()}' after the formula")
    return f


def postfix(f):
    """The tree as the postfix words of stcsp_ctl_request."""
    if f[0] in ("true", "false"):
        return [TOKEN[f[0]]]
    if f[0] == "cmp":
        kind, arg = f[3]
        return [TOKEN["cmpc" if kind == "int" else "cmpv"], f[1], OP_ORDER.index(f[2]), arg]
    return [w for g in f[1:] for w in postfix(g)] + [TOKEN[f[0]]]


def show(f, names):
    """The tree as text the parsers read back."""
    if f[0] in ("true", "false"):
        return f[0]
    if f[0] == "cmp":
        return f"{names[f[1]]} {f[2]} {f[3][1] if f[3][0] == 'int' else names[f[3][1]]}"
    if f[0] == "!":
        return f"!({show(f[1], names)})"
    if f[0] in UNARY:
        return f"{f[0]} ({show(f[1], names)})"
    if f[0] in ("EU", "AU"):
        return f"{f[0][0]}[{show(f[1], names)} U {show(f[2], names)}]"
    return f"(({show(f[1], names)}) {f[0]} ({show(f[2], names)}))"


def random_formula(rng, n_vars, bounds, depth):
    """A random tree of depth <= `depth` over the variables' own value ranges. rng: random.Random."""
    if depth == 0 or rng.random() < 0.15:
        k = rng.random()
        if k < 0.08:
            return (rng.choice(["true", "false"]),)
        v = rng.randrange(n_vars)
        if k < 0.25 and n_vars > 1:
            return ("cmp", v, rng.choice(OP_ORDER), ("var", rng.randrange(n_vars)))
        lo, hi = bounds[v]
        return ("cmp", v, rng.choice(OP_ORDER), ("int", rng.randint(lo - 1, hi + 1)))
    op = rng.choice(["!", "&", "|", "->", "EX", "EF", "EG", "EU", "AX", "AF", "AG", "AU"])
    if op in ("&", "|", "->", "EU", "AU"):
        return (op, random_formula(rng, n_vars, bounds, depth - 1), random_formula(rng, n_vars, bounds, depth - 1))
    return (op, random_formula(rng, n_vars, bounds, depth - 1))


# ----------------------------------------------------------------------------------------------------------- the world graph
class Worlds:
    """The world graph of a Result under flags. eid[w]: the export edge of world w; succ / pred: lists of worlds; fin[w];
    rows[w]: the full row as a tuple; initial: the worlds out of the root."""

    def __init__(self, r, valid, final, alive):
        ref = R.yardstick(r, valid, final, alive)
        num = ref["num"]
        omega = {s for s in num if ref["omega"][num[s]]}
        src, dst, val = Q.result_arrays(r)
        rows = val.tolist()
        self.n_edges = r.n_edges
        self.eid = [e for e in range(r.n_edges) if alive[e] and int(src[e]) in omega and int(dst[e]) in omega]
        self.src = [int(src[e]) for e in self.eid]
        self.dst = [int(dst[e]) for e in self.eid]
        self.rows = [tuple(rows[e]) for e in self.eid]
        self.fin = [bool(final[d]) for d in self.dst]
        out = {}
        for w, s in enumerate(self.src):
            out.setdefault(s, []).append(w)
        self.succ = [out.get(d, []) for d in self.dst]
        self.pred = [[] for _ in self.eid]
        for w, ss in enumerate(self.succ):
            for x in ss:
                self.pred[x].append(w)
        self.initial = out.get(0, [])
        self.all = set(range(len(self.eid)))
        self.num = num
        assert all(self.succ), "a world without a successor"

    # ---- path statements
    def reach_through(self, through, targets):
        """The worlds with a finite path, all of whose worlds but the last lie in `through`, to a world of `targets`."""
        seen = set(targets)
        q = deque(seen)
        while q:
            v = q.popleft()
            for u in self.pred[v]:
                if u not in seen and u in through:
                    seen.add(u)
                    q.append(u)
        return seen

    def stays_for_ever(self, inside):
        """The worlds from which a solution stays in `inside` for ever."""
        succ = {w: [x for x in self.succ[w] if x in inside] for w in inside}
        comp = R.tarjan(sorted(inside), succ)
        members = {}
        for w, c in comp.items():
            members.setdefault(c, []).append(w)
        good = set()
        for c, ms in members.items():
            cyclic = len(ms) > 1 or ms[0] in succ[ms[0]]
            if cyclic and any(self.fin[w] for w in ms):
                good.update(ms)
        return self.reach_through(inside, good) & inside

    def sat(self, f):
        k = f[0]
        if k == "true":
            return set(self.all)
        if k == "false":
            return set()
        if k == "cmp":
            kind, arg = f[3]
            return {w for w in self.all if OPS[f[2]](self.rows[w][f[1]], arg if kind == "int" else self.rows[w][arg])}
        a = self.sat(f[1])
        if k == "!":
            return self.all - a
        if k == "EX":
            return {w for w in self.all if any(x in a for x in self.succ[w])}
        if k == "EF":
            return self.reach_through(self.all, a)
        if k == "EG":
            return self.stays_for_ever(a)
        if k == "AX":
            return {w for w in self.all if not any(x not in a for x in self.succ[w])}
        if k == "AF":
            return self.all - self.stays_for_ever(self.all - a)
        if k == "AG":
            return self.all - self.reach_through(self.all, self.all - a)
        b = self.sat(f[2])
        if k == "&":
            return a & b
        if k == "|":
            return a | b
        if k == "->":
            return (self.all - a) | b
        if k == "EU":
            return self.reach_through(a, b)
        assert k == "AU"
        not_g = self.all - b
        return self.all - (self.stays_for_ever(not_g) | (self.reach_through(not_g, not_g - a) & not_g) | (not_g - a))

    # ---- witnesses
    def witness_of(self, f):
        """(kind, rows) as the contract words it: a witness for a top EX / EF / E[U], a counterexample for a top AX / AG and for
        ! over EX / EF / E[U]; ("none", ()) otherwise and when no initial world qualifies."""
        k = f[0]
        if k in ("EX", "EF", "EU"):
            kind, g = "witness", f
        elif k == "AX":
            kind, g = "counterexample", ("EX", ("!", f[1]))
        elif k == "AG":
            kind, g = "counterexample", ("EF", ("!", f[1]))
        elif k == "!" and f[1][0] in ("EX", "EF", "EU"):
            kind, g = "counterexample", f[1]
        else:
            return "none", ()
        if g[0] == "EX":
            target = self.sat(g[1])
            paths = [(self.rows[w], self.rows[x]) for w in self.initial for x in self.succ[w] if x in target]
            return (kind, min(paths)) if paths else ("none", ())
        through, targets = (self.all, self.sat(g[1])) if g[0] == "EF" else (self.sat(g[1]), self.sat(g[2]))
        dist = {t: 0 for t in targets}
        q = deque(targets)
        while q:
            v = q.popleft()
            for u in self.pred[v]:
                if u not in dist and u in through:
                    dist[u] = dist[v] + 1
                    q.append(u)
        starts = [w for w in self.initial if w in dist]
        if not starts:
            return "none", ()
        least = min(dist[w] for w in starts)
        starts = [w for w in starts if dist[w] == least]
        # every shortest path, where there are few; a dictionary programme over the distances beyond
        count = {}
        for w in sorted(dist, key=dist.get):
            count[w] = 1 if dist[w] == 0 else sum(count[x] for x in self.succ[w] if dist.get(x) == dist[w] - 1)
        if sum(count[w] for w in starts) <= 20000:
            paths = []

            def walk(w, rows):
                rows = rows + (self.rows[w],)
                if dist[w] == 0:
                    paths.append(rows)
                    return
                for x in self.succ[w]:
                    if dist.get(x) == dist[w] - 1:
                        walk(x, rows)
            for w in starts:
                walk(w, ())
            return kind, min(paths)
        best = {}
        for w in sorted(dist, key=dist.get):
            if dist[w] <= least:
                best[w] = (self.rows[w],) + (min(best[x] for x in self.succ[w] if dist.get(x) == dist[w] - 1) if dist[w] else ())
        return kind, min(best[w] for w in starts)

    # ---- the result in the shape of the implementations
    def result(self, f, witness=False):
        s = self.sat(f)
        edge_world, edge_sat = np.zeros(self.n_edges, np.uint8), np.zeros(self.n_edges, np.uint8)
        edge_world[self.eid] = 1
        edge_sat[[self.eid[w] for w in s]] = 1
        d = dict(n_worlds=len(self.eid), n_initial=len(self.initial), n_initial_sat=sum(w in s for w in self.initial), edge_world=edge_world,
                 edge_sat=edge_sat, n_sat=len(s))
        if witness:
            d["witness"] = self.witness_of(f)
        return d


def same_verdict(res, ref):
    """An implementation's dict against the yardstick's result on the SAME Result (same edge indices)."""
    return (all(int(res[k]) == int(ref[k]) for k in ("n_worlds", "n_initial", "n_initial_sat")) and np.array_equal(res["edge_world"], ref["edge_world"])
            and np.array_equal(res["edge_sat"], ref["edge_sat"]))


def witness_rows(res):
    kind, rows = res["witness"]
    return kind, tuple(map(tuple, np.asarray(rows).tolist()))


def signature(r, valid, alive, res):
    """What a result says, in terms that do not depend on state or edge numbering: the counts and the set of (canonical number of
    the source state, full row) of the worlds and of the worlds the formula holds at."""
    num = Q.canonical_numbers(Q.live_out_edges(r, valid, alive), bool(r.n_states) and bool(valid[0]))
    src, _, val = Q.result_arrays(r)
    rows = val.tolist()

    def keyed(flags):
        return {(num[int(src[e])], tuple(rows[e])) for e in np.flatnonzero(flags).tolist()}
    return (int(res["n_worlds"]), int(res["n_initial"]), int(res["n_initial_sat"]), keyed(res["edge_world"]), keyed(res["edge_sat"]))


def same(a, b):
    """Two results of the implementations (device, host twin) on the same automaton: equal array by array, witness included."""
    if any(int(a[k]) != int(b[k]) for k in ("n_worlds", "n_initial", "n_initial_sat", "n_vars")):
        return False
    if a["witness"][0] != b["witness"][0] or not np.array_equal(a["witness"][1], b["witness"][1]):
        return False
    return np.array_equal(a["edge_world"], b["edge_world"]) and np.array_equal(a["edge_sat"], b["edge_sat"])
