"""The plain bounds-consistency model of one search node (tests only): from the constraints as the front end normalises them, the
domains of every (time point, variable), the until-expire bits and the look-ahead K to (consistent, fixpoint domains), and the
classification of the fixpoint (fail / branch / leaf). It is what process_node_wide (dev_wide.hpp, W = 2 and 4) and the interval
revisions (dev_interval.hpp) state as their strength, enforcePointConsistencyAt as dev_wide.hpp:192-253 gives it:

  * a point constraint is a tree of tests/expr_ref.py, evaluated by its `evaluate`, revised at every point p < K (at point 0
    alone when it holds a `first`). One revision of one scope variable drops its least value while that has no support, then its
    greatest likewise; a support is a tuple of the other scope variables' current domains on which the constraint is non-zero.
    Values in between stay. strength="gac" removes every unsupported value (the textbook rule of oracle/frontier_model.cpp);
  * an arc A == next(B): A[p] and B[p + 1] both become their intersection, p + 1 < K;
  * X until Y: a check only -- with the expire bit clear and both fixed at point 0 it fails unless one of them is 1;
  * all of it iterated to the fixpoint. The rules are monotone and only ever shrink domains, so the fixpoint does not depend on
    the order of the revisions.

The supports of one revision are found by ONE enumeration of the constraint's solutions inside the current box: a variable's
least supported value is the least value it takes on a solution, and trimming one variable to its supported range removes no
solution, so revising the scope variables one after the other (the rule above, `revise_literal` below) gives the same domains
(tests/test_bounds_ref.py holds the two against each other). A constraint v == e with v not in e is enumerated over e's variables
alone -- v's supported values are the values of e inside v's domain -- which is what lets v be as wide as [INT_MIN, INT_MAX].

Constraints (a list, in the order of Model.constraint_string): ("point", tree)  ("arc", A, B)  ("until", X, Y); a tree may hold
("first", ("v", name)). `show` renders one as Model.constraint_string does, so that a test pins the front end's normalisation
instead of imitating it. Domains: a list indexed p * N + v of Python sets (bitset forms) or (lo, hi) pairs (interval form).

Plain Python, no numpy, no GPU."""
import itertools

from expr_ref import ROOT_COMPARE, evaluate

_memo = {}  # (tree, arrays' identity) -> {tuple of values: evaluate's result}: rows meet the same tuples parent after parent
MAX_TUPLES = 1 << 18  # one enumeration of the yardstick: rows are built to stay far below (a guard against a mis-built row)


# ------------------------------------------------------------------ rendering (frontend.cpp print_tree)
def show_tree(t, root=False) -> str:
    k = t[0]
    if k == "c":
        return str(t[1])
    if k == "v":
        return t[1]
    if k == "arr":
        return f"{t[1]}[{show_tree(t[2])}]"
    if k in ("abs", "not", "first"):
        return f"{k}({show_tree(t[1])})"
    if k == "if":
        return f"if ({show_tree(t[1])}) then ({show_tree(t[2])}) else ({show_tree(t[3])})"
    s = f"{show_tree(t[1])} {k} {show_tree(t[2])}"
    return s if root else f"({s})"


def show(con) -> str:
    if con[0] == "arc":
        return f"{con[1]} == next({con[2]})"
    if con[0] == "until":
        return f"{con[1]} until {con[2]}"
    assert con[0] == "point" and (con[1][0] in ROOT_COMPARE or con[1][0] == "->"), con
    return show_tree(con[1], root=True)


def scope_of(t, out=None) -> list:
    """Variables of a tree in first-occurrence order."""
    out = [] if out is None else out
    if t[0] == "v":
        if t[1] not in out:
            out.append(t[1])
    else:
        for x in t[1:]:
            if isinstance(x, tuple):
                scope_of(x, out)
    return out


def has_first(t) -> bool:
    return t[0] == "first" or any(isinstance(x, tuple) and has_first(x) for x in t[1:])


def strip_first(t):
    if t[0] == "first":
        return strip_first(t[1])
    return tuple(strip_first(x) if isinstance(x, tuple) else x for x in t)


# ------------------------------------------------------------------ domains: a set of ints or a (lo, hi) pair
def is_pair(d) -> bool:
    return isinstance(d, tuple)


def d_lo(d):
    return d[0] if is_pair(d) else min(d)


def d_hi(d):
    return d[1] if is_pair(d) else max(d)


def d_size(d) -> int:
    return d[1] - d[0] + 1 if is_pair(d) else len(d)


def d_values(d):
    return range(d[0], d[1] + 1) if is_pair(d) else sorted(d)


def d_has(d, x) -> bool:
    return d[0] <= x <= d[1] if is_pair(d) else x in d


def d_trim(d, lo, hi):
    """d between lo and hi (both supported values of d): the ends go, what lies between stays."""
    return (lo, hi) if is_pair(d) else {x for x in d if lo <= x <= hi}


def d_meet(a, b):
    """The intersection, None when empty."""
    if is_pair(a) and is_pair(b):
        lo, hi = max(a[0], b[0]), min(a[1], b[1])
        return (lo, hi) if lo <= hi else None
    if is_pair(a) or is_pair(b):
        raise TypeError("one domain form per block")
    m = a & b
    return m or None


# ------------------------------------------------------------------ one point constraint at one point
def solutions_by_variable(tree, scope, doms, arrays=None):
    """{variable: set of the values it takes on a solution of `tree` inside the box `doms` (name -> domain)}."""
    supp = {v: set() for v in scope}
    if tree[0] == "==":
        for side in (1, 2):
            v, e = tree[side], tree[3 - side]
            if v[0] != "v" or v[1] in scope_of(e):
                continue
            if e[0] == "v" and d_size(doms[e[1]]) > d_size(doms[v[1]]):
                continue  # two plain variables: the narrower one is enumerated (the other side of the loop takes it)
            inner = scope_of(e)
            n = 1
            for x in inner:
                n *= d_size(doms[x])
            assert n <= MAX_TUPLES, (show_tree(tree, True), n)
            memo = _memo.setdefault((e, id(arrays)), {})
            for combo in itertools.product(*(d_values(doms[x]) for x in inner)):
                values = dict(zip(inner, combo))
                if combo not in memo:
                    memo[combo] = evaluate(e, values, arrays)
                val, valid = memo[combo]
                if valid and d_has(doms[v[1]], val):
                    supp[v[1]].add(val)
                    for x, a in values.items():
                        supp[x].add(a)
            return supp
    n = 1
    for x in scope:
        n *= d_size(doms[x])
    assert n <= MAX_TUPLES, (show_tree(tree, True), n)
    memo = _memo.setdefault((tree, id(arrays)), {})
    for combo in itertools.product(*(d_values(doms[x]) for x in scope)):
        if combo not in memo:
            memo[combo] = evaluate(tree, dict(zip(scope, combo)), arrays)
        if memo[combo][0] != 0:
            for x, a in zip(scope, combo):
                supp[x].add(a)
    return supp


def revise(tree, doms, strength="bounds", arrays=None):
    """One revision of every scope variable of `tree`: the new domains (name -> domain) of those that changed, None on a wipe-out."""
    scope = scope_of(tree)
    supp = solutions_by_variable(tree, scope, doms, arrays)
    out = {}
    for v in scope:
        if not supp[v]:
            return None
        d = doms[v]
        if strength == "gac":
            assert not is_pair(d), "gac needs sets"
            new = set(supp[v])
        else:
            new = d_trim(d, min(supp[v]), max(supp[v]))
        if new != d:
            out[v] = new
    return out


def revise_literal(tree, doms, arrays=None):
    """The rule as it is stated, one scope variable after the other and one support search per dropped value (sets only): the
    cross-check of `revise`."""
    scope = scope_of(tree)
    doms = {v: set(doms[v]) for v in scope}

    def supported(v, a):
        others = [x for x in scope if x != v]
        for combo in itertools.product(*(sorted(doms[x]) for x in others)):
            values = dict(zip(others, combo))
            values[v] = a
            if evaluate(tree, values, arrays)[0] != 0:
                return True
        return False

    for v in scope:
        while doms[v] and not supported(v, min(doms[v])):
            doms[v].discard(min(doms[v]))
        while doms[v] and not supported(v, max(doms[v])):
            doms[v].discard(max(doms[v]))
        if not doms[v]:
            return None
    return doms


# ------------------------------------------------------------------ the node
def propagate(cons, names, domains, expire, K, strength="bounds", arrays=None):
    """(consistent, fixpoint domains). `expire`: the until-expire bits as one integer (bit u: until constraint u, in the order
    of `cons`, has expired). The input is not changed; the domains of a failed node are None."""
    N = len(names)
    at = {v: i for i, v in enumerate(names)}
    assert len(domains) == N * K
    dom = [set(d) if not is_pair(d) else d for d in domains]
    if any(d_size(d) <= 0 for d in dom):
        return False, None
    untils = [c for c in cons if c[0] == "until"]
    points = [(strip_first(c[1]), 1 if has_first(c[1]) else K) for c in cons if c[0] == "point"]
    arcs = [c for c in cons if c[0] == "arc"]
    changed = True
    while changed:
        changed = False
        for tree, npoints in points:
            scope = scope_of(tree)
            for p in range(npoints):
                new = revise(tree, {v: dom[p * N + at[v]] for v in scope}, strength, arrays)
                if new is None:
                    return False, None
                for v, d in new.items():
                    dom[p * N + at[v]] = d
                    changed = True
        for _, a, b in arcs:
            for p in range(K - 1):
                ia, ib = p * N + at[a], (p + 1) * N + at[b]
                m = d_meet(dom[ia], dom[ib])
                if m is None:
                    return False, None
                if m != dom[ia] or m != dom[ib]:
                    dom[ia], dom[ib] = m, (m if is_pair(m) else set(m))
                    changed = True
    for u, (_, x, y) in enumerate(untils):
        dx, dy = dom[at[x]], dom[at[y]]
        if not (expire >> u) & 1 and d_size(dx) == 1 and d_size(dy) == 1 and d_lo(dx) != 1 and d_lo(dy) != 1:
            return False, None
    return True, dom


def classify(ok, dom, n_vars):
    """("fail",) / ("leaf",) / ("branch", variable index, mid): a leaf has every time-0 variable fixed, a branch bisects the first
    open one in engine order at mid = lo + (hi - lo) // 2 -- the lower child keeps the values <= mid. (Bit positions are values
    minus the declared lower bound: the same midpoint; Python integers do not overflow.)"""
    if not ok:
        return ("fail",)
    for v in range(n_vars):
        if d_size(dom[v]) > 1:
            lo, hi = d_lo(dom[v]), d_hi(dom[v])
            return ("branch", v, lo + (hi - lo) // 2)
    return ("leaf",)


def split(dom, v, mid):
    """The two children of a branch: (lower, upper) blocks, differing in word (0, v) alone."""
    d = dom[v]
    low = (d[0], mid) if is_pair(d) else {x for x in d if x <= mid}
    up = (mid + 1, d[1]) if is_pair(d) else {x for x in d if x > mid}
    a, b = list(dom), list(dom)
    a[v], b[v] = low, up
    return a, b


def next_expire(cons, names, dom, expire) -> int:
    """The until rule of a leaf: a flag is set once Y has been 1 at time 0, and stays."""
    at = {v: i for i, v in enumerate(names)}
    for u, c in enumerate(c for c in cons if c[0] == "until"):
        if d_lo(dom[at[c[2]]]) == 1:
            expire |= 1 << u
    return expire


def brute_solutions(cons, names, domains, expire, K, arrays=None):
    """Every assignment of the whole block inside `domains` (sets) that satisfies every constraint as `propagate` reads it: the
    laws of tests/test_bounds_ref.py are stated against it. Small blocks only."""
    N = len(names)
    at = {v: i for i, v in enumerate(names)}
    out = []
    untils = [c for c in cons if c[0] == "until"]
    for combo in itertools.product(*(d_values(d) for d in domains)):
        good = True
        for c in cons:
            if c[0] == "point":
                tree = strip_first(c[1])
                for p in range(1 if has_first(c[1]) else K):
                    values = {v: combo[p * N + at[v]] for v in scope_of(tree)}
                    if evaluate(tree, values, arrays)[0] == 0:
                        good = False
            elif c[0] == "arc":
                for p in range(K - 1):
                    if combo[p * N + at[c[1]]] != combo[(p + 1) * N + at[c[2]]]:
                        good = False
            if not good:
                break
        for u, (_, x, y) in enumerate(untils):
            if good and not (expire >> u) & 1 and combo[at[x]] != 1 and combo[at[y]] != 1:
                good = False
        if good:
            out.append(combo)
    return out
