"""The independent yardstick of the optimisation pass (tests only), in plain Python int and fractions.Fraction over the
out-edge lists of tests/quotient_ref.py on the automaton of the CPU oracle. It repeats neither implementation.

Definition (include/stcsp_engine.h, stcsp_engine_optimise): the cost of a live edge is the weighted sum of its full label
row; best[L] is the least total cost of a path of L live edges from the root (that ends in a final state under end_final),
with the lexicographically least such path as its witness; the mean of a cyclic component is the least mean cost per edge
of a cycle inside it.

  enumerate_paths    every live path of at most 6 steps from the root, where there are at most 20,000: least cost and
                     lexicographically least argmin per length
  dynamic_programme  the same for any horizon with dictionaries, and the greedy walk
  least_cycle_mean   every simple cycle of a component of at most 12 states
  check_certificate  for a component of any size and a claimed mean p/q: the costs q*c - p admit no negative cycle
                     (Bellman-Ford converges), the tight edges under the resulting potentials hold a cycle, gcd(p, q) == 1:
                     this verifies Karp's answer without repeating Karp"""
from fractions import Fraction
from math import gcd

NONE = 2 ** 63 - 1
MAX_PATHS = 20000
MAX_ENUM_LEN = 6
MAX_CYCLE_STATES = 12
MAX_CYCLES = 200000


def cost(weights, row):
    return sum(w * x for w, x in zip(weights, row))


def enumerate_paths(out, final, weights, end_final=False, root_live=True, max_len=MAX_ENUM_LEN):
    """{L: (least cost, its lexicographically least rows) or None} for L = 0 .. max_len, or None when the automaton has more
    than MAX_PATHS paths of at most max_len steps. out: state -> [(row, destination)] over the live edges."""
    res = {L: None for L in range(max_len + 1)}
    if not root_live:
        return res
    paths = [((), 0, 0)]  # (rows, end state, cost)
    total = 1
    for L in range(max_len + 1):
        for rows, s, c in paths:
            if end_final and not final[s]:
                continue
            if res[L] is None or (c, rows) < res[L]:
                res[L] = (c, rows)
        if L == max_len:
            break
        total += sum(len(out.get(s, ())) for _, s, _ in paths)
        if total > MAX_PATHS:  # (counted before the level is built: a level that is too long costs nothing)
            return None
        paths = [(rows + (row,), v, c + cost(weights, row)) for rows, s, c in paths for row, v in out.get(s, ())]
    return res


def dynamic_programme(out, states, final, weights, horizon, end_final=False):
    """V[k][s]: the least cost of k live edges from s (to a final state under end_final); states without such a path are absent."""
    V = [{s: 0 for s in states if not end_final or final[s]}]
    priced = {s: [(cost(weights, row), v) for row, v in out.get(s, ())] for s in states}
    for _ in range(horizon):
        prev, cur = V[-1], {}
        for s in states:
            cands = [c + prev[v] for c, v in priced[s] if v in prev]
            if cands:
                cur[s] = min(cands)
        V.append(cur)
    return V


def greedy_witness(out, V, weights, length):
    """The rows and the entered states of the lexicographically least path of `length` steps from the root that attains V[length][0]."""
    rows, visited, s = [], [], 0
    for left in range(length, 0, -1):
        tight = sorted((row, v) for row, v in out[s] if v in V[left - 1] and cost(weights, row) + V[left - 1][v] == V[left][s])
        assert len(tight) == 1 or tight[0][0] != tight[1][0], "two out-edges of one state with the same full row"
        rows.append(tight[0][0])
        s = tight[0][1]
        visited.append(s)
    return tuple(rows), visited


def component_edges(out, members, weights):
    """(u, v) -> the least cost of a live edge from u to v, both in `members`."""
    inside, edges = set(members), {}
    for u in members:
        for row, v in out.get(u, ()):
            if v in inside:
                c = cost(weights, row)
                if (u, v) not in edges or c < edges[u, v]:
                    edges[u, v] = c
    return edges


def least_cycle_mean(out, members, weights):
    """The least mean of a simple cycle of the component (a Fraction), None without a cycle or beyond the limits."""
    if len(members) > MAX_CYCLE_STATES:
        return None
    edges = component_edges(out, members, weights)
    succ = {}
    for (u, v), c in edges.items():
        succ.setdefault(u, []).append((v, c))
    best, seen = None, 0
    for start in sorted(members):  # the cycles whose least state is `start`
        stack = [(start, 0, 0, frozenset([start]))]
        while stack:
            u, total, n, on = stack.pop()
            for v, c in succ.get(u, ()):
                if v == start:
                    seen += 1
                    if seen > MAX_CYCLES:
                        return None
                    m = Fraction(total + c, n + 1)
                    best = m if best is None or m < best else best
                elif v > start and v not in on:
                    stack.append((v, total + c, n + 1, on | {v}))
    return best


def check_certificate(out, members, weights, p, q):
    """Asserts that p/q is the minimum cycle mean of the component."""
    assert q > 0 and gcd(abs(p), q) == 1, (p, q)
    edges = {e: q * c - p for e, c in component_edges(out, members, weights).items()}
    pot = {s: 0 for s in members}
    for _ in range(len(members) + 1):
        changed = False
        for (u, v), c in edges.items():
            if pot[u] + c < pot[v]:
                pot[v] = pot[u] + c
                changed = True
        if not changed:
            break
    assert not changed, f"a cycle of mean below {p}/{q}"
    tight = {}
    for (u, v), c in edges.items():
        if pot[u] + c == pot[v]:
            tight.setdefault(u, []).append(v)
    # a cycle among the tight edges: peel the states without a tight out-edge into what is left
    left = set(members)
    while True:
        gone = {s for s in left if not any(v in left for v in tight.get(s, ()))}
        if not gone:
            break
        left -= gone
    assert left, f"no cycle of mean {p}/{q}"


def yardstick(comp_ref, final, weights, horizon, end_final=False, maximise=False):
    """best [horizon + 1] (NONE where there is no prefix), the tables V, and per length <= 6 the enumeration's (cost, rows) or None.
    comp_ref: the yardstick of tests/components_ref.py (its out-edge lists and live states). maximise: the sign convention of the
    contract -- the weights are negated, and the caller negates the costs back."""
    w = [-x for x in weights] if maximise else list(weights)
    out, states = comp_ref["out"], sorted(comp_ref["num"])
    V = dynamic_programme(out, states, final, w, horizon, end_final)
    best = [V[L].get(0, NONE) if states else NONE for L in range(horizon + 1)]
    brute = enumerate_paths(out, final, w, end_final, bool(states), min(horizon, MAX_ENUM_LEN))
    if brute is not None:
        for L, hit in brute.items():
            assert (best[L] == NONE) == (hit is None) and (hit is None or hit[0] == best[L]), L
    return best, V, brute, w
