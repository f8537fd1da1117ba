"""The independent yardstick of the component pass (tests only): a plain recursive-free Tarjan, the component flags,
omega-liveness and the greedy lassos, over the out-edge lists of tests/quotient_ref.py on the automaton of the CPU oracle.

Definition (include/stcsp_engine.h, stcsp_engine_components): the strongly connected components of the live automaton over
its live edges; a component is CYCLIC with more than one state or a self-loop, FINAL with a final state, BOTTOM when no
edge leaves it, ACCEPTING when CYCLIC and FINAL; a state is omega-live when it reaches an accepting component; the lasso of
an accepting component is the shortest, lexicographically least stem from the root to a final state of it, and the
shortest, lexicographically least loop from that state back to it inside the component."""
from collections import deque

import numpy as np

import quotient_ref as Q

CYCLIC, FINAL, BOTTOM, ACCEPTING = 1, 2, 4, 8


def tarjan(states, succ):
    """state -> a representative of its strongly connected component. succ[s] = list of successor states."""
    index, low, comp, on, stack = {}, {}, {}, set(), []
    for root in states:
        if root in index:
            continue
        index[root] = low[root] = len(index)
        stack.append(root)
        on.add(root)
        call = [(root, iter(succ.get(root, ())))]
        while call:
            u, it = call[-1]
            for v in it:
                if v not in index:
                    index[v] = low[v] = len(index)
                    stack.append(v)
                    on.add(v)
                    call.append((v, iter(succ.get(v, ()))))
                    break
                if v in on:
                    low[u] = min(low[u], index[v])
            else:
                call.pop()
                if call:
                    low[call[-1][0]] = min(low[call[-1][0]], low[u])
                if low[u] == index[u]:
                    while True:
                        w = stack.pop()
                        on.discard(w)
                        comp[w] = u
                        if w == u:
                            break
    return comp


def bfs_depth(out, root=0):
    depth = {root: 0}
    q = deque([root])
    while q:
        u = q.popleft()
        for _, v in out.get(u, ()):
            if v not in depth:
                depth[v] = depth[u] + 1
                q.append(v)
    return depth


def yardstick(r, valid, final, alive, lassos=False, bottom_only=False):
    """Everything the contract fixes, keyed by nothing that depends on state indices:
    counts: dict of n_states, n_edges, n_components, n_cyclic, n_accepting, n_bottom, largest, n_omega, root_omega
    partition: the components as a partition of the canonical state numbers (Q.as_partition)
    omega: tuple of 0/1 by canonical number
    profile: sorted list of (size, depth, flags) over the components
    lassos: set of (stem rows, loop rows), rows as tuples (None unless asked for)
    plus the working data: out, num (state -> canonical number), comp (state -> representative), depth."""
    out = Q.live_out_edges(r, valid, alive)
    num = Q.canonical_numbers(out, bool(r.n_states) and bool(valid[0]))
    states = sorted(num)
    out = {s: out.get(s, []) for s in states}
    succ = {s: [v for _, v in out[s]] for s in states}
    comp = tarjan(states, succ)
    depth = bfs_depth(out) if states else {}
    members = {}
    for s in states:
        members.setdefault(comp[s], []).append(s)
    flags = {}
    for c, ms in members.items():
        f = BOTTOM
        if any(final[s] for s in ms):
            f |= FINAL
        for s in ms:
            for v in succ[s]:
                if comp[v] == c:
                    f |= CYCLIC
                else:
                    f &= ~BOTTOM
        if f & CYCLIC and f & FINAL:
            f |= ACCEPTING
        flags[c] = f
    pred = {}
    for s in states:
        for v in succ[s]:
            pred.setdefault(v, []).append(s)
    omega = {s for s in states if flags[comp[s]] & ACCEPTING}
    work = list(omega)
    while work:
        v = work.pop()
        for u in pred.get(v, ()):
            if u not in omega:
                omega.add(u)
                work.append(u)
    counts = dict(n_states=len(states), n_edges=sum(len(e) for e in out.values()), n_components=len(members),
                  n_cyclic=sum(bool(f & CYCLIC) for f in flags.values()), n_accepting=sum(bool(f & ACCEPTING) for f in flags.values()),
                  n_bottom=sum(bool(f & BOTTOM) for f in flags.values()), largest=max((len(m) for m in members.values()), default=0),
                  n_omega=len(omega), root_omega=int(0 in omega))
    res = dict(counts=counts, partition=Q.as_partition({num[s]: comp[s] for s in states}),
               omega=tuple(int(s in omega) for s in sorted(states, key=num.get)),
               profile=sorted((len(ms), min(depth[s] for s in ms), flags[c]) for c, ms in members.items()),
               lassos=None, out=out, num=num, comp=comp, depth=depth, flags=flags, members=members)
    if lassos:
        res["lassos"] = {lasso(out, pred, depth, final, ms) for c, ms in members.items()
                         if flags[c] & ACCEPTING and (not bottom_only or flags[c] & BOTTOM)}
    return res


def least_path(out, pred, start, targets, inside=None, at_least_one=False):
    """The shortest, lexicographically least row sequence from `start` to a state of `targets` (over states of `inside`), and its
    end state: backward distances to the targets, then the greedy walk. Labels are deterministic per state, so greedy is exact."""
    dist = {t: 0 for t in targets}
    q = deque(targets)
    while q:
        v = q.popleft()
        for u in pred.get(v, ()):
            if u not in dist and (inside is None or u in inside):
                dist[u] = dist[v] + 1
                q.append(u)

    def steps(s):  # (label, destination, what is left after it) over the usable out-edges
        return [(lab, v, dist[v]) for lab, v in out[s] if (inside is None or v in inside) and v in dist]
    rows, u = [], start
    left = 1 + min(d for _, _, d in steps(u)) if at_least_one else dist[start]
    while left > 0:
        cands = sorted((lab, v) for lab, v, d in steps(u) if d == left - 1)
        assert len(cands) == 1 or cands[0][0] != cands[1][0], "two out-edges of one state with the same full row"
        rows.append(cands[0][0])
        u = cands[0][1]
        left -= 1
    return tuple(rows), u


def lasso(out, pred, depth, final, ms):
    finals = [s for s in ms if final[s]]
    least = min(depth[s] for s in finals)
    stem, anchor = least_path(out, pred, 0, [s for s in finals if depth[s] == least])
    assert len(stem) == least and anchor in finals
    loop, end = least_path(out, pred, anchor, [anchor], inside=set(ms), at_least_one=True)
    assert end == anchor and len(loop) >= 1
    return stem, loop


def result_lassos(res):
    """The lassos of an implementation's result as the yardstick's set of (stem rows, loop rows)."""
    return {(tuple(map(tuple, stem.tolist())), tuple(map(tuple, loop.tolist()))) for _, stem, loop in res["lassos"]}


def check_result(r, valid, alive, res, ref, same_numbering=True):
    """An implementation's result (the dict of Engine.components() / Automaton.components(), indexed by the state indices of ITS
    Result r) against the yardstick `ref`, everything but the lassos. same_numbering: `ref` was computed on the same Result, so the
    components can be compared one by one; otherwise through the canonical numbers and as a multiset of (size, depth, flags)."""
    sc, om = res["state_component"], res["state_omega"]
    c = ref["counts"]
    got = {k: int(res[k]) for k in ("n_states", "n_components", "n_cyclic", "n_accepting", "n_bottom", "n_omega", "root_omega")}
    assert got == {k: c[k] for k in got}
    assert Q.engine_partition(r, valid, alive, sc) == ref["partition"]
    num = Q.canonical_numbers(Q.live_out_edges(r, valid, alive), bool(r.n_states) and bool(valid[0]))
    assert tuple(int(om[s]) for s in sorted(num, key=num.get)) == ref["omega"]
    assert not om[sc < 0].any()
    # numbered by least member
    firsts = [int(np.flatnonzero(sc == k)[0]) for k in range(got["n_components"])]
    assert firsts == sorted(firsts)
    assert sorted(zip(res["comp_size"].tolist(), res["comp_depth"].tolist(), res["comp_flags"].tolist())) == ref["profile"]
    for k in range(got["n_components"] if same_numbering else 0):  # ... and per component, not only as a multiset
        ms = np.flatnonzero(sc == k).tolist()
        rep = ref["comp"][ms[0]]
        assert sorted(ms) == sorted(ref["members"][rep]) and res["comp_size"][k] == len(ms)
        assert res["comp_depth"][k] == min(ref["depth"][s] for s in ms) and res["comp_flags"][k] == ref["flags"][rep]


def same(a, b):
    """Two results of the implementations (device, host twin) on the same automaton: equal array by array, lassos included."""
    keys = ("n_states", "n_components", "n_cyclic", "n_accepting", "n_bottom", "n_omega", "root_omega", "n_lassos", "n_vars")
    if any(int(a[k]) != int(b[k]) for k in keys):
        return False
    if any(not np.array_equal(a[k], b[k]) for k in ("state_component", "state_omega", "comp_size", "comp_depth", "comp_flags")):
        return False
    return all(x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) for x, y in zip(a["lassos"], b["lassos"]))
