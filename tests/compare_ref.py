"""The independent yardstick of the comparison of two observable languages (tests only): a plain Python product over dicts of
two observer dicts (Engine.observer() / Automaton.observer()), and a brute-force check of its verdicts for tiny operands.

Definition (include/stcsp_engine.h, stcsp_engine_compare): each operand is completed with a sink that is not final and that
every missing (state, row) leads to; the product's states are the pairs other than (sink, sink) reachable from the pair of
the roots (the sink for an operand without states), one edge per row that a component has; pairs are numbered breadth-first
with the children of a pair in sorted row order; verdict k is the least-numbered pair that satisfies predicate k, and its
witness is the pair's access sequence, found by walking the parents."""
import numpy as np

SCALARS = ("n_pairs", "n_pair_edges", "levels", "n_observable")
ARRAYS = ("witness_off", "witness_len", "witness_left", "witness_right", "witness_values")
SINK = -1


def transitions(obs):
    """state -> {row: destination} of an observer dict."""
    out = {}
    for s, row, d in zip(obs["edge_src"].tolist(), obs["edge_values"].tolist(), obs["edge_dst"].tolist()):
        out.setdefault(s, {})[tuple(row)] = d
    return out


def predicates(l, r, lfin, rfin):
    fl = l != SINK and bool(lfin[l])
    fr = r != SINK and bool(rfin[r])
    return (l != SINK and r == SINK, r != SINK and l == SINK, fl and not fr, fr and not fl)


def product(left, right):
    """The dict an implementation must return (SCALARS and ARRAYS), from two observer dicts."""
    assert left["n_observable"] == right["n_observable"]
    n_obs = left["n_observable"]
    tl, tr = transitions(left), transitions(right)
    lfin, rfin = left["state_final"].tolist(), right["state_final"].tolist()
    root = (0 if left["n_states"] else SINK, 0 if right["n_states"] else SINK)
    pairs, number, parent, label, depth = [], {}, [], [], []
    if root != (SINK, SINK):
        pairs, number, parent, label, depth = [root], {root: 0}, [None], [None], [0]
    edges = q = 0
    while q < len(pairs):
        l, r = pairs[q]
        ol, orr = tl.get(l, {}), tr.get(r, {})
        for row in sorted(set(ol) | set(orr)):
            t = (ol.get(row, SINK), orr.get(row, SINK))
            if t not in number:
                number[t] = len(pairs)
                pairs.append(t)
                parent.append(q)
                label.append(row)
                depth.append(depth[q] + 1)
            edges += 1
        q += 1
    wlen, wleft, wright, witnesses = [-1] * 4, [-1] * 4, [-1] * 4, [[], [], [], []]
    for k in range(4):
        hit = next((i for i, (l, r) in enumerate(pairs) if predicates(l, r, lfin, rfin)[k]), None)
        if hit is None:
            continue
        wleft[k], wright[k] = pairs[hit]
        rows = []
        while parent[hit] is not None:
            rows.append(label[hit])
            hit = parent[hit]
        witnesses[k] = rows[::-1]
        wlen[k] = len(rows)
    off = np.cumsum([0] + [len(w) for w in witnesses]).astype(np.int64)
    values = np.array([row for w in witnesses for row in w], np.int32).reshape(int(off[4]), n_obs)
    return {"n_pairs": len(pairs), "n_pair_edges": edges, "levels": max(depth) + 1 if pairs else 0, "n_observable": n_obs, "witness_off": off,
            "witness_len": np.array(wlen, np.int32), "witness_left": np.array(wleft, np.int32), "witness_right": np.array(wright, np.int32),
            "witness_values": values}


def same(a, b):
    return all(a[k] == b[k] for k in SCALARS) and all(np.array_equal(a[k], b[k]) and a[k].shape == b[k].shape for k in ARRAYS)


def witness(cmp, k):
    """Witness k as a list of row tuples, or None when the inclusion holds."""
    if cmp["witness_len"][k] < 0:
        return None
    a, b = int(cmp["witness_off"][k]), int(cmp["witness_off"][k + 1])
    assert b - a == cmp["witness_len"][k]
    return [tuple(r) for r in cmp["witness_values"][a:b].tolist()]


def swapped(cmp):
    """What the comparison of the swapped operands must return."""
    order = [1, 0, 3, 2]
    ws = [witness(cmp, k) or [] for k in order]
    off = np.cumsum([0] + [len(w) for w in ws]).astype(np.int64)
    d = {k: cmp[k] for k in SCALARS}
    d.update(witness_off=off, witness_len=cmp["witness_len"][order], witness_left=cmp["witness_right"][order], witness_right=cmp["witness_left"][order],
             witness_values=np.array([row for w in ws for row in w], np.int32).reshape(int(off[4]), cmp["n_observable"]))
    return d


def languages(obs, bound):
    """Brute force: (P, F) of an observer dict up to `bound` rows, as sets of tuples of rows."""
    t, fin = transitions(obs), obs["state_final"].tolist()
    prefixes, finals = set(), set()
    level = {(): 0} if obs["n_states"] else {}
    for _ in range(bound + 1):
        prefixes |= set(level)
        finals |= {w for w, s in level.items() if fin[s]}
        level = {w + (row,): d for w, s in level.items() for row, d in t.get(s, {}).items()}
    return prefixes, finals


def check_by_brute_force(left, right, cmp, bound):
    """Each witness is the shortest, lexicographically least member of its set difference; a reported inclusion has no
    counterexample of up to `bound` rows."""
    (pl, fl), (pr, fr) = languages(left, bound), languages(right, bound)
    for k, diff in enumerate((pl - pr, pr - pl, fl - fr, fr - fl)):
        w = witness(cmp, k)
        if w is None:
            assert not diff, f"verdict {k}: the inclusion is reported, {min(diff, key=lambda x: (len(x), x))} refutes it"
        else:
            assert len(w) <= bound, "the bound of the brute force is too small for this witness"
            assert tuple(w) == min(diff, key=lambda x: (len(x), x)), f"verdict {k}"


def malformed(obs):
    """name -> a copy of the observer dict `obs` (at least two edges out of one state and two states) with one thing wrong."""
    def copy(**changes):
        d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in obs.items()}
        d.update(changes)
        return d
    src, dst, val = obs["edge_src"], obs["edge_dst"], obs["edge_values"]
    e = next(i for i in range(1, len(src)) if src[i] == src[i - 1])  # two edges of one source
    swap = list(range(len(src)))
    swap[e - 1], swap[e] = swap[e], swap[e - 1]
    bad = {"n_observable": copy(n_observable=obs["n_observable"] + 1, edge_values=np.concatenate([val, val[:, :1]], axis=1)),
           "dst out of range": copy(edge_dst=np.where(np.arange(len(dst)) == len(dst) - 1, obs["n_states"], dst).astype(np.int32)),
           "src negative": copy(edge_src=np.where(np.arange(len(src)) == 0, -1, src).astype(np.int32)),
           "rows not sorted": copy(edge_values=val[swap], edge_dst=dst[swap]),
           "sources not sorted": copy(edge_src=src[::-1].copy()),
           "duplicate (source, row)": copy(edge_values=np.where((np.arange(len(src)) == e)[:, None], val[e - 1], val).astype(np.int32))}
    return bad
