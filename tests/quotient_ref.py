"""The independent yardstick of the bisimulation quotient (tests only): plain partition refinement over the automaton
of the CPU oracle, and the canonical state numbering that matches its states with the engine's.

Definition (include/stcsp_engine.h): the live automaton is the valid states the root reaches over alive edges; the
result is the coarsest partition in which two states share a class only if they have the same final flag and their
live out-edges give the same set of (projected label, class of destination)."""
import ctypes as C
from collections import deque

import numpy as np


def result_arrays(r):
    """(src, dst, values[E, N]) of a Result as numpy arrays (copies)."""
    E, N = r.n_edges, r.n_vars
    if E == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, N), np.int32)
    src = np.ctypeslib.as_array(r.edge_src, shape=(E,)).copy()
    dst = np.ctypeslib.as_array(r.edge_dst, shape=(E,)).copy()
    val = np.ctypeslib.as_array(r.edge_values, shape=(E * N,)).copy().reshape(E, N)
    return src, dst, val


def post_flags(post):
    """(valid, final, alive) bytes of a PostResult."""
    return (C.string_at(post.state_valid, post.n_states), C.string_at(post.state_final, post.n_states),
            C.string_at(post.edge_alive, post.n_edges) if post.n_edges else b"")


def live_out_edges(r, valid, alive):
    """state -> sorted list of (full label tuple, destination) over its alive edges into valid states."""
    src, dst, val = result_arrays(r)
    out = {}
    rows = val.tolist()
    for e in range(r.n_edges):
        if alive[e] and valid[dst[e]] and valid[src[e]]:
            out.setdefault(int(src[e]), []).append((tuple(rows[e]), int(dst[e])))
    for edges in out.values():
        edges.sort()
    return out


def canonical_numbers(out, root_valid):
    """tests/canon.py's numbering on the arrays: breadth-first from the root, out-edges in label order. With full labels
    the automaton is deterministic, so the numbering depends on nothing else. state -> number, live states only."""
    if not root_valid:
        return {}
    num = {0: 0}
    q = deque([0])
    while q:
        u = q.popleft()
        for _, v in out.get(u, ()):
            if v not in num:
                num[v] = len(num)
                q.append(v)
    return num


def coarsest_partition(states, final, pairs):
    """Plain partition refinement. pairs[s] = iterable of (label, destination). Returns (state -> class, rounds)."""
    cls = dict.fromkeys(states, 0)
    count, rounds = 0, 0
    while True:
        rounds += 1
        ids = {}
        new = {}
        for s in states:
            key = (cls[s], final[s], frozenset((l, cls[d]) for l, d in pairs.get(s, ())))
            new[s] = ids.setdefault(key, len(ids))
        cls = new
        if len(ids) == count:
            return cls, rounds
        count = len(ids)


def project(out, mask):
    """Out-edge lists with labels projected on the mask (one flag per variable) and interned as small integers."""
    keep = [i for i, m in enumerate(mask) if m]
    ids = {}
    return {s: [(ids.setdefault(tuple(lab[i] for i in keep), len(ids)), d) for lab, d in edges] for s, edges in out.items()}


def default_mask(names):
    return [0 if n.startswith("_V") else 1 for n in names]


def as_partition(classes_by_number):
    """{canonical number -> class label} -> tuple of class ids renumbered by first appearance in number order."""
    ren = {}
    return tuple(ren.setdefault(classes_by_number[k], len(ren)) for k in sorted(classes_by_number))


def yardstick(model, r, valid, final, alive, mask):
    """Partition of the live automaton of (r, flags) by the plain refinement, keyed by canonical number.
    Returns (partition tuple, number of classes, out-edge map, numbering, state -> class)."""
    out = live_out_edges(r, valid, alive)
    num = canonical_numbers(out, bool(valid[0]))
    states = sorted(num)
    cls, _ = coarsest_partition(states, {s: final[s] for s in states}, project({s: out.get(s, []) for s in states}, mask))
    return as_partition({num[s]: cls[s] for s in states}), len(set(cls.values())), out, num, cls


def engine_partition(r, valid, alive, state_class):
    """The partition an implementation returned (state_class indexed by ITS state index) keyed by canonical number."""
    out = live_out_edges(r, valid, alive)
    num = canonical_numbers(out, bool(valid[0]))
    live = {s for s in range(r.n_states) if state_class[s] >= 0}
    assert live == set(num), "the classes must cover exactly the live automaton"
    return as_partition({num[s]: int(state_class[s]) for s in num})


def quotient_counts(out, num, cls, mask):
    """(states, edges) of the quotient: classes, distinct (source class, projected label, destination class)."""
    keep = [i for i, m in enumerate(mask) if m]
    edges = {(cls[s], tuple(lab[i] for i in keep), cls[d]) for s in num for lab, d in out.get(s, ())}
    return len(set(cls.values())), len(edges)
