"""The independent yardstick of the observer (tests only): a plain Python subset construction over the transition map of
monitor_ref.Yardstick (the automaton of the CPU oracle), numbered breadth-first with the out-edges of a set in label order.

Definition (include/stcsp_engine.h, stcsp_engine_observer): D_0 = {root}; delta(D, l) = the destinations of the live edges
that leave a member of D and project on l; the states are the sets reachable from D_0, final(D) = some member is final.
Results of an implementation are compared after mapping its members through quotient_ref.canonical_numbers: the list of
member sets in number order, the final flags and the edge list (src, row, dst) must be exactly equal."""
import numpy as np

import monitor_ref as M
import quotient_ref as Q


def subset_construction(y):
    """y: monitor_ref.Yardstick. Returns (sets, final, edges, levels): sets[i] = sorted canonical numbers of the members of
    observer state i, final[i] 0/1, edges = [(src, projected row, dst)] sorted by (src, row), levels = breadth-first levels."""
    if not y.live:
        return [], [], [], 0
    by_state = {}
    for (s, p), d in y.trans.items():
        by_state.setdefault(s, {})[p] = d
    root = frozenset([0])
    sets, number, depth, edges = [root], {root: 0}, [0], []
    q = 0
    while q < len(sets):
        succ = {}
        for s in sets[q]:
            for p, d in by_state.get(s, {}).items():
                succ.setdefault(p, set()).update(d)
        for p in sorted(succ):
            t = frozenset(succ[p])
            if t not in number:
                number[t] = len(sets)
                sets.append(t)
                depth.append(depth[q] + 1)
            edges.append((q, p, number[t]))
        q += 1
    final = [int(any(y.final[s] for s in d)) for d in sets]
    return [sorted(y.live[s] for s in d) for d in sets], final, edges, max(depth) + 1


def normalised(obs, numbers):
    """An implementation's observer (the dict of Engine.observer() / Automaton.observer()) in the yardstick's form; numbers:
    its state index -> canonical number (quotient_ref.canonical_numbers on its own automaton)."""
    off = obs["member_off"].tolist()
    member = obs["member"].tolist()
    sets = [sorted(numbers[s] for s in member[off[i]:off[i + 1]]) for i in range(obs["n_states"])]
    rows = obs["edge_values"].tolist()
    edges = [(s, tuple(r), d) for s, r, d in zip(obs["edge_src"].tolist(), rows, obs["edge_dst"].tolist())]
    return sets, obs["state_final"].tolist(), edges, obs["levels"]


def check_shape(obs):
    """What holds for every result: offsets, ascending members, edges sorted by (source, row) and deterministic."""
    ns, ne = obs["n_states"], obs["n_edges"]
    off = obs["member_off"]
    assert off.shape == (ns + 1,) and off[0] == 0 and (np.diff(off) > 0).all()
    assert obs["member"].shape == (int(off[-1]),) and obs["state_final"].shape == (ns,)
    for i in range(ns):
        assert (np.diff(obs["member"][off[i]:off[i + 1]]) > 0).all()
    assert obs["max_set"] == (int(np.diff(off).max()) if ns else 0)
    assert obs["edge_values"].shape == (ne, obs["n_observable"])
    keys = [(s, tuple(r)) for s, r in zip(obs["edge_src"].tolist(), obs["edge_values"].tolist())]
    assert keys == sorted(keys) and len(set(keys)) == ne
    if ns:
        assert obs["member"][:1].tolist() == [0] and off[1] == 1  # number 0 is {root}


def yardstick_for(RefOracle, model, mask, adversarial=None):
    """(oracle, its result, its automaton, monitor yardstick, subset construction) under one mask."""
    o = RefOracle(model)
    r = o.solve()
    a = o.automaton(r).traverse()
    if adversarial is not None:
        a.adversarial(adversarial)
    valid, final, alive = a.flags()
    y = M.Yardstick(r, valid, final, alive, mask)
    return o, r, a, y, subset_construction(y)


def numbers_of(r, valid, alive):
    return Q.canonical_numbers(Q.live_out_edges(r, valid, alive), bool(valid[0]))


def only(model, name):
    assert name in model.var_names
    return [int(n == name) for n in model.var_names]


def resolve_mask(model, which):
    """"default" | "all" | "only:NAME" -> one flag per variable."""
    if which == "default":
        return Q.default_mask(model.var_names)
    if which == "all":
        return [1] * model.n_vars
    return only(model, which.split(":", 1)[1])


CRAFTED = "var x:[0,%d]; var h:[0,%d]; next h == h; x <= h;"

# the table of the issue: (instance, mask) -> (live states, live edges, observer states, observer edges, largest set, levels)
TABLE = {
    ("juggling_b4_f5", "only:B0"): (121, 224, 621, 1041, 48, 30),
    ("digitinvader3", "only:D0"): (505, 2020, 489, 1933, 101, 27),
    ("digitinvader3", "only:D1"): (505, 2020, 897, 3501, 54, 24),
    ("digitinvader5", "only:D0"): (2773, 16638, 4585, 24733, 336, 36),
    ("digitinvader5", "only:D1"): (2773, 16638, 14239, 78751, 140, 36),
    ("partialorder_10", "default"): (1920, 28778, 1920, 28784, 2, 11),
    ("partialorder_10", "only:succ"): (1920, 28778, 20, 30, 1919, 11),
    ("partialorder_12", "only:seen0"): (7936, 142822, 34, 46, 7679, 13),
    ("crafted63", "only:x"): (65, 4160, 65, 4160, 64, 2),
}
