"""Optimal solution streams, host side (include/stcsp_host.h: stcsp_automaton_optimise): the CPU twin of the device pass
against an independent yardstick -- the enumeration, dictionary programme, cycle enumeration and certificate check of
tests/optimise_ref.py, run on the automaton of the CPU oracle. The device pass itself: tests/test_optimise_gpu.py."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import components_ref as CR
import optimise_ref as R
from test_components import LADDER, TABLE, edited_flags, oracle_case

NONE = R.NONE
HORIZONS = (0, 1, 9)


def small_weights(n):
    """Small, of mixed signs."""
    return [(i * 7 + 3) % 5 - 2 for i in range(n)]


def big_weights(n):
    """About 2^30, of mixed signs: the costs leave 32 bits."""
    return [(-1) ** i * (2 ** 30 - 977 * i) for i in range(n)]


def rows_of(rows):
    return tuple(map(tuple, rows.tolist()))


def check_finite(a, ref, final, w, maximise, end_final, res_of=None):
    """The implementation (a.optimise, or res_of(**kwargs)) == the yardstick for the horizons 0, 1 and 9: best, state_best, witnesses."""
    run = res_of or (lambda **kw: a.optimise(w, **kw))
    best, V, brute, wmin = R.yardstick(ref, final, w, max(HORIZONS), end_final, maximise)
    sign = -1 if maximise else 1
    for horizon in HORIZONS:
        lengths = sorted({0, 1, 6, horizon} & set(range(horizon + 1)))
        res = run(horizon=horizon, lengths=lengths, maximise=maximise, end_final=end_final, state_best=True)
        assert res["best"].tolist() == [NONE if b == NONE else sign * b for b in best[:horizon + 1]]
        assert res["n_states"] == len(ref["num"]) and res["horizon"] == horizon and res["n_components"] == 0 and res["comp_mean"] == []
        assert res["omega_mean"] == (0, 0) and res["omega_component"] == -1 and res["state_component"] is None
        sb = res["state_best"]
        assert [int(s) for s in np.flatnonzero(sb != NONE)] == sorted(V[horizon]) and all(sb[s] == sign * c for s, c in V[horizon].items())
        assert [length for length, _, _ in res["witnesses"]] == lengths
        for length, rows, states in res["witnesses"]:
            if best[length] == NONE:
                assert len(rows) == 0 and len(states) == 0
                continue
            want_rows, want_states = R.greedy_witness(ref["out"], V, wmin, length)
            assert rows_of(rows) == want_rows and states.tolist() == want_states
            assert sign * sum(R.cost(wmin, row) for row in rows.tolist()) == res["best"][length]  # its cost, recomputed from its rows
            if brute is not None and length <= R.MAX_ENUM_LEN:
                assert brute[length] == (best[length], want_rows)  # the lexicographically least argmin of the enumeration
        wit = [rows for length, rows, _ in res["witnesses"] if best[length] != NONE and length > 0]
        if wit:
            acc, nend, fin, _ = a.check_streams(wit, "all")
            assert acc.tolist() == [len(x) for x in wit] and nend.tolist() == [1] * len(wit)  # accepted whole
            assert not end_final or fin.tolist() == [1] * len(wit)
        if not res_of:  # two rows instead of horizon + 1 give the same
            plain = a.optimise(w, horizon=horizon, maximise=maximise, end_final=end_final)
            assert plain["best"].tolist() == res["best"].tolist() and plain["witnesses"] == [] and plain["state_best"] is None


def check_mean(a, ref, w, comps=None, res_of=None):
    """The component means == the yardstick: the numbering of components(), the cycle enumeration, the certificate, omega."""
    res = res_of(mean=True) if res_of else a.optimise(w, mean=True)
    comps = comps or a.components("all")
    assert res["n_components"] == comps["n_components"] and np.array_equal(res["state_component"], comps["state_component"])
    assert res["best"].tolist() == [0 if ref["num"] else NONE]
    sc = comps["state_component"]
    largest = 0
    for c, (p, q) in enumerate(res["comp_mean"]):
        members = np.flatnonzero(sc == c).tolist()
        if not comps["comp_flags"][c] & CR.CYCLIC:
            assert (p, q) == (0, 0)
            continue
        largest = max(largest, len(members))
        R.check_certificate(ref["out"], members, w, p, q)
        least = R.least_cycle_mean(ref["out"], members, w)
        assert least is None or least == Fraction(p, q)
    assert res["largest_cyclic"] == largest
    accepting = [(Fraction(*res["comp_mean"][c]), c) for c in range(res["n_components"]) if comps["comp_flags"][c] & CR.ACCEPTING]
    if accepting:
        m, c = min(accepting)
        assert res["omega_mean"] == (m.numerator, m.denominator) and res["omega_component"] == c
    else:
        assert res["omega_mean"] == (0, 0) and res["omega_component"] == -1
    for c, _, loop in comps["lassos"]:  # the lasso's loop is a cycle of the component
        assert Fraction(*res["comp_mean"][c]) <= Fraction(sum(R.cost(w, row) for row in loop.tolist()), len(loop))
    return res


def check_host_twin(stcsp, RefOracle, name, adversarial=None, prefix_k=2):
    m, r, a, (valid, final, alive), ref, _ = oracle_case(stcsp, RefOracle, name, adversarial, prefix_k)
    for w in (small_weights(m.n_vars), big_weights(m.n_vars)):
        for maximise in (False, True):
            for end_final in (False, True):
                check_finite(a, ref, final, w, maximise, end_final)
        res = check_mean(a, ref, w)
        neg = a.optimise([-x for x in w], mean=True, maximise=True)  # MAXIMISE(w) == -MINIMISE(-w)
        assert neg["comp_mean"] == [(-p, q) for p, q in res["comp_mean"]] and neg["omega_mean"] == (-res["omega_mean"][0], res["omega_mean"][1])
        assert neg["omega_component"] == res["omega_component"]
        both = a.optimise(w, horizon=9, lengths=[9], mean=True, state_best=True)  # everything in one call
        alone = a.optimise(w, horizon=9, lengths=[9], state_best=True)
        assert both["comp_mean"] == res["comp_mean"] and both["best"].tolist() == alone["best"].tolist()
        assert all(np.array_equal(x, y) for x, y in zip(both["witnesses"][0], alone["witnesses"][0]))
    # all-zero weights: 0 exactly where there is a prefix
    for end_final in (False, True):
        zero = a.optimise([0] * m.n_vars, horizon=9, end_final=end_final)
        count = a.count_streams(9, end_final)
        assert zero["best"].tolist() == [0 if n > 0 else NONE for n in count.tolist()]


@pytest.mark.parametrize("name", list(TABLE))
def test_host_twin_on_the_table(stcsp, RefOracle, name):
    check_host_twin(stcsp, RefOracle, name)


@pytest.mark.parametrize("probe", ["until", "arr", "at", "misc", "adversarial"])
def test_host_twin_on_the_probes(stcsp, RefOracle, probe):
    check_host_twin(stcsp, RefOracle, "probe:" + probe)


def test_host_twin_after_adversarial_pass(stcsp, RefOracle):
    check_host_twin(stcsp, RefOracle, "probe:adversarial", adversarial=5)


@pytest.mark.parametrize("block", range(4))
def test_host_twin_on_random_models(stcsp, RefOracle, block):
    for seed in range(block, 60, 4):
        check_host_twin(stcsp, RefOracle, f"random:{seed}")


def ladder(stcsp, RefOracle):
    m, r, a, flags, ref, _ = oracle_case(stcsp, RefOracle, "LADDER")
    return m, a


def test_pins_on_the_ladder(stcsp, RefOracle):
    """LADDER: m starts at 0 and never falls, t flips. A prefix of L steps costs, under {m: 1}, 0 at the least (m stays 0) and
    3 (L - 1) at the most (the first m is 0, every later one 3); under {t: 1} floor(L / 2) at the least (t = 0 1 0 1 ..), and the
    least long-run mean is 1/2. A rung m = j is a cycle of two edges that cost 2 j + 0 and 2 j + 1 under {m: 2, t: 1}: (4 j + 1) / 2."""
    m, a = ladder(stcsp, RefOracle)
    L = 12
    assert a.optimise({"m": 1}, horizon=L)["best"].tolist() == [0] * (L + 1)
    assert a.optimise({"m": 1}, horizon=L, maximise=True)["best"].tolist() == [0] + [3 * (k - 1) for k in range(1, L + 1)]
    res = a.optimise({"t": 1}, horizon=L, lengths=[5], mean=True)
    assert res["best"].tolist() == [k // 2 for k in range(L + 1)] and res["omega_mean"] == (1, 2)
    assert res["witnesses"][0][1][:, m.var_names.index("t")].tolist() == [0, 1, 0, 1, 0]
    assert res["witnesses"][0][1][:, m.var_names.index("m")].tolist() == [0] * 5  # the least rows among the best
    res = a.optimise({"m": 2, "t": 1}, mean=True)
    cyclic = [pq for pq in res["comp_mean"] if pq[1]]
    assert sorted(cyclic) == [(4 * j + 1, 2) for j in range(4)] and res["comp_mean"].count((0, 0)) == 1 and res["largest_cyclic"] == 2
    assert res["omega_mean"] == (1, 2) and res["comp_mean"][res["omega_component"]] == (1, 2)
    res = a.optimise({"m": 2, "t": 1}, mean=True, maximise=True)
    assert res["omega_mean"] == (13, 2) and sorted(pq for pq in res["comp_mean"] if pq[1]) == [(4 * j + 1, 2) for j in range(4)]


def test_pins_on_trap_and_fuse(stcsp, RefOracle):
    """TRAP: t counts 0 1 2 round while m is 0 or 2 (mean 1) and stands still while m is 1 (three self-loops, t = 0, 1, 2). FUSE: a
    live root without an edge. FUSE_UNTIL: no live root."""
    m, r, a, flags, ref, _ = oracle_case(stcsp, RefOracle, "TRAP")
    res = a.optimise({"t": 1}, mean=True)
    assert sorted(pq for pq in res["comp_mean"] if pq[1]) == [(0, 1), (1, 1), (1, 1), (1, 1), (2, 1)] and res["omega_mean"] == (0, 1)
    m, r, a, flags, ref, _ = oracle_case(stcsp, RefOracle, "FUSE")
    res = a.optimise({"c": 1}, horizon=5, lengths=[0, 3], mean=True, state_best=True)
    assert res["best"].tolist() == [0] + [NONE] * 5 and res["comp_mean"] == [(0, 0)] and res["omega_mean"] == (0, 0)
    assert res["omega_component"] == -1 and [len(rows) for _, rows, _ in res["witnesses"]] == [0, 0] and (res["state_best"] == NONE).all()
    m, r, a, flags, ref, _ = oracle_case(stcsp, RefOracle, "FUSE_UNTIL")
    res = a.optimise({"c": 1}, horizon=5, lengths=[0], mean=True, maximise=True)
    assert res["best"].tolist() == [NONE] * 6 and res["n_components"] == 0 and res["n_states"] == 0 and res["omega_mean"] == (0, 0)


def test_end_final_witnesses_end_in_a_final_state(stcsp, RefOracle):
    """LADDER_UNTIL has states that are not final: the witness under end_final ends in a final one and may cost more."""
    m, r, a, (valid, final, alive), ref, _ = oracle_case(stcsp, RefOracle, "LADDER_UNTIL")
    assert not all(final[s] for s in ref["num"])
    w = {"m": -1, "y": 3}
    free, fin = (a.optimise(w, horizon=7, lengths=range(8), end_final=f) for f in (False, True))
    assert all(x <= y for x, y in zip(free["best"].tolist(), fin["best"].tolist())) and free["best"].tolist() != fin["best"].tolist()
    for length, rows, states in fin["witnesses"]:
        if fin["best"][length] != NONE:
            assert final[int(states[-1]) if length else 0]


def test_edited_flags_on_the_ladder(stcsp, RefOracle):
    """The flags are the automaton's current ones: the top rung without its internal edges is no cycle any more."""
    m = stcsp.Model(text=LADDER)
    o = RefOracle(m)
    r = o.solve()
    a = o.automaton(r).traverse()
    valid, final, alive = a.flags()
    ref = CR.yardstick(r, valid, final, alive)
    top = next(c for c, f in ref["flags"].items() if f & CR.BOTTOM)
    src, dst, _ = CR.Q.result_arrays(r)
    alive2 = bytes(0 if ref["comp"].get(int(src[e])) == top and ref["comp"].get(int(dst[e])) == top else alive[e] for e in range(r.n_edges))
    flags = edited_flags(a, valid, final, alive2)
    ref2 = CR.yardstick(r, *flags, lassos=True)
    w = [2 if n == "m" else 1 if n == "t" else 0 for n in m.var_names]
    res = check_mean(a, ref2, w)
    assert sorted(pq for pq in res["comp_mean"] if pq[1]) == [(1, 2), (5, 2), (9, 2)] and res["omega_mean"] == (1, 2)
    check_finite(a, ref2, flags[1], w, True, False)
    whole = oracle_case(stcsp, RefOracle, "LADDER")[2].optimise(w, horizon=9, maximise=True)["best"]
    assert a.optimise(w, horizon=9, maximise=True)["best"][9] < whole[9] == 2 * 3 * 8 + 5  # no staying on the top rung any more


def widened(stcsp, model, ub):
    """A model object whose problem is `model`'s with every upper bound replaced by `ub` (for the bounds of the contract alone)."""
    p = stcsp.Problem.from_buffer_copy(model.problem.contents)
    ubs = (C.c_int32 * model.n_vars)(*([ub] * model.n_vars))
    p.var_ub = C.cast(ubs, C.POINTER(C.c_int32))

    class Widened:
        problem = C.pointer(p)
        keep = (ubs, model)
    return Widened


def test_errors(stcsp, RefOracle):
    m, a = ladder(stcsp, RefOracle)
    for bad in (dict(horizon=-1), dict(horizon=3, lengths=[4]), dict(horizon=3, lengths=[-1]), dict(horizon=2 ** 31 - 1, weights={"m": 2 ** 31 - 1})):
        with pytest.raises(stcsp.StcspError) as ex:
            a.optimise(bad.pop("weights", {"m": 1}), **bad)
        assert ex.value.code == -1
    with pytest.raises(ValueError):
        a.optimise({"nobody": 1})
    with pytest.raises(ValueError):
        a.optimise([1])
    lib, h = stcsp.host_lib(), C.c_void_p()
    rq = stcsp.OptimiseRequest(None, None, 0, 0, 0, 0)  # a null weights
    assert lib.stcsp_automaton_optimise(a._h, C.byref(rq), C.byref(h)) == -1
    w = (C.c_int32 * m.n_vars)()
    rq = stcsp.OptimiseRequest(w, None, 3, 2, 0, 0)  # lengths promised and not given
    assert lib.stcsp_automaton_optimise(a._h, C.byref(rq), C.byref(h)) == -1
    rq = stcsp.OptimiseRequest(w, None, 3, -1, 0, 0)
    assert lib.stcsp_automaton_optimise(a._h, C.byref(rq), C.byref(h)) == -1
    # the bounds: cmax = |w| * max(|lb|, |ub|) summed; cmax * max(horizon, 1) <= 2^62, and with mean nmax^2 * cmax <= 2^62
    r = oracle_case(stcsp, RefOracle, "LADDER")[1]
    wide = stcsp.Automaton(widened(stcsp, m, 2 ** 31 - 1), r).traverse()
    wide._model = m
    one = {"m": 2 ** 31 - 1}  # cmax = (2^31 - 1)^2 < 2^62
    assert wide.optimise(one, horizon=1)["best"].tolist() == [0, 0]
    with pytest.raises(stcsp.StcspError) as ex:
        wide.optimise(one, horizon=2)
    assert ex.value.code == -1
    with pytest.raises(stcsp.StcspError) as ex:
        wide.optimise(one, horizon=1, mean=True)  # nmax = 2
    assert ex.value.code == -2
    with pytest.raises(stcsp.StcspError) as ex:
        wide.optimise({"m": 2 ** 31 - 1, "t": 2 ** 31 - 1})  # cmax > 2^62 at horizon 0
    assert ex.value.code == -1
    assert wide.optimise({"m": 2 ** 29}, mean=True)["omega_mean"] == (0, 1)  # 4 * 2^29 * (2^31 - 1) < 2^62


def test_twin_on_a_binary_file(stcsp, RefOracle, tmp_path):
    m, r, a, flags, ref, _ = oracle_case(stcsp, RefOracle, "juggling_b4_f4_nosym")
    a.write_binary(str(tmp_path / "a.bin"))
    b = stcsp.Automaton.read_binary(str(tmp_path / "a.bin"))
    w = {n: i + 1 for i, n in enumerate(m.var_names) if not n.startswith("_V")}
    x, y = (t.optimise(w, horizon=6, lengths=[6], mean=True) for t in (a, b))
    assert x["best"].tolist() == y["best"].tolist() and rows_of(x["witnesses"][0][1]) == rows_of(y["witnesses"][0][1])
    assert sorted(x["comp_mean"]) == sorted(y["comp_mean"]) and x["omega_mean"] == y["omega_mean"]


def test_optimise_abi(stcsp):
    """The new symbols are exported and the two new structs have the sizes of include/stcsp_engine.h (LP64)."""
    hip = C.CDLL(str(stcsp.CSRC / "libstcsp_hip.so"))
    assert hasattr(hip, "stcsp_engine_optimise")
    for n in ("stcsp_automaton_optimise", "stcsp_optimise_get", "stcsp_optimise_free"):
        assert hasattr(stcsp.host_lib(), n), n
    assert C.sizeof(stcsp.OptimiseRequest) == 32
    assert C.sizeof(stcsp.OptimiseResult) == 144  # int64, 2 pointers, int64, 3 pointers, int64, 3 pointers, 2 x int64, 6 x int32, 2 x double
    assert stcsp.OptimiseResult.omega_component.offset == 104 and stcsp.OptimiseResult.seconds.offset == 128
    assert stcsp.OPT_NONE == 2 ** 63 - 1
