"""Strongly connected components, omega-liveness and lasso solutions, host side (include/stcsp_host.h:
stcsp_automaton_components): the CPU twin of the device pass against an independent yardstick -- the plain Python Tarjan and
greedy walks of tests/components_ref.py, run on the automaton of the CPU oracle. The device pass itself:
tests/test_components_gpu.py."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import components_ref as R
from fuzz_models import random_model
from test_quotient import COUNTER, PROBES, SMALLEST_GOLDENS

LADDER = "var m:[0,3]; var t:[0,1]; first m == 0; next m >= m; next t == 1 - t;"
LADDER_UNTIL = "var m:[0,2]; var t:[0,1]; var y:[0,1]; first m == 0; next m >= m; next t == 1 - t; (m lt 2) until (y eq 1);"
TRAP = "var m:[0,2]; var t:[0,2]; first m == 0; next m >= m; next t == if (m eq 1) then t else ((t + 1) % 3);"
FUSE = "var c:[0,3]; first c == 0; next c == c + 1;"
FUSE_BRANCH = "var c:[0,3]; var b:[0,1]; first c == 0; first b == 0; next c == if (b eq 1) then c else (c + 1); next b >= b;"
FUSE_UNTIL = "var c:[0,3]; var y:[0,1]; first c == 0; next c == c + 1; (c lt 9) until (y eq 1);"
CRAFTED = {"COUNTER": COUNTER, "LADDER": LADDER, "LADDER_UNTIL": LADDER_UNTIL, "TRAP": TRAP, "FUSE": FUSE, "FUSE_BRANCH": FUSE_BRANCH,
           "FUSE_UNTIL": FUSE_UNTIL}

# name -> (live states, live edges, components, cyclic, accepting, bottom, largest, omega-live states)
TABLE = {
    "juggling_b4_f4_nosym": (25, 48, 7, 6, 6, 6, 4, 25),
    "juggling_b4_f5": (121, 224, 2, 1, 1, 1, 120, 121),
    "digitinvader3": (505, 2020, 2, 1, 1, 1, 504, 505),
    "partialorder_8": (448, 5358, 448, 447, 447, 1, 1, 448),
    "partialorder_10": (1920, 28778, 1920, 1919, 1919, 1, 1, 1920),
    "probe:until": (3, 10, 3, 2, 1, 1, 1, 3),
    "probe:at": (7, 13, 4, 1, 1, 1, 4, 7),
    "probe:misc": (6, 10, 6, 5, 5, 5, 1, 6),
    "COUNTER": (4, 8, 4, 1, 1, 1, 1, 4),
    "LADDER": (9, 28, 5, 4, 4, 1, 2, 9),
    "LADDER_UNTIL": (13, 58, 8, 5, 3, 1, 2, 13),
    "TRAP": (10, 27, 6, 5, 5, 1, 3, 10),
    "FUSE_BRANCH": (6, 8, 6, 3, 3, 3, 1, 6),
    "FUSE": (1, 0, 1, 0, 0, 1, 1, 0),
    "random:0": (1, 0, 1, 0, 0, 1, 1, 0),
    "random:2": (1, 0, 1, 0, 0, 1, 1, 0),
    "random:3": (1, 0, 1, 0, 0, 1, 1, 0),
    "FUSE_UNTIL": (0, 0, 0, 0, 0, 0, 0, 0),
}
# name -> the (stem length, loop length) of its lassos, sorted: fixed by the contract
LASSO_LENGTHS = {
    "juggling_b4_f4_nosym": [(1, 4)] * 6, "juggling_b4_f5": [(1, 4)], "digitinvader3": [(1, 4)], "probe:at": [(3, 4)],
    "probe:until": [(1, 1)], "random:5": [(3, 1)] * 2,
}


def text_of(stcsp, name):
    if name.startswith("probe:"):
        return PROBES[name[6:]]["text"]
    if name.startswith("random:"):
        return random_model(int(name[7:]))
    return CRAFTED[name] if name in CRAFTED else stcsp.instances.by_name(name)


@functools.lru_cache(maxsize=None)
def oracle_case(stcsp, RefOracle, name, adversarial=None, prefix_k=2):
    """(model, Result, automaton, (valid, final, alive), yardstick with every lasso) of the CPU oracle's automaton; computed once."""
    m = stcsp.Model(text=text_of(stcsp, name), prefix_k=prefix_k)
    o = RefOracle(m)
    r = o.solve()
    a = o.automaton(r).traverse()
    if adversarial is not None:
        a.adversarial(adversarial)
    flags = a.flags()
    return m, r, a, flags, R.yardstick(r, *flags, lassos=True), o


def table_row(ref):
    c = ref["counts"]
    return tuple(c[k] for k in ("n_states", "n_edges", "n_components", "n_cyclic", "n_accepting", "n_bottom", "largest", "n_omega"))


def check_host_twin(stcsp, RefOracle, name, adversarial=None, prefix_k=2):
    """Host twin == yardstick: the partition, the flags, the depths, omega, and every lasso."""
    m, r, a, (valid, final, alive), ref, _ = oracle_case(stcsp, RefOracle, name, adversarial, prefix_k)
    res = a.components("all")
    R.check_result(r, valid, alive, res, ref)
    assert R.result_lassos(res) == ref["lassos"] and res["n_lassos"] == len(ref["lassos"]) == ref["counts"]["n_accepting"], name
    assert res["n_vars"] == m.n_vars and res["rounds"].tolist() == [0, 0, 0] and res["seconds_kernels"] == 0
    # in order of (depth, component number), each lasso under its own component's number
    keys = [(int(res["comp_depth"][c]), c) for c, _, _ in res["lassos"]]
    assert keys == sorted(keys) and all(res["comp_flags"][c] & R.ACCEPTING for c, _, _ in res["lassos"])
    none = a.components()
    assert none["lassos"] == [] and R.same({**res, "lassos": [], "n_lassos": 0}, none)
    return res, ref


@pytest.mark.parametrize("name", list(TABLE))
def test_the_table(stcsp, RefOracle, name):
    res, ref = check_host_twin(stcsp, RefOracle, name)
    assert table_row(ref) == TABLE[name]
    got = (res["n_states"], ref["counts"]["n_edges"], res["n_components"], res["n_cyclic"], res["n_accepting"], res["n_bottom"],
           int(res["comp_size"].max(initial=0)), res["n_omega"])
    assert got == TABLE[name]
    assert res["root_omega"] == int(TABLE[name][7] > 0)


@pytest.mark.parametrize("name", SMALLEST_GOLDENS)
def test_host_twin_matches_yardstick_on_goldens(stcsp, RefOracle, name):
    check_host_twin(stcsp, RefOracle, name)


@pytest.mark.parametrize("probe", ["until", "arr", "at", "misc", "adversarial"])
def test_host_twin_matches_yardstick_on_probes(stcsp, RefOracle, probe):
    check_host_twin(stcsp, RefOracle, "probe:" + probe)


def test_host_twin_after_adversarial_pass(stcsp, RefOracle):
    """The flags are the ones the adversarial pass left."""
    res, ref = check_host_twin(stcsp, RefOracle, "probe:adversarial", adversarial=5)
    assert res["n_states"] == PROBES["adversarial"]["adver1_live_states"]


@pytest.mark.parametrize("block", range(4))
def test_host_twin_matches_yardstick_on_random_models(stcsp, RefOracle, block):
    dead_roots = 0
    for seed in range(block, 60, 4):
        res, ref = check_host_twin(stcsp, RefOracle, f"random:{seed}")
        dead_roots += table_row(ref) == TABLE["FUSE"]
    assert dead_roots >= 1  # a live root without an edge: "not empty" for every other service, yet no infinite solution


def test_edgeless_live_roots_among_the_random_models(stcsp, RefOracle):
    assert sum(table_row(oracle_case(stcsp, RefOracle, f"random:{seed}")[4]) == TABLE["FUSE"] for seed in range(60)) == 38


@pytest.mark.parametrize("name", list(LASSO_LENGTHS))
def test_lasso_lengths(stcsp, RefOracle, name):
    res, ref = check_host_twin(stcsp, RefOracle, name)
    assert sorted((len(stem), len(loop)) for _, stem, loop in res["lassos"]) == LASSO_LENGTHS[name]
    assert sorted((len(stem), len(loop)) for stem, loop in ref["lassos"]) == LASSO_LENGTHS[name]


def test_the_bottom_components_of_juggling_are_its_patterns(stcsp, RefOracle):
    m, r, a, flags, ref, _ = oracle_case(stcsp, RefOracle, "juggling_b4_f4_nosym")
    res = a.components("bottom")
    assert res["n_lassos"] == 6 and R.result_lassos(res) == R.yardstick(r, *flags, lassos=True, bottom_only=True)["lassos"]
    assert all(res["comp_flags"][c] == R.CYCLIC | R.FINAL | R.BOTTOM | R.ACCEPTING for c, _, _ in res["lassos"])


def test_component_depth_is_the_breadth_first_depth(stcsp, RefOracle):
    for name in ("LADDER_UNTIL", "TRAP", "probe:at", "juggling_b4_f5"):
        m, r, a, flags, ref, _ = oracle_case(stcsp, RefOracle, name)
        res = a.components()
        sc = res["state_component"]
        for k in range(res["n_components"]):
            assert res["comp_depth"][k] == min(ref["depth"][s] for s in np.flatnonzero(sc == k).tolist())
        assert res["comp_depth"][sc[0]] == 0 and sc[0] == 0  # the root's component is number 0


def edited_flags(a, valid, final, alive):
    keep = [np.frombuffer(bytes(x), np.uint8).copy() for x in (valid, final, alive)]
    a.import_flags(SimpleNamespace(state_valid=keep[0].ctypes.data, state_final=keep[1].ctypes.data, edge_alive=keep[2].ctypes.data))
    return a.flags()


def test_edited_flags_on_the_ladder(stcsp, RefOracle):
    """LADDER is a root above four rungs (m = 0 .. 3), each a cycle of two states (t flips), every state final and every rung
    leading to the higher ones. Cutting the top rung's two internal edges makes its states edgeless singletons, a dead end: 7 of
    the 9 states still start an infinite solution. Clearing `final` on the rung below it as well leaves that rung cyclic but not
    accepting, and it reaches only the dead end: the root and the rungs m = 0 and m = 1 remain, 5 states."""
    m = stcsp.Model(text=LADDER)
    o = RefOracle(m)
    r = o.solve()
    a = o.automaton(r).traverse()
    valid, final, alive = a.flags()
    ref = R.yardstick(r, valid, final, alive)
    top = next(c for c, f in ref["flags"].items() if f & R.BOTTOM)
    src, dst, _ = R.Q.result_arrays(r)
    alive2 = bytes(0 if ref["comp"].get(int(src[e])) == top and ref["comp"].get(int(dst[e])) == top else alive[e] for e in range(r.n_edges))
    flags = edited_flags(a, valid, final, alive2)
    ref2 = R.yardstick(r, *flags, lassos=True)
    res = a.components("all")
    R.check_result(r, flags[0], flags[2], res, ref2)
    assert (res["n_states"], res["n_components"], res["n_cyclic"], res["n_accepting"], res["n_bottom"], res["n_omega"]) == (9, 6, 3, 3, 2, 7)
    assert R.result_lassos(res) == ref2["lassos"] and res["n_lassos"] == 3
    below = next(c for c, ms in ref["members"].items() if c != top and all(ref["comp"][v] in (c, top) for s in ms for _, v in ref["out"][s]))
    final2 = bytes(0 if ref["comp"].get(s) == below else final[s] for s in range(r.n_states))
    flags = edited_flags(a, valid, final2, alive2)
    ref3 = R.yardstick(r, *flags, lassos=True)
    res = a.components("all")
    R.check_result(r, flags[0], flags[2], res, ref3)
    assert (res["n_states"], res["n_components"], res["n_cyclic"], res["n_accepting"], res["n_bottom"], res["n_omega"]) == (9, 6, 3, 2, 2, 5)
    assert 0 < res["n_omega"] < res["n_states"] and res["root_omega"] == 1
    assert R.result_lassos(res) == ref3["lassos"] and res["n_lassos"] == 2
    k = res["state_component"][ref["members"][below][0]]
    assert res["comp_flags"][k] == R.CYCLIC and res["state_omega"][ref["members"][below]].tolist() == [0, 0]


@pytest.mark.parametrize("name", ["juggling_b4_f4_nosym", "juggling_b4_f5", "probe:at", "probe:until", "random:5", "LADDER_UNTIL", "TRAP",
                                  "FUSE_BRANCH", "partialorder_8"])
def test_unrolled_lassos_are_solutions(stcsp, RefOracle, name):
    """stem + loop * k, k = 1, 2, 3, is accepted in full under the all-variables mask and ends in a final state every time."""
    m, r, a, flags, ref, _ = oracle_case(stcsp, RefOracle, name)
    lassos = a.components("all")["lassos"][:70]
    assert lassos
    streams = [np.concatenate([stem] + [loop] * k) for _, stem, loop in lassos for k in (1, 2, 3)]
    acc, nend, fin, _ = a.check_streams(streams, "all")
    assert acc.tolist() == [len(s) for s in streams] and nend.tolist() == [1] * len(streams) and fin.tolist() == [1] * len(streams)


def test_max_lassos_truncates(stcsp, RefOracle):
    for name, total in (("juggling_b4_f4_nosym", 6), ("partialorder_8", 447), ("TRAP", 5)):
        m, r, a, flags, ref, _ = oracle_case(stcsp, RefOracle, name)
        full = a.components("all")
        assert full["n_lassos"] == total
        for n in (1, 2, total - 1, total, total + 5):
            res = a.components(n)
            assert res["n_lassos"] == len(res["lassos"]) == min(n, total)
            assert R.result_lassos(res) <= ref["lassos"]
            assert R.same(res, {**full, "lassos": full["lassos"][:n], "n_lassos": min(n, total)})  # the first by (depth, number)


def test_bottom_only_on_partialorder(stcsp, RefOracle):
    m, r, a, flags, ref, _ = oracle_case(stcsp, RefOracle, "partialorder_8")
    res = a.components("bottom")
    assert res["n_lassos"] == 1 and res["n_bottom"] == 1
    (c, stem, loop), = res["lassos"]
    assert res["comp_flags"][c] & R.BOTTOM and len(loop) == 1 and (tuple(map(tuple, stem.tolist())), tuple(map(tuple, loop.tolist()))) in ref["lassos"]
    assert a.components(3)["n_lassos"] == 3


def test_twin_on_a_binary_file_and_bad_arguments(stcsp, RefOracle, tmp_path):
    m, r, a, flags, ref, _ = oracle_case(stcsp, RefOracle, "juggling_b4_f4_nosym")
    a.write_binary(str(tmp_path / "a.bin"))
    b = stcsp.Automaton.read_binary(str(tmp_path / "a.bin")).components("all")
    assert R.result_lassos(b) == ref["lassos"] and (b["n_states"], b["n_components"], b["n_bottom"], b["n_omega"]) == (25, 7, 6, 25)
    with pytest.raises(ValueError):
        a.components(-3)
    with pytest.raises(ValueError):
        a.components("some")
    h = C.c_void_p()
    assert stcsp.host_lib().stcsp_automaton_components(a._h, -2, 0, C.byref(h)) == -1


def test_components_abi(stcsp):
    """The new symbols are exported and the two new structs have the sizes of include/stcsp_engine.h (LP64)."""
    hip = C.CDLL(str(stcsp.CSRC / "libstcsp_hip.so"))
    assert hasattr(hip, "stcsp_engine_components")
    for n in ("stcsp_automaton_components", "stcsp_components_get", "stcsp_components_free"):
        assert hasattr(stcsp.host_lib(), n), n
    assert C.sizeof(stcsp.ComponentsOptions) == 16
    assert C.sizeof(stcsp.ComponentsResult) == 168  # 6 x int64, 5 pointers, int64, 4 pointers, 6 x int32, 2 x double
    assert stcsp.ComponentsResult.n_vars.offset == 128 and stcsp.ComponentsResult.seconds.offset == 152
