"""Comparing two observable languages, host side (include/stcsp_host.h: stcsp_compare_observers): the CPU twin of the device pass
against an independent yardstick -- the plain Python product of tests/compare_ref.py -- on the observers of the CPU oracle's
automata, and the properties the verdicts must have. The device pass itself: tests/test_compare_gpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import compare_ref as R
import observer_ref as O
from test_monitor import NO_LIVE_ROOT

U = "var x:[0,1]; var y:[0,1]; x until y;"
F = "var x:[0,1]; var y:[0,1];"
TEXTS = {"U": U, "F": F, "dead": NO_LIVE_ROOT}

# (left, right, observable names) -> (left states, left edges, right states, right edges, pairs, pair edges, levels, witness_len[0..3])
TABLE = {
    ("juggling_b4_f4", "juggling_b4_f4_nosym", "A"): (5, 5, 2, 2, 5, 5, 5, (-1, -1, -1, -1)),  # equal languages, different automata
    ("juggling_b4_f5", "juggling_b4_f5_nosym", "A"): (124, 233, 9, 27, 129, 243, 10, (-1, 1, -1, 1)),
    ("juggling_b5_f6", "juggling_b4_f6", "A"): (725, 1344, 417, 1100, 1203, 2618, 14, (5, 2, 5, 2)),
    ("digitinvader3", "digitinvader4", "GAMEOVER"): (85, 145, 131, 231, 521, 921, 51, (-1, -1, -1, -1)),
    ("digitinvader3", "digitinvader4", "D0"): (489, 1933, 1536, 7231, 8162, 41433, 47, (10, 8, 10, 8)),
    ("digitinvader3", "digitinvader4", "I,GAMEOVER"): (505, 2020, 1261, 6305, 22187, 129218, 45, (7, 1, 7, 1)),
    ("digitinvader5", "digitinvader4", "D1"): (14239, 78751, 3626, 17286, 64843, 385598, 60, (8, 10, 8, 10)),
    ("crafted70", "crafted130", "x"): (72, 5112, 132, 17292, 132, 17292, 2, (-1, 1, -1, 1)),
    ("crafted130", "crafted70", "x"): (132, 17292, 72, 5112, 132, 17292, 2, (1, -1, 1, -1)),
    ("U", "F", "x,y"): (3, 10, 1, 4, 4, 16, 2, (-1, 1, -1, 0)),
    ("U", "F", "x"): (3, 6, 1, 2, 3, 6, 2, (-1, -1, -1, 0)),  # prefix-equal, final-different
}
WITNESSES = {  # the witnesses the issue names
    ("juggling_b4_f5", "juggling_b4_f5_nosym", "A"): {1: [(0,)], 3: [(0,)]},
    ("juggling_b5_f6", "juggling_b4_f6", "A"): {0: [(5,)] * 5, 1: [(1,)] * 2},
    ("crafted70", "crafted130", "x"): {1: [(71,)]},
    ("U", "F", "x,y"): {1: [(0, 0)], 3: []},
    ("U", "F", "x"): {3: []},
}


def text_of(stcsp, name):
    if name.startswith("crafted"):
        k = int(name[7:])
        return O.CRAFTED % (k, k)
    return TEXTS.get(name) or stcsp.instances.by_name(name)


def mask_of(model, names):
    names = names.split(",")
    assert all(n in model.var_names for n in names)
    return [int(n in names) for n in model.var_names]


@functools.lru_cache(maxsize=None)
def oracle_observer(stcsp, RefOracle, name, names, prefix_k=2):
    """(automaton of the CPU oracle, mask, its observer by the host twin) for one model under the named variables."""
    m = stcsp.Model(text=text_of(stcsp, name), prefix_k=prefix_k)
    o = RefOracle(m)
    a = o.automaton(o.solve()).traverse()
    mask = mask_of(m, names)
    return a, mask, a.observer(mask)


def twin_against_yardstick(stcsp, RefOracle, left, right, names, prefix_k=2):
    (al, ml, ol), (ar, mr, orr) = oracle_observer(stcsp, RefOracle, left, names, prefix_k), oracle_observer(stcsp, RefOracle, right, names, prefix_k)
    twin = stcsp.compare_observers(ol, orr)
    assert R.same(twin, R.product(ol, orr)), f"{left} | {right} [{names}]: twin and yardstick differ"
    return (al, ml, ol), (ar, mr, orr), twin


def accepted(a, mask, obs, stream):
    """The rows of `stream` that the observer, as an automaton, accepts."""
    if not obs["n_states"]:
        return -1  # no run at all, not even of the empty stream
    return int(a.from_observer(obs, mask).check_streams([np.array(stream, np.int32).reshape(len(stream), sum(mask))], mask)[0][0])


def check_prefix_witnesses(stcsp, sides, twin):
    """A prefix witness is accepted in full by the automaton of the side that has it, and not by the other's."""
    for k in (0, 1):
        w = R.witness(twin, k)
        if w is None:
            continue
        has, lacks = (sides[0], sides[1]) if k == 0 else (sides[1], sides[0])
        assert accepted(*has, w) == len(w) and accepted(*lacks, w) < len(w)


@pytest.mark.parametrize("left,right,names", list(TABLE))
def test_twin_matches_yardstick_on_the_table(stcsp, RefOracle, left, right, names):
    sl, sr, twin = twin_against_yardstick(stcsp, RefOracle, left, right, names)
    got = (sl[2]["n_states"], sl[2]["n_edges"], sr[2]["n_states"], sr[2]["n_edges"], twin["n_pairs"], twin["n_pair_edges"], twin["levels"],
           tuple(twin["witness_len"].tolist()))
    assert got == TABLE[(left, right, names)]
    for k, rows in WITNESSES.get((left, right, names), {}).items():
        assert R.witness(twin, k) == rows
    if (left, right) == ("crafted70", "crafted130"):
        assert (twin["witness_left"][1], twin["witness_right"][1]) == (-1, 72)  # the pair (sink, 72)
    check_prefix_witnesses(stcsp, (sl, sr), twin)
    # swapping the operands swaps the verdicts 0 <-> 1 and 2 <-> 3
    assert R.same(stcsp.compare_observers(sr[2], sl[2]), R.swapped(twin))


def test_wide_states_are_in_the_table(stcsp, RefOracle):
    """The device tests run these rows: a pair with more than 64 out-edges and one with more than 128."""
    for name, least in (("crafted70", 64), ("crafted130", 128)):
        obs = oracle_observer(stcsp, RefOracle, name, "x")[2]
        assert np.bincount(obs["edge_src"]).max() > least


@pytest.mark.parametrize("left,right,names", [("dead", "U", "x,y"), ("U", "dead", "x,y"), ("dead", "dead", "x,y"), ("dead", "F", "x")])
def test_an_operand_without_states(stcsp, RefOracle, left, right, names):
    sl, sr, twin = twin_against_yardstick(stcsp, RefOracle, left, right, names)
    full = sr[2] if left == "dead" else sl[2]
    if left == right:
        assert (twin["n_pairs"], twin["n_pair_edges"], twin["levels"]) == (0, 0, 0) and twin["witness_len"].tolist() == [-1] * 4
        assert twin["witness_values"].shape == (0, 2)
        return
    assert sl[2]["n_states"] == 0 or sr[2]["n_states"] == 0
    assert twin["n_pairs"] == full["n_states"]  # every pair is (sink, state) or (state, sink)
    k = 1 if left == "dead" else 0
    assert twin["witness_len"][k] == 0 and twin["witness_len"][1 - k] == -1  # the empty stream is on the side that has a state
    assert (twin["witness_left"][k], twin["witness_right"][k]) == ((-1, 0) if left == "dead" else (0, -1))
    assert twin["witness_len"][2 + k] >= 0 and twin["witness_len"][3 - k] == -1
    if (left, right, names) == ("dead", "F", "x"):
        assert twin["n_pairs"] == 1 and twin["witness_len"].tolist() == [-1, 0, -1, 0]


@pytest.mark.parametrize("name,names", [("juggling_b4_f5", "A"), ("digitinvader3", "D0"), ("crafted70", "x"), ("U", "x,y")])
def test_an_operand_compared_with_itself(stcsp, RefOracle, name, names):
    sl, sr, twin = twin_against_yardstick(stcsp, RefOracle, name, name, names)
    assert twin["n_pairs"] == sl[2]["n_states"] and twin["n_pair_edges"] == sl[2]["n_edges"] and twin["witness_len"].tolist() == [-1] * 4


@pytest.mark.parametrize("left,right,names,bound", [("U", "F", "x,y", 4), ("F", "U", "x,y", 4), ("U", "F", "x", 5), ("crafted5", "crafted3", "x", 3),
                                                    ("crafted3", "crafted5", "x", 3), ("juggling_b4_f4", "juggling_b4_f4_nosym", "A", 8),
                                                    ("juggling_b4_f4", "U", "A:x", 4)])
def test_brute_force(stcsp, RefOracle, left, right, names, bound):
    """The witnesses against the enumerated languages of both sides (compare_ref.check_by_brute_force)."""
    ln, rn = names.split(":") if ":" in names else (names, names)  # (two models whose one observable variable has two names)
    ol, orr = oracle_observer(stcsp, RefOracle, left, ln)[2], oracle_observer(stcsp, RefOracle, right, rn)[2]
    twin = stcsp.compare_observers(ol, orr)
    assert R.same(twin, R.product(ol, orr))
    R.check_by_brute_force(ol, orr, twin, bound)


def test_malformed_operands(stcsp, RefOracle):
    good = oracle_observer(stcsp, RefOracle, "juggling_b4_f5_nosym", "A")[2]
    left = oracle_observer(stcsp, RefOracle, "juggling_b4_f5", "A")[2]
    assert stcsp.compare_observers(left, good)["n_pairs"] == 129
    for what, bad in R.malformed(good).items():
        for pair in ((left, bad), (bad, left)):
            with pytest.raises(stcsp.StcspError) as ex:
                stcsp.compare_observers(*pair)
            assert ex.value.code == -1, what
    with pytest.raises(stcsp.StcspError) as ex:
        stcsp.compare_observers(left, good, max_pairs=-1)
    assert ex.value.code == -1


def test_max_pairs(stcsp, RefOracle):
    sl, sr, twin = twin_against_yardstick(stcsp, RefOracle, "juggling_b4_f5", "juggling_b4_f5_nosym", "A")
    n = twin["n_pairs"]
    assert R.same(stcsp.compare_observers(sl[2], sr[2], max_pairs=n), twin)
    with pytest.raises(stcsp.StcspError) as ex:
        stcsp.compare_observers(sl[2], sr[2], max_pairs=n - 1)
    assert ex.value.code == -4


def test_compare_abi(stcsp):
    """The new symbols are exported and the two new structs have the sizes of include/stcsp_engine.h (LP64)."""
    hip = C.CDLL(str(stcsp.CSRC / "libstcsp_hip.so"))
    assert hasattr(hip, "stcsp_engine_compare")
    host = stcsp.host_lib()
    for n in ("stcsp_compare_observers", "stcsp_comparison_get", "stcsp_comparison_free"):
        assert hasattr(host, n), n
    assert C.sizeof(stcsp.CompareRequest) == 24  # pointer, int64, int32[2]
    assert C.sizeof(stcsp.CompareResult) == 152  # 2 x int64, int64[5], pointer, 3 x int32[4], int64, 2 x int32, 3 x double
    assert stcsp.CompareResult.witness_len.offset == 64 and stcsp.CompareResult.table_bytes.offset == 112 and stcsp.CompareResult.seconds.offset == 128
