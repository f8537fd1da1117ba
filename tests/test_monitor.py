"""Checking observed streams, host side (include/stcsp_host.h: stcsp_automaton_check_streams): the CPU twin of the device
monitor against an independent yardstick -- the plain Python sets of states of tests/monitor_ref.py, run on the automaton
of the CPU oracle. The device pass itself: tests/test_monitor_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import monitor_ref as M
import quotient_ref as Q
from fuzz_models import random_model
from test_quotient import COUNTDOWN, COUNTER, DUPLICATES, FUZZ_SEEDS, PROBES, SMALLEST_GOLDENS, oracle_automaton

# x until y with y pinned to 0 never reaches a final state: the root is not valid, there is no live automaton
NO_LIVE_ROOT = "var x:[0,1]; var y:[0,1]; x until y; y == 0;"


def check_host_twin(stcsp, RefOracle, model, what, adversarial=None, n_walks=12, max_len=200, seed=1):
    """Host twin == yardstick on the oracle's automaton, for the default mask, `all`, and a mask hiding a signature
    variable, on walks, mutated walks and random rows. Returns {mask name: largest set met}."""
    o, r, a = oracle_automaton(stcsp, RefOracle, model, adversarial)
    valid, final, alive = a.flags()
    res = {}
    for name, mask in M.masks(model, r).items():
        y = M.Yardstick(r, valid, final, alive, mask)
        streams, kinds, where = M.make_streams(y, model.var_bounds(), seed, n_walks, max_len)
        yacc, ynend, yfin, ymax = y.check_all(streams)
        acc, nend, fin, largest = a.check_streams(streams, None if name == "default" else mask)
        assert np.array_equal(acc, yacc) and np.array_equal(nend, ynend) and np.array_equal(fin, yfin), f"{what} [{name}]"
        assert largest == ymax, f"{what} [{name}]"
        for i, k in enumerate(kinds):
            if k == "walk":
                assert acc[i] == len(streams[i]), f"{what} [{name}]: a walk on the live automaton is accepted whole"
            if k == "mutated":
                assert acc[i] >= where[i], f"{what} [{name}]: the prefix before the mutated step is a walk"
        if name == "all" and y.live:
            assert (nend == 1).all() and largest == 1, f"{what}: deterministic with every variable observable"
        if not y.live:
            assert not acc.any() and not nend.any() and not fin.any()
        res[name] = largest
    return res


@pytest.mark.parametrize("name", SMALLEST_GOLDENS)
def test_host_twin_matches_yardstick_on_goldens(stcsp, RefOracle, name):
    check_host_twin(stcsp, RefOracle, stcsp.Model.from_name(name), name)


@pytest.mark.parametrize("probe", ["until", "arr", "at", "misc", "adversarial"])
def test_host_twin_matches_yardstick_on_probes(stcsp, RefOracle, probe):
    check_host_twin(stcsp, RefOracle, stcsp.Model(text=PROBES[probe]["text"]), probe)


@pytest.mark.parametrize("which", ["COUNTER", "COUNTDOWN", "DUPLICATES"])
def test_host_twin_matches_yardstick_on_witness_models(stcsp, RefOracle, which):
    text = {"COUNTER": COUNTER, "COUNTDOWN": COUNTDOWN, "DUPLICATES": DUPLICATES}[which]
    check_host_twin(stcsp, RefOracle, stcsp.Model(text=text), which)


@pytest.mark.parametrize("block", range(4))
def test_host_twin_matches_yardstick_on_fuzz_models(stcsp, RefOracle, block):
    for seed in [s for s in FUZZ_SEEDS if s % 4 == block]:
        text = random_model(seed)
        check_host_twin(stcsp, RefOracle, stcsp.Model(text=text), f"seed {seed}\n{text}", n_walks=5, max_len=40, seed=seed)


def test_host_twin_after_adversarial_pass(stcsp, RefOracle):
    check_host_twin(stcsp, RefOracle, stcsp.Model(text=PROBES["adversarial"]["text"]), "adversarial -a", adversarial=5)


def test_hand_derived_answers(stcsp, RefOracle):
    """COUNTER (tests/test_quotient.py): c runs 0, 1, 2, 3, 3, ... beside a free x; four live states, all final.
    Only x observable: every stream over {0, 1} is accepted, in exactly one state (the counter is a function of time).
    COUNTDOWN: x must be 1 from the fourth step on (c == 3 there): 0 0 0 1 1 is a prefix, 0 0 0 0 stops at index 3.
    A value outside x's domain is an ordinary rejection at its index."""
    m = stcsp.Model(text=COUNTDOWN)
    o, r, a = oracle_automaton(stcsp, RefOracle, m)
    only_x = [int(n == "x") for n in m.var_names]
    streams = [np.array([[0], [0], [0], [1], [1]]), np.array([[0], [0], [0], [0]]), np.array([[1], [7], [1]]), np.zeros((0, 1))]
    acc, nend, fin, largest = a.check_streams(streams, only_x)
    assert acc.tolist() == [5, 3, 1, 0] and nend.tolist() == [1, 1, 1, 1] and fin.tolist() == [1, 1, 1, 1] and largest == 1
    # DUPLICATES under x alone: h is free while c < 3, but it is not in the signature: still one state per step
    m = stcsp.Model(text=DUPLICATES)
    o, r, a = oracle_automaton(stcsp, RefOracle, m)
    acc, nend, fin, largest = a.check_streams([np.array([[0], [1], [0], [1], [1], [0]])], [int(n == "x") for n in m.var_names])
    assert acc.tolist() == [6] and nend.tolist() == [1]


def test_nondeterminism_under_a_hiding_mask(stcsp, RefOracle):
    """A hidden h of 5 values that the signature carries (next h == h) beside a free x: after the first step a stream
    over x alone may be in any of 5 states."""
    m = stcsp.Model(text="var x:[0,1]; var h:[0,4]; next h == h;")
    o, r, a = oracle_automaton(stcsp, RefOracle, m)
    only_x = [int(n == "x") for n in m.var_names]
    acc, nend, fin, largest = a.check_streams([np.array([[0], [1], [1]]), np.zeros((0, 1)), np.array([[2]])], only_x)
    assert acc.tolist() == [3, 0, 0] and nend.tolist() == [5, 1, 1] and largest == 5
    valid, final, alive = a.flags()
    y = M.Yardstick(r, valid, final, alive, only_x)
    assert y.check(np.array([[0], [1], [1]]))[:2] == (3, 5)


def test_edge_cases(stcsp, RefOracle):
    m = stcsp.Model(text=NO_LIVE_ROOT)
    o, r, a = oracle_automaton(stcsp, RefOracle, m)
    assert a.flags()[0][0] == 0  # the root is not valid
    acc, nend, fin, largest = a.check_streams([np.array([[0, 0], [1, 0]]), np.zeros((0, 2))], "all")
    assert acc.tolist() == [0, 0] and nend.tolist() == [0, 0] and fin.tolist() == [0, 0] and largest == 0
    check_host_twin(stcsp, RefOracle, m, "no live root")
    m = stcsp.Model(text=COUNTER)
    o, r, a = oracle_automaton(stcsp, RefOracle, m)
    n_obs = m.n_vars
    acc, nend, fin, largest = a.check_streams([], "all")  # n_streams = 0
    assert len(acc) == len(nend) == len(fin) == 0 and largest == 1
    acc, nend, fin, largest = a.check_streams((np.zeros(0, np.int32), np.zeros(1, np.int64)), "all")  # the same, packed
    assert len(acc) == 0
    acc, nend, fin, largest = a.check_streams([np.zeros((0, n_obs))], "all")  # one empty stream
    assert acc.tolist() == [0] and nend.tolist() == [1] and fin.tolist() == [1]
    rows = np.zeros(4 * n_obs, np.int32)
    for bad in ([0, 3, 2, 4], [1, 2, 3, 4], [0, -1, 2, 4]):  # decreasing; not starting at 0; negative
        with pytest.raises(stcsp.StcspError) as ex:
            a.check_streams((rows, np.array(bad, np.int64)), "all")
        assert ex.value.code == -1
    with pytest.raises(ValueError):
        a.check_streams([np.zeros((2, n_obs + 1))], "all")
    with pytest.raises(ValueError):
        a.check_streams([], [1])


@pytest.mark.parametrize("name", ["juggling_b4_f5", "digitinvader2"])
def test_binary_round_trip_answers_the_same(stcsp, RefOracle, tmp_path, name):
    m = stcsp.Model.from_name(name)
    o, r, a = oracle_automaton(stcsp, RefOracle, m)
    valid, final, alive = a.flags()
    for mname, mask in M.masks(m, r).items():
        y = M.Yardstick(r, valid, final, alive, mask)
        streams, _, _ = M.make_streams(y, m.var_bounds(), 3)
        before = a.check_streams(streams, mask)
        a.write_binary(str(tmp_path / "a.bin"))
        b = stcsp.Automaton.read_binary(str(tmp_path / "a.bin"))
        after = b.check_streams(streams, None if mname == "default" else mask)
        assert all(np.array_equal(x, z) for x, z in zip(before[:3], after[:3])) and before[3] == after[3], f"{name} [{mname}]"


def test_monitor_abi(stcsp):
    """The new symbols are exported and the new structs have the sizes of include/stcsp_engine.h (LP64)."""
    hip = C.CDLL(str(stcsp.CSRC / "libstcsp_hip.so"))
    assert hasattr(hip, "stcsp_engine_monitor_build") and hasattr(hip, "stcsp_engine_monitor_check")
    host = stcsp.host_lib()
    assert hasattr(host, "stcsp_automaton_check_streams") and hasattr(host, "stcsp_automaton_num_observable")
    assert C.sizeof(stcsp.MonitorOptions) == 16          # pointer + int32[2]
    assert C.sizeof(stcsp.MonitorInfo) == 5 * 8 + 4 * 4 + 8
    assert C.sizeof(stcsp.MonitorStreams) == 32          # int64, 2 pointers, 2 x int32
    assert C.sizeof(stcsp.MonitorResult) == 8 + 3 * 8 + 8 + 2 * 4 + 3 * 8
