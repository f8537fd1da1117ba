"""Counting, enumerating and sampling solution prefixes, host side (include/stcsp_host.h: stcsp_automaton_generate): the CPU
twin of the device generator against an independent yardstick -- the plain Python of tests/generate_ref.py, run on the
automaton of the CPU oracle. Nothing is compared with a tolerance: counts below 2^53 are exact integers, and beyond that
the contract fixes the order of every sum, so the doubles agree bit for bit. The device pass itself:
tests/test_generate_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import generate_ref as G
import monitor_ref as M
from fuzz_models import random_model
from test_quotient import COUNTDOWN, COUNTER, DUPLICATES, FUZZ_SEEDS, PROBES, oracle_automaton

HIDDEN_H = "var x:[0,1]; var h:[0,4]; next h == h;"
UNTIL = "var x:[0,1]; var y:[0,1]; x until y;"
# x until y with y pinned to 0 never reaches a final state: the root is not valid, there is no live automaton
NO_LIVE_ROOT = "var x:[0,1]; var y:[0,1]; x until y; y == 0;"

_solved = {}


def solved(stcsp, RefOracle, text, prefix_k=2):
    """(model, oracle, result, automaton) of a model text, solved once per session (and prefix length, where it is not 2)."""
    key = text if prefix_k == 2 else (text, prefix_k)
    if key not in _solved:
        m = stcsp.Model(text=text, prefix_k=prefix_k)
        _solved[key] = (m,) + oracle_automaton(stcsp, RefOracle, m)
    return _solved[key]


def text_of(stcsp, name):
    return PROBES[name[6:]]["text"] if name.startswith("probe:") else stcsp.instances.by_name(name)


def check_sampling(stcsp, RefOracle, text, what, horizon=64, seeds=(0, 7), n=12, lengths=None, mask_names=("default", "all", "hidden"), prefix_k=2):
    """Twin == yardstick value for value (count, streams, end_final), and every stream is accepted whole by the monitor's
    host twin under the same mask. Returns the yardstick of the last mask."""
    m, o, r, a = solved(stcsp, RefOracle, text, prefix_k)
    valid, final, alive = a.flags()
    y = None
    for name, mask in M.masks(m, r).items():
        if name not in mask_names:
            continue
        arg = None if name == "default" else mask
        y = G.Yardstick(r, valid, final, alive, mask, horizon)
        for length in lengths or (horizon, 1, horizon // 3):
            for seed in seeds:
                if y.count[length] == 0:
                    with pytest.raises(stcsp.StcspError) as ex:
                        a.generate(n, length, seed, observable=arg, horizon=horizon)
                    assert ex.value.code == -1, f"{what} [{name}]"
                    continue
                values, fin, count = a.generate(n, length, seed, observable=arg, horizon=horizon)
                assert np.array_equal(count, y.count), f"{what} [{name}]: count"
                yv, yf = y.streams(n, length, seed)
                assert values.shape == (n, length, sum(mask)) and np.array_equal(values, yv), f"{what} [{name}] seed {seed} len {length}"
                assert np.array_equal(fin, yf), f"{what} [{name}] seed {seed} len {length}: end_final"
                acc, nend, mfin, _ = a.check_streams(list(values), arg)
                assert (acc == length).all(), f"{what} [{name}]: a generated stream is a prefix of a solution"
                if name == "all":  # deterministic: the monitor ends in the one state the generator ended in
                    assert np.array_equal(mfin, fin), f"{what} [all]: end_final against the monitor"
    return y


def test_hand_derived_counts(stcsp, RefOracle):
    """count[t], t = 0 .. 8, all exact.
    COUNTER: x free at every step, the counter a function of time: 2^t.
    COUNTDOWN: x is forced to 1 from the fourth step on: 1, 2, 4, 8, then 8.
    DUPLICATES: x and h free for three steps (4 per step), then h == 0 (2 per step).
    HIDDEN_H: the first step chooses x and h (10), every later one x only.
    UNTIL: counted over all paths, and over those that end in a final state.
    partialorder_10: the weights against the yardstick's plain enumeration up to 20,000 paths (t <= 4)."""
    expect = {
        COUNTER: [2 ** t for t in range(9)],
        COUNTDOWN: [1, 2, 4, 8, 8, 8, 8, 8, 8],
        DUPLICATES: [1, 4, 16, 64, 128, 256, 512, 1024, 2048],
        HIDDEN_H: [1] + [10 * 2 ** (t - 1) for t in range(1, 9)],
        UNTIL: [1, 3, 11, 43, 171, 683, 2731, 10923, 43691],
        stcsp.instances.by_name("partialorder_10"): [1, 8, 120, 1600, 20000, 240000, 2800000, 32000000, 360000000],
    }
    for text, counts in expect.items():
        m, o, r, a = solved(stcsp, RefOracle, text)
        assert a.count_streams(8).tolist() == counts, text[:60]
        values, fin, count = a.generate(0, 8, observable="all")
        assert count.tolist() == counts, text[:60]
        y = G.Yardstick(r, *a.flags(), [1] * m.n_vars, 8)
        assert y.count.tolist() == counts, text[:60]
        for t in [t for t in range(9) if counts[t] <= 20000]:  # the weights against plain enumeration
            assert len(y.enumerate(t)) == counts[t], (text[:60], t)
    m, o, r, a = solved(stcsp, RefOracle, UNTIL)
    final = [0, 2, 10, 42, 170, 682, 2730, 10922, 43690]
    assert a.count_streams(8, end_final=True).tolist() == final
    y = G.Yardstick(r, *a.flags(), [1] * m.n_vars, 8, end_final=True)
    assert y.count.tolist() == final and [len(y.enumerate(t, end_final=True)) for t in range(6)] == final[:6]
    with pytest.raises(stcsp.StcspError) as ex:  # no prefix of length 0 ends in a final state
        a.generate(1, 0, horizon=8, end_final=True)
    assert ex.value.code == -1
    values, fin, _ = a.generate(3, 0, horizon=8)  # but the empty prefix exists
    assert values.shape == (3, 0, 2) and fin.tolist() == [0, 0, 0]
    values, fin, _ = a.generate(5, 4, seed=3, horizon=8, end_final=True)
    assert fin.tolist() == [1] * 5


def test_hand_derived_unranking(stcsp, RefOracle):
    """COUNTDOWN with only x observable, L = 5: x is variable 0 and every other variable is a function of time, so the
    lexicographic order of the paths is the order of the x columns: x is free for three steps and 1 afterwards."""
    m, o, r, a = solved(stcsp, RefOracle, COUNTDOWN)
    only_x = [int(n == "x") for n in m.var_names]
    assert m.var_names[0] == "x"
    values, fin, count = a.generate(8, 5, ranks=np.arange(8), observable=only_x)
    assert count[5] == 8
    for rank in range(8):
        assert values[rank, :, 0].tolist() == [rank >> 2 & 1, rank >> 1 & 1, rank & 1, 1, 1]
    for bad in ([8], [2 ** 53], [2 ** 64 - 1]):
        with pytest.raises(stcsp.StcspError) as ex:
            a.generate(1, 5, ranks=bad, observable=only_x)
        assert ex.value.code == -1
    with pytest.raises(stcsp.StcspError) as ex:  # a length beyond the horizon
        a.generate(1, 6, horizon=5)
    assert ex.value.code == -1


@pytest.mark.parametrize("which", ["COUNTDOWN", "UNTIL", "probe:at", "probe:misc", "probe:until"])
def test_exhaustive_unranking(stcsp, RefOracle, which):
    """Ranks 0 .. count[L] - 1 give count[L] pairwise distinct streams in strictly increasing lexicographic order: the
    yardstick's enumeration, which does not use the weights. L is the longest length of at most 12 steps with at most
    5,000 paths. Every stream is accepted whole by the monitor's host twin."""
    text = {"COUNTDOWN": COUNTDOWN, "UNTIL": UNTIL}.get(which) or text_of(stcsp, which)
    m, o, r, a = solved(stcsp, RefOracle, text)
    all_ = [1] * m.n_vars
    for end_final in (False, True):
        y = G.Yardstick(r, *a.flags(), all_, 12, end_final)
        fits = [t for t in range(1, 13) if 0 < y.count[t] <= 5000]
        if not fits:
            assert end_final
            continue
        L = fits[-1]
        n = int(y.count[L])
        values, fin, count = a.generate(n, L, ranks=np.arange(n), observable="all", horizon=12, end_final=end_final)
        assert np.array_equal(count, y.count)
        got = [tuple(map(tuple, s)) for s in values.tolist()]
        assert all(x < z for x, z in zip(got, got[1:])), f"{which}: strictly increasing"
        assert got == y.enumerate(L, end_final), f"{which}: the enumeration"
        yv, yf = y.streams(n, L, ranks=range(n))
        assert np.array_equal(values, yv) and np.array_equal(fin, yf)
        acc, nend, mfin, _ = a.check_streams(list(values), "all")
        assert (acc == L).all() and np.array_equal(mfin, fin)
        if end_final:
            assert fin.all()
        with pytest.raises(stcsp.StcspError) as ex:
            a.generate(1, L, ranks=[n], observable="all", horizon=12, end_final=end_final)
        assert ex.value.code == -1


@pytest.mark.parametrize("which", ["COUNTER", "COUNTDOWN", "DUPLICATES", "HIDDEN_H", "UNTIL", "probe:at", "probe:misc", "probe:until",
                                   "juggling_b4_f5", "digitinvader1", "digitinvader3", "partialorder_10"])
def test_sampling_at_horizon_64(stcsp, RefOracle, which):
    text = {"COUNTER": COUNTER, "COUNTDOWN": COUNTDOWN, "DUPLICATES": DUPLICATES, "HIDDEN_H": HIDDEN_H, "UNTIL": UNTIL}.get(which) or text_of(stcsp, which)
    y = check_sampling(stcsp, RefOracle, text, which)
    print(f"{which}: count[64] = {y.count[64]:.6g}")
    if which in ("partialorder_10", "digitinvader3", "UNTIL"):
        assert y.count[64] > 2.0 ** 64  # no integer counter carries this horizon


def test_sampling_ending_in_a_final_state(stcsp, RefOracle):
    m, o, r, a = solved(stcsp, RefOracle, UNTIL)
    valid, final, alive = a.flags()
    y = G.Yardstick(r, valid, final, alive, [1, 1], 64, end_final=True)
    values, fin, count = a.generate(40, 64, seed=7, observable="all", end_final=True)
    yv, yf = y.streams(40, 64, seed=7)
    assert np.array_equal(count, y.count) and np.array_equal(values, yv) and np.array_equal(fin, yf) and fin.all()


@pytest.mark.parametrize("block", range(4))
def test_sampling_on_fuzz_models(stcsp, RefOracle, block):
    checked = 0
    for seed in [s for s in FUZZ_SEEDS if s % 4 == block]:
        text = random_model(seed)
        check_sampling(stcsp, RefOracle, text, f"seed {seed}\n{text}", horizon=9, seeds=(seed,), n=6, lengths=(9, 4), mask_names=("default", "hidden"))
        _solved.pop(text)
        checked += 1
    assert checked >= 45


def test_no_live_root(stcsp, RefOracle):
    m, o, r, a = solved(stcsp, RefOracle, NO_LIVE_ROOT)
    assert a.flags()[0][0] == 0
    assert a.count_streams(6).tolist() == [0] * 7
    for length in (0, 3):
        with pytest.raises(stcsp.StcspError) as ex:
            a.generate(2, length, horizon=6)
        assert ex.value.code == -1


def test_binary_round_trip_generates_the_same(stcsp, RefOracle, tmp_path):
    m, o, r, a = solved(stcsp, RefOracle, stcsp.instances.by_name("juggling_b4_f5"))
    before = a.generate(10, 20, seed=5, observable="all")
    a.write_binary(str(tmp_path / "a.bin"))
    after = stcsp.Automaton.read_binary(str(tmp_path / "a.bin")).generate(10, 20, seed=5, observable=[1] * m.n_vars)
    assert all(np.array_equal(x, z) for x, z in zip(before, after))


def test_generator_abi(stcsp):
    """The new symbols are exported and the new structs have the sizes of include/stcsp_engine.h (LP64)."""
    hip = C.CDLL(str(stcsp.CSRC / "libstcsp_hip.so"))
    assert hasattr(hip, "stcsp_engine_generator_build") and hasattr(hip, "stcsp_engine_generate")
    host = stcsp.host_lib()
    assert hasattr(host, "stcsp_automaton_generate") and hasattr(host, "stcsp_automaton_count_streams")
    assert C.sizeof(stcsp.GeneratorOptions) == 24        # pointer, 2 x int32, int32[2]
    assert C.sizeof(stcsp.GeneratorInfo) == 3 * 8 + 8 + 4 * 4 + 8
    assert C.sizeof(stcsp.GenerateRequest) == 32         # int64, pointer, uint64, 2 x int32
    assert C.sizeof(stcsp.GenerateResult) == 8 + 2 * 8 + 2 * 4 + 2 * 8
