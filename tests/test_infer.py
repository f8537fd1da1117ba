"""Inferring the unobserved entries of streams, host side (include/stcsp_host.h: stcsp_automaton_infer_streams): the CPU twin
of the device pass against an independent yardstick -- the plain Python of tests/infer_ref.py, its recurrences and its brute
force, run on the automaton of the CPU oracle. Counts are doubles added in a fixed order, supports are sets, everything is
compared with ==, the doubles by their bits. The device pass itself: tests/test_infer_gpu.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import infer_ref as I
import monitor_ref as M
from test_generate import HIDDEN_H, NO_LIVE_ROOT, UNTIL, solved, text_of
from test_quotient import COUNTDOWN, COUNTER, DUPLICATES, SMALLEST_GOLDENS

WITNESS = {"COUNTER": COUNTER, "COUNTDOWN": COUNTDOWN, "DUPLICATES": DUPLICATES}
X = I.MISSING


def only(model, *names):
    assert all(n in model.var_names for n in names)
    return [int(n in names) for n in model.var_names]


def one(a, stream, observable, **kw):
    """(count, supports, n_states) of one stream, and with draws also (draws, end_final), as plain Python values."""
    n_obs = sum(observable)
    count, supports, n_states, draws, fin = a.infer_streams([np.array(stream, dtype=np.int32).reshape(-1, n_obs)], observable, **kw)
    head = (float(count[0]), supports[0], n_states[0].tolist())
    return head + (draws[0].tolist(), fin[0].tolist()) if kw.get("draws") else head


def test_hand_derived_countdown(stcsp, RefOracle):
    """COUNTDOWN: c runs 0, 1, 2, 3, 3 and x must be 1 while c == 3, that is at steps 3 and 4; x is free before. Under x alone:
    five unobserved steps have 2^3 completions, the tail is forced: the supports are {0,1} three times, then {1} twice. The
    automaton is a chain, one state per step. Observing x = 1 at step 1 halves the count and leaves the other entries as they
    were. c is a function of time, so a late observation that contradicts it, x = 0 at step 3, leaves nothing: count 0, every
    support empty, no state. The 8 completions in order of their rows are the binary numbers 000 .. 111 followed by 1, 1."""
    m, o, r, a = solved(stcsp, RefOracle, COUNTDOWN)
    x = only(m, "x")
    free, forced = [[0, 1]], [[1]]
    assert one(a, [[X]] * 5, x) == (8.0, [free, free, free, forced, forced], [1] * 6)
    assert one(a, [[X], [1], [X], [X], [X]], x) == (4.0, [free, forced, free, forced, forced], [1] * 6)
    assert one(a, [[X], [X], [X], [0], [X]], x) == (0.0, [[[]]] * 5, [0] * 6)
    got = one(a, [[X]] * 5, x, draws=8, ranks=[list(range(8))])
    assert got[3] == [[[k >> 2 & 1], [k >> 1 & 1], [k & 1], [1], [1]] for k in range(8)] and got[4] == [1] * 8
    assert one(a, [[X], [X], [X], [0], [X]], x, draws=2, ranks=[[5, 99]])[3:] == ([[[X]] * 5] * 2, [0, 0])  # ranks of an infeasible stream: ignored


def test_hand_derived_pinning(stcsp, RefOracle):
    """HIDDEN_H, x free and h constant over time, both observable: h seen as 3 at the last of four steps pins the three
    unobserved h before it to {3}; x stays free: 2^4 completions. Without the late observation h can be any of 0 .. 4 at every
    step: 5 * 2^4. After the first step the automaton is in one of five states, one per value of h."""
    m, o, r, a = solved(stcsp, RefOracle, HIDDEN_H)
    mask = only(m, "x", "h")
    assert [n for n, k in zip(m.var_names, mask) if k] == ["x", "h"]
    free = [0, 1]
    assert one(a, [[X, X]] * 3 + [[X, 3]], mask) == (16.0, [[free, [3]]] * 4, [1, 1, 1, 1, 1])
    assert one(a, [[X, X]] * 4, mask) == (80.0, [[free, [0, 1, 2, 3, 4]]] * 4, [1, 5, 5, 5, 5])
    assert one(a, [[X, 2], [X, X], [X, 3]], mask)[0] == 0.0  # h does not change


def test_hand_derived_until(stcsp, RefOracle):
    """UNTIL, x until y: the root waits for y and is not final; from it (x, y) = (1, 0) stays, (0, 1) and (1, 1) lead to the one
    final state, where every row is allowed. Two unobserved steps: 3 + 2 * 4 = 11 paths, of which (1,0), (1,0) alone does not
    end in the final state: 10 with END_FINAL; every value occurs. After an observed (1, 0) the run still waits: 3 ways on, two
    of them final, and with END_FINAL y must be 1. (0, 0) at the first step has no edge."""
    m, o, r, a = solved(stcsp, RefOracle, UNTIL)
    mask = only(m, "x", "y")
    assert [n for n, k in zip(m.var_names, mask) if k] == ["x", "y"]
    both = [[0, 1], [0, 1]]
    assert one(a, [[X, X]] * 2, mask) == (11.0, [both, both], [1, 2, 2])
    assert one(a, [[X, X]] * 2, mask, end_final=True) == (10.0, [both, both], [1, 2, 1])
    assert one(a, [[1, 0], [X, X]], mask) == (3.0, [[[1], [0]], both], [1, 1, 2])
    assert one(a, [[1, 0], [X, X]], mask, end_final=True) == (2.0, [[[1], [0]], [[0, 1], [1]]], [1, 1, 1])
    assert one(a, [[0, 0], [X, X]], mask) == (0.0, [[[], []]] * 2, [0, 0, 0])
    assert one(a, [], mask) == (1.0, [], [1])                    # length 0: the empty path
    assert one(a, [], mask, end_final=True) == (0.0, [], [0])   # the root is not final


def test_no_live_root_and_a_value_no_edge_carries(stcsp, RefOracle):
    m, o, r, a = solved(stcsp, RefOracle, NO_LIVE_ROOT)
    mask = only(m, "x", "y")
    assert one(a, [[1, 0]] * 3, mask) == (0.0, [[[], []]] * 3, [0] * 4)
    assert one(a, [], mask) == (0.0, [], [0])
    assert one(a, [[X, X]], mask, draws=1) == (0.0, [[[], []]], [0, 0], [[[X, X]]], [0])
    m, o, r, a = solved(stcsp, RefOracle, COUNTDOWN)
    assert one(a, [[X], [5], [X]], only(m, "x")) == (0.0, [[[]]] * 3, [0] * 4)


def longest_enumerable(y, limit=5000, cap=6):
    return max([t for t in range(1, cap + 1) if 0 < y.n_paths(t) <= limit], default=0)


def specialisation(a, arg, streams, counts, supports, bounds, keep, what):
    """Replacing a MISSING entry by a value of its support keeps count > 0, any other value makes it 0, and the counts of the
    specialised streams sum to the stream's: one twin call over all the specialised streams."""
    cases, special = [], []
    for i, s in enumerate(streams):
        for t, v in zip(*np.nonzero(s == X)):
            sup = supports[i][t][v]
            lo, hi = bounds[keep[v]]
            others = (set(range(max(lo, -10 ** 6), min(hi, lo + 12) + 1)) | {x + d for x in sup for d in (-1, 1)}) - set(sup)
            for value in list(sup) + sorted(others):
                z = s.copy()
                z[t, v] = value
                special.append(z)
            cases.append((i, t, v, len(sup), len(others)))
    if not special:
        return 0
    got = a.infer_streams(special, arg)[0]
    at = 0
    for i, t, v, n_in, n_out in cases:
        inside, outside = got[at:at + n_in], got[at + n_in:at + n_in + n_out]
        at += n_in + n_out
        assert (inside > 0).all() and (outside == 0).all(), f"{what}: stream {i} step {t} variable {v}"
        if counts[i] < 2 ** 53:
            assert sum(int(c) for c in inside) == int(counts[i]), f"{what}: stream {i} step {t} variable {v}: the counts add up"
    return len(cases)


def check_twin(stcsp, RefOracle, text, what, mask_names=("default", "all", "hidden"), length=None, brute=True, seed=1, n=5, most=None, prefix_k=2):
    """Twin == the yardstick's recurrences == its brute force on seeded streams at MISSING rates 0, 30 % and 100 %, with and
    without END_FINAL, all five outputs; and the consequences of the contract against the monitor's, the repair's and the
    generator's host twins."""
    m, o, r, a = solved(stcsp, RefOracle, text, prefix_k)
    valid, final, alive = a.flags()
    bounds = m.var_bounds()
    for name, mask in M.masks(m, r).items():
        if name not in mask_names:
            continue
        arg = None if name == "default" else mask
        y = I.Yardstick(r, valid, final, alive, mask)
        L = length or longest_enumerable(y)
        streams = I.make_streams(y, bounds, seed, L, n=n)
        n_obs = sum(mask)
        paths = {0: y.paths(0), L: y.paths(L)} if brute else None
        for end_final in (False, True):
            tag = f"{what} [{name}] end_final={end_final}"
            count, supports, n_states, draws, fin = a.infer_streams(streams, arg, end_final=end_final, draws=2, seed=seed)
            for i, s in enumerate(streams[:most]):
                want = y.dp(s, end_final)
                got = (float(count[i]), supports[i], n_states[i].tolist())
                assert (I.bits(got[0]),) + got[1:] == (I.bits(want[0]),) + want[1:], f"{tag} stream {s.tolist()}: twin {got} yardstick {want}"
                if brute:
                    b = y.brute(s, end_final, paths[len(s)])
                    assert b[:3] == want, f"{tag} stream {s.tolist()}: brute force against the recurrences"
                for j in range(2):  # the samples, bit for bit the Python float walk
                    expect = y.walk(s, i * 2 + j, end_final, seed) if want[0] > 0 else ([[X] * n_obs] * len(s), 0)
                    assert (draws[i][j].tolist(), int(fin[i][j])) == expect, f"{tag} stream {i} draw {j}"
                if brute and 0 < want[0] <= 200:  # every rank: the brute-force list in order
                    k = int(want[0])
                    u = a.infer_streams([s], arg, end_final=end_final, draws=k, ranks=[list(range(k))])
                    assert (u[3][0].tolist(), u[4][0].tolist()) == (b[3], b[4]), f"{tag} stream {i}: unranking every rank"
            # the consequences
            dist, repaired, rfin, _ = a.repair_streams(streams, arg, end_final=end_final)
            assert np.array_equal(count > 0, dist == 0), f"{tag}: count > 0 exactly when the repair's distance is 0"
            acc, nend = a.check_streams(streams, arg)[:2]
            for i, s in enumerate(streams):
                if name == "all" and not end_final and (s != X).all():  # (accepted in a state: without a live root there is none)
                    assert count[i] in (0.0, 1.0) and (count[i] == 1.0) == (acc[i] == len(s) and nend[i] > 0), f"{tag}: fully observed, stream {i}"
                if count[i] > 0:
                    for j in range(2):
                        assert ((s == X) | (s == draws[i][j])).all(), f"{tag}: a draw keeps the observed entries"
                    if count[i] < 2 ** 53:
                        u = a.infer_streams([s], arg, end_final=end_final, draws=1, ranks=[[0]])
                        assert (u[3][0][0].tolist(), int(u[4][0][0])) == (repaired[i].tolist(), int(rfin[i])), f"{tag}: rank 0 is the repair"
            ok = [d for i in range(len(streams)) if count[i] > 0 for d in draws[i]]
            assert (a.check_streams(ok, arg)[0] == [len(d) for d in ok]).all(), f"{tag}: a draw is a prefix of a solution"
            blank = a.infer_streams([np.full((L, n_obs), X, np.int32)], arg, end_final=end_final)[0][0]
            assert I.bits(blank) == I.bits(a.count_streams(L, end_final)[L]), f"{tag}: all MISSING is the generator's count"
        if name == "default" and most is None:
            count, supports = a.infer_streams(streams, arg)[:2]
            missing = [s for s in streams if (s == X).any()]
            assert len(missing) >= 20 or n_obs == 0 or L == 0, f"{what}: {len(missing)} streams with MISSING entries"
            specialisation(a, arg, streams, count, supports, bounds, y.keep, what)


@pytest.mark.parametrize("which", ["COUNTER", "COUNTDOWN", "DUPLICATES"])
def test_twin_on_witness_models(stcsp, RefOracle, which):
    check_twin(stcsp, RefOracle, WITNESS[which], which)


@pytest.mark.parametrize("probe", ["until", "arr", "at", "misc", "adversarial"])
def test_twin_on_probes(stcsp, RefOracle, probe):
    check_twin(stcsp, RefOracle, text_of(stcsp, "probe:" + probe), probe)


@pytest.mark.parametrize("name", SMALLEST_GOLDENS)
def test_twin_on_goldens(stcsp, RefOracle, name):
    check_twin(stcsp, RefOracle, text_of(stcsp, name), name)


def test_twin_at_length_24(stcsp, RefOracle):
    """partialorder_10, 24 steps: far beyond the brute force (8 paths after one step, 2.4e5 after five); the recurrences alone,
    on one sampled prefix at every MISSING rate (the specialisation property is left to the smaller models)."""
    check_twin(stcsp, RefOracle, text_of(stcsp, "partialorder_10"), "partialorder_10", mask_names=("default",), length=24, brute=False, n=1, most=4)


def test_infinite_count(stcsp, RefOracle):
    """A free binary variable, 1,100 unobserved steps: 2^1100 overflows a double, the count is +inf. Supports and |F_t| are still
    exact, draws are refused with STCSP_E_UNSUPPORTED; one observed entry per step brings everything back."""
    m, o, r, a = solved(stcsp, RefOracle, "var x:[0,1];")
    s = np.full((1100, 1), X, np.int32)
    count, supports, n_states, _, _ = a.infer_streams([s], "all")
    assert count[0] == np.inf and supports[0] == [[[0, 1]]] * 1100 and (n_states[0] == 1).all()
    for kw in (dict(seed=3), dict(ranks=[[0]])):
        with pytest.raises(stcsp.StcspError) as ex:
            a.infer_streams([s], "all", draws=1, **kw)
        assert ex.value.code == -2
    s[100:] = 1
    assert one(a, s, [1], draws=1, seed=3)[0] == 2.0 ** 100


def test_invalid_requests(stcsp, RefOracle):
    m, o, r, a = solved(stcsp, RefOracle, COUNTDOWN)
    x = only(m, "x")
    s = np.full((5, 1), X, np.int32)
    with pytest.raises(stcsp.StcspError) as ex:
        a.infer_streams([s], x, draws=-1)
    assert ex.value.code == -1
    assert one(a, s, x, draws=1, ranks=[[7]])[3] == [[[1]] * 5]
    for bad in (8, 2 ** 53, 2 ** 64 - 1):  # not below the count of 8
        with pytest.raises(stcsp.StcspError) as ex:
            a.infer_streams([s], x, draws=1, ranks=[[bad]])
        assert ex.value.code == -1
    for offsets in ([1, 3], [0, 3, 2], [0, -1]):  # not starting at 0, decreasing, negative
        with pytest.raises(stcsp.StcspError) as ex:
            a.infer_streams((np.zeros(max(offsets[-1], 0), np.int32), offsets), x)
        assert ex.value.code == -1
    with pytest.raises(ValueError):
        a.infer_streams([s], x, draws=2, ranks=[[0]])


def test_cli_options(stcsp, tmp_path):
    """--infer= needs a device for the solve; without one the option parsing is what can be checked here: --infer excludes
    --check, --repair, --sample and --count. The round trip itself: tests/test_infer_gpu.py."""
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    (tmp_path / "c.csp").write_text(COUNTDOWN)
    (tmp_path / "s.txt").write_text("# x\n0\n?\n\n")
    for other in ("--check=s.txt", "--repair=s.txt", "--sample=1:1", "--count=2"):
        p = subprocess.run([str(exe), "--infer=s.txt", other, "c.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert p.returncode == 1 and "exclude each other" in p.stderr


def test_infer_abi(stcsp):
    """The new symbols are exported and the new structs have the sizes of include/stcsp_engine.h (LP64)."""
    hip = C.CDLL(str(stcsp.CSRC / "libstcsp_hip.so"))
    assert hasattr(hip, "stcsp_engine_infer")
    assert hasattr(stcsp.host_lib(), "stcsp_automaton_infer_streams")
    assert C.sizeof(stcsp.InferRequest) == 8 + 3 * 8 + 8 + 2 * 4
    assert C.sizeof(stcsp.InferResult) == 8 + 7 * 8 + 2 * 8 + 4 * 4 + 6 * 8
    assert stcsp.INFER_MISSING == stcsp.REPAIR_MISSING == -2 ** 31 and stcsp.INFER_END_FINAL == 1
