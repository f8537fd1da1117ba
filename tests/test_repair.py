"""Repairing observed streams, host side (include/stcsp_host.h: stcsp_automaton_repair_streams): the CPU twin of the device
pass against an independent yardstick -- the plain Python of tests/repair_ref.py, its recurrence and its brute force, run on
the automaton of the CPU oracle. Everything is integer arithmetic and compared with ==. The device pass itself:
tests/test_repair_gpu.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import monitor_ref as M
import repair_ref as R
from test_generate import NO_LIVE_ROOT, UNTIL, solved, text_of
from test_quotient import COUNTDOWN, COUNTER, DUPLICATES, SMALLEST_GOLDENS

WITNESS = {"COUNTER": COUNTER, "COUNTDOWN": COUNTDOWN, "DUPLICATES": DUPLICATES}
X = R.MISSING


def only(model, *names):
    assert all(n in model.var_names for n in names)
    return [int(n in names) for n in model.var_names]


def column(model, mask, name):
    return [n for n, k in zip(model.var_names, mask) if k].index(name)


def one(a, stream, observable, **kw):
    dist, values, fin, nchg = a.repair_streams([np.array(stream, dtype=np.int32)], observable, **kw)
    return int(dist[0]), values[0].tolist(), int(fin[0]), int(nchg[0])


def test_hand_derived_countdown(stcsp, RefOracle):
    """COUNTDOWN: c runs 0, 1, 2, 3, 3 and x must be 1 while c == 3, that is at steps 3 and 4; x is free before. Under x alone:
    0,0,0,0,0 has two wrong steps and the nearest prefix is 0,0,0,1,1; with weight 3 on x the distance is 6; 1,1,1,1,1 is a
    prefix; five unobserved steps repair to the lexicographically least path, which is again 0,0,0,1,1, at distance 0. The model
    has no `until`, so every state is final."""
    m, o, r, a = solved(stcsp, RefOracle, COUNTDOWN)
    x = only(m, "x")
    assert one(a, [[0]] * 5, x) == (2, [[0], [0], [0], [1], [1]], 1, 2)
    assert one(a, [[1]] * 5, x) == (0, [[1]] * 5, 1, 0)
    assert one(a, [[0]] * 5, x, weights=[3]) == (6, [[0], [0], [0], [1], [1]], 1, 2)
    assert one(a, [[X]] * 5, x) == (0, [[0], [0], [0], [1], [1]], 1, 0)
    assert one(a, [[0]] * 5, x, weights=[0]) == (0, [[0], [0], [0], [1], [1]], 1, 2)  # a weight of 0: free to change


def test_hand_derived_counter(stcsp, RefOracle):
    """COUNTER with x and c observable: c is a function of time, 0, 1, 2, 3, 3, and x is free. c = 0,0,0,0,0 is wrong at four
    steps; x stays what it was."""
    m, o, r, a = solved(stcsp, RefOracle, COUNTER)
    mask = only(m, "x", "c")
    ix, ic = column(m, mask, "x"), column(m, mask, "c")
    xs = [1, 0, 1, 1, 0]
    stream = np.zeros((5, 2), np.int32)
    stream[:, ix] = xs
    d, rows, fin, nchg = one(a, stream, mask)
    assert (d, nchg) == (4, 4)
    assert [row[ic] for row in rows] == [0, 1, 2, 3, 3] and [row[ix] for row in rows] == xs


def test_hand_derived_until(stcsp, RefOracle):
    """UNTIL, x until y: the root waits for y and is not final; from it (x, y) = (1, 0) stays, (0, 1) and (1, 1) lead to the one
    final state, where every row is allowed. The stream (1,0), (1,0), (1,0) is a prefix of a solution and ends in the waiting
    state: distance 0, end_final 0. A prefix that ends in a final state needs y == 1 once: distance 1; among the three ways
    to set one y the least in lexicographic order of the rows keeps (1,0) < (1,1) as long as it can, so the last step
    changes. (0,0) at the first step has no edge at all: x or y must change, (0,1) < (1,0) wins, and the run is final at once."""
    m, o, r, a = solved(stcsp, RefOracle, UNTIL)
    mask = only(m, "x", "y")
    assert [n for n, k in zip(m.var_names, mask) if k] == ["x", "y"]
    wait = [[1, 0]] * 3
    assert one(a, wait, mask) == (0, wait, 0, 0)
    assert one(a, wait, mask, end_final=True) == (1, [[1, 0], [1, 0], [1, 1]], 1, 1)
    assert one(a, [[0, 0], [0, 0]], mask) == (1, [[0, 1], [0, 0]], 1, 1)
    assert one(a, [], mask) == (0, [], 0, 0)
    assert one(a, [], mask, end_final=True) == (-1, [], 0, 0)  # the root is not final


def test_no_live_root(stcsp, RefOracle):
    m, o, r, a = solved(stcsp, RefOracle, NO_LIVE_ROOT)
    mask = only(m, "x", "y")
    assert one(a, [[1, 0]] * 3, mask) == (-1, [[0, 0]] * 3, 0, 0)
    assert one(a, [], mask) == (-1, [], 0, 0)


def longest_enumerable(y, limit=5000, cap=7):
    return max([t for t in range(1, cap + 1) if 0 < y.n_paths(t) <= limit], default=0)


def check_twin(stcsp, RefOracle, text, what, mask_names=("default", "all", "hidden"), length=None, brute=True, seed=1, first=0, most=100, prefix_k=2):
    """Twin == the yardstick's recurrence == its brute force on seeded streams, all four outputs; and the properties of the
    contract against the monitor's and the generator's host twins."""
    m, o, r, a = solved(stcsp, RefOracle, text, prefix_k)
    valid, final, alive = a.flags()
    for name, mask in M.masks(m, r).items():
        if name not in mask_names:
            continue
        arg = None if name == "default" else mask
        y = R.Yardstick(r, valid, final, alive, mask)
        L = length or longest_enumerable(y)
        streams = R.make_streams(y, m.var_bounds(), seed, L)[first:]
        n_obs = sum(mask)
        rng = np.random.RandomState(seed)
        variants = [dict(), dict(end_final=True), dict(weights=[int(w) for w in rng.randint(0, 5, size=n_obs)])]
        for kw in variants:
            got = R.unpack(a.repair_streams(streams, arg, **kw))
            for j, (s, g) in enumerate(zip(streams, got)):
                if j >= most:
                    break
                want = y.dp(s, **kw)
                assert g == want, f"{what} [{name}] {kw} stream {s.tolist()}: twin {g} yardstick {want}"
                if brute and j < 7:  # (one stream of every kind make_streams() has)
                    assert y.brute(s, **kw) == want, f"{what} [{name}] {kw} stream {s.tolist()}: brute force against the recurrence"
        # the properties, on the plain variant
        dist, values, fin, nchg = a.repair_streams(streams, arg)
        acc, nend = a.check_streams(streams, arg)[:2]
        for i, s in enumerate(streams):
            if (s != X).all() and n_obs:  # (accepted in some state: without a live root the monitor "accepts" the empty stream in none)
                assert (dist[i] == 0) == (acc[i] == len(s) and nend[i] > 0), f"{what} [{name}]: distance 0 exactly when the monitor accepts"
            if dist[i] == 0 and (s != X).all():
                assert np.array_equal(values[i], s)
            if dist[i] >= 0:
                assert nchg[i] == int(((s != X) & (s != values[i])).sum())
        ok = [v for d, v in zip(dist, values) if d >= 0]
        assert (a.check_streams(ok, arg)[0] == [len(v) for v in ok]).all(), f"{what} [{name}]: a repaired stream is a prefix of a solution"
        if y.n_paths(L) > 0:  # all-MISSING == the generator's rank 0
            d0, v0, f0, c0 = one(a, [[X] * n_obs] * L, arg)
            gv, gf, _ = a.generate(1, L, ranks=[0], observable=arg) if y.n_paths(L) < 2 ** 53 else (None, None, None)
            if gv is not None:
                assert (d0, v0, f0, c0) == (0, gv[0].tolist(), int(gf[0]), 0), f"{what} [{name}]: all-MISSING"
            # never farther than a sampled solution prefix
            gs = a.generate(20, L, seed=seed, observable=arg)[0]
            for i, s in enumerate(streams):
                if len(s) == L and dist[i] >= 0:
                    least = min(int(((s != X) & (s != g)).sum()) for g in gs)
                    assert dist[i] <= least, f"{what} [{name}]: a sampled prefix is nearer than the repair"


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
    """partialorder_10, 24 steps: far beyond the brute force (8 paths after one step, 2.4e5 after five); the recurrence alone."""
    check_twin(stcsp, RefOracle, text_of(stcsp, "partialorder_10"), "partialorder_10", mask_names=("default",), length=24, brute=False, first=3, most=1)


def test_invalid_requests(stcsp, RefOracle):
    m, o, r, a = solved(stcsp, RefOracle, COUNTDOWN)
    x = only(m, "x")
    s = np.zeros((3, 1), np.int32)
    with pytest.raises(stcsp.StcspError) as ex:
        a.repair_streams([s], x, weights=[-1])
    assert ex.value.code == -1
    # (sum of the weights) x (longest stream) may reach 2^31 - 2 and no more
    big = (2 ** 31 - 2) // 3
    assert one(a, s, x, weights=[big])[0] == 0
    with pytest.raises(stcsp.StcspError) as ex:
        a.repair_streams([s], x, weights=[big + 1])
    assert ex.value.code == -1
    for offsets in ([1, 3], [0, 3, 2], [0, -1]):  # not starting at 0, decreasing, negative
        with pytest.raises(stcsp.StcspError) as ex:
            a.repair_streams((np.zeros(max(offsets[-1], 0), np.int32), offsets), x)
        assert ex.value.code == -1


def test_cli_round_trip_on_the_host_twin(stcsp, tmp_path):
    """--repair= with --shards=2 (the merged automaton lives on the host: the twin) needs a device; without one the option
    parsing is what can be checked here: --repair excludes --check, --sample and --count. The round trip itself:
    tests/test_repair_gpu.py."""
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    (tmp_path / "c.csp").write_text(COUNTDOWN)
    (tmp_path / "s.txt").write_text("# x\n0\n?\n\n")
    for other in ("--check=s.txt", "--sample=1:1", "--count=2"):
        p = subprocess.run([str(exe), "--repair=s.txt", other, "c.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert p.returncode == 1 and "exclude each other" in p.stderr


def test_repair_abi(stcsp):
    """The new symbols are exported and the new structs have the sizes of include/stcsp_engine.h (LP64)."""
    hip = C.CDLL(str(stcsp.CSRC / "libstcsp_hip.so"))
    assert hasattr(hip, "stcsp_engine_repair")
    assert hasattr(stcsp.host_lib(), "stcsp_automaton_repair_streams")
    assert C.sizeof(stcsp.RepairRequest) == 8 + 3 * 8 + 2 * 4
    assert C.sizeof(stcsp.RepairResult) == 8 + 4 * 8 + 2 * 8 + 2 * 4 + 4 * 8
    assert stcsp.REPAIR_MISSING == -2 ** 31 and stcsp.REPAIR_END_FINAL == 1
