"""Counting, unranking and sampling solution prefixes on the device (stcsp_engine_generator_build / stcsp_engine_generate,
dev_generate.hpp) through the C ABI, against the host twin on the same automaton and flags and against the independent yardstick
of tests/generate_ref.py (plain Python floats over the automaton of the CPU oracle). Run on the GPU box: pytest -m gpu.

count[] and the streams depend on no state or edge number, so the device, the host twin and the yardstick -- which runs on the
ORACLE's automaton, numbered differently -- are compared directly, and nothing is compared with a tolerance: the contract fixes
the order of every floating-point sum."""
import subprocess

import numpy as np
import pytest

import generate_ref as G
import monitor_ref as M
import quotient_ref as Q
from test_quotient import COUNTDOWN, COUNTER, DUPLICATES, PROBES, SMALLEST_GOLDENS

pytestmark = pytest.mark.gpu

UNTIL = "var x:[0,1]; var y:[0,1]; x until y;"
NO_LIVE_ROOT = "var x:[0,1]; var y:[0,1]; x until y; y == 0;"
# one state whose 8,192 out-edges are past kGenWaveSegment (4,096) of dev_generate.hpp: the one-lane road of k_g_order
WIDE = "var x:[0,127]; var y:[0,63];"
# tests/test_monitor_gpu.py: the adversary e is variable 5. t remembers the last d4, and a state with t == 1 offers e == 0 only:
# the adversarial pass drops it and the edges into it; the root and the state with t == 0 survive.
PRUNED_BY_ADVERSARY = ("var d0:[0,0]; var d1:[0,0]; var d2:[0,0]; var d3:[0,0]; var d4:[0,1]; var e:[0,1]; var t:[0,1]; "
                       "first t == 0; next t == d4; (t eq 1) -> (e eq 0);")
WITNESS = {"COUNTER": COUNTER, "COUNTDOWN": COUNTDOWN, "DUPLICATES": DUPLICATES}


def solved(stcsp, m, adversarial=-1, **opts):
    e = stcsp.Engine(m, **opts)
    r = e.solve()
    post = e.postprocess(adversarial=adversarial)
    host = e.automaton(r).import_flags(post)
    return e, r, post, host


def some_ranks(count, seed):
    n = int(count)
    rng = np.random.RandomState(seed)
    return np.array(sorted({0, 1 % n, n - 1, n // 2} | {int(rng.randint(0, min(n, 2 ** 62))) for _ in range(12)}), dtype=np.uint64)


def check_device(stcsp, RefOracle, m, what, horizon=32, oracle=True, masks=("default", "all"), n=100):
    """Device == host twin on the same automaton == yardstick on the oracle's automaton: count, sampled and unranked streams,
    end_final; the device's own monitor accepts every stream whole."""
    e, r, post, host = solved(stcsp, m)
    if oracle:
        o = RefOracle(m)
        ro = o.solve()
        flags, rr = o.automaton(ro).traverse().flags(), ro
    for name, mask in M.masks(m, r).items():
        if name not in masks:
            continue
        arg = None if name == "default" else mask
        info = e.generator(arg, horizon)
        assert (info.n_observable, info.horizon) == (sum(mask), horizon) and len(info.count) == horizon + 1, f"{what} [{name}]"
        hcount = host.count_streams(horizon)
        assert np.array_equal(info.count, hcount), f"{what} [{name}]: count, device {info.count} host twin {hcount}"
        y = None
        if oracle:
            y = G.Yardstick(rr, *flags, mask, horizon)
            assert np.array_equal(info.count, y.count), f"{what} [{name}]: count against the yardstick"
            assert (info.n_states, info.n_edges, info.max_out_degree, info.root_live) == (len(y.live), y.n_edges(), y.max_out_degree(), int(bool(y.live)))
        print(f"{what} [{name}]: live {info.n_states} edges {info.n_edges} max out-degree {info.max_out_degree} count[{horizon}] {info.count[horizon]:.6g}")
        e.monitor(arg)  # the two sets of structures live apart: building the monitor's leaves the generator's valid
        exact = [t for t in range(horizon + 1) if 0 < info.count[t] < 2.0 ** 53]
        for length, seed in ((horizon, 0), (horizon, 7), (1, 0), (horizon // 3, 7)):
            if info.count[length] == 0:  # no prefix of that length: both refuse
                for run in (lambda: e.generate(n, length, seed), lambda: host.generate(n, length, seed, observable=arg, horizon=horizon)):
                    with pytest.raises(stcsp.StcspError) as ex:
                        run()
                    assert ex.value.code == -1, f"{what} [{name}] len {length}"
                continue
            dev = e.generate(n, length, seed)
            hst = host.generate(n, length, seed, observable=arg, horizon=horizon)
            assert np.array_equal(dev[0], hst[0]) and np.array_equal(dev[1], hst[1]), f"{what} [{name}] seed {seed} len {length}: device and host twin differ"
            if y is not None:
                yv, yf = y.streams(n, length, seed)
                assert np.array_equal(dev[0], yv) and np.array_equal(dev[1], yf), f"{what} [{name}] seed {seed} len {length}: device and yardstick differ"
            acc = e.check_streams(list(dev[0]))[0]
            assert (acc == length).all(), f"{what} [{name}]: a generated stream is a prefix of a solution"
        if exact:
            L = exact[-1]
            ranks = some_ranks(info.count[L], L)
            dev = e.generate(len(ranks), L, ranks=ranks)
            hst = host.generate(len(ranks), L, ranks=ranks, observable=arg, horizon=horizon)
            assert np.array_equal(dev[0], hst[0]) and np.array_equal(dev[1], hst[1]), f"{what} [{name}] unrank at {L}: device and host twin differ"
            if y is not None:
                yv, yf = y.streams(len(ranks), L, ranks=ranks)
                assert np.array_equal(dev[0], yv) and np.array_equal(dev[1], yf), f"{what} [{name}] unrank at {L}: device and yardstick differ"
            assert (e.check_streams(list(dev[0]))[0] == L).all()
            if name == "all":  # full rows: increasing ranks give strictly increasing streams
                got = [tuple(map(tuple, s)) for s in dev[0].tolist()]
                assert all(a < b for a, b in zip(got, got[1:])), f"{what} [all]: lexicographic order"
            with pytest.raises(stcsp.StcspError) as ex:
                e.generate(1, L, ranks=[int(info.count[L])])
            assert ex.value.code == -1


@pytest.mark.parametrize("which", ["COUNTER", "COUNTDOWN", "DUPLICATES"])
def test_device_on_witness_models(stcsp, RefOracle, which):
    check_device(stcsp, RefOracle, stcsp.Model(text=WITNESS[which]), which, masks=("default", "all", "hidden"))


@pytest.mark.parametrize("probe", ["until", "arr", "at", "misc", "adversarial"])
def test_device_on_probes(stcsp, RefOracle, probe):
    check_device(stcsp, RefOracle, stcsp.Model(text=PROBES[probe]["text"]), probe, masks=("default", "all", "hidden"))


@pytest.mark.parametrize("name", SMALLEST_GOLDENS + ["digitinvader3", "partialorder_10"])
def test_device_on_goldens(stcsp, RefOracle, name):
    check_device(stcsp, RefOracle, stcsp.Model.from_name(name), name)


def test_hand_derived_on_the_device(stcsp):
    """tests/test_generate.py derives these by hand: COUNTDOWN's counts, its unranking under x alone, UNTIL's counts of the
    prefixes that end in a final state."""
    m = stcsp.Model(text=COUNTDOWN)
    e, r, post, host = solved(stcsp, m)
    info = e.generator([int(n == "x") for n in m.var_names], 8)
    assert info.count.tolist() == [1, 2, 4, 8, 8, 8, 8, 8, 8]
    values, fin = e.generate(8, 5, ranks=np.arange(8))
    for rank in range(8):
        assert values[rank, :, 0].tolist() == [rank >> 2 & 1, rank >> 1 & 1, rank & 1, 1, 1]
    e, r, post, host = solved(stcsp, stcsp.Model(text=UNTIL))
    assert e.generator("all", 8).count.tolist() == [1, 3, 11, 43, 171, 683, 2731, 10923, 43691]
    info = e.generator("all", 8, end_final=True)
    assert info.count.tolist() == [0, 2, 10, 42, 170, 682, 2730, 10922, 43690]
    with pytest.raises(stcsp.StcspError) as ex:  # no prefix of length 0 ends in a final state
        e.generate(1, 0)
    assert ex.value.code == -1
    values, fin = e.generate(170, 4, ranks=np.arange(170))
    hv, hf, _ = host.generate(170, 4, ranks=np.arange(170), observable="all", horizon=8, end_final=True)
    assert fin.all() and np.array_equal(values, hv) and len({tuple(map(tuple, s)) for s in values.tolist()}) == 170


def test_smallest_shapes(stcsp):
    """Stream counts around the wavefront and the block, lengths 0 and 1, horizon 0, a mask without a variable."""
    m = stcsp.Model.from_name("juggling_b4_f5")
    e, r, post, host = solved(stcsp, m)
    e.generator(None, 6)
    for n in (0, 1, 63, 64, 65, 1000):
        for length in (0, 1, 6):
            dev = e.generate(n, length, seed=n)
            hst = host.generate(n, length, seed=n, horizon=6)
            assert dev[0].shape == (n, length, e.generator_info.n_observable)
            assert np.array_equal(dev[0], hst[0]) and np.array_equal(dev[1], hst[1]), (n, length)
    with pytest.raises(stcsp.StcspError) as ex:  # beyond the horizon
        e.generate(1, 7)
    assert ex.value.code == -1
    info = e.generator("all", 0)
    assert info.count.tolist() == [1.0]
    dev = e.generate(65, 0)
    assert dev[0].shape == (65, 0, m.n_vars) and np.array_equal(dev[1], host.generate(65, 0, observable="all")[1])
    info = e.generator([0] * m.n_vars, 5)
    assert info.n_observable == 0 and np.array_equal(info.count, host.count_streams(5))
    dev = e.generate(65, 5, seed=1)
    assert dev[0].shape == (65, 5, 0) and np.array_equal(dev[1], host.generate(65, 5, seed=1, observable=[0] * m.n_vars)[1])


def test_out_degree_720(stcsp):
    """juggling_b6_f6_nosym: 720 edges leave the root, twelve chunks of 64 in k_g_order. The oracle takes 45 s on it: the host
    twin is the comparison."""
    m = stcsp.Model.from_name("juggling_b6_f6_nosym")
    e, r, post, host = solved(stcsp, m)
    info = e.generator(None, 32)
    assert info.max_out_degree == 720
    assert np.array_equal(info.count, host.count_streams(32))
    for length, seed in ((32, 0), (1, 7)):
        dev = e.generate(200, length, seed)
        hst = host.generate(200, length, seed, horizon=32)
        assert np.array_equal(dev[0], hst[0]) and np.array_equal(dev[1], hst[1])
    ranks = np.arange(720, dtype=np.uint64)  # every edge of the root, in canonical order
    info = e.generator("all", 1)
    assert info.count.tolist() == [1.0, 720.0]
    dev = e.generate(720, 1, ranks=ranks)
    rows = [tuple(x[0]) for x in dev[0].tolist()]
    assert rows == sorted(rows) and len(set(rows)) == 720
    assert np.array_equal(dev[0], host.generate(720, 1, ranks=ranks, observable="all")[0])


def test_segment_past_the_wave_threshold(stcsp):
    """WIDE: one live state, 8,192 loops. x is variable 0 and y variable 1, so the canonical order is (x, y) and the rank of
    a step is x * 64 + y: checked by arithmetic."""
    m = stcsp.Model(text=WIDE)
    assert m.var_names[:2] == ["x", "y"]
    e, r, post, host = solved(stcsp, m)
    info = e.generator("all", 2)
    assert (info.n_states, info.n_edges, info.max_out_degree) == (1, 8192, 8192)
    assert info.count.tolist() == [1.0, 8192.0, 8192.0 ** 2]
    ranks = np.array([0, 1, 63, 64, 65, 4095, 4096, 4097, 5000, 8190, 8191], dtype=np.uint64)
    values, fin = e.generate(len(ranks), 1, ranks=ranks)
    assert values[:, 0, 0].tolist() == [int(k) >> 6 for k in ranks] and values[:, 0, 1].tolist() == [int(k) & 63 for k in ranks]
    two = np.array([0, 8191, 8192, 12345678, 8192 ** 2 - 1], dtype=np.uint64)
    values, fin = e.generate(len(two), 2, ranks=two)
    for row, k in zip(values.tolist(), two.tolist()):
        first, second = k >> 13, k & 8191
        assert row == [[first >> 6, first & 63], [second >> 6, second & 63]]
    dev = e.generate(300, 2, seed=4)
    hst = host.generate(300, 2, seed=4, observable="all")
    assert np.array_equal(dev[0], hst[0])


def test_no_live_root(stcsp):
    m = stcsp.Model(text=NO_LIVE_ROOT)
    e, r, post, host = solved(stcsp, m)
    info = e.generator(None, 5)
    assert info.root_live == 0 and info.n_states == 0 and info.count.tolist() == [0.0] * 6
    for n, length in ((3, 0), (3, 2), (0, 2)):
        with pytest.raises(stcsp.StcspError) as ex:
            e.generate(n, length)
        assert ex.value.code == -1


def test_counts_follow_the_flags_of_a_second_postprocess(stcsp):
    """Derived by hand. Before: from the root and from the state with t == 0, d4 and e are free (4 edges, two into each of the
    states t == 0 and t == 1); from t == 1, e == 0 (2 edges, one into each). With a = W(t == 0) and b = W(t == 1):
    a' = 2a + 2b, b' = a + b, count = 1, 4, 12, 36, 108, 324. After -a the state t == 1 and the edges into it are gone: 2 states,
    4 edges, count[t] = 2^t."""
    m = stcsp.Model(text=PRUNED_BY_ADVERSARY)
    e = stcsp.Engine(m)
    r = e.solve()
    e.postprocess()
    info = e.generator("all", 5)
    assert (info.n_states, info.n_edges, info.max_out_degree) == (3, 10, 4)
    assert info.count.tolist() == [1, 4, 12, 36, 108, 324]
    before = e.generate(50, 5, seed=2)[0]
    post = e.postprocess(adversarial=5)
    with pytest.raises(stcsp.StcspError) as ex:  # the structures are invalidated
        e.generate(50, 5, seed=2)
    assert ex.value.code == -6
    info = e.generator("all", 5)
    assert (info.n_states, info.n_edges, info.max_out_degree) == (2, 4, 2)
    assert info.count.tolist() == [1, 2, 4, 8, 16, 32]
    after = e.generate(32, 5, ranks=np.arange(32))[0]
    d4, adv = m.var_names.index("d4"), m.var_names.index("e")
    assert (after[:, :, d4] == 0).all() and (before[:, :, d4] == 1).any()
    assert [sum(int(x) << (4 - t) for t, x in enumerate(s[:, adv])) for s in after] == list(range(32))  # e is the only free variable
    host = e.automaton(r).import_flags(post)
    assert np.array_equal(after, host.generate(32, 5, ranks=np.arange(32), observable="all")[0])


def test_contract_errors(stcsp):
    m = stcsp.Model.from_name("partialorder_10")
    e = stcsp.Engine(m)
    with pytest.raises(stcsp.StcspError) as ex:  # before any solve
        e.generator()
    assert ex.value.code == -6
    e.solve()
    with pytest.raises(stcsp.StcspError) as ex:  # before postprocess
        e.generator()
    assert ex.value.code == -6
    e.postprocess()
    with pytest.raises(stcsp.StcspError) as ex:  # generate before generator_build
        e.generate(1, 1)
    assert ex.value.code == -6
    with pytest.raises(stcsp.StcspError) as ex:
        e.generator(horizon=-1)
    assert ex.value.code == -1
    info = e.generator("all", 12)
    assert info.count[3] == 1600
    e.generate(4, 3, ranks=[0, 1, 2, 1599])
    for bad in ([0, 1, 2, 1600], [2 ** 64 - 1, 0, 0, 0], [2 ** 53, 0, 0, 0]):  # malformed ranks
        with pytest.raises(stcsp.StcspError) as ex:
            e.generate(4, 3, ranks=bad)
        assert ex.value.code == -1
    with pytest.raises(stcsp.StcspError) as ex:  # beyond the horizon
        e.generate(1, 13)
    assert ex.value.code == -1
    info = e.generator("all", 64)  # count[64] = 1.2e65: sampling works, unranking is refused
    assert info.count[64] > 2.0 ** 64
    e.generate(3, 64)
    with pytest.raises(stcsp.StcspError) as ex:
        e.generate(1, 64, ranks=[0])
    assert ex.value.code == -1
    assert len(e.generate(0, 5)[0]) == 0  # n_streams = 0
    e.postprocess()  # a second postprocess invalidates the structures
    with pytest.raises(stcsp.StcspError) as ex:
        e.generate(1, 1)
    assert ex.value.code == -6
    e.generator("all", 4)
    e.solve()  # and so does a new solve
    with pytest.raises(stcsp.StcspError) as ex:
        e.generate(1, 1)
    assert ex.value.code == -6
    t = stcsp.Engine(m, max_search_nodes=2000, batch_nodes=256)  # truncated solve
    assert t.solve().truncated == 1
    t.postprocess()
    with pytest.raises(stcsp.StcspError) as ex:
        t.generator()
    assert ex.value.code == -6
    s = stcsp.Engine(m, flags=stcsp.F_STEPPED)  # the sharded pipeline
    with pytest.raises(stcsp.StcspError) as ex:
        s.generator()
    assert ex.value.code == -2


def test_cli_round_trip(stcsp, tmp_path):
    """--sample prints what Engine.generate() returns, in the format --check reads: fed back, every stream is accepted whole.
    --shards=2 (the host twin on the merged automaton) prints the same bytes. --count prints COUNTDOWN's hand-derived numbers."""
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    m = stcsp.Model.from_name("juggling_b4_f5")
    (tmp_path / "m.csp").write_text(stcsp.instances.by_name("juggling_b4_f5"))
    e, r, post, host = solved(stcsp, m)
    e.generator(None, 30)
    values, fin = e.generate(20, 30, seed=3)
    names = [n for n, k in zip(m.var_names, Q.default_mask(m.var_names)) if k]
    expect = "# " + " ".join(names) + "\n" + "".join("".join(" ".join(str(x) for x in row) + "\n" for row in s) + "\n" for s in values.tolist())
    outs = []
    for extra in ((), ("--shards=2",)):
        p = subprocess.run([str(exe), *extra, "--sample=20:30:3", "m.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert p.returncode == 0, p.stderr
        outs.append(p.stdout)
    assert outs[0] == expect and outs[1] == outs[0]
    (tmp_path / "streams.txt").write_text(outs[0])
    p = subprocess.run([str(exe), "--check=streams.txt", "m.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    lines = [l.split() for l in p.stdout.splitlines()]
    assert len(lines) == 20 and all(l[1] == l[2] == "30" for l in lines)
    (tmp_path / "c.csp").write_text(COUNTDOWN)
    for extra in ((), ("--shards=2",)):
        p = subprocess.run([str(exe), *extra, "--count=8", "c.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert p.returncode == 0, p.stderr
        assert p.stdout.splitlines() == [f"{t} {c}" for t, c in enumerate([1, 2, 4, 8, 8, 8, 8, 8, 8])]
