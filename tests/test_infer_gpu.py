"""Inferring the unobserved entries of streams on the device (stcsp_engine_infer, dev_infer.hpp) through the C ABI, against the
host twin on the same automaton and flags and against the independent yardstick of tests/infer_ref.py (plain Python over the
automaton of the CPU oracle). Run on the GPU box: pytest -m gpu.

Counts, supports, |F_t|, draws and end_final depend on no state or edge number, so the device, the host twin and the yardstick
-- which runs on the ORACLE's automaton, numbered differently -- are compared directly, with ==, the doubles by their bits."""
import subprocess

import numpy as np
import pytest

import infer_ref as I
import monitor_ref as M
import quotient_ref as Q
from test_generate_gpu import NO_LIVE_ROOT, PRUNED_BY_ADVERSARY, UNTIL, WIDE, WITNESS, solved
from test_quotient import COUNTDOWN, PROBES

pytestmark = pytest.mark.gpu

X = I.MISSING
# x alternates between two values a million apart, y is free: the dictionary of x has 2 entries, not ub - lb + 1
FAR_APART = "var x:[0,1000000]; var y:[0,1]; first x == 0; next x == (if (x eq 0) then 1000000 else 0);"


def counter(n):
    """A model with exactly n live states in a row: c0 counts 0 .. top0 and stays, c1 counts once c0 is at its top, and so
    on; every domain has at most 128 values. x is free: two edges leave every state."""
    tops, left = [], n - 1
    while left > 0:
        tops.append(min(left, 127))
        left -= tops[-1]
    text = "var x:[0,1]; " + " ".join(f"var c{i}:[0,{t}]; first c{i} == 0;" for i, t in enumerate(tops))
    for i, t in enumerate(tops):
        step = f"if (c{i} lt {t}) then (c{i} + 1) else {t}"
        text += f" next c{i} == " + (step if i == 0 else f"if (c{i - 1} eq {tops[i - 1]}) then ({step}) else 0") + ";"
    return text


def same(a, b):
    """All five outputs, the counts by their bits."""
    return I.unpack(a) == I.unpack(b)


def blanked(streams, rate, seed):
    rng = np.random.RandomState(seed)
    return [I.blank(s, rate, rng) for s in streams]


def check_device(stcsp, RefOracle, m, what, masks=("default", "all"), lengths=(4, 9), seed=3, engine=None):
    """Device == host twin on the same automaton == yardstick on the oracle's automaton, all five outputs, with and without
    END_FINAL, sampled and unranked."""
    e, r, post, host = engine or solved(stcsp, m)
    o = RefOracle(m)
    ro = o.solve()
    flags = o.automaton(ro).traverse().flags()
    for name, mask in M.masks(m, r).items():
        if name not in masks:
            continue
        arg = None if name == "default" else mask
        n_obs = sum(mask)
        y = I.Yardstick(ro, *flags, mask)
        info = e.generator(arg, 0)  # the horizon does not limit the inference
        streams = [s for L in lengths for s in I.make_streams(y, m.var_bounds(), seed + L, L, n=2)]
        few = range(len(streams)) if info.n_edges <= 2000 else range(1, 4)  # the plain Python recurrences then take a few streams only
        for end_final in (False, True):
            tag = f"{what} [{name}] end_final={end_final}"
            dev = e.infer_streams(streams, end_final=end_final, draws=2, seed=seed)
            res = e.infer_result
            # without a live root nothing runs on the device: no batch, as for the repair
            assert (res.n_batches, res.n_observable, res.draws) == (1 if info.root_live else 0, n_obs, 2)
            assert same(dev, host.infer_streams(streams, arg, end_final=end_final, draws=2, seed=seed)), f"{tag}: device and host twin differ"
            got = I.unpack(dev)
            for i in few:
                count, supports, n_states = y.dp(streams[i], end_final)
                assert got[i][:3] == (I.bits(count), supports, n_states), f"{tag} stream {i}: device and yardstick differ"
                for j in range(2):
                    expect = y.walk(streams[i], i * 2 + j, end_final, seed) if count > 0 else ([[X] * n_obs] * len(streams[i]), 0)
                    assert (got[i][3][j], got[i][4][j]) == expect, f"{tag} stream {i} draw {j}"
            ranks = [[0, int(min(c, 2.0 ** 52)) - 1] if c > 0 else [0, 0] for c in dev[0]]
            if all(c < 2.0 ** 53 for c in dev[0]):
                un = e.infer_streams(streams, end_final=end_final, draws=2, ranks=ranks)
                assert same(un, host.infer_streams(streams, arg, end_final=end_final, draws=2, ranks=ranks)), f"{tag}: unranking"
                for i in few:
                    if dev[0][i] > 0:
                        for j in range(2):
                            assert (un[3][i][j].tolist(), int(un[4][i][j])) == y.walk(streams[i], 0, end_final, rank=ranks[i][j]), f"{tag} stream {i}"
        print(f"{what} [{name}]: live {info.n_states} edges {info.n_edges} labels {e.infer_result.n_labels} streams {len(streams)}")


@pytest.mark.parametrize("which", ["COUNTER", "COUNTDOWN", "DUPLICATES"])
def test_device_on_witness_models(stcsp, RefOracle, which):
    check_device(stcsp, RefOracle, stcsp.Model(text=WITNESS[which]), which, masks=("default", "all", "hidden"))


@pytest.mark.parametrize("probe", ["until", "adversarial"])
def test_device_on_probes(stcsp, RefOracle, probe):
    check_device(stcsp, RefOracle, stcsp.Model(text=PROBES[probe]["text"]), probe, masks=("default", "all", "hidden"))


@pytest.mark.parametrize("text", [UNTIL, NO_LIVE_ROOT], ids=["UNTIL", "NO_LIVE_ROOT"])
def test_device_on_until_and_no_live_root(stcsp, RefOracle, text):
    check_device(stcsp, RefOracle, stcsp.Model(text=text), "until", masks=("all",), lengths=(0, 3))


def test_hand_derived_on_the_device(stcsp):
    """tests/test_infer.py derives these by hand."""
    m = stcsp.Model(text=COUNTDOWN)
    e, r, post, host = solved(stcsp, m)
    e.generator([int(n == "x") for n in m.var_names], 0)
    s = [np.array(rows, np.int32).reshape(5, 1) for rows in ([X] * 5, [X, 1, X, X, X], [X, X, X, 0, X])]
    count, supports, n_states, draws, fin = e.infer_streams(s, draws=8, ranks=[list(range(8)), [0, 1, 2, 3] * 2, [99] * 8])
    free, forced = [[0, 1]], [[1]]
    assert count.tolist() == [8.0, 4.0, 0.0]
    assert supports == [[free, free, free, forced, forced], [free, forced, free, forced, forced], [[[]]] * 5]
    assert [k.tolist() for k in n_states] == [[1] * 6, [1] * 6, [0] * 6]
    assert draws[0].tolist() == [[[k >> 2 & 1], [k >> 1 & 1], [k & 1], [1], [1]] for k in range(8)] and fin[0].tolist() == [1] * 8
    assert (draws[2] == X).all() and fin[2].tolist() == [0] * 8
    m = stcsp.Model(text=UNTIL)
    e, r, post, host = solved(stcsp, m)
    e.generator([int(n in "xy") for n in m.var_names], 0)
    s = [np.array([[X, X]] * 2, np.int32), np.array([[1, 0], [X, X]], np.int32), np.zeros((0, 2), np.int32)]
    both = [[0, 1], [0, 1]]
    count, supports, n_states, _, _ = e.infer_streams(s)
    assert (count.tolist(), supports, [k.tolist() for k in n_states]) == ([11.0, 3.0, 1.0], [[both, both], [[[1], [0]], both], []], [[1, 2, 2], [1, 1, 2], [1]])
    count, supports, n_states, _, _ = e.infer_streams(s, end_final=True)
    assert (count.tolist(), supports, [k.tolist() for k in n_states]) == ([10.0, 2.0, 0.0], [[both, both], [[[1], [0]], [[0, 1], [1]]], []],
                                                                             [[1, 2, 1], [1, 1, 1], [0]])


@pytest.mark.parametrize("n", [63, 64, 65, 1025])
def test_live_state_counts_around_a_wavefront_and_a_block(stcsp, n):
    """n live states in a row, two edges each: the last lane of the per-state kernels' grid is the last state, one short of it,
    or alone in a new wavefront / block. c0 takes more than 32 values: its supports span several bitmap words. A stream longer
    than the row (the last state loops), one that stops inside it, and one with a late observation that fits no early state."""
    m = stcsp.Model(text=counter(n))
    e, r, post, host = solved(stcsp, m)
    info = e.generator("all", 0)
    assert info.n_states == n and info.n_edges == 2 * n
    rng = np.random.RandomState(n)
    c0 = m.var_names.index("c0")
    path = host.repair_streams([np.full((n + 2, m.n_vars), X, np.int32)], "all")[1][0]  # the least path; 2^(n + 2) of them overflow the generator
    path[:, m.var_names.index("x")] = np.random.RandomState(n).randint(0, 2, size=n + 2)  # x is free
    streams = blanked([path, path[:n - 1], path[:1], path[:40]], 0.3, n) + [np.full((40, m.n_vars), X, np.int32)]
    streams[3][39, c0] = 7  # c0 is 39 at step 39
    streams[4][35, c0] = 35
    dev = e.infer_streams(streams, draws=1, seed=n)
    assert same(dev, host.infer_streams(streams, "all", draws=1, seed=n))
    assert dev[0][3] == 0 and dev[0][4] == 2.0 ** 40 and dev[1][4][20][c0] == [20] and (dev[2][4] == 1).all()
    assert dev[0][0] > 0 and len(dev[2][0]) == n + 3


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_stream_counts(stcsp, n):
    m = stcsp.Model.from_name("juggling_b4_f5")
    e, r, post, host = solved(stcsp, m)
    e.generator(None, 6)
    streams = blanked(list(e.generate(n, 6, seed=n)[0]), 0.3, n)
    for kw in (dict(draws=0), dict(draws=3, seed=n)):
        dev = e.infer_streams(streams, **kw)
        assert len(dev[0]) == n and (dev[0] > 0).all() and same(dev, host.infer_streams(streams, **kw))


def test_lengths_0_1_7_33_in_one_call(stcsp):
    """Streams of different lengths share the launches of a level, backward (a stream takes part while r <= len) and forward
    (while t < len)."""
    m = stcsp.Model.from_name("juggling_b4_f5")
    e, r, post, host = solved(stcsp, m)
    e.generator(None, 33)
    lengths = (33, 0, 7, 1, 0, 33, 1, 7)
    streams = blanked([e.generate(1, L, seed=L + i)[0][0] for i, L in enumerate(lengths)], 0.3, 5)
    streams[5][20] += 1  # most likely no solution
    for kw in (dict(), dict(end_final=True, draws=1), dict(draws=3, seed=2)):
        dev = e.infer_streams(streams, **kw)
        assert e.infer_result.n_batches == 1
        assert same(dev, host.infer_streams(streams, **kw))
        assert [len(k) for k in dev[2]] == [L + 1 for L in lengths]


@pytest.mark.parametrize("segment", [None, "16", "100000"])
def test_out_degree_720(stcsp, monkeypatch, segment):
    """juggling_b6_f6_nosym: 720 edges leave the root: the wavefront-per-state road of k_i_forward_long by default, and with
    STCSP_REPAIR_WAVE_SEGMENT the same answers with more states on that road (16) and with none (100000)."""
    if segment:
        monkeypatch.setenv("STCSP_REPAIR_WAVE_SEGMENT", segment)
    m = stcsp.Model.from_name("juggling_b6_f6_nosym")
    e, r, post, host = solved(stcsp, m)
    info = e.generator(None, 8)
    assert info.max_out_degree == 720
    good = e.generate(6, 8, seed=1)[0]
    streams = blanked(list(good), 0.3, 2) + blanked(list(good), 0.7, 3) + [np.full((8, info.n_observable), X, np.int32)]
    dev = e.infer_streams(streams, draws=2, seed=1)
    assert (dev[0] > 0).all() and dev[0][-1] == info.count[8]
    assert all(v in sup for s, rows in zip(dev[1][:6], good) for row, sets in zip(rows.tolist(), s) for v, sup in zip(row, sets))
    assert same(dev, host.infer_streams(streams, draws=2, seed=1))


def test_out_degree_8192(stcsp):
    """WIDE: one live state, 8,192 loops, x variable 0 in [0,127] and y variable 1 in [0,63], every row a solution step. By
    arithmetic: an observed in-domain pair leaves 1 way, an unobserved x 128, an unobserved y 64, both 8,192, a value outside
    the domain none. x has 128 values: four bitmap words."""
    m = stcsp.Model(text=WIDE)
    assert m.var_names[:2] == ["x", "y"]
    e, r, post, host = solved(stcsp, m)
    info = e.generator("all", 0)
    assert (info.n_states, info.max_out_degree) == (1, 8192)
    s = np.array([[5, 7], [X, 63], [100, X], [X, X]], np.int32)
    count, supports, n_states, draws, fin = e.infer_streams([s, np.array([[X, 64]], np.int32)], draws=1, ranks=[[127 * 64 * 8192 + 9 * 8192 + 8191], [0]])
    assert e.infer_result.n_labels == 8192
    assert count.tolist() == [128.0 * 64 * 8192, 0.0] and n_states[0].tolist() == [1] * 5 and n_states[1].tolist() == [0, 0]
    full_x, full_y = list(range(128)), list(range(64))
    assert supports == [[[[5], [7]], [full_x, [63]], [[100], full_y], [full_x, full_y]], [[[], []]]]
    assert draws[0][0].tolist() == [[5, 7], [127, 63], [100, 9], [127, 63]]
    both = [s, s[:2]]
    assert same(e.infer_streams(both, draws=2, seed=5), host.infer_streams(both, "all", draws=2, seed=5))


def test_interval_domains_with_values_far_apart(stcsp, RefOracle):
    m = stcsp.Model(text=FAR_APART)
    e = stcsp.Engine(m, flags=stcsp.F_INTERVAL_DOMAINS)
    r = e.solve()
    post = e.postprocess()
    host = e.automaton(r).import_flags(post)
    check_device(stcsp, RefOracle, m, "far apart", masks=("default",), lengths=(5,), engine=(e, r, post, host))
    mask = [int(n in "xy") for n in m.var_names]
    e.generator(mask, 0)
    count, supports, _, _, _ = e.infer_streams([np.full((3, 2), X, np.int32)])
    assert count.tolist() == [8.0] and supports[0] == [[[0], [0, 1]], [[1000000], [0, 1]], [[0], [0, 1]]]


def test_batches(stcsp, monkeypatch):
    """STCSP_INFER_BYTES: 9 streams under a budget that holds four of the longest run in at least 3 batches and give what one
    batch gives; a budget below one stream's structures is STCSP_E_NOMEM."""
    m = stcsp.Model.from_name("juggling_b4_f5")
    e, r, post, host = solved(stcsp, m)
    info = e.generator(None, 12)
    good = e.generate(9, 12, seed=4)[0]
    streams = blanked([g[:12 - i % 3] for i, g in enumerate(good)], 0.3, 4)
    kw = dict(draws=2, seed=6)
    whole = e.infer_streams(streams, **kw)
    res = e.infer_result
    assert res.n_batches == 1 and same(whole, host.infer_streams(streams, **kw))
    e.infer_streams(streams[:1], **kw)
    one = e.infer_result.table_bytes  # the structures of one stream of 12 steps
    assert len(streams[0]) == 12 and one >= 13 * info.n_states * 9 + 12 * res.n_labels * 2
    monkeypatch.setenv("STCSP_INFER_BYTES", str(4 * one))
    cut = e.infer_streams(streams, **kw)
    assert e.infer_result.n_batches >= 3 and e.infer_result.table_bytes <= 4 * one
    assert same(cut, whole)
    monkeypatch.setenv("STCSP_INFER_BYTES", str(one))
    assert same(e.infer_streams(streams, **kw), whole) and e.infer_result.n_batches == 9
    monkeypatch.setenv("STCSP_INFER_BYTES", str(one - 4))
    with pytest.raises(stcsp.StcspError) as ex:
        e.infer_streams(streams, **kw)
    assert ex.value.code == -4
    monkeypatch.delenv("STCSP_INFER_BYTES")
    assert same(e.infer_streams(streams, **kw), whole)


def test_infer_follows_the_flags_of_a_second_postprocess_and_shares_the_labels(stcsp):
    """PRUNED_BY_ADVERSARY: before the adversarial pass d4 can be 0 or 1 at every step; after it the state with t == 1 and the
    edges into it are gone, so the support of d4 is {0}. In between: infer and repair interleaved on one generator build use one
    set of label ids, a monitor_build touches neither, and none of the other passes' answers change."""
    m = stcsp.Model(text=PRUNED_BY_ADVERSARY)
    e = stcsp.Engine(m)
    r = e.solve()
    post = e.postprocess()
    e.generator("all", 5)
    d4 = m.var_names.index("d4")
    blank = [np.full((5, m.n_vars), X, np.int32)]
    through = list(e.generate(8, 5, seed=2)[0])
    host = e.automaton(r).import_flags(post)
    first = e.infer_streams(blank + through, draws=1, seed=1)
    labels = e.infer_result.n_labels
    assert [sets[d4] for sets in first[1][0][:4]] == [[0, 1]] * 4 and same(first, host.infer_streams(blank + through, "all", draws=1, seed=1))
    rep = e.repair_streams(through)
    assert e.repair_result.n_labels == labels and (rep[0] == 0).all()
    e.monitor("all")
    mon = e.check_streams(through)
    gen = e.generate(16, 5, seed=9)
    again = e.infer_streams(blank + through, draws=1, seed=1)
    assert same(again, first)
    rep2 = e.repair_streams(through)
    assert np.array_equal(rep[0], rep2[0]) and all(np.array_equal(x, z) for x, z in zip(rep[1], rep2[1]))
    assert np.array_equal(gen[0], e.generate(16, 5, seed=9)[0]) and all(np.array_equal(x, z) for x, z in zip(mon[:3], e.check_streams(through)[:3]))
    post = e.postprocess(adversarial=5)
    with pytest.raises(stcsp.StcspError) as ex:  # the structures are invalidated
        e.infer_streams(blank)
    assert ex.value.code == -6
    e.generator("all", 0)
    host = e.automaton(r).import_flags(post)
    dev = e.infer_streams(blank + through, draws=1, seed=1)
    assert same(dev, host.infer_streams(blank + through, "all", draws=1, seed=1))
    assert [sets[d4] for sets in dev[1][0][:4]] == [[0]] * 4 and dev[0][0] < first[0][0]


def test_contract_errors(stcsp):
    m = stcsp.Model.from_name("juggling_b4_f5")
    e = stcsp.Engine(m)
    e.solve()
    e.postprocess()
    e.generator_info = None
    with pytest.raises(stcsp.StcspError) as ex:  # no generator_build: refused by the wrapper ...
        e.infer_streams([])
    assert ex.value.code == -6
    rq, out = stcsp.InferRequest(), stcsp.InferResult()
    assert e._f("infer")(e._h, rq, out) == -6  # ... and by the library
    info = e.generator(None, 3)
    n_obs = info.n_observable
    s = np.full((3, n_obs), X, np.int32)
    assert len(e.infer_streams([])[0]) == 0 and e.infer_result.n_batches == 0
    with pytest.raises(stcsp.StcspError) as ex:
        e.infer_streams([s], draws=-1)
    assert ex.value.code == -1
    count = int(info.count[3])
    assert e.infer_streams([s], draws=1, ranks=[[count - 1]])[0][0] == count
    with pytest.raises(stcsp.StcspError) as ex:
        e.infer_streams([s], draws=1, ranks=[[count]])
    assert ex.value.code == -1
    for offsets in ([1, 3], [0, 3, 2], [0, -1]):
        with pytest.raises(stcsp.StcspError) as ex:
            e.infer_streams((np.zeros(max(offsets[-1], 0) * n_obs, np.int32), offsets))
        assert ex.value.code == -1
    e.postprocess()  # a second postprocess invalidates the structures
    with pytest.raises(stcsp.StcspError) as ex:
        e.infer_streams([s])
    assert ex.value.code == -6
    sh = stcsp.Engine(m, flags=stcsp.F_STEPPED)  # the sharded pipeline
    sh.generator_info = info
    with pytest.raises(stcsp.StcspError) as ex:
        sh.infer_streams([s])
    assert ex.value.code == -2


def test_infinite_count_on_the_device(stcsp):
    """A free binary variable, 1,100 unobserved steps: the count is +inf, supports and |F_t| are still exact, draws refused."""
    m = stcsp.Model(text="var x:[0,1];")
    e, r, post, host = solved(stcsp, m)
    e.generator("all", 0)
    s = [np.full((1100, 1), X, np.int32)]
    dev = e.infer_streams(s)
    assert dev[0][0] == np.inf and dev[1][0] == [[[0, 1]]] * 1100 and (dev[2][0] == 1).all() and same(dev, host.infer_streams(s, "all"))
    with pytest.raises(stcsp.StcspError) as ex:
        e.infer_streams(s, draws=1)
    assert ex.value.code == -2


@pytest.mark.parametrize("name", ["digitinvader3", "partialorder_10"])
def test_consequences_on_the_device(stcsp, name):
    """The consequences of the contract against the device's own monitor, repair and generator."""
    m = stcsp.Model.from_name(name)
    e, r, post, host = solved(stcsp, m)
    L = 6
    for arg in (None, "all"):
        for end_final in (False, True):
            tag = f"{name} [{arg}] end_final={end_final}"
            info = e.generator(arg, L, end_final=end_final)
            n_obs = info.n_observable
            e.monitor(arg)
            good = list(e.generate(6, L, seed=1)[0]) if info.count[L] > 0 else []
            rng = np.random.RandomState(7)
            bad = [g.copy() for g in good]
            for b in bad:
                b[rng.randint(L), rng.randint(n_obs)] += 1
            streams = good + bad + blanked(good, 0.3, 8) + blanked(bad, 0.3, 9) + [np.full((L, n_obs), X, np.int32)]
            count, supports, n_states, draws, fin = e.infer_streams(streams, end_final=end_final, draws=2, seed=4)
            assert I.bits(count[-1]) == I.bits(info.count[L]), f"{tag}: all MISSING is the generator's count"
            dist, repaired, rfin, _ = e.repair_streams(streams, end_final=end_final)
            assert np.array_equal(count > 0, dist == 0), f"{tag}: count > 0 exactly when the repair's distance is 0"
            acc = e.check_streams(streams)[0]
            for i, s in enumerate(streams):
                if arg == "all" and not end_final and (s != X).all():
                    assert count[i] in (0.0, 1.0) and (count[i] == 1.0) == (acc[i] == L), f"{tag}: fully observed, stream {i}"
                if count[i] > 0:
                    assert all(((s == X) | (s == d)).all() for d in draws[i]), f"{tag}: a draw keeps the observed entries"
            ok = [d for i in range(len(streams)) if count[i] > 0 for d in draws[i]]
            assert (e.check_streams(ok)[0] == L).all(), f"{tag}: a draw is a prefix of a solution"
            zero = e.infer_streams(streams, end_final=end_final, draws=1, ranks=[[0]] * len(streams))
            for i in range(len(streams)):
                if count[i] > 0:
                    assert (zero[3][i][0].tolist(), int(zero[4][i][0])) == (repaired[i].tolist(), int(rfin[i])), f"{tag}: rank 0 is the repair"
            # specialisation, on the first streams with MISSING entries
            special, cases = [], []
            for i in [i for i, s in enumerate(streams) if (s == X).any() and count[i] > 0][:3]:
                for t, v in list(zip(*np.nonzero(streams[i] == X)))[:6]:
                    sup = supports[i][t][v]
                    others = sorted({x + d for x in sup for d in (-1, 1)} - set(sup))
                    for value in sup + others:
                        z = streams[i].copy()
                        z[t, v] = value
                        special.append(z)
                    cases.append((i, len(sup), len(others)))
            got, at = e.infer_streams(special, end_final=end_final)[0], 0
            for i, n_in, n_out in cases:
                inside, outside = got[at:at + n_in], got[at + n_in:at + n_in + n_out]
                at += n_in + n_out
                assert (inside > 0).all() and (outside == 0).all() and sum(int(c) for c in inside) == int(count[i]), f"{tag}: specialisation, stream {i}"


def test_cli_round_trip(stcsp, tmp_path):
    """--infer= prints what Engine.infer_streams() returns; its draws, fed to --check=, are accepted whole; a solution sampled by
    --sample=, with entries blanked, has feasible 1 and the original value in every support. --shards=2 (the host twin on the
    merged automaton) prints the same bytes."""
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    (tmp_path / "m.csp").write_text(stcsp.instances.by_name("juggling_b4_f5"))

    def run(*args):
        p = subprocess.run([str(exe), *args, "m.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert p.returncode == 0, p.stderr
        return p.stdout

    sampled = run("--sample=5:8:3").splitlines()
    rng = np.random.RandomState(3)
    rows = [line.split() for line in sampled[1:]]
    text = sampled[0] + "\n" + "".join(" ".join("?" if rng.rand() < 0.3 else v for v in row) + "\n" for row in rows)
    (tmp_path / "in.txt").write_text(text)
    outs = [run(*extra, "--infer=in.txt", "--infer-draws=2:5") for extra in ((), ("--shards=2",))]
    assert outs[0] == outs[1]
    lines = outs[0].splitlines()
    assert lines[0] == sampled[0]
    heads = [l.split() for l in lines if l.startswith("# ") and " count " in l]
    assert len(heads) == 5 and all(h[3] != "0" and h[5] == "8" and h[7] == "1" for h in heads)
    sets = [[set(tok[1:-1].split(",")) for tok in l.split()[1:]] for l in lines if l.startswith("# {")]
    steps = [row for row in rows if row]
    assert len(sets) == len(steps) == 40 and all(v in sup for row, sup_row in zip(steps, sets) for v, sup in zip(row, sup_row))
    (tmp_path / "out.txt").write_text(outs[0])
    checked = [l.split() for l in run("--check=out.txt").splitlines()]
    assert len(checked) == 10 and all(l[1] == l[2] == "8" for l in checked)
    m = stcsp.Model.from_name("juggling_b4_f5")
    e, r, post, host = solved(stcsp, m)
    e.generator(None, 0)
    names = [n for n, k in zip(m.var_names, Q.default_mask(m.var_names)) if k]
    assert sampled[0].split()[1:] == names
    streams = [np.array([[X if v == "?" else int(v) for v in l.split()] for l in block.splitlines()], np.int32) for block in text.split("\n", 1)[1].split("\n\n") if block]
    count, supports, _, draws, _ = e.infer_streams(streams, draws=2, seed=5)
    assert [h[3] for h in heads] == [f"{c:.0f}" for c in count]
    assert sets == [[{str(v) for v in sup} for sup in row] for s in supports for row in s]
    drawn = [[int(v) for v in l.split()] for l in lines if l and not l.startswith("#")]
    assert drawn == [row for d in draws for one in d for row in one.tolist()]
