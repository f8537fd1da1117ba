"""Aligning observed streams on the device (stcsp_engine_align, dev_align.hpp) through the C ABI, on both roads -- the fused
kernel, and with STCSP_ALIGN_FUSED=0 the launch per level and sweep -- against the host twin on the same automaton and flags
and against the independent yardstick of tests/align_ref.py (plain Python over the automaton of the CPU oracle). Run on the
GPU box: pytest -m gpu.

No output depends on a state or edge number, so the device, the host twin and the yardstick -- which runs on the ORACLE's
automaton, numbered differently -- are compared directly, with ==. Every model is solved once for the module."""
import subprocess

import numpy as np
import pytest

import align_ref as A
import monitor_ref as Mo
import quotient_ref as Q
from align_ref import D, I, M
from test_align import COSTS, seeded_streams, settings
from test_generate_gpu import NO_LIVE_ROOT, PRUNED_BY_ADVERSARY, UNTIL, WIDE, WITNESS
from test_quotient import COUNTDOWN, PROBES
from test_repair_gpu import counter
from test_services_fuzz import TEXT

pytestmark = pytest.mark.gpu

X = A.MISSING
FUSED, GENERAL = 1, 2
TABLE = "table:37:16x16:3:60:10:3"
_solved = {}


def solved(stcsp, key, model=None):
    """(model, engine, Result, PostResult, the host's automaton with the device's flags), solved once per module."""
    if key not in _solved:
        m = model() if model else stcsp.Model(text=key)
        e = stcsp.Engine(m)
        r = e.solve()
        post = e.postprocess()
        _solved[key] = (m, e, r, post, e.automaton(r).import_flags(post))
    return _solved[key]


def named(stcsp, name):
    return solved(stcsp, name, lambda: stcsp.Model.from_name(name))


@pytest.fixture(params=["fused", "general"])
def road(request, monkeypatch):
    """The road the call takes while the automaton fits the fused kernel: the default, and the general one forced."""
    if request.param == "general":
        monkeypatch.setenv("STCSP_ALIGN_FUSED", "0")
    return FUSED if request.param == "fused" else GENERAL


def row_at(n, k):
    """The values of c0, c1, ... of counter(n) in its state k: c0 counts to its top, then c1 does, and so on."""
    tops, left = [], n - 1
    while left > 0:
        tops.append(min(left, 127))
        left -= tops[-1]
    return [min(max(k - sum(tops[:i]), 0), t) for i, t in enumerate(tops)]


def counters_only(m):
    return [int(name[0] == "c" and name[1:].isdigit()) for name in m.var_names]


def random_rows(rng, m, mask, length):
    lo, hi = zip(*[b for b, k in zip(m.var_bounds(), mask) if k])
    return np.stack([rng.randint(lo[c], hi[c] + 1, size=length) for c in range(len(lo))], axis=1).astype(np.int32).reshape(length, len(lo))


def check_device(stcsp, RefOracle, case, what, road, masks=("default", "all"), lengths=(5, 12)):
    """Device == host twin on the same automaton == yardstick on the oracle's automaton, every output, under the four cost
    settings with and without END_FINAL; path_kernel; and the consequences against the device's own monitor and repair."""
    m, e, r, post, host = case
    o = RefOracle(m)
    ro = o.solve()
    flags = o.automaton(ro).traverse().flags()
    for name, mask in Mo.masks(m, r).items():
        if name not in masks:
            continue
        arg = None if name == "default" else mask
        n_obs = sum(mask)
        y = A.Yardstick(ro, *flags, mask)
        info = e.generator(arg, 0)  # the horizon does not limit the alignment
        e.monitor(arg)
        streams = [s for L in lengths for s in seeded_streams(y, m.var_bounds(), 3 + L, L)]
        few = range(len(streams)) if info.n_edges <= 2000 else range(2, 5)  # the plain Python then takes a few streams only
        for costs in COSTS:
            for end_final in (False, True):
                kw = dict(settings(costs, n_obs), end_final=end_final)
                dev = e.align_streams(streams, **kw)
                res = e.align_result
                assert res.path_kernel == (road if info.root_live else 0) and res.n_batches == (1 if info.root_live else 0)
                assert res.n_observable == n_obs
                assert A.same(dev, host.align_streams(streams, arg, **kw)), f"{what} [{name}] {kw}: device and host twin differ"
                got = A.unpack(dev)
                for i in few:
                    assert got[i] == y.walk(streams[i], **kw), f"{what} [{name}] {kw} stream {i}: device and yardstick differ"
                    assert got[i][0] == y.distance(streams[i], **kw), f"{what} [{name}] {kw} stream {i}: Dijkstra over the product graph"
                for s, g in zip(streams, got):
                    if g[0] >= 0:
                        assert A.recomputed_cost(y, s, g, kw.get("weights"), kw.get("skip_cost", 1), kw.get("gap_cost", 1)) == g[0]
                ok = [v for d, v in zip(dev[0], dev[1]) if d >= 0]
                assert (e.check_streams(ok)[0] == [len(v) for v in ok]).all(), f"{what} [{name}] {kw}: an emitted prefix is a prefix of a solution"
        dist = e.align_streams(streams)[0]
        acc, nend = e.check_streams(streams)[:2]
        rd, rv, rf, rc = e.repair_streams(streams)
        for i, s in enumerate(streams):
            if (s != X).all() and n_obs:
                assert (dist[i] == 0) == (acc[i] == len(s) and nend[i] > 0), f"{what} [{name}]: distance 0 exactly when the monitor accepts"
            if rd[i] >= 0:  # indels dearer than the repair: the repair's answer, every op a match
                g = A.unpack(e.align_streams([s], skip_cost=int(rd[i]) + 1, gap_cost=int(rd[i]) + 1))[0]
                assert g == (int(rd[i]), rv[i].tolist(), [M] * len(s), int(rc[i]), 0, 0, int(rf[i])), f"{what} [{name}]: the repair's answer"
        print(f"{what} [{name}]: live {info.n_states} edges {info.n_edges} labels {e.align_result.n_labels} streams {len(streams)}")


@pytest.mark.parametrize("which", ["COUNTER", "COUNTDOWN", "DUPLICATES"])
def test_device_on_witness_models(stcsp, RefOracle, road, which):
    check_device(stcsp, RefOracle, solved(stcsp, WITNESS[which]), which, road, masks=("default", "all", "hidden"))


@pytest.mark.parametrize("probe", ["until", "arr", "at", "misc", "adversarial"])
def test_device_on_probes(stcsp, RefOracle, road, probe):
    check_device(stcsp, RefOracle, solved(stcsp, PROBES[probe]["text"]), probe, road, masks=("default", "all", "hidden"))


@pytest.mark.parametrize("name", ["juggling_b4_f4", "digitinvader1"])
def test_device_on_goldens(stcsp, RefOracle, road, name):
    check_device(stcsp, RefOracle, named(stcsp, name), name, road, lengths=(6,))


@pytest.mark.parametrize("mask", ["default", "all", "hidden", "colour"])
def test_device_on_a_table_automaton(stcsp, RefOracle, road, monkeypatch, mask):
    """262 live states, three colours; the colour-only mask of tests/test_services_fuzz.py among the masks."""
    import observer_ref as OR
    plain = Mo.masks
    monkeypatch.setattr(Mo, "masks", lambda model, r: {**plain(model, r), "colour": OR.only(model, "c")})
    check_device(stcsp, RefOracle, solved(stcsp, TEXT[TABLE]), TABLE, road, masks=(mask,), lengths=(6,))


def test_hand_derived_on_the_device(stcsp, road):
    """tests/test_align.py derives these by hand."""
    m, e, r, post, host = solved(stcsp, WITNESS["COUNTER"])
    e.generator([int(n == "c") for n in m.var_names], 0)
    s = [np.array(v, np.int32).reshape(-1, 1) for v in ([0, 1, 3, 3], [0, 1, 1, 2, 3], [0, 0, 2, 3], [0, X, 3])]
    got = A.unpack(e.align_streams(s, weights=[3]))
    assert got[0] == (1, [[0], [1], [2], [3], [3]], [M, M, I, M, M], 0, 0, 1, 1)
    assert got[1] == (1, [[0], [1], [2], [3]], [M, M, D, M, M], 0, 1, 0, 1)
    assert got[3] == (1, [[0], [1]], [M, M, D], 0, 1, 0, 1)
    assert A.unpack(e.align_streams(s, weights=[5]))[2] == (2, [[0], [1], [2], [3]], [M, D, I, M, M], 0, 1, 1, 1)
    assert A.unpack(e.align_streams(s, weights=[2]))[2] == (2, [[0], [1], [2], [3]], [M, M, M, M], 1, 0, 0, 1)  # all three rules tie
    m, e, r, post, host = solved(stcsp, UNTIL)
    e.generator([int(n in "xy") for n in m.var_names], 0)
    wait = np.array([[1, 0]] * 3, np.int32)
    got = A.unpack(e.align_streams([wait, np.zeros((0, 2), np.int32)], end_final=True, gap_cost=2))
    assert got == [(1, [[1, 0], [1, 0], [1, 1]], [M, M, M], 1, 0, 0, 1), (2, [[0, 1]], [I], 0, 0, 1, 1)]
    assert A.unpack(e.align_streams([wait], end_final=True))[0] == (1, wait.tolist() + [[0, 1]], [M, M, M, I], 0, 0, 1, 1)
    assert e.align_result.path_kernel == road


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_live_state_counts_around_a_wavefront_and_a_block(stcsp, road, n):
    """n live states in a row, two edges each: the last lane of a row is the last state, one short of it, or alone in a new
    wavefront / block. Under the counters alone: random streams (every step a substitution or a skip), an unobserved one, and
    one that observes the row's last state at once: n - 1 inserts deep, through every state."""
    m, e, r, post, host = solved(stcsp, counter(n))
    mask = counters_only(m)
    info = e.generator(mask, 0)
    n_obs = info.n_observable
    assert info.n_states == n and info.n_edges == 2 * n and n_obs == len(row_at(n, 0))
    rng = np.random.RandomState(n)
    streams = [rng.randint(0, 3, size=(L, n_obs)).astype(np.int32) for L in (9, 1, 0)]
    streams.append(np.full((7, n_obs), X, np.int32))
    streams.append(np.array([row_at(n, n - 1)], np.int32))
    for kw in (dict(), dict(weights=[n] * n_obs, skip_cost=n)):
        dev = e.align_streams(streams, **kw)
        assert e.align_result.path_kernel == road
        assert A.same(dev, host.align_streams(streams, mask, **kw))
    assert dev[0][4] == n - 1 and dev[5][4] == n - 1 and dev[2][4].tolist() == [I] * (n - 1) + [M]
    assert dev[1][4].tolist() == [row_at(n, k) for k in range(n)]


def test_insert_runs(stcsp, road):
    """Closure depth past a wavefront and past a stride of the workgroup: a one-step stream that shows the counter k steps
    ahead, under the counters alone, with every weight and the skip dearer than k inserts. The answer is the row's first
    k + 1 states."""
    m, e, r, post, host = solved(stcsp, counter(310))
    mask = counters_only(m)
    runs = [1, 2, 63, 64, 65, 300]
    n_obs = e.generator(mask, 0).n_observable
    streams = [np.array([row_at(310, k)], np.int32) for k in runs]
    dev = e.align_streams(streams, weights=[301] * n_obs, skip_cost=301)
    assert e.align_result.path_kernel == road
    assert A.same(dev, host.align_streams(streams, mask, weights=[301] * n_obs, skip_cost=301))
    for i, k in enumerate(runs):
        assert dev[0][i] == k and dev[5][i] == k and dev[2][i].tolist() == [I] * k + [M]
        assert dev[1][i].tolist() == [row_at(310, j) for j in range(k + 1)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_stream_counts(stcsp, road, n):
    m, e, r, post, host = named(stcsp, "juggling_b4_f5")
    e.generator(None, 0)
    rng = np.random.RandomState(n)
    streams = [random_rows(rng, m, Q.default_mask(m.var_names), 6) for _ in range(n)]
    dev = e.align_streams(streams)
    assert len(dev[0]) == n and e.align_result.path_kernel == road and A.same(dev, host.align_streams(streams))


def test_lengths_0_1_7_33_in_one_call(stcsp, road):
    """Streams of different lengths share the launches of a level on the general road: stream b takes part while r <= len_b."""
    m, e, r, post, host = named(stcsp, "juggling_b4_f5")
    e.generator(None, 0)
    rng = np.random.RandomState(5)
    lengths = [33, 0, 7, 1, 0, 33, 1, 7]
    streams = [random_rows(rng, m, Q.default_mask(m.var_names), L) for L in lengths]
    for kw in (dict(), dict(end_final=True, skip_cost=2)):
        dev = e.align_streams(streams, **kw)
        assert e.align_result.n_batches == 1 and e.align_result.path_kernel == road
        assert A.same(dev, host.align_streams(streams, **kw))
        assert [int((o != I).sum()) for o in dev[2]] == lengths


def test_out_degree_720(stcsp, road):
    """juggling_b6_f6_nosym: 720 edges leave the root, the wavefront-per-state road of both roads. Solution prefixes as they
    are, with a step deleted, with a step duplicated, and with entries overwritten or not observed."""
    m, e, r, post, host = named(stcsp, "juggling_b6_f6_nosym")
    info = e.generator(None, 8)
    assert info.max_out_degree == 720
    good = e.generate(6, 8, seed=1)[0]
    rng = np.random.RandomState(2)
    bad = good.copy()
    bad[rng.rand(*bad.shape) < 0.2] = 0
    bad[rng.rand(*bad.shape) < 0.1] = X
    streams = list(good) + [np.delete(g, 3, axis=0) for g in good[:3]] + [np.insert(g, 2, g[2], axis=0) for g in good[:3]] + list(bad)
    for kw in (dict(), dict(weights=[5] * info.n_observable, skip_cost=2, gap_cost=3)):
        dev = e.align_streams(streams, **kw)
        assert e.align_result.path_kernel == road
        assert (dev[0][:6] == 0).all() and all(np.array_equal(v, g) for v, g in zip(dev[1][:6], good))
        assert (dev[0][6:9] <= kw.get("gap_cost", 1)).all() and (dev[0][9:12] <= kw.get("skip_cost", 1)).all()
        assert A.same(dev, host.align_streams(streams, **kw))


def test_out_degree_8192(stcsp, road):
    """WIDE: one live state, 8,192 loops, x in [0,127] and y in [0,63], every in-domain row a solution step. By arithmetic under
    weights (2, 2) and indels of 3: a row with one value out of its domain is substituted (2), one with both out is skipped
    (3 < 4)."""
    m, e, r, post, host = solved(stcsp, WIDE)
    info = e.generator("all", 0)
    assert (info.n_states, info.max_out_degree) == (1, 8192)
    s = np.array([[5, 7], [500, 9], [-1, 64], [X, 33], [3, 200]], np.int32)
    got = A.unpack(e.align_streams([s, s[:2]], weights=[2, 2], skip_cost=3, gap_cost=3))
    assert e.align_result.path_kernel == road
    assert got[0] == (2 + 3 + 0 + 2, [[5, 7], [0, 9], [0, 33], [3, 0]], [M, M, D, M, M], 2, 1, 0, 1)
    assert A.same(e.align_streams([s, s[:2]]), host.align_streams([s, s[:2]], "all"))


def test_batches(stcsp, road, monkeypatch):
    """STCSP_ALIGN_BYTES: 9 streams under a budget that holds the tables and costs of four of the longest run in at least 3
    batches and give what one batch gives; a budget below one stream's table is STCSP_E_NOMEM."""
    m, e, r, post, host = named(stcsp, "juggling_b4_f5")
    info = e.generator(None, 12)
    good = e.generate(9, 12, seed=4)[0]
    rng = np.random.RandomState(4)
    bad = good.copy()
    bad[rng.rand(*bad.shape) < 0.1] = 1
    streams = [b[:12 - i % 3] for i, b in enumerate(bad)]
    whole = e.align_streams(streams)
    res = e.align_result
    assert res.n_batches == 1
    e.align_streams(streams[:1])
    one = e.align_result.table_bytes  # the table and costs of one stream of 12 steps
    assert len(streams[0]) == 12 and one >= (13 * info.n_states + 12 * res.n_labels) * 4
    monkeypatch.setenv("STCSP_ALIGN_BYTES", str(4 * one))
    cut = e.align_streams(streams)
    assert e.align_result.n_batches >= 3 and e.align_result.table_bytes <= 4 * one and e.align_result.path_kernel == road
    assert A.same(cut, whole) and A.same(cut, host.align_streams(streams))
    monkeypatch.setenv("STCSP_ALIGN_BYTES", str(one))
    assert A.same(e.align_streams(streams), whole) and e.align_result.n_batches == 9
    monkeypatch.setenv("STCSP_ALIGN_BYTES", str(one - 4))
    with pytest.raises(stcsp.StcspError) as ex:
        e.align_streams(streams)
    assert ex.value.code == -4
    monkeypatch.delenv("STCSP_ALIGN_BYTES")
    assert A.same(e.align_streams(streams), whole)


def test_states_above_the_fused_capacity_take_the_general_road(stcsp):
    """digitinvader9, 30,031 states, is the smallest shipped instance above the 20,352 states two LDS rows hold: with nothing
    set in the environment the call takes the general road. Solution prefixes as they are, with a step deleted, with a step
    duplicated and with entries overwritten; the device against its twin."""
    m, e, r, post, host = named(stcsp, "digitinvader9")
    assert r.n_states > 20352
    info = e.generator(None, 6)
    good = e.generate(4, 6, seed=1)[0]
    rng = np.random.RandomState(9)
    noisy = good[3].copy()
    noisy[rng.rand(*noisy.shape) < 0.2] = 0
    streams = [good[0], np.delete(good[1], 2, axis=0), np.insert(good[2], 1, good[2][1], axis=0), noisy, good[0][:0]]
    for kw in (dict(), dict(weights=[4] * info.n_observable, skip_cost=2, gap_cost=3, end_final=True)):
        dev = e.align_streams(streams, **kw)
        assert e.align_result.path_kernel == GENERAL and e.align_result.n_batches == 1
        assert dev[0][0] == 0 and dev[0][1] <= kw.get("gap_cost", 1) and dev[0][2] <= kw.get("skip_cost", 1)
        assert A.same(dev, host.align_streams(streams, **kw))


def test_the_boundary_of_a_lowered_fused_capacity(stcsp, monkeypatch):
    """STCSP_ALIGN_FUSED_STATES lowers the capacity: 257 states against a capacity of 256 go the general road, against one
    of 257 the fused one; and only STCSP_ALIGN_FUSED=0 forces the general road."""
    m, e, r, post, host = solved(stcsp, counter(257))
    e.generator("all", 0)
    rng = np.random.RandomState(1)
    streams = [rng.randint(0, 3, size=(L, m.n_vars)).astype(np.int32) for L in (9, 3)]
    want = host.align_streams(streams, "all")
    for capacity, path in (("256", GENERAL), ("257", FUSED), ("0", GENERAL)):
        monkeypatch.setenv("STCSP_ALIGN_FUSED_STATES", capacity)
        assert A.same(e.align_streams(streams), want) and e.align_result.path_kernel == path
    monkeypatch.delenv("STCSP_ALIGN_FUSED_STATES")
    for value, path in (("yes", FUSED), ("1", FUSED), ("0", GENERAL)):
        monkeypatch.setenv("STCSP_ALIGN_FUSED", value)
        assert A.same(e.align_streams(streams), want) and e.align_result.path_kernel == path
    monkeypatch.delenv("STCSP_ALIGN_FUSED")
    assert A.same(e.align_streams(streams), want) and e.align_result.path_kernel == FUSED


def test_rows_above_64_kib_of_lds(stcsp, road):
    """partialorder_13: 16,128 states, two LDS rows of 126 KiB together: the fused launch raises the limit of dynamic shared
    memory. Solution prefixes with a step deleted, a step duplicated and entries overwritten."""
    m, e, r, post, host = named(stcsp, "partialorder_13")
    info = e.generator(None, 6)
    assert 8192 < r.n_states <= 20352
    good = e.generate(4, 6, seed=1)[0]
    rng = np.random.RandomState(13)
    noisy = good[3].copy()
    noisy[rng.rand(*noisy.shape) < 0.2] = 0
    streams = [good[0], np.delete(good[1], 2, axis=0), np.insert(good[2], 1, good[2][1], axis=0), noisy, good[0][:0]]
    for kw in (dict(), dict(weights=[4] * info.n_observable, skip_cost=2, gap_cost=3, end_final=True)):
        dev = e.align_streams(streams, **kw)
        assert e.align_result.path_kernel == road and dev[0][0] == 0 and dev[0][1] <= kw.get("gap_cost", 1) and dev[0][2] <= kw.get("skip_cost", 1)
        assert A.same(dev, host.align_streams(streams, **kw))


def test_no_live_root(stcsp, road):
    m, e, r, post, host = solved(stcsp, NO_LIVE_ROOT)
    e.generator("all", 0)
    streams = [np.zeros((3, m.n_vars), np.int32), np.zeros((0, m.n_vars), np.int32)]
    for kw in (dict(), dict(end_final=True)):
        got = A.unpack(e.align_streams(streams, **kw))
        assert got == [A.NONE, A.NONE] and e.align_result.path_kernel == 0
        assert got == A.unpack(host.align_streams(streams, "all", **kw))


def test_align_follows_the_flags_of_a_second_postprocess(stcsp, road):
    """PRUNED_BY_ADVERSARY: before the adversarial pass a step with d4 == 1 is a solution step; after it the state with t == 1
    and the edges into it are gone, so such a stream is no longer at distance 0. The call touches no other structure."""
    m = stcsp.Model(text=PRUNED_BY_ADVERSARY)
    e = stcsp.Engine(m)
    r = e.solve()
    e.postprocess()
    e.generator("all", 5)
    e.monitor("all")
    through = e.generate(64, 5, seed=2)[0]
    d4 = m.var_names.index("d4")
    through = [s for s in through if s[:4, d4].any()][:8]
    assert through
    before = e.generate(16, 5, seed=9), e.check_streams(through), e.repair_streams(through)
    assert (e.align_streams(through)[0] == 0).all()
    after = e.generate(16, 5, seed=9), e.check_streams(through), e.repair_streams(through)
    assert np.array_equal(before[0][0], after[0][0]) and all(np.array_equal(x, z) for x, z in zip(before[1][:3], after[1][:3]))
    assert np.array_equal(before[2][0], after[2][0])
    post = e.postprocess(adversarial=5)
    with pytest.raises(stcsp.StcspError) as ex:  # the structures are invalidated
        e.align_streams(through)
    assert ex.value.code == -6
    e.generator("all", 0)
    host = e.automaton(r).import_flags(post)
    dev = e.align_streams(through)
    assert A.same(dev, host.align_streams(through, "all")) and (dev[0] > 0).all() and e.align_result.path_kernel == road


def test_contract_errors(stcsp):
    m = stcsp.Model.from_name("juggling_b4_f5")
    e = stcsp.Engine(m)
    e.solve()
    e.postprocess()
    e.generator_info = None
    with pytest.raises(stcsp.StcspError) as ex:  # no generator_build: refused by the wrapper ...
        e.align_streams([])
    assert ex.value.code == -6
    rq, out = stcsp.AlignRequest(), stcsp.AlignResult()
    rq.skip_cost = rq.gap_cost = 1
    assert e._f("align")(e._h, rq, out) == -6  # ... and by the library
    info = e.generator(None, 0)
    n_obs = info.n_observable
    s = np.zeros((3, n_obs), np.int32)
    assert len(e.align_streams([])[0]) == 0 and e.align_result.n_batches == 0 and e.align_result.path_kernel == 0
    bad = [dict(weights=[1] * (n_obs - 1) + [-1]), dict(skip_cost=0), dict(gap_cost=0), dict(gap_cost=-3)]
    for kw in bad:
        with pytest.raises(stcsp.StcspError) as ex:
            e.align_streams([s], **kw)
        assert ex.value.code == -1
    big = (2 ** 31 - 2) // 3
    for kw in (dict(weights=[big + 1] + [0] * (n_obs - 1)), dict(skip_cost=big + 1), dict(gap_cost=2 ** 31 - 1)):
        with pytest.raises(stcsp.StcspError) as ex:  # over the bound whatever the number of states
            e.align_streams([s], **kw)
        assert ex.value.code == -1
    e.align_streams([s], weights=[big // 2] + [0] * (n_obs - 1), skip_cost=big // 2)
    for offsets in ([1, 3], [0, 3, 2], [0, -1]):
        with pytest.raises(stcsp.StcspError) as ex:
            e.align_streams((np.zeros(max(offsets[-1], 0) * n_obs, np.int32), offsets))
        assert ex.value.code == -1
    e.postprocess()  # a second postprocess invalidates the structures
    with pytest.raises(stcsp.StcspError) as ex:
        e.align_streams([s])
    assert ex.value.code == -6
    sh = stcsp.Engine(m, flags=stcsp.F_STEPPED)  # the sharded pipeline
    sh.generator_info = info
    with pytest.raises(stcsp.StcspError) as ex:
        sh.align_streams([s])
    assert ex.value.code == -2


def test_cli_round_trip(stcsp, tmp_path):
    """--align= prints what Engine.align_streams() returns, in the format --check= reads: fed back, every emitted prefix is
    accepted whole. --shards=2 (the host twin on the merged automaton) prints the same bytes."""
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    m, e, r, post, host = named(stcsp, "juggling_b4_f5")
    (tmp_path / "m.csp").write_text(stcsp.instances.by_name("juggling_b4_f5"))
    e.generator(None, 10)
    good = e.generate(6, 10, seed=3)[0]
    rng = np.random.RandomState(3)
    bad = good.copy()
    bad[rng.rand(*bad.shape) < 0.1] = X
    streams = [np.delete(bad[0], 4, axis=0), np.insert(bad[1], 3, bad[1][3], axis=0)] + list(bad[2:]) + [bad[0][:4]]
    names = [n for n, k in zip(m.var_names, Q.default_mask(m.var_names)) if k]
    text = "# " + " ".join(names) + "\n" + "".join("".join(" ".join("?" if x == X else str(x) for x in row) + "\n" for row in s) + "\n" for s in
                                                   [s.tolist() for s in streams])
    (tmp_path / "in.txt").write_text(text)
    dist, rows, ops, nchg, nskip, nins, fin = e.align_streams(streams, skip_cost=2, gap_cost=3)
    assert (dist >= 0).all() and nskip.sum() + nins.sum() > 0
    expect = "# " + " ".join(names) + "\n" + "".join(
        f"# {i} distance {dist[i]} len {len(streams[i])} out_len {len(v)} n_changed {nchg[i]} n_skipped {nskip[i]} n_inserted {nins[i]} "
        f"end_final {fin[i]} ops {''.join('MDI'[k] for k in ops[i])}\n" + "".join(" ".join(str(x) for x in row) + "\n" for row in v.tolist()) + "\n"
        for i, v in enumerate(rows))
    outs = []
    for extra in ((), ("--shards=2",)):
        p = subprocess.run([str(exe), *extra, "--align=in.txt", "--align-costs=2:3", "m.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert p.returncode == 0, p.stderr
        outs.append(p.stdout)
    assert outs[0] == expect and outs[1] == outs[0]
    (tmp_path / "out.txt").write_text(outs[0])
    p = subprocess.run([str(exe), "--check=out.txt", "m.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    lines = [l.split() for l in p.stdout.splitlines()]
    assert len(lines) == len(streams) and all(l[1] == l[2] for l in lines)
    (tmp_path / "u.csp").write_text(UNTIL)
    (tmp_path / "u.txt").write_text("# x y\n1 0\n1 0\n1 0\n\n")
    p = subprocess.run([str(exe), "--align=u.txt", "--align-final", "u.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    assert p.stdout == "# x y\n# 0 distance 1 len 3 out_len 4 n_changed 0 n_skipped 0 n_inserted 1 end_final 1 ops MMMI\n1 0\n1 0\n1 0\n0 1\n\n"
