"""Repairing observed streams on the device (stcsp_engine_repair, dev_repair.hpp) through the C ABI, against the host twin on
the same automaton and flags and against the independent yardstick of tests/repair_ref.py (plain Python over the automaton of
the CPU oracle). Run on the GPU box: pytest -m gpu.

Distance, repaired stream, end_final and n_changed depend on no state or edge number, so the device, the host twin and the
yardstick -- which runs on the ORACLE's automaton, numbered differently -- are compared directly, with ==."""
import subprocess

import numpy as np
import pytest

import monitor_ref as M
import quotient_ref as Q
import repair_ref as R
from test_generate_gpu import NO_LIVE_ROOT, PRUNED_BY_ADVERSARY, UNTIL, WIDE, WITNESS, solved
from test_quotient import COUNTDOWN, PROBES, SMALLEST_GOLDENS

pytestmark = pytest.mark.gpu

X = R.MISSING


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
    return (np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, z) for x, z in zip(a[1], b[1]))
            and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]))


def check_device(stcsp, RefOracle, m, what, masks=("default", "all"), oracle=True, lengths=(5, 12), seed=3):
    """Device == host twin on the same automaton == yardstick on the oracle's automaton, all four outputs, with and without
    weights, END_FINAL and MISSING entries; the device's own monitor accepts every repaired stream whole, and
    distance 0 <=> accepted_len == len."""
    e, r, post, host = solved(stcsp, m)
    o = RefOracle(m)
    ro = o.solve()
    flags = o.automaton(ro).traverse().flags()
    for name, mask in M.masks(m, r).items():
        if name not in masks:
            continue
        arg = None if name == "default" else mask
        n_obs = sum(mask)
        y = R.Yardstick(ro, *flags, mask)
        info = e.generator(arg, 0)  # the horizon does not limit the repair
        e.monitor(arg)
        streams = [s for L in lengths for s in R.make_streams(y, m.var_bounds(), seed + L, L)]
        rng = np.random.RandomState(seed)
        slow = info.n_edges > 2000  # the plain Python recurrence then takes a few streams only
        for kw in (dict(), dict(end_final=True), dict(weights=[int(w) for w in rng.randint(0, 5, size=n_obs)]),
                   dict(weights=[int(w) for w in rng.randint(1, 9, size=n_obs)], end_final=True)):
            dev = e.repair_streams(streams, **kw)
            # (without a live root nothing runs on the device: no batch, as for the inference)
            assert e.repair_result.n_batches == (1 if info.root_live else 0) and e.repair_result.n_observable == n_obs
            assert same(dev, host.repair_streams(streams, arg, **kw)), f"{what} [{name}] {kw}: device and host twin differ"
            if oracle:
                got = R.unpack(dev)
                for i in (range(len(streams)) if not slow else range(2, 5)):
                    assert got[i] == y.dp(streams[i], **kw), f"{what} [{name}] {kw} stream {i}: device and yardstick differ"
            ok = [v for d, v in zip(dev[0], dev[1]) if d >= 0]
            assert (e.check_streams(ok)[0] == [len(v) for v in ok]).all(), f"{what} [{name}] {kw}: a repaired stream is a prefix of a solution"
            if not kw and n_obs:
                acc, nend = e.check_streams(streams)[:2]
                for i, s in enumerate(streams):
                    if (s != X).all():  # (accepted in some state: without a live root the monitor "accepts" the empty stream in none)
                        assert (dev[0][i] == 0) == (acc[i] == len(s) and nend[i] > 0), f"{what} [{name}]: distance 0 exactly when the monitor accepts"
        print(f"{what} [{name}]: live {info.n_states} edges {info.n_edges} labels {e.repair_result.n_labels} streams {len(streams)}")


@pytest.mark.parametrize("which", ["COUNTER", "COUNTDOWN", "DUPLICATES"])
def test_device_on_witness_models(stcsp, RefOracle, which):
    check_device(stcsp, RefOracle, stcsp.Model(text=WITNESS[which]), which, masks=("default", "all", "hidden"))


@pytest.mark.parametrize("probe", ["until", "arr", "at", "misc", "adversarial"])
def test_device_on_probes(stcsp, RefOracle, probe):
    check_device(stcsp, RefOracle, stcsp.Model(text=PROBES[probe]["text"]), probe, masks=("default", "all", "hidden"))


@pytest.mark.parametrize("name", SMALLEST_GOLDENS + ["digitinvader3", "partialorder_10"])
def test_device_on_goldens(stcsp, RefOracle, name):
    check_device(stcsp, RefOracle, stcsp.Model.from_name(name), name, masks=("default", "all", "hidden"))


def test_hand_derived_on_the_device(stcsp):
    """tests/test_repair.py derives these by hand."""
    m = stcsp.Model(text=COUNTDOWN)
    e, r, post, host = solved(stcsp, m)
    e.generator([int(n == "x") for n in m.var_names], 0)
    s = [np.array([[v]] * 5, np.int32) for v in (0, 1, X)]
    dist, values, fin, nchg = e.repair_streams(s)
    assert dist.tolist() == [2, 0, 0] and nchg.tolist() == [2, 0, 0]
    assert [v[:, 0].tolist() for v in values] == [[0, 0, 0, 1, 1], [1] * 5, [0, 0, 0, 1, 1]]
    assert e.repair_streams(s, weights=[3])[0].tolist() == [6, 0, 0]
    m = stcsp.Model(text=UNTIL)
    e, r, post, host = solved(stcsp, m)
    e.generator([int(n in "xy") for n in m.var_names], 0)
    wait = np.array([[1, 0]] * 3, np.int32)
    dist, values, fin, nchg = e.repair_streams([wait, np.zeros((0, 2), np.int32)])
    assert (dist.tolist(), fin.tolist(), nchg.tolist()) == ([0, 0], [0, 0], [0, 0]) and np.array_equal(values[0], wait)
    dist, values, fin, nchg = e.repair_streams([wait, np.zeros((0, 2), np.int32)], end_final=True)
    assert (dist.tolist(), fin.tolist(), nchg.tolist()) == ([1, -1], [1, 0], [1, 0]) and values[0].tolist() == [[1, 0], [1, 0], [1, 1]]


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_live_state_counts_around_a_wavefront_and_a_block(stcsp, n):
    """n live states in a row, two edges each: the last lane of k_r_relax's grid is the last state, one short of it, or
    alone in a new wavefront / block. A stream longer than the row (the last state loops) and one that stops inside it."""
    m = stcsp.Model(text=counter(n))
    e, r, post, host = solved(stcsp, m)
    info = e.generator("all", 0)
    assert info.n_states == n and info.n_edges == 2 * n
    rng = np.random.RandomState(n)
    streams = [rng.randint(0, 3, size=(L, m.n_vars)).astype(np.int32) for L in (n + 2, n - 1, 1)]
    streams.append(np.full((7, m.n_vars), X, np.int32))
    dev = e.repair_streams(streams)
    assert same(dev, host.repair_streams(streams, "all"))
    e.generator("all", 7)
    assert dev[0][3] == 0 and np.array_equal(dev[1][3], e.generate(1, 7, ranks=[0])[0][0])  # unobserved: the least path


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_stream_counts(stcsp, n):
    m = stcsp.Model.from_name("juggling_b4_f5")
    e, r, post, host = solved(stcsp, m)
    info = e.generator(None, 0)
    rng = np.random.RandomState(n)
    lo, hi = zip(*[b for b, k in zip(m.var_bounds(), Q.default_mask(m.var_names)) if k])
    streams = [np.stack([rng.randint(lo[c], hi[c] + 1, size=6) for c in range(info.n_observable)], axis=1).astype(np.int32) for _ in range(n)]
    dev = e.repair_streams(streams)
    assert len(dev[0]) == n and same(dev, host.repair_streams(streams))


def test_lengths_0_1_7_33_in_one_call(stcsp):
    """Streams of different lengths share the launches of a level: stream b takes part while r <= len_b."""
    m = stcsp.Model.from_name("juggling_b4_f5")
    e, r, post, host = solved(stcsp, m)
    info = e.generator(None, 0)
    rng = np.random.RandomState(5)
    lo, hi = zip(*[b for b, k in zip(m.var_bounds(), Q.default_mask(m.var_names)) if k])
    streams = [np.stack([rng.randint(lo[c], hi[c] + 1, size=L) for c in range(info.n_observable)], axis=1).astype(np.int32).reshape(L, info.n_observable)
               for L in (33, 0, 7, 1, 0, 33, 1, 7)]
    for kw in (dict(), dict(end_final=True)):
        dev = e.repair_streams(streams, **kw)
        assert e.repair_result.n_batches == 1
        assert same(dev, host.repair_streams(streams, **kw))
        assert [len(v) for v in dev[1]] == [33, 0, 7, 1, 0, 33, 1, 7]


@pytest.mark.parametrize("segment", [None, "16", "100000"])
def test_out_degree_720(stcsp, monkeypatch, segment):
    """juggling_b6_f6_nosym: 720 edges leave the root: the wavefront-per-state road of k_r_relax_long by default, and with
    STCSP_REPAIR_WAVE_SEGMENT the same answers with more states on that road (16) and with none (100000)."""
    if segment:
        monkeypatch.setenv("STCSP_REPAIR_WAVE_SEGMENT", segment)
    m = stcsp.Model.from_name("juggling_b6_f6_nosym")
    e, r, post, host = solved(stcsp, m)
    info = e.generator(None, 8)
    assert info.max_out_degree == 720
    good = e.generate(6, 8, seed=1)[0]
    rng = np.random.RandomState(2)
    bad = good.copy()
    bad[rng.rand(*bad.shape) < 0.2] = 0
    part = bad.copy()
    part[rng.rand(*part.shape) < 0.3] = X
    streams = list(good) + list(bad) + list(part)
    dev = e.repair_streams(streams)
    assert (dev[0][:6] == 0).all() and all(np.array_equal(v, g) for v, g in zip(dev[1][:6], good))
    assert same(dev, host.repair_streams(streams))


def test_out_degree_8192(stcsp):
    """WIDE: one live state, 8,192 loops, x variable 0 in [0,127] and y variable 1 in [0,63], every row a solution step. By
    arithmetic: an in-domain row costs 0 and stays; x out of its domain costs 1 and becomes the least x, 0; both out cost 2
    and give (0, 0); an unobserved x is filled with 0."""
    m = stcsp.Model(text=WIDE)
    assert m.var_names[:2] == ["x", "y"]
    e, r, post, host = solved(stcsp, m)
    info = e.generator("all", 0)
    assert (info.n_states, info.max_out_degree) == (1, 8192)
    s = np.array([[5, 7], [127, 63], [500, 9], [-1, 64], [X, 33], [X, X], [3, 200]], np.int32)
    dist, values, fin, nchg = e.repair_streams([s], weights=[1, 1])
    assert e.repair_result.n_labels == 8192
    assert dist.tolist() == [4] and nchg.tolist() == [4]
    assert values[0].tolist() == [[5, 7], [127, 63], [0, 9], [0, 0], [0, 33], [0, 0], [3, 0]]
    assert e.repair_streams([s], weights=[10, 1])[0].tolist() == [10 + 11 + 1]
    assert same(e.repair_streams([s, s[:3]]), host.repair_streams([s, s[:3]], "all"))


def test_batches(stcsp, monkeypatch):
    """STCSP_REPAIR_BYTES: 9 streams under a budget that holds the tables and costs of four of the longest run in at least 3
    batches and give what one batch gives; a budget below one stream's table is STCSP_E_NOMEM."""
    m = stcsp.Model.from_name("juggling_b4_f5")
    e, r, post, host = solved(stcsp, m)
    info = e.generator(None, 12)
    good = e.generate(9, 12, seed=4)[0]
    rng = np.random.RandomState(4)
    bad = good.copy()
    bad[rng.rand(*bad.shape) < 0.1] = 1
    streams = [b[:12 - i % 3] for i, b in enumerate(bad)]
    whole = e.repair_streams(streams)
    res = e.repair_result
    assert res.n_batches == 1
    e.repair_streams(streams[:1])
    one = e.repair_result.table_bytes  # the table and costs of one stream of 12 steps
    assert len(streams[0]) == 12 and one >= (13 * info.n_states + 12 * res.n_labels) * 4
    monkeypatch.setenv("STCSP_REPAIR_BYTES", str(4 * one))
    cut = e.repair_streams(streams)
    assert e.repair_result.n_batches >= 3 and e.repair_result.table_bytes <= 4 * one
    assert same(cut, whole) and same(cut, host.repair_streams(streams))
    monkeypatch.setenv("STCSP_REPAIR_BYTES", str(one))
    assert same(e.repair_streams(streams), whole) and e.repair_result.n_batches == 9
    monkeypatch.setenv("STCSP_REPAIR_BYTES", str(one - 4))
    with pytest.raises(stcsp.StcspError) as ex:
        e.repair_streams(streams)
    assert ex.value.code == -4
    monkeypatch.delenv("STCSP_REPAIR_BYTES")
    assert same(e.repair_streams(streams), whole)


def test_no_live_root(stcsp):
    m = stcsp.Model(text=NO_LIVE_ROOT)
    e, r, post, host = solved(stcsp, m)
    e.generator("all", 0)
    streams = [np.array([[1, 0]] * 3, np.int32), np.zeros((0, m.n_vars), np.int32)]
    if m.n_vars != 2:
        streams = [np.zeros((3, m.n_vars), np.int32), np.zeros((0, m.n_vars), np.int32)]
    dist, values, fin, nchg = e.repair_streams(streams)
    assert dist.tolist() == [-1, -1] and not values[0].any() and fin.tolist() == [0, 0] and nchg.tolist() == [0, 0]


def test_repair_follows_the_flags_of_a_second_postprocess(stcsp):
    """PRUNED_BY_ADVERSARY: before the adversarial pass a step with d4 == 1 is a solution step; after it the state with t == 1
    and the edges into it are gone, so a stream with d4 == 1 is repaired onto d4 == 0: one change per such step."""
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
    before_gen, before_mon = e.generate(16, 5, seed=9), e.check_streams(through)
    dist = e.repair_streams(through)[0]
    assert (dist == 0).all()
    after_gen, after_mon = e.generate(16, 5, seed=9), e.check_streams(through)  # neither pass's structures were touched
    assert np.array_equal(before_gen[0], after_gen[0]) and all(np.array_equal(x, z) for x, z in zip(before_mon[:3], after_mon[:3]))
    post = e.postprocess(adversarial=5)
    with pytest.raises(stcsp.StcspError) as ex:  # the structures are invalidated
        e.repair_streams(through)
    assert ex.value.code == -6
    e.generator("all", 0)
    host = e.automaton(r).import_flags(post)
    dev = e.repair_streams(through)
    assert same(dev, host.repair_streams(through, "all"))
    assert (dev[0] > 0).all() and all((v[:, d4] == 0).all() for v in dev[1])


def test_contract_errors(stcsp):
    m = stcsp.Model.from_name("juggling_b4_f5")
    e = stcsp.Engine(m)
    e.solve()
    e.postprocess()
    e.generator_info = None
    with pytest.raises(stcsp.StcspError) as ex:  # no generator_build: refused by the wrapper ...
        e.repair_streams([])
    assert ex.value.code == -6
    rq, out = stcsp.RepairRequest(), stcsp.RepairResult()
    assert e._f("repair")(e._h, rq, out) == -6  # ... and by the library
    info = e.generator(None, 0)
    n_obs = info.n_observable
    s = np.zeros((3, n_obs), np.int32)
    assert len(e.repair_streams([])[0]) == 0 and e.repair_result.n_batches == 0
    with pytest.raises(stcsp.StcspError) as ex:
        e.repair_streams([s], weights=[1] * (n_obs - 1) + [-1])
    assert ex.value.code == -1
    big = (2 ** 31 - 2) // 3
    e.repair_streams([s], weights=[big] + [0] * (n_obs - 1))
    with pytest.raises(stcsp.StcspError) as ex:
        e.repair_streams([s], weights=[big] + [0] * (n_obs - 2) + [1])
    assert ex.value.code == -1
    for offsets in ([1, 3], [0, 3, 2], [0, -1]):
        with pytest.raises(stcsp.StcspError) as ex:
            e.repair_streams((np.zeros(max(offsets[-1], 0) * n_obs, np.int32), offsets))
        assert ex.value.code == -1
    e.postprocess()  # a second postprocess invalidates the structures
    with pytest.raises(stcsp.StcspError) as ex:
        e.repair_streams([s])
    assert ex.value.code == -6
    sh = stcsp.Engine(m, flags=stcsp.F_STEPPED)  # the sharded pipeline
    sh.generator_info = info
    with pytest.raises(stcsp.StcspError) as ex:
        sh.repair_streams([s])
    assert ex.value.code == -2


def test_cli_round_trip(stcsp, tmp_path):
    """--repair= prints what Engine.repair_streams() returns, in the format --check= reads: fed back, every stream is accepted
    whole. "?" is a value that was not observed. --shards=2 (the host twin on the merged automaton) prints the same bytes."""
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    m = stcsp.Model.from_name("juggling_b4_f5")
    (tmp_path / "m.csp").write_text(stcsp.instances.by_name("juggling_b4_f5"))
    e, r, post, host = solved(stcsp, m)
    info = e.generator(None, 10)
    good = e.generate(6, 10, seed=3)[0]
    rng = np.random.RandomState(3)
    bad = good.copy()
    bad[rng.rand(*bad.shape) < 0.1] = 0
    bad[rng.rand(*bad.shape) < 0.1] = X
    streams = list(bad) + [bad[0][:4]]
    names = [n for n, k in zip(m.var_names, Q.default_mask(m.var_names)) if k]
    text = "# " + " ".join(names) + "\n" + "".join("".join(" ".join("?" if x == X else str(x) for x in row) + "\n" for row in s) + "\n" for s in
                                                   [s.tolist() for s in streams])
    (tmp_path / "in.txt").write_text(text)
    dist, values, fin, nchg = e.repair_streams(streams)
    assert (dist >= 0).all()
    expect = "# " + " ".join(names) + "\n" + "".join(
        f"# {i} distance {dist[i]} len {len(v)} n_changed {nchg[i]} end_final {fin[i]}\n" + "".join(" ".join(str(x) for x in row) + "\n" for row in v.tolist()) + "\n"
        for i, v in enumerate(values))
    outs = []
    for extra in ((), ("--shards=2",)):
        p = subprocess.run([str(exe), *extra, "--repair=in.txt", "m.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert p.returncode == 0, p.stderr
        outs.append(p.stdout)
    assert outs[0] == expect and outs[1] == outs[0]
    (tmp_path / "out.txt").write_text(outs[0])
    p = subprocess.run([str(exe), "--check=out.txt", "m.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    lines = [l.split() for l in p.stdout.splitlines()]
    assert len(lines) == len(streams) and all(l[1] == l[2] for l in lines)
    (tmp_path / "c.csp").write_text(COUNTDOWN)
    (tmp_path / "c.txt").write_text("# x\n0\n0\n0\n0\n0\n\n?\n?\n?\n?\n?\n")
    p = subprocess.run([str(exe), "--repair=c.txt", "c.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    rows = "0\n0\n0\n1\n1\n\n"
    assert p.stdout == "# x\n# 0 distance 2 len 5 n_changed 2 end_final 1\n" + rows + "# 1 distance 0 len 5 n_changed 0 end_final 1\n" + rows
