"""Posterior marginals of unobserved stream entries on the device (stcsp_engine_posterior, dev_posterior.hpp) through the C ABI,
against the host twin on the same automaton and flags and against the independent yardstick of tests/posterior_ref.py (plain
Python over the automaton of the CPU oracle). Run on the GPU box: pytest -m gpu.

Masses, exact, final_mass and the marginals depend on no state or edge number, so the device, the host twin and the yardstick
-- which runs on the ORACLE's automaton, numbered differently -- are compared directly, with ==, the doubles by their bits.
The shapes are the smallest at which the kernels can go wrong: see each test."""
import subprocess

import numpy as np
import pytest

import infer_ref as I
import monitor_ref as M
import posterior_ref as P
import quotient_ref as Q
from test_generate_gpu import PRUNED_BY_ADVERSARY, UNTIL, WITNESS, solved
from test_infer_gpu import FAR_APART, blanked, counter
from test_quotient import COUNTDOWN

pytestmark = pytest.mark.gpu

X = P.MISSING
BIG = 2 ** 31 - 1


def oracle_yardstick(RefOracle, m, mask, weights=None):
    o = RefOracle(m)
    ro = o.solve()
    return P.Yardstick(ro, *o.automaton(ro).traverse().flags(), mask, weights)


def check(e, host, streams, arg, y=None, few=None, end_final=False, weights=None):
    """Device == host twin on every output of every stream, and == the yardstick `y` (built under the same weights) on the
    streams `few` (None: all). Returns the device's answer, unpacked."""
    dev = P.unpack(e.posterior_streams(streams, end_final=end_final, weights=weights))
    twin = P.unpack(host.posterior_streams(streams, arg, end_final=end_final, weights=weights))
    assert dev == twin, "device and host twin differ: " + str([i for i, (a, b) in enumerate(zip(dev, twin)) if a != b])
    res = e.posterior_result
    assert [bool(f) for f in np.ctypeslib.as_array(res.feasible, shape=(len(streams),))] == [np.uint64(d[0]).view(np.float64) > 0 for d in dev]
    if y is not None:
        for i in (range(len(streams)) if few is None else few):
            want = P.expected(y, streams[i], end_final)
            assert dev[i] == want, f"stream {i}: device {dev[i]} yardstick {want}"
    return dev


def first_weights(n_obs, streams):
    """A positive weight set and one with a 0 and a 2^31 - 1, on values the first variable takes in the streams."""
    seen = sorted({int(s[t, 0]) for s in streams for t in range(len(s)) if s[t, 0] != X})
    a, b = seen[0], seen[-1]
    rest = [None] * (n_obs - 1)
    return [{a: 2, b: 3}] + rest, [{a: 0, b: BIG} if a != b else {a: BIG}] + rest


def test_hand_derived_on_the_device(stcsp):
    """tests/test_posterior.py derives these by hand."""
    m = stcsp.Model(text=COUNTDOWN)
    e, r, post, host = solved(stcsp, m)
    e.generator([int(n == "x") for n in m.var_names], 0)
    s = [np.array(rows, np.int32).reshape(5, 1) for rows in ([X] * 5, [X, 1, X, X, X], [X, X, X, 0, X])]
    mass, exact, fmass, marg = e.posterior_streams(s)
    free, forced = [[(0, 2), (1, 2)]], [[(1, 4)]]
    assert (mass.tolist(), exact.tolist(), fmass) == ([8.0, 4.0, 0.0], [1, 1, 1], [8, 4, 0])
    assert marg == [[[[(0, 4), (1, 4)]]] * 3 + [[[(1, 8)]]] * 2, [free, forced, free, forced, forced], [[[]]] * 5]
    mass, exact, fmass, marg = e.posterior_streams(s[:1], weights=[{1: 3}])
    assert (mass.tolist(), fmass, marg[0]) == ([576.0], [576], [[[(0, 144), (1, 432)]]] * 3 + [[[(1, 576)]]] * 2)
    res = e.posterior_result
    e.infer_streams(s)
    assert (res.n_batches, res.n_observable, res.n_labels) == (1, 1, e.infer_result.n_labels)
    m = stcsp.Model(text=UNTIL)
    e, r, post, host = solved(stcsp, m)
    e.generator([int(n in "xy") for n in m.var_names], 0)
    s = [np.array([[X, X]] * 2, np.int32), np.array([[1, 0], [X, X]], np.int32), np.zeros((0, 2), np.int32)]
    mass, exact, fmass, marg = e.posterior_streams(s)
    assert (mass.tolist(), fmass) == ([11.0, 3.0, 1.0], [10, 2, 0])
    assert marg == [[[[(0, 4), (1, 7)], [(0, 3), (1, 8)]], [[(0, 5), (1, 6)], [(0, 5), (1, 6)]]], [[[(1, 3)], [(0, 3)]], [[(0, 1), (1, 2)], [(0, 1), (1, 2)]]], []]
    mass, exact, fmass, marg = e.posterior_streams(s, end_final=True)
    assert (mass.tolist(), fmass) == ([10.0, 2.0, 0.0], [10, 2, 0])
    assert marg == [[[[(0, 4), (1, 6)], [(0, 2), (1, 8)]], [[(0, 5), (1, 5)], [(0, 4), (1, 6)]]], [[[(1, 2)], [(0, 2)]], [[(0, 1), (1, 1)], [(1, 2)]]], []]


@pytest.mark.parametrize("which", ["COUNTER", "COUNTDOWN", "DUPLICATES"])
def test_device_on_witness_models(stcsp, RefOracle, which):
    """Every mask, with and without END_FINAL, unweighted and under both weight sets, every stream against the yardstick."""
    m = stcsp.Model(text=WITNESS[which])
    e, r, post, host = solved(stcsp, m)
    for name, mask in M.masks(m, r).items():
        arg = None if name == "default" else mask
        e.generator(arg, 0)
        plain = oracle_yardstick(RefOracle, m, mask)
        streams = [s for L in (4, 9) for s in I.make_streams(plain, m.var_bounds(), 3 + L, L, n=2)]
        for weights in (None,) + (first_weights(sum(mask), streams) if sum(mask) else ()):
            y = oracle_yardstick(RefOracle, m, mask, weights)
            for end_final in (False, True):
                check(e, host, streams, arg, y, end_final=end_final, weights=weights)


@pytest.mark.parametrize("n", [63, 65, 257, 1025])
def test_live_state_counts_around_a_wavefront_a_block_and_a_grid_row(stcsp, RefOracle, n):
    """n live states in a row, two edges each: the last lane of the per-state kernels' grid is the last state of a wavefront, alone
    in a new wavefront, alone in a new block of 256, alone in a fifth block. c0 takes more than 32 values (up to 128): its bins
    span what were several bitmap words in infer. A stream longer than the row (the last state loops; from 257 states on its
    mass is beyond 2^53: an inexact stream among exact ones), one that stops inside it, one of one step, 30 unobserved rows
    (2^30, and 3^30 < 2^53 under the weights), a late observation that fits no early state, and a walk down the whole row with
    five unobserved x: an exact mass whose forward sweep reaches the last state."""
    m = stcsp.Model(text=counter(n))
    e, r, post, host = solved(stcsp, m)
    info = e.generator("all", 0)
    assert info.n_states == n and info.n_edges == 2 * n
    c0, x = m.var_names.index("c0"), m.var_names.index("x")
    path = host.repair_streams([np.full((n + 2, m.n_vars), X, np.int32)], "all")[1][0]
    path[:, x] = np.random.RandomState(n).randint(0, 2, size=n + 2)  # x is free
    streams = blanked([path, path[:n - 1], path[:1], path[:40]], 0.3, n) + [np.full((30, m.n_vars), X, np.int32), np.full((40, m.n_vars), X, np.int32)]
    streams[3][39, c0] = 7  # c0 is 39 at step 39
    streams[5][35, c0] = 35
    walk = path.copy()  # the whole row of states under an exact mass: five x unobserved, every counter unobserved now and then
    walk[np.random.RandomState(n + 1).random_sample(walk.shape) < 0.3] = X
    walk[:, x] = 0  # (an observed value has its weight too: 0 weighs 1)
    walk[[0, n // 3, n // 2, n - 1, n + 1], x] = X
    streams.append(walk)
    weights = [None] * m.n_vars
    weights[x] = {0: 1, 1: 2}
    mask = [1] * m.n_vars
    for ws in (None, weights):
        y = oracle_yardstick(RefOracle, m, mask, ws)
        dev = check(e, host, streams, "all", y, few=(2, 3, 4, 5) + ((1, 6) if n <= 257 else ()), weights=ws)
        assert dev[3][0] == 0 and dev[5][1] == (ws is None) and dev[6][1] and dev[6][2] > 0
        assert dev[6][3][n][x] == [(0, 32 if ws is None else 3 ** 5)] and dev[6][0] == P.bits(32.0 if ws is None else 243.0)
        assert dev[4][:3] == (P.bits(2.0 ** 30 if ws is None else 3.0 ** 30), 1, 2 ** 30 if ws is None else 3 ** 30)
        assert dev[5][3][20][c0] == ([(20, 2 ** 40)] if ws is None else []) and len(dev[4][3][7][c0]) == 1


def test_unweighted_backward_is_infers_backward_on_the_device(stcsp):
    """The two instantiations of k_i_backward on one generator build: without weights every label weighs 1.0, so the weighted
    sweep must leave the bits of the unweighted one's counts, and the values of non-zero mass are infer's supports. The row of
    65 states is two wavefronts of lanes; streams of 0, 1 and 7 steps, which stay among the first states, and one of 70 steps,
    whose count at the root comes through state 64, the one lane of the second wavefront, where it loops. About 30 % of the
    entries are unobserved; x is free, so every count is a power of two far below 2^53."""
    m = stcsp.Model(text=counter(65))
    e, r, post, host = solved(stcsp, m)
    e.generator("all", 0)
    path = host.repair_streams([np.full((70, m.n_vars), X, np.int32)], "all")[1][0]
    streams = blanked([path[:0], path[:1], path[:7], path], 0.3, 65)
    mass, exact, fmass, marginals = e.posterior_streams(streams, weights=None)
    count, supports = e.infer_streams(streams)[:2]
    assert mass.view(np.uint64).tolist() == count.view(np.uint64).tolist()
    assert exact.tolist() == [1, 1, 1, 1] and (mass > 0).all()
    for i in range(len(streams)):
        assert [[[value for value, _ in pairs] for pairs in step] for step in marginals[i]] == supports[i]


@pytest.mark.parametrize("n", [1, 257])
def test_stream_counts(stcsp, n):
    """1 stream, and 257: blockIdx.y of every per-(state, stream) kernel, a second block of k_p_root."""
    m = stcsp.Model.from_name("juggling_b4_f5")
    e, r, post, host = solved(stcsp, m)
    info = e.generator(None, 6)
    streams = blanked(list(e.generate(n, 6, seed=n)[0]), 0.3, n)
    for ws in (None,) + first_weights(info.n_observable, streams):
        dev = check(e, host, streams, None, weights=ws)
        assert len(dev) == n and (ws is not None or all(d[0] > 0 and d[1] for d in dev))


def test_lengths_0_1_7_33_in_one_call(stcsp):
    """Streams of different lengths share the launches of a level; the rolling rows of A alternate, and a stream that has ended
    (after 0, 1 or 7 levels, in row 0 or 1) keeps its A_len for final_mass while the others go on."""
    m = stcsp.Model.from_name("juggling_b4_f5")
    e, r, post, host = solved(stcsp, m)
    info = e.generator(None, 33)
    lengths = (33, 0, 7, 1, 0, 33, 1, 7, 2)
    streams = blanked([e.generate(1, L, seed=L + i)[0][0] for i, L in enumerate(lengths)], 0.3, 5)
    streams[5][20] += 1  # most likely no solution
    for ws in (None, first_weights(info.n_observable, streams)[0]):
        for end_final in (False, True):
            dev = check(e, host, streams, None, end_final=end_final, weights=ws)
            assert e.posterior_result.n_batches == 1 and [len(d[3]) for d in dev] == list(lengths)


@pytest.mark.parametrize("segment", ["16", None, "100000"])
def test_out_degree_720(stcsp, monkeypatch, segment):
    """juggling_b6_f6_nosym: 720 edges leave the root, many of them into one destination and onto one label under the default mask:
    the atomics' worst case. The wavefront-per-state road of k_p_forward_long by default (128), with more states on it (16) and
    with none (100000): each equals the host twin, hence the three agree."""
    if segment:
        monkeypatch.setenv("STCSP_REPAIR_WAVE_SEGMENT", segment)
    m = stcsp.Model.from_name("juggling_b6_f6_nosym")
    e, r, post, host = solved(stcsp, m)
    info = e.generator(None, 8)
    assert info.max_out_degree == 720
    good = e.generate(6, 8, seed=1)[0]
    streams = blanked(list(good), 0.3, 2) + blanked(list(good), 0.7, 3) + [np.full((8, info.n_observable), X, np.int32)]
    for ws in (None,) + first_weights(info.n_observable, streams):
        dev = check(e, host, streams, None, weights=ws)
        if ws is None:
            assert all(d[1] and d[0] > 0 for d in dev) and dev[-1][0] == P.bits(info.count[8])
            assert all(sum(k for _, k in cell) == int(np.uint64(d[0]).view(np.float64)) for d in dev for row in d[3] for cell in row)


def test_interval_domains_with_values_far_apart(stcsp, RefOracle):
    """The dictionary of x has 2 entries a million apart, not ub - lb + 1 bins."""
    m = stcsp.Model(text=FAR_APART)
    e = stcsp.Engine(m, flags=stcsp.F_INTERVAL_DOMAINS)
    r = e.solve()
    post = e.postprocess()
    host = e.automaton(r).import_flags(post)
    mask = [int(n in "xy") for n in m.var_names]
    e.generator(mask, 0)
    streams = [np.full((3, 2), X, np.int32), np.array([[X, 1], [1000000, X]], np.int32), np.array([[1000000, X]], np.int32)]
    for ws in (None, [{1000000: 3}, {0: 0}], [{0: BIG, 1000000: 2}, None]):
        dev = check(e, host, streams, mask, oracle_yardstick(RefOracle, m, mask, ws), weights=ws)
    assert e.posterior_streams(streams[:1])[3][0] == [[[(0, 8)], [(0, 4), (1, 4)]], [[(1000000, 8)], [(0, 4), (1, 4)]], [[(0, 8)], [(0, 4), (1, 4)]]]


def test_batches(stcsp, monkeypatch):
    """STCSP_POSTERIOR_BYTES: 9 streams under a budget that holds four of the longest run in at least 3 batches and give what one
    batch gives; one stream per batch likewise; a budget below one stream's structures is STCSP_E_NOMEM."""
    m = stcsp.Model.from_name("juggling_b4_f5")
    e, r, post, host = solved(stcsp, m)
    info = e.generator(None, 12)
    good = e.generate(9, 12, seed=4)[0]
    streams = blanked([g[:12 - i % 3] for i, g in enumerate(good)], 0.3, 4)
    ws = first_weights(info.n_observable, streams)[0]
    whole = check(e, host, streams, None, weights=ws)
    res = e.posterior_result
    assert res.n_batches == 1
    e.posterior_streams(streams[:1], weights=ws)
    one = e.posterior_result.table_bytes  # the structures of one stream of 12 steps
    assert len(streams[0]) == 12 and one >= (13 + 2) * info.n_states * 8 + 12 * res.n_labels * 9
    monkeypatch.setenv("STCSP_POSTERIOR_BYTES", str(4 * one))
    cut = P.unpack(e.posterior_streams(streams, weights=ws))
    assert e.posterior_result.n_batches >= 3 and e.posterior_result.table_bytes <= 4 * one and cut == whole
    monkeypatch.setenv("STCSP_POSTERIOR_BYTES", str(one))
    assert P.unpack(e.posterior_streams(streams, weights=ws)) == whole and e.posterior_result.n_batches == 9
    monkeypatch.setenv("STCSP_POSTERIOR_BYTES", str(one - 4))
    with pytest.raises(stcsp.StcspError) as ex:
        e.posterior_streams(streams, weights=ws)
    assert ex.value.code == -4
    monkeypatch.delenv("STCSP_POSTERIOR_BYTES")
    assert P.unpack(e.posterior_streams(streams, weights=ws)) == whole


def test_the_bound_and_weights_of_0_and_of_2_to_the_31_minus_1(stcsp, RefOracle):
    """A free binary variable: L unobserved rows have 2^L completions. 54 rows (not exact: the mass alone), 3 rows and 52 rows
    (exact, halves of 2^52) in one batch. Under {0: 0, 1: 2^31 - 1}: one step alone is exact, 40 steps overflow a double, and no NaN
    arises from the skipped terms; under {0: 2^31 - 1, 1: 2^31 - 1} likewise."""
    m = stcsp.Model(text="var x:[0,1];")
    e, r, post, host = solved(stcsp, m)
    e.generator("all", 0)
    streams = [np.full((L, 1), X, np.int32) for L in (54, 3, 52, 1, 40, 1100)]
    dev = check(e, host, streams, "all", oracle_yardstick(RefOracle, m, [1]))
    assert [d[:3] for d in dev[:3]] == [(P.bits(2.0 ** 54), 0, 0), (P.bits(8.0), 1, 8), (P.bits(2.0 ** 52), 1, 2 ** 52)]
    assert dev[0][3] == [[[]]] * 54 and dev[2][3] == [[[(0, 2 ** 51), (1, 2 ** 51)]]] * 52 and dev[5][0] == P.bits(np.inf)
    for ws in ([{0: 0, 1: BIG}], [{0: BIG, 1: BIG}]):
        dev = check(e, host, streams, "all", oracle_yardstick(RefOracle, m, [1], ws), weights=ws)
        mass = np.array([d[0] for d in dev], np.uint64).view(np.float64)
        assert not np.isnan(mass).any() and mass[4] == np.inf and mass[5] == np.inf and [d[1] for d in dev] == [0, 0, 0, 1, 0, 0]
    assert dev[3][3] == [[[(0, BIG), (1, BIG)]]]


def test_posterior_follows_a_second_postprocess_and_leaves_infer_and_repair_alone(stcsp):
    """PRUNED_BY_ADVERSARY: before the adversarial pass d4 can be 0 or 1 at every step; after it the state with t == 1 and the
    edges into it are gone, so the marginal of d4 is {0: mass}. In between: posterior, infer and repair interleaved on one
    generator build use one set of label ids and dictionaries, and infer's and repair's outputs are what they were."""
    m = stcsp.Model(text=PRUNED_BY_ADVERSARY)
    e = stcsp.Engine(m)
    r = e.solve()
    post = e.postprocess()
    e.generator("all", 5)
    d4 = m.var_names.index("d4")
    blank = [np.full((5, m.n_vars), X, np.int32)]
    through = list(e.generate(8, 5, seed=2)[0])
    host = e.automaton(r).import_flags(post)
    streams = blank + blanked(through, 0.3, 1)
    first = check(e, host, streams, "all")  # posterior first: it builds the labels and the dictionaries
    labels = e.posterior_result.n_labels
    assert [[k for k, _ in row[d4]] for row in first[0][3][:4]] == [[0, 1]] * 4
    inf = e.infer_streams(streams, draws=1, seed=1)
    assert e.infer_result.n_labels == labels and I.unpack(inf) == I.unpack(host.infer_streams(streams, "all", draws=1, seed=1))
    rep = e.repair_streams(through)
    assert e.repair_result.n_labels == labels and (rep[0] == 0).all()
    ws = [None] * m.n_vars
    ws[d4] = {0: 2, 1: 5}
    check(e, host, streams, "all", weights=ws)
    assert I.unpack(e.infer_streams(streams, draws=1, seed=1)) == I.unpack(inf)
    rep2 = e.repair_streams(through)
    assert np.array_equal(rep[0], rep2[0]) and all(np.array_equal(a, b) for a, b in zip(rep[1], rep2[1]))
    assert check(e, host, streams, "all") == first
    # (b) against the device's own infer
    assert [[[[k for k, _ in cell] for cell in row] for row in d[3]] for d in first] == inf[1] and [d[0] for d in first] == I.bits(inf[0])
    post = e.postprocess(adversarial=5)
    with pytest.raises(stcsp.StcspError) as ex:  # the structures are invalidated
        e.posterior_streams(blank)
    assert ex.value.code == -6
    e.generator("all", 0)
    host = e.automaton(r).import_flags(post)
    dev = check(e, host, streams, "all")
    mass = int(np.uint64(dev[0][0]).view(np.float64))
    assert [row[d4] for row in dev[0][3][:4]] == [[(0, mass)]] * 4 and dev[0][0] < first[0][0]


def test_contract_errors(stcsp):
    m = stcsp.Model.from_name("juggling_b4_f5")
    e = stcsp.Engine(m)
    e.solve()
    e.postprocess()
    e.generator_info = None
    with pytest.raises(stcsp.StcspError) as ex:  # no generator_build: refused by the wrapper ...
        e.posterior_streams([])
    assert ex.value.code == -6
    rq, out = stcsp.PosteriorRequest(), stcsp.PosteriorResult()
    assert e._f("posterior")(e._h, rq, out) == -6  # ... and by the library: STCSP_E_STATE
    info = e.generator(None, 3)
    n_obs = info.n_observable
    s = np.full((3, n_obs), X, np.int32)
    assert len(e.posterior_streams([])[0]) == 0 and e.posterior_result.n_batches == 0
    assert e.posterior_streams([s])[0][0] == info.count[3]  # (g)
    rest = [None] * (n_obs - 1)
    for bad in ([[(1, 3), (0, 2)]], [[(1, 3), (1, 3)]], [[(0, -1)]]):
        with pytest.raises(stcsp.StcspError) as ex:
            e.posterior_streams([s], weights=bad + rest)
        assert ex.value.code == -1
    for offsets in ([1, 3], [0, 3, 2], [0, -1]):
        with pytest.raises(stcsp.StcspError) as ex:
            e.posterior_streams((np.zeros(max(offsets[-1], 0) * n_obs, np.int32), offsets))
        assert ex.value.code == -1
    e.postprocess()  # a second postprocess invalidates the structures
    with pytest.raises(stcsp.StcspError) as ex:
        e.posterior_streams([s])
    assert ex.value.code == -6
    sh = stcsp.Engine(m, flags=stcsp.F_STEPPED)  # the sharded pipeline
    sh.generator_info = info
    with pytest.raises(stcsp.StcspError) as ex:
        sh.posterior_streams([s])
    assert ex.value.code == -2


def test_cli_round_trip(stcsp, tmp_path):
    """--posterior= prints what Engine.posterior_streams() returns, weights included; --shards=2 (the host twin on the merged
    automaton) prints the same bytes."""
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
    m = stcsp.Model.from_name("juggling_b4_f5")
    e, r, post, host = solved(stcsp, m)
    info = e.generator(None, 0)
    names = [n for n, k in zip(m.var_names, Q.default_mask(m.var_names)) if k]
    assert sampled[0].split()[1:] == names
    streams = [np.array([[X if v == "?" else int(v) for v in l.split()] for l in block.splitlines()], np.int32) for block in text.split("\n", 1)[1].split("\n\n") if block]
    ws = first_weights(info.n_observable, streams)[0]
    option = "--posterior-weights=" + ",".join(f"{names[0]}={value}:{weight}" for value, weight in sorted(ws[0].items()))
    for extra, weights in (((), None), ((option,), ws), (("--posterior-final",), None)):
        outs = [run(*shards, *extra, "--posterior=in.txt") for shards in ((), ("--shards=2",))]
        assert outs[0] == outs[1]
        lines = outs[0].splitlines()
        assert lines[0] == sampled[0]
        heads = [l.split() for l in lines if l.startswith("# ") and " mass " in l]
        mass, exact, fmass, marg = e.posterior_streams(streams, end_final=extra == ("--posterior-final",), weights=weights)
        assert [h[1:] for h in heads] == [[str(i), "mass", f"{c:.0f}", "len", "8", "exact", str(x), "final_mass", str(f)]
                                          for i, (c, x, f) in enumerate(zip(mass, exact, fmass))]
        cells = [l.split()[1:] for l in lines if l.startswith("# {")]
        assert cells == [["{" + ",".join(f"{a}:{k}" for a, k in cell) + "}" for cell in row] for g in marg for row in g]
