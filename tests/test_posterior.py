"""Posterior marginals of unobserved stream entries, host side (include/stcsp_host.h: stcsp_automaton_posterior_streams): the
CPU twin of the device pass against an independent yardstick -- the plain Python of tests/posterior_ref.py, its recurrences
and its brute force over every path, run on the automaton of the CPU oracle. Masses are doubles multiplied and added in a
fixed order, marginals are integers; everything is compared with ==, the doubles by their bits. The device pass itself:
tests/test_posterior_gpu.py (which also holds STCSP_E_STATE without a generator: an engine needs a device)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import infer_ref as I
import monitor_ref as M
import posterior_ref as P
from test_generate import UNTIL, solved, text_of
from test_infer import WITNESS, longest_enumerable, only
from test_infer_gpu import counter
from test_quotient import COUNTDOWN, SMALLEST_GOLDENS

X = P.MISSING


def one(a, stream, observable, **kw):
    """(mass, exact, final_mass, marginals) of one stream as plain Python values."""
    n_obs = sum(observable)
    mass, exact, fmass, marg = a.posterior_streams([np.array(stream, dtype=np.int32).reshape(-1, n_obs)], observable, **kw)
    return float(mass[0]), int(exact[0]), fmass[0], marg[0]


def test_hand_derived_countdown(stcsp, RefOracle):
    """COUNTDOWN: c runs 0, 1, 2, 3, 3 and x must be 1 while c == 3, at steps 3 and 4; x is free before; the automaton is a
    chain and every state of it is final (there is no until). Under x alone, five unobserved steps: 2^3 = 8
    completions; a free step splits them 4 : 4, a forced one has all 8 on the value 1.
    Under the weight x: {1: 3} a free step weighs 1 + 3 = 4 and a forced one 3: mass 4^3 * 3 * 3 = 576; at a free step the value
    0 keeps 1/4 of it, 144, and the value 1 keeps 432; a forced step has all 576 on 1.
    With the second row observed as 1, unweighted: mass 4, that row {1: 4}, the other free rows {0: 2, 1: 2}."""
    m, o, r, a = solved(stcsp, RefOracle, COUNTDOWN)
    x = only(m, "x")
    assert one(a, [[X]] * 5, x) == (8.0, 1, 8, [[[(0, 4), (1, 4)]]] * 3 + [[[(1, 8)]]] * 2)
    assert one(a, [[X]] * 5, x, weights=[{1: 3}]) == (576.0, 1, 576, [[[(0, 144), (1, 432)]]] * 3 + [[[(1, 576)]]] * 2)
    free = [[(0, 2), (1, 2)]]
    assert one(a, [[X], [1], [X], [X], [X]], x) == (4.0, 1, 4, [free, [[(1, 4)]], free, [[(1, 4)]], [[(1, 4)]]])
    assert one(a, [[X], [X], [X], [0], [X]], x) == (0.0, 1, 0, [[[]]] * 5)  # x = 0 while c == 3: nothing is left


def test_hand_derived_until(stcsp, RefOracle):
    """UNTIL, x until y: the root waits for y and is not final; from it (x, y) = (1, 0) stays, (0, 1) and (1, 1) lead to the one
    final state, where all four rows are allowed. Two unobserved steps, both variables observable.
    Without END_FINAL there are 3 + 2 * 4 = 11 paths: (1,0) then one of 3 rows; (0,1) then one of 4; (1,1) then one of 4.
      step 0: x = 0 on the 4 paths through (0,1), x = 1 on 3 + 4 = 7; y = 0 on the 3 paths through (1,0), y = 1 on 8.
      step 1: out of the waiting root (1 path into it) the rows (1,0), (0,1), (1,1); out of the final state (2 paths into it)
      all four rows: x = 0 on 1 + 2 * 2 = 5, x = 1 on 2 + 2 * 2 = 6; y = 0 on 1 + 2 * 2 = 5, y = 1 on 2 + 2 * 2 = 6.
      Ten of the 11 end in the final state: final_mass 10.
    With END_FINAL the path (1,0), (1,0) falls away: mass 10 == final_mass.
      step 0: x = 0 on 4, x = 1 on 2 + 4 = 6; y = 0 on 2, y = 1 on 8.
      step 1: x = 0 on 1 + 4 = 5, x = 1 on 1 + 4 = 5; y = 0 on 0 + 4 = 4, y = 1 on 2 + 4 = 6.
    After an observed (1, 0) the run still waits: 3 ways on, two of them final; the observed entries carry the whole mass."""
    m, o, r, a = solved(stcsp, RefOracle, UNTIL)
    mask = only(m, "x", "y")
    assert [n for n, k in zip(m.var_names, mask) if k] == ["x", "y"]
    blank = [[X, X]] * 2
    assert one(a, blank, mask) == (11.0, 1, 10, [[[(0, 4), (1, 7)], [(0, 3), (1, 8)]], [[(0, 5), (1, 6)], [(0, 5), (1, 6)]]])
    assert one(a, blank, mask, end_final=True) == (10.0, 1, 10, [[[(0, 4), (1, 6)], [(0, 2), (1, 8)]], [[(0, 5), (1, 5)], [(0, 4), (1, 6)]]])
    assert one(a, [[1, 0], [X, X]], mask) == (3.0, 1, 2, [[[(1, 3)], [(0, 3)]], [[(0, 1), (1, 2)], [(0, 1), (1, 2)]]])
    assert one(a, [[1, 0], [X, X]], mask, end_final=True) == (2.0, 1, 2, [[[(1, 2)], [(0, 2)]], [[(0, 1), (1, 1)], [(1, 2)]]])
    assert one(a, [[0, 0], [X, X]], mask) == (0.0, 1, 0, [[[], []]] * 2)
    assert one(a, [], mask) == (1.0, 1, 0, [])                   # length 0: the empty path; the root is not final
    assert one(a, [], mask, end_final=True) == (0.0, 1, 0, [])


def weight_sets(bounds, keep):
    """None, a positive set and a set with a 0, over the values the variables can take: by the bounds alone. Three variables at
    the most are weighted, by 5 at the most: over 6 steps and 5,000 paths every mass stays far below 2^53."""
    lo = [max(bounds[v][0], -10 ** 6) for v in keep]
    hi = [min(bounds[v][1], 10 ** 6) for v in keep]
    positive = [{lo[c]: 2, hi[c]: 3} if c in (0, 2) else None for c in range(len(keep))]
    with_zero = [{lo[c]: 0, hi[c]: 5} if c == 0 else {min(lo[c] + 1, hi[c]): 2} if c == 1 else None for c in range(len(keep))]
    return {"unweighted": None, "positive": positive, "with a zero": with_zero}


def without_edges_that_carry(y, zeros):
    """The yardstick of the automaton without the edges that carry a value of weight 0; those weights are then not listed."""
    cut = P.Yardstick.__new__(P.Yardstick)
    cut.__dict__.update(y.__dict__)
    cut.out = {s: [(lab, d) for lab, d in edges if not any(lab[i] in zeros[c] for c, i in enumerate(y.keep))] for s, edges in y.out.items()}
    cut.weights = [{k: w for k, w in ws.items() if w} for ws in y.weights]
    return cut


def specialisation(a, arg, streams, got, weights, bounds, keep, what, end_final=False):
    """(d): replacing a MISSING entry by a value a gives a stream whose mass is m(t, v, a), any value outside the marginal gives
    0: one twin call over all the specialised streams of every MISSING entry."""
    special, want = [], []
    for i, s in enumerate(streams):
        if not got[i][1]:
            continue
        for t, v in zip(*np.nonzero(s == X)):
            marginal = dict(got[i][3][t][v])
            lo, hi = bounds[keep[v]]
            around = set(range(max(lo, -10 ** 6), min(hi, lo + 12) + 1)) | {x + d for x in marginal for d in (-1, 1)} | set(marginal)
            for value in sorted(around):
                z = s.copy()
                z[t, v] = value
                special.append(z)
                want.append(marginal.get(value, 0))
    if special:
        mass = a.posterior_streams(special, arg, end_final=end_final, weights=weights)[0]
        assert [float(w) for w in want] == mass.tolist(), f"{what}: the mass of a specialised stream is the marginal's"
    return len(special)


def check_twin(stcsp, RefOracle, text, what, mask_names=("default", "all", "hidden"), length=None, brute=True, seed=1, n=5):
    """Twin == the yardstick's recurrences == its brute force over every path (up to 5,000) on seeded streams at MISSING rates
    0, 30 % and 100 %, with and without END_FINAL, unweighted and under two weight sets, every output; and the consequences
    (a), (b), (c), (d), (e) and (g) of the contract."""
    m, o, r, a = solved(stcsp, RefOracle, text)
    valid, final, alive = a.flags()
    bounds = m.var_bounds()
    for name, mask in M.masks(m, r).items():
        if name not in mask_names:
            continue
        arg = None if name == "default" else mask
        n_obs = sum(mask)
        plain = I.Yardstick(r, valid, final, alive, mask)
        L = length or longest_enumerable(plain)
        streams = I.make_streams(plain, bounds, seed, L, n=n)
        paths = {0: plain.paths(0), L: plain.paths(L)} if brute else None
        for wname, weights in weight_sets(bounds, plain.keep).items():
            y = P.Yardstick(r, valid, final, alive, mask, weights)
            for end_final in (False, True):
                tag = f"{what} [{name}] {wname} end_final={end_final}"
                got = P.unpack(a.posterior_streams(streams, arg, end_final=end_final, weights=weights))
                for i, s in enumerate(streams):
                    want = P.expected(y, s, end_final)
                    assert got[i] == want, f"{tag} stream {s.tolist()}: twin {got[i]} yardstick {want}"
                    mass, exact, fmass, marg = y.dp(s, end_final)
                    if brute:
                        assert exact and y.brute(s, end_final, paths[len(s)]) == (int(mass), fmass, marg), f"{tag} stream {s.tolist()}: brute force"
                    if exact and mass > 0:
                        for t in range(len(s)):
                            for v in range(n_obs):
                                assert sum(k for _, k in marg[t][v]) == int(mass), f"{tag}: (a) the masses of a marginal sum to the mass"
                                if s[t][v] != X:
                                    assert marg[t][v] == [(int(s[t][v]), int(mass))], f"{tag}: (c) an observed entry"
                    if end_final:
                        assert fmass == (int(mass) if exact else 0), f"{tag}: with END_FINAL final_mass is the mass"
                if wname != "with a zero":  # (b), and by bits the count where every weight is 1
                    count, supports = a.infer_streams(streams, arg, end_final=end_final)[:2]
                    assert [[[[k for k, _ in cell] for cell in row] for row in g[3]] for g in got] == supports, f"{tag}: (b) infer's supports"
                    if weights is None:
                        assert [g[0] for g in got] == I.bits(count), f"{tag}: all weights 1: the mass is infer's count"
                        blank = a.posterior_streams([np.full((L, n_obs), X, np.int32)], arg, end_final=end_final)[0][0]
                        assert P.bits(blank) == P.bits(a.count_streams(L, end_final)[L]), f"{tag}: (g) all MISSING is the generator's count"
                else:  # (e)
                    zeros = [{k for k, w in (ws or {}).items() if w == 0} for ws in weights]
                    cut = without_edges_that_carry(y, zeros)
                    assert got == [P.expected(cut, s, end_final) for s in streams], f"{tag}: (e) a weight of 0 deletes the edges"
                if name == "default" and wname != "positive":
                    missing = [s for s in streams if (s == X).any()]
                    assert len(missing) >= 20 or n_obs == 0 or L == 0, f"{what}: {len(missing)} streams with MISSING entries"
                    specialisation(a, arg, streams, got, weights, bounds, plain.keep, tag, end_final)


@pytest.mark.parametrize("which", ["COUNTER", "COUNTDOWN", "DUPLICATES"])
def test_twin_on_witness_models(stcsp, RefOracle, which):
    check_twin(stcsp, RefOracle, WITNESS[which], which)


@pytest.mark.parametrize("probe", ["until", "arr", "at", "misc", "adversarial"])
def test_twin_on_probes(stcsp, RefOracle, probe):
    check_twin(stcsp, RefOracle, text_of(stcsp, "probe:" + probe), probe)


@pytest.mark.parametrize("name", SMALLEST_GOLDENS)
def test_twin_on_goldens(stcsp, RefOracle, name):
    check_twin(stcsp, RefOracle, text_of(stcsp, name), name)


@pytest.mark.parametrize("which", ["COUNTER", "DUPLICATES"])
def test_scaling_one_variable(stcsp, RefOracle, which):
    """(f): multiplying every weight of one variable by c multiplies mass and every marginal by c^len, while exact. x is 0 or 1;
    both values are listed, so that the factor reaches every edge."""
    m, o, r, a = solved(stcsp, RefOracle, WITNESS[which])
    mask = [1] * m.n_vars
    x = m.var_names.index("x")
    valid, final, alive = a.flags()
    y = I.Yardstick(r, valid, final, alive, mask)
    streams = I.make_streams(y, m.var_bounds(), 4, 5, n=3)
    base = [None] * m.n_vars
    for c, w in ((3, {0: 1, 1: 2}), (7, {0: 5, 1: 1})):
        base[x] = w
        scaled = list(base)
        scaled[x] = {k: c * v for k, v in w.items()}
        p, q = (P.unpack(a.posterior_streams(streams, mask, weights=ws)) for ws in (base, scaled))
        assert any(g[3] and g[3][0][0] for g in p)
        for s, (m0, e0, f0, g0), (m1, e1, f1, g1) in zip(streams, p, q):
            k = c ** len(s)
            assert e0 and e1
            assert np.uint64(m1).view(np.float64) == np.uint64(m0).view(np.float64) * k and f1 == f0 * k
            assert g1 == [[[(value, mass * k) for value, mass in cell] for cell in row] for row in g0]


def test_the_bound(stcsp, RefOracle):
    """counter(3): three live states in a row, the last one loops, x is free: two edges leave every state, so L rows of MISSING
    have 2^L completions. 52 rows: exact, mass 2^52, every marginal of x splits it in halves. 54 rows: 2^54 is a double but not
    below 2^53: exact 0, the mass is still given, the marginals are empty and final_mass is 0. The short stream between them in
    the same call is answered in full."""
    m, o, r, a = solved(stcsp, RefOracle, counter(3))
    mask = [1] * m.n_vars
    x = m.var_names.index("x")
    streams = [np.full((L, m.n_vars), X, np.int32) for L in (54, 3, 52)]
    mass, exact, fmass, marg = a.posterior_streams(streams, mask)
    assert mass.tolist() == [2.0 ** 54, 8.0, 2.0 ** 52] and exact.tolist() == [0, 1, 1] and fmass == [0, 8, 2 ** 52]
    assert marg[0] == [[[]] * m.n_vars] * 54
    assert [row[x] for row in marg[1]] == [[(0, 4), (1, 4)]] * 3 and [row[x] for row in marg[2]] == [[(0, 2 ** 51), (1, 2 ** 51)]] * 52
    valid, final, alive = a.flags()
    y = P.Yardstick(r, valid, final, alive, mask)
    assert P.unpack((mass, exact, fmass, marg)) == [P.expected(y, s) for s in streams]
    # 2^53 itself is not exact; one observed x brings it back below
    s = np.full((53, m.n_vars), X, np.int32)
    assert one(a, s, mask)[:3] == (2.0 ** 53, 0, 0)
    s[7, x] = 1
    assert one(a, s, mask)[:3] == (2.0 ** 52, 1, 2 ** 52)


def test_infinite_mass_from_weights(stcsp, RefOracle):
    """A free binary variable under weights of 2^31 - 1: 40 steps overflow a double. The mass is +inf, exact 0, and nothing is NaN;
    with a weight of 0 beside it the skipped terms never meet the infinity (0 * inf would be NaN). A short stream beside them is
    exact: its marginals are the powers of the weight."""
    m, o, r, a = solved(stcsp, RefOracle, "var x:[0,1];")
    big = 2 ** 31 - 1
    streams = [np.full((L, 1), X, np.int32) for L in (40, 1100, 1)]
    valid, final, alive = a.flags()
    for weights in ([{0: big, 1: big}], [{0: 0, 1: big}]):
        mass, exact, fmass, marg = a.posterior_streams(streams, "all", weights=weights)
        assert mass[0] == np.inf and mass[1] == np.inf and not np.isnan(mass).any()
        assert exact.tolist() == [0, 0, 1] and fmass[:2] == [0, 0] and marg[0] == [[[]]] * 40
        y = P.Yardstick(r, valid, final, alive, [1] * m.n_vars, weights)
        assert P.unpack((mass, exact, fmass, marg)) == [P.expected(y, s) for s in streams]
    assert marg[2] == [[[(1, big)]]] and mass[2] == float(big)


def test_invalid_requests(stcsp, RefOracle):
    m, o, r, a = solved(stcsp, RefOracle, COUNTDOWN)
    x = only(m, "x")
    s = np.full((5, 1), X, np.int32)
    assert one(a, s, x, weights=[[(0, 2), (1, 3)]])[0] == 5.0 ** 3 * 9
    for bad in ([[(1, 3), (0, 2)]], [[(1, 3), (1, 3)]], [[(0, -1)]], [[(0, 2), (1, -2 ** 31)]]):  # out of order, twice, negative
        with pytest.raises(stcsp.StcspError) as ex:
            a.posterior_streams([s], x, weights=bad)
        assert ex.value.code == -1
    for offsets in ([1, 3], [0, 3, 2], [0, -1]):  # not starting at 0, decreasing, negative
        with pytest.raises(stcsp.StcspError) as ex:
            a.posterior_streams((np.zeros(max(offsets[-1], 0), np.int32), offsets), x)
        assert ex.value.code == -1
    with pytest.raises(ValueError):
        a.posterior_streams([s], x, weights=[{0: 1}, {0: 1}])
    # the weights' own offsets, and arrays that are missing: through the library itself
    lib = stcsp.host_lib()
    mask = np.array(x, np.uint8)
    off = np.array([0, 5], np.int64)
    out = [np.zeros(1, t) for t in (np.float64, np.uint8, np.uint64)]
    moff = np.zeros(6, np.int64)

    def call(woff, wval, ww):
        mv, mm = C.c_void_p(), C.c_void_p()
        ptr = [None if z is None else z.ctypes.data for z in (woff, wval, ww)]
        rc = lib.stcsp_automaton_posterior_streams(a._h, mask.ctypes.data, 0, 1, off.ctypes.data, s.ctypes.data, *ptr, *[z.ctypes.data for z in out],
                                                   moff.ctypes.data, C.byref(mv), C.byref(mm))
        lib.stcsp_host_free(mv)
        lib.stcsp_host_free(mm)
        return rc

    val, w = np.array([0, 1], np.int32), np.array([2, 3], np.int32)
    assert call(np.array([0, 2], np.int64), val, w) == 0 and out[0][0] == 5.0 ** 3 * 9
    assert call(None, None, None) == 0 and out[0][0] == 8.0
    assert call(np.array([0, 0], np.int64), None, None) == 0 and out[0][0] == 8.0  # nothing listed
    for woff in ([1, 2], [0, -1], [2, 0]):
        assert call(np.array(woff, np.int64), val, w) == -1
    assert call(np.array([0, 2], np.int64), None, w) == -1 and call(np.array([0, 2], np.int64), val, None) == -1
    assert call(None, val, w) == -1


def test_cli_options(stcsp, tmp_path):
    """--posterior= needs a device for the solve; without one the option parsing is what can be checked here: --posterior excludes
    --check, --repair, --infer, --sample and --count. The round trip itself: tests/test_posterior_gpu.py."""
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    (tmp_path / "c.csp").write_text(COUNTDOWN)
    (tmp_path / "s.txt").write_text("# x\n0\n?\n\n")
    for other in ("--check=s.txt", "--repair=s.txt", "--infer=s.txt", "--sample=1:1", "--count=2"):
        p = subprocess.run([str(exe), "--posterior=s.txt", other, "c.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert p.returncode == 1 and "exclude each other" in p.stderr


def test_posterior_abi(stcsp):
    """The new symbols are exported and the new structs have the sizes of include/stcsp_engine.h (LP64)."""
    hip = C.CDLL(str(stcsp.CSRC / "libstcsp_hip.so"))
    assert hasattr(hip, "stcsp_engine_posterior")
    assert hasattr(stcsp.host_lib(), "stcsp_automaton_posterior_streams")
    assert C.sizeof(stcsp.PosteriorRequest) == 8 + 5 * 8 + 2 * 4
    assert C.sizeof(stcsp.PosteriorResult) == 8 + 7 * 8 + 2 * 8 + 2 * 4 + 5 * 8
    assert stcsp.POSTERIOR_MISSING == stcsp.INFER_MISSING == -2 ** 31 and stcsp.POSTERIOR_END_FINAL == 1
