"""Aligning observed streams, host side (include/stcsp_host.h: stcsp_automaton_align_streams): the CPU twin of the device
pass against an independent yardstick -- the plain Python of tests/align_ref.py: Dijkstra over the product graph for the
distance, the contract's recurrence and rules for rows and ops, and a brute force over every solution prefix with the
classical edit distance -- run on the automaton of the CPU oracle. Everything is integer arithmetic and compared with ==.
The device pass itself: tests/test_align_gpu.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import align_ref as A
import monitor_ref as Mo
import repair_ref as R
from align_ref import D, I, M
from test_generate import NO_LIVE_ROOT, UNTIL, solved, text_of
from test_quotient import COUNTDOWN, COUNTER, DUPLICATES, SMALLEST_GOLDENS
from test_repair import only

WITNESS = {"COUNTER": COUNTER, "COUNTDOWN": COUNTDOWN, "DUPLICATES": DUPLICATES}
X = A.MISSING
# skip:gap 1:1, 3:1, 1:3, and weights of 0 with indels of 2
COSTS = [dict(), dict(skip_cost=3, gap_cost=1), dict(skip_cost=1, gap_cost=3), dict(skip_cost=2, gap_cost=2, weights=0)]


def settings(kw, n_obs):
    kw = dict(kw)
    if "weights" in kw:
        kw["weights"] = [kw["weights"]] * n_obs
    return kw


def one(a, stream, observable, **kw):
    n_obs = sum(observable)
    return A.unpack(a.align_streams([np.array(stream, dtype=np.int32).reshape(-1, n_obs)], observable, **kw))[0]


def col(values):
    return [[v] for v in values]


def test_hand_derived_counter(stcsp, RefOracle):
    """COUNTER under c alone: c runs 0, 1, 2, 3, 3, ... and every state has one label. With weight 3 on c and indels of 1:
    0,1,3,3 has lost the step c == 2: the insert (1) beats the substitution (3). 0,1,1,2,3 has the step c == 1 twice: the
    first copy matches (rule 2 comes first), the second is skipped. With weight 1 and indels of 3 the wrong value in
    0,0,2,3 is substituted; with weight 5 and indels of 1 it is skipped and the step c == 1 inserted, D before I because rule
    3 comes before rule 4; with weight 2 and indels of 1 match, skip and insert all cost 2 there, and the match wins."""
    m, o, r, a = solved(stcsp, RefOracle, COUNTER)
    c = only(m, "c")
    assert one(a, col([0, 1, 3, 3]), c, weights=[3]) == (1, col([0, 1, 2, 3, 3]), [M, M, I, M, M], 0, 0, 1, 1)
    assert one(a, col([0, 1, 1, 2, 3]), c, weights=[3]) == (1, col([0, 1, 2, 3]), [M, M, D, M, M], 0, 1, 0, 1)
    assert one(a, col([0, 0, 2, 3]), c, skip_cost=3, gap_cost=3) == (1, col([0, 1, 2, 3]), [M, M, M, M], 1, 0, 0, 1)
    assert one(a, col([0, 0, 2, 3]), c, weights=[5]) == (2, col([0, 1, 2, 3]), [M, D, I, M, M], 0, 1, 1, 1)
    assert one(a, col([0, 0, 2, 3]), c, weights=[2]) == (2, col([0, 1, 2, 3]), [M, M, M, M], 1, 0, 0, 1)
    # MISSING entries match everything; the late 3 of 0,?,3 is dropped at the end (skip and insert tie at 1: rule 3 first)
    assert one(a, col([0, X, X, 3]), c, weights=[3]) == (0, col([0, 1, 2, 3]), [M, M, M, M], 0, 0, 0, 1)
    assert one(a, col([0, X, 3]), c, weights=[3]) == (1, col([0, 1]), [M, M, D], 0, 1, 0, 1)
    # the same stream when skipping is dear: the step c == 2 is inserted
    assert one(a, col([0, X, 3]), c, weights=[3], skip_cost=2) == (1, col([0, 1, 2, 3]), [M, M, I, M], 0, 0, 1, 1)


def test_hand_derived_countdown(stcsp, RefOracle):
    """COUNTDOWN under x alone: x must be 1 at steps 3 and 4 (c == 3) and is free before. 0,0,0,0,0: two substitutions
    cost 2 under 1:1, and so do two skips, two steps short; rule 2 comes first wherever a match attains the minimum."""
    m, o, r, a = solved(stcsp, RefOracle, COUNTDOWN)
    x = only(m, "x")
    assert one(a, col([1] * 5), x) == (0, col([1] * 5), [M] * 5, 0, 0, 0, 1)
    d, rows, ops, nchg, nskip, nins, fin = one(a, col([0] * 5), x, skip_cost=3, gap_cost=3)
    assert (d, rows, ops, nchg, nskip, nins) == (2, col([0, 0, 0, 1, 1]), [M] * 5, 2, 0, 0)
    # with a heavy x the two late samples are dropped instead: three matches, two skips
    assert one(a, col([0] * 5), x, weights=[5]) == (2, col([0, 0, 0]), [M, M, M, D, D], 0, 2, 0, 1)


def test_hand_derived_until(stcsp, RefOracle):
    """UNTIL, x until y: the root waits and is not final; (1,0) stays, (0,1) < (1,1) lead to the final state. With END_FINAL the
    empty stream is aligned with the shortest path to a final state: one insert of the least row; the waiting stream
    (1,0) x 3 matches whole (the match attains 1 at the last step as the insert after it does) and then inserts (0,1)."""
    m, o, r, a = solved(stcsp, RefOracle, UNTIL)
    mask = only(m, "x", "y")
    wait = [[1, 0]] * 3
    assert one(a, [], mask) == (0, [], [], 0, 0, 0, 0)
    assert one(a, [], mask, end_final=True, gap_cost=2) == (2, [[0, 1]], [I], 0, 0, 1, 1)
    assert one(a, wait, mask) == (0, wait, [M] * 3, 0, 0, 0, 0)
    assert one(a, wait, mask, end_final=True) == (1, wait + [[0, 1]], [M, M, M, I], 0, 0, 1, 1)
    assert one(a, wait, mask, end_final=True, gap_cost=2) == (1, [[1, 0], [1, 0], [1, 1]], [M, M, M], 1, 0, 0, 1)


def test_no_live_root(stcsp, RefOracle):
    m, o, r, a = solved(stcsp, RefOracle, NO_LIVE_ROOT)
    mask = only(m, "x", "y")
    assert one(a, [[1, 0]] * 3, mask) == A.NONE
    assert one(a, [], mask, end_final=True) == A.NONE


BRUTE_LIMIT = 1000  # solution prefixes the brute force enumerates per alignment (the contract of the tests allows up to 5,000)
# the four cost settings, END_FINAL with two of them
SETTINGS = [(COSTS[0], False), (COSTS[0], True), (COSTS[1], False), (COSTS[2], True), (COSTS[3], False)]


def brute_length(y, cap=5):
    """The longest stream whose prefixes of two more steps the brute force can enumerate."""
    return max([t for t in range(cap + 1) if y.n_prefixes(t + 2) <= BRUTE_LIMIT], default=0)


def fit_the_brute_force(y, a, arg, streams, kws):
    """Every stream cut at its end until, under every setting, the solution prefixes of up to len + distance / gap steps
    number at most BRUTE_LIMIT: the brute force then runs on every alignment, none is left out."""
    count = {}

    def prefixes(longest):
        if longest not in count:
            count[longest] = y.n_prefixes(longest)
        return count[longest]

    def fits(s):
        return all(prefixes(len(s) + max(int(a.align_streams([s], arg, **kw)[0][0]), 0) // kw.get("gap_cost", 1)) <= BRUTE_LIMIT for kw in kws)

    out = []
    for s in streams:
        while len(s) and not fits(s):
            s = s[:-1]
        out.append(s)
    return out


def seeded_streams(y, bounds, seed, L):
    """repair_ref's kinds of streams, and sampled prefixes with a step deleted and with a step duplicated."""
    streams = R.make_streams(y, bounds, seed, L)
    rng = np.random.RandomState(seed)
    for _ in range(3):
        w = y.sample_prefix(rng, L + 1)
        if len(w) >= 2:
            k = int(rng.randint(len(w)))
            streams.append(np.array(w[:k] + w[k + 1:], np.int32).reshape(-1, len(y.keep)))
            streams.append(np.array(w[:k + 1] + w[k:], np.int32).reshape(-1, len(y.keep)))
    return streams


def check_twin(stcsp, RefOracle, text, what, mask_names=("default", "all", "hidden")):
    """Twin == the yardstick's walk, its Dijkstra and its brute force on seeded streams, every output; and the
    consequences of the contract against the monitor's and the repair's host twins."""
    m, o, r, a = solved(stcsp, RefOracle, text)
    valid, final, alive = a.flags()
    for name, mask in Mo.masks(m, r).items():
        if name not in mask_names:
            continue
        arg = None if name == "default" else mask
        n_obs = sum(mask)
        y = A.Yardstick(r, valid, final, alive, mask)
        L = brute_length(y)
        kws = [dict(settings(costs, n_obs), end_final=end_final) for costs, end_final in SETTINGS]
        streams = fit_the_brute_force(y, a, arg, seeded_streams(y, m.var_bounds(), 1, L), kws)
        for kw in kws:
            got = A.unpack(a.align_streams(streams, arg, **kw))
            for s, g in zip(streams, got):
                where = f"{what} [{name}] {kw} stream {s.tolist()}"
                assert g == y.walk(s, **kw), f"{where}: twin and yardstick differ"
                assert g[0] == y.distance(s, **kw), f"{where}: Dijkstra over the product graph"
                if g[0] >= 0:
                    assert A.recomputed_cost(y, s, g, kw.get("weights"), kw.get("skip_cost", 1), kw.get("gap_cost", 1)) == g[0], where
                assert y.brute(s, g[0], limit=BRUTE_LIMIT, **kw) == g[0], f"{where}: brute force"  # (asserts the cap itself)
        for kw in kws[2:4]:  # beyond the brute force: four steps more, the recurrence and Dijkstra alone
            longer = seeded_streams(y, m.var_bounds(), 2, L + 4)
            for s, g in zip(longer, A.unpack(a.align_streams(longer, arg, **kw))):
                assert g == y.walk(s, **kw) and g[0] == y.distance(s, **kw), f"{what} [{name}] {kw} stream {s.tolist()}: twin and yardstick differ"
        # the consequences, under 1:1 and under weights
        dist, rows, ops, nchg, nskip, nins, fin = a.align_streams(streams, arg)
        ok = [v for d, v in zip(dist, rows) if d >= 0]
        assert (a.check_streams(ok, arg)[0] == [len(v) for v in ok]).all(), f"{what} [{name}]: an emitted prefix is a prefix of a solution"
        acc, nend = a.check_streams(streams, arg)[:2]
        rd, rv, rf, rc = a.repair_streams(streams, arg)
        for i, s in enumerate(streams):
            if (s != X).all() and n_obs:
                assert (dist[i] == 0) == (acc[i] == len(s) and nend[i] > 0), f"{what} [{name}]: distance 0 exactly when the monitor accepts"
            if rd[i] >= 0:  # indels dearer than the repair: the repair's answer, every op a match
                g = A.unpack(a.align_streams([s], arg, skip_cost=int(rd[i]) + 1, gap_cost=int(rd[i]) + 1))[0]
                assert g == (int(rd[i]), rv[i].tolist(), [M] * len(s), int(rc[i]), 0, 0, int(rf[i])), f"{what} [{name}]: the repair's answer"
        rng = np.random.RandomState(5)
        for _ in range(4):  # one step deleted: at most a gap; one duplicated: at most a skip
            w = y.sample_prefix(rng, L + 2)
            if len(w) >= 2:
                k = int(rng.randint(len(w)))
                cut, twice = np.array(w[:k] + w[k + 1:], np.int32).reshape(-1, n_obs), np.array(w[:k + 1] + w[k:], np.int32).reshape(-1, n_obs)
                d = a.align_streams([cut, twice], arg, skip_cost=2, gap_cost=3, weights=[4] * n_obs)[0]
                assert 0 <= d[0] <= 3 and 0 <= d[1] <= 2, f"{what} [{name}]: one deleted step, one duplicated step"


@pytest.mark.parametrize("which", ["COUNTER", "COUNTDOWN", "DUPLICATES"])
def test_twin_on_witness_models(stcsp, RefOracle, which):
    check_twin(stcsp, RefOracle, WITNESS[which], which)


@pytest.mark.parametrize("probe", ["until", "arr", "at", "misc", "adversarial"])
def test_twin_on_probes(stcsp, RefOracle, probe):
    check_twin(stcsp, RefOracle, text_of(stcsp, "probe:" + probe), probe)


@pytest.mark.parametrize("name", SMALLEST_GOLDENS)
def test_twin_on_goldens(stcsp, RefOracle, name):
    check_twin(stcsp, RefOracle, text_of(stcsp, name), name)


def test_end_final_of_the_empty_stream_is_a_shortest_path(stcsp, RefOracle):
    m, o, r, a = solved(stcsp, RefOracle, text_of(stcsp, "probe:until"))
    valid, final, alive = a.flags()
    mask = [1] * m.n_vars
    y = A.Yardstick(r, valid, final, alive, mask)
    level, steps = {0}, 0
    while not any(final[s] for s in level):  # breadth first: the edge distance from the root to a final state
        level = {d for s in level for _, d in y.out[s]}
        steps += 1
    g = one(a, [], mask, end_final=True, gap_cost=7)
    assert g[0] == 7 * steps and g[2] == [I] * steps and g[5] == steps and g[6] == 1
    assert a.check_streams([np.array(g[1], np.int32).reshape(-1, m.n_vars)], mask)[0][0] == steps


def test_invalid_requests(stcsp, RefOracle):
    m, o, r, a = solved(stcsp, RefOracle, COUNTDOWN)
    x = only(m, "x")
    s = np.zeros((3, 1), np.int32)
    n_states = stcsp.host_lib().stcsp_automaton_num_states(a._h)
    for kw in (dict(skip_cost=0), dict(gap_cost=0), dict(skip_cost=-1), dict(weights=[-1])):
        with pytest.raises(stcsp.StcspError) as ex:
            a.align_streams([s], x, **kw)
        assert ex.value.code == -1
    # max(sum of the weights, skip) x (longest stream) + gap x (states) may reach 2^31 - 2 and no more
    big = (2 ** 31 - 2 - n_states) // 3
    assert one(a, s, x, weights=[big])[0] >= 0 and one(a, s, x, skip_cost=big)[0] >= 0
    for kw in (dict(weights=[big + 1]), dict(skip_cost=big + 1), dict(gap_cost=(2 ** 31 - 2 - 3) // n_states + 1)):
        with pytest.raises(stcsp.StcspError) as ex:
            a.align_streams([s], x, **kw)
        assert ex.value.code == -1
    for offsets in ([1, 3], [0, 3, 2], [0, -1]):  # not starting at 0, decreasing, negative
        with pytest.raises(stcsp.StcspError) as ex:
            a.align_streams((np.zeros(max(offsets[-1], 0), np.int32), offsets), x)
        assert ex.value.code == -1


def test_cli_options(stcsp, tmp_path):
    """--align= needs a device for the solve; without one the option parsing is what can be checked here. The round trip into
    --check=: tests/test_align_gpu.py."""
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    (tmp_path / "c.csp").write_text(COUNTDOWN)
    (tmp_path / "s.txt").write_text("# x\n0\n?\n\n")
    for other in ("--check=s.txt", "--repair=s.txt", "--sample=1:1", "--count=2"):
        p = subprocess.run([str(exe), "--align=s.txt", other, "c.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert p.returncode == 1 and "exclude each other" in p.stderr
    for costs in ("0:1", "1:0", "1", "a:b"):
        p = subprocess.run([str(exe), "--align=s.txt", "--align-costs=" + costs, "c.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert p.returncode == 1 and "--align-costs" in p.stderr


def test_align_abi(stcsp):
    """The new symbols are exported and the new structs have the sizes of include/stcsp_engine.h (LP64)."""
    hip = C.CDLL(str(stcsp.CSRC / "libstcsp_hip.so"))
    assert hasattr(hip, "stcsp_engine_align")
    assert hasattr(stcsp.host_lib(), "stcsp_automaton_align_streams")
    assert C.sizeof(stcsp.AlignRequest) == 8 + 3 * 8 + 4 * 4
    assert C.sizeof(stcsp.AlignResult) == 8 + 9 * 8 + 2 * 8 + 4 * 4 + 4 * 8
    assert stcsp.ALIGN_END_FINAL == 1 and (stcsp.ALIGN_MATCH, stcsp.ALIGN_SKIP, stcsp.ALIGN_INSERT) == (0, 1, 2)
