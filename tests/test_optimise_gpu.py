"""Optimal solution streams on the device (stcsp_engine_optimise, dev_optimise.hpp) through the C ABI: device == host twin on
the engine's own automaton, array by array; == the yardstick of tests/optimise_ref.py on that automaton and == the twin on the
CPU oracle's automaton wherever the oracle runs in seconds. Run on the GPU box: pytest -m gpu."""
import ctypes as C
import functools
import re
import subprocess

import numpy as np
import pytest

import components_ref as CR
import quotient_ref as Q
from test_components import oracle_case, text_of
from test_optimise import big_weights, check_finite, check_mean, rows_of, small_weights
from test_wide_gpu import WIDE

pytestmark = pytest.mark.gpu

# a and b are free: every state has 100 live out-edges, more than a wavefront of k_opt_walk takes in one stride
FANOUT = "var a:[0,9]; var b:[0,9]; var t:[0,1]; first t == 0; next t == 1 - t;"
# s flips, and the aux variables of `/` and `%` under next have the whole int range (interval domains)
INT_RANGE = "var w:[-2,-1]; var s:[0,1]; var z:[0,4]; first s == 0; next s == 1 - s; z == next ((-2147483648 / w) % 5); w == s - 2;"
LOCAL = {"FANOUT": FANOUT, "neg_w4": WIDE["neg_w4"], "INT_RANGE": INT_RANGE}


@functools.lru_cache(maxsize=None)
def device_case(stcsp, name, interval=False):
    """(model, engine, Result, (valid, final, alive), the host's automaton with the device's flags): solved and post-processed once."""
    m = stcsp.Model(text=LOCAL[name] if name in LOCAL else text_of(stcsp, name))
    e = stcsp.Engine(m, flags=stcsp.F_INTERVAL_DOMAINS if interval else 0)
    r = e.solve()
    assert not r.truncated
    post = e.postprocess()
    flags = Q.post_flags(post)
    return m, e, r, flags, e.automaton(r).import_flags(post)


@functools.lru_cache(maxsize=None)
def engine_ref(stcsp, name, interval=False):
    m, e, r, flags, a = device_case(stcsp, name, interval)
    return CR.yardstick(r, *flags)


def same(x, y):
    """Two results of the implementations (device, host twin) on the same automaton: equal array by array."""
    keys = ("n_states", "n_components", "n_vars", "horizon", "largest_cyclic", "omega_component", "omega_mean", "comp_mean")
    if any(x[k] != y[k] for k in keys) or not np.array_equal(x["best"], y["best"]):
        return False
    for k in ("state_best", "state_component"):
        if (x[k] is None) != (y[k] is None) or (x[k] is not None and not np.array_equal(x[k], y[k])):
            return False
    return len(x["witnesses"]) == len(y["witnesses"]) and all(
        p[0] == q[0] and np.array_equal(p[1], q[1]) and np.array_equal(p[2], q[2]) for p, q in zip(x["witnesses"], y["witnesses"]))


def check_device(stcsp, name, w, interval=False, RefOracle=None, prefix_k=2):
    """Device == twin for every flag, == the yardstick on the engine's automaton; with RefOracle also == the oracle's automaton."""
    m, e, r, (valid, final, alive), a = device_case(stcsp, name, interval)
    ref = engine_ref(stcsp, name, interval)
    for maximise in (False, True):
        for end_final in (False, True):
            for kw in (dict(horizon=0), dict(horizon=1, lengths=[1, 0]), dict(horizon=9, lengths=[0, 1, 9, 6], state_best=True, mean=True), dict(horizon=9)):
                dev, twin = (x.optimise(w, maximise=maximise, end_final=end_final, **kw) for x in (e, a))
                assert same(dev, twin), f"{name} maximise={maximise} end_final={end_final} {kw}: device and host twin differ"
                assert dev["seconds"] > 0 and dev["rounds"][0] >= 2 * kw["horizon"] + 2 and (dev["rounds"][1] > 0) == (dev["largest_cyclic"] > 0)
        check_finite(a, ref, final, w, maximise, True, res_of=lambda **k: e.optimise(w, **k))
    check_finite(a, ref, final, w, False, False, res_of=lambda **k: e.optimise(w, **k))
    comps = e.components("all")
    dev = check_mean(a, ref, w, comps=comps, res_of=lambda **k: e.optimise(w, **k))
    assert CR.same(e.components("all"), comps)
    if RefOracle is not None:
        mo, ro, ao, (_, final_o, _), ref_o, _ = oracle_case(stcsp, RefOracle, name, None, prefix_k)
        for maximise in (False, True):
            kw = dict(horizon=9, lengths=[0, 1, 6, 9], maximise=maximise, mean=True)
            d, o = e.optimise(w, **kw), ao.optimise(w, **kw)
            assert d["best"].tolist() == o["best"].tolist() and d["omega_mean"] == o["omega_mean"] and sorted(d["comp_mean"]) == sorted(o["comp_mean"])
            assert [rows_of(x[1]) for x in d["witnesses"]] == [rows_of(x[1]) for x in o["witnesses"]]
    return dev


@pytest.mark.parametrize("weights", [small_weights, big_weights])
@pytest.mark.parametrize("name", ["LADDER", "juggling_b4_f5", "digitinvader3", "partialorder_8", "LADDER_UNTIL", "TRAP", "FUSE", "FUSE_UNTIL",
                                  "probe:until"])
def test_device_equals_twin_and_yardstick(stcsp, RefOracle, name, weights):
    """LADDER: 28 live edges, one partial wavefront. juggling_b4_f5: 224 edges, less than a workgroup, a component of 120.
    digitinvader3: 2,020 edges, several workgroups and no multiple of 256, a component of 504. partialorder_8: 5,358 edges,
    447 self-loop components, nmax == 1. The others: states that are not final, an edgeless live root, no live root."""
    m = device_case(stcsp, name)[0]
    dev = check_device(stcsp, name, weights(m.n_vars), RefOracle=RefOracle)
    expect = {"LADDER": 2, "juggling_b4_f5": 120, "digitinvader3": 504, "partialorder_8": 1, "FUSE": 0, "FUSE_UNTIL": 0}
    assert name not in expect or dev["largest_cyclic"] == expect[name]


def test_pins_on_the_ladder(stcsp):
    m, e, r, flags, a = device_case(stcsp, "LADDER")
    L = 12
    assert e.optimise({"m": 1}, horizon=L)["best"].tolist() == [0] * (L + 1)
    assert e.optimise({"m": 1}, horizon=L, maximise=True)["best"].tolist() == [0] + [3 * (k - 1) for k in range(1, L + 1)]
    res = e.optimise({"t": 1}, horizon=L, mean=True)
    assert res["best"].tolist() == [k // 2 for k in range(L + 1)] and res["omega_mean"] == (1, 2)
    res = e.optimise({"m": 2, "t": 1}, mean=True)
    assert sorted(pq for pq in res["comp_mean"] if pq[1]) == [(4 * j + 1, 2) for j in range(4)]
    m2, e2, *_ = device_case(stcsp, "TRAP")
    assert sorted(pq for pq in e2.optimise({"t": 1}, mean=True)["comp_mean"] if pq[1]) == [(0, 1), (1, 1), (1, 1), (1, 1), (2, 1)]


def test_lane_striding_and_ties_of_the_walk(stcsp, RefOracle):
    """A state with more than 64 live out-edges: the lanes of k_opt_walk stride. Under {t: 1} all 100 candidates of a step tie on
    cost, so the row order alone decides (a = b = 0); under {a: -1} ten of them tie (a = 9, b = 0)."""
    m, e, r, (valid, final, alive), a = device_case(stcsp, "FANOUT")
    o = RefOracle(m)
    ro = o.solve()
    ao = o.automaton(ro).traverse()
    out = Q.live_out_edges(ro, *ao.flags()[::2])
    assert max(len(edges) for edges in out.values()) == 100 > 64  # the degree, on the oracle
    ia, ib, it = (m.var_names.index(n) for n in "abt")
    for w, col_a in (({"t": 1}, 0), ({"a": -1}, 9), ({"a": 1, "b": 0, "t": -2 ** 30}, 0)):
        dev = e.optimise(w, horizon=7, lengths=[7, 3], state_best=True)
        assert same(dev, a.optimise(w, horizon=7, lengths=[7, 3], state_best=True))
        oracle = ao.optimise(w, horizon=7, lengths=[7, 3])
        assert dev["best"].tolist() == oracle["best"].tolist()
        for (length, rows, _), (_, rows_o, _) in zip(dev["witnesses"], oracle["witnesses"]):
            assert np.array_equal(rows, rows_o) and len(rows) == length
            assert rows[:, ia].tolist() == [col_a] * length and rows[:, ib].tolist() == [0] * length
    wv = [0] * m.n_vars
    wv[it] = 1
    check_device(stcsp, "FANOUT", wv)


def test_wide_domain_with_negative_values(stcsp, RefOracle):
    """neg_w4 of tests/test_wide_gpu.py: a starts at -50 and climbs, so the costs are negative under a positive weight."""
    m, e, r, flags, a = device_case(stcsp, "neg_w4")
    assert min(lo for lo, hi in m.var_bounds()) < 0
    w = [3 if n == "a" else -1 if n == "b" else 0 for n in m.var_names]
    check_device(stcsp, "neg_w4", w)
    best = e.optimise(w, horizon=9)["best"].tolist()
    assert best[0] == 0 and best[1] == 3 * -50 - 3 and all(x > y for x, y in zip(best, best[1:]))  # first a == -50, b at most 3
    big = big_weights(m.n_vars)
    check_device(stcsp, "neg_w4", big)
    o = RefOracle(m)
    ao = o.automaton(o.solve()).traverse()
    for ww in (w, big):
        d, t = (x.optimise(ww, horizon=9, lengths=[9], mean=True) for x in (e, ao))
        assert d["best"].tolist() == t["best"].tolist() and rows_of(d["witnesses"][0][1]) == rows_of(t["witnesses"][0][1])
        assert sorted(d["comp_mean"]) == sorted(t["comp_mean"]) and d["omega_mean"] == t["omega_mean"]


def test_interval_domains(stcsp, RefOracle):
    m = device_case(stcsp, "juggling_b4_f5", True)[0]
    dev = check_device(stcsp, "juggling_b4_f5", small_weights(m.n_vars), interval=True)
    plain = device_case(stcsp, "juggling_b4_f5")[1].optimise(small_weights(m.n_vars), mean=True)
    assert dev["largest_cyclic"] == 120 and dev["omega_mean"] == plain["omega_mean"]


@pytest.mark.parametrize("name", ["juggling_b5_f6", "digitinvader5"])
def test_larger_components_against_the_twin(stcsp, name):
    """Components of 720 and 2,772 states: the two Karp passes take 4 nmax launches."""
    m, e, r, flags, a = device_case(stcsp, name)
    for w in (small_weights(m.n_vars), big_weights(m.n_vars)):
        dev = e.optimise(w, mean=True)
        assert same(dev, a.optimise(w, mean=True))
        assert dev["largest_cyclic"] == {"juggling_b5_f6": 720, "digitinvader5": 2772}[name] and dev["rounds"][1] == 4 * dev["largest_cyclic"] + 2
    ones = {n: 1 for n in m.var_names if not n.startswith("_V")}
    assert same(e.optimise(ones, mean=True, maximise=True), a.optimise(ones, mean=True, maximise=True))


def test_partialorder_14_with_witnesses(stcsp):
    m, e, r, flags, a = device_case(stcsp, "partialorder_14")
    for w, maximise in ((small_weights(m.n_vars), False), (big_weights(m.n_vars), True)):
        kw = dict(horizon=16, lengths=[0, 1, 16], maximise=maximise, state_best=True)
        dev = e.optimise(w, **kw)
        assert same(dev, a.optimise(w, **kw)) and [len(rows) for _, rows, _ in dev["witnesses"]] == [0, 1, 16]
        assert same(e.optimise(w, horizon=16, maximise=maximise), a.optimise(w, horizon=16, maximise=maximise))
        acc, nend, fin, _ = a.check_streams([dev["witnesses"][2][1]], "all")
        assert acc.tolist() == [16]


def test_byte_budget(stcsp, monkeypatch):
    """Too small a budget is STCSP_E_NOMEM with the limit and the need in the message; the engine stays usable."""
    m, e, r, flags, a = device_case(stcsp, "digitinvader3")
    w = small_weights(m.n_vars)
    good = e.optimise(w, horizon=9, lengths=[9], mean=True)
    for budget, kw in ((4096, dict(horizon=9, lengths=[9])), (2 * r.n_states * 8 + 64, dict(horizon=9)), (10 * r.n_states * 8 + 64, dict(horizon=9, lengths=[9]))):
        monkeypatch.setenv("STCSP_OPTIMISE_BYTES", str(budget))
        with pytest.raises(stcsp.StcspError) as ex:
            e.optimise(w, **kw)
        assert ex.value.code == -4 and str(budget) in str(ex.value) and "STCSP_OPTIMISE_BYTES" in str(ex.value) and "need" in str(ex.value)
    monkeypatch.setenv("STCSP_OPTIMISE_BYTES", str(1 << 24))
    assert same(e.optimise(w, horizon=9, lengths=[9], mean=True), good)
    monkeypatch.delenv("STCSP_OPTIMISE_BYTES")
    assert same(e.optimise(w, horizon=9, lengths=[9], mean=True), good) and same(good, a.optimise(w, horizon=9, lengths=[9], mean=True))


def raw_optimise(stcsp, e, n_vars, horizon=0, flags=0, weights=True, lengths=None):
    w = (C.c_int32 * n_vars)(*([1] * n_vars))
    ln = (C.c_int32 * len(lengths))(*lengths) if lengths else None
    rq = stcsp.OptimiseRequest(w if weights else None, ln, horizon, len(lengths or ()), flags, 0)
    out = stcsp.OptimiseResult()
    return e._f("optimise")(e._h, C.byref(rq), C.byref(out))


def test_error_paths(stcsp):
    m = stcsp.Model.from_name("partialorder_10")
    n = m.n_vars
    e = stcsp.Engine(m)
    assert raw_optimise(stcsp, e, n) == -6  # before any solve
    e.solve()
    assert raw_optimise(stcsp, e, n) == -6  # before postprocess
    with pytest.raises(stcsp.StcspError) as ex:
        e.optimise([1] * n)
    assert ex.value.code == -6 and "postprocess" in str(ex.value)
    e.postprocess()
    assert raw_optimise(stcsp, e, n, 3, lengths=[0, 3]) == 0
    assert raw_optimise(stcsp, e, n, weights=False) == -1
    assert raw_optimise(stcsp, e, n, -1) == -1
    assert raw_optimise(stcsp, e, n, 3, lengths=[4]) == -1 and raw_optimise(stcsp, e, n, 3, lengths=[-1]) == -1
    with pytest.raises(stcsp.StcspError) as ex:
        e.optimise([2 ** 31 - 1] * n, horizon=2 ** 31 - 1)
    assert ex.value.code == -1 and "2^62" in str(ex.value)
    assert e._f("optimise")(e._h, None, C.byref(stcsp.OptimiseResult())) == -1
    assert raw_optimise(stcsp, e, n, 2, stcsp.OPT_MEAN) == 0  # the engine is still usable
    e.solve()  # a new solve ends the flags' validity
    assert raw_optimise(stcsp, e, n) == -6
    t = stcsp.Engine(m, max_search_nodes=2000, batch_nodes=256)  # truncated solve
    assert t.solve().truncated == 1
    t.postprocess()
    with pytest.raises(stcsp.StcspError) as ex:
        t.optimise([1] * n)
    assert ex.value.code == -6 and "truncated" in str(ex.value)
    s = stcsp.Engine(m, flags=stcsp.F_STEPPED)  # the sharded pipeline
    with pytest.raises(stcsp.StcspError) as ex:
        s.optimise([1] * n)
    assert ex.value.code == -2 and "stcsp_automaton_optimise" in str(ex.value)


def test_unsupported_beyond_the_exact_range(stcsp):
    """nmax^2 * cmax > 2^62: an aux variable with the whole int range, weight 2^31 - 1, a cycle of at least two states."""
    m, e, r, flags, a = device_case(stcsp, "INT_RANGE", True)
    whole = [i for i, b in enumerate(m.var_bounds()) if b == (-(2 ** 31), 2 ** 31 - 1)]
    nmax = int(e.components()["comp_size"].max())
    assert whole and nmax >= 2
    w = [0] * m.n_vars
    w[whole[0]] = 2 ** 31 - 1  # cmax = (2^31 - 1) 2^31 <= 2^62
    fine = e.optimise(w, horizon=1, lengths=[1], state_best=True)
    assert same(fine, a.optimise(w, horizon=1, lengths=[1], state_best=True))
    with pytest.raises(stcsp.StcspError) as ex:
        e.optimise(w, horizon=1, mean=True)
    assert ex.value.code == -2 and f"nmax = {nmax}" in str(ex.value) and f"cmax = {(2 ** 31 - 1) * 2 ** 31}" in str(ex.value)
    with pytest.raises(stcsp.StcspError) as ex:
        a.optimise(w, horizon=1, mean=True)
    assert ex.value.code == -2
    with pytest.raises(stcsp.StcspError) as ex:
        e.optimise(w, horizon=2)
    assert ex.value.code == -1
    w[whole[0]] = 2 ** 20
    assert same(e.optimise(w, horizon=3, mean=True), a.optimise(w, horizon=3, mean=True))


@pytest.mark.parametrize("first", [True, False])
def test_other_services_are_not_disturbed(stcsp, first):
    """monitor, generator, repair, infer, observer and compare give the same with an optimise() call between build and use, before or
    after the first use."""
    m = stcsp.Model.from_name("juggling_b4_f5")
    e = stcsp.Engine(m)
    e.solve()
    e.postprocess()
    mask = [int(n == "A") for n in m.var_names]
    e.monitor(mask)
    e.generator(mask, 6)
    obs = e.observer()
    streams = [obs["edge_values"][:1], np.zeros((0, 1), np.int32)]
    w = small_weights(m.n_vars)

    def use():
        acc, nend, fin, _ = e.check_streams(streams)
        values, gfin = e.generate(5, 6, ranks=[0, 1, 2, 3, 4])
        cmp = e.compare(obs)
        inf = e.infer_streams(streams)
        return [acc, nend, fin, values, gfin, e.repair_streams(streams)[0], cmp["witness_len"], np.int64(cmp["n_pairs"]), inf[0], np.concatenate(inf[2])]
    if first:
        opt = e.optimise(w, horizon=6, lengths=[6], mean=True, state_best=True)
        before = use()
    else:
        before = use()
        opt = e.optimise(w, horizon=6, lengths=[6], mean=True, state_best=True)
    assert opt["n_states"] == 121
    after = use()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    again = e.observer()
    assert all(np.array_equal(obs[k], again[k]) for k in ("member_off", "member", "state_final", "edge_src", "edge_dst", "edge_values"))
    assert same(e.optimise(w, horizon=6, lengths=[6], mean=True, state_best=True), opt)


def test_cli_optimise(stcsp, tmp_path):
    """--optimise= on LADDER, on the device and through the host twin (--shards=2): the lines are the twin's result, stdout and the
    written automaton those of the run without the option."""
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    (tmp_path / "m.csp").write_text(text_of(stcsp, "LADDER"))
    m, e, r, flags, a = device_case(stcsp, "LADDER")
    twin = a.optimise({"m": 2, "t": 1}, horizon=5, lengths=[5], maximise=True, mean=True)
    shown = [i for i, n in enumerate(m.var_names) if not n.startswith("_V")]

    def run(*opts, ok=True):
        p = subprocess.run([str(exe), "-s", *opts, str(tmp_path / "m.csp")], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert (p.returncode == 0) == ok, p.stderr
        return p, (tmp_path / "solutions.dot").read_bytes() if ok else None
    plain, dot = run()
    assert "optimise:" not in plain.stderr
    for opts in (("--optimise=max:m=2,t=1:5:mean",), ("--optimise=max:m=2,t=1:5:mean", "--shards=2")):
        p, dot2 = run(*opts)
        assert dot2 == dot and p.stdout.split()[:3] == plain.stdout.split()[:3]
        lines = [line[len("optimise: "):] for line in p.stderr.splitlines() if line.startswith("optimise: ")]
        assert lines[:6] == [f"best[{L}] = {twin['best'][L]}" for L in range(6)]
        assert lines[6] == "# " + " ".join(m.var_names[i] for i in shown)
        assert lines[7].startswith("witness:")
        got = tuple(tuple(map(int, row.split())) for row in lines[7][len("witness:"):].split(";"))
        assert got == tuple(tuple(int(row[i]) for i in shown) for row in twin["witnesses"][0][1])
        means = sorted(tuple(map(int, re.fullmatch(r"component \d+: mean (-?\d+)/(\d+)", line).groups())) for line in lines[8:-1])
        assert means == sorted(pq for pq in twin["comp_mean"] if pq[1]) and len(means) == 4
        assert re.fullmatch(r"omega: mean 13/2 in component \d+", lines[-1])
    p, _ = run("--optimise=min:t=1:4")
    lines = [line for line in p.stderr.splitlines() if line.startswith("optimise: ")]
    assert lines[:5] == [f"optimise: best[{L}] = {L // 2}" for L in range(5)] and not any("omega" in line or "component" in line for line in lines)
    for bad in ("--optimise=least:t=1", "--optimise=min:nobody=1", "--optimise=min:t=x", "--optimise=min:t=1:-3", "--optimise=min"):
        run(bad, ok=False)
