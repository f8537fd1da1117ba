"""Strongly connected components, omega-liveness and lasso solutions on the device (stcsp_engine_components, dev_components.hpp)
through the C ABI: device == host twin on the engine's own automaton, array by array, == the yardstick of
tests/components_ref.py on the CPU oracle's automaton wherever the oracle runs in seconds. Run on the GPU box: pytest -m gpu."""
import ctypes as C
import functools
import re
import subprocess

import numpy as np
import pytest

import components_ref as R
import quotient_ref as Q
from test_components import LASSO_LENGTHS, TABLE, oracle_case, text_of

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_case(stcsp, name, interval=False):
    """(model, engine, Result, (valid, final, alive), the host's automaton with the device's flags): solved and post-processed once."""
    m = stcsp.Model(text=text_of(stcsp, name))
    e = stcsp.Engine(m, flags=stcsp.F_INTERVAL_DOMAINS if interval else 0)
    r = e.solve()
    assert not r.truncated
    post = e.postprocess()
    return m, e, r, Q.post_flags(post), e.automaton(r).import_flags(post)


def check_device(stcsp, name, lassos="all", no_trim=False, interval=False, RefOracle=None, prefix_k=2):
    """Device == twin, exactly and array by array; with RefOracle also == the yardstick on the oracle's automaton."""
    m, e, r, (valid, final, alive), a = device_case(stcsp, name, interval)
    dev = e.components(lassos, no_trim)
    twin = a.components(lassos)
    assert R.same(dev, twin), f"{name} [{lassos}, no_trim={no_trim}]: device and host twin differ"
    assert dev["n_vars"] == m.n_vars and dev["seconds"] > 0
    assert dev["rounds"][1] <= dev["n_components"] and (dev["rounds"][0] == 0 if no_trim else True)  # a colouring round finds a component
    if RefOracle is not None:
        ref = oracle_case(stcsp, RefOracle, name, None, prefix_k)[4]
        R.check_result(r, valid, alive, dev, ref, same_numbering=False)
        if lassos == "all":
            assert R.result_lassos(dev) == ref["lassos"], f"{name}: device and yardstick differ"
    return dev


@pytest.mark.parametrize("name", list(TABLE))
def test_device_on_the_table(stcsp, RefOracle, name):
    dev = check_device(stcsp, name, RefOracle=RefOracle)
    got = (dev["n_states"], dev["n_components"], dev["n_cyclic"], dev["n_accepting"], dev["n_bottom"], int(dev["comp_size"].max(initial=0)),
           dev["n_omega"])
    assert got == TABLE[name][:1] + TABLE[name][2:]
    assert dev["root_omega"] == int(TABLE[name][7] > 0)
    if name in LASSO_LENGTHS:
        assert sorted((len(stem), len(loop)) for _, stem, loop in dev["lassos"]) == LASSO_LENGTHS[name]
    assert R.same(check_device(stcsp, name, 0), {**dev, "lassos": [], "n_lassos": 0})


@pytest.mark.parametrize("probe", ["until", "arr", "at", "misc", "adversarial"])
def test_device_on_the_probes(stcsp, RefOracle, probe):
    check_device(stcsp, "probe:" + probe, RefOracle=RefOracle)


def test_device_after_adversarial_pass(stcsp, RefOracle):
    """The flags are those of the last postprocess(), adversarial passes included."""
    m = stcsp.Model(text=text_of(stcsp, "probe:adversarial"))
    e = stcsp.Engine(m)
    r = e.solve()
    post = e.postprocess(adversarial=5)
    dev = e.components("all")
    assert R.same(dev, e.automaton(r).import_flags(post).components("all"))
    ref = oracle_case(stcsp, RefOracle, "probe:adversarial", 5)[4]
    R.check_result(r, *Q.post_flags(post)[::2], dev, ref, same_numbering=False)
    assert R.result_lassos(dev) == ref["lassos"]


def test_interval_domains(stcsp, RefOracle):
    dev = check_device(stcsp, "juggling_b4_f5", interval=True, RefOracle=RefOracle)
    assert (dev["n_states"], dev["n_components"], int(dev["comp_size"].max())) == (121, 2, 120)


def test_trim_corners(stcsp):
    """Self-looping singletons, a chain, an edgeless live root and no live root: the trimming finds all of them without a colouring
    round; no live root is zero components and no error."""
    for name in ("partialorder_8", "COUNTER", "FUSE", "FUSE_UNTIL"):
        dev = check_device(stcsp, name)
        assert dev["rounds"][1] == 0 and dev["n_components"] == TABLE[name][2], name
    dev = check_device(stcsp, "FUSE_UNTIL")
    assert (dev["n_states"], dev["n_components"], dev["n_omega"], dev["root_omega"], dev["n_lassos"]) == (0, 0, 0, 0, 0)
    assert (dev["state_component"] == -1).all() and not dev["state_omega"].any()


@pytest.mark.parametrize("name", ["LADDER", "LADDER_UNTIL", "TRAP", "FUSE_BRANCH", "juggling_b4_f4_nosym", "juggling_b4_f5", "random:1", "random:4",
                                  "random:5", "random:7"])
def test_colouring_alone_gives_the_same(stcsp, RefOracle, name):
    trimmed = check_device(stcsp, name, RefOracle=RefOracle)
    assert trimmed["n_states"] <= 130
    alone = check_device(stcsp, name, no_trim=True, RefOracle=RefOracle)
    assert R.same(alone, trimmed)
    assert alone["rounds"][0] == 0 and (alone["rounds"][1] >= 1 or alone["n_states"] == 0)


def test_sweep_depth(stcsp, RefOracle):
    """digitinvader3: one component of 504 states below the root."""
    dev = check_device(stcsp, "digitinvader3", RefOracle=RefOracle)
    assert sorted(dev["comp_size"].tolist()) == [1, 504] and dev["rounds"][1] == 1 and dev["rounds"][2] > 8
    assert R.same(check_device(stcsp, "digitinvader3", no_trim=True), dev)


def test_more_than_64_lassos(stcsp, RefOracle):
    """partialorder_8: 447 accepting components, seven stem passes of 64."""
    dev = check_device(stcsp, "partialorder_8", RefOracle=RefOracle)
    assert dev["n_lassos"] == 447 and all(len(loop) == 1 for _, _, loop in dev["lassos"])
    for n in (1, 64, 65, 130):
        assert R.same(check_device(stcsp, "partialorder_8", n), {**dev, "lassos": dev["lassos"][:n], "n_lassos": n})
    assert check_device(stcsp, "partialorder_8", "bottom")["n_lassos"] == 1


@pytest.mark.parametrize("name", ["digitinvader5", "partialorder_14"])
def test_device_equals_twin_on_larger_instances(stcsp, name):
    dev = check_device(stcsp, name, 64)
    assert dev["n_lassos"] == min(64, dev["n_accepting"]) > 0 and dev["root_omega"] == 1
    assert R.same(check_device(stcsp, name, 0), {**dev, "lassos": [], "n_lassos": 0})


def raw_components(stcsp, e, max_lassos=0, flags=0):
    co, out = stcsp.ComponentsOptions(max_lassos, flags), stcsp.ComponentsResult()
    return e._f("components")(e._h, C.byref(co), C.byref(out))


def test_error_paths(stcsp):
    m = stcsp.Model.from_name("partialorder_10")
    e = stcsp.Engine(m)
    assert raw_components(stcsp, e) == -6  # before any solve
    e.solve()
    assert raw_components(stcsp, e) == -6  # before postprocess
    with pytest.raises(stcsp.StcspError) as ex:
        e.components()
    assert ex.value.code == -6 and "postprocess" in str(ex.value)
    e.postprocess()
    assert raw_components(stcsp, e) == 0
    assert raw_components(stcsp, e, -2) == -1
    out = stcsp.ComponentsResult()
    assert e._f("components")(e._h, None, C.byref(out)) == 0 and (out.n_states, out.n_lassos) == (1920, 0)  # no options: no lassos
    e.solve()  # a new solve ends the flags' validity
    assert raw_components(stcsp, e) == -6
    t = stcsp.Engine(m, max_search_nodes=2000, batch_nodes=256)  # truncated solve
    assert t.solve().truncated == 1
    t.postprocess()
    with pytest.raises(stcsp.StcspError) as ex:
        t.components()
    assert ex.value.code == -6 and "truncated" in str(ex.value)
    s = stcsp.Engine(m, flags=stcsp.F_STEPPED)  # the sharded pipeline
    with pytest.raises(stcsp.StcspError) as ex:
        s.components()
    assert ex.value.code == -2 and "stcsp_automaton_components" in str(ex.value)


@pytest.mark.parametrize("first", [True, False])
def test_other_services_are_not_disturbed(stcsp, first):
    """monitor, generator, observer and compare give the same with a components() call between build and use, before or after
    the first use."""
    m = stcsp.Model.from_name("juggling_b4_f5")
    e = stcsp.Engine(m)
    e.solve()
    e.postprocess()
    mask = [int(n == "A") for n in m.var_names]
    e.monitor(mask)
    e.generator(mask, 6)
    obs = e.observer()
    streams = [obs["edge_values"][:1], np.zeros((0, 1), np.int32)]

    def use():
        acc, nend, fin, _ = e.check_streams(streams)
        values, gfin = e.generate(5, 6, ranks=[0, 1, 2, 3, 4])
        cmp = e.compare(obs)
        return [acc, nend, fin, values, gfin, e.repair_streams(streams)[0], cmp["witness_len"], np.int64(cmp["n_pairs"])]
    if first:
        comps = e.components("all", no_trim=True)
        before = use()
    else:
        before = use()
        comps = e.components("all")
    assert comps["n_states"] == 121
    after = use()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    again = e.observer()
    assert all(np.array_equal(obs[k], again[k]) for k in ("member_off", "member", "state_final", "edge_src", "edge_dst", "edge_values"))
    assert R.same(e.components("all"), comps)


def test_cli_components(stcsp, tmp_path):
    """--components=bottom on the device and through the host twin (--shards=2): the lines parse back to the twin's result, and
    stdout and the written automaton are those of the run without the option."""
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    name = "juggling_b4_f4_nosym"
    (tmp_path / "m.csp").write_text(text_of(stcsp, name))
    m, e, r, flags, a = device_case(stcsp, name)
    twin = a.components("bottom")
    shown = [i for i, n in enumerate(m.var_names) if not n.startswith("_V")]

    def run(*opts):
        p = subprocess.run([str(exe), "-s", *opts, str(tmp_path / "m.csp")], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert p.returncode == 0, p.stderr
        return p, (tmp_path / "solutions.dot").read_bytes()
    plain, dot = run()
    assert "components:" not in plain.stderr
    for opts in (("--components=bottom",), ("--components=bottom", "--shards=2")):
        p, dot2 = run(*opts)
        assert dot2 == dot and p.stdout.split()[:3] == plain.stdout.split()[:3]
        lines = [line[len("components: "):] for line in p.stderr.splitlines() if line.startswith("components: ")]
        head = list(map(int, re.findall(r"\d+", lines[0])))
        assert head == [twin[k] for k in ("n_states", "n_components", "n_cyclic", "n_accepting", "n_bottom", "n_omega")]
        assert lines[0].endswith("infinite solution: yes")
        comps = [re.fullmatch(r"component (\d+): size (\d+), depth (\d+), flags ([CFBA]+|-)", line) for line in lines[1:1 + twin["n_components"]]]
        assert all(comps)
        # (component numbers follow each solve's state numbering: compared as a multiset)
        letters = {R.CYCLIC: "C", R.FINAL: "F", R.BOTTOM: "B", R.ACCEPTING: "A"}
        expect = sorted((int(s), int(d), "".join(c for bit, c in letters.items() if f & bit) or "-")
                        for s, d, f in zip(twin["comp_size"], twin["comp_depth"], twin["comp_flags"]))
        assert sorted((int(c.group(2)), int(c.group(3)), c.group(4)) for c in comps) == expect
        assert [int(c.group(1)) for c in comps] == list(range(twin["n_components"]))
        rest = lines[1 + twin["n_components"]:]
        assert rest[0] == "# " + " ".join(m.var_names[i] for i in shown) and len(rest) == 1 + 3 * twin["n_lassos"]

        def rows(line, key):
            assert line.startswith(key)
            body = line[len(key):]
            return tuple(tuple(map(int, row.split())) for row in body.split(";")) if body.strip() else ()
        got = {(rows(rest[2 + 3 * i], "stem:"), rows(rest[3 + 3 * i], "loop:")) for i in range(twin["n_lassos"])}
        assert got == {(tuple(tuple(int(row[i]) for i in shown) for row in stem), tuple(tuple(int(row[i]) for i in shown) for row in loop))
                       for _, stem, loop in twin["lassos"]}
        assert all(re.fullmatch(r"lasso of component \d+: 1 \+ 4 steps", rest[1 + 3 * i]) for i in range(twin["n_lassos"]))
    none, _ = run("--components")
    assert sum(line.startswith("components: component") for line in none.stderr.splitlines()) == 7 and "stem:" not in none.stderr
