"""The observer (subset construction) on the device (stcsp_engine_observer, dev_observer.hpp) through the C ABI: device == host twin on
the same automaton == the yardstick of tests/observer_ref.py on the automaton of the CPU oracle (states matched by the canonical
numbering). Run on the GPU box: pytest -m gpu."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import monitor_ref as M
import observer_ref as R
import quotient_ref as Q
from canon import canon
from fuzz_models import random_model
from test_monitor import NO_LIVE_ROOT

pytestmark = pytest.mark.gpu

SCALARS = ("n_states", "n_edges", "n_labels", "max_set", "levels", "n_observable")
ARRAYS = ("member_off", "member", "state_final", "edge_src", "edge_dst", "edge_values")
GPU_TABLE = [k for k in R.TABLE if k[0] != "crafted63"]
# fuzz_models.random_model seeds whose automaton has more than one live state, and two without a live root. Sized on the CPU with the
# twin: under the three masks of the test their observers have 0 to 13 sets with up to 24 members, all below FUZZ_MAX_STATES.
FUZZ_SEEDS = [1, 4, 5, 6, 7, 10, 13, 16, 21, 24, 29, 32, 34, 36, 37]
FUZZ_MAX_STATES = 64


def text_of(stcsp, name):
    if name.startswith("crafted"):
        k = int(name[7:])
        return R.CRAFTED % (k, k)
    if name.startswith("fuzz"):
        return random_model(int(name[4:]))
    return {"dead": NO_LIVE_ROOT}.get(name) or stcsp.instances.by_name(name)


@functools.lru_cache(maxsize=2)
def oracle_of(stcsp, RefOracle, name, prefix_k=2):
    m = stcsp.Model(text=text_of(stcsp, name), prefix_k=prefix_k)
    o = RefOracle(m)
    r = o.solve()
    a = o.automaton(r).traverse()
    return m, o, r, a


def solved(stcsp, name, **opts):
    m = stcsp.Model(text=text_of(stcsp, name))
    e = stcsp.Engine(m, **opts)
    r = e.solve()
    post = e.postprocess()
    return m, e, r, post, e.automaton(r).import_flags(post)


def same(a, b):
    return all(a[k] == b[k] for k in SCALARS) and all(np.array_equal(a[k], b[k]) for k in ARRAYS)


def check_device(stcsp, RefOracle, name, which, max_states=0, oracle=True, prefix_k=2):
    """Device == twin, exactly and array by array; device == yardstick after mapping the members through the canonical numbers."""
    m, e, r, post, host = solved(stcsp, name)
    mask = which if isinstance(which, list) else R.resolve_mask(m, which)
    e.generator(mask, 0)
    dev = e.observer(max_states)
    R.check_shape(dev)
    twin = host.observer(mask, max_states)
    assert same(dev, twin), f"{name} [{which}]: device and host twin differ"
    if oracle:
        mo, o, ro, ao = oracle_of(stcsp, RefOracle, name, prefix_k)
        ovalid, ofinal, oalive = ao.flags()
        expect = R.subset_construction(M.Yardstick(ro, ovalid, ofinal, oalive, mask))
        valid, final, alive = Q.post_flags(post)
        assert R.normalised(dev, R.numbers_of(r, valid, alive)) == expect, f"{name} [{which}]: device and yardstick differ"
    return m, e, host, mask, dev


@pytest.mark.parametrize("name,which", GPU_TABLE)
def test_device_observer_on_the_table(stcsp, RefOracle, name, which):
    dev = check_device(stcsp, RefOracle, name, which)[4]
    assert (dev["n_states"], dev["n_edges"], dev["max_set"], dev["levels"]) == R.TABLE[(name, which)][2:]


@pytest.mark.parametrize("k", [5, 63, 127])
def test_device_observer_on_the_crafted_model(stcsp, RefOracle, k):
    """tests/test_observer.py::test_hand_derived_observers: k + 2 sets, (k + 2)(k + 1) edges, the largest set holds every h."""
    dev = check_device(stcsp, RefOracle, f"crafted{k}", "only:x")[4]
    assert (dev["n_states"], dev["n_edges"], dev["max_set"], dev["levels"]) == (k + 2, (k + 2) * (k + 1), k + 1, 2)


@pytest.mark.parametrize("name", ["juggling_b4_f5", "digitinvader3"])
def test_device_observer_under_all_and_default(stcsp, RefOracle, name):
    m, e, host, mask, dev = check_device(stcsp, RefOracle, name, "all")
    assert dev["max_set"] == 1 and dev["n_states"] == host.n_live_states and dev["n_edges"] == host.n_live_edges
    assert host.from_observer(dev, mask).renumber().canonical() == host.renumber().canonical()
    check_device(stcsp, RefOracle, name, "default")


def test_empty_observer(stcsp, RefOracle):
    dev = check_device(stcsp, RefOracle, "dead", "default")[4]
    assert (dev["n_states"], dev["n_edges"], dev["levels"], dev["max_set"]) == (0, 0, 0, 0) and dev["member_off"].tolist() == [0]


def test_no_observable_variable(stcsp, RefOracle):
    """Every label projects on the empty row: the observer is the chain of the breadth-first levels of the live automaton."""
    m = stcsp.Model(text=text_of(stcsp, "juggling_b4_f5"))
    dev = check_device(stcsp, RefOracle, "juggling_b4_f5", [0] * m.n_vars)[4]
    assert dev["n_labels"] == 1 and dev["n_observable"] == 0 and dev["edge_values"].shape == (dev["n_edges"], 0)
    assert dev["n_edges"] == dev["n_states"] and dev["edge_src"].tolist() == list(range(dev["n_states"]))  # a chain into a loop


@pytest.mark.parametrize("name,which", [("juggling_b4_f5", "only:B0"), ("partialorder_10", "only:succ")])
def test_global_scratch_path_equals_lds_path(stcsp, RefOracle, monkeypatch, name, which):
    m, e, host, mask, dev = check_device(stcsp, RefOracle, name, which, oracle=False)
    monkeypatch.setenv("STCSP_OBSERVER_GLOBAL_SCRATCH", "1")
    assert same(e.observer(), dev)
    monkeypatch.delenv("STCSP_OBSERVER_GLOBAL_SCRATCH")
    assert same(e.observer(), dev)


def test_byte_budget(stcsp, RefOracle, monkeypatch):
    """A budget that one set's work items do not fit, and one that holds the items of a level but not the member lists: STCSP_E_NOMEM
    both times, nothing else on the engine is disturbed, and the next call with room succeeds."""
    m, e, host, mask, dev = check_device(stcsp, RefOracle, "juggling_b4_f5", "only:B0", oracle=False)
    e.generator(mask, 3)
    e.monitor(mask)
    streams = [dev["edge_values"][:1], np.zeros((0, 1), np.int32)]

    def others():
        acc, nend, fin, _ = e.check_streams(streams)
        values, gfin = e.generate(4, 3, ranks=[0, 1, 2, 3])
        return [acc, nend, fin, values, gfin, e.repair_streams(streams)[0]]
    before = others()
    for tiny in (64, max(8300, int(dev["member_off"][-1]) * 4 // 2)):
        monkeypatch.setenv("STCSP_OBSERVER_BYTES", str(tiny))
        with pytest.raises(stcsp.StcspError) as ex:
            e.observer()
        assert ex.value.code == -4 and "STCSP_OBSERVER_BYTES" in str(ex.value) and "level" in str(ex.value)
        assert all(np.array_equal(x, y) for x, y in zip(before, others()))
    monkeypatch.delenv("STCSP_OBSERVER_BYTES")
    assert same(e.observer(), dev)
    assert all(np.array_equal(x, y) for x, y in zip(before, others()))
    monkeypatch.setenv("STCSP_OBSERVER_BYTES", str(1 << 20))  # room for everything, in smaller chunks
    assert same(e.observer(), dev)


def test_max_states(stcsp, RefOracle):
    m, e, host, mask, dev = check_device(stcsp, RefOracle, "digitinvader3", "only:D1", oracle=False)
    n = dev["n_states"]
    with pytest.raises(stcsp.StcspError) as ex:
        e.observer(n - 1)
    assert ex.value.code == -4 and "max_states" in str(ex.value) and "level" in str(ex.value)
    assert same(e.observer(n), dev)
    with pytest.raises(stcsp.StcspError) as ex:
        host.observer(mask, n - 1)
    assert ex.value.code == -4


def raw_observer(stcsp, e):
    oo, out = stcsp.ObserverOptions(0), stcsp.ObserverResult()
    return e._f("observer")(e._h, C.byref(oo), C.byref(out))


def test_error_paths(stcsp):
    m = stcsp.Model.from_name("partialorder_10")
    e = stcsp.Engine(m)
    assert raw_observer(stcsp, e) == -6  # before any solve
    e.solve()
    assert raw_observer(stcsp, e) == -6  # before postprocess
    e.postprocess()
    assert raw_observer(stcsp, e) == -6  # without a generator
    with pytest.raises(stcsp.StcspError) as ex:
        e.observer()
    assert ex.value.code == -6
    e.generator(None, 0)
    assert e.observer()["n_states"] == 1920
    e.postprocess()                       # new flags invalidate the generator
    assert raw_observer(stcsp, e) == -6
    e.generator(None, 0)
    e.solve()                             # and so does a new solve
    assert raw_observer(stcsp, e) == -6
    with pytest.raises(stcsp.StcspError) as ex:
        e.observer()
    assert ex.value.code == -6
    t = stcsp.Engine(m, max_search_nodes=2000, batch_nodes=256)  # truncated solve
    assert t.solve().truncated == 1
    t.postprocess()
    assert raw_observer(stcsp, t) == -6
    s = stcsp.Engine(m, flags=stcsp.F_STEPPED)  # the sharded pipeline
    assert raw_observer(stcsp, s) == -2
    oo, out = stcsp.ObserverOptions(-1), stcsp.ObserverResult()
    e.postprocess()
    e.generator(None, 0)
    assert e._f("observer")(e._h, C.byref(oo), C.byref(out)) == -1


@pytest.mark.parametrize("block", range(3))
def test_device_observer_on_fuzz_models(stcsp, RefOracle, block):
    grown = 0
    for seed in [s for s in FUZZ_SEEDS if s % 3 == block]:
        name = f"fuzz{seed}"
        m, o, r, a = oracle_of(stcsp, RefOracle, name)
        first = next(n for n in m.var_names if not n.startswith("_V"))
        for which, mask in (("default", Q.default_mask(m.var_names)), ("hidden", M.hidden_signature_mask(m, r)), ("only", R.only(m, first))):
            dev = check_device(stcsp, RefOracle, name, mask, max_states=FUZZ_MAX_STATES)[4]
            grown += dev["max_set"] > 1
    assert grown >= 1


def run_cli(stcsp, tmp_path, text, *flags):
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    f = tmp_path / "m.csp"
    f.write_text(text)
    r = subprocess.run([str(exe), "-s", *flags, str(f)], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_observer(stcsp, RefOracle, tmp_path):
    """--observer=B0 on the device, through the host twin (--shards=2) and folded (--quotient): the files are the ones the twin's
    observer of the oracle's automaton gives, byte for byte the same on both roads."""
    name, which = "juggling_b4_f5", "only:B0"
    m, o, ro, ao = oracle_of(stcsp, RefOracle, name)
    mask = R.resolve_mask(m, which)
    obs = ao.observer(mask)
    expect = ao.from_observer(obs, mask).renumber()
    r = run_cli(stcsp, tmp_path, text_of(stcsp, name), "--observer=B0", f"--binary={tmp_path / 'dev.bin'}")
    assert r.stderr.strip().splitlines()[-1] == f"observer: 121 -> {obs['n_states']} states, {obs['n_edges']} edges"
    dot = (tmp_path / "solutions.dot").read_bytes()
    text, ns, ne = canon(str(tmp_path / "solutions.dot"))
    assert text == expect.canonical() and (ns, ne) == (621, 1041)
    assert stcsp.Automaton.read_binary(str(tmp_path / "dev.bin")).canonical() == expect.canonical()
    run_cli(stcsp, tmp_path, text_of(stcsp, name), "--observer=B0", "--shards=2", f"--binary={tmp_path / 'twin.bin'}")
    assert (tmp_path / "solutions.dot").read_bytes() == dot and (tmp_path / "twin.bin").read_bytes() == (tmp_path / "dev.bin").read_bytes()
    sets, final, edges, _ = R.subset_construction(M.Yardstick(ro, *ao.flags(), mask))
    pairs = {}
    for s, p, d in edges:
        pairs.setdefault(s, []).append((p, d))
    classes = len(set(Q.coarsest_partition(range(len(sets)), final, pairs)[0].values()))
    r = run_cli(stcsp, tmp_path, text_of(stcsp, name), "--observer=B0", "--quotient")
    assert r.stderr.strip().splitlines()[-2:] == [f"observer: 121 -> 621 states, 1041 edges", f"quotient: 621 -> {classes}"]
    assert canon(str(tmp_path / "solutions.dot"))[1] == classes
