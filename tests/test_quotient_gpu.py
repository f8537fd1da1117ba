"""Bisimulation quotient on the device (stcsp_engine_quotient, dev_quotient.hpp) through the C ABI, against the independent
yardstick of tests/quotient_ref.py (plain Python partition refinement on the automaton of the CPU oracle; states matched by the
canonical numbering) and against the host twin. Run on the GPU box: pytest -m gpu.

The oracle restates the reference's single-threaded search: 46 s on partialorder_14 and 25 minutes on digitinvader9 (one core).
The yardstick therefore runs by default on 21 of the 26 shipped instances and on all of them with STCSP_SLOW=1 (SLOW_ORACLE below);
the host twin -- itself pinned to the yardstick in tests/test_quotient.py -- is compared with the device on every instance always.
The yardstick was run once on the oracle's partialorder_14 and digitinvader9 (CPU only): equal to the host twin's partition,
32,256 and 30,030 classes under both masks."""
import json
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import quotient_ref as Q
from canon import canon
from fuzz_models import random_model
from test_quotient import COUNTDOWN, COUNTER, DUPLICATES, FUZZ_SEEDS, PROBES

pytestmark = pytest.mark.gpu

SLOW = os.environ.get("STCSP_SLOW") == "1"
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "reference_golden.json").read_text())
ALL_EXAMPLES = [n for n, v in GOLDEN.items() if isinstance(v, dict) and "edges" in v]
assert len(ALL_EXAMPLES) == 26
SLOW_ORACLE = {"partialorder_14", "digitinvader6", "digitinvader7", "digitinvader8", "digitinvader9"}  # minutes of oracle each


def device_classes(stcsp, m, adversarial=-1, **opts):
    e = stcsp.Engine(m, **opts)
    r = e.solve()
    post = e.postprocess(adversarial=adversarial)
    return e, r, Q.post_flags(post)


def check_device(stcsp, RefOracle, m, what, adversarial=-1, oracle=True, **opts):
    """Device partition == host twin (same automaton, same flags) == yardstick on the oracle's automaton, for the default mask
    and for `all`; canonical class numbers; rounds <= live states + 1. Returns {mask name: (live, classes)}."""
    e, r, (valid, final, alive) = device_classes(stcsp, m, adversarial, **opts)
    host = e.automaton(r).import_flags(e.postprocess(adversarial=adversarial))
    if oracle:
        o = RefOracle(m)
        ro = o.solve()
        ao = o.automaton(ro).traverse()
        if adversarial >= 0:
            ao.adversarial(adversarial)
        ovalid, ofinal, oalive = ao.flags()
    res = {}
    for name, mask in {"default": Q.default_mask(m.var_names), "all": [1] * m.n_vars}.items():
        arg = None if name == "default" else "all"
        cls, n_classes, rounds, seconds = e.quotient(arg)
        qr = e.quotient_result
        n_live = int((cls >= 0).sum())
        assert qr.n_states == n_live and rounds <= n_live + 1, f"{what} [{name}]"
        hc, hn, _ = host.bisimulation(arg)
        assert hn == n_classes and np.array_equal(hc, cls), f"{what} [{name}]: device and host twin differ"
        firsts = [int(np.flatnonzero(cls == c)[0]) for c in range(n_classes)]
        assert firsts == sorted(firsts), f"{what} [{name}]: classes are numbered by their least member"
        q = host.quotient(cls, mask).renumber()
        assert (q.n_live_states, q.n_live_edges) == (n_classes if n_live else 0, qr.n_class_edges), f"{what} [{name}]"
        if oracle:
            part, yn, out, num, ycls = Q.yardstick(m, ro, ovalid, ofinal, oalive, mask)
            assert n_classes == yn and Q.engine_partition(r, valid, alive, cls) == part, f"{what} [{name}]: device and yardstick differ"
            assert (q.n_live_states, q.n_live_edges) == (Q.quotient_counts(out, num, ycls, mask) if num else (0, 0)), f"{what} [{name}]"
            if name == "all" and num:
                # no state matching needed: the quotient built from the oracle's automaton and the Python classes
                ycanon = {}
                yarr = np.full(ro.n_states, -1, dtype=np.int32)
                for s in sorted(ycls):
                    yarr[s] = ycanon.setdefault(ycls[s], len(ycanon))
                assert q.canonical() == ao.quotient(yarr, mask).renumber().canonical(), f"{what} [all]"
        res[name] = (n_live, n_classes)
    return res


@pytest.mark.parametrize("name", ALL_EXAMPLES)
def test_device_partition_on_goldens(stcsp, RefOracle, name):
    check_device(stcsp, RefOracle, stcsp.Model.from_name(name), name, oracle=SLOW or name not in SLOW_ORACLE)


@pytest.mark.parametrize("probe", ["until", "arr", "at", "misc", "adversarial"])
def test_device_partition_on_probes(stcsp, RefOracle, probe):
    m = stcsp.Model(text=PROBES[probe]["text"])
    check_device(stcsp, RefOracle, m, probe)
    if probe == "adversarial":
        res = check_device(stcsp, RefOracle, m, probe, adversarial=5)
        assert res["all"][0] == PROBES[probe]["adver1_live_states"]


@pytest.mark.parametrize("block", range(4))
def test_device_partition_on_fuzz_models(stcsp, RefOracle, block):
    checked = folded = 0
    for seed in [s for s in FUZZ_SEEDS if s % 4 == block]:
        text = random_model(seed)
        try:
            res = check_device(stcsp, RefOracle, stcsp.Model(text=text), f"seed {seed}\n{text}")
        except stcsp.StcspError as ex:
            assert ex.code == -2, f"seed {seed}: {ex}\n{text}"  # a domain the bitset kernels refuse
            continue
        checked += 1
        folded += res["default"][1] < res["default"][0]
    assert checked >= 45 and folded >= 1


@pytest.mark.parametrize("name", ["juggling_b4_f5", "digitinvader3", "partialorder_10"])
def test_device_partition_under_interval_domains(stcsp, RefOracle, name):
    check_device(stcsp, RefOracle, stcsp.Model.from_name(name), name, flags=stcsp.F_INTERVAL_DOMAINS)


@pytest.mark.parametrize("n", [6, 7, 8, 9])
def test_device_partition_after_adversarial_pass(stcsp, RefOracle, n):
    """-a on digitinvader: state_valid / edge_alive are what the adversarial pass left, which postprocess() wrote last."""
    check_device(stcsp, RefOracle, stcsp.Model.from_name(f"digitinvader{n}"), f"digitinvader{n} -a", adversarial=5, oracle=SLOW)


def test_device_partition_partialorder_14(stcsp, RefOracle):
    res = check_device(stcsp, RefOracle, stcsp.Model.from_name("partialorder_14"), "partialorder_14", oracle=SLOW)
    assert res["all"][0] == GOLDEN["partialorder_14"]["states"]


def test_device_hand_derived_counts(stcsp, RefOracle):
    """The counts derived by hand in tests/test_quotient.py::test_hand_derived_counts, on the device."""
    expect = {(COUNTER, "x"): (4, 1, 2), (COUNTER, "all"): (4, 4, 8), (COUNTDOWN, "x"): (4, 4, 7), (DUPLICATES, "x"): (4, 1, 2),
              (DUPLICATES, "all"): (4, 4, 14)}
    for (text, which), (live, classes, edges) in expect.items():
        m = stcsp.Model(text=text)
        e, r, _ = device_classes(stcsp, m)
        cls, n_classes, rounds, _ = e.quotient("all" if which == "all" else [int(n == "x") for n in m.var_names])
        assert (int((cls >= 0).sum()), n_classes, e.quotient_result.n_class_edges) == (live, classes, edges), (text, which)
        assert rounds <= live + 1 and (text != COUNTDOWN or rounds >= 4)
        check_device(stcsp, RefOracle, m, text)


def test_a_shipped_family_folds_on_the_device(stcsp, RefOracle):
    res = {n: check_device(stcsp, RefOracle, stcsp.Model.from_name(n), n)["default"] for n in ["juggling_b4_f4", "juggling_b4_f4_nosym"]}
    assert res["juggling_b4_f4"] == (5, 4) and res["juggling_b4_f4_nosym"] == (25, 25)


def test_error_paths(stcsp):
    m = stcsp.Model.from_name("partialorder_10")
    e = stcsp.Engine(m)
    with pytest.raises(stcsp.StcspError) as ex:  # before any solve
        e.quotient()
    assert ex.value.code == -6
    e.solve()
    with pytest.raises(stcsp.StcspError) as ex:  # before postprocess
        e.quotient()
    assert ex.value.code == -6
    e.postprocess()
    e.quotient()
    e.solve()                                    # a new solve invalidates the flags
    with pytest.raises(stcsp.StcspError) as ex:
        e.quotient()
    assert ex.value.code == -6
    with pytest.raises(ValueError):
        e.quotient([1, 0])
    t = stcsp.Engine(m, max_search_nodes=2000, batch_nodes=256)  # truncated solve
    assert t.solve().truncated == 1
    t.postprocess()
    with pytest.raises(stcsp.StcspError) as ex:
        t.quotient()
    assert ex.value.code == -6
    s = stcsp.Engine(m, flags=stcsp.F_STEPPED)  # the sharded pipeline
    with pytest.raises(stcsp.StcspError) as ex:
        s.quotient()
    assert ex.value.code == -2


def run_cli(stcsp, tmp_path, text, *flags):
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    f = tmp_path / "m.csp"
    f.write_text(text)
    r = subprocess.run([str(exe), "-s", *flags, str(f)], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("name", ["juggling_b4_f5", "digitinvader3", "counter"])
def test_cli_quotient(stcsp, RefOracle, tmp_path, name):
    text = DUPLICATES if name == "counter" else stcsp.instances.by_name(name)
    m = stcsp.Model(text=text)
    o = RefOracle(m)
    ro = o.solve()
    ao = o.automaton(ro).traverse()
    valid, final, alive = ao.flags()
    plain = run_cli(stcsp, tmp_path, text)
    assert "quotient" not in plain.stderr
    plain_canon = canon(str(tmp_path / "solutions.dot"))[0]
    assert plain_canon == o.automaton(ro).traverse().renumber().canonical()
    # --quotient=all: the same canonical text as the quotient built from the oracle's automaton and the yardstick's classes
    mask = [1] * m.n_vars
    part, yn, out, num, ycls = Q.yardstick(m, ro, valid, final, alive, mask)
    ycanon, yarr = {}, np.full(ro.n_states, -1, dtype=np.int32)
    for s in sorted(ycls):
        yarr[s] = ycanon.setdefault(ycls[s], len(ycanon))
    r = run_cli(stcsp, tmp_path, text, "--quotient=all")
    assert r.stderr.strip().splitlines()[-1] == f"quotient: {len(num)} -> {yn}"
    assert r.stdout.split("\t")[1:6] == plain.stdout.split("\t")[1:6]  # the reference's line: var con dom node fail
    assert canon(str(tmp_path / "solutions.dot"))[0] == ao.quotient(yarr, mask).renumber().canonical()
    # --quotient: state and edge counts of the yardstick's quotient under the default mask
    mask = Q.default_mask(m.var_names)
    part, yn, out, num, ycls = Q.yardstick(m, ro, valid, final, alive, mask)
    r = run_cli(stcsp, tmp_path, text, "--quotient")
    assert r.stderr.strip().splitlines()[-1] == f"quotient: {len(num)} -> {yn}"
    _, ns, ne = canon(str(tmp_path / "solutions.dot"))
    assert (ns, ne) == Q.quotient_counts(out, num, ycls, mask)
