"""Checking observed streams on the device (stcsp_engine_monitor_build / stcsp_engine_monitor_check, dev_monitor.hpp) through the C
ABI, against the host twin on the same automaton and flags and against the independent yardstick of tests/monitor_ref.py (plain
Python sets of states over the automaton of the CPU oracle). Run on the GPU box: pytest -m gpu.

The answers (accepted_len, n_end, end_final) do not depend on state numbers, so the device, the host twin and the yardstick are
compared directly. As in tests/test_quotient_gpu.py the oracle takes minutes on five instances (SLOW_ORACLE): the yardstick runs on
the other 21 by default and on all 26 with STCSP_SLOW=1; the host twin is compared with the device on every instance always.

The fallback is a cap that must not hide failures. Everywhere the exact relation is asserted: the device hands a stream to the host
twin if and only if the host twin, on the same automaton, meets a set larger than the kernel's capacity (256 states). Where the
yardstick runs, the host twin is run on the ORACLE's automaton with the same streams first, and n_host_fallback == 0 is asserted
from that. Largest sets measured that way under the default mask (CPU, seed 7, 16 walks of up to 200 steps): 1 on the 5 digitinvader
and 16 juggling instances outside SLOW_ORACLE, 2 on partialorder_10 .. 13; 1 everywhere under `all`. No shipped instance comes
near the capacity, so none is compared through the fallback; the crafted models below are (100 and 300 hidden values)."""
import json
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import monitor_ref as M
import quotient_ref as Q
from fuzz_models import random_model
from test_quotient import COUNTDOWN, COUNTER, DUPLICATES, FUZZ_SEEDS, PROBES

pytestmark = pytest.mark.gpu

SLOW = os.environ.get("STCSP_SLOW") == "1"
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "reference_golden.json").read_text())
ALL_EXAMPLES = [n for n, v in GOLDEN.items() if isinstance(v, dict) and "edges" in v]
assert len(ALL_EXAMPLES) == 26
SLOW_ORACLE = {"partialorder_14", "digitinvader6", "digitinvader7", "digitinvader8", "digitinvader9"}  # as in test_quotient_gpu.py
CAPACITY = 256  # kMonSetCap of dev_monitor.hpp; MonitorInfo.set_capacity reports it

# A free observable x beside a hidden h of 100 / 300 / 5 values that the signature carries: a stream over x alone holds that many
# states after its first step.
HIDDEN = "var x:[0,1]; var h:[0,%d]; next h == h;"


def solved(stcsp, m, adversarial=-1, **opts):
    e = stcsp.Engine(m, **opts)
    r = e.solve()
    post = e.postprocess(adversarial=adversarial)
    host = e.automaton(r).import_flags(post)
    return e, r, post, host


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


def check_device(stcsp, RefOracle, m, what, adversarial=-1, oracle=True, masks=("default", "all"), n_walks=16, max_len=200, seed=7, **opts):
    """Device == host twin on the same automaton and flags == yardstick on the oracle's automaton, on walks, mutated walks and
    random rows; the deterministic walk and the state-set walk agree; the fallback relation. Returns {mask: MonitorInfo dict}."""
    e, r, post, host = solved(stcsp, m, adversarial, **opts)
    if oracle:
        o = RefOracle(m)
        ro = o.solve()
        ao = o.automaton(ro).traverse()
        if adversarial >= 0:
            ao.adversarial(adversarial)
        flags, rr = ao.flags(), ro
    else:
        flags, rr = Q.post_flags(post), r
    res = {}
    for name, mask in M.masks(m, rr).items():
        if name not in masks:
            continue
        arg = None if name == "default" else mask
        y = M.Yardstick(rr, *flags, mask)  # (the streams come from a numbering-independent order of its edges)
        streams, kinds, where = M.make_streams(y, m.var_bounds(), seed, n_walks, max_len)
        info = e.monitor(arg)
        assert info.set_capacity == CAPACITY and info.n_observable == sum(mask) and info.root_live == int(bool(y.live)), f"{what} [{name}]"
        assert info.n_states == len(y.live) and info.n_edges == len(y.edges) and info.n_pairs == len(y.trans), f"{what} [{name}]"
        assert info.n_labels == len({p for _, p, _ in y.edges}), f"{what} [{name}]"
        assert info.max_destinations == max((len(d) for d in y.trans.values()), default=0), f"{what} [{name}]"
        dev = e.check_streams(streams)
        kernel = e.monitor_result.walk_kernel
        assert kernel == (0 if not y.live else 2 if info.max_destinations > 1 else 1), f"{what} [{name}]"
        hst = host.check_streams(streams, arg)
        print(f"{what} [{name}]: live {info.n_states} labels {info.n_labels} pairs {info.n_pairs} max destinations {info.max_destinations} "
              f"kernel {kernel} host twin's largest set {hst[3]} fallback {dev[3]}")
        assert same(dev, hst), f"{what} [{name}]: device and host twin differ"
        assert (dev[3] > 0) == (hst[3] > CAPACITY), f"{what} [{name}]: fallback {dev[3]}, host twin's largest set {hst[3]}"
        if oracle:
            on_oracle = ao.check_streams(streams, arg)  # the host twin on the oracle's automaton, the same streams
            yard = y.check_all(streams)
            assert same(on_oracle, yard) and on_oracle[3] == yard[3] == hst[3], f"{what} [{name}]: host twin and yardstick differ"
            assert same(dev, yard), f"{what} [{name}]: device and yardstick differ"
            if on_oracle[3] <= CAPACITY:
                assert dev[3] == 0, f"{what} [{name}]: sets of at most {on_oracle[3]} states need no fallback"
        for i, k in enumerate(kinds):
            if k == "walk":
                assert dev[0][i] == len(streams[i]), f"{what} [{name}]: a walk on the live automaton is accepted whole"
        if name == "all":  # determinism: no measurement needed
            assert info.max_destinations <= 1 and dev[3] == 0, f"{what} [all]"
            assert (dev[1] == (1 if y.live else 0)).all(), f"{what} [all]"
        if y.live:  # the state-set kernel gives the same answers where the deterministic walk ran (and the other way round)
            forced = e.check_streams(streams, force_sets=True)
            assert e.monitor_result.walk_kernel == 2 and same(forced, dev) and forced[3] == dev[3], f"{what} [{name}]: the two walk kernels differ"
        res[name] = info.as_dict()
    return res


@pytest.mark.parametrize("name", ALL_EXAMPLES)
def test_device_answers_on_goldens(stcsp, RefOracle, name):
    check_device(stcsp, RefOracle, stcsp.Model.from_name(name), name, oracle=SLOW or name not in SLOW_ORACLE)


@pytest.mark.parametrize("name", ["juggling_b4_f5", "digitinvader3", "partialorder_10"])
def test_device_answers_under_a_mask_hiding_a_signature_variable(stcsp, RefOracle, name):
    check_device(stcsp, RefOracle, stcsp.Model.from_name(name), name, masks=("hidden",))


@pytest.mark.parametrize("probe", ["until", "arr", "at", "misc", "adversarial"])
def test_device_answers_on_probes(stcsp, RefOracle, probe):
    m = stcsp.Model(text=PROBES[probe]["text"])
    check_device(stcsp, RefOracle, m, probe, masks=("default", "all", "hidden"))
    if probe == "adversarial":
        check_device(stcsp, RefOracle, m, probe + " -a", adversarial=5, masks=("default", "all", "hidden"))


@pytest.mark.parametrize("which", ["COUNTER", "COUNTDOWN", "DUPLICATES"])
def test_device_answers_on_witness_models(stcsp, RefOracle, which):
    text = {"COUNTER": COUNTER, "COUNTDOWN": COUNTDOWN, "DUPLICATES": DUPLICATES}[which]
    m = stcsp.Model(text=text)
    check_device(stcsp, RefOracle, m, which, masks=("default", "all", "hidden"))
    e, r, post, host = solved(stcsp, m)
    e.monitor([int(n == "x") for n in m.var_names])
    if which == "COUNTDOWN":  # derived by hand in tests/test_monitor.py::test_hand_derived_answers
        acc, nend, fin, fb = e.check_streams([np.array([[0], [0], [0], [1], [1]]), np.array([[0], [0], [0], [0]]), np.array([[1], [7], [1]]), np.zeros((0, 1))])
        assert acc.tolist() == [5, 3, 1, 0] and nend.tolist() == [1, 1, 1, 1] and fin.tolist() == [1, 1, 1, 1] and fb == 0


@pytest.mark.parametrize("block", range(4))
def test_device_answers_on_fuzz_models(stcsp, RefOracle, block):
    checked = 0
    for seed in [s for s in FUZZ_SEEDS if s % 4 == block]:
        text = random_model(seed)
        try:
            check_device(stcsp, RefOracle, stcsp.Model(text=text), f"seed {seed}\n{text}", masks=("default",), n_walks=5, max_len=40, seed=seed)
        except stcsp.StcspError as ex:
            assert ex.code == -2, f"seed {seed}: {ex}\n{text}"  # a domain the bitset kernels refuse
            continue
        checked += 1
    assert checked >= 45


def test_state_set_kernel_below_the_capacity(stcsp, RefOracle):
    """Five hidden values: the state-set kernel itself answers, n_end == 5 after the first step, no fallback."""
    m = stcsp.Model(text=HIDDEN % 4)
    only_x = [int(n == "x") for n in m.var_names]
    e, r, post, host = solved(stcsp, m)
    info = e.monitor(only_x)
    assert info.max_destinations == 5 and info.n_observable == 1
    streams = [np.array([[0], [1], [1]]), np.zeros((0, 1)), np.array([[2]]), np.array([[1]] * 300)]
    acc, nend, fin, fb = e.check_streams(streams)
    assert e.monitor_result.walk_kernel == 2 and fb == 0
    assert acc.tolist() == [3, 0, 0, 300] and nend.tolist() == [5, 1, 1, 5]
    o = RefOracle(m)
    ro = o.solve()
    ao = o.automaton(ro).traverse()
    y = M.Yardstick(ro, *ao.flags(), only_x)
    assert same((acc, nend, fin), y.check_all(streams)) and y.check_all(streams)[3] == 5 <= CAPACITY
    # and through the generators, under every mask
    check_device(stcsp, RefOracle, m, "hidden 5", masks=("default", "all", "hidden"))


@pytest.mark.parametrize("values", [100, 300])
def test_sets_beyond_the_capacity_fall_back_to_the_host_twin(stcsp, RefOracle, values):
    """100 hidden values stay below the capacity of 256 and are answered by the kernel; 300 must exceed it: those streams are
    finished by the host twin, and the answers still equal the yardstick's."""
    # (300 = 20 x 15 over two hidden variables: the bitset domains of the default kernels take at most 128 values each)
    m = stcsp.Model(text=HIDDEN % 99 if values == 100 else "var x:[0,1]; var h:[0,19]; var g:[0,14]; next h == h; next g == g;")
    only_x = [int(n == "x") for n in m.var_names]
    e, r, post, host = solved(stcsp, m)
    info = e.monitor(only_x)
    assert info.max_destinations == values
    streams = [np.array([[0], [1], [1], [0]]), np.zeros((0, 1)), np.array([[2], [0]]), np.array([[1]] * 50)]
    acc, nend, fin, fb = e.check_streams(streams)
    o = RefOracle(m)
    ro = o.solve()
    ao = o.automaton(ro).traverse()
    y = M.Yardstick(ro, *ao.flags(), only_x)
    yard = y.check_all(streams)
    assert yard[3] == values
    assert same((acc, nend, fin), yard)
    assert nend.tolist() == [values, 1, 1, values]
    if values > CAPACITY:
        assert fb == 2 and fb > 0  # the two streams that take a step; the empty and the rejected one never grow
    else:
        assert fb == 0
    hst = host.check_streams(streams, only_x)
    assert same(hst, yard) and hst[3] == values


def test_contract_errors(stcsp):
    m = stcsp.Model.from_name("partialorder_10")
    e = stcsp.Engine(m)
    with pytest.raises(stcsp.StcspError) as ex:  # before any solve
        e.monitor()
    assert ex.value.code == -6
    e.solve()
    with pytest.raises(stcsp.StcspError) as ex:  # before postprocess
        e.monitor()
    assert ex.value.code == -6
    e.postprocess()
    info = e.monitor("all")
    rows = np.zeros((2, info.n_observable), np.int32)
    e.check_streams([rows])
    for bad in ([0, 3, 2], [1, 2, 2], [0, -1, 2]):  # malformed offsets
        with pytest.raises(stcsp.StcspError) as ex:
            e.check_streams((rows.reshape(-1), np.array(bad, np.int64)))
        assert ex.value.code == -1
    acc, nend, fin, fb = e.check_streams([])  # n_streams = 0
    assert len(acc) == 0 and fb == 0
    e.postprocess()  # a second postprocess invalidates the structures
    with pytest.raises(stcsp.StcspError) as ex:
        e.check_streams([rows])
    assert ex.value.code == -6
    e.monitor("all")
    e.solve()  # and so does a new solve
    with pytest.raises(stcsp.StcspError) as ex:
        e.check_streams([rows])
    assert ex.value.code == -6
    t = stcsp.Engine(m, max_search_nodes=2000, batch_nodes=256)  # truncated solve
    assert t.solve().truncated == 1
    t.postprocess()
    with pytest.raises(stcsp.StcspError) as ex:
        t.monitor()
    assert ex.value.code == -6
    s = stcsp.Engine(m, flags=stcsp.F_STEPPED)  # the sharded pipeline
    with pytest.raises(stcsp.StcspError) as ex:
        s.monitor()
    assert ex.value.code == -2


# The adversary e is variable 5, as the reference's -a has it. t remembers the last d4, and a state with t == 1 offers e == 0 only: the
# adversarial pass drops it and the edges into it (the steps with d4 == 1); the root and the state with t == 0 survive.
PRUNED_BY_ADVERSARY = ("var d0:[0,0]; var d1:[0,0]; var d2:[0,0]; var d3:[0,0]; var d4:[0,1]; var e:[0,1]; var t:[0,1]; "
                       "first t == 0; next t == d4; (t eq 1) -> (e eq 0);")


def test_answers_follow_the_flags_of_a_second_postprocess(stcsp, RefOracle):
    """postprocess() again with -a: the structures must be rebuilt, and the answers are those of the new flags. Derived by hand:
    3 live states and 10 edges before (root and t == 0: d4 x e free, 4 edges each; t == 1: e == 0, 2 edges), 2 states and 4 edges
    after; a walk that sets d4 = 1 is then rejected at that step."""
    m = stcsp.Model(text=PRUNED_BY_ADVERSARY)
    e = stcsp.Engine(m)
    r = e.solve()
    e.postprocess()
    info = e.monitor("all")
    assert (info.n_states, info.n_edges) == (3, 10)
    o = RefOracle(m)
    ro = o.solve()
    plain = o.automaton(ro).traverse()
    y0 = M.Yardstick(ro, *plain.flags(), [1] * m.n_vars)
    streams, _, _ = M.make_streams(y0, m.var_bounds(), 11)
    before = e.check_streams(streams)
    assert same(before, y0.check_all(streams))
    e.postprocess(adversarial=5)
    with pytest.raises(stcsp.StcspError) as ex:
        e.check_streams(streams)
    assert ex.value.code == -6
    info = e.monitor("all")
    assert (info.n_states, info.n_edges) == (2, 4)
    after = e.check_streams(streams)
    adv = o.automaton(ro).traverse()
    assert adv.adversarial(5) == 1  # the root survives
    y1 = M.Yardstick(ro, *adv.flags(), [1] * m.n_vars)
    assert same(after, y1.check_all(streams))
    assert (len(y0.live), len(y0.edges), len(y1.live), len(y1.edges)) == (3, 10, 2, 4)
    assert not same(before, after)  # walks of the plain automaton leave the pruned one
    assert (after[0] <= before[0]).all()


def test_services_share_one_live_set_in_any_order(stcsp):
    """Monitor, quotient and generator read one live set per postprocess(), whichever of them is called first, and one call drops
    everything after new flags or a new solve. PRUNED_BY_ADVERSARY by hand: 3 live states before the adversarial pass, 2 after;
    the root and the state with t == 0 offer the same steps into the same states, so they fold: 2 classes before, 1 after."""
    m = stcsp.Model(text=PRUNED_BY_ADVERSARY)
    e = stcsp.Engine(m)
    r = e.solve()
    ranks = np.arange(4)
    streams = list(e.automaton(r).traverse().generate(12, 5, seed=3, observable="all")[0])  # walks of the plain automaton

    def answers(order, host, n_live, n_folded):
        got = {}
        for what in order:
            if what == "monitor":
                info = e.monitor("all")
                assert (info.n_states, info.root_live) == (n_live, 1)
                got[what] = e.check_streams(streams)
                assert same(got[what], host.check_streams(streams, "all")) and got[what][3] == 0
            elif what == "quotient":
                cls, n_classes, _, _ = e.quotient("all")
                hc, hn, _ = host.bisimulation("all")
                assert e.quotient_result.n_states == n_live == int((cls >= 0).sum())
                assert n_classes == hn == n_folded and np.array_equal(cls, hc)
                got[what] = cls
            else:
                info = e.generator("all", 5)
                assert (info.n_states, info.root_live) == (n_live, 1)
                got[what] = e.generate(len(ranks), 5, ranks=ranks)
                hst = host.generate(len(ranks), 5, ranks=ranks, observable="all", horizon=5)
                assert np.array_equal(got[what][0], hst[0]) and np.array_equal(got[what][1], hst[1])
        return got

    post = e.postprocess()
    before = answers(("monitor", "quotient", "generator"), e.automaton(r).import_flags(post), 3, 2)
    post = e.postprocess(adversarial=5)
    after = answers(("generator", "quotient", "monitor"), e.automaton(r).import_flags(post), 2, 1)
    assert not same(before["monitor"], after["monitor"]) and not np.array_equal(before["quotient"], after["quotient"])
    assert not np.array_equal(before["generator"][0], after["generator"][0])
    e.solve()  # a new solve: nothing of the old one answers before the next postprocess()
    for call in (lambda: e.monitor("all"), lambda: e.quotient("all"), lambda: e.generator("all", 5), lambda: e.repair_streams(streams)):
        with pytest.raises(stcsp.StcspError) as ex:
            call()
        assert ex.value.code == -6


def write_check_file(path, names, streams):
    lines = ["# " + " ".join(names)]
    for i, s in enumerate(streams):
        if i:
            lines.append("")
        lines += [" ".join(str(int(x)) for x in row) for row in s]
    path.write_text("\n".join(lines) + "\n")


@pytest.mark.parametrize("name,flags", [("juggling_b4_f5", ()), ("digitinvader3", ()), ("digitinvader3", ("-a",)), ("hidden", ())])
def test_cli_check(stcsp, tmp_path, name, flags):
    """--check prints the Python answers, one line per stream; --shards=2 --check (the host twin on the merged automaton) prints the
    same lines."""
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    text = HIDDEN % 4 if name == "hidden" else stcsp.instances.by_name(name)
    m = stcsp.Model(text=text)
    e, r, post, host = solved(stcsp, m, adversarial=5 if "-a" in flags else -1)
    mask = [int(n == "x") for n in m.var_names] if name == "hidden" else Q.default_mask(m.var_names)
    names = [n for n, k in zip(m.var_names, mask) if k]
    y = M.Yardstick(r, *Q.post_flags(post), mask)
    streams, _, _ = M.make_streams(y, m.var_bounds(), 5, n_walks=6, max_len=60)
    streams = [s for s in streams if len(s)]  # (an empty stream is written as two blank lines in a row: not exercised here)
    e.monitor(mask)
    acc, nend, fin, _ = e.check_streams(streams)
    expect = [f"{i} {acc[i]} {len(streams[i])} {nend[i]} {fin[i]}" for i in range(len(streams))]
    (tmp_path / "m.csp").write_text(text)
    write_check_file(tmp_path / "streams.txt", names, streams)
    for extra in ((), ("--shards=2",)):
        p = subprocess.run([str(exe), *flags, *extra, "--check=streams.txt", "m.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert p.returncode == 0, p.stderr
        assert p.stdout.splitlines() == expect, (extra, p.stderr)
    # columns may come in any order; an unknown name is an error
    if len(names) > 1:
        write_check_file(tmp_path / "rev.txt", names[::-1], [s[:, ::-1] for s in streams])
        p = subprocess.run([str(exe), *flags, "--check=rev.txt", "m.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert p.returncode == 0 and p.stdout.splitlines() == expect
    write_check_file(tmp_path / "bad.txt", names + ["nosuchvariable"], [])
    p = subprocess.run([str(exe), "--check=bad.txt", "m.csp"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert p.returncode != 0 and "nosuchvariable" in p.stderr
