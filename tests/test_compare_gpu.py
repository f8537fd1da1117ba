"""Comparing two observable languages on the device (stcsp_engine_compare, dev_compare.hpp) through the C ABI: two engines in one
process, the right one's observer() dict is the request; device == host twin on the same operands, array by array, == the
yardstick of tests/compare_ref.py on the observers of the CPU oracle's automata. Run on the GPU box: pytest -m gpu."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import compare_ref as R
from test_compare import TABLE, WITNESSES, mask_of, oracle_observer, text_of

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=4)
def device_observer(stcsp, name, names):
    """(engine, observer dict): the model solved on the device and its observer under the named variables, the last one built on
    that engine."""
    m = stcsp.Model(text=text_of(stcsp, name))
    wide = any(ub - lb >= 128 for lb, ub in m.var_bounds())  # (more than 128 values: the engine holds the variables as intervals)
    e = stcsp.Engine(m, flags=stcsp.F_INTERVAL_DOMAINS if wide else 0)
    e.solve()
    e.postprocess()
    e.generator(mask_of(m, names), 0)
    return e, e.observer()


def check_device(stcsp, left, right, names, max_pairs=0):
    """Device == twin, exactly and array by array."""
    (e, ol), (_, orr) = device_observer(stcsp, left, names), device_observer(stcsp, right, names)
    dev = e.compare(orr, max_pairs)
    assert R.same(dev, stcsp.compare_observers(ol, orr)), f"{left} | {right} [{names}]: device and host twin differ"
    assert dev["table_bytes"] > 0 or dev["n_pairs"] == 0
    return e, ol, orr, dev


@pytest.mark.parametrize("left,right,names", list(TABLE))
def test_device_compare_on_the_table(stcsp, RefOracle, left, right, names):
    e, ol, orr, dev = check_device(stcsp, left, right, names)
    got = (ol["n_states"], ol["n_edges"], orr["n_states"], orr["n_edges"], dev["n_pairs"], dev["n_pair_edges"], dev["levels"], tuple(dev["witness_len"].tolist()))
    assert got == TABLE[(left, right, names)]
    for k, rows in WITNESSES.get((left, right, names), {}).items():
        assert R.witness(dev, k) == rows
    if not left.startswith("digitinvader"):  # (the CPU oracle is left out of the digitinvader rows for time)
        expect = R.product(oracle_observer(stcsp, RefOracle, left, names)[2], oracle_observer(stcsp, RefOracle, right, names)[2])
        assert R.same(dev, expect), f"{left} | {right} [{names}]: device and yardstick differ"


def test_wide_pairs_take_both_kernels(stcsp):
    """A state with more than 64 out-edges and one with more than 128, compared with themselves (the rows crafted70 | crafted130 of the
    table put them on the two sides of one pair): every pair then has 2 x 71 or 2 x 131 items, more than a wavefront has lanes."""
    for name, least in (("crafted70", 64), ("crafted130", 128)):
        e, obs = device_observer(stcsp, name, "x")
        assert np.bincount(obs["edge_src"]).max() > least
        dev = e.compare(obs)  # with itself: the pairs are its states
        assert dev["n_pairs"] == obs["n_states"] and dev["n_pair_edges"] == obs["n_edges"] and dev["witness_len"].tolist() == [-1] * 4


@pytest.mark.parametrize("left,right,names", [("dead", "U", "x,y"), ("U", "dead", "x,y"), ("dead", "dead", "x,y")])
def test_an_operand_without_states(stcsp, left, right, names):
    e, ol, orr, dev = check_device(stcsp, left, right, names)
    if left == right:
        assert (dev["n_pairs"], dev["levels"]) == (0, 0) and dev["witness_len"].tolist() == [-1] * 4
    else:
        k = 1 if left == "dead" else 0
        assert dev["n_pairs"] == 3 and dev["witness_len"][k] == 0 and dev["witness_len"][1 - k] == -1


def test_the_table_grows(stcsp, monkeypatch):
    e, ol, orr, dev = check_device(stcsp, "digitinvader3", "digitinvader4", "D0")
    monkeypatch.setenv("STCSP_COMPARE_SLOTS", "64")
    small = e.compare(orr)
    assert R.same(small, dev)
    monkeypatch.delenv("STCSP_COMPARE_SLOTS")
    assert R.same(e.compare(orr), dev)


def test_limits(stcsp, monkeypatch):
    """A byte budget that the operands do not fit, one that the table outgrows, and max_pairs = n_pairs - 1: STCSP_E_NOMEM each time,
    nothing else on the engine is disturbed, and the next call with room succeeds."""
    m = stcsp.Model(text=text_of(stcsp, "juggling_b4_f5"))
    mask = mask_of(m, "A")
    e = stcsp.Engine(m)
    e.solve()
    e.postprocess()
    e.generator(mask, 3)
    e.monitor(mask)
    obs = e.observer()
    right = device_observer(stcsp, "juggling_b4_f5_nosym", "A")[1]
    dev = e.compare(right)
    assert R.same(dev, stcsp.compare_observers(obs, right)) and dev["n_pairs"] == 129
    streams = [obs["edge_values"][:1], np.zeros((0, 1), np.int32)]

    def others():
        acc, nend, fin, _ = e.check_streams(streams)
        values, gfin = e.generate(4, 3, ranks=[0, 1, 2, 3])
        again = e.observer()
        return [acc, nend, fin, values, gfin, e.repair_streams(streams)[0]] + [again[k] for k in ("member_off", "member", "state_final", "edge_src", "edge_dst", "edge_values")]
    before = others()
    for tiny in (64, dev["table_bytes"] - 1024):
        monkeypatch.setenv("STCSP_COMPARE_BYTES", str(tiny))
        with pytest.raises(stcsp.StcspError) as ex:
            e.compare(right)
        assert ex.value.code == -4 and "STCSP_COMPARE_BYTES" in str(ex.value) and "level" in str(ex.value)
        assert all(np.array_equal(x, y) for x, y in zip(before, others()))
    monkeypatch.delenv("STCSP_COMPARE_BYTES")
    with pytest.raises(stcsp.StcspError) as ex:
        e.compare(right, dev["n_pairs"] - 1)
    assert ex.value.code == -4 and "max_pairs" in str(ex.value) and "level" in str(ex.value)
    assert all(np.array_equal(x, y) for x, y in zip(before, others()))
    assert R.same(e.compare(right, dev["n_pairs"]), dev)
    monkeypatch.setenv("STCSP_COMPARE_BYTES", str(1 << 20))  # room for everything
    assert R.same(e.compare(right), dev)


def test_two_right_operands_against_one_observer(stcsp):
    e, ol = device_observer(stcsp, "juggling_b4_f5", "A")
    e.observer()
    first, second = device_observer(stcsp, "juggling_b4_f5_nosym", "A")[1], device_observer(stcsp, "juggling_b4_f4", "A")[1]
    results = [e.compare(r) for r in (first, second, first, ol)]  # (no observer() in between)
    assert R.same(results[0], stcsp.compare_observers(ol, first)) and R.same(results[1], stcsp.compare_observers(ol, second))
    assert R.same(results[2], results[0]) and not R.same(results[0], results[1])
    assert results[3]["n_pairs"] == ol["n_states"] and results[3]["witness_len"].tolist() == [-1] * 4


def raw_compare(stcsp, e, right, max_pairs=0):
    res, keep = stcsp._observer_pack(right)
    rq, out = stcsp.CompareRequest(C.pointer(res), max_pairs), stcsp.CompareResult()
    return e._f("compare")(e._h, C.byref(rq), C.byref(out))


def test_error_paths(stcsp):
    m = stcsp.Model.from_name("partialorder_10")
    right = device_observer(stcsp, "crafted70", "x")[1]
    e = stcsp.Engine(m)
    assert raw_compare(stcsp, e, right) == -6  # before any solve
    e.solve()
    assert raw_compare(stcsp, e, right) == -6  # before postprocess
    e.postprocess()
    assert raw_compare(stcsp, e, right) == -6  # without a generator
    e.generator(None, 0)
    assert raw_compare(stcsp, e, right) == -6  # without an observer
    with pytest.raises(stcsp.StcspError) as ex:
        e.compare(right)
    assert ex.value.code == -6
    own = e.observer()
    mine = e.compare(own)
    assert (mine["n_pairs"], mine["n_pair_edges"]) == (1920, 28784) and R.same(mine, stcsp.compare_observers(own, own))
    assert raw_compare(stcsp, e, right) == -1  # one observable variable against partialorder's default mask
    for what, bad in R.malformed(own).items():
        assert raw_compare(stcsp, e, bad) == -1, what
    assert raw_compare(stcsp, e, own, -1) == -1
    rq, out = stcsp.CompareRequest(None, 0), stcsp.CompareResult()
    assert e._f("compare")(e._h, C.byref(rq), C.byref(out)) == -1
    assert R.same(e.compare(own), mine)  # the refused requests have not disturbed the observer
    with pytest.raises(stcsp.StcspError) as ex:
        e.observer(5)  # a failed observer() ends the left operand
    assert ex.value.code == -4 and raw_compare(stcsp, e, own) == -6
    e.observer()
    assert raw_compare(stcsp, e, own) == 0
    e.generator(None, 0)                     # a new generator ends it too
    assert raw_compare(stcsp, e, own) == -6
    e.observer()
    e.solve()                                # and so does a new solve
    assert raw_compare(stcsp, e, own) == -6
    s = stcsp.Engine(m, flags=stcsp.F_STEPPED)  # the sharded pipeline
    assert raw_compare(stcsp, s, own) == -2


def run_cli(stcsp, tmp_path, name, *flags, ok=True):
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    f = tmp_path / f"{name}.csp"
    f.write_text(text_of(stcsp, name))
    r = subprocess.run([str(exe), "-s", *flags, str(f)], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def lines_of(cmp):
    """The five stderr lines of --compare= for a comparison result."""
    out = [f"compare: {cmp['n_pairs']} pairs, {cmp['n_pair_edges']} edges, {cmp['levels']} levels"]
    for k, claim in enumerate(("P(left) in P(right)", "P(right) in P(left)", "F(left) in F(right)", "F(right) in F(left)")):
        w = R.witness(cmp, k)
        out.append(f"compare: {claim}: yes" if w is None else
                   f"compare: {claim}: no, {len(w)} steps:" + ";".join("".join(f" {v}" for v in row) for row in w))
    return out


def test_cli_compare(stcsp, tmp_path):
    """--observer=A --compare=FILE on the device and through the host twin (--shards=2): the five lines are the ones the twin's
    result gives, the written automaton is the one of the run without --compare, and a name FILE lacks is an error that says so."""
    sym, nosym = device_observer(stcsp, "juggling_b4_f5", "A")[1], device_observer(stcsp, "juggling_b4_f5_nosym", "A")[1]
    run_cli(stcsp, tmp_path, "juggling_b4_f5", "--observer=A", f"--binary={tmp_path / 'left.bin'}")
    expect = lines_of(stcsp.compare_observers(nosym, sym))  # (this run's model is the left operand, the file's the right one)
    assert expect[2] == "compare: P(right) in P(left): yes" and expect[1] == "compare: P(left) in P(right): no, 1 steps: 0"
    def compare_lines(r):
        return [line for line in r.stderr.splitlines() if line.startswith("compare:")]
    plain = run_cli(stcsp, tmp_path, "juggling_b4_f5_nosym", "--observer=A")
    dot = (tmp_path / "solutions.dot").read_bytes()
    assert compare_lines(plain) == []
    r = run_cli(stcsp, tmp_path, "juggling_b4_f5_nosym", "--observer=A", f"--compare={tmp_path / 'left.bin'}")
    assert compare_lines(r) == expect and (tmp_path / "solutions.dot").read_bytes() == dot
    assert r.stdout.split()[:3] == plain.stdout.split()[:3]
    r = run_cli(stcsp, tmp_path, "juggling_b4_f5_nosym", "--observer=A", "--shards=2", f"--compare={tmp_path / 'left.bin'}")
    assert compare_lines(r) == expect and (tmp_path / "solutions.dot").read_bytes() == dot
    r = run_cli(stcsp, tmp_path, "crafted5", "--observer=x", f"--compare={tmp_path / 'left.bin'}", ok=False)
    assert "no variable named 'x'" in r.stderr
    r = run_cli(stcsp, tmp_path, "juggling_b4_f5_nosym", f"--compare={tmp_path / 'left.bin'}", ok=False)
    assert "--compare needs --observer" in r.stderr
