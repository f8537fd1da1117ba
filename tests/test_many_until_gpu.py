"""Models with more than 32 `until` constraints (k_expand_until / k_commit_until: up to four expire words per node, device_types.hpp)
against oracle/ref_dfs.cpp like tests/test_wide_gpu.py. The flags of tests/test_many_until.py's models expire at different
times, and g_1..g_3 are held by ordinals of 32 and above only, so nodes are refuted there (fails > 0 on both sides)."""
import subprocess

import pytest

from conftest import finish
from test_many_until import N_SIG, many_until
from test_wide_gpu import compare

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("u", [33, 63, 64, 65, 96, 97, 125 - N_SIG])
def test_many_until_match_reference(stcsp, RefOracle, u):
    m, r, ro = compare(stcsp, RefOracle, many_until(u))
    assert r.n_until_cons == u and r.n_states >= 32
    if u > 32:
        assert r.counters.fails > 0 and ro.counters.fails > 0


@pytest.mark.parametrize("u,top", [(40, 50), (70, 100)])
def test_many_until_wide_domains(stcsp, RefOracle, u, top):
    m, r, ro = compare(stcsp, RefOracle, many_until(u, top=top))
    assert max(hi - lo + 1 for lo, hi in m.var_bounds()) > 32 and r.n_states > top


@pytest.mark.parametrize("u", [40, 100])
def test_many_until_interval_domains(stcsp, RefOracle, u):
    compare(stcsp, RefOracle, many_until(u, top=40), flags=stcsp.F_INTERVAL_DOMAINS)


@pytest.mark.parametrize("u", [45, 110])
def test_many_until_block_over_256_words(stcsp, RefOracle, u):
    m, r, ro = compare(stcsp, RefOracle, many_until(u, pad=100))
    assert m.n_vars * 2 > 256 and r.counters.fails > 0


def test_many_until_prefix_k3(stcsp, RefOracle):
    compare(stcsp, RefOracle, many_until(70), prefix_k=3)


def test_many_until_small_pools_and_same_engine_twice(stcsp, RefOracle, monkeypatch):
    text = many_until(100)
    m = stcsp.Model(text=text)
    o = RefOracle(m)
    ao, _ = finish(o, o.solve())
    e = stcsp.Engine(m)
    k = e.kernel_choice()  # k_expand_until<4, true, 1, 2, ..> (100 until items and the y_b at two time points: CS) and k_commit_until<4, 2, ..>
    assert (k["family"], k["dom_regs"], k["domain_form"], k["key_regs"], k["compact_sweeps"], k["commit_family"], k["commit_key_regs"]) == \
           (stcsp.KF_UNTIL_HEAVY, 4, 1, 2, 1, stcsp.KC_COMMIT_UNTIL, 2)
    for _ in range(2):
        a, _ = finish(e, e.solve())
        assert a.canonical() == ao.canonical()
    monkeypatch.setenv("STCSP_SMALL_POOLS", "1")
    compare(stcsp, RefOracle, text, batch_nodes=64)
    compare(stcsp, RefOracle, many_until(40), batch_nodes=64)


@pytest.mark.parametrize("world,u", [(1, 70), (2, 40), (2, 124), (3, 97)])
def test_many_until_sharded(stcsp, RefOracle, monkeypatch, world, u):
    """Candidate records with expire words after the block, k_commit_until, and (SHARE) transfer records with expire words in
    their header, between in-process shards; world 1 is STCSP_F_STEPPED. Every leaf goes through the exchange, own ones too."""
    from test_native_sharded_gpu import SHARE, run_local
    monkeypatch.setenv("STCSP_FORCE_CANDIDATES", "1")
    m = stcsp.Model(text=many_until(u, free=6))
    o = RefOracle(m)
    ro = o.solve()
    ao, _ = finish(o, ro)
    for knobs in (None, SHARE):
        if knobs:  # one expansion per slot and round: the frontier grows wide enough to be shared out
            monkeypatch.setenv("STCSP_CHAIN_SMALL", "1")
            monkeypatch.setenv("STCSP_CHAIN_BIG", "1")
        a, merged, stats, nodes, engines, g = run_local(stcsp, m, world, knobs=knobs)
        assert a.canonical() == ao.canonical()
        assert merged.counters.dominance == ro.counters.dominance
        assert sum(s["candidates_sent"] for s in stats) == sum(s["candidates_received"] for s in stats) > 0
        assert sum(s["nodes_donated"] for s in stats) == sum(s["nodes_adopted"] for s in stats)
        if knobs and world > 1:
            assert sum(s["nodes_donated"] for s in stats) > 0


def test_many_until_device_postprocessing(stcsp):
    """The device passes (traverse, and -a on g0 and on g2) give what the host passes give."""
    from test_postproc_gpu import host_and_device
    m = stcsp.Model(text=many_until(70))
    e = stcsp.Engine(m)
    r = e.solve()
    host_and_device(stcsp, e, r)
    for g in ("g0", "g2"):
        host_and_device(stcsp, e, r, adv=m.var_names.index(g))


def test_many_until_cli_solutions_dot(stcsp, RefOracle, tmp_path):
    from canon import canon
    text = many_until(65)
    src = tmp_path / "many_until.csp"
    src.write_text(text)
    m = stcsp.Model(text=text)
    o = RefOracle(m)
    ao, _ = finish(o, o.solve())
    ref = tmp_path / "oracle.dot"
    ao.write_dot(str(ref))
    d = tmp_path / "run"
    d.mkdir()
    p = subprocess.run([str(stcsp.CSRC / "stcsp"), "-s", str(src)], cwd=d, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert canon(str(d / "solutions.dot")) == canon(str(ref))


def test_many_until_node_level_seam_is_refused(stcsp):
    import numpy as np
    m = stcsp.Model(text=many_until(33))
    e = stcsp.Engine(m)
    with pytest.raises(stcsp.StcspError) as ex:
        e.propagate(np.zeros((1, m.n_vars * 2), dtype=np.uint32), 0, 0)
    assert ex.value.code == -2 and "32" in str(ex.value)
