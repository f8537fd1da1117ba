"""Every kernel select_kernels() can choose, run against oracle/ref_dfs.cpp: one row of tests/kernel_matrix.py per cell. Each
test first asserts the exact Engine.kernel_choice() -- the instantiation by its template arguments, written by the statements
that assign the function pointers -- so a change of the selection that re-routes a model to a neighbouring kernel fails here
even though the neighbour computes the same automaton.

  * expansion: the assertions of `compare` of tests/test_wide_gpu.py (canonical automaton, `dom`, and the search tree when neither
    side fails) for three solves on one engine, and for one row per family and DR `compare` itself from the smallest pools in
    64-node batches;
  * probe: 64 blocks through Engine.propagate against the scalar GAC model, for the rows the node-level seam takes
    (W = 1, at most 32 until constraints): all 30 probe kernels;
  * commit: F_STEPPED and two in-process shards with every leaf sent through the exchange, one row per commit kernel."""
import numpy as np
import pytest

import kernel_matrix as km
from conftest import finish
from test_wide_gpu import compare

pytestmark = pytest.mark.gpu

FAMILIES = ["variant", "prefix", "wide", "long_key", "large_block", "until", "big_scope"]
BY_FAMILY = [pytest.param(r.name, id=f"{r.cell.family}-{r.name}") for f in FAMILIES for r in km.ROWS if r.cell.family == f]


def setenv(monkeypatch, r):
    for k in ("STCSP_LITE", "STCSP_IMG_LDS", "STCSP_BIG", "STCSP_LITE_SHAPE", "STCSP_SMALL_POOLS", "STCSP_FORCE_CANDIDATES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in r.env.items():
        monkeypatch.setenv(k, v)


def opts(r):
    return {"flags": r.flags} if r.flags else {}


def agrees(e, ro, ao):
    """One solve on `e` against the oracle's run: what `compare` of tests/test_wide_gpu.py asserts, on an engine whose kernels the
    caller has already asserted (compare builds its own engine and oracle)."""
    r = e.solve()
    a, _ = finish(e, r)
    assert a.canonical() == ao.canonical()
    assert r.counters.dominance == ro.counters.dominance
    if ro.counters.fails == 0 and r.counters.fails == 0:
        assert (r.n_states, r.counters.search_nodes) == (ro.n_states, ro.counters.search_nodes)
    return r


@pytest.mark.parametrize("name", BY_FAMILY)
def test_expansion_kernel_matches_reference(stcsp, RefOracle, monkeypatch, name):
    r = km.ROW[name]
    setenv(monkeypatch, r)
    m = stcsp.Model(text=r.text(), prefix_k=r.prefix_k)
    e = stcsp.Engine(m, **opts(r))
    assert e.kernel_choice() == km.choice(r)
    o = RefOracle(m, time_limit_s=20.0)
    ro = o.solve()
    assert not ro.truncated
    ao, _ = finish(o, ro)
    r1 = agrees(e, ro, ao)
    for _ in range(2):  # the same engine again: the table's generation starts over
        res = agrees(e, ro, ao)
        assert (res.n_states, res.counters.search_nodes, res.counters.fails) == (r1.n_states, r1.counters.search_nodes, r1.counters.fails)
    assert e.kernel_choice() == km.choice(r)
    e.close()


@pytest.mark.parametrize("name", km.SMALL_POOL_ROWS)
def test_expansion_kernel_small_pools_and_batches(stcsp, RefOracle, monkeypatch, name):
    """Records of every stride through the depth-first segment stack (64-node batches) and every pool growing from its smallest size."""
    r = km.ROW[name]
    setenv(monkeypatch, r)
    monkeypatch.setenv("STCSP_SMALL_POOLS", "1")
    e = stcsp.Engine(stcsp.Model(text=r.text(), prefix_k=r.prefix_k), batch_nodes=64, **opts(r))
    assert e.kernel_choice() == km.choice(r)
    e.close()
    compare(stcsp, RefOracle, r.text(), prefix_k=r.prefix_k, batch_nodes=64, **opts(r))


@pytest.mark.parametrize("name", [p for p in BY_FAMILY if km.seam_ok(km.ROW[p.values[0]])])
def test_probe_kernel_equals_gac_fixpoint(stcsp, oracle_lib, FrontierModel, monkeypatch, name):
    from test_propagate_gpu import fmodel_propagate
    r = km.ROW[name]
    setenv(monkeypatch, r)
    m = stcsp.Model(text=r.text(), prefix_k=r.prefix_k)
    blocks = km.seam_inputs(r, m)
    e = stcsp.Engine(m)
    assert e.kernel_choice() == km.choice(r)
    got, outcome, skipped = e.propagate(blocks, 0, 0)
    want, ok = fmodel_propagate(oracle_lib, FrontierModel, m, blocks)
    live = ok != 0
    if skipped == 0:  # every revision ran: the verdicts and the blocks of the unique GAC fixpoint
        assert ((outcome != 0) == live).all()
        assert (got[live] == want[live]).all()
    else:  # revisions over the enumeration budget were skipped (sound): a superset, never wiped out where the fixpoint is not
        assert (outcome[live] != 0).all()
        assert ((got[live] & want[live]) == want[live]).all()
    assert 0 < int(live.sum()) < len(blocks)
    e.close()


@pytest.mark.parametrize("name", km.COMMIT_ROWS)
def test_commit_kernel_stepped_and_two_shards(stcsp, RefOracle, monkeypatch, name):
    from test_native_sharded_gpu import run_local
    r = km.ROW[name]
    setenv(monkeypatch, r)
    monkeypatch.setenv("STCSP_FORCE_CANDIDATES", "1")
    m = stcsp.Model(text=r.text(), prefix_k=r.prefix_k)
    o = RefOracle(m, time_limit_s=20.0)
    ro = o.solve()
    assert not ro.truncated
    ao, _ = finish(o, ro)
    for world in (1, 2):
        # a sharded engine chooses what the unsharded one does (only the one-register shape is unsharded, and no commit row has it)
        e = stcsp.Engine(m, rank=0, world=world, flags=stcsp.F_STEPPED if world == 1 else 0)
        assert e.kernel_choice() == km.choice(r)
        e.close()
        a, merged, stats, nodes, engines, g = run_local(stcsp, m, world)
        assert all(e.kernel_choice() == km.choice(r) for e in engines)
        assert a.canonical() == ao.canonical()
        assert merged.counters.dominance == ro.counters.dominance
        assert sum(s["candidates_sent"] for s in stats) == sum(s["candidates_received"] for s in stats) > 0
        assert sum(s["nodes_donated"] for s in stats) == sum(s["nodes_adopted"] for s in stats)
        for e in engines:
            e.close()
