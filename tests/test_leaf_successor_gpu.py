"""The leaf path of the one-register LITE shape kernel: the time-advanced successor block finds its last point without a division
(dev_propagate.hpp successor_word; with STCSP_LEAF_SUCCESSOR_ON_DEMAND=1 it is built by expand_node after table_commit, for a leaf
that opens a new state only), and a new state is published without an L2 write-back (dev_kernels.hpp table_commit). The smallest
programs at which that code can go wrong, against the generic LITE kernel and against oracle/ref_dfs.cpp."""
import pytest

from conftest import finish

pytestmark = pytest.mark.gpu

LITE, SHAPE, IN_LDS = 1, 2, 4  # bits of Engine.expand_variant()

# The four-item partial-order program of test_lite_shape_gpu.py: six variables, every one under `first` and `next`.
BASE = """var succ : [0, 1];
var giveTo : [0, 3];
var seen0 : [0, 1];
var seen1 : [0, 1];
var seen2 : [0, 1];
var seen3 : [0, 1];
first giveTo < 1;
first seen0 == 0;
next seen0 == seen0 or (giveTo eq 0);
first seen1 == 0;
next seen1 == seen1 or (giveTo eq 1);
first seen2 == 0;
next seen2 == seen2 or (giveTo eq 2);
first seen3 == 0;
next seen3 == seen3 or (giveTo eq 3);
first succ == 0;
succ >= (seen0 and seen1 and seen2 and seen3);
next succ >= succ;
"""
# `drift` starts at -2 and has no `first` constraint: the fresh time point of a successor block gets its whole domain from the
# var_init row (bit 0 = value -2), where every other variable's fresh point is pruned by a `next` arc at once.
NEG_INIT = BASE + "var drift : [-2, 1];\nnext drift >= drift;\n"
# `first pick` as a value: a leaf captures pick's time-0 value and goes on under the constraint set translated for it, so the
# var_init row read for the successor is the NEXT set's, not the row of the set the leaf was propagated under.
SET_CHANGE = BASE + "var pick : [-1, 2];\npick >= first pick;\n"


def counters(r):  # (the ones that do not depend on timing or scheduling)
    return {f: getattr(r.counters, f) for f in ("search_nodes", "fails", "dominance", "leaves")}


def solve(engine):
    r = engine.solve()
    a, _ = finish(engine, r)
    return {"sha": a.canonical_sha256(), "states": a.n_live_states, "edges": a.n_live_edges, "n_states": r.n_states, "sets": r.n_constraint_sets,
            **counters(r)}


_REF = {}


@pytest.fixture
def reference(stcsp, RefOracle):
    """oracle/ref_dfs.cpp on (text, prefix_k): solved once per program, shared by the tests."""
    def get(text, k):
        if (text, k) not in _REF:
            _REF[text, k] = solve(RefOracle(stcsp.Model(text=text, prefix_k=k)))
        return dict(_REF[text, k])
    return get


def check_against_reference(got, ref):
    assert (got["sha"], got["states"], got["edges"], got["dominance"]) == (ref["sha"], ref["states"], ref["edges"], ref["dominance"])
    if got["fails"] == 0 and ref["fails"] == 0:  # (a failed node is where the two searches may take different turns)
        assert (got["n_states"], got["search_nodes"]) == (ref["n_states"], ref["search_nodes"])


@pytest.mark.parametrize("k", [2, 3])
def test_prefix_length_shape_kernel_generic_kernel_and_reference_agree(stcsp, monkeypatch, reference, k):
    """K = 2: every word of a successor block is either shifted or fresh. K = 3: a middle point that shifts too."""
    m = stcsp.Model(text=BASE, prefix_k=k)
    out = []
    for switch in ("1", "0"):
        monkeypatch.setenv("STCSP_LITE_SHAPE", switch)
        e = stcsp.Engine(m)
        assert e.expand_variant() == (LITE | IN_LDS | (SHAPE if switch == "1" else 0))
        out.append(solve(e))
    assert out[0] == out[1]
    check_against_reference(out[0], reference(BASE, k))


@pytest.mark.parametrize("k", [2, 3])
def test_chain_length_does_not_change_the_result(stcsp, monkeypatch, reference, k):
    """One expansion per slot: a new state's first node always goes through emit_state_node. Four: it mostly stays in registers."""
    m = stcsp.Model(text=BASE, prefix_k=k)
    out = []
    for chain in ("1", "2", "4"):
        monkeypatch.setenv("STCSP_CHAIN_SMALL", chain)
        e = stcsp.Engine(m)
        assert e.expand_variant() == LITE | SHAPE | IN_LDS
        out.append(solve(e))
    assert out[0] == out[1] == out[2]
    check_against_reference(out[0], reference(BASE, k))


@pytest.mark.parametrize("k", [2, 3])
def test_fresh_point_from_var_init_with_a_negative_lower_bound(stcsp, reference, k):
    e = stcsp.Engine(stcsp.Model(text=NEG_INIT, prefix_k=k))
    assert e.expand_variant() == LITE | SHAPE | IN_LDS
    check_against_reference(solve(e), reference(NEG_INIT, k))


@pytest.mark.parametrize("k", [2, 3])
def test_fresh_point_from_the_next_constraint_sets_row(stcsp, reference, k):
    e = stcsp.Engine(stcsp.Model(text=SET_CHANGE, prefix_k=k))
    assert e.expand_variant() == LITE | SHAPE | IN_LDS
    got = solve(e)
    assert got.pop("sets") > 1  # the leaves do change set
    check_against_reference(got, reference(SET_CHANGE, k))


def test_repeat_solve_on_one_engine_matches_golden_both_times(stcsp, golden):
    """The second solve runs under the next state-table generation, over the entries the first one left behind; partialorder_10's
    wide rounds publish from many wavefronts at once."""
    g = golden["partialorder_10"]
    e = stcsp.Engine(stcsp.Model.from_name("partialorder_10"))
    assert e.expand_variant() == LITE | SHAPE | IN_LDS
    for _ in range(2):
        r = e.solve()
        a, _ = finish(e, r)
        assert (a.n_live_states, a.n_live_edges, a.canonical_sha256()) == (g["states"], g["edges"], g["canonical_sha256"])
        assert (r.n_states, r.counters.search_nodes, r.counters.dominance) == (g["node"], g["search"], g["dom"])
