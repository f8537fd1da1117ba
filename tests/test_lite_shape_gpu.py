"""The one-register LITE shape kernel (k_expand<1, true, false, true, false, 1, 1, true>, engine.hip shape1): which programs it
runs, and that it computes what the generic LITE kernel and the reference compute."""
import pytest

from conftest import finish
from fuzz_models import random_model

pytestmark = pytest.mark.gpu

LITE, SHAPE, IN_LDS = 1, 2, 4  # bits of Engine.expand_variant()


def variant(stcsp, text, prefix_k=2, **opts):
    return stcsp.Engine(stcsp.Model(text=text, prefix_k=prefix_k), **opts).expand_variant()


def counters(r):  # (the ones that do not depend on timing or scheduling)
    return {f: getattr(r.counters, f) for f in ("search_nodes", "fails", "dominance", "leaves")}


@pytest.mark.parametrize("n", [10, 11, 12, 13, 14])
def test_partialorder_runs_the_shape_kernel_and_matches_golden(stcsp, golden, n):
    name = f"partialorder_{n}"
    e = stcsp.Engine(stcsp.Model.from_name(name))
    assert e.expand_variant() == LITE | SHAPE | IN_LDS
    k = e.kernel_choice()  # k_expand<1, true, false, true, false, 1, 1, true>
    assert (k["family"], k["dom_regs"], k["image_in_lds"], k["compact_sweeps"], k["lite"], k["big_workgroup"], k["one_register_shape"]) == (stcsp.KF_VARIANT, 1, 1, 0, 1, 0, 1)
    r = e.solve()
    a, _ = finish(e, r)
    g = golden[name]
    assert (a.n_live_states, a.n_live_edges, a.canonical_sha256()) == (g["states"], g["edges"], g["canonical_sha256"])
    assert (r.n_states, r.counters.search_nodes, r.counters.dominance) == (g["node"], g["search"], g["dom"])


@pytest.mark.parametrize("n", [12, 14, 15, 16])
def test_partialorder_shape_kernel_matches_generic_lite_kernel(stcsp, monkeypatch, n):
    """The same solve with the shape kernel allowed and switched off (STCSP_LITE_SHAPE=0: the generic LITE kernel)."""
    m = stcsp.Model(text=stcsp.instances.partialorder(n))
    out = []
    for switch in ("1", "0"):
        monkeypatch.setenv("STCSP_LITE_SHAPE", switch)
        e = stcsp.Engine(m)
        assert e.expand_variant() & (LITE | IN_LDS) == LITE | IN_LDS
        if switch == "0" or n <= 14:
            assert bool(e.expand_variant() & SHAPE) == (switch == "1")
        r = e.solve()
        a, _ = finish(e, r)
        out.append((a.canonical_sha256(), a.n_live_states, a.n_live_edges, r.n_states, counters(r)))
    assert out[0] == out[1]


# A program the shape kernel takes, and one change per shape fact that sends it back to the generic kernels.
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
MORE_SMALL = "".join(f"seen{i} <= seen{(i + 1) % 4} or (giveTo eq {i});\n" for i in range(4))
# 48 more point constraints of three variables, each revised at both time points: between 64 and 128 lane-revised items
MANY_SMALL = "".join(f"seen{i} <= seen{j} or (giveTo eq {c});\n" for i in range(4) for j in range(4) if i != j for c in range(4))


def test_base_model_runs_the_shape_kernel(stcsp):
    assert variant(stcsp, BASE) == LITE | SHAPE | IN_LDS
    assert variant(stcsp, BASE + MORE_SMALL) == LITE | SHAPE | IN_LDS


@pytest.mark.parametrize("case", ["until", "arity4", "more_than_64_small_items", "block_over_64_words", "wide_domain", "sharded"])
def test_shape_fact_violations_fall_back(stcsp, case):
    text, k, opts = BASE, 2, {}
    if case == "until":
        text = BASE + "seen0 until seen1;\n"
    elif case == "arity4":
        text = BASE + "seen0 + seen1 + seen2 + seen3 != 3;\n"
    elif case == "more_than_64_small_items":
        text = BASE + MANY_SMALL
    elif case == "block_over_64_words":
        k = 12  # 6 variables x 12 points: two block registers
    elif case == "wide_domain":
        text = BASE + "var wide : [0, 40];\nnext wide >= wide;\n"
    elif case == "sharded":
        opts = {"flags": stcsp.F_STEPPED}
    v = variant(stcsp, text, prefix_k=k, **opts)
    assert not v & SHAPE
    if case in ("arity4", "more_than_64_small_items", "block_over_64_words", "sharded"):
        assert v & LITE  # the same generic LITE kernels as before
    if case in ("arity4", "more_than_64_small_items", "sharded"):
        assert v & IN_LDS


@pytest.mark.parametrize("block", range(3))
def test_fuzz_shape_programs_match_reference(stcsp, RefOracle, block):
    checked = 0
    for seed in range(block * 150, (block + 1) * 150):
        text = random_model(seed)
        m = stcsp.Model(text=text)
        try:
            e = stcsp.Engine(m)
        except stcsp.StcspError as ex:
            assert ex.code == -2, f"seed {seed}: {ex}\n{text}"
            continue
        if not e.expand_variant() & SHAPE:
            continue
        o = RefOracle(m)
        ro = o.solve()
        ao, _ = finish(o, ro)
        r = e.solve()
        a, _ = finish(e, r)
        assert a.canonical() == ao.canonical(), f"seed {seed}\n{text}"
        assert r.counters.dominance == ro.counters.dominance, f"seed {seed}\n{text}"
        if ro.counters.fails == 0 and r.counters.fails == 0:
            assert (r.n_states, r.counters.search_nodes) == (ro.n_states, ro.counters.search_nodes), f"seed {seed}\n{text}"
        checked += 1
    assert checked >= 20
