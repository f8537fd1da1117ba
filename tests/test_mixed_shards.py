"""The rows of tests/mixed_rows.py with scalar frontier models on every rank (no GPU): each row is a model the scalar model
solves, small, and one whose sharded run really moves open nodes -- what tests/test_mixed_shards_gpu.py relies on when it
puts the HIP engine on one of the ranks."""
import pytest

import mixed_rows as mr
from test_sharded import launch


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", mr.NAMES)
def test_mixed_row_on_scalar_models(stcsp, oracle_lib, RefOracle, FrontierModel, tmp_path, name, world):
    row = mr.ROW[name]
    ref = mr.reference(stcsp, RefOracle, FrontierModel, row)
    src = tmp_path / "model.csp"
    src.write_text(mr.text(row))
    r = launch(world, f"file:{src}", "fmodel", tmp_path, timeout=120, env=mr.env(row), prefix_k=mr.prefix_k(row))
    print(f"{name} world {world}: donated {r['donated']} adopted {r['adopted']} nodes {r['rank_nodes']} fails {r['rank_fails']}")
    assert r["backend"] == ["fmodel"] * world
    assert r["sha"] == ref["sha"] and r["dom"] == ref["dom"]
    if r["canonical"] is not None:
        assert r["canonical"] == ref["canonical"]
    assert sum(r["rank_nodes"]) == ref["nodes"]
    assert sum(r["rank_fails"]) == ref["fails"]
    assert sum(r["donated"]) == sum(r["adopted"])
    if world == 2:
        assert sum(r["donated"]) > 0


def test_mixed_layout_is_checked():
    from _sharded_worker import mixed_layout
    assert mixed_layout("mixed:fhf", 3) == "fhf"
    for bad, world in [("mixed:hh", 2), ("mixed:hf", 3), ("mixed:hx", 2)]:
        with pytest.raises(ValueError):
            mixed_layout(bad, world)


@pytest.mark.parametrize("name", ["long_key_plain_kl65_free4", "prefix_dr1"])
def test_shards_that_start_from_different_set_registries(stcsp, oracle_lib, RefOracle, FrontierModel, tmp_path, name):
    """The HIP engine translates constraint sets ahead of need when it is created, the scalar model does not: in a mixed run
    the ranks start from different registries. Rank 1 here does what the engine does. When rank 0 then derives in its first
    superstep the very set rank 1 already knows, the counts in the gathered table agree with rank 1's own start and differ
    from rank 0's: solve_sharded used to let each rank compare with its own start, so rank 0 went into the set exchange alone
    and the run never ended (mixed:fh of these rows on the GPU). The branch is now taken from the gathered table alone."""
    row = mr.ROW[name]
    ref = mr.reference(stcsp, RefOracle, FrontierModel, row)
    src = tmp_path / "model.csp"
    src.write_text(mr.text(row))
    r = launch(2, f"file:{src}", "fmodel", tmp_path, timeout=60, env=dict(mr.env(row), STCSP_TEST_PRETRANSLATE="1"), prefix_k=mr.prefix_k(row))
    assert r["sha"] == ref["sha"] and r["dom"] == ref["dom"]
    assert sum(r["rank_nodes"]) == ref["nodes"] and sum(r["rank_fails"]) == ref["fails"]
