"""Sharded solves in which ONE rank is the HIP engine and its peers are the scalar frontier model (oracle/frontier_model.cpp).
Engine against engine, a layout error made alike by k_donate and k_adopt, or by the leaf's candidate writer and k_commit,
cancels out. Here every transfer record k_donate writes and every candidate record the leaf and the outbox write is decoded by
plain scalar C++ (the model's adopt() and commit()), and every record k_adopt and k_commit<DR, KR> read was written by that
code (its donate() and its leaf): header words 0..3, the strides, the label values, the key hash that picks the owner. The
dirty seed in word 4 is NOT pinned here: the model revises every item of a node, so its adopt() never reads the word and its
donate() writes 0; the seed is covered by the work counters of test_transfer_records_round_trip (tests/test_native_sharded_gpu.py). The result is compared with oracle/ref_dfs.cpp's automaton and with the unsharded scalar search tree.

One row of tests/mixed_rows.py per record stride and commit kernel; tests/test_mixed_shards.py proves on the CPU that each
row is small and shares work. All comparisons are equalities."""
import pytest

import mixed_rows as mr
from test_sharded import launch

pytestmark = pytest.mark.gpu

_runs = {}


def run(tmp_path_factory, name, layout):
    """One mixed run per (row, layout), shared by the tests that look at it."""
    if (name, layout) not in _runs:
        row = mr.ROW[name]
        d = tmp_path_factory.mktemp("mixed")
        src = d / "model.csp"
        src.write_text(mr.text(row))
        world = len(layout) - len("mixed:")
        r = launch(world, f"file:{src}", layout, d, timeout=120, env=mr.env(row), prefix_k=mr.prefix_k(row))
        r["h"] = r["backend"].index("hip")
        print(f"{name} {layout}: donated {r['donated']} adopted {r['adopted']} nodes {r['rank_nodes']} fails {r['rank_fails']} "
              f"candidates committed {r['candidates_committed']} of them own {r['candidates_to_self']}")
        _runs[name, layout] = r
    return _runs[name, layout]


@pytest.mark.parametrize("layout", mr.LAYOUTS)
@pytest.mark.parametrize("name", mr.NAMES)
def test_mixed_run_matches_reference(stcsp, oracle_lib, RefOracle, FrontierModel, tmp_path_factory, name, layout):
    row = mr.ROW[name]
    ref = mr.reference(stcsp, RefOracle, FrontierModel, row)
    r = run(tmp_path_factory, name, layout)
    h = r["h"]
    assert r["backend"] == [{"h": "hip", "f": "fmodel"}[c] for c in layout[len("mixed:"):]]
    assert all(s == r["strides"][0] for s in r["strides"])
    k = r["kernel_choice"][h]
    assert {f: k[f] for f in row.expect} == row.expect
    assert k == mr.choice(row)
    assert [c for i, c in enumerate(r["kernel_choice"]) if i != h] == [None] * (len(r["backend"]) - 1)
    assert r["sha"] == ref["sha"] and r["dom"] == ref["dom"]
    if r["canonical"] is not None:
        assert r["canonical"] == ref["canonical"]
    # the model adopts with seed 0 (it revises everything), the engine revises from its own seeds and from the model's seed 0:
    # both reach the unique GAC fixpoint of every node, so the search tree is the unsharded scalar one
    assert r["rank_skipped_revisions"][h] == 0
    assert sum(r["rank_nodes"]) == ref["nodes"]
    assert sum(r["rank_fails"]) == ref["fails"]
    assert sum(r["donated"]) == sum(r["adopted"])


@pytest.mark.parametrize("name", mr.NAMES)
def test_mixed_row_moves_records_both_ways(tmp_path_factory, name):
    """Over the three layouts together the HIP rank donates (k_donate writes, the model decodes), adopts (the model writes,
    k_adopt decodes) and commits candidates a model rank wrote (k_commit decodes); in every layout every rank searches. The
    HIP rank expands its whole frontier in a round where a model rank expands eight nodes, so it ends up with most of the tree
    and in some layouts every state it owns is reached from its own leaves: candidates of its peers in at least one layout."""
    runs = [run(tmp_path_factory, name, layout) for layout in mr.LAYOUTS]
    donated = [r["donated"][r["h"]] for r in runs]
    adopted = [r["adopted"][r["h"]] for r in runs]
    foreign = [r["candidates_committed"][r["h"]] - r["candidates_to_self"][r["h"]] for r in runs]
    print(f"{name}: the HIP rank donated {donated}, adopted {adopted}, committed {foreign} candidates of its peers (hf, fh, fhf)")
    assert max(donated) > 0
    assert max(adopted) > 0
    assert max(foreign) > 0
    assert all(n > 0 for r in runs for n in r["rank_nodes"])
