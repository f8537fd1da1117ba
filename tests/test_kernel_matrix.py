"""The table of tests/kernel_matrix.py against the reference alone (no GPU): every row's model lands in the ranges that make
select_kernels() choose the row's cell, the oracle finishes it within the limit the GPU test gives it, and the oracle's own
run walks the paths a kernel can get wrong -- a bisection, a refuted node, a leaf that finds a known state. The table has one
row per compiled cell, less the cells documented as unreachable, and its rows cover every probe and commit kernel."""
import re

import numpy as np
import pytest

import kernel_matrix as km

FORCED_DR4 = ("long_key", "until", "big_scope")  # create() raises DR to 4 for these


@pytest.fixture(scope="module")
def solved(stcsp, RefOracle):
    """model text, K -> (model, oracle result): one oracle run per distinct model."""
    cache = {}

    def get(row):
        key = (row.text(), row.prefix_k)
        if key not in cache:
            m = stcsp.Model(text=key[0], prefix_k=row.prefix_k)
            ro = RefOracle(m, time_limit_s=20.0).solve()
            cache[key] = (m, ro)
        return cache[key]

    return get


def widest_scope(m) -> int:
    names = set(m.var_names)
    return max(len(set(re.findall(r"[A-Za-z_][A-Za-z_0-9]*", m.constraint_string(i))) & names) for i in range(m.n_constraints))


def test_table_is_the_enumerated_product(capsys):
    cells = km.compiled_cells()
    assert len(cells) == len(set(cells)) == 90
    assert len(km.compiled_probes()) == len(set(km.compiled_probes())) == 30
    assert len(km.compiled_commits()) == len(set(km.compiled_commits())) == 10
    assert set(km.UNREACHABLE) <= set(cells) and all(km.UNREACHABLE.values())
    rows = [r.cell for r in km.ROWS]
    assert len(rows) == len(set(rows)), "a cell has two rows"
    assert len({r.name for r in km.ROWS}) == len(km.ROWS)
    assert set(rows) == set(cells) - set(km.UNREACHABLE)
    assert len(rows) == len(cells) - len(km.UNREACHABLE)
    seam = {r.probe for r in km.ROWS if km.seam_ok(r)}
    assert seam == set(km.compiled_probes()), sorted(set(km.compiled_probes()) - seam)
    assert {r.commit for r in km.ROWS} == set(km.compiled_commits())
    assert {km.ROW[n].commit for n in km.COMMIT_ROWS} == set(km.compiled_commits()) and len(km.COMMIT_ROWS) == 10
    assert not any(km.ROW[n].flags for n in km.COMMIT_ROWS)
    # the step-down switches are the engine's own tuning switches
    assert {k for r in km.ROWS for k in r.env} <= {"STCSP_LITE", "STCSP_IMG_LDS", "STCSP_BIG", "STCSP_LITE_SHAPE"}
    # sizes at the edges: per DR one block at its upper bound and one just above the lower one; keys of 65 and 126 words
    assert {64, 65, 128, 129, 256, 257, 512} <= {r.words for r in km.ROWS}
    assert {65, 126} <= {r.key for r in km.ROWS}
    with capsys.disabled():
        print(f"\n[kernel matrix] {len(cells)} expansion cells compiled, {len(km.UNREACHABLE)} documented as unreachable, {len(rows)} rows; "
              f"{len(seam)} probe kernels and {len({km.ROW[n].commit for n in km.COMMIT_ROWS})} commit kernels covered")


@pytest.mark.parametrize("name", [r.name for r in km.ROWS])
def test_row_reaches_its_cell_and_the_oracle_walks_it(solved, name):
    r = km.ROW[name]
    c = r.cell
    m, ro = solved(r)
    # the ranges select_kernels() and create() decide by
    words = km.block_words(m, r.prefix_k, bool(r.flags))
    assert words == r.words
    assert max(km.dom_regs(words), 4 if c.family in FORCED_DR4 else 1) == c.dr
    width = max(hi - lo + 1 for lo, hi in m.var_bounds())
    if r.flags:
        assert c.form == km.INTERVALS and width > 128  # (a width no bitset kernel takes: the flag is what runs it)
    else:
        assert c.form == (1 if width <= 32 else 2 if width <= 64 else 4) and width <= 128
    key = 1 + ro.sig_len
    assert (key > 64) == (c.kr == 2) and key <= 126 and (r.key is None or key == r.key)
    assert ro.n_until_cons == r.untils and (ro.n_until_cons > 32) == (c.family == "until")
    scope = widest_scope(m)
    assert (scope > 64) == (c.family == "big_scope") == r.scope and scope <= 256
    if c.family in ("variant", "prefix"):
        assert words <= 256 and width <= 32 and key <= 64
    if c.family == "wide":
        assert c.form != 1 and key <= 64
    if c.family == "large_block":
        assert words > 256
    # the oracle's run
    assert not ro.truncated
    k = ro.counters
    assert ro.n_states >= 4
    assert ro.n_edges > ro.n_states          # some leaf finds a state that is already known
    assert k.search_nodes > k.leaves         # a bisection
    if r.need_fail:
        assert k.fails > 0                   # a refuted node
    else:                                    # a big-scope row only, with what its run has instead stated beside it (NO_FAIL)
        assert c.family == "big_scope" and r.note


@pytest.mark.parametrize("name", [r.name for r in km.ROWS if km.seam_ok(r)])
def test_seam_blocks_survive_and_fail_under_the_scalar_model(stcsp, oracle_lib, FrontierModel, solved, name):
    """The blocks the GPU test sends through Engine.propagate: under the scalar GAC model some survive and some are wiped out."""
    from test_propagate_gpu import fmodel_propagate
    r = km.ROW[name]
    m, _ = solved(r)
    blocks = km.seam_inputs(r, m)
    assert blocks.shape == (64, m.n_vars * r.prefix_k) and blocks.dtype == np.uint32
    want, ok = fmodel_propagate(oracle_lib, FrontierModel, m, blocks)
    assert 0 < int((ok != 0).sum()) < len(blocks)
