"""Rows for the mixed sharded runs: one rank is the HIP engine, its peers are the scalar frontier model (oracle/frontier_model.cpp),
so every transfer record and candidate record the engine writes is decoded by plain scalar code and every record it reads was
written by that code (tests/test_mixed_shards.py on the CPU, tests/test_mixed_shards_gpu.py).

A mixed row can only be a model the scalar model takes: W = 1, no interval domains, at most 32 until constraints (it keeps one
expire word) and no big scope (it enumerates whole products). Within that, one row per record stride (DR 1 / 2 / 4 / 8, which
follow N*K) and commit kernel (k_commit<DR, KR>, KR = 2 for keys of more than 64 words), with and without compacted sweeps.
The texts are the kernel matrix's (tests/kernel_matrix.py); the KR = 2 ones are widened with free booleans.

Plain Python, no GPU."""
from collections import namedtuple

import kernel_matrix as km

# redistribution knobs of the sharded worker: share from the first round on, two open nodes per rank are enough
SHARE = {"STCSP_TEST_BUDGET_ROUNDS": "1", "STCSP_TEST_SHARE": "2"}
LAYOUTS = ["mixed:hf", "mixed:fh", "mixed:fhf"]


def free_booleans(n: int) -> str:
    """n unconstrained booleans. The long-key models of the kernel matrix have a search tree of 32 nodes, one open node at a
    time: nothing to share, so neither k_donate nor k_adopt would run. A free boolean doubles the leaves below every node and
    leaves the kernel choice alone: no constraint (no item, so no change of CS), no signature word (the key stays), and N*K
    stays inside the row's DR."""
    return "".join(f"var h{i}:[0,1]; " for i in range(n))


# name, the kernel-matrix row it takes its text and switches from, free booleans appended, and the fields of
# Engine.kernel_choice() the HIP rank must report (the GPU test asserts the whole of km.choice(base) beside them)
MixedRow = namedtuple("MixedRow", "name base free expect")
ROWS = []


def mixed(base: str, free: int = 0, **expect):
    r = km.ROW[base]
    c = km.choice(r)
    assert all(c[k] == v for k, v in expect.items()), (base, expect, c)  # the stated cell is the kernel matrix's
    ROWS.append(MixedRow(base + (f"_free{free}" if free else ""), base, free, expect))


V, P, LK, LB = km.st.KF_VARIANT, km.st.KF_PREFIX, km.st.KF_LONG_KEY, km.st.KF_LARGE_BLOCK
KC = km.st.KC_COMMIT
# DR 1 / 2 / 4 with and without CS, image in LDS, LITE
for dr in (1, 2, 4):
    for cs in (0, 1):
        mixed(f"variant_dr{dr}_l1_cs{cs}_lite1", family=V, dom_regs=dr, key_regs=1, compact_sweeps=cs, lite=1, commit_family=KC, commit_key_regs=1)
# ... one general (LITE = 0) kernel and the big workgroup
mixed("variant_dr4_l0_cs1_lite0", family=V, dom_regs=4, key_regs=1, compact_sweeps=1, lite=0, commit_family=KC, commit_key_regs=1)
mixed("bigwg_dr2_cs1", family=V, dom_regs=2, key_regs=1, compact_sweeps=1, big_workgroup=1, commit_family=KC, commit_key_regs=1)
mixed("prefix_dr1", family=P, dom_regs=1, key_regs=1, compact_sweeps=0, commit_family=KC, commit_key_regs=1)
mixed("prefix_dr4", family=P, dom_regs=4, key_regs=1, compact_sweeps=0, commit_family=KC, commit_key_regs=1)
# DR 8, KR 1
mixed("block8_cs", family=LB, dom_regs=8, key_regs=1, compact_sweeps=1, commit_family=KC, commit_key_regs=1)
mixed("block8_plain_257", family=LB, dom_regs=8, key_regs=1, compact_sweeps=0, commit_family=KC, commit_key_regs=1)
# KR 2 (k_commit<4, 2> and k_commit<8, 2>), widened
mixed("long_key_plain_kl65", free=4, family=LK, dom_regs=4, key_regs=2, compact_sweeps=0, commit_family=KC, commit_key_regs=2)
mixed("long_key_cs_kl126", free=3, family=LK, dom_regs=4, key_regs=2, compact_sweeps=1, commit_family=KC, commit_key_regs=2)
mixed("block8_plain_kr2", free=4, family=LB, dom_regs=8, key_regs=2, compact_sweeps=0, commit_family=KC, commit_key_regs=2)
mixed("block8_cs_kr2", free=4, family=LB, dom_regs=8, key_regs=2, compact_sweeps=1, commit_family=KC, commit_key_regs=2)

ROW = {r.name: r for r in ROWS}
NAMES = [r.name for r in ROWS]


def text(r: MixedRow) -> str:
    return km.ROW[r.base].text() + free_booleans(r.free)


def prefix_k(r: MixedRow) -> int:
    return km.ROW[r.base].prefix_k


def env(r: MixedRow) -> dict:
    """The row's own engine switches beside the sharing knobs."""
    return dict(km.ROW[r.base].env, **SHARE)


def choice(r: MixedRow) -> dict:
    """Every field of Engine.kernel_choice(): free booleans move none of them."""
    return km.choice(km.ROW[r.base])


_reference = {}


def reference(st, RefOracle, FrontierModel, r: MixedRow) -> dict:
    """What a row's runs are compared with, computed once: the canonical automaton and `dom` of oracle/ref_dfs.cpp, and the
    search tree (nodes, fails) of the unsharded scalar model."""
    if r.name not in _reference:
        m = st.Model(text=text(r), prefix_k=prefix_k(r))
        o = RefOracle(m, time_limit_s=60.0)
        ro = o.solve()
        assert not ro.truncated
        a = o.automaton(ro).traverse().renumber()
        f = FrontierModel(m)
        rf = f.solve()
        _reference[r.name] = dict(sha=a.canonical_sha256(), canonical=a.canonical(), dom=ro.counters.dominance,
                                  nodes=rf.counters.search_nodes, fails=rf.counters.fails)
        o.close()
        f.close()
    return _reference[r.name]
