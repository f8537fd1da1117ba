"""Constraints over 65..256 variables: the k_expand_big kernels (DR = 4 and 8, W = 1 / 2 / 4, one or two key registers) and
k_probe_big<DR, CS>, whose revisions compact a scope's open variables into lanes (dev_propagate.hpp
big_scope_prologue). Against oracle/ref_dfs.cpp like tests/test_wide_gpu.py: canonical automaton, `dom`, and the search tree
whenever neither side fails.

The models are the chain backbones of tests/test_large_block_gpu.py (few solutions per state) with one big constraint over the
chain: a conjunction, a disjunction, a `<=` count or an `if` over many flags. The reference's support search starts from the lower
bounds and refutes a value only by enumerating the whole product of the open domains, so every constraint here has a support at the
lower bounds and can only be refuted once (nearly) all of its variables are fixed: that keeps the oracle fast."""
import subprocess
import time

import numpy as np
import pytest

from conftest import finish
from test_large_block_gpu import WideBlockGen, block_words, bools, chain, token_ring
from test_wide_gpu import compare

pytestmark = pytest.mark.gpu


def big(kind: str, xs) -> str:
    """One constraint over the variables `xs` (names)."""
    h, rest = xs[0], xs[1:]
    if kind == "and":
        return f"{h} >= ({' and '.join(rest)});"
    if kind == "or":
        return f"{xs[-1]} <= ({' or '.join(xs[:-1])});"
    if kind == "sum":  # (violated only when every variable is 1)
        return f"({' + '.join(xs)}) <= {len(xs) - 1};"
    if kind == "if":  # an `if` over many flags; each branch is 1 for every tuple only when (all but one of) its flags are fixed to 1
        mid = xs[1:-1]
        return f"{xs[-1]} >= (if ({h} eq 1) then ({' and '.join(mid)}) else (({' + '.join(mid)}) ge {len(mid) - 1}));"
    raise ValueError(kind)


def family(kind: str, scope: int, n: int) -> str:
    """bools(n) (a chain of n booleans beside the counter c) and one `kind` constraint over x0 .. x_(scope-1)."""
    return bools(n) + big(kind, [f"x{i}" for i in range(scope)])


KINDS = ["and", "or", "sum", "if"]
# (kind, scope, chain length, K)
FAMILIES = [(k, s, n, 2) for k in KINDS for s, n in [(65, 70), (100, 110), (200, 210)]] + [(k, 256, 300, 1) for k in KINDS]


def check(stcsp, RefOracle, text, prefix_k=2, **opts):
    m, r, ro = compare(stcsp, RefOracle, text, prefix_k=prefix_k, **opts)
    return m, r, ro


@pytest.mark.parametrize("kind,scope,n,k", FAMILIES)
def test_big_scope_families_match_reference(stcsp, RefOracle, kind, scope, n, k):
    m, r, ro = check(stcsp, RefOracle, family(kind, scope, n), prefix_k=k)
    assert r.n_states >= 2


@pytest.mark.parametrize("kind", KINDS)
def test_big_scope_prefix_k3(stcsp, RefOracle, kind):
    m, r, ro = check(stcsp, RefOracle, family(kind, 120, 160), prefix_k=3)
    assert block_words(m, 3) == 3 * 162


@pytest.mark.parametrize("kind,scope", [("and", 70), ("sum", 100)])
def test_big_scope_dr4_and_dr8(stcsp, RefOracle, kind, scope):
    """The same constraint in a block of at most 256 words (DR = 4, forced up from 2 or 3) and of more (DR = 8)."""
    small = check(stcsp, RefOracle, family(kind, scope, 110))[0]   # N = 112: 224 words
    large = check(stcsp, RefOracle, family(kind, scope, 200))[0]   # N = 202: 404 words
    assert block_words(small) <= 256 < block_words(large)
    check(stcsp, RefOracle, chain(70) + big(kind, [f"x{i}" for i in range(70)]), prefix_k=1)  # 70 words: DR = 4 all the same


def test_big_scope_long_key(stcsp, RefOracle):
    """A key of 101 words (KR = 2): the token ring of tests/test_large_block_gpu.py and a conjunction over 90 of its flags."""
    m, r, ro = check(stcsp, RefOracle, token_ring(100) + big("and", ["b"] + [f"x{i}" for i in range(1, 90)]))
    assert r.sig_len + 1 > 64 and r.n_states >= 2


def test_big_scope_w2_and_w4(stcsp, RefOracle):
    """W = 2: a 40-value walker beside 80 chain variables and an 80-variable count. W = 4 at K = 1: a 100-value variable beside a
    70-variable disjunction."""
    xs = [f"x{i}" for i in range(80)]
    w2 = chain(80, 1, ("==",) * 9 + ("<=",)) + "var y:[0,40]; first y == 0; next y == (if (y lt 40) then (y + 1) else 0); x0 <= (y ge 20);" + big("sum", xs)
    check(stcsp, RefOracle, w2)
    w4 = (chain(70, 1, ("==",) * 9 + ("<=",)) + "var y:[0,99]; first y == 3; next y == (if (y eq 3) then 50 else (if (y eq 50) then 97 else 3)); "
          "x69 >= (y ge 50);" + big("or", xs[:70]))
    check(stcsp, RefOracle, w4, prefix_k=1)


@pytest.mark.parametrize("name", ["and100", "sum200"])
def test_big_scope_pipelines(stcsp, RefOracle, monkeypatch, name):
    """STCSP_F_STEPPED and two in-process shards, solving twice on one engine, STCSP_SMALL_POOLS with 64-node batches."""
    from test_native_sharded_gpu import run_local
    text = family("and", 100, 110) if name == "and100" else family("sum", 200, 210)
    m = stcsp.Model(text=text)
    o = RefOracle(m, time_limit_s=20.0)
    ro = o.solve()
    assert not ro.truncated
    ao, _ = finish(o, ro)
    for world in (1, 2):
        a, merged, stats, nodes, engines, g = run_local(stcsp, m, world)
        assert a.canonical() == ao.canonical()
        assert all(e.expand_variant() & 8 for e in engines)
        for e in engines:
            e.close()
    e = stcsp.Engine(m)
    for _ in range(2):
        a, _ = finish(e, e.solve())
        assert a.canonical() == ao.canonical()
    e.close()
    monkeypatch.setenv("STCSP_SMALL_POOLS", "1")
    compare(stcsp, RefOracle, text, batch_nodes=64)


def seam_blocks(m, scope, k, rng, count, max_open=10):
    """Blocks of the chain model: every chain variable fixed to a step (x_i = [i >= t]) at every point, then up to max_open of the
    big constraint's variables opened again, and now and then one flipped (a failing block)."""
    names = m.var_names
    N = m.n_vars
    bounds = m.var_bounds()
    full = [(1 << (hi - lo + 1)) - 1 for lo, hi in bounds]
    out = np.zeros((count, N * k), dtype=np.uint32)
    xi = {names.index(f"x{i}"): i for i in range(sum(1 for v in names if v.startswith("x")))}
    for b in range(count):
        t = int(rng.integers(0, len(xi) + 1))
        row = []
        for p in range(k):
            for v in range(N):
                row.append((1 << int(xi[v] >= t)) if v in xi else full[v])
        for _ in range(int(rng.integers(0, max_open + 1))):
            j = int(rng.integers(0, scope))
            row[int(rng.integers(0, k)) * N + names.index(f"x{j}")] = 3
        if rng.random() < 0.2:
            w = names.index(f"x{int(rng.integers(0, scope))}")
            row[w] = 3 - row[w] if row[w] != 3 else row[w]
        out[b] = row
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_big_scope_node_seam_equals_gac_fixpoint(stcsp, oracle_lib, FrontierModel, kind):
    """stcsp_engine_propagate through k_probe_big<DR, CS> on blocks with at most 10 of the big constraint's variables
    open: every revision is exact (no skip), and the blocks and outcomes equal the scalar GAC model's bit for bit."""
    from test_propagate_gpu import fmodel_propagate
    scope = 80
    m = stcsp.Model(text=chain(scope) + big(kind, [f"x{i}" for i in range(scope)]))
    blocks = seam_blocks(m, scope, 2, np.random.default_rng(20261016), 64)
    e = stcsp.Engine(m)
    assert e.expand_variant() & 8
    k = e.kernel_choice()  # k_expand_big<4, true, 1, 1> and k_probe_big<4, true> (79 links at two time points: CS)
    assert (k["family"], k["dom_regs"], k["compact_sweeps"], k["probe_family"], k["probe_compact_sweeps"]) == (stcsp.KF_BIG_SCOPE, 4, 1, stcsp.KP_PROBE_BIG, 1)
    got, outcome, skipped = e.propagate(blocks, 0, 0)
    want, ok = fmodel_propagate(oracle_lib, FrontierModel, m, blocks)
    assert skipped == 0
    live = ok != 0
    assert ((outcome != 0) == live).all()
    assert (got[live] == want[live]).all()
    assert 0 < int(live.sum()) < len(blocks)
    e.close()


def test_kernel_routing(stcsp):
    """expand_variant() bit 3: the big-scope kernels run exactly for the models with a constraint over more than 64 variables."""
    from test_large_block_gpu import MODELS
    for text in MODELS.values():
        e = stcsp.Engine(stcsp.Model(text=text))
        assert not e.expand_variant() & 8
        e.close()
    e = stcsp.Engine(stcsp.Model(text=family("and", 64, 70)))  # a scope of 64: the plain kernels
    assert not e.expand_variant() & 8
    e.close()
    for kind, scope, n, k in FAMILIES:
        e = stcsp.Engine(stcsp.Model(text=family(kind, scope, n), prefix_k=k))
        assert e.expand_variant() & 8
        e.close()


def test_cli_big_scope_solutions_dot(stcsp, tmp_path):
    """`stcsp -s` on a written .csp with a 100-variable constraint writes the automaton the Python path computes."""
    from canon import canon
    text = family("and", 100, 110)
    src = tmp_path / "and100.csp"
    src.write_text(text)
    m = stcsp.Model(text=text)
    e = stcsp.Engine(m)
    a, _ = finish(e, e.solve())
    e.close()
    ref = tmp_path / "python.dot"
    a.write_dot(str(ref))
    d = tmp_path / "run"
    d.mkdir()
    p = subprocess.run([str(stcsp.CSRC / "stcsp"), "-s", str(src)], cwd=d, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert canon(str(d / "solutions.dot")) == canon(str(ref))


def test_big_scope_measured(stcsp, RefOracle):
    """Solve times and skipped revisions of the families (printed: pytest -s)."""
    for kind, scope, n, k in FAMILIES[::3]:
        m = stcsp.Model(text=family(kind, scope, n), prefix_k=k)
        e = stcsp.Engine(m)
        e.solve()
        t0 = time.perf_counter()
        r = e.solve()
        dt = time.perf_counter() - t0
        c = e.counters()
        print(f"[big-scope] {kind} scope {scope} N {m.n_vars} K {k}: {dt * 1e3:.2f} ms, {r.n_states} states, "
              f"{c.search_nodes} nodes, {c.skipped_revisions} skipped of {c.wave_revisions} wavefront revisions")
        assert c.search_nodes > 0
        e.close()


class BigScopeGen(WideBlockGen):
    """WideBlockGen's models with one random constraint (`and`, `or`, `+ ... <=`, `if`) over 65..150 backbone and core variables."""

    def model(self):
        text = super().model()
        names = [ln.split()[1] for ln in text.splitlines() if ln.startswith("var w")]
        core = [v for v in self.vars if v not in names]
        flags = [f"(w{i} gt 0)" for i in range(len(names))] + [f"({v} gt 0)" for v in core]
        s = min(len(flags), 65 + self.r.below(86))
        order = sorted(range(len(flags)), key=lambda _: self.r.below(1 << 20))[:s]
        xs = [flags[i] for i in order]
        kind = self.pick(KINDS)
        if kind == "and":
            c = f"{xs[0]} >= ({' and '.join(xs[1:])});"
        elif kind == "or":
            c = f"{xs[-1]} <= ({' or '.join(xs[:-1])});"
        elif kind == "sum":
            c = f"({' + '.join(xs)}) <= {len(xs) - 1};"
        else:
            mid = xs[1:-1]
            c = f"{xs[-1]} >= (if {xs[0]} then ({' and '.join(mid)}) else (({' + '.join(mid)}) ge {len(mid) - 1}));"
        return text + c + "\n"


@pytest.mark.parametrize("block", range(2))
def test_fuzz_big_scope(stcsp, RefOracle, block):
    checked = nontrivial = 0
    for seed in range(block * 25, (block + 1) * 25):
        text = BigScopeGen(seed).model()
        m = stcsp.Model(text=text)
        o = RefOracle(m, time_limit_s=20.0)
        ro = o.solve()
        if ro.truncated:
            continue
        ao, _ = finish(o, ro)
        e = stcsp.Engine(m)
        assert e.expand_variant() & 8, f"seed {seed}"
        r = e.solve()
        a, _ = finish(e, r)
        assert a.canonical() == ao.canonical(), f"seed {seed}\n{text}"
        assert r.counters.dominance == ro.counters.dominance, f"seed {seed}\n{text}"
        if ro.counters.fails == 0 and r.counters.fails == 0:
            assert (r.n_states, r.counters.search_nodes) == (ro.n_states, ro.counters.search_nodes), f"seed {seed}\n{text}"
        checked += 1
        nontrivial += a.n_live_states > 3
        e.close()
    assert checked >= 15 and nontrivial >= 3


def test_right_nested_100_terms(stcsp, RefOracle):
    """An explicitly right-nested 100-term conjunction: an operand stack 100 deep (the front end nests `a and b and c` to the left:
    a stack of 2). The big-scope kernels take it: their LDS is asked for beyond 64 KB, within the 160 KB of a CU."""
    xs = [f"x{i}" for i in range(100)]
    e = xs[-1]
    for v in reversed(xs[1:-1]):
        e = f"({v} and {e})"
    text = bools(110) + f"x0 >= {e};"
    compare(stcsp, RefOracle, text)
