"""Blocks of 257..512 words (N*K*W, aux variables included): the DR = 8 kernels, k_expand<8, false, CS, false, false, W, KR>,
k_probe<8, ..> and k_commit<8, KR>, which hold the block in eight registers per lane. Against oracle/ref_dfs.cpp like
tests/test_wide_gpu.py: canonical automaton, `dom`, and the search tree whenever neither side fails.

The models are wide in variables, not in values: a backbone of small variables tied into a chain (few solutions per state
whatever its length) beside a small part that makes the states -- a counter, a token ring, `until` flags."""
import subprocess

import numpy as np
import pytest

from conftest import finish
from fuzz_models import Gen
from test_wide_gpu import compare

pytestmark = pytest.mark.gpu

COUNTER = "var c:[0,3]; first c == 0; next c == (if (c lt 3) then (c + 1) else 0); "


def chain(n: int, top: int = 1, ops=("<=",)) -> str:
    """n variables over [0, top] in a chain x_i op x_(i+1) (ops cycle): monotone sequences, a handful per state."""
    t = "".join(f"var x{i}:[0,{top}]; " for i in range(n))
    return t + "".join(f"x{i} {ops[i % len(ops)]} x{i + 1}; " for i in range(n - 1))


def bools(n: int) -> str:
    """About 130-250 booleans under point constraints beside a small counter that picks where the chain may switch."""
    return chain(n, 1, ("<=", "==", "==")) + COUNTER + f"x0 >= (c eq 3); x{n - 1} <= (c ne 1);"


def token_ring(m: int) -> str:
    """A signature of m words that is the ring itself (no constant words): one token travels through x_0 .. x_(m-1)
    (`x_i == next x_(i-1)`). Only x_0 is fixed by `first` (a set takes at most 64 `first` variables); it empties the others."""
    t = "".join(f"var x{i}:[0,1]; " for i in range(m)) + "var b:[0,1]; first x0 == 1; "
    t += "".join(f"x{i} <= 1 - x0; " for i in range(1, m))
    return t + f"x0 == next x{m - 1}; " + "".join(f"x{i} == next x{i - 1}; " for i in range(1, m)) + "b <= (x0 eq 1);"


def block_words(m, k: int = 2) -> int:
    w = max(hi - lo + 1 for lo, hi in m.var_bounds())
    return m.n_vars * k * (1 if w <= 32 else (2 if w <= 64 else 4))


MODELS = {
    "bools140": bools(140),                   # N = 142 (the counter and its `next` aux): 284 words
    "bools250": bools(250),                   # N = 252: 504 words
    "until130": bools(130) + "var g:[0,1]; var y:[0,1]; y == (c eq 3); g until y;",
    "ring100": token_ring(100),               # the ring is the signature: N = 201, a key of 101 words (KR = 2)
    "w2_walk": chain(70, 2, ("==",) * 9 + ("<=",)) + "var y:[0,40]; first y == 0; next y == (if (y lt 40) then (y + 1) else 0); x0 <= (y ge 20);",
    "w4_walk": chain(40, 3, ("==",) * 9 + ("<=",)) + "var y:[0,99]; first y == 3; next y == (if (y ge 96) then 1 else (y + 5)); x39 >= (y ge 50);",
}
WORDS = {"until130": 268, "bools140": 284, "bools250": 504, "ring100": 402, "w2_walk": 288, "w4_walk": 336}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_large_blocks_match_reference(stcsp, RefOracle, name):
    m, r, ro = compare(stcsp, RefOracle, MODELS[name])
    assert block_words(m) == WORDS[name] and 256 < WORDS[name] <= 512
    assert r.n_states >= 4
    if name == "ring100":
        assert r.sig_len + 1 > 64 and r.n_states == 101


def test_block_limit_is_512_words(stcsp, RefOracle):
    """Exactly 512 words solve (at K = 2 and K = 1); 513 and more are refused with STCSP_E_UNSUPPORTED naming the limit."""
    m = stcsp.Model(text=chain(256, 1, ("<=", "==")))
    assert block_words(m) == 512
    compare(stcsp, RefOracle, chain(256, 1, ("<=", "==")))
    compare(stcsp, RefOracle, chain(512, 1, ("==", "==", "<=")), prefix_k=1)
    for text, k in [(chain(257), 2), (chain(513), 1), (chain(171), 3)]:
        m = stcsp.Model(text=text, prefix_k=k)
        assert block_words(m, k) > 512
        with pytest.raises(stcsp.StcspError) as ex:
            stcsp.Engine(m)
        assert ex.value.code == -2 and "512" in str(ex.value)


@pytest.mark.parametrize("name", ["bools140", "ring100", "w2_walk", "w4_walk"])
def test_large_blocks_small_batches_and_pools(stcsp, RefOracle, monkeypatch, name):
    """Depth-first segment stack (64-node batches) and every pool growing from its smallest size, 2-KB records included."""
    monkeypatch.setenv("STCSP_SMALL_POOLS", "1")
    compare(stcsp, RefOracle, MODELS[name], batch_nodes=64)


def test_large_blocks_prefix_k3(stcsp, RefOracle):
    m, r, ro = compare(stcsp, RefOracle, bools(140), prefix_k=3)
    assert block_words(m, 3) == 426


def test_large_block_same_engine_twice(stcsp, RefOracle):
    for name in ("bools250", "ring100"):
        m = stcsp.Model(text=MODELS[name])
        o = RefOracle(m)
        ao, _ = finish(o, o.solve())
        e = stcsp.Engine(m)
        k = e.kernel_choice()  # k_expand<8, false, true, false, false, 1, KR> (more than 128 lane-revised items: CS), KR = 2 for the ring's key
        assert (k["family"], k["dom_regs"], k["compact_sweeps"], k["key_regs"], k["commit_key_regs"]) == (stcsp.KF_LARGE_BLOCK, 8, 1, 1 + (name == "ring100"), 1 + (name == "ring100"))
        for _ in range(2):
            a, _ = finish(e, e.solve())
            assert a.canonical() == ao.canonical()
        e.close()


@pytest.mark.parametrize("name", ["bools250", "ring100", "w4_walk"])
def test_large_blocks_two_shards(stcsp, RefOracle, monkeypatch, name):
    """Candidate records and transfer records of 2-KB blocks through k_commit<8, KR>, k_donate / k_adopt and LocalGroup. The
    ring's search holds one open node at a time (on the scalar model two shards donate nothing), so every model gets four free
    booleans (still at most 512 words), the shards share from the first round on and expand once per slot and round: open
    nodes really move."""
    from mixed_rows import free_booleans
    from test_native_sharded_gpu import SHARE, one_expansion_per_round, run_local
    m = stcsp.Model(text=MODELS[name] + free_booleans(4))
    assert 256 < block_words(m) <= 512
    o = RefOracle(m)
    ro = o.solve()
    ao, _ = finish(o, ro)
    one_expansion_per_round(monkeypatch)
    a, merged, stats, nodes, engines, g = run_local(stcsp, m, 2, knobs=SHARE)
    assert a.canonical() == ao.canonical()
    assert merged.counters.dominance == ro.counters.dominance
    assert sum(s["candidates_sent"] for s in stats) == sum(s["candidates_received"] for s in stats) > 0
    assert sum(s["nodes_donated"] for s in stats) == sum(s["nodes_adopted"] for s in stats) > 0


@pytest.mark.parametrize("name", ["bools140", "ring100"])
def test_cli_large_block_sharded_writes_the_same_dot(stcsp, tmp_path, name):
    exe = stcsp.CSRC / "stcsp"
    src = tmp_path / f"{name}.csp"
    src.write_text(MODELS[name])
    outs = []
    for extra in ([], ["--shards=2"]):
        d = tmp_path / ("one" if not extra else "two")
        d.mkdir()
        r = subprocess.run([str(exe), "-s", *extra, str(src)], cwd=d, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append((r.stdout.strip().split("\n")[-1].split("\t")[1:4], (d / "solutions.dot").read_bytes()))
    assert outs[0] == outs[1]
    assert len(outs[0][1]) > 0


def game(n: int) -> str:
    """The device -a / -z passes on a DR = 8 automaton: a wide backbone in front of a small game (tests/test_wide_adversarial_gpu.py)."""
    return (chain(n, 1, ("<=", "==")) + "var s:[0,1]; var a:[0,3]; var e:[0,1]; "
            "first s == 0; next s == (if (e eq 1) then (a ge 2) else s); a >= s; x0 <= e;")


def test_large_block_device_adversarial_passes_match_host(stcsp):
    from test_postproc_gpu import host_and_device
    m = stcsp.Model(text=game(140))
    assert block_words(m) > 256
    e = stcsp.Engine(m)
    r = e.solve()
    assert r.n_states >= 2
    names = m.var_names
    s, a, ev = names.index("s"), names.index("a"), names.index("e")
    for v in (a, ev, 0, s):
        host_and_device(stcsp, e, r, adv=v)
    for op, ava in [(ev, a), (a, ev), (0, a), (s, s)]:
        host_and_device(stcsp, e, r, adv2=(op, ava))
    host_and_device(stcsp, e, r, adv=a, adv2=(ev, a))


@pytest.mark.parametrize("name", ["bools250", "ring100"])
def test_large_block_node_propagation_equals_gac_fixpoint(stcsp, oracle_lib, FrontierModel, name):
    """stcsp_engine_propagate through k_probe<8, ..> against the scalar GAC model, like tests/test_propagate_gpu.py."""
    from test_propagate_gpu import fmodel_propagate, random_blocks
    m = stcsp.Model(text=MODELS[name])
    rng = np.random.default_rng(20261015)
    blocks = random_blocks(m, 2, rng, 64)
    assert blocks.shape[1] > 256
    e = stcsp.Engine(m)
    got, outcome, skipped = e.propagate(blocks, 0, 0)
    want, ok = fmodel_propagate(oracle_lib, FrontierModel, m, blocks)
    assert skipped == 0
    live = ok != 0
    assert ((outcome != 0) == live).all()
    assert (got[live] == want[live]).all()
    assert 0 < int(live.sum())


class WideBlockGen(Gen):
    """Random models of 130-250 variables: a random small model over a few variables (fuzz_models.Gen: every operator, `next`,
    `first`, `until`, arrays) beside a backbone of small variables, equal in runs that one or two other links join (at most a
    few dozen solutions per state whatever its length), tied to the small model at both ends. Expressions are one operator
    deep, so that no aux variable gets more than 32 values (one-word domains: the block is N*K words)."""

    def expr(self, depth):
        return super().expr(min(depth, 1))

    def model(self):
        core = super().model()
        small = list(self.vars)
        n = 128 + self.r.below(95)
        top = self.pick([1, 1, 2, 3])
        out = [core] + [f"var w{i} : [0, {top}];" for i in range(n)]
        links = {1 + self.r.below(n - 1): self.pick(["<=", ">=", "!=", "<="]) for _ in range(1 + self.r.below(2))}
        out += [f"w{i} {links.get(i + 1, '==')} w{i + 1};" for i in range(n - 1)]
        out.append(f"w0 {self.pick(['<=', '>=', '=='])} ({self.pick(small)} {self.pick(['gt', 'eq', 'ne'])} {self.r.below(2)});")
        if self.chance(60):
            out.append(f"w{n - 1} {self.pick(['<=', '>=', '!='])} {self.pick(small)};")
        if self.chance(40):  # a backbone word in the signature
            out.append(f"next w{self.r.below(n)} {self.pick(['==', '>=', '<='])} {self.pick(small + ['w0'])};")
        return "\n".join(out) + "\n"


@pytest.mark.parametrize("block", range(4))
def test_fuzz_large_blocks(stcsp, RefOracle, block):
    checked = nontrivial = 0
    for seed in range(block * 50, (block + 1) * 50):
        text = WideBlockGen(seed).model()
        m = stcsp.Model(text=text)
        assert 130 <= m.n_vars <= 250 and 256 < block_words(m) <= 512, f"seed {seed}: {m.n_vars} variables"
        o = RefOracle(m, time_limit_s=20.0)
        ro = o.solve()
        assert not ro.truncated, f"seed {seed}\n{text}"
        ao, _ = finish(o, ro)
        e = stcsp.Engine(m)  # no refusals
        r = e.solve()
        a, _ = finish(e, r)
        assert a.canonical() == ao.canonical(), f"seed {seed}\n{text}"
        assert r.counters.dominance == ro.counters.dominance, f"seed {seed}\n{text}"
        if ro.counters.fails == 0 and r.counters.fails == 0:
            assert (r.n_states, r.counters.search_nodes) == (ro.n_states, ro.counters.search_nodes), f"seed {seed}\n{text}"
        checked += 1
        nontrivial += a.n_live_states > 3
        e.close()
    assert checked == 50 and nontrivial >= 5
