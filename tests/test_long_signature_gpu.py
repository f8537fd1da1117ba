"""State keys of more than 64 words (set tag + signature of up to 125 words; the reference's signature is an unbounded
vector, src/solveralgorithm.cpp:812-837): every lane of a wavefront holds key words j and 64 + j, in the general kernels
k_expand<4, false, .., false, false, W, 2> and k_commit<4, 2>. Against oracle/ref_dfs.cpp like tests/test_wide_gpu.py.

Every `next` of the language brings an auxiliary variable (`_V == next(y)`), and that variable is the signature word; with
N*K*W <= 256 a long signature is mostly a chain `next next ... next z` over a variable of one value (constant words), and
the words that tell states apart -- a token ring, a counter, `until` flags -- are put after it, on lanes 64 and up."""
import pytest

from conftest import finish
from test_wide_gpu import compare

pytestmark = pytest.mark.gpu


def chain(c: int) -> str:
    """c constant signature words: z, next z, ..., next^c z all take the one value 0."""
    return "var z:[0,0]; z <= " + "next " * c + "z; " if c else ""


def ring(n: int, m: int = 0, lo: int = 0, hi: int = 1) -> str:
    """A signature of n words: a chain of n - m constant words, then a ring of m variables over [lo, hi] through which one
    token travels (m states, `x_i == next x_(i-1)`, every x fixed at time 0 by `first`), then a free input bit b that the
    token prunes. m = 0: a counter over [0, 5] takes the ring's place (one word, six states)."""
    t = chain(n - max(m, 1))
    t += "".join(f"var x{i}:[{lo},{hi}]; " for i in range(m)) if m else "var x0:[0,5]; "
    t += "var b:[0,1]; "
    if m:
        t += f"first x0 == {hi}; " + "".join(f"first x{i} == {lo}; " for i in range(1, m))
        t += f"x0 == next x{m - 1}; " + "".join(f"x{i} == next x{i - 1}; " for i in range(1, m))
        t += f"b <= (x0 eq {hi});"
    else:
        t += "first x0 == 0; next x0 == (if (x0 lt 5) then (x0 + 1) else 0); b <= (x0 eq 2);"
    return t


def until_model(c: int, u: int, top: int = 3) -> str:
    """c constant words, a counter over [0, top], then u `until` flags that flip together when the counter reaches `top`
    (key words 1 + n_sig + u). top > 31: a domain of more than 32 values, W = 2."""
    return (chain(c) + f"var p:[0,{top}]; var b:[0,1]; var y:[0,1]; var g:[0,1]; first p == 0; "
            f"next p == (if (p lt {top}) then (p + 1) else 0); y == (p eq {top}); b <= (p eq 1); " + "g until y; " * u)


RINGS = {
    "ring64": ring(64, 24),      # KL = 65: the ring on lanes 41..64
    "ring80": ring(80, 30),      # KL = 81: lanes 51..80
    "ring125": ring(125),        # KL = 126: the counter on lane 125
}


def key_len(res) -> int:
    return 1 + res.sig_len


@pytest.mark.parametrize("name", sorted(RINGS))
def test_long_signature_rings_match_reference(stcsp, RefOracle, name):
    m, r, ro = compare(stcsp, RefOracle, RINGS[name])
    assert key_len(r) > 64 and r.n_states >= 6


@pytest.mark.parametrize("c,u", [(35, 30), (94, 30)])
def test_until_flags_cross_lane_64(stcsp, RefOracle, c, u):
    """The flags sit at key words 1 + n_sig .. n_sig + u: across lane 64 (c = 35: words 37..66), or all beyond it (KL = 126)."""
    m, r, ro = compare(stcsp, RefOracle, until_model(c, u))
    assert key_len(r) == c + u + 2 and r.n_until_cons == u and r.n_states >= 8


@pytest.mark.parametrize("c,top", [(31, 40), (50, 63)])
def test_long_signature_wide_domains(stcsp, RefOracle, c, top):
    """dev_wide.hpp's leaf with the second key register: W = 2 (N*K*W <= 256 leaves no room for a key of more than 64 words
    at W = 4), the 32 until flags on lanes 33..64 / 52..83."""
    m, r, ro = compare(stcsp, RefOracle, until_model(c, 32, top))
    assert key_len(r) == c + 34 and max(hi - lo + 1 for lo, hi in m.var_bounds()) > 32 and r.n_states > top


def test_long_signature_prefix_k3(stcsp, RefOracle):
    compare(stcsp, RefOracle, ring(70, 12), prefix_k=3)


def test_long_signature_two_shards(stcsp, RefOracle):
    """Candidate records with more than 64 signature words, k_commit<4, 2>, and the owner shard from the two-register hash."""
    from test_native_sharded_gpu import run_local
    m = stcsp.Model(text=RINGS["ring80"])
    o = RefOracle(m)
    ro = o.solve()
    ao, _ = finish(o, ro)
    a, merged, stats, nodes, engines, g = run_local(stcsp, m, 2)
    assert a.canonical() == ao.canonical()
    assert merged.counters.dominance == ro.counters.dominance
    assert sum(s["candidates_sent"] for s in stats) == sum(s["candidates_received"] for s in stats) > 0


def test_long_signature_same_engine_twice_and_small_pools(stcsp, RefOracle, monkeypatch):
    """The table's generation starts over on the second solve; under STCSP_SMALL_POOLS the table grows and k_rehash moves
    every key (host key_hash) to where the two-register device hash looks for it."""
    text = until_model(94, 30)
    m = stcsp.Model(text=text)
    o = RefOracle(m)
    ao, _ = finish(o, o.solve())
    e = stcsp.Engine(m)
    k = e.kernel_choice()  # k_expand<4, false, false, false, false, 1, 2> and k_commit<4, 2>
    assert (k["family"], k["dom_regs"], k["domain_form"], k["key_regs"], k["compact_sweeps"], k["commit_key_regs"]) == (stcsp.KF_LONG_KEY, 4, 1, 2, 0, 2)
    for _ in range(2):
        a, _ = finish(e, e.solve())
        assert a.canonical() == ao.canonical()
    monkeypatch.setenv("STCSP_SMALL_POOLS", "1")
    compare(stcsp, RefOracle, RINGS["ring80"], batch_nodes=64)
    compare(stcsp, RefOracle, text, batch_nodes=64)


def test_key_length_limit(stcsp, RefOracle):
    """KL = 126 solves; KL = 127 is refused with STCSP_E_UNSUPPORTED and a message that names the limit."""
    compare(stcsp, RefOracle, ring(125))
    m = stcsp.Model(text=until_model(95, 30))  # (a ring of 126 would be refused for its block first: N*K = 2 * 129)
    assert m.n_vars * 2 <= 256
    with pytest.raises(stcsp.StcspError) as ex:
        stcsp.Engine(m)
    assert ex.value.code == -2 and "125" in str(ex.value) and "126" in str(ex.value)
