"""Interval domains (STCSP_F_INTERVAL_DOMAINS, dev_interval.hpp): every variable held as one pair of bounds per time point, like
the reference's Variable::currLB/currUB (src/variable.h:19-20), so that any width in [INT_MIN, INT_MAX] is accepted.

Yardsticks: the recorded reference results of the 26 shipped instances, and oracle/ref_dfs.cpp (RefOracle) on models wider
than the bitset kernels take -- canonical automaton and `dom` always; states and search nodes when neither side fails and the
engine skipped no revision (a revision over its budget keeps its bounds: sound, but the search tree may grow)."""
import re
import subprocess

import pytest

from canon import canon
from conftest import finish
from fuzz_models import WideGen
from test_postproc_gpu import host_and_device

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1

WIDE_IV = {
    "w129": "var x:[0,128]; var y:[0,1]; first x == 0; next x == (if (x ge 127) then 0 else (x + 1 + y)); y == (x % 3 eq 0);",
    "w256_walk": "var x:[0,255]; first x == 0; next x == (if (x lt 255) then (x + 1) else 0);",
    "w1000_counter": "var x:[0,999]; var y:[0,1]; first x == 0; next x == (if (x lt 999) then (x + 1) else 0); y == (x ge 500);",
    "negative": "var a:[-300,-100]; var b:[0,2]; first a == -300; next a == (if (a ge -105) then -300 else (a + b + 1)); b != 1;",
    "hull_next_sum": "var x:[0,100]; var y:[0,100]; var z:[0,200]; z == next (x + y); x + y <= 197; x >= 95; y >= 98;",
    "until_wide": "var x:[0,300]; var g:[0,1]; var y:[0,1]; first x == 0; next x == (if (x lt 300) then (x + 1) else x); "
                  "y == (x ge 300); g until y;",
    "two_wide": "var x:[-500,1500]; var y:[-500,1500]; var s:[0,1]; first x == 3; next x == y; y <= x + 2; y >= x - 1; y <= 40; "
                "s == ((x + y) % 2);",
}


def iv(stcsp, m, **opts):
    return stcsp.Engine(m, flags=stcsp.F_INTERVAL_DOMAINS, **opts)


def compare(stcsp, RefOracle, text, prefix_k=2, **opts):
    m = stcsp.Model(text=text, prefix_k=prefix_k)
    o = RefOracle(m, time_limit_s=30.0)
    ro = o.solve()
    assert not ro.truncated
    ao, _ = finish(o, ro)
    e = iv(stcsp, m, time_limit_s=120.0, **opts)
    assert e.kernel_choice()["domain_form"] == 0  # an interval kernel: k_expand<DR, .., kWIntervals, KR> or k_expand_until<4, false, kWIntervals, ..>
    r = e.solve()
    assert not r.truncated
    a, _ = finish(e, r)
    assert a.canonical() == ao.canonical()
    assert r.counters.dominance == ro.counters.dominance
    exact = ro.counters.fails == 0 and r.counters.fails == 0 and r.counters.skipped_revisions == 0
    if exact:
        assert (r.n_states, r.counters.search_nodes) == (ro.n_states, ro.counters.search_nodes)
    return m, r, ro, ao


def test_interval_mode_reproduces_the_reference_instances(stcsp, golden):
    """All 26 shipped instances under interval domains, with the assertions of test_engine_matches_reference_golden, the table
    size and the search tree included wherever the reference never fails -- also where the engine skipped revisions (there the
    skipped ones pruned nothing the reference prunes: every such instance keeps the reference's search tree)."""
    names = stcsp.instances.REFERENCE_EXAMPLES
    exact, gave_up = [], []
    for name in names:
        m = stcsp.Model.from_name(name)
        e = iv(stcsp, m, time_limit_s=120.0)
        r = e.solve()
        assert r.truncated == 0, name
        a, _ = finish(e, r)
        g = golden[name]
        assert (a.n_live_states, a.n_live_edges, a.canonical_sha256()) == (g["states"], g["edges"], g["canonical_sha256"]), name
        assert r.counters.dominance == g["dom"], name
        if r.counters.skipped_revisions:
            gave_up.append(name)
        if g["fail"] == 0:
            assert (r.n_states, r.counters.search_nodes) == (g["node"], g["search"]), name
            exact.append(name)
        e.close()
    print(f"\ninterval mode: exact search on {len(exact)} of {len(names)}; skipped revisions on {gave_up}")
    assert len(exact) >= 13


@pytest.mark.parametrize("name", sorted(WIDE_IV))
def test_wide_models_match_oracle(stcsp, RefOracle, name):
    m, r, ro, ao = compare(stcsp, RefOracle, WIDE_IV[name])
    assert max(hi - lo + 1 for lo, hi in m.var_bounds()) > 128
    assert ao.n_live_states > 3


@pytest.mark.parametrize("prefix_k", [1, 3])
@pytest.mark.parametrize("name", ["w256_walk", "hull_next_sum", "negative"])
def test_wide_models_prefix_k(stcsp, RefOracle, name, prefix_k):
    compare(stcsp, RefOracle, WIDE_IV[name], prefix_k=prefix_k)


@pytest.mark.parametrize("name", ["w1000_counter", "hull_next_sum"])
def test_wide_models_small_batches_and_pools(stcsp, RefOracle, monkeypatch, name):
    monkeypatch.setenv("STCSP_SMALL_POOLS", "1")
    compare(stcsp, RefOracle, WIDE_IV[name], batch_nodes=64)


@pytest.mark.parametrize("name", ["w256_walk", "hull_next_sum"])
def test_wide_models_two_hip_shards_one_gpu(stcsp, RefOracle, tmp_path, name):
    """Interval blocks through the sharded pipeline (candidate records, commit, frontier redistribution): the existing sharded
    worker, switched to interval domains by STCSP_INTERVAL_DOMAINS=1."""
    from test_sharded import launch, SHARE
    f = tmp_path / f"{name}.csp"
    f.write_text(WIDE_IV[name])
    m = stcsp.Model(text=WIDE_IV[name])
    o = RefOracle(m, time_limit_s=30.0)
    ro = o.solve()
    assert not ro.truncated
    ao, _ = finish(o, ro)
    r = launch(2, f"file:{f}", "hip", tmp_path, env=dict(SHARE, STCSP_INTERVAL_DOMAINS="1"))
    assert r["sha"] == ao.canonical_sha256() and r["dom"] == ro.counters.dominance
    assert sum(r["donated"]) == sum(r["adopted"])


# ---- `/` and `%` under next: aux variables of [INT_MIN, INT_MAX]
def c_div(a, b):
    if b == 0 or (a == INT_MIN and b == -1):
        return 0
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


class CI(int):
    """int32 arithmetic of the engine and the reference (cvalue.hpp): wrap-around, x / 0 = x % 0 = 0."""

    @staticmethod
    def w(v):
        return CI((v - INT_MIN) % 2 ** 32 + INT_MIN)

    def __add__(a, b): return CI.w(int(a) + int(b))
    def __radd__(a, b): return CI.w(int(b) + int(a))
    def __sub__(a, b): return CI.w(int(a) - int(b))
    def __rsub__(a, b): return CI.w(int(b) - int(a))
    def __mul__(a, b): return CI.w(int(a) * int(b))
    def __rmul__(a, b): return CI.w(int(b) * int(a))
    def __neg__(a): return CI.w(-int(a))
    def __truediv__(a, b): return CI(c_div(int(a), int(b)))
    def __rtruediv__(a, b): return CI(c_div(int(b), int(a)))
    def __mod__(a, b): return CI(0 if int(b) == 0 or (int(a) == INT_MIN and int(b) == -1) else int(a) - int(b) * c_div(int(a), int(b)))
    def __rmod__(a, b): return CI.__mod__(CI(b), a)


def narrowed(stcsp, text):
    """A second Model of `text` whose [INT_MIN, INT_MAX] aux variables get the exact bounds of their defining expression's image
    over the declared domains (enumerated here): an aux variable is pinned by its defining constraint, so both models have the
    same automaton."""
    m = stcsp.Model(text=text)
    names, bounds = m.var_names, m.var_bounds()
    index = {n: i for i, n in enumerate(names)}
    defs = {}
    for k in range(m.n_constraints):
        s = m.constraint_string(k)
        mm = re.fullmatch(r"(\w+) == (.*)", s)
        if mm and mm.group(1) in index and bounds[index[mm.group(1)]] == (INT_MIN, INT_MAX):
            defs[mm.group(1)] = mm.group(2)
    assert defs, "no [INT_MIN, INT_MAX] aux variable"
    image = {}

    def image_of(v):
        if v in image:
            return image[v]
        ex = defs[v]
        nx = re.fullmatch(r"next\((\w+)\)", ex)
        if nx:
            image[v] = image_of(nx.group(1)) if nx.group(1) in defs else set(range(bounds[index[nx.group(1)]][0], bounds[index[nx.group(1)]][1] + 1))
            return image[v]
        used = sorted(set(re.findall(r"[A-Za-z_]\w*", ex)), key=len, reverse=True)
        py = re.sub(r"\b\d+\b", lambda t: f"CI({t.group(0)})", ex)
        vals = {u: sorted(image_of(u)) if u in defs else list(range(bounds[index[u]][0], bounds[index[u]][1] + 1)) for u in used}
        out = set()

        def rec(i, env):
            if i == len(used):
                out.add(int(eval(py, {"CI": CI}, env)))
                return
            for x in vals[used[i]]:
                env[used[i]] = CI(x)
                rec(i + 1, env)

        rec(0, {})
        image[v] = out
        return out

    m2 = stcsp.Model(text=text)
    for v in defs:
        img = image_of(v)
        m2.problem.contents.var_lb[index[v]] = min(img)
        m2.problem.contents.var_ub[index[v]] = max(img)
    return m, m2, {v: (min(image[v]), max(image[v])) for v in defs}


DIVMOD = {
    "div_mod_negative": "var x:[-6,6]; var y:[-2,3]; var z:[-12,12]; first x == 0; next x == (if (x lt 6) then (x + 1) else -6); "
                        "z == next (x / y) + next (x % y);",
    "div_by_zero_range": "var x:[-5,7]; var y:[-1,2]; var z:[-8,8]; first x == 7; next x == (if (x gt -5) then (x - 2) else 7); "
                         "z == next (x / y); y != 1;",
    "int_min_by_minus_one": "var w:[-2,-1]; var s:[0,1]; var z:[0,4]; first s == 0; next s == 1 - s; "
                            "z == next ((-2147483648 / w) % 5); w == s - 2;",
}


@pytest.mark.parametrize("name", sorted(DIVMOD))
def test_div_mod_under_next_against_narrowed_oracle(stcsp, RefOracle, name):
    m, m2, images = narrowed(stcsp, DIVMOD[name])
    o = RefOracle(m2, time_limit_s=30.0)
    ro = o.solve()
    assert not ro.truncated
    ao, _ = finish(o, ro)
    e = iv(stcsp, m, time_limit_s=120.0)
    r = e.solve()
    assert not r.truncated
    a, _ = finish(e, r)
    assert a.canonical() == ao.canonical()
    assert ao.n_live_states >= 2


# ---- fuzz: WideGen's models with the wide span stretched past the bitset kernels
class WiderGen(WideGen):
    """WideGen (tests/fuzz_models.py) with its wide span mapped from 33..128 to 129..1,934 values."""

    @property
    def span(self):
        return self._span

    @span.setter
    def span(self, v):
        self._span = 129 + (v - 33) * 19


@pytest.mark.parametrize("block", range(2))
def test_fuzz_interval_domains(stcsp, RefOracle, block):
    checked = nontrivial = 0
    capacity = []
    for seed in range(block * 100, (block + 1) * 100):
        text = WiderGen(seed).model()
        m = stcsp.Model(text=text)
        o = RefOracle(m, time_limit_s=2.0)
        ro = o.solve()
        if ro.truncated:
            continue
        ao, _ = finish(o, ro)
        e = iv(stcsp, m, time_limit_s=60.0)
        try:
            r = e.solve()
        except stcsp.StcspError as ex:
            # a bound scan over its cap keeps the bound where the reference would have moved it: a few models then search a
            # tree deeper than the frontier's segment stack (a capacity error, never a wrong automaton)
            assert ex.code == -4 and "segment stack" in str(ex), f"seed {seed}: {ex}\n{text}"
            capacity.append(seed)
            continue
        assert not r.truncated, f"seed {seed}\n{text}"
        a, _ = finish(e, r)
        assert a.canonical() == ao.canonical(), f"seed {seed}\n{text}"
        assert r.counters.dominance == ro.counters.dominance, f"seed {seed}\n{text}"
        if ro.counters.fails == 0 and r.counters.fails == 0 and r.counters.skipped_revisions == 0:
            assert (r.n_states, r.counters.search_nodes) == (ro.n_states, ro.counters.search_nodes), f"seed {seed}\n{text}"
        checked += 1
        nontrivial += a.n_live_states > 3
        e.close()
    print(f"\nblock {block}: {checked} models checked, {nontrivial} non-trivial, capacity errors on seeds {capacity}")
    assert checked >= 60 and nontrivial >= 8 and len(capacity) <= 3


# ---- post-processing
@pytest.mark.parametrize("name", ["digitinvader6", "digitinvader7", "digitinvader8", "digitinvader9"])
def test_interval_mode_adversarial_flags_match_default_path(stcsp, name):
    m = stcsp.Model.from_name(name)
    out = []
    for flags in (0, stcsp.F_INTERVAL_DOMAINS):
        e = stcsp.Engine(m, flags=flags)
        r = e.solve()
        post = e.postprocess(adversarial=5)
        a = e.automaton(r).import_flags(post).renumber()
        out.append((post.adver1, a.canonical()))
        e.close()
    assert out[0] == out[1]


def test_interval_mode_adversarial_probe(stcsp):
    from test_engine_gpu import PROBES
    p = PROBES["adversarial"]
    m = stcsp.Model(text=p["text"])
    e = iv(stcsp, m)
    r = e.solve()
    post = e.postprocess(adversarial=5)
    assert post.adver1 == p["adver1"]
    e2 = iv(stcsp, m)
    r2 = e2.solve()
    post2 = e2.postprocess(adversarial2=(5, 6))
    assert post2.adver2 == p["adver2"]
    host_and_device(stcsp, e, r, adv=5, adv2=(5, 6))


def game(w: int) -> str:
    """tests/test_wide_adversarial_gpu.py's game: variables 5 and 6 take w values."""
    return ("var d0:[0,0]; var d1:[0,0]; var d2:[0,0]; var d3:[0,0]; var s:[0,1]; "
            f"var a:[0,{w - 1}]; var c:[0,{w - 1}]; var e:[0,1]; "
            f"first s == 0; next s == (if (e eq 1) then (a ge {w // 2}) else s); a >= s; c + s <= {w - 1};")


def test_adversarial_200_values_device_matches_host(stcsp):
    m = stcsp.Model(text=game(200))
    e = iv(stcsp, m)
    r = e.solve()
    for v in (5, 6):
        host_and_device(stcsp, e, r, adv=v)
    host_and_device(stcsp, e, r, adv2=(5, 6))
    host_and_device(stcsp, e, r, adv2=(6, 5))


OVER_CAP = ("var d0:[0,0]; var d1:[0,0]; var d2:[0,0]; var d3:[0,0]; var s:[0,1]; var a:[0,4999]; var c:[0,1]; "
            "first s == 0; next s == 1 - s; a == 17 * s + 3; c == s;")


def test_adversarial_variable_over_the_cap_is_refused(stcsp):
    m = stcsp.Model(text=OVER_CAP)
    e = iv(stcsp, m)
    e.solve()
    with pytest.raises(stcsp.StcspError) as ex:
        e.postprocess(adversarial=5)
    assert ex.value.code == -2 and "4096" in str(ex.value)
    with pytest.raises(stcsp.StcspError) as ex:
        e.postprocess(adversarial2=(5, 6))
    assert ex.value.code == -2
    post = e.postprocess(adversarial=6)  # a narrow one still runs on the device
    assert post.adver1 in (0, 1)


# ---- command line
def run_cli(stcsp, args, d):
    d.mkdir()
    r = subprocess.run([str(stcsp.CSRC / "stcsp"), *args], cwd=d, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("name", ["w1000_counter", "hull_next_sum"])
def test_cli_intervals_writes_the_oracle_automaton(stcsp, RefOracle, tmp_path, name):
    src = tmp_path / f"{name}.csp"
    src.write_text(WIDE_IV[name])
    m = stcsp.Model(text=WIDE_IV[name])
    o = RefOracle(m, time_limit_s=30.0)
    ro = o.solve()
    ao, _ = finish(o, ro)
    ref = tmp_path / "oracle.dot"
    ao.write_dot(str(ref))
    for extra in ([], ["--shards=2"]):
        d = tmp_path / ("one" if not extra else "two")
        run_cli(stcsp, ["-s", "--intervals", *extra, str(src)], d)
        assert canon(str(d / "solutions.dot")) == canon(str(ref))


def test_cli_adversarial_over_the_cap_runs_the_host_passes(stcsp, tmp_path):
    src = tmp_path / "wide.csp"
    src.write_text(OVER_CAP)
    outs = []
    for extra in ([], ["--shards=2"]):  # (--shards runs the host passes on the merged automaton)
        r = run_cli(stcsp, ["-s", "-a", "-z", "--intervals", *extra, str(src)], tmp_path / ("one" if not extra else "two"))
        outs.append(re.findall(r"adver\d: -?\d+", r.stdout))
    assert len(outs[0]) == 2 and outs[0] == outs[1]


# ---- limits
def test_interval_block_limit(stcsp):
    text = " ".join(f"var v{i}:[0,1];" for i in range(65)) + " v0 != v1;"
    m = stcsp.Model(text=text)
    stcsp.Engine(m).close()  # 65 * 2 one-word domains fit the bitset block
    with pytest.raises(stcsp.StcspError) as ex:
        iv(stcsp, m)
    assert ex.value.code == -2 and "block limit" in str(ex.value) and "256" in str(ex.value)


def test_interval_mode_refuses_the_node_seam(stcsp):
    m = stcsp.Model(text="var x:[0,3]; var y:[0,3]; x < y;")
    e = iv(stcsp, m)
    import numpy as np
    with pytest.raises(stcsp.StcspError) as ex:
        e.propagate(np.zeros((1, 8), dtype=np.uint32))
    assert ex.value.code == -2


def test_environment_switches_interval_mode_on(stcsp, monkeypatch):
    m = stcsp.Model(text="var x:[0,499]; first x == 0; next x == (if (x lt 499) then (x + 1) else 0);")
    monkeypatch.setenv("STCSP_INTERVAL_DOMAINS", "1")
    r = stcsp.Engine(m).solve()
    assert r.n_states >= 500
