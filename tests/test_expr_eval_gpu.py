"""The device's expression evaluators against the plain Python evaluator of tests/expr_ref.py: k_tabulate (dev_kernels.hpp) and
eval_program (dev_propagate.hpp) in each of its instantiations -- W = 1, W = 2 / 4 (dev_wide.hpp), interval domains
(dev_interval.hpp), big scopes (BS = true) -- on declared domains whose product is beyond what the host tabulates, so that no
satisfying tuple below was decided by cset.cpp eval_tree. Every model is solved through the C ABI and finished like solverSolve;
the distinct value rows of its live edges must be exactly `solutions()`, and a model without a solution must leave the root alone.
Four models per leg are also compared with oracle/ref_dfs.cpp (canonical automaton; the support search of the restatement is slow
on these products: the first four random models of the leg).

Which evaluator ran is read from the engine's STCSP_DEBUG line "point constraints: h host-tabulated, d device-tabulated, i
interpreted" (every pin is a host-tabulated row table, the one big constraint is the rest) and from counters.evaluations."""
import re

import pytest

import expr_ref as X
from conftest import finish
from test_expr_eval import HAND, IV_RANDOM, LONE_ROOT, RANDOM, body, edge_rows, shape_corpus

pytestmark = pytest.mark.gpu

COUNTS = re.compile(r"\[engine\] point constraints: (\d+) host-tabulated, (\d+) device-tabulated, (\d+) interpreted")
ORACLE_MODELS = 4


def device(stcsp, monkeypatch, capfd, m, tabulate, **opts):
    """Solve `m` on the device. Returns (canonical sha256, counters, (host-tabulated, device-tabulated, interpreted), engine variant,
    canonical text)."""
    monkeypatch.setenv("STCSP_DEBUG", "1")
    monkeypatch.setenv("STCSP_DEVICE_TABULATE", "1" if tabulate else "0")
    monkeypatch.setenv("STCSP_SPLIT_WIDE", "0")  # a wide conditional stays ONE constraint (else its branches may fit the host's bitmaps)
    model = stcsp.Model(text=m.text())
    capfd.readouterr()
    e = stcsp.Engine(model, **opts)  # (no except: a refusal fails the test)
    r = e.solve()
    assert not r.truncated, m.label
    counts = COUNTS.findall(capfd.readouterr().err)
    assert counts, "no `point constraints` line under STCSP_DEBUG"
    want = X.solutions(m)
    rows = edge_rows(r)
    variant = e.expand_variant()
    a, _ = finish(e, r)
    assert rows == want, f"{m.label}: {len(rows)} rows, {len(want)} solutions\n{m.text()}"
    assert a.n_live_edges == len(want), m.label
    if not want:
        assert body(a) == LONE_ROOT, m.label
    c = type(r.counters).from_buffer_copy(r.counters)  # (the result's counters, as the other suites read them; the engine owns `r`)
    out = (a.canonical_sha256(), c, tuple(map(int, counts[-1])), variant, a.canonical())
    e.close()
    return out


def against_oracle(stcsp, RefOracle, m, canonical, counters):
    o = RefOracle(stcsp.Model(text=m.text()), time_limit_s=30.0)
    ro = o.solve()
    assert not ro.truncated, m.label
    ao, _ = finish(o, ro)
    assert canonical == ao.canonical(), m.label
    assert counters.dominance == ro.counters.dominance, m.label
    if ro.counters.fails == 0 and counters.fails == 0 and counters.skipped_revisions == 0:
        assert (counters.search_nodes,) == (ro.counters.search_nodes,), m.label
    o.close()


# The models of each leg that oracle/ref_dfs.cpp solves too: the first four random ones (two per big-scope shape). Every pin is
# stated before the big constraint, so the restatement narrows the domains to the pins before its support search meets the big
# constraint, and takes well under a second per model on a CPU -- but for this one, which took it 3.5 s.
ORACLE_SKIP = {"big130 seed 6000"}


def for_oracle(m):
    return "seed" in m.label and m.label not in ORACLE_SKIP


def pins_of(m):
    return 2 * len(m.pins)


# ---------------------------------------------------------------- k_tabulate, and the same models through the W = 1 interpreter
@pytest.mark.parametrize("shape", ["odd", "mult64", "vars16"])
def test_k_tabulate_and_wavefront_interpreter(stcsp, RefOracle, monkeypatch, capfd, shape):
    oracle_left = ORACLE_MODELS
    tabulated = 0
    for m in shape_corpus(shape):
        assert 1 << 22 < m.declared_product() <= 1 << 28
        fits = X.stack_depth(m.constraints[0]) <= 32  # (deeper programs are left to the wavefront interpreter: cset.cpp build_entry)
        sha1, c1, n1, _, canon1 = device(stcsp, monkeypatch, capfd, m, True)
        assert n1 == (pins_of(m), 1, 0) if fits else n1 == (pins_of(m), 0, 1), f"{m.label}: {n1}"
        tabulated += fits
        sha0, c0, n0, _, _ = device(stcsp, monkeypatch, capfd, m, False)
        assert n0 == (pins_of(m), 0, 1), f"{m.label}: {n0}"
        assert c0.evaluations > 0 and c0.wave_revisions > 0, m.label
        assert sha1 == sha0, m.label
        if oracle_left and for_oracle(m):
            against_oracle(stcsp, RefOracle, m, canon1, c1)
            oracle_left -= 1
    assert oracle_left == 0 and tabulated >= RANDOM[shape]


# ---------------------------------------------------------------- W = 2 and W = 4
@pytest.mark.parametrize("shape", ["w2", "w4"])
def test_wide_domain_interpreter(stcsp, RefOracle, monkeypatch, capfd, shape):
    oracle_left = ORACLE_MODELS
    for m in shape_corpus(shape):
        assert m.declared_product() > 1 << 22
        width = max(hi - lo + 1 for lo, hi in m.declared.values())
        assert 32 < width <= 64 if shape == "w2" else 64 < width <= 128
        sha, c, n, _, canon = device(stcsp, monkeypatch, capfd, m, False)
        assert n == (pins_of(m), 0, 1), f"{m.label}: {n}"
        assert c.evaluations > 0 and c.wave_revisions > 0, m.label
        if oracle_left and for_oracle(m):
            against_oracle(stcsp, RefOracle, m, canon, c)
            oracle_left -= 1
    assert oracle_left == 0


# ---------------------------------------------------------------- interval domains
@pytest.mark.parametrize("form", ["exists", "def", "image"])
def test_interval_domain_interpreter(stcsp, RefOracle, monkeypatch, capfd, form):
    oracle_left = ORACLE_MODELS
    for m in X.interval_models(form, IV_RANDOM):
        assert m.declared_product() > 1 << 22
        sha, c, n, _, canon = device(stcsp, monkeypatch, capfd, m, False, flags=stcsp.F_INTERVAL_DOMAINS)
        assert n == (pins_of(m), 0, 1), f"{m.label}: {n}"
        assert c.evaluations > 0 and c.wave_revisions > 0, m.label
        if oracle_left and for_oracle(m):
            against_oracle(stcsp, RefOracle, m, canon, c)
            oracle_left -= 1
    assert oracle_left == 0


# ---------------------------------------------------------------- big scopes
@pytest.mark.parametrize("shape", ["big65", "big130"])
def test_big_scope_interpreter(stcsp, RefOracle, monkeypatch, capfd, shape):
    oracle_left = ORACLE_MODELS // 2
    for m in shape_corpus(shape):
        assert sum(a != b for a, b in m.pins.values()) == 8
        sha, c, n, variant, canon = device(stcsp, monkeypatch, capfd, m, True)
        assert variant & 8, m.label
        assert n == (pins_of(m), 0, 1), f"{m.label}: {n}"
        assert c.evaluations > 0 and c.wave_revisions > 0, m.label
        if oracle_left and for_oracle(m):
            against_oracle(stcsp, RefOracle, m, canon, c)
            oracle_left -= 1
    assert oracle_left == 0


# ---------------------------------------------------------------- scopes of 17 to 64 two-valued variables
@pytest.mark.parametrize("n", X.SCOPES)
def test_scopes_of_17_to_64_variables(stcsp, RefOracle, monkeypatch, capfd, n):
    """Products 2^17 .. 2^64 around the host's limit (2^22) and the device's (2^28). k_tabulate decodes at most 16 scope variables
    (kTabulateMaxScope), so a product in its band over 23 to 28 variables is interpreted -- the engine used to refuse such a model
    with an internal error."""
    for i, m in enumerate(X.scope_models(n)):
        assert m.declared_product() == 1 << n
        sha, c, counts, _, canon = device(stcsp, monkeypatch, capfd, m, True)
        assert counts == ((pins_of(m) + 1, 0, 0) if n <= 22 else (pins_of(m), 0, 1)), f"{m.label}: {counts}"
        if n > 22:
            assert c.evaluations > 0, m.label
        if i == 0:  # x0 <= sum: a support at the lower bounds, refuted only when everything is fixed
            against_oracle(stcsp, RefOracle, m, canon, c)


def test_conditional_nesting_of_32_is_refused_by_the_engine(stcsp):
    with pytest.raises(stcsp.StcspError) as ex:
        stcsp.Engine(stcsp.Model(text=X.too_deep_text()))
    assert ex.value.code == -2 and "conditional nesting deeper than 31" in str(ex.value)
