"""The expression corpus of tests/expr_ref.py on the CPU: the plain Python evaluator, the reference-faithful oracle (ref_dfs.cpp,
its own tree walk) and the frontier model (cset.cpp eval_tree on small products, its scalar postfix interpreter on large ones)
must name the same satisfying tuples, before any device interpreter is compared with the Python evaluator
(tests/test_expr_eval_gpu.py). Also here: the conditions the corpus itself has to meet, counted with the Python evaluator alone."""
import collections
import ctypes as C

import numpy as np
import pytest

import expr_ref as X
from conftest import finish

# (leg, models): what tests/test_expr_eval_gpu.py solves on the device, a part of it here (the whole corpus takes minutes on a CPU)
RANDOM = {"odd": 24, "mult64": 12, "vars16": 12, "w2": 12, "w4": 12, "big65": 10, "big130": 6}
HAND = {"odd", "vars16", "w2", "w4", "big65"}
IV_RANDOM = 14


def shape_corpus(shape):
    return X.shape_models(shape, RANDOM[shape], hand=shape in HAND)


def random_corpus():
    out = [m for shape in RANDOM for m in X.shape_models(shape, RANDOM[shape], hand=False)]
    out += [m for form in ("exists", "def", "image") for m in X.interval_models(form, IV_RANDOM)]
    out += [m for n in X.SCOPES for m in X.scope_models(n)[1:]]
    return out


def edge_rows(result) -> set:
    """The distinct value rows of a result's edges. (A model without a temporal operator has one state: every edge is a loop on
    the root, one per satisfying tuple, and all of them are live or none exists.)"""
    n, nv = result.n_edges, result.n_vars
    if n == 0:
        return set()
    return set(map(tuple, np.ctypeslib.as_array(result.edge_values, shape=(n * nv,)).reshape(n, nv).tolist()))


# The automaton of a model without a satisfying tuple: the reference's ok / fail pass never fails the root (src/solveralgorithm.cpp:857-874),
# so what is left is the root alone, without an edge (not the EMPTY automaton of a partition without a live root).
LONE_ROOT = "S 0 0 1 S\n"


def body(a) -> str:
    """The canonical text after its two header lines (variable names, signature names)."""
    return a.canonical().split("\n", 2)[2]


def solve_rows(stcsp, cls, text, **opts):
    m = stcsp.Model(text=text)
    e = cls(m, **opts)
    r = e.solve()
    assert not r.truncated
    rows = edge_rows(r)
    a, _ = finish(e, r)
    assert a.n_live_edges == len(rows) == r.n_edges
    if not rows:
        assert body(a) == LONE_ROOT
    e.close()
    return rows


def sizes(oracle_lib, f):
    out = (C.c_longlong * 11)()
    assert oracle_lib.stcsp_fmodel_program_sizes(f._h, out, 11) == 11
    return list(out)


# ---------------------------------------------------------------- the Python evaluator itself, on values worked out by hand
def test_python_evaluator_on_hand_values():
    ev = lambda t, **v: X.evaluate(t, v, {"T": [5, -7]})
    c, v = (lambda n: ("c", n)), (lambda n: ("v", n))
    assert ev(("/", c(-7), c(2))) == (-3, True) and ev(("%", c(-7), c(2))) == (-1, True)
    assert ev(("/", c(7), c(-2))) == (-3, True) and ev(("%", c(7), c(-2))) == (1, True)
    assert ev(("/", c(5), c(0))) == (0, True) and ev(("%", c(5), c(0))) == (0, True)
    assert ev(("/", c(X.INT_MIN), c(-1))) == (0, True) and ev(("%", c(X.INT_MIN), c(-1))) == (0, True)
    assert ev(("abs", c(X.INT_MIN))) == (X.INT_MIN, True) and ev(("abs", c(-3))) == (3, True)
    assert ev(("+", c(X.INT_MAX), c(1))) == (X.INT_MIN, True) and ev(("*", c(1 << 30), c(4))) == (0, True)
    assert ev(("-", c(X.INT_MIN), c(1))) == (X.INT_MAX, True)
    assert ev(("->", c(0), c(-5))) == (1, True) and ev(("->", c(2), c(-1))) == (0, True) and ev(("->", c(-1), c(2))) == (1, True)
    assert ev(("and", c(2), c(-1))) == (-1, True) and ev(("and", c(0), c(-1))) == (0, True)
    assert ev(("or", c(2), c(-1))) == (1, True) and ev(("or", c(0), c(-1))) == (-1, True)
    assert ev(("not", c(-1))) == (0, True) and ev(("not", c(0))) == (1, True)
    assert ev(("arr", "T", c(1))) == (-7, True) and ev(("arr", "T", c(2))) == (0, False) and ev(("arr", "T", c(-1))) == (0, False)
    bad = ("arr", "T", v("x"))
    assert ev(("if", v("x"), c(4), bad), x=2) == (4, True)            # the lookup is not evaluated
    assert ev(("+", ("if", v("x"), bad, c(4)), c(1)), x=2) == (0, False)  # it is: every later arithmetic node yields 0
    assert ev(("not", ("+", bad, c(1))), x=2) == (1, False)           # ... `not` does not
    assert ev(("or", c(1), bad), x=2) == (1, True) and ev(("and", c(0), bad), x=2) == (0, True) and ev(("->", c(0), bad), x=2) == (1, True)
    events = set()
    X.evaluate(("if", v("x"), c(4), bad), {"x": 2}, {"T": [5, -7]}, events)
    assert events == {"invalid_untaken"}


def test_render_is_what_the_front_end_parses(stcsp):
    """Rendered text, parsed and printed again by the front end, evaluates to the same thing: the oracle comparison below would
    catch a precedence slip as well, this names it."""
    m = X.shape_models("odd", 3, hand=False)[1]
    model = stcsp.Model(text=m.text())
    assert model.n_vars == len(m.names) and model.var_names == m.names
    assert model.n_constraints == len(m.all_constraints())
    assert model.var_bounds() == [m.declared[v] for v in m.names]


# ---------------------------------------------------------------- corpus conditions (Python evaluator alone)
def test_corpus_conditions():
    models = random_corpus()
    seen = collections.Counter()
    nontrivial = 0
    for m in models:
        events = set()
        s = X.solutions(m, events)
        assert m.pinned_tuples() <= 2048, m.label
        whole = m.pinned_tuples() if not m.defined else None
        nontrivial += len(s) > 0 and (whole is None or len(s) < whole)
        seen.update(events)
        used = set()
        stack = list(m.constraints)
        while stack:
            t = stack.pop()
            if t[0] == "v":
                used.add(t[1])
            stack += [x for x in t[1:] if isinstance(x, tuple)]
        assert used == set(m.names), f"{m.label}: the constraint's scope is not the declared variables"
        values = {x for v in m.names if v in m.pins for x in range(m.pins[v][0], m.pins[v][1] + 1)}
        if min(lo for lo, _ in m.declared.values()) < 0:  # (the scope legs have two-valued variables over [0, 1])
            assert min(values) < 0 < max(values) and 0 in values, m.label
    print(f"\n{len(models)} random models, {nontrivial} neither empty nor whole; events {dict(seen)}")
    assert nontrivial >= 0.8 * len(models)
    for name in X.EVENTS:
        assert seen[name] >= 5, name


def test_hand_built_programs_have_their_shapes():
    labels = [m.label for m in X.hand_models(X.dom(8, -3, 3))]
    for want in [f"stack depth {d}" for d in (3, 4, 5, 31, 32, 33)] + [f"{w} code words" for w in (63, 64, 65, 127, 128, 129, 201)] + \
                [f"conditional nesting {d}" for d in (1, 2, 31)]:
        assert want in labels
    by = {m.label: m for m in X.hand_models(X.dom(8, -3, 3))}
    for d in (1, 2, 31):  # the lookup at the bottom is evaluated on some tuples and untaken on others
        events = set()
        X.solutions(by[f"conditional nesting {d}"], events)
        assert {"invalid_live", "invalid_untaken"} <= events
    events = set()
    X.solutions(by["untaken lookup under 31 conditionals"], events)
    assert "invalid_untaken" in events and "invalid_live" not in events


# ---------------------------------------------------------------- three CPU yardsticks
LEGS = sorted(RANDOM) + ["interval", "scopes"]
STRIDE = {"big65": 6, "big130": 3, "vars16": 6, "scopes": 3, "interval": 2}  # (the legs whose models take the C++ yardsticks a second each: a part of them)


def leg_models(leg):
    if leg == "interval":
        return [m for form in ("exists", "def", "image") for m in X.interval_models(form, IV_RANDOM)]
    if leg == "scopes":
        return [m for n in X.SCOPES for m in X.scope_models(n)]
    return shape_corpus(leg)


@pytest.mark.parametrize("leg", LEGS)
def test_three_cpu_yardsticks_agree(stcsp, RefOracle, FrontierModel, leg):
    """Declared domains reduced to the pins: every constraint is a table cset.cpp eval_tree fills. No model is skipped."""
    for m in leg_models(leg)[::STRIDE.get(leg, 1)]:
        want = X.solutions(m)
        text = m.host_text()
        assert solve_rows(stcsp, RefOracle, text) == want, f"{m.label}\n{text}"
        assert solve_rows(stcsp, FrontierModel, text) == want, f"{m.label}\n{text}"


@pytest.mark.parametrize("leg", ["odd", "mult64", "vars16", "big65", "big130", "scopes"])
def test_scalar_postfix_interpreter_on_the_declared_domains(stcsp, oracle_lib, FrontierModel, monkeypatch, leg):
    """The full declared domains (every variable of at most 32 values): the product is beyond what the host tabulates, so the
    frontier model interprets the compiled postfix program (no strides: no tuple bitmap), the program the device executes."""
    monkeypatch.setenv("STCSP_SPLIT_WIDE", "0")  # (a wide conditional stays one interpreted constraint)
    models = leg_models(leg)
    if leg == "scopes":
        models = [m for m in models if m.declared_product() > 1 << 22]
    for m in models[::max(2, STRIDE.get(leg, 1))]:
        model = stcsp.Model(text=m.text())
        f = FrontierModel(model)
        assert sizes(oracle_lib, f)[5] == 0, m.label
        r = f.solve()
        assert edge_rows(r) == X.solutions(m), f"{m.label}\n{m.text()}"
        f.close()


def test_conditional_nesting_of_32_is_refused(stcsp, FrontierModel):
    with pytest.raises(stcsp.StcspError) as ex:
        FrontierModel(stcsp.Model(text=X.too_deep_text()))
    assert ex.value.code == -2 and "conditional nesting deeper than 31" in str(ex.value)
