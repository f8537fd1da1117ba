"""Fair CTL over the infinite solutions, host side (include/stcsp_host.h: stcsp_ctl_parse, stcsp_automaton_ctl): the CPU twin of
the device pass against an independent yardstick -- the plain Python path definitions of tests/ctl_ref.py, run on the automaton
of the CPU oracle. The device pass itself: tests/test_ctl_gpu.py."""
import ctypes as C
import functools
import random
from collections import Counter

import numpy as np
import pytest

import ctl_ref as T
from fuzz_models import table_by_name
from test_components import CRAFTED, TABLE, edited_flags, text_of
from test_services_fuzz import TABLES

NAMES = list(TABLE) + ["probe:arr", "probe:adversarial"]
SMALL = [n for n in NAMES if n not in ("partialorder_8", "partialorder_10")] + TABLES[:13]  # where 200 random formulas stay quick
ALONE = ["{p}", "!{p}", "{p} & {q}", "{p} | {q}", "{p} -> {q}", "EX {p}", "EF {p}", "EG {p}", "E[{p} U {q}]", "AX {p}", "AF {p}", "AG {p}",
         "A[{p} U {q}]", "true", "false"]
NESTED = ["AG EF {p}", "AG ({p} -> AF {q})", "EG EF {p}", "E[{p} U EG {q}]", "A[{p} U {q}]", "!AG EF {p}", "!AG ({p} -> AF {q})", "!EG EF {p}",
          "!E[{p} U EG {q}]", "!A[{p} U {q}]", "!EX {p}", "!EF ({p} & {q})", "AX AX {p}", "A[{p} U AG {q}]", "EG ({p} | EX {q})"]


@functools.lru_cache(maxsize=None)
def case(stcsp, RefOracle, name, adversarial=None):
    """(model, Result, automaton, (valid, final, alive), the yardstick's world graph, the oracle) of the CPU oracle's automaton; once."""
    m = stcsp.Model(text=table_by_name(name) if name.startswith("table:") else text_of(stcsp, name))
    o = RefOracle(m)
    r = o.solve()
    a = o.automaton(r).traverse()
    if adversarial is not None:
        a.adversarial(adversarial)
    flags = a.flags()
    return m, r, a, flags, T.Worlds(r, *flags), o


def atoms_for(w, names):
    """Two atoms NAME == VALUE that split the worlds as evenly as the rows allow, on two variables where there are two."""
    if not w.rows:
        return f"{names[0]} == 0", f"{names[-1]} != 0"
    cands = sorted((abs(2 * cnt - len(w.rows)), v, val) for v in range(len(names)) for val, cnt in Counter(row[v] for row in w.rows).items())
    p = cands[0]
    q = next((c for c in cands[1:] if c[1] != p[1]), cands[-1])
    return f"{names[p[1]]} == {p[2]}", f"{names[q[1]]} == {q[2]}"


def holds_on_row(f, row):
    """A temporal-free tree on one full row."""
    k = f[0]
    if k in ("true", "false"):
        return k == "true"
    if k == "cmp":
        return T.OPS[f[2]](row[f[1]], f[3][1] if f[3][0] == "int" else row[f[3][1]])
    if k == "!":
        return not holds_on_row(f[1], row)
    a, b = holds_on_row(f[1], row), holds_on_row(f[2], row)
    return (a and b) if k == "&" else (a or b) if k == "|" else (not a or b)


def temporal_free(f):
    return f[0] in ("true", "false", "cmp") or (f[0] in ("!", "&", "|", "->") and all(temporal_free(g) for g in f[1:]))


def check(stcsp, RefOracle, name, text, adversarial=None):
    """Twin == yardstick on formula `text`: the verdict arrays, and the witness with what it claims."""
    m, r, a, flags, w, _ = case(stcsp, RefOracle, name, adversarial)
    tree = T.parse(text, m.var_names)
    ref = w.result(tree, witness=True)
    res = a.ctl(text, witness=True)
    assert T.same_verdict(res, ref), f"{name}: {text}"
    assert T.witness_rows(res) == ref["witness"], f"{name}: {text}"
    plain = a.ctl(text)
    assert plain["witness"][0] == "none" and T.same_verdict(plain, ref)
    assert res["n_vars"] == m.n_vars and res["rounds"].tolist() == [0, 0, 0] and res["seconds_kernels"] == 0
    assert res["holds"] == (ref["n_initial_sat"] == ref["n_initial"]) and res["vacuous"] == (ref["n_initial"] == 0)
    kind, rows = res["witness"]
    if kind != "none":
        # a witness is a solution prefix: accepted whole under the all-variables mask
        acc, nend, _, _ = a.check_streams([rows], "all")
        assert acc.tolist() == [len(rows)] and nend.tolist() == [1]
        # ... and shows what it claims, wherever the operands are temporal-free: recomputed from the rows
        g = tree if kind == "witness" else tree[1] if tree[0] == "!" else ("EX", ("!", tree[1])) if tree[0] == "AX" else ("EF", ("!", tree[1]))
        ops = (("true",), g[1]) if g[0] in ("EX", "EF") else (g[1], g[2])
        if all(temporal_free(x) for x in ops):
            rows = rows.tolist()
            assert holds_on_row(ops[1], rows[-1])
            if g[0] == "EX":
                assert len(rows) == 2
            else:
                assert all(holds_on_row(ops[0], row) for row in rows[:-1]) and not any(holds_on_row(ops[1], row) for row in rows[:-1])
    return res, ref


@pytest.mark.parametrize("name", NAMES + TABLES)
def test_every_operator_and_the_nested_list(stcsp, RefOracle, name):
    m, r, a, flags, w, _ = case(stcsp, RefOracle, name)
    p, q = atoms_for(w, m.var_names)
    for f in ALONE + NESTED:
        check(stcsp, RefOracle, name, f.format(p=p, q=q))


def test_after_an_adversarial_pass(stcsp, RefOracle):
    m, r, a, flags, w, _ = case(stcsp, RefOracle, "probe:adversarial", 5)
    p, q = atoms_for(w, m.var_names)
    for f in ALONE + NESTED:
        check(stcsp, RefOracle, "probe:adversarial", f.format(p=p, q=q), 5)


@pytest.mark.parametrize("block", range(4))
def test_random_models(stcsp, RefOracle, block):
    for seed in range(block, 60, 4):
        m, r, a, flags, w, _ = case(stcsp, RefOracle, f"random:{seed}")
        p, q = atoms_for(w, m.var_names)
        for f in ALONE + NESTED[:6]:
            check(stcsp, RefOracle, f"random:{seed}", f.format(p=p, q=q))


@pytest.mark.parametrize("block", range(8))
def test_random_formulas(stcsp, RefOracle, block):
    """200 seeded random formulas of depth <= 4, formula i on model i modulo the list, over that model's variables and value ranges. A
    formula whose lowering is over a limit is refused by the twin (-2); at least nine in ten are answered."""
    answered = 0
    for i in range(block, 200, 8):
        name = SMALL[i % len(SMALL)]
        m = case(stcsp, RefOracle, name)[0]
        tree = T.random_formula(random.Random(1000 + i), m.n_vars, m.var_bounds(), 4)
        text = T.show(tree, m.var_names)
        assert T.parse(text, m.var_names) == tree
        try:
            check(stcsp, RefOracle, name, text)
            answered += 1
        except stcsp.StcspError as ex:
            assert ex.code == -2, text
    assert answered >= 22


# --------------------------------------------------------------------------------------------------------------------- the pins
def tally(stcsp, RefOracle, name, text):
    """(first steps the formula holds at, first steps), twin and yardstick agreeing."""
    res, ref = check(stcsp, RefOracle, name, text)
    return res["n_initial_sat"], res["n_initial"]


def test_pins_on_the_ladder(stcsp, RefOracle):
    """LADDER: m never decreases (next m >= m) and t flips; nothing else is constrained and there is no until: every state is final
    and every live step lies on an infinite solution. With prefix length 2 a step's full row also carries the NEXT values (m, t, _V0 =
    the next m, _V1 = the next t), so a step has already chosen the rung it goes to. The first steps: m == 0, t in {0, 1}, _V0 in
    0 .. 3: eight of them.
      AG EF m == 3: from any step m can still be raised to 3 later: all 8.
      EG m == 0: staying on the rung m == 0 for ever is a solution, for the first steps that have not already chosen to leave it:
                 _V0 == 0, one per t: 2 of 8.
      AF m == 3: the system can stay on any rung below 3 for ever; m == 3 is inevitable only where it is already chosen: _V0 == 3, 2 of 8.
      AG (m == 3 -> AG m == 3): m == 3 once is m == 3 for ever: all 8.
    The shortest way to m == 3 is a first step with _V0 == 3 and the step after it; the same two steps refute AG m < 3."""
    assert tally(stcsp, RefOracle, "LADDER", "AG EF m == 3") == (8, 8)
    assert tally(stcsp, RefOracle, "LADDER", "EG m == 0") == (2, 8)
    assert tally(stcsp, RefOracle, "LADDER", "AF m == 3") == (2, 8)
    assert tally(stcsp, RefOracle, "LADDER", "AG (m == 3 -> AG m == 3)") == (8, 8)
    res, _ = check(stcsp, RefOracle, "LADDER", "EF m == 3")
    kind, rows = res["witness"]
    im = case(stcsp, RefOracle, "LADDER")[0].var_names.index("m")
    assert kind == "witness" and rows[:, im].tolist() == [0, 3]
    res, _ = check(stcsp, RefOracle, "LADDER", "AG m < 3")
    assert res["witness"][0] == "counterexample" and res["witness"][1][:, im].tolist() == [0, 3]


def test_fairness_bites_on_the_ladder_with_until(stcsp, RefOracle):
    """LADDER_UNTIL adds (m lt 2) until (y eq 1): a solution must reach y == 1 once (with m < 2 until then); after that y is free.
    From a first step, a path with y == 0 for ever never fulfils the until flag, so it is final only finitely often and is NOT a
    solution, although the world graph has cycles inside y == 0 from there (t flips on a rung): EG y == 0 holds at no first step,
    where the greatest fixpoint without the Buechi condition keeps four of the six first steps with y == 0 (the two that have chosen
    the next m == 2 must show y == 1 at once). It does hold later, once the flag is fulfilled. Hence AF y == 1 holds at every first step (m, y and the next t are chosen freely there, m < 2 ... 12 of them)."""
    res, ref = check(stcsp, RefOracle, "LADDER_UNTIL", "EG y == 0")
    assert res["n_worlds"] == 58 and (res["n_initial_sat"], res["n_initial"]) == (0, 12) and res["edge_sat"].any()
    w = case(stcsp, RefOracle, "LADDER_UNTIL")[4]
    iy = case(stcsp, RefOracle, "LADDER_UNTIL")[0].var_names.index("y")
    plain = {x for x in w.all if w.rows[x][iy] == 0}  # the plain greatest fixpoint of Z = f & EX Z
    while True:
        keep = {x for x in plain if any(y in plain for y in w.succ[x])}
        if keep == plain:
            break
        plain = keep
    assert len(plain & set(w.initial)) == 4
    assert tally(stcsp, RefOracle, "LADDER_UNTIL", "AF y == 1") == (12, 12)
    assert tally(stcsp, RefOracle, "LADDER_UNTIL", "A[m < 2 U y == 1]") == (12, 12)


def test_pins_on_the_trap(stcsp, RefOracle):
    """TRAP: m never decreases, m in 0 .. 2, and t stands still exactly while m == 1; as on the ladder a step's row carries the next m
    (_V0). The first steps: m == 0, t in 0 .. 2, _V0 in 0 .. 2: nine.
      EG m == 1: the first step has m == 0: 0 of 9.
      EF EG m == 1: the system can step to m == 1 and stay, unless the first step has already chosen m == 2: _V0 in {0, 1}, 6 of 9.
      AF m == 2: it can stay at m == 0 or m == 1 for ever; inevitable only where chosen: _V0 == 2, 3 of 9.
      E[m == 0 U m == 2]: m may jump from 0 to 2, but not by way of 1: _V0 in {0, 2}, 6 of 9."""
    assert tally(stcsp, RefOracle, "TRAP", "EG m == 1") == (0, 9)
    assert tally(stcsp, RefOracle, "TRAP", "EF EG m == 1") == (6, 9)
    assert tally(stcsp, RefOracle, "TRAP", "AF m == 2") == (3, 9)
    assert tally(stcsp, RefOracle, "TRAP", "E[m == 0 U m == 2]") == (6, 9)


@pytest.mark.parametrize("name", ["FUSE", "FUSE_UNTIL"])
def test_no_infinite_solution_is_vacuous(stcsp, RefOracle, name):
    """FUSE counts c up to 3 and cannot go on: no infinite solution, 0 worlds. Every query is vacuous, `false` included."""
    for text in ("false", "true", "AG c == 0", "EF c == 3", "EG true"):
        res, _ = check(stcsp, RefOracle, name, text)
        assert (res["n_worlds"], res["n_initial"], res["n_initial_sat"]) == (0, 0, 0)
        assert res["vacuous"] and res["holds"] and not res["possible"] and res["witness"][0] == "none"


def test_pins_on_the_branching_fuse(stcsp, RefOracle):
    """FUSE_BRANCH: c counts up while b == 0 and stands still once b == 1; b never falls. c cannot pass 3, so every infinite solution
    raises b before c would have to: the prefixes that keep b == 0 too long cannot be continued and are not quantified over. The first
    steps: c == 0, b == 0, the next c is 1, the next b is 0 or 1: two. AF b == 1 holds at both and EG b == 0 at neither. With b == 1
    the system stays where it is: AG (b == 1 -> AX b == 1). c == 3 is reachable from the first step that keeps b == 0 a while, not from
    the one that raises it at once (c stops at 1): EF c == 3 at 1 of 2."""
    assert tally(stcsp, RefOracle, "FUSE_BRANCH", "AF b == 1") == (2, 2)
    assert tally(stcsp, RefOracle, "FUSE_BRANCH", "EG b == 0") == (0, 2)
    assert tally(stcsp, RefOracle, "FUSE_BRANCH", "AG (b == 1 -> AX b == 1)") == (2, 2)
    assert tally(stcsp, RefOracle, "FUSE_BRANCH", "EF c == 3") == (1, 2)


@pytest.mark.parametrize("name", ["LADDER_UNTIL", "TRAP", "juggling_b4_f5", "probe:at", TABLES[4]])
def test_identities(stcsp, RefOracle, name):
    m, r, a, flags, w, _ = case(stcsp, RefOracle, name)
    p, q = atoms_for(w, m.var_names)
    eg_true = a.ctl("EG true")
    assert np.array_equal(eg_true["edge_sat"], eg_true["edge_world"])  # every world starts a solution
    for x, y in ((f"AF {p}", f"!EG !{p}"), (f"EF {p}", f"E[true U {p}]"), (f"AG {p}", f"!EF !{p}"), (f"AX {p}", f"!EX !{p}"),
                 (f"A[{p} U {q}]", f"!E[!{q} U (!{p} & !{q})] & !EG !{q}"), (f"{p} -> {q}", f"!{p} | {q}")):
        assert np.array_equal(a.ctl(x)["edge_sat"], a.ctl(y)["edge_sat"]), (x, y)


@pytest.mark.parametrize("name", NAMES)
def test_the_worlds_are_the_live_edges_into_omega_states(stcsp, RefOracle, name):
    m, r, a, (valid, final, alive), w, _ = case(stcsp, RefOracle, name)
    comps = a.components()
    src, dst, _ = T.Q.result_arrays(r)
    omega, live = comps["state_omega"], comps["state_component"] >= 0
    expect = np.array([bool(alive[e]) and live[src[e]] and live[dst[e]] and bool(omega[dst[e]]) for e in range(r.n_edges)], dtype=np.uint8)
    res = a.ctl("true")
    assert np.array_equal(res["edge_world"], expect) and res["n_worlds"] == int(expect.sum()) == len(w.eid)
    assert res["n_initial"] == int(expect[src == 0].sum())


def test_edited_flags_on_the_ladder(stcsp, RefOracle):
    """The flags are the automaton's current ones: with the top rung's two internal edges cut (test_components: its states become a
    dead end) m == 3 lies on no infinite solution any more."""
    m = stcsp.Model(text=CRAFTED["LADDER"])
    o = RefOracle(m)
    r = o.solve()
    a = o.automaton(r).traverse()
    valid, final, alive = a.flags()
    before = a.ctl("EF m == 3")
    assert before["holds"]
    src, dst, val = T.Q.result_arrays(r)
    im = m.var_names.index("m")
    top = {int(dst[e]) for e in range(r.n_edges) if val[e][im] == 3}
    alive2 = bytes(0 if int(src[e]) in top and int(dst[e]) in top else alive[e] for e in range(r.n_edges))
    flags = edited_flags(a, valid, final, alive2)
    w = T.Worlds(r, *flags)
    for text in ("EF m == 3", "AG m < 3", "AG EF m == 2", "EG m == 0"):
        tree = T.parse(text, m.var_names)
        res = a.ctl(text, witness=True)
        ref = w.result(tree, witness=True)
        assert T.same_verdict(res, ref) and T.witness_rows(res) == ref["witness"]
    after = a.ctl("EF m == 3")
    assert after["n_worlds"] < before["n_worlds"] and not after["possible"] and a.ctl("AG m < 3")["holds"]


def test_twin_on_a_binary_file(stcsp, RefOracle, tmp_path):
    m, r, a, flags, w, _ = case(stcsp, RefOracle, "juggling_b4_f4_nosym")
    a.write_binary(str(tmp_path / "a.bin"))
    b = stcsp.Automaton.read_binary(str(tmp_path / "a.bin"))
    p, q = atoms_for(w, m.var_names)
    for f in ("AG EF {p}", "E[{p} U {q}]", "EG {p}"):
        x, y = a.ctl(f.format(p=p, q=q), witness=True), b.ctl(f.format(p=p, q=q), witness=True)
        assert (x["n_worlds"], x["n_initial"], x["n_initial_sat"]) == (y["n_worlds"], y["n_initial"], y["n_initial_sat"])
        assert int(x["edge_sat"].sum()) == int(y["edge_sat"].sum()) and T.witness_rows(x) == T.witness_rows(y)
    assert b.ctl(stcsp.ctl_parse(m, "EG true"))["holds"]  # a pre-parsed program


# ------------------------------------------------------------------------------------------------- parser, validator, limits
VARS = ["x", "y", "GAMEOVER", "EX", "U", "m_1"]
TEXTS = ["x == 1", "x==1&y!=2", "x < -3 | y >= +4", "x <= y -> y > x", "!x == 1", "!(x == 1)", "EX x == 1", "EF EG AX AF AG x == y",
         "E[x == 1 U y == 2]", "A[ x == 1 | y == 1 U EX y == 2 ]", "true & false", "GAMEOVER == 1 -> AG GAMEOVER == 1",
         "x == 1 -> y == 1 -> x == 2", "x == 1 | y == 1 & x == 2", "EX == 1 & U == 2", "E[U == 1 U U == 2]", "m_1 == -2147483648",
         "m_1 == 2147483647", "AG (x == 3 -> AF y == 1)", "  AG   EF(m_1==0)  ", "!!x == 1", "!EX!x == 1", "A[true U false]"]


def test_the_parser_agrees_with_the_yardsticks_token_by_token(stcsp):
    rng = random.Random(7)
    bounds = [(-3, 3)] * len(VARS)
    texts = TEXTS + [T.show(T.random_formula(rng, len(VARS), bounds, 4), VARS) for _ in range(200)]
    for text in texts:
        assert stcsp.ctl_parse(VARS, text).tolist() == T.postfix(T.parse(text, VARS)), text
    assert stcsp.ctl_parse(VARS, "x == 1 & y < 2 -> EX x != y").tolist() == [3, 0, 0, 1, 3, 1, 2, 2, 11, 4, 0, 1, 1, 20, 13]


@pytest.mark.parametrize("text, position, part", [
    ("", 0, "ends"), ("x ==", 4, "integer"), ("z == 1", 0, "unknown variable 'z'"), ("x == z", 5, "unknown variable 'z'"),
    ("x == 1 &", 8, "ends"), ("(x == 1", 7, "expected )"), ("x == 1)", 6, "unexpected ')'"), ("E[x == 1 y == 2]", 9, "expected U"),
    ("E[x == 1 U y == 2", 17, "expected ]"), ("E x == 1", 2, "expected ["), ("x", 0, "comparison"), ("foo", 0, "unknown word 'foo'"),
    ("x == 2147483648", 5, "outside int32"), ("x == -2147483649", 5, "outside int32"), ("x == 99999999999999999999", 5, "outside int32"),
    ("x = 1", 0, "comparison"), ("x == 1 # y", 7, "unexpected '#'"), ("AG", 2, "ends"), ("x == 1 y == 2", 7, "unexpected 'y'"),
])
def test_parse_errors_carry_a_position_and_a_message(stcsp, text, position, part):
    with pytest.raises(stcsp.CtlSyntaxError) as ex:
        stcsp.ctl_parse(VARS, text)
    assert ex.value.position == position and part in ex.value.message, (ex.value.position, ex.value.message)
    with pytest.raises(T.ParseError):
        T.parse(text, VARS)


def raw(stcsp, a, words, flags=0):
    prog = np.asarray(words, np.int32)
    rq = stcsp.CtlRequest(prog.ctypes.data_as(C.POINTER(C.c_int32)), prog.size, flags)
    h = C.c_void_p()
    rc = stcsp.host_lib().stcsp_automaton_ctl(a._h, C.byref(rq), C.byref(h))
    if rc == 0:
        stcsp.host_lib().stcsp_ctl_free(h)
    return rc


# malformed programs, each STCSP_E_INVALID
MALFORMED = [[], [10], [1, 11], [1, 1], [3, 0, 0], [3, 1000, 0, 1], [3, -1, 0, 1], [3, 0, 6, 1], [3, 0, -1, 1], [4, 0, 0, 1000], [4, 0, 0, -1], [99],
             [0], [1, 1, 23, 1], [1, 20, 27], [3, 0, 0, 1, 3]]


def test_the_program_validator(stcsp, RefOracle):
    a = case(stcsp, RefOracle, "LADDER")[2]
    for words in MALFORMED:
        assert raw(stcsp, a, words) == -1, words
    assert raw(stcsp, a, [1]) == 0 and raw(stcsp, a, [4, 0, 5, 1, 20]) == 0
    rq = stcsp.CtlRequest(None, 3, 0)
    h = C.c_void_p()
    assert stcsp.host_lib().stcsp_automaton_ctl(a._h, C.byref(rq), C.byref(h)) == -1
    with pytest.raises(stcsp.StcspError) as ex:
        a.ctl([10])
    assert ex.value.code == -1


def at_the_node_limit(stcsp):
    """Programs whose LOWERED form has 255, 256 and 257 nodes: 128 atoms under 127 &, then one and two !."""
    base = [stcsp.CTL_TRUE] + [stcsp.CTL_TRUE, stcsp.CTL_AND] * 127
    return base, base + [stcsp.CTL_NOT], base + [stcsp.CTL_NOT, stcsp.CTL_NOT]


def slot_chain(stcsp, k):
    """EX true & (EX true & ( .. )), k conjunctions nested to the right: k + 2 sets at once."""
    return [stcsp.CTL_TRUE, stcsp.CTL_EX] * (k + 1) + [stcsp.CTL_AND] * k


def test_the_limits(stcsp, RefOracle):
    """STCSP_CTL_MAX_NODES = 256 lowered atoms and operators, a predicate stack of 64, STCSP_CTL_MAX_SLOTS = 16 sets at once."""
    assert (stcsp.CTL_MAX_NODES, stcsp.CTL_MAX_SLOTS) == (256, 16)
    a = case(stcsp, RefOracle, "LADDER")[2]
    under, at, over = at_the_node_limit(stcsp)
    assert raw(stcsp, a, under) == 0 and raw(stcsp, a, at) == 0 and raw(stcsp, a, over) == -2
    assert not a.ctl(at)["possible"] and a.ctl(under)["holds"]
    # the lowering counts: A[f U g] is 10 operators around f and three copies of g
    f, g = [stcsp.CTL_TRUE, stcsp.CTL_TRUE, stcsp.CTL_AND], [stcsp.CTL_TRUE] + [stcsp.CTL_TRUE, stcsp.CTL_AND] * 40  # 3 and 81 nodes
    assert raw(stcsp, a, f + g + [stcsp.CTL_AU]) == 0  # 3 + 3 * 81 + 10 = 256
    assert raw(stcsp, a, f + g + [stcsp.CTL_AU, stcsp.CTL_NOT]) == -2
    # a predicate stack of 64: 64 atoms then 63 &, and one more
    assert raw(stcsp, a, [stcsp.CTL_TRUE] * 64 + [stcsp.CTL_AND] * 63) == 0
    assert raw(stcsp, a, [stcsp.CTL_TRUE] * 65 + [stcsp.CTL_AND] * 64) == -2
    assert raw(stcsp, a, slot_chain(stcsp, 14)) == 0 and raw(stcsp, a, slot_chain(stcsp, 15)) == -2
    res = a.ctl(slot_chain(stcsp, 14))
    assert res["holds"] and np.array_equal(res["edge_sat"], res["edge_world"])
    with pytest.raises(stcsp.StcspError) as ex:
        a.ctl(over)
    assert ex.value.code == -2 and "256" in str(ex.value)


def test_ctl_abi(stcsp):
    """The new symbols are exported and the two new structs have the sizes of include/stcsp_engine.h (LP64)."""
    hip = C.CDLL(str(stcsp.CSRC / "libstcsp_hip.so"))
    assert hasattr(hip, "stcsp_engine_ctl")
    for n in ("stcsp_ctl_parse", "stcsp_automaton_ctl", "stcsp_ctl_get", "stcsp_ctl_free"):
        assert hasattr(stcsp.host_lib(), n), n
    assert C.sizeof(stcsp.CtlRequest) == 16
    assert C.sizeof(stcsp.CtlResult) == 96  # 4 x int64, 3 pointers, 6 x int32, 2 x double
    assert stcsp.CtlResult.witness_kind.offset == 56 and stcsp.CtlResult.seconds.offset == 80
    text = (stcsp.CSRC.parents[1] / "include" / "stcsp_engine.h").read_text()
    import re
    for name, value in re.findall(r"#define STCSP_CTL_([A-Z_]+) (\d+)", text):
        if hasattr(stcsp, "CTL_" + name):
            assert getattr(stcsp, "CTL_" + name) == int(value), name
    assert [stcsp.CTL_OPS[int(v)] for _, v in sorted(re.findall(r"#define STCSP_CTL_OP_([A-Z]+) (\d+)", text), key=lambda x: int(x[1]))] == list(T.OP_ORDER)
