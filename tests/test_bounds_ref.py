"""The plain bounds model (tests/bounds_ref.py) against fixpoints derived by hand, one per rule, and against brute force on random
small rows: the yardstick of tests/test_node_seam_gpu.py has to be right on its own. No GPU."""
import itertools

import pytest

import bounds_ref as br
from expr_ref import INT_MAX, INT_MIN, ExprGen

V, C_ = (lambda n: ("v", n)), (lambda n: ("c", n))
P = lambda t: ("point", t)  # noqa: E731


def S(a, b):
    return set(range(a, b + 1))


# ------------------------------------------------------------------ by hand
def test_lower_bound_trim():
    # x >= y, y in 3..4: 0, 1, 2 have no support; 5 is supported by either y
    ok, d = br.propagate([P((">=", V("x"), V("y")))], ["x", "y"], [S(0, 5), S(3, 4)], 0, 1)
    assert ok and d == [S(3, 5), S(3, 4)]


def test_upper_bound_trim():
    # x + y <= 4, y in 2..3: x <= 2; y keeps 3 (x = 0, 1)
    ok, d = br.propagate([P(("<=", ("+", V("x"), V("y")), C_(4)))], ["x", "y"], [S(0, 5), S(2, 3)], 0, 1)
    assert ok and d == [S(0, 2), S(2, 3)]


def test_values_between_the_bounds_stay():
    # x % 2 == 0 on 1..6: the ends 1 goes, 6 stays; 3 and 5 lie between supported bounds and stay; gac drops them
    c = [P(("==", ("%", V("x"), C_(2)), C_(0)))]
    assert br.propagate(c, ["x"], [S(1, 6)], 0, 1) == (True, [S(2, 6)])
    assert br.propagate(c, ["x"], [S(1, 6)], 0, 1, "gac") == (True, [{2, 4, 6}])
    assert br.propagate(c, ["x"], [(1, 7)], 0, 1) == (True, [(2, 6)])  # the same on a pair of bounds


def test_wipe_out():
    # x > y with x <= 1 and y >= 1
    assert br.propagate([P((">", V("x"), V("y")))], ["x", "y"], [S(0, 1), S(1, 2)], 0, 1) == (False, None)


def test_chain_needs_a_second_visit_of_an_earlier_constraint():
    # x < y, then y < z, all 0..3. Pass 1: x < y gives x 0..2, y 1..3; y < z gives y 1..2, z 2..3. Only a second visit of x < y
    # takes 2 from x.
    cons = [P(("<", V("x"), V("y"))), P(("<", V("y"), V("z")))]
    ok, d = br.propagate(cons, ["x", "y", "z"], [S(0, 3), S(0, 3), S(0, 3)], 0, 1)
    assert ok and d == [S(0, 1), S(1, 2), S(2, 3)]
    one = br.revise(cons[0][1], {"x": S(0, 3), "y": S(0, 3)})
    assert one == {"x": S(0, 2), "y": S(1, 3)}  # what one visit alone gives


def test_arc_intersection_with_a_shift():
    # a in [5, 12] == next(b), b in [2, 9]: a at point 0 and b at point 1 both become {6, 7}; over their own lower bounds the same
    # values are bits 1..2 of a and bits 4..5 of b (the shift sh = 3 of revise_next_wide)
    import node_seam as ns
    doms = [S(5, 7), S(2, 9), S(5, 12), S(6, 9)]  # point 0: a, b; point 1: a, b
    ok, d = br.propagate([("arc", "a", "b")], ["a", "b"], doms, 0, 2)
    assert ok and d == [S(6, 7), S(2, 9), S(5, 12), S(6, 7)]
    assert ns.to_mask(d[0], 5) == 0b110 and ns.to_mask(d[3], 2) == 0b110000
    assert br.propagate([("arc", "a", "b")], ["a", "b"], [S(5, 6), S(2, 9), S(5, 12), S(7, 9)], 0, 2) == (False, None)
    # K = 3: the arc holds at points 0 and 1
    ok, d = br.propagate([("arc", "a", "b")], ["a", "b"], [(5, 7), (2, 9), (8, 12), (6, 9), (5, 12), (2, 8)], 0, 3)
    assert ok and d == [(6, 7), (2, 9), (8, 8), (6, 7), (5, 12), (8, 8)]


def test_until_live_and_expired():
    cons = [("until", "g", "y")]
    fixed = [{0}, {0}]
    assert br.propagate(cons, ["g", "y"], fixed, 0, 1) == (False, None)          # live, both fixed, neither is 1
    assert br.propagate(cons, ["g", "y"], fixed, 1, 1) == (True, fixed)          # expired: no check
    assert br.propagate(cons, ["g", "y"], [{1}, {0}], 0, 1)[0]                   # g holds
    assert br.propagate(cons, ["g", "y"], [{0}, {1}], 0, 1)[0]                   # y arrived
    assert br.propagate(cons, ["g", "y"], [{0, 1}, {0}], 0, 1) == (True, [{0, 1}, {0}])  # a check only: nothing is pruned
    # the second until constraint has bit 1; a leaf sets the flag of an until whose y is 1 and keeps what was set
    two = [("until", "g", "y"), ("until", "h", "g")]
    assert br.propagate(two, ["g", "y", "h"], [{0}, {1}, {0}], 0b00, 1) == (False, None)
    assert br.propagate(two, ["g", "y", "h"], [{0}, {1}, {0}], 0b10, 1)[0]
    assert br.next_expire(two, ["g", "y", "h"], [{0}, {1}, {0}], 0b10) == 0b11
    assert br.next_expire(two, ["g", "y", "h"], [{1}, {0}, {0}], 0b00) == 0b10


def test_defining_constraint_over_the_whole_int_range():
    # v == a * b + c with v anywhere: a in 2..3, b in -1..4, c = 1: least value 3 * -1 + 1 = -2, greatest 3 * 4 + 1 = 13
    tree = ("==", V("v"), ("+", ("*", V("a"), V("b")), V("c")))
    ok, d = br.propagate([P(tree)], ["v", "a", "b", "c"], [(INT_MIN, INT_MAX), (2, 3), (-1, 4), (1, 1)], 0, 1)
    assert ok and d == [(-2, 13), (2, 3), (-1, 4), (1, 1)]
    # v fixed: 9 = a * b + 1 needs a * b = 8 = 2 * 4 alone
    ok, d = br.propagate([P(tree)], ["v", "a", "b", "c"], [(9, 9), (2, 3), (-1, 4), (1, 1)], 0, 1)
    assert ok and d == [(9, 9), (2, 2), (4, 4), (1, 1)]
    # two plain variables, one of them the whole range: the intersection
    ok, d = br.propagate([P(("==", V("z"), V("w")))], ["z", "w"], [(-9, 200), (INT_MIN, INT_MAX)], 0, 1)
    assert ok and d == [(-9, 200), (-9, 200)]
    # the project's division: x / 0 = 0, truncation toward zero
    ok, d = br.propagate([P(("==", V("v"), ("/", V("x"), V("y"))))], ["v", "x", "y"], [(INT_MIN, INT_MAX), (-7, -7), (0, 2)], 0, 1)
    assert ok and d == [(-7, 0), (-7, -7), (0, 2)]  # -7 / 0 = 0, -7 / 1 = -7, -7 / 2 = -3


def test_wrap_around_arithmetic():
    # a + 1 > 0 in int32: INT_MAX + 1 wraps to INT_MIN
    ok, d = br.propagate([P((">", ("+", V("a"), C_(1)), C_(0)))], ["a"], [(INT_MAX - 2, INT_MAX)], 0, 1)
    assert ok and d == [(INT_MAX - 2, INT_MAX - 1)]
    # b - 1 < 0: INT_MIN - 1 wraps to INT_MAX
    ok, d = br.propagate([P(("<", ("-", V("b"), C_(1)), C_(0)))], ["b"], [(INT_MIN, INT_MIN + 2)], 0, 1)
    assert ok and d == [(INT_MIN + 1, INT_MIN + 2)]


def test_first_holds_at_point_0_alone_and_rendering():
    c = P(("<", ("first", V("x")), C_(2)))
    assert br.show(c) == "first(x) < 2"
    ok, d = br.propagate([c], ["x"], [S(0, 3), S(0, 3)], 0, 2)
    assert ok and d == [S(0, 1), S(0, 3)]
    assert br.show(P(("<=", ("+", V("x"), V("y")), C_(30)))) == "(x + y) <= 30"
    assert br.show(P(("==", V("_V0"), ("if", ("lt", V("p"), C_(31)), ("+", V("p"), C_(1)), C_(0))))) == "_V0 == if ((p lt 31)) then ((p + 1)) else (0)"
    assert br.show(("arc", "_V1", "_V0")) == "_V1 == next(_V0)" and br.show(("until", "g", "y")) == "g until y"
    assert br.show(P((">=", ("abs", ("-", V("x"), C_(3))), C_(2)))) == "abs((x - 3)) >= 2"


def test_classification_and_split():
    assert br.classify(False, None, 2) == ("fail",)
    assert br.classify(True, [{3}, {4}, {1, 2}], 2) == ("leaf",)                 # time 0 = the first N words
    assert br.classify(True, [{3}, {4, 5, 9}], 2) == ("branch", 1, 6)            # mid = 4 + (9 - 4) // 2
    assert br.classify(True, [(INT_MIN, INT_MAX), (0, 1)], 2) == ("branch", 0, -1)  # needs 64 bits on the device
    assert br.classify(True, [(INT_MAX - 1, INT_MAX)], 1) == ("branch", 0, INT_MAX - 1)
    assert br.split([{3}, {4, 5, 9}], 1, 6) == ([{3}, {4, 5}], [{3}, {9}])
    assert br.split([(INT_MIN, INT_MAX)], 0, -1) == ([(INT_MIN, -1)], [(0, INT_MAX)])


# ------------------------------------------------------------------ laws, against brute force
def random_row(seed):
    """Three variables of at most four values, K = 2, two generated point constraints, sometimes an arc and an until."""
    g = ExprGen(9000 + seed, allow_arrays=False)
    names = ["x", "y", "z"]
    cons = [P(g.constraint(names[: 2 + g.below(2)])), P(g.constraint(["y", "z"] if g.chance(50) else names))]
    if g.chance(50):
        cons.append(("arc", "x", "z"))
    if g.chance(40):
        cons.append(("until", "x", "y"))
    doms = []
    for _ in range(6):
        lo = g.below(2) - 1
        doms.append(S(lo, lo + 1 + g.below(3)))
    return names, cons, doms, g.below(2)


@pytest.mark.parametrize("block", range(4))
def test_laws_on_random_rows(block):
    met = {"consistent": 0, "failed": 0, "pruned": 0, "gac_smaller": 0}
    for seed in range(block * 30, block * 30 + 30):
        names, cons, doms, expire = random_row(seed)
        sols = br.brute_solutions(cons, names, doms, expire, 2)
        ok, fp = br.propagate(cons, names, doms, expire, 2)
        ok_g, fp_g = br.propagate(cons, names, doms, expire, 2, "gac")
        where = (seed, [br.show(c) for c in cons], doms, expire)
        if not ok:
            assert not sols and not ok_g, where  # (gac is at least as strong)
            met["failed"] += 1
            continue
        met["consistent"] += 1
        met["pruned"] += fp != doms
        assert all(d <= d0 for d, d0 in zip(fp, doms)), where
        # every solution inside the input box lies inside the fixpoint
        for s in sols:
            assert all(a in d for a, d in zip(s, fp)), (where, s)
        # both bounds of every variable are supported in the fixpoint, constraint by constraint and point by point
        for c in cons:
            if c[0] != "point":
                continue
            tree = br.strip_first(c[1])
            for p in range(2):
                box = {v: fp[p * 3 + names.index(v)] for v in br.scope_of(tree)}
                assert br.revise_literal(tree, box) == box, (where, br.show(c), p)
        # propagating the fixpoint again changes nothing
        assert br.propagate(cons, names, fp, expire, 2) == (True, fp), where
        # gac is a subset of bounds
        if ok_g:
            assert all(a <= b for a, b in zip(fp_g, fp)), where
            met["gac_smaller"] += fp_g != fp
            for s in sols:
                assert all(a in d for a, d in zip(s, fp_g)), (where, s)
        else:
            assert not sols
    print(met)
    assert met["consistent"] >= 8 and met["failed"] >= 3 and met["pruned"] >= 5, met


def test_one_enumeration_is_the_stated_rule():
    """`revise` (one enumeration of the solutions) == `revise_literal` (drop the least value while it has no support, then the
    greatest, one variable after the other) on generated constraints."""
    changed = 0
    for seed in range(150):
        g = ExprGen(12000 + seed, allow_arrays=False)
        names = ["x", "y", "z"][: 2 + g.below(2)]
        tree = g.constraint(names)
        box = {}
        for v in names:
            lo = g.below(5) - 2
            box[v] = S(lo, lo + g.below(5))
        new = br.revise(tree, box)
        lit = br.revise_literal(tree, box)
        if new is None:
            assert lit is None, (seed, br.show(P(tree)), box)
            continue
        merged = dict(box)
        merged.update(new)
        assert lit == merged, (seed, br.show(P(tree)), box)
        changed += bool(new)
    assert changed >= 20


def test_gac_equals_bounds_on_interval_closed_constraints():
    """x <= y, x + y <= c, x == y + c: the supported values of a variable form an interval whenever the domains do."""
    trees = [("<=", V("x"), V("y")), ("<=", ("+", V("x"), V("y")), C_(3)), ("==", V("x"), ("+", V("y"), C_(1))), ("<", V("x"), V("y"))]
    n = 0
    for tree, (a, b, c, d) in itertools.product(trees, itertools.product(range(-2, 3), range(0, 4), range(-2, 3), range(0, 4))):
        doms = [S(a, a + b), S(c, c + d)]
        got = br.propagate([P(tree)], ["x", "y"], doms, 0, 1)
        assert got == br.propagate([P(tree)], ["x", "y"], doms, 0, 1, "gac"), (tree, doms)
        n += got[0]
    assert n > 100
