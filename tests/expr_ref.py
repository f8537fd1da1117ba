"""Constraint expressions as Python trees (tests only): one tree is rendered to model text (`render`) and evaluated by a plain
Python evaluator (`evaluate`), so no parser sits between the yardstick and the text the engine reads. `solutions` brute-forces a
model over its pinned domains. A seeded generator covers the operator set of a point constraint (no temporal operator: the
automaton of such a model is one state whose live edges are exactly the satisfying tuples), and hand-built programs aim at the
edges of the two device interpreters (k_tabulate in dev_kernels.hpp, eval_program in dev_propagate.hpp).

Semantics: the reference's solverValidateRe (src/solveralgorithm.cpp:336-424) as the project states them -- int32 arithmetic that
wraps, `/` and `%` truncating toward zero, x / 0 = x % 0 = INT_MIN / -1 = INT_MIN % -1 = 0 (the project's definition; the reference
traps), abs INT_MIN = INT_MIN, `if` / `and` / `or` / `->` evaluating the taken side only, a -> b = 1 if a == 0 else a <= b, and an
array index outside [0, len) in an evaluated position clearing `valid` and yielding 0, after which every arithmetic or comparison
node yields 0 (abs, not and the selects do not).

Trees (nested tuples): ("c", n)  ("v", name)  ("arr", name, index)  ("abs", a)  ("not", a)  ("if", c, a, b)
(op, a, b) with op in + - * / % lt gt le ge eq ne and or, and at the root of a constraint only: < > <= >= == != ->."""
import importlib
import itertools
from dataclasses import dataclass, field

_inst = importlib.import_module("stcsp-solver_amd").instances

INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1
ARITH = ("+", "-", "*", "/", "%")
COMPARE = {"lt": "<", "gt": ">", "le": "<=", "ge": ">=", "eq": "==", "ne": "!="}
ROOT_COMPARE = {"<": "lt", ">": "gt", "<=": "le", ">=": "ge", "==": "eq", "!=": "ne"}
EVENTS = ("div_zero", "mod_zero", "neg_dividend", "neg_divisor", "wrap", "abs_int_min", "int_min_div_m1", "invalid_live",
          "invalid_untaken")


# ------------------------------------------------------------------ text
def render(t) -> str:
    k = t[0]
    if k == "c":
        return str(t[1])
    if k == "v":
        return t[1]
    if k == "arr":
        return f"{t[1]}[{render(t[2])}]"
    if k in ("abs", "not"):
        return f"({k} ({render(t[1])}))"
    if k == "if":  # (the else arm is a unary expression in the grammar: always parenthesised)
        return f"(if ({render(t[1])}) then ({render(t[2])}) else ({render(t[3])}))"
    if k in ROOT_COMPARE or k == "->":
        return f"{render(t[1])} {k} {render(t[2])}"
    return f"({render(t[1])} {k} {render(t[2])})"


# ------------------------------------------------------------------ evaluator
def wrap32(x: int) -> int:
    return (x + 2 ** 31) % 2 ** 32 - 2 ** 31


class _Run:
    def __init__(self, values, arrays, events):
        self.values, self.arrays, self.events, self.valid = values, arrays or {}, events, True

    def note(self, name):
        if self.events is not None:
            self.events.add(name)

    def scan_untaken(self, t):
        """Instrumentation only: does a sub-tree that is NOT evaluated hold a lookup that would leave its array? (Its operands are
        computed with a scratch run so that the real one sees nothing of it.)"""
        if self.events is None:
            return
        scratch = _Run(self.values, self.arrays, set())
        scratch.go(t)
        if "invalid_live" in scratch.events or "invalid_untaken" in scratch.events:
            self.events.add("invalid_untaken")

    def go(self, t) -> int:
        k = t[0]
        if k == "c":
            return t[1]
        if k == "v":
            return self.values[t[1]]
        if k == "arr":
            i = self.go(t[2])
            a = self.arrays[t[1]]
            if i < 0 or i >= len(a):
                self.valid = False
                self.note("invalid_live")
                return 0
            return a[i]
        if k == "abs":
            v = self.go(t[1])
            if v == INT_MIN:
                self.note("abs_int_min")
            return wrap32(-v) if v < 0 else v
        if k == "not":
            return int(self.go(t[1]) == 0)
        if k == "if":
            c = self.go(t[1])
            self.scan_untaken(t[3] if c else t[2])
            return self.go(t[2]) if c else self.go(t[3])
        if k == "and":
            a = self.go(t[1])
            if a == 0:
                self.scan_untaken(t[2])
                return 0
            return self.go(t[2])
        if k == "or":
            a = self.go(t[1])
            if a != 0:
                self.scan_untaken(t[2])
                return 1
            return self.go(t[2])
        if k == "->":
            a = self.go(t[1])
            if a == 0:
                self.scan_untaken(t[2])
                return 1
            return int(a <= self.go(t[2]))
        a = self.go(t[1])
        b = self.go(t[2])
        if not self.valid:
            return 0
        k = ROOT_COMPARE.get(k, k)
        if k == "lt":
            return int(a < b)
        if k == "gt":
            return int(a > b)
        if k == "le":
            return int(a <= b)
        if k == "ge":
            return int(a >= b)
        if k == "eq":
            return int(a == b)
        if k == "ne":
            return int(a != b)
        if k in ("+", "-", "*"):
            r = a + b if k == "+" else (a - b if k == "-" else a * b)
            if r != wrap32(r) and k != "-":
                self.note("wrap")
            return wrap32(r)
        if k in ("/", "%"):
            if a < 0:
                self.note("neg_dividend")
            if b < 0:
                self.note("neg_divisor")
            if b == 0:
                self.note("div_zero" if k == "/" else "mod_zero")
                return 0
            if a == INT_MIN and b == -1:
                if k == "/":
                    self.note("int_min_div_m1")
                return 0
            q = abs(a) // abs(b)
            if (a < 0) != (b < 0):
                q = -q
            return q if k == "/" else a - q * b
        raise ValueError(f"unknown node {k!r}")


def evaluate(tree, values, arrays=None, events=None):
    """(value, valid) of `tree` under `values` (name -> int). `arrays`: name -> list. `events`: a set that collects the EVENTS
    met on the way."""
    run = _Run(values, arrays, events)
    v = run.go(tree)
    return v, run.valid


# ------------------------------------------------------------------ models
@dataclass
class ExprModel:
    """Variables in declaration order (the engine's variable order: no temporal operator, so no auxiliary variable), the
    declared domain and the pinned range of each, arrays, and the constraints beside the pins. `defined`: a variable without pins
    whose value the constraint `v == e` fixes (the interval legs), as (name, e)."""
    names: list
    declared: dict
    pins: dict
    constraints: list
    arrays: dict = field(default_factory=dict)
    defined: tuple = None
    label: str = ""

    def pin_constraints(self):
        out = []
        for v in self.names:
            if v in self.pins:
                a, b = self.pins[v]
                out += [(">=", ("v", v), ("c", a)), ("<=", ("v", v), ("c", b))]
        return out

    def all_constraints(self):
        return self.pin_constraints() + list(self.constraints)

    def text(self, declared=None) -> str:
        d = declared or self.declared
        out = [f"var {v} : [{d[v][0]}, {d[v][1]}];" for v in self.names]
        out += [f"arr {a} : {{{', '.join(map(str, xs))}}};" for a, xs in self.arrays.items()]
        out += [render(c) + ";" for c in self.all_constraints()]
        return "\n".join(out) + "\n"

    def host_text(self) -> str:
        """The same model with every declared domain reduced to its pinned range (a defined variable to at most 32 values around
        what `e` can give): the product is small enough for the host to tabulate."""
        d = dict(self.declared)
        d.update(self.pins)
        if self.defined:
            lo, hi = self.declared[self.defined[0]]
            got = sorted({t[self.names.index(self.defined[0])] for t in solutions(self)})
            a = max(lo, got[0]) if got else lo
            d[self.defined[0]] = (a, min(hi, a + 31))
        return self.text(d)

    def pinned_tuples(self) -> int:
        n = 1
        for a, b in self.pins.values():
            n *= b - a + 1
        return n

    def declared_product(self) -> int:
        n = 1
        for lo, hi in self.declared.values():
            n *= hi - lo + 1
        return n


def holds(model: ExprModel, values, events=None) -> bool:
    for c in model.all_constraints():
        if evaluate(c, values, model.arrays, events)[0] == 0:
            return False
    return True


_solutions_cache = {}


def solutions(model: ExprModel, events=None) -> set:
    """Every tuple (declaration order) of the pinned product on which every constraint of the model is non-zero. (The pins are
    constraints over one variable each: they are evaluated once per value, the others once per tuple.)"""
    key = model.text() if events is None else None
    if key in _solutions_cache:
        return _solutions_cache[key]
    free = [v for v in model.names if v in model.pins]
    unary = {v: [c for c in model.pin_constraints() if c[1] == ("v", v)] for v in free}
    ranges = [[x for x in range(model.pins[v][0], model.pins[v][1] + 1)
               if all(evaluate(c, {v: x}, model.arrays, events)[0] != 0 for c in unary[v])] for v in free]
    out = set()
    for combo in itertools.product(*ranges):
        values = dict(zip(free, combo))
        if model.defined:
            v, e = model.defined
            values[v] = evaluate(e, values, model.arrays, events)[0]
            if not model.declared[v][0] <= values[v] <= model.declared[v][1]:
                continue
        if all(evaluate(c, values, model.arrays, events)[0] != 0 for c in model.constraints):
            out.add(tuple(values[v] for v in model.names))
    if key is not None:
        _solutions_cache[key] = out
    return out


def whole_product(model: ExprModel) -> int:
    return model.pinned_tuples()


# ------------------------------------------------------------------ generator
class ExprGen:
    """Random expressions over a given list of variables, each of which appears at least once (so that the constraint's scope
    product is the declared one). Sub-expressions stay small in value -- extreme intermediate results (INT_MIN, INT_MAX, across the
    wrap) are folded back by a comparison, a remainder or a division -- so that the root comparison is not decided by magnitude."""

    def __init__(self, seed, arrays=None, allow_arrays=True):
        self.r = _inst.SplitMix64(0xE5A10000 + seed)
        self.arrays = arrays if arrays is not None else {}
        self.allow_arrays = allow_arrays
        self.pool = []

    def below(self, n):
        return self.r.below(n)

    def pick(self, xs):
        return xs[self.r.below(len(xs))]

    def chance(self, pct):
        return self.r.below(100) < pct

    def const(self):
        return ("c", self.pick([-3, -2, -1, -1, 0, 0, 1, 1, 2, 2, 3, 5, 7]))

    def leaf(self):
        return ("v", self.pick(self.pool)) if self.chance(70) else self.const()

    def extreme(self, x, y):
        """A sub-expression around x (and y) whose intermediate results reach INT_MIN / INT_MAX / wrap, folded back to a small value."""
        k = self.below(9)
        if k == 0:  # x + INT_MAX wraps for x > 0
            return ("lt", ("+", x, ("c", INT_MAX)), ("c", 0))
        if k == 1:  # INT_MIN - x ... and back
            return ("%", ("+", ("c", INT_MIN), x), ("c", 7))
        if k == 2:  # x * 2^30 * 2: INT_MIN for odd x, 0 for even
            return ("eq", ("*", ("*", x, ("c", 1 << 30)), ("c", 2)), ("c", INT_MIN))
        if k == 3:  # abs INT_MIN (x == 0)
            return ("lt", ("abs", ("+", ("c", INT_MIN), x)), y)
        if k == 4:  # INT_MIN / -1 (x == 0, y == -1); / by zero (y == 0)
            return ("/", ("/", ("+", ("c", INT_MIN), x), y), ("c", 1 << 29))
        if k == 5:  # INT_MIN % -1, % by zero
            return ("%", ("-", ("c", INT_MIN), ("abs", x)), y)
        if k == 6:  # INT_MAX * x wraps for |x| > 1
            return ("%", ("*", ("c", INT_MAX), x), ("c", 5))
        if k == 7:  # (INT_MAX + x) / y
            return ("/", ("/", ("+", ("c", INT_MAX), x), y), ("c", 1 << 28))
        return ("ge", ("*", ("+", x, ("c", 46341)), ("+", y, ("c", 46341))), ("c", 0))  # 46341^2 > INT_MAX

    def lookup(self, index):
        name = self.pick(sorted(self.arrays))
        n = len(self.arrays[name])
        k = self.below(3)
        if k == 0:  # leaves the array on both sides
            return ("arr", name, ("+", index, ("c", self.below(3) - 1)))
        if k == 1:
            return ("arr", name, ("+", index, ("c", n - 2)))
        return ("arr", name, ("%", index, ("c", n)))  # negative remainders leave it below

    def expr(self, need, depth=0):
        """An expression in which every variable of `need` occurs."""
        if len(need) <= 1:
            x = ("v", need[0]) if need else self.leaf()
            k = self.below(100)
            if depth > 6 or k < 40:
                return x
            y = self.leaf()
            if k < 50:
                return self.extreme(x, y)
            if k < 58 and self.arrays and self.allow_arrays:
                return self.lookup(x)
            if k < 64:
                return ("abs", ("-", x, y))
            if k < 70:
                return ("not", x)
            if k < 76:
                return (self.pick(["/", "%"]), x, self.pick([y, ("c", self.pick([-3, -2, 2, 3]))]))
            if k < 84:
                return ("*", x, ("c", self.pick([-2, -1, 2, 3])))
            if k < 92:
                return (self.pick(sorted(COMPARE)), x, y)
            return ("if", (self.pick(sorted(COMPARE)), x, y), self.expr([], depth + 1), self.expr([], depth + 1))
        k = self.below(100)
        if k < 14 and len(need) >= 3:
            i = 1 + self.below(len(need) - 2)
            j = i + 1 + self.below(len(need) - i - 1) if len(need) - i > 1 else i + 1
            c = self.expr(need[:i], depth + 1)
            if self.chance(60):
                c = (self.pick(sorted(COMPARE)), c, self.const())
            return ("if", c, self.expr(need[i:j], depth + 1), self.expr(need[j:], depth + 1))
        i = 1 + self.below(len(need) - 1)
        a, b = self.expr(need[:i], depth + 1), self.expr(need[i:], depth + 1)
        if k < 34:
            return ("+", a, b)
        if k < 48:
            return ("-", a, b)
        if k < 56:
            return ("*", a, b)
        if k < 62:
            return ("/", a, b)
        if k < 68:
            return ("%", a, b)
        if k < 84:
            return (self.pick(sorted(COMPARE)), a, b)
        if k < 92:
            return ("and", a, b)
        return ("or", a, b)

    def constraint(self, names):
        """A root comparison (or `->`) over all of `names`, in a shuffled order."""
        self.pool = list(names)
        order = sorted(names, key=lambda _: self.below(1 << 20))
        i = 1 + self.below(len(order) - 1) if len(order) > 1 else len(order)
        a, b = self.expr(order[:i]), self.expr(order[i:])
        op = self.pick(["<=", ">=", "<", ">", "!=", "<=", ">=", "==", "->"])
        return (op, a, b)


PIN_RANGES = [(-1, 1), (-1, 0), (0, 1), (-2, -1), (1, 2), (-1, 1), (0, 1), (-1, 0)]


def pinned(gen, names, max_tuples=2048):
    """Two or three values per variable; the first three variables get a negative value, zero and a positive one between them."""
    pins, tuples = {}, 1
    for i, v in enumerate(names):
        a, b = [(-1, 0), (0, 1), (-1, 1)][i] if i < 3 else gen.pick(PIN_RANGES)
        if tuples * (b - a + 1) > max_tuples:
            b = a + 1 if tuples * 2 <= max_tuples else a
        if tuples * (b - a + 1) > max_tuples:
            b = a
        pins[v] = (a, b)
        tuples *= b - a + 1
    return pins


def clamp(pin, dom):
    """The pinned range moved into the declared domain, its width kept."""
    (a, b), (lo, hi) = pin, dom
    w = min(b - a, hi - lo)
    a = min(max(a, lo), hi - w)
    return (a, a + w)


def random_model(seed, declared, single=(), arrays=True, label="") -> ExprModel:
    """One generated constraint over the variables of `declared` (name -> (lo, hi), in order), every variable pinned to two or
    three values inside its declared domain -- those of `single` to one value. Five seeds of six draw again (up to six times, from
    a stream of their own) while the constraint holds on no tuple or on all of them; every sixth takes what comes."""
    names = list(declared)
    for attempt in range(1 if seed % 6 == 0 else 6):
        g = ExprGen(seed * 8 + attempt)
        arr = {}
        if arrays and g.chance(60):
            arr = {"T": [g.below(7) - 3 for _ in range(2 + g.below(4))]}
        g.arrays = arr
        pins = pinned(g, [v for v in names if v not in single])
        for v in single:
            pins[v] = (g.pick([-1, 0, 1]),) * 2
        pins = {v: clamp(pins[v], declared[v]) for v in names}
        m = ExprModel(names, dict(declared), pins, [g.constraint(names)], arr, label=label or f"seed {seed}")
        if 0 < len(solutions(m)) < m.pinned_tuples():
            break
    return m


def defining_model(seed, declared, v, label="") -> ExprModel:
    """`v == e` with e generated over the other variables and no array (the defining form of cset.cpp); v has no pins."""
    names = list(declared)
    others = [x for x in names if x != v]
    g = ExprGen(seed, allow_arrays=False)
    pins = {x: clamp(r, declared[x]) for x, r in pinned(g, others).items()}
    g.pool = list(others)
    e = g.expr(sorted(others, key=lambda _: g.below(1 << 20)))
    return ExprModel(names, dict(declared), pins, [("==", ("v", v), e)], {}, defined=(v, e), label=label or f"seed {seed}")


# ------------------------------------------------------------------ hand-built programs
def right_sum(names, depth):
    """x0 + (x1 + (x2 + ...)) nested `depth` - 1 times: an operand stack of `depth` entries."""
    e = ("v", names[(depth - 1) % len(names)])
    for k in reversed(range(depth - 1)):
        e = ("+", ("v", names[k % len(names)]), e)
    return e


def left_chain(names, terms):
    """((x0 - x1) + x2) - ... nested to the left: a stack of two, 2 * terms - 1 code words (plus the comparison's)."""
    e = ("v", names[0])
    for k in range(1, terms):
        e = ("+" if k % 2 else "-", e, ("v", names[k % len(names)]))
    return e


def code_words(t) -> int:
    """Words of the compiled postfix program of a tree without array lookups (no guard markers), without OP_END."""
    k = t[0]
    if k == "c":
        return 2
    if k == "v":
        return 1
    if k in ("abs", "not", "arr"):
        return 1 + code_words(t[-1])
    n = 1  # (plain loops: one Python frame per level, the left-nested chains are hundreds of levels deep)
    for x in t[1:]:
        n += code_words(x)
    return n


def stack_depth(t) -> int:
    k = t[0]
    if k in ("c", "v"):
        return 1
    if k in ("abs", "not", "arr"):
        return stack_depth(t[-1])
    d = 0
    for i, x in enumerate(t[1:]):
        d = max(d, stack_depth(x) + i)
    return d


def nested_if(names, depth, bottom, at=None):
    """if (x0 ge a0) then (if (x1 ge a1) then ( ... bottom ... ) else 1) else 0, `depth` conditionals deep: the bottom is evaluated
    only when every condition on the way holds (`at`: name -> threshold, 1 without)."""
    e = bottom
    for k in reversed(range(depth)):
        v = names[k % len(names)]
        e = ("if", ("ge", ("v", v), ("c", at[v] if at else 1)), e, ("c", k % 2))
    return e


def _bad(c):
    raise AssertionError(f"hand-built program misses its shape: {code_words(c) + 1} words, stack {stack_depth(c)}")


def hand_models(declared, single=()) -> list:
    """The hand-built programs over the variables of `declared` (at least eight), pinned like the random ones."""
    names = list(declared)
    free = [v for v in names if v not in single]
    out = []
    base = random_model(0, declared, single, arrays=False)
    top = {v: base.pins[v][1] for v in names}  # a condition `v ge top[v]` holds on v's greatest pinned value alone

    def add(label, constraint, arrays=None, check=None):
        m = ExprModel(names, dict(declared), dict(base.pins), [], label=label)
        used = set()

        def walk(t):
            if t[0] == "v":
                used.add(t[1])
            for x in t[1:]:
                if isinstance(x, tuple):
                    walk(x)
        walk(constraint)
        left = constraint[1]
        for v in names:  # every declared variable in the scope: (l + v) - v is l in wrapping arithmetic, on a stack of two
            if v not in used:
                left = ("-", ("+", left, ("v", v)), ("v", v))
        constraint = (constraint[0], left, constraint[2])
        if check:
            check(constraint, len(used) == len(names))
        m.constraints = [constraint]
        m.arrays = arrays or {}
        out.append(m)

    for d in (3, 4, 5, 31, 32, 33):  # operand-stack depths (the root comparison's left operand sits below the sum: d - 1 + 1)
        e = right_sum(free, d - 1)
        add(f"stack depth {d}", (">=", ("v", free[0]), e), check=lambda c, whole, d=d: stack_depth(c) == d or _bad(c))
    for words in (63, 64, 65, 127, 128, 129, 201):  # code words, OP_END included
        # `chain >= c`: 2 * terms - 1 words, 2 for the constant, 1 for the comparison, 1 for OP_END; an `abs` adds one
        terms, odd = (words - 3) // 2, (words - 3) % 2
        e = left_chain(free, terms)
        if odd:
            e = ("abs", e)
        add(f"{words} code words", ("!=", e, ("c", 1)),
            check=lambda c, whole, words=words: (stack_depth(c) == 2 and (not whole or code_words(c) + 1 == words)) or _bad(c))
    T = {"T": [2, -1, 3]}
    for depth in (1, 2, 31):
        # an out-of-range lookup at the bottom of `depth` conditionals: in an evaluated position when they all hold, untaken otherwise
        bottom = ("arr", "T", ("+", ("v", free[0]), ("c", 3)))  # (the first variable is pinned to -1 .. 0: index 2 or 3 of three)
        c = (">=", ("+", nested_if(free[1:], depth, bottom, top), ("v", free[0])), ("c", 1))
        add(f"conditional nesting {depth}", c, T)
    # the same lookup under 31 conditionals of which the outermost never holds: never evaluated
    c = (">=", ("+", ("if", ("gt", ("v", free[0]), ("c", 5)), nested_if(free[1:], 30, ("arr", "T", ("c", 7)), top), ("v", free[1])), ("v", free[2])), ("c", 0))
    add("untaken lookup under 31 conditionals", c, T)
    two, m1 = ("+", ("v", free[0]), ("c", 2)), ("-", ("v", free[1]), ("c", 1))  # 1..3 and -2..0 over the pins: operands like 2 and -1
    add("-> with operands 2 and -1", ("->", ("+", ("*", ("v", free[0]), ("c", 2)), ("v", free[2])), ("-", ("*", ("v", free[1]), ("c", 2)), ("v", free[3]))))
    add("and / or with operands 2 and -1", ("==", ("+", ("and", two, m1), ("or", m1, two)), ("+", ("and", m1, ("v", free[2])), ("or", ("v", free[3]), m1))))
    add("and / or raw right operand", ("<", ("and", ("v", free[0]), ("*", ("v", free[1]), ("c", 2))), ("or", ("v", free[2]), ("*", ("v", free[3]), ("c", -3)))))
    return out


def too_deep_text(n=8) -> str:
    """32 nested conditionals over an array lookup: refused with STCSP_E_UNSUPPORTED 'conditional nesting deeper than 31'."""
    names = [f"x{i}" for i in range(n)]
    e = nested_if(names, 32, ("arr", "T", ("v", names[0])))
    return "".join(f"var {v} : [0, 1];\n" for v in names) + "arr T : {1, 0};\n" + render((">=", e, ("c", 1))) + ";\n"


# ------------------------------------------------------------------ the corpus, leg by leg
def dom(n, lo, hi):
    return {f"x{i}": (lo, hi) for i in range(n)}


def spread(names, k=8):
    """k names spread over the list (the variables of a big scope that stay open)."""
    return [names[(2 * i + 1) * len(names) // (2 * k)] for i in range(k)]


# name -> (declared domains, seed base). Products: 7^8 = 5,764,801 (odd: the last wavefront and bitmap word are partial),
# 8^8 = 2^24 (a multiple of 64), 3^16 = 43,046,721 (16 variables: the most k_tabulate decodes), 40 * 7^7 and 100 * 7^6 (W = 2, 4):
# all above 2^22 (the host's limit) and below 2^28 (the device's).
SHAPES = {
    "odd": (dom(8, -3, 3), 0),
    "mult64": (dom(8, -4, 3), 1000),
    "vars16": (dom(16, -1, 1), 2000),
    "w2": ({"w": (-20, 19), **dom(7, -3, 3)}, 3000),
    "w4": ({"w": (-50, 49), **dom(6, -3, 3)}, 4000),
    "big65": (dom(65, -1, 1), 5000),
    "big130": (dom(130, -1, 1), 6000),
}
SCOPES = (17, 22, 23, 24, 28, 29, 64)


def shape_models(shape, n_random, hand=True) -> list:
    declared, base = SHAPES[shape]
    single = ()
    if shape.startswith("big"):
        names = list(declared)
        keep = set(spread(names))
        single = tuple(v for v in names if v not in keep)
    out = [random_model(base + i, declared, single, label=f"{shape} seed {base + i}") for i in range(n_random)]
    if hand:
        for m in hand_models(declared, single):
            m.label = f"{shape}: {m.label}"
            out.append(m)
    return out


def sum_le_model(n) -> ExprModel:
    """x0 <= (x1 + ... + x_(n-1)) over n two-valued variables, the first eleven open."""
    declared = dom(n, 0, 1)
    names = list(declared)
    pins = {v: ((0, 1) if i < 11 else ((i % 2,) * 2)) for i, v in enumerate(names)}
    e = ("v", names[1])
    for v in names[2:]:
        e = ("+", e, ("v", v))
    return ExprModel(names, declared, pins, [("<=", ("v", names[0]), e)], label=f"scope {n}: x0 <= sum")


def scope_models(n, n_random=1) -> list:
    return [sum_le_model(n)] + [random_model(7000 + 10 * n + i, dom(n, 0, 1), label=f"scope {n} seed {7000 + 10 * n + i}")
                                for i in range(n_random)]


def interval_models(form, n_random) -> list:
    """form: "exists" (a plain constraint), "def" (v == e, v of seven values), "image" (v == e, v far wider than e's hull)."""
    if form == "exists":
        return [random_model(8000 + i, dom(8, -3, 3), label=f"interval exists seed {8000 + i}") for i in range(n_random)]
    declared = {"v": (-3, 3) if form == "def" else (-1000, 1000), **dom(8, -3, 3)}
    base = 8500 if form == "def" else 9000
    return [defining_model(base + i, declared, "v", label=f"interval {form} seed {base + i}") for i in range(n_random)]
