"""Seeded random stCSP models over the whole constraint language (tests only): small domains, a
few constraints, every operator the front end accepts except the ones the reference itself
mis-normalises (`not`, `@` after `next`) and `/`, `%` by a variable
(SIGFPE in the reference). Used to compare implementations with each other on inputs nobody
hand-picked."""
import importlib

_inst = importlib.import_module("stcsp-solver_amd").instances


class Gen:
    def __init__(self, seed):
        self.r = _inst.SplitMix64(0x5EED0000 + seed)
        self.vars = []
        self.arr_len = 0

    def pick(self, xs):
        return xs[self.r.below(len(xs))]

    def chance(self, pct):
        return self.r.below(100) < pct

    def var(self):
        return self.pick(self.vars)

    def atom(self):
        k = self.r.below(100)
        if k < 50:
            return self.var()
        if k < 70:
            return str(self.r.below(4))
        if k < 82:
            return f"next {self.var()}"
        if k < 90:
            return f"first {self.var()}"
        if k < 95:
            return f"({self.var()} fby {self.var()})"
        return f"({self.var()} @ {1 + self.r.below(2)})"

    def expr(self, depth):
        if depth == 0 or self.chance(35):
            return self.atom()
        k = self.r.below(100)
        a, b = self.expr(depth - 1), self.expr(depth - 1)
        if k < 18:
            return f"({a} + {b})"
        if k < 32:
            return f"({a} - {b})"
        if k < 40:
            return f"({a} * {self.r.below(3)})"
        if k < 44:
            return f"({a} % {2 + self.r.below(2)})"
        if k < 46:
            return f"({a} / {1 + self.r.below(3)})"
        if k < 50:
            return f"(abs {a})"
        if k < 78:
            return f"({a} {self.pick(['lt', 'gt', 'le', 'ge', 'eq', 'ne'])} {b})"
        if k < 88:
            return f"({a} {self.pick(['and', 'or'])} {b})"
        if k < 95:
            return f"(if ({a} {self.pick(['lt', 'eq', 'ge'])} {b}) then {self.atom()} else {self.atom()})"
        if self.arr_len:
            return f"T[({a}) % {self.arr_len}]" if self.chance(50) else f"T[{self.var()}]"
        return f"({a} + {b})"

    def model(self):
        n = 2 + self.r.below(3)
        out = []
        for i in range(n):
            lo = self.r.below(3) - 1
            hi = lo + self.r.below(4)
            self.vars.append(f"v{chr(97 + i)}")
            out.append(f"var {self.vars[-1]} : [{lo}, {hi}];")
        if self.chance(30):
            self.arr_len = 2 + self.r.below(3)
            out.append("arr T : {" + ", ".join(str(self.r.below(4)) for _ in range(self.arr_len)) + "};")
        if self.chance(60):  # an initial condition and a transition, like every shipped model
            v = self.var()
            out.append(f"first {v} == {self.r.below(2)};")
        if self.chance(70):
            v = self.var()
            out.append(f"next {v} {self.pick(['==', '>=', '<=', '!='])} {self.expr(1)};")
        for _ in range(1 + self.r.below(3)):
            if self.chance(8):
                out.append(f"{self.var()} until {self.var()};")
                continue
            op = self.pick(["==", "==", "!=", "<", ">", "<=", ">=", "->"])
            out.append(f"{self.expr(2)} {op} {self.expr(2)};")
        return "\n".join(out) + "\n"


def random_model(seed: int) -> str:
    return Gen(seed).model()


class WideGen(Gen):
    """The same language over domains of 33..128 values (bitset blocks of two and four words per variable: the engine's
    W = 2 / 4 kernels): one or two wide variables, the others small, constants that reach into the wide ranges, and
    transitions that walk through them so that the automata are not trivial."""

    def atom(self):
        k = self.r.below(100)
        if k < 50:
            return self.var()
        if k < 62:
            return str(self.r.below(4))
        if k < 72:
            return str(self.r.below(self.span))
        if k < 84:
            return f"next {self.var()}"
        if k < 92:
            return f"first {self.var()}"
        return f"({self.var()} fby {self.var()})"

    def model(self):
        n = 2 + self.r.below(2)
        n_wide = 1 + self.r.below(2)
        out = []
        self.span = 33 + self.r.below(96 if self.chance(50) else 32)  # 33..64 (W = 2) or 33..128 (W = 4)
        for i in range(n):
            lo = self.r.below(3) - 1
            hi = lo + (self.span - 1 if i < n_wide else self.r.below(4))
            self.vars.append(f"v{chr(97 + i)}")
            out.append(f"var {self.vars[-1]} : [{lo}, {hi}];")
        if self.chance(25):
            self.arr_len = 2 + self.r.below(3)
            out.append("arr T : {" + ", ".join(str(self.r.below(4)) for _ in range(self.arr_len)) + "};")
        w = self.vars[0]
        step = 1 + self.r.below(5)
        k = self.r.below(100)
        if k < 70:  # the wide variable walks: few successors per state, many states
            out.append(f"first {w} == {self.r.below(3)};")
            if self.chance(50):
                out.append(f"next {w} == (if ({w} ge {self.span - step - 2}) then {self.r.below(3)} else ({w} + {step}));")
            else:
                out.append(f"next {w} >= {w} + {step - 1};")
                out.append(f"next {w} <= {w} + {step};")
        elif k < 85:
            out.append(f"next {w} {self.pick(['==', '>=', '<='])} {self.expr(1)};")
        if n_wide > 1:  # tie the second wide variable to the first, or it multiplies every state's edges by its whole domain
            d = self.r.below(4)
            out.append(f"{self.vars[1]} {self.pick(['==', '<=', '>='])} {w} {self.pick(['+', '-'])} {d};")
            if self.chance(70):
                out.append(f"{self.vars[1]} {self.pick(['>=', '<='])} {w} {self.pick(['+', '-'])} {self.r.below(3)};")
        for _ in range(1 + self.r.below(2)):
            if self.chance(6):
                out.append(f"{self.var()} until {self.var()};")
                continue
            op = self.pick(["==", "!=", "<", ">", "<=", ">=", "->"])
            out.append(f"{self.expr(1)} {op} {self.expr(2)};")
        return "\n".join(out) + "\n"


def random_wide_model(seed: int) -> str:
    return WideGen(seed).model()


# WideGen seeds that no node cap cuts short: seed 142 has no solution, but the oracle's support search over three
# occurrences of 87-value variables in one constraint takes minutes before the first search node. Fuzzes that must check
# the same models on every machine (a max_search_nodes cap, no wall-clock limit) leave these out by name.
WIDE_SLOW_SEEDS = (142,)


class UntilGen(Gen):
    """Gen's model with one more `until` constraint over two of its variables, so that most automata carry until flags
    and the backward traverse has something to decide."""

    def model(self):
        text = super().model()
        a = self.var()
        b = self.var()
        return text + f"{a} until {b};\n"


def random_until_model(seed: int) -> str:
    return UntilGen(seed).model()


def game_model(W: int, alo: int, shift: int = 0) -> str:
    """A game over an opponent variable o of W values (var 0) and an avatar a (var 1): o's low half adds a to the
    counter s, its high half takes one off; the top value of o is forbidden once s reaches 3. Eight states whatever W
    is. The top value of o is missing exactly in the states the adversarial passes invalidate, so the answer changes
    with a wrong last cover word. `shift` moves o's domain and the two constants that mention it."""
    lo, top, mid = shift, W - 1 + shift, W // 2 + shift
    return (f"var o:[{lo},{top}]; var a:[{alo},2]; var s:[0,6]; first s == 0;\n"
            f"next s == (if (o lt {_const(mid)}) then (s + a) else (if (s gt 0) then (s - 1) else 0));\n"
            f"((s lt 3) or (o ne {_const(top)})) == 1;\n")


def _const(c: int) -> str:
    return str(c) if c >= 0 else f"(0 - {-c})"


def adv_chain(L: int) -> str:
    """A chain of L + 1 states whose last one lacks o == 1: adversarial(o) invalidates one state per sweep, back to
    the root."""
    return (f"var o:[0,1]; var s:[0,{L}]; first s == 0;\n"
            f"next s == (if (s lt {L}) then (s + 1) else s);\n"
            f"((s lt {L}) or (o ne 1)) == 1;\n")


def until_chain(L: int) -> str:
    """An until flag that only the end of a chain of L steps fulfils: validity travels backwards over L edges."""
    return (f"var x:[0,{L}]; var y:[0,1]; var g:[0,1]; first x == 0; next x == if (x lt {L}) then x + 1 else x; "
            f"y == (x eq {L}); g until y;")


NO_SOLUTION = "var x:[0,1]; x == 0; x == 1;\n"


def table_automaton(seed, digits, letters, keep_pct, goal_pct, rooted=True, colours=2):
    """A random automaton of a chosen size through the ordinary front end: the model's arrays are its transition table. The
    state is one variable s of S values, or two digits s1, s0 of bases `digits` (S their product: several hundred states with
    every domain at most 32 values); the letter x picks the successor T[s * A + x], OK keeps `keep_pct` of the S * A entries,
    G makes `goal_pct` of the states goals of `w until g`, and the colour c == CC[s * A + x] is a random function of state and
    letter: observed alone it hides both. rooted=False drops the `first` of the low digit: one edge of the root per start state."""
    digits = tuple(digits)
    assert len(digits) in (1, 2) and all(b >= 1 for b in digits) and letters >= 1 and colours >= 1
    A, B0 = letters, digits[-1]
    S = digits[0] * B0 if len(digits) == 2 else B0
    r = _inst.SplitMix64(0x7AB1E000 + seed)
    T = [r.below(S) for _ in range(S * A)]
    OK = [int(r.below(100) < keep_pct) for _ in range(S * A)]
    G = [int(r.below(100) < goal_pct) for _ in range(S)]
    CC = [r.below(colours) for _ in range(S * A)]
    # what the front end needs: every array as long as its index range, every index inside it, every entry inside its variable's domain
    assert len(T) == len(OK) == len(CC) == S * A and len(G) == S
    assert (S - 1) * A + (A - 1) < len(T) and S - 1 < len(G)  # the largest indices the model forms
    assert all(0 <= t < S for t in T) and all(0 <= c < colours for c in CC)

    def arr(name, xs):
        return f"arr {name} : {{{', '.join(map(str, xs))}}};"
    if len(digits) == 1:
        out = [f"var s:[0,{S - 1}];", arr("T", T)]
        state, index = "s", f"s * {A} + x"
        rules = (["first s == 0;"] if rooted else []) + [f"next s == T[{index}];"]
    else:
        out = [f"var s1:[0,{digits[0] - 1}]; var s0:[0,{B0 - 1}];", arr("T1", [t // B0 for t in T]), arr("T0", [t % B0 for t in T])]
        state = f"s1 * {B0} + s0"
        index = f"({state}) * {A} + x"
        rules = ["first s1 == 0;"] + (["first s0 == 0;"] if rooted else []) + [f"next s1 == T1[{index}];", f"next s0 == T0[{index}];"]
    out.insert(1, f"var x:[0,{A - 1}]; var g:[0,1]; var w:[0,1]; var c:[0,{colours - 1}];")
    out += [arr("OK", OK), arr("G", G), arr("CC", CC)]
    out += rules + [f"OK[{index}] == 1;", f"c == CC[{index}];", f"g == G[{state}];", "w until g;"]
    return "\n".join(out) + "\n"


def _table_reach(T, OK, A, starts):
    """The table's states that a start state reaches over kept entries (the until flag aside), in breadth-first order."""
    seen, order = set(starts), list(starts)
    for s in order:
        for x in range(A):
            t = T[s * A + x]
            if OK[s * A + x] and t not in seen:
                seen.add(t)
                order.append(t)
    return order


def table_mutant(text, seed):
    """The table automaton `text` with one more constraint that forbids one state its table reaches (no start state where
    another is reached): every solution prefix of the mutant is one of the original. The arrays are read back from the text."""
    arrays = {}
    for line in text.splitlines():
        if line.startswith("arr "):
            name, body = line[4:].split(":", 1)
            arrays[name.strip()] = [int(v) for v in body.strip(" {};").split(",")]
    two = "T1" in arrays
    B0 = int(text.split("var s0:[0,")[1].split("]")[0]) + 1 if two else len(arrays["G"])
    T = [hi * B0 + lo for hi, lo in zip(arrays["T1"], arrays["T0"])] if two else arrays["T"]
    S = len(arrays["G"])
    A = len(T) // S
    assert len(T) == S * A == len(arrays["OK"])
    rooted = ("first s0 == 0;" if two else "first s == 0;") in text
    order = _table_reach(T, arrays["OK"], A, [0] if rooted else list(range(B0)))
    later = order[1 if rooted else B0:] or order
    k = later[_inst.SplitMix64(0x7AB1E000 + seed).below(len(later))]
    if two:
        return text + f"((s1 ne {k // B0}) or (s0 ne {k % B0})) == 1;\n"
    return text + f"(s ne {k}) == 1;\n"


def table_by_name(name):
    """`table:<seed>:<digits>:<letters>:<keep>:<goal>[:unrooted][:<colours>]`, digits as `20` or `32x33`: its model text."""
    kind, seed, digits, letters, keep, goal, *rest = name.split(":")
    assert kind == "table" and all(x == "unrooted" or x.isdigit() for x in rest)
    colours = [int(x) for x in rest if x.isdigit()]
    return table_automaton(int(seed), tuple(int(b) for b in digits.split("x")), int(letters), int(keep), int(goal),
                           rooted="unrooted" not in rest, colours=colours[0] if colours else 2)
