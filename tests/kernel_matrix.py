"""The table of kernels that select_kernels() (stcsp-solver_amd/csrc/engine.hip) can return, with one model per cell.

Enumerated from the rule table in the comment above `struct Kernels` and the code below it, not from a run. Expansion cells:

    (L, CS, LITE) x DR 1/2/4                                   24
    big workgroup (needs L and LITE), CS 0/1 x DR 1/2/4         6
    one-register shape                                          1
    prefix x DR 1/2/4                                           3
    wide domains: W 2 / 4 / intervals x DR 1/2/4                9
    long key (DR 4, KR 2): plain, CS, W2, W4, intervals         5
    large block (DR 8): plain, CS, W2, W4 x KR 1/2              8
    until-heavy: DR 4/8 x plain, CS, W2, W4 x KR 1/2           16
    until-heavy with intervals, DR 4 x KR 1/2                   2
    big scope: DR 4/8 x plain, CS, W2, W4 x KR 1/2             16
                                                               --
                                                               90 compiled, 2 of them reachable by no model (UNREACHABLE)

Beside them 30 probe kernels (k_probe<DR, L, CS, LITE> at DR <= 4: 24, k_probe<8, false, CS, false>: 2, k_probe_big<DR, CS>: 4)
and 10 commit kernels (k_commit<DR, 1>: 4, k_commit<4|8, 2>: 2, k_commit_until<4|8, 1|2>: 4).

A row names its cell (every field of Engine.kernel_choice()), and carries a function that builds the smallest model text that
reaches the cell, `prefix_k`, engine flags and the engine's own tuning switches (STCSP_LITE, STCSP_IMG_LDS, STCSP_BIG,
STCSP_LITE_SHAPE) that step a model down to a plainer variant. The knobs:

  * block words N*K*W (intervals: 2*N*K) pick DR: <= 64 one register, <= 128 two, <= 256 four (three round up), <= 512 eight;
    padding variables `var zz<i>:[0,0]` (no constraint, no item) move a model between them;
  * the widest domain picks W; a chain of constant signature words and until flags make the key longer than 64 words;
    more than 32 until constraints pick the until family, one constraint over more than 64 variables the big-scope one;
  * more than 128 lane-revised items in one set pick CS: `ties` adds implied binary constraints over a few booleans.

Plain Python, no GPU: tests/test_kernel_matrix.py checks every row against the oracle alone, tests/test_kernel_matrix_gpu.py
runs them."""
import importlib
import re
from collections import namedtuple

from test_big_scope_gpu import big
from test_large_block_gpu import COUNTER, bools, chain, token_ring
from test_long_signature_gpu import until_model
from test_many_until import many_until

st = importlib.import_module("stcsp-solver_amd")
inst = st.instances

KF = {"variant": st.KF_VARIANT, "prefix": st.KF_PREFIX, "wide": st.KF_WIDE_DOMAINS, "long_key": st.KF_LONG_KEY,
      "large_block": st.KF_LARGE_BLOCK, "until": st.KF_UNTIL_HEAVY, "big_scope": st.KF_BIG_SCOPE}
INTERVALS = 0  # domain_form of the interval kernels (W = 1, 2, 4 otherwise)

# An expansion cell: the template arguments of one k_expand / k_expand_until / k_expand_big instantiation.
Cell = namedtuple("Cell", "family dr form kr in_lds cs lite big shape")
Probe = namedtuple("Probe", "big dr in_lds cs lite")   # k_probe<DR, L, CS, LITE> / k_probe_big<DR, CS>
Commit = namedtuple("Commit", "until dr kr")           # k_commit<DR, KR> / k_commit_until<DR, KR, ..>


def compiled_cells():
    """Every expansion kernel select_kernels() names, from its rule table."""
    out = []
    for dr in (1, 2, 4):
        out += [Cell("variant", dr, 1, 1, l, cs, lite, 0, 0) for l in (0, 1) for cs in (0, 1) for lite in (0, 1)]
        out += [Cell("variant", dr, 1, 1, 1, cs, 1, 1, 0) for cs in (0, 1)]
        out += [Cell("prefix", dr, 1, 1, 1, 0, 0, 0, 0)]
        out += [Cell("wide", dr, form, 1, 0, 0, 0, 0, 0) for form in (2, 4, INTERVALS)]
    out += [Cell("variant", 1, 1, 1, 1, 0, 1, 0, 1)]
    four = [(1, 0), (1, 1), (2, 0), (4, 0)]  # "the four (CS, W)": W = 1 plain or compacted, W = 2, W = 4
    out += [Cell("long_key", 4, form, 2, 0, cs, 0, 0, 0) for form, cs in four + [(INTERVALS, 0)]]
    out += [Cell("large_block", 8, form, kr, 0, cs, 0, 0, 0) for form, cs in four for kr in (1, 2)]
    out += [Cell("until", dr, form, kr, 0, cs, 0, 0, 0) for dr in (4, 8) for form, cs in four for kr in (1, 2)]
    out += [Cell("until", 4, INTERVALS, kr, 0, 0, 0, 0, 0) for kr in (1, 2)]
    out += [Cell("big_scope", dr, form, kr, 0, cs, 0, 0, 0) for dr in (4, 8) for form, cs in four for kr in (1, 2)]
    return out


def compiled_probes():
    out = [Probe(0, dr, l, cs, lite) for dr in (1, 2, 4) for l in (0, 1) for cs in (0, 1) for lite in (0, 1)]
    out += [Probe(0, 8, 0, cs, 0) for cs in (0, 1)]
    return out + [Probe(1, dr, 0, cs, 0) for dr in (4, 8) for cs in (0, 1)]


def compiled_commits():
    return ([Commit(0, dr, 1) for dr in (1, 2, 4, 8)] + [Commit(0, dr, 2) for dr in (4, 8)] +
            [Commit(1, dr, kr) for dr in (4, 8) for kr in (1, 2)])


# Compiled, reachable by no model create() accepts. A big scope is a constraint over more than 64 variables, so N >= 65; at
# W = 4 the block then has N*K*W >= 65 * 1 * 4 = 260 words, more than the 256 that four registers hold: create() makes it DR = 8.
UNREACHABLE = {
    Cell("big_scope", 4, 4, 1, 0, 0, 0, 0, 0): "scope > 64 => N >= 65 => N*K*W >= 65*1*4 = 260 > 256 words",
    Cell("big_scope", 4, 4, 2, 0, 0, 0, 0, 0): "scope > 64 => N >= 65 => N*K*W >= 65*1*4 = 260 > 256 words",
}


# ---------------------------------------------------------------------------------------------------------------- model parts
def pad(n: int) -> str:
    """n variables of one value, under no constraint: block words and nothing else."""
    return "".join(f"var zz{i}:[0,0]; " for i in range(n))


def ties(n: int, items: int, name: str = "q") -> str:
    """n booleans that are all equal, said `items` times over distinct pairs: two solutions, `items` lane-revised items."""
    pairs = [(i, j) for d in range(1, n) for i in range(n - d) for j in [i + d]][:items]
    assert len(pairs) == items, (n, items)
    return "".join(f"var {name}{i}:[0,1]; " for i in range(n)) + "".join(f"{name}{i} == {name}{j}; " for i, j in pairs)


# Lane-revised items are (constraint, time point) pairs: 61 binary constraints are 122 items at K = 2 (no CS), 59 are 59 at K = 1
# (no CS, and at most 64: the one-register shape unless switched off).
SYNTH = (12, 8, 58, 3, 6)  # 15 variables, 61 constraints: refuted nodes, bisections
SYNTH_ONE_NEXT = (12, 8, 58, 1, 6)  # 13 variables, 59 constraints, one `next`: the core of the K = 1 rows (an aux variable is free there)


def synth(padding=0, cs=False, shape=SYNTH):
    """The synthetic core; cs: 70 more constraints over 13 booleans, 131 in all (262 items at K = 2)."""
    return lambda: inst.synthetic(*shape) + (ties(13, 70) if cs else "") + pad(padding)


def walker(top: int) -> str:
    """A walker over top + 1 values whose step two small variables choose (s != t beside s + t == 3: refuted halves), with an until."""
    return (f"var x:[0,{top}]; var s:[0,3]; var t:[0,3]; var g:[0,1]; var y:[0,1]; first x == 0; "
            f"next x == (if (x ge {top}) then 0 else (x + 1 + (s gt t))); s != t; s + t == 3; y == (x ge {top - 1}); g until y; ")


Row = namedtuple("Row", "name cell text prefix_k flags env probe commit words key untils scope need_fail note")
ROWS = []


def row(name, cell, text, *, k=2, intervals=False, env=None, words=None, key=None, untils=0, scope=False,
        need_fail=True, note=""):
    """need_fail = False, with a note, is for the big-scope rows named in NO_FAIL only. The probe and commit kernels follow from the cell: the probe takes the (L, CS, LITE) variant of the program (the
    capacity families are general_only(): L = 0, LITE = 0; DR = 8 keeps CS only), k_probe_big under a big scope; the commit
    kernel takes DR and KR from the cell, k_commit_until with more than 32 until constraints."""
    fam = cell.family
    cs = cell.cs  # (the probe kernel's CS is the program's, like the expansion kernel's wherever that has a CS form)
    if fam == "big_scope":
        probe = Probe(1, cell.dr, 0, cs, 0)
    elif fam == "variant":
        probe = Probe(0, cell.dr, cell.in_lds, cs, cell.lite)
    else:  # the prefix family: a general program without CS whose image is not in LDS
        probe = Probe(0, cell.dr, 0, cs, 0)
    commit = Commit(int(fam == "until"), cell.dr, cell.kr)
    ROWS.append(Row(name, cell, text, k, st.F_INTERVAL_DOMAINS if intervals else 0, dict(env or {}), probe, commit, words, key, untils,
                    scope, need_fail, note))


# ------------------------------------------------------------------------------------------- the (L, CS, LITE) variants et al.
def variant_env(l, lite, big=0, shape=0):
    env = {"STCSP_BIG": "2" if big else "0", "STCSP_LITE_SHAPE": "1" if shape else "0"}
    if not l:
        env["STCSP_IMG_LDS"] = "0"
    if not lite:
        env["STCSP_LITE"] = "0"
    return env


# (DR, CS) -> (padding, K, block words). One block per DR at its upper bound (64, 128, 256) and one just above the lower one
# (65, 129): 15 + 17 = 32 variables at K = 2; 13 + 52 = 65 at K = 1; 28 + 36 = 64 at K = 2; 13 + 116 = 129 at K = 1;
# 28 + 100 = 128 at K = 2.
VARIANT_MODELS = {(1, 0): (17, 2, 64), (1, 1): (0, 2, 56), (2, 0): (52, 1, 65), (2, 1): (36, 2, 128), (4, 0): (116, 1, 129), (4, 1): (100, 2, 256)}
for dr in (1, 2, 4):
    for cs in (0, 1):
        padding, K, words = VARIANT_MODELS[dr, cs]
        core = SYNTH_ONE_NEXT if K == 1 else SYNTH
        for l in (0, 1):
            for lite in (0, 1):
                row(f"variant_dr{dr}_l{l}_cs{cs}_lite{lite}", Cell("variant", dr, 1, 1, l, cs, lite, 0, 0), synth(padding, cs, core), k=K,
                    env=variant_env(l, lite), words=words)
        row(f"bigwg_dr{dr}_cs{cs}", Cell("variant", dr, 1, 1, 1, cs, 1, 1, 0), synth(padding, cs, core), k=K, env=variant_env(1, 1, big=1), words=words)
row("shape1", Cell("variant", 1, 1, 1, 1, 0, 1, 0, 1), synth(shape=SYNTH_ONE_NEXT), k=1, env=variant_env(1, 1, shape=1), words=13)


# prefix: a general program (a ternary sum has more than one violating tuple) whose tables do not fit LDS beside the scratch but
# whose descriptors do: 16 sums over three variables of 32 values, one 4-KB bitmap each (different constants: no shared table).
# A counter p over 32 values fixes a0 .. a3 through binary constraints; the sums hold for every solution. The refuted nodes are
# walker's: s and t choose p's step (s != t beside s + t == 3), and the half with s > t has no successor at p = 30.
def prefix_model(padding):
    def text():
        t = "var s:[0,3]; var t:[0,3]; var p:[0,31]; first p == 0; next p == (if (p ge 31) then 0 else (p + 1 + (s gt t))); s != t; s + t == 3; "
        t += "var u:[0,3]; var v:[0,3]; u != v; u + v == 3; (p % 4) + 2 * (u gt v) <= 4; "  # (... and the half with u > v at every fourth p)
        t += "".join(f"var a{i}:[0,31]; a{i} == {'p' if i % 2 == 0 else '31 - p'}; " for i in range(4))
        t += "".join(f"a{i % 4} + a{(i + 1) % 4} + p <= {62 + i}; a{i % 4} + 2 * a{(i + 1) % 4} + {i} >= p; " for i in range(8))
        return t + pad(padding)
    return text


for dr, padding, words in [(1, 22, 64), (2, 23, 66), (4, 55, 130)]:  # N = 10 + padding, K = 2
    row(f"prefix_dr{dr}", Cell("prefix", dr, 1, 1, 1, 0, 0, 0, 0), prefix_model(padding), env={"STCSP_BIG": "0"}, words=words)

# ------------------------------------------------------------------------------------------------------------- wide domains
# walker(top): x, s, t, g, y and the aux variable of `next x`: N = 6
for form, top in [(2, 40), (4, 100), (INTERVALS, 200)]:
    for dr in (1, 2, 4):
        per = 2 if form == INTERVALS else form     # block words per variable and time point
        lo = {1: 1, 2: 65, 4: 129}[dr]
        n = max(6, -(-lo // (per * 2)))             # the fewest variables whose block needs DR registers at K = 2
        if dr == 4 and form == 4:
            n = 32                                   # 32 * 2 * 4 = 256 words: the upper bound
        row(f"wide_w{form}_dr{dr}", Cell("wide", dr, form, 1, 0, 0, 0, 0, 0), (lambda top=top, n=n: walker(top) + pad(n - 6)),
            intervals=form == INTERVALS, words=n * 2 * per, untils=1)

# ----------------------------------------------------------------------------------------------------------------- long key
# until_model(c, u): N = c + 6, a key of c + u + 2 words
row("long_key_plain_kl65", Cell("long_key", 4, 1, 2, 0, 0, 0, 0, 0), lambda: until_model(31, 32), words=2 * 37, key=65, untils=32)
row("long_key_cs_kl126", Cell("long_key", 4, 1, 2, 0, 1, 0, 0, 0), lambda: until_model(94, 30) + ties(17, 130), words=2 * 117, key=126, untils=30)
row("long_key_w2", Cell("long_key", 4, 2, 2, 0, 0, 0, 0, 0), lambda: until_model(31, 32, 40), words=37 * 4, key=65, untils=32)
row("long_key_w4", Cell("long_key", 4, 4, 2, 0, 0, 0, 0, 0), lambda: until_model(31, 32, 100), k=1, words=37 * 4, key=65, untils=32)
row("long_key_intervals", Cell("long_key", 4, INTERVALS, 2, 0, 0, 0, 0, 0), lambda: until_model(31, 32, 200), intervals=True, words=37 * 4,
    key=65, untils=32)

# -------------------------------------------------------------------------------------------------------------- large block
row("block8_plain_257", Cell("large_block", 8, 1, 1, 0, 0, 0, 0, 0), lambda: bools(30) + walker(3) + pad(219), k=1, words=257, untils=1)
row("block8_cs", Cell("large_block", 8, 1, 1, 0, 1, 0, 0, 0), lambda: bools(140) + walker(3), words=296, untils=1)
row("block8_plain_kr2", Cell("large_block", 8, 1, 2, 0, 0, 0, 0, 0), lambda: until_model(50, 30) + pad(80), words=2 * 136, key=82, untils=30)
row("block8_cs_kr2", Cell("large_block", 8, 1, 2, 0, 1, 0, 0, 0), lambda: until_model(50, 30) + ties(17, 130) + pad(60), words=2 * 133, key=82,
    untils=30)
row("block8_w2", Cell("large_block", 8, 2, 1, 0, 0, 0, 0, 0), lambda: walker(40) + pad(59), words=65 * 4, untils=1)
row("block8_w4", Cell("large_block", 8, 4, 1, 0, 0, 0, 0, 0), lambda: walker(100) + pad(58), words=64 * 8, untils=1)
row("block8_w2_kr2", Cell("large_block", 8, 2, 2, 0, 0, 0, 0, 0), lambda: until_model(31, 32, 40) + pad(28), words=65 * 4, key=65, untils=32)
row("block8_w4_kr2", Cell("large_block", 8, 4, 2, 0, 0, 0, 0, 0), lambda: until_model(31, 32, 100), words=37 * 8, key=65, untils=32)


# -------------------------------------------------------------------------------------------------------------- until-heavy
def few_until(u: int, top: int) -> str:
    """many_until in 14 variables: the counter p over [0, top] with its aux, eight y_b (1 when p is at b * top // 7), g_0 .. g_3;
    until i is `g_(i % 4) until y_(i % 8)`."""
    t = f"var p:[0,{top}]; first p == 0; next p == (if (p lt {top}) then (p + 1) else 0); "
    t += "".join(f"var y{b}:[0,1]; y{b} == (p eq {b * top // 7}); " for b in range(8)) + "".join(f"var g{a}:[0,1]; " for a in range(4))
    return t + "".join(f"g{i % 4} until y{i % 8}; " for i in range(u))


# many_until(u, top, pad): N = 36 + pad for u = 33 and 63, a key of 2 + u words; its 32 y_b at two time points and the u until
# items are more than 128 items at u = 63 (CS), so the KR = 2 rows without CS take few_until's eight; W = 4 in four registers,
# N*K*4 <= 256, has no room for 36 variables at K = 2 either. KR = 1: u = 33, KR = 2: u = 63 (a key of 65 words).
def heavy(fn, *args, extra="", padding=0, **kw):
    return lambda: fn(*args, **kw) + extra + pad(padding)


UNTIL_HEAVY = [
    # name            cell (dr, form, kr, cs)   builder                                                     words
    ("dr4_plain_kr1", (4, 1, 1, 0), heavy(many_until, 33), 2 * 36),
    ("dr4_plain_kr2", (4, 1, 2, 0), heavy(few_until, 63, 31), 2 * 14),
    ("dr4_cs_kr1", (4, 1, 1, 1), heavy(many_until, 33, extra=ties(17, 100)), 2 * 53),
    ("dr4_cs_kr2", (4, 1, 2, 1), heavy(many_until, 63, extra=ties(17, 100)), 2 * 53),
    ("dr4_w2_kr1", (4, 2, 1, 0), heavy(many_until, 33, top=62), 4 * 36),
    ("dr4_w2_kr2", (4, 2, 2, 0), heavy(many_until, 63, top=62), 4 * 36),
    ("dr4_w4_kr1", (4, 4, 1, 0), heavy(few_until, 33, 124), 8 * 14),
    ("dr4_w4_kr2", (4, 4, 2, 0), heavy(few_until, 63, 124), 8 * 14),
    ("dr4_intervals_kr1", (4, INTERVALS, 1, 0), heavy(many_until, 33, top=200), 4 * 36),
    ("dr4_intervals_kr2", (4, INTERVALS, 2, 0), heavy(many_until, 63, top=200), 4 * 36),
    ("dr8_plain_kr1", (8, 1, 1, 0), heavy(many_until, 33, padding=95), 2 * 131),
    ("dr8_plain_kr2", (8, 1, 2, 0), heavy(few_until, 63, 31, padding=120), 2 * 134),
    ("dr8_cs_kr1", (8, 1, 1, 1), heavy(many_until, 33, extra=ties(17, 100), padding=95), 2 * 148),
    ("dr8_cs_kr2", (8, 1, 2, 1), heavy(many_until, 63, extra=ties(17, 100), padding=95), 2 * 148),
    ("dr8_w2_kr1", (8, 2, 1, 0), heavy(many_until, 33, top=62, padding=30), 4 * 66),
    ("dr8_w2_kr2", (8, 2, 2, 0), heavy(many_until, 63, top=62, padding=30), 4 * 66),
    ("dr8_w4_kr1", (8, 4, 1, 0), heavy(many_until, 33, top=124), 8 * 36),
    ("dr8_w4_kr2", (8, 4, 2, 0), heavy(many_until, 63, top=124), 8 * 36),
]
for name, (dr, form, kr, cs), text, words in UNTIL_HEAVY:
    u = 33 if kr == 1 else 63
    row(f"until_{name}", Cell("until", dr, form, kr, 0, cs, 0, 0, 0), text, intervals=form == INTERVALS, words=words, key=2 + u, untils=u)


# ---------------------------------------------------------------------------------------------------------------- big scope
# chain(n) with one big constraint over all of it beside the counter c, which asks for a 1 at the chain's end now and then and
# for a 0 at its start. top: a variable of top + 1 values that follows the counter (W = 2 / 4; no `next` of its own: at K = 1 an
# aux variable is free over its whole domain). KR = 2: until_model(32, 32) in front, a key of 66 words, its counter p for c.
def scoped(n, kind="sum", top=0, long_key=False, extra="", padding=0):
    def text():
        t = chain(n, 1, ("<=", "==", "==")) + big(kind, [f"x{i}" for i in range(n)])
        c = "p" if long_key else "c"
        t += until_model(32, 32) if long_key else COUNTER
        t += f"x{n - 1} >= ({c} eq 3); x0 <= ({c} ne 1); "
        if top:
            t += f"var w:[0,{top}]; w == {top // 3} * {c}; "
        return t + extra + pad(padding)
    return text


# N: chain + 2 (counter or walker, its aux); with the long key chain + 38
BIG_SCOPE = [
    # name            cell (dr, form, kr, cs)   builder                                          K  words       key
    # (the chain's 64 links at two time points are 128 items: the rows without CS run at K = 1)
    ("dr4_plain_kr1", (4, 1, 1, 0), scoped(65, "sum"), 1, 67, None),
    ("dr4_cs_kr1", (4, 1, 1, 1), scoped(120, "if"), 2, 2 * 122, None),  # (no refuted node: see NO_FAIL)
    ("dr4_w2_kr1", (4, 2, 1, 0), scoped(65, "sum", top=40), 1, 2 * 68, None),
    ("dr4_plain_kr2", (4, 1, 2, 0), scoped(65, "if", long_key=True), 1, 103, 66),
    ("dr4_cs_kr2", (4, 1, 2, 1), scoped(65, "sum", long_key=True, extra=ties(12, 66)), 2, 2 * 115, 66),
    ("dr4_w2_kr2", (4, 2, 2, 0), scoped(65, "and", top=40, long_key=True), 1, 2 * 104, 66),
    ("dr8_plain_kr1", (8, 1, 1, 0), scoped(65, "sum", padding=190), 1, 257, None),
    ("dr8_cs_kr1", (8, 1, 1, 1), scoped(200, "and"), 2, 2 * 202, None),
    ("dr8_w2_kr1", (8, 2, 1, 0), scoped(80, "or", top=40), 2, 4 * 83, None),
    ("dr8_w4_kr1", (8, 4, 1, 0), scoped(65, "and", top=100), 1, 4 * 68, None),
    ("dr8_plain_kr2", (8, 1, 2, 0), scoped(65, "or", long_key=True, padding=160), 1, 263, 66),
    ("dr8_cs_kr2", (8, 1, 2, 1), scoped(65, "if", long_key=True, extra=ties(12, 66), padding=100), 2, 2 * 215, 66),
    ("dr8_w2_kr2", (8, 2, 2, 0), scoped(65, "sum", top=40, long_key=True), 2, 4 * 104, 66),
    ("dr8_w4_kr2", (8, 4, 2, 0), scoped(65, "and", top=100, long_key=True), 1, 4 * 104, 66),
]
# the big-scope rows whose oracle run refutes no node; what it does fulfil is stated here and asserted by the CPU test
NO_FAIL = {"dr4_cs_kr1": "an `if` over 120 flags keeps a support until its last flag is fixed: bisections and revisited states only"}
for name, (dr, form, kr, cs), text, K, words, key in BIG_SCOPE:
    row(f"big_scope_{name}", Cell("big_scope", dr, form, kr, 0, cs, 0, 0, 0), text, k=K, words=words, key=key, untils=32 if kr == 2 else 0,
        scope=True, need_fail=name not in NO_FAIL, note=NO_FAIL.get(name, ""))


ROW = {r.name: r for r in ROWS}
# one row per commit kernel
COMMIT_ROWS = ["variant_dr1_l1_cs0_lite1", "variant_dr2_l1_cs0_lite1", "variant_dr4_l1_cs0_lite1", "block8_cs", "long_key_w2", "block8_plain_kr2",
               "until_dr4_plain_kr1", "until_dr4_w2_kr2", "until_dr8_cs_kr1", "until_dr8_plain_kr2"]
# one row per family and DR for the run with small pools and 64-node batches (records of every stride)
SMALL_POOL_ROWS = ["variant_dr1_l1_cs1_lite1", "variant_dr2_l0_cs0_lite0", "variant_dr4_l1_cs0_lite0", "bigwg_dr2_cs1", "shape1", "prefix_dr1", "prefix_dr2",
                   "prefix_dr4", "wide_w2_dr1", "wide_w0_dr2", "wide_w4_dr4", "long_key_w4", "block8_cs_kr2", "until_dr4_intervals_kr2",
                   "until_dr8_w4_kr1", "big_scope_dr4_w2_kr2", "big_scope_dr8_w4_kr2"]


def choice(r: Row) -> dict:
    """What Engine.kernel_choice() must return for the row: every field."""
    c = r.cell
    return {"family": KF[c.family], "dom_regs": c.dr, "domain_form": c.form, "key_regs": c.kr, "image_in_lds": c.in_lds,
            "compact_sweeps": c.cs, "lite": c.lite, "big_workgroup": c.big, "one_register_shape": c.shape,
            "expand_threads": 1024 if c.big else 256, "probe_family": st.KP_PROBE_BIG if r.probe.big else st.KP_PROBE,
            "probe_image_in_lds": r.probe.in_lds, "probe_compact_sweeps": r.probe.cs, "probe_lite": r.probe.lite,
            "commit_family": st.KC_COMMIT_UNTIL if r.commit.until else st.KC_COMMIT, "commit_key_regs": r.commit.kr}


def seam_ok(r: Row) -> bool:
    """The node-level seam (Engine.propagate) takes the row's model: W = 1, no intervals, at most 32 until constraints."""
    return r.cell.form == 1 and r.untils <= 32


def block_words(m, k: int, intervals: bool) -> int:
    w = max(hi - lo + 1 for lo, hi in m.var_bounds())
    return m.n_vars * k * (2 if intervals else 1 if w <= 32 else 2 if w <= 64 else 4)


def dom_regs(words: int) -> int:
    return 1 if words <= 64 else 2 if words <= 128 else 4 if words <= 256 else 8


def seam_inputs(r: Row, m, count: int = 64):
    """The blocks of the row's probe test: seam_blocks for a big scope (at most 10 of its variables open: every revision exact),
    else random_blocks with, in every second block, two more open words of time point 0 fixed to one value each (padding
    variables take most of random_blocks' own restrictions)."""
    import numpy as np
    from test_big_scope_gpu import seam_blocks
    from test_propagate_gpu import random_blocks
    rng = np.random.default_rng(20261019)
    if r.scope:
        return seam_blocks(m, sum(1 for v in m.var_names if re.fullmatch(r"x\d+", v)), r.prefix_k, rng, count)
    blocks = random_blocks(m, r.prefix_k, rng, count)
    open_words = [v for v, (lo, hi) in enumerate(m.var_bounds()) if hi > lo]
    for i in range(0, count, 2):
        for v in rng.choice(open_words, size=2, replace=False):
            bits = [b for b in range(32) if (int(blocks[i, v]) >> b) & 1]
            blocks[i, v] = 1 << bits[int(rng.integers(0, len(bits)))]
    return blocks
