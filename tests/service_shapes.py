"""The catalogue of export shapes the automaton services are run on (tests/test_service_shapes.py on the CPU oracle's automaton,
tests/test_service_shapes_gpu.py on the engine's own export): the shapes of `d_oval[E][N]`, `d_state_keys[S][KL]`, `n_sig`,
`n_until`, the bounds and the mask that the services' kernels index by hand, beyond the one shape every other service test has
(a dozen variables, a key far below 64 words, a few until flags, K = 2, small non-negative values).

One entry per shape: the model text, `prefix_k`, the engine flags, the row of tests/kernel_matrix.py it is taken from (with the
row's tuning switches; the device test asserts that row's whole Engine.kernel_choice()) or, for the others, the key registers,
block registers and domain form to assert; one extra constraint line that makes its compare mutant (it only forbids); the one or
two variables that carry its behaviour and its last padding variable; and the floors the CPU oracle's automaton has to keep, the
facts the shape is in the list for. Plain Python, no GPU."""
import importlib
from collections import namedtuple

import kernel_matrix as km
from test_long_signature_gpu import RINGS

st = importlib.import_module("stcsp-solver_amd")

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1

# A toggle s under interval domains; v and u take the ends of int32 on live edges: v is INT_MIN / INT_MAX, u is INT_MIN + 1 / -1.
# f is free: two edges per state. (INT_MIN on an edge is a value like any other; in an input row it means "not observed".)
# Not among SHAPES: the CPU oracle searches supports value by value and does not finish a variable over the whole int range, so
# this model has no oracle automaton; the device test runs twin and yardsticks on the engine's own export of it.
ENDS = (f"var s:[0,1]; var v:[{INT_MIN},{INT_MAX}]; var u:[{INT_MIN + 1},-1]; var f:[0,1]; first s == 0; next s == 1 - s; "
        f"v == (if (s eq 0) then {INT_MIN} else {INT_MAX}); u == (if (s eq 0) then {INT_MIN + 1} else -1); ")

# name, text (a function), prefix_k, engine flags, kernel-matrix row name or None, environment of the row, (key_regs, dom_regs,
# domain_form) to assert where there is no row, the mutant's extra line, behaviour variable names, last padding variable or None,
# floors: {figure: least value} on the oracle's automaton (figures of shape_of() below), exact: {figure: value}
Shape = namedtuple("Shape", "name text prefix_k flags row env regs mutant behaviour pad floors exact note")
SHAPES = []


def shape(name, *, row=None, text=None, k=None, flags=0, regs=None, mutant, behaviour, pad=None, floors=None, exact=None, note=""):
    r = km.ROW[row] if row else None
    assert (r is None) != (text is None) and (r is None) == (regs is not None)
    SHAPES.append(Shape(name, r.text if r else text, r.prefix_k if r else k, r.flags if r else flags, row, dict(r.env) if r else {}, regs,
                        mutant, behaviour, pad, dict(floors or {}), dict(exact or {}), note))


# ---- keys and until flags
shape("until_dr4_plain_kr2", row="until_dr4_plain_kr2", mutant="(p eq 3) -> (g0 eq 1); ", behaviour="p,g0",
      floors=dict(live=64, final=1, nonfinal=1), exact=dict(n_vars=14, key=65, untils=63),
      note="a key of 65 words whose 63 until flags differ from state to state: KR = 2, flags across key word 64")
shape("until_dr4_plain_kr1", row="until_dr4_plain_kr1", mutant="(p eq 3) -> (g0 eq 1); ", behaviour="p,g0",
      floors=dict(live=64), exact=dict(n_vars=36, key=35, untils=33), note="33 until flags in one key register: one more than a flag word holds")
shape("until_dr8_cs_kr2", row="until_dr8_cs_kr2", mutant="(p eq 3) -> (g0 eq 1); ", behaviour="p,g0", pad="zz94",
      floors=dict(live=64), exact=dict(n_vars=148, key=65, untils=63), note="N > 128 with 63 flags and KR = 2, DR = 8")
shape("until_dr4_intervals_kr2", row="until_dr4_intervals_kr2", mutant="(p eq 3) -> (g0 eq 1); ", behaviour="p,g0",
      floors=dict(live=256), exact=dict(n_vars=36, key=65, untils=63), note="interval domains, 201 values, under a key of 65 words")
shape("long_key_intervals", row="long_key_intervals", mutant="(p eq 1) -> (b eq 0); ", behaviour="p,b",
      floors=dict(live=256), exact=dict(n_vars=37, key=65, untils=32), note="interval domains, 32 flags that end at key word 64")
shape("long_key_cs_kl126", row="long_key_cs_kl126", mutant="(p eq 1) -> (b eq 0); ", behaviour="p,b", pad="q16",
      floors=dict(live=6), exact=dict(n_vars=117, key=126, untils=30), note="the longest key, 126 words, the flags at its end")
shape("ring125", text=lambda: RINGS["ring125"], k=2, regs=(2, 4, 1), mutant="(x0 eq 2) -> (b eq 0); ", behaviour="x0,b",
      floors=dict(live=6), exact=dict(key=126, untils=0), note="a key of 126 words with the counter in its last word")
# ---- label rows
shape("prefix_dr4", row="prefix_dr4", mutant="(p eq 5) -> (s lt t); ", behaviour="p,s", pad="zz54",
      floors=dict(live=32), exact=dict(n_vars=65), note="N = 65: one variable past a 64-bit mask word")
shape("variant_dr4_l1_cs1_lite1", row="variant_dr4_l1_cs1_lite1", mutant="x0 != 3; ", behaviour="x0,x1", pad="zz99",
      floors=dict(removed=1), exact=dict(n_vars=128), note="N = 128, and states the traverse removes")
shape("big_scope_dr8_plain_kr2", row="big_scope_dr8_plain_kr2", mutant="(p eq 1) -> (b eq 0); ", behaviour="p,b", pad="zz159",
      floors=dict(live=8), exact=dict(n_vars=263, key=66, untils=32), note="K = 1, N = 263, DR = 8, KR = 2")
shape("block8_w4", row="block8_w4", mutant="(x eq 5) -> (s lt t); ", behaviour="x,s", pad="zz57",
      floors=dict(live=128), exact=dict(n_vars=64), note="W = 4 at DR = 8: 101 values, N = 64 exactly")
# ---- prefix length 3
shape("few_until_k3", text=lambda: km.few_until(40, 31), k=3, regs=(1, 4, 1), mutant="(p eq 3) -> (g0 eq 1); ", behaviour="p,g0",
      floors=dict(live=64, final=1, nonfinal=1), exact=dict(untils=40), note="K = 3: two signature words per `next`, 40 until flags behind them")



def late_flags(u: int = 40, top: int = 31) -> str:
    """u until constraints, each with a right-hand variable of its own (the traverse reads one flag per distinct right-hand
    variable: `n_until`, not `n_until_cons`). The first 32 expire together early (p == 2), the others one by one later (p == 10,
    12, ..): between the two a state has its first 32 flags set and later ones clear, so it is final only for a reader that stops
    after 32 flags. The models of tests/kernel_matrix.py have at most 32 distinct right-hand variables: their loop ends at 32."""
    t = f"var p:[0,{top}]; first p == 0; next p == (if (p lt {top}) then (p + 1) else 0); "
    t += "".join(f"var ya{i}:[0,1]; ya{i} == (p eq 2); " for i in range(32))
    t += "".join(f"var yb{j}:[0,1]; yb{j} == (p eq {10 + 2 * j}); " for j in range(u - 32)) + "var g0:[0,1]; var g1:[0,1]; "
    return t + "".join(f"g0 until ya{i}; " for i in range(32)) + "".join(f"g1 until yb{j}; " for j in range(u - 32))


shape("late_flags", text=late_flags, k=2, regs=(1, 4, 1), mutant="(p eq 3) -> (g0 eq 1); ", behaviour="p,g0",
      floors=dict(live=57, final=32, nonfinal=25), exact=dict(n_vars=44, key=42, untils=40),
      note="flags of ordinal 32 and above that are still clear when the first 32 are set")

BY_NAME = {s.name: s for s in SHAPES}
NAMES = [s.name for s in SHAPES]
PREFIX = "shape:"  # the name the helpers of the other files find the text under


def key_of(name):
    return PREFIX + name


def mutant_key(name):
    return PREFIX + "mutant:" + name


TEXT = {}
for _s in SHAPES:
    TEXT[key_of(_s.name)] = _s.text()
    TEXT[mutant_key(_s.name)] = TEXT[key_of(_s.name)] + _s.mutant + "\n"
K_OF = {key: BY_NAME[key.split(":")[-1]].prefix_k for key in TEXT}

# ------------------------------------------------------------------------------------------------------------------------- masks
MASKS = ("default", "all", "hidden", "last", "high", "behaviour")
MASK_GROUPS = {"plain": MASKS[:3], "high": MASKS[3:]}


def behaviour_names(s):
    return s.behaviour + ("," + s.pad if s.pad else "")


def high_from(n):
    """The first index of the `high` mask: 64, 32 where N <= 64, and the upper half where N <= 32 (no variable of index 32)."""
    return 64 if n > 64 else 32 if n > 32 else n // 2


def extra_masks(s, var_names):
    """last: variable N - 1 alone; high: every variable from high_from(N) on; behaviour: the behaviour variables and the last
    padding variable."""
    n = len(var_names)
    names = behaviour_names(s).split(",")
    assert all(v in var_names for v in names), (s.name, names)
    return {"last": [int(i == n - 1) for i in range(n)], "high": [int(i >= high_from(n)) for i in range(n)],
            "behaviour": [int(v in names) for v in var_names]}


def masks_for(plain, s, names=MASKS):
    """A stand-in for monitor_ref.masks() while the shape `s` (or its mutant) is checked: the plain three and the three that reach
    the high indices, those of `names` only."""
    def masks(model, r):
        every = {**plain(model, r), **extra_masks(s, model.var_names)}
        return {k: every[k] for k in names}
    return masks


# ----------------------------------------------------------------------------------------------------------------------- figures
def figures(model, r, valid, final, alive, components_ref):
    """What the floors are about, of one automaton (a Result with its flags)."""
    ref = components_ref.yardstick(r, valid, final, alive)
    live = sorted(ref["num"])
    val = components_ref.Q.result_arrays(r)[2]
    values = set(val[[e for e in range(r.n_edges) if alive[e]]].ravel().tolist())
    return dict(n_vars=model.n_vars, k=model.problem.contents.prefix_k, key=1 + r.sig_len, untils=r.n_until_cons, live=len(live), edges=ref["counts"]["n_edges"],
                final=sum(1 for s in live if final[s]), nonfinal=sum(1 for s in live if not final[s]), removed=r.n_states - len(live),
                components=ref["counts"]["n_components"], values=values)


def large(f):
    """Where the plain Python recurrences are given fewer and shorter streams: they grow with edges x row length x stream length."""
    return f["edges"] > 500 or f["n_vars"] > 64


def huge(f):
    """Where even those take seconds per stream: the repair's recurrence is then given the fewest."""
    return f["edges"] * f["n_vars"] > 60000


def line(name, f):
    return (f"{name}: N {f['n_vars']} K {f['k']} key {f['key']} untils {f['untils']} live {f['live']} edges {f['edges']} final {f['final']} "
            f"non-final {f['nonfinal']} removed {f['removed']} components {f['components']}")


def check_floors(figs):
    """figs: {shape name: figures()} over the whole catalogue. Every shape keeps its own floors and exact figures, and the
    features of the table in DESIGN 4.10.1 are each reached by the shapes named there."""
    assert list(figs) == NAMES and 10 <= len(NAMES) <= 13
    for name, f in figs.items():
        s = BY_NAME[name]
        assert all(f[k] >= v for k, v in s.floors.items()), f"{name}: {f} below {s.floors}"
        assert all(f[k] == v for k, v in s.exact.items()), f"{name}: {f} is not {s.exact}"
        assert f["k"] == s.prefix_k

    def meet(names, cond):
        assert all(cond(figs[n]) for n in names), [(n, figs[n]) for n in names if not cond(figs[n])]
    meet(["until_dr4_plain_kr2"], lambda f: f["key"] > 64 and f["live"] >= 64 and f["final"] and f["nonfinal"])
    meet(["ring125", "long_key_cs_kl126"], lambda f: f["key"] == 126 and f["live"] >= 6)
    meet(["until_dr4_plain_kr1"], lambda f: 33 <= f["untils"] <= 63 and f["key"] <= 64 and f["live"] >= 64)
    meet(["until_dr4_plain_kr2"], lambda f: 33 <= f["untils"] <= 63 and f["key"] > 64 and f["live"] >= 64)
    meet(["prefix_dr4"], lambda f: f["n_vars"] > 64 and f["live"] >= 32)
    meet(["until_dr8_cs_kr2"], lambda f: f["n_vars"] > 128 and f["live"] >= 64)
    meet(["big_scope_dr8_plain_kr2"], lambda f: f["n_vars"] >= 257 and f["live"] >= 8 and f["edges"] <= 2000)
    meet(["variant_dr4_l1_cs1_lite1"], lambda f: f["n_vars"] >= 128 and f["removed"] >= 1)
    meet(["long_key_intervals", "until_dr4_intervals_kr2"], lambda f: f["key"] > 64 and f["live"] >= 256)
    meet(["block8_w4"], lambda f: f["live"] >= 128)
    assert any(f["k"] == 1 for f in figs.values()) and any(f["k"] == 3 for f in figs.values())
