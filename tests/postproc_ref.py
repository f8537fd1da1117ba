"""The independent yardstick of the post-search graph passes (tests only): traverse, adversarial and adversarial2 as
whole-set fixpoints over Python sets. It reads a Result, the variable bounds and nothing else; the host twin
(postproc.cpp) and the device kernels (dev_postproc.hpp) are both measured against it.

Definitions (state 0 is the root; an edge is (src, dst, one value per variable); every edge starts alive):

  final         final[v] = every until flag of v's signature is 1; final[0] = root_final.
  traverse      valid = the least set that contains final and is closed backwards over edges.
                An edge dies if (valid[src] or src == 0) and not valid[dst].
  adversarial   valid = the greatest subset of valid in which every state has, for every value of variable i, an alive
                edge with that value into the subset. Then an edge dies if valid[src] and not valid[dst].
  adversarial2  The alive edges of a state into valid states fall into classes by their `ava` value; a class is complete
                if it shows every value of `op`. To a fixpoint: a state without a complete class leaves valid; in a
                state with one, the edges of the incomplete classes die. The clean-up valid[src] and not valid[dst]
                runs only if the root stayed valid.

Both adversarial passes return valid[0]. What these definitions determine is the relation same_flags(): after
adversarial2 with an invalidated root no clean-up runs, and whether an edge from a kept state into an invalidated one was
thinned before its destination fell depends on the order of the visits."""
from collections import namedtuple

Graph = namedtuple("Graph", "n_states src dst rows out final")
Flags = namedtuple("Flags", "valid final alive ret")  # bytes, bytes, bytes, (adver1, adver2) with -1 = not run


def graph(r):
    """A Result as plain lists: edge arrays, label rows, the edge indices leaving every state, the final flags."""
    S, E, N = int(r.n_states), int(r.n_edges), int(r.n_vars)
    src = r.edge_src[:E] if E else []
    dst = r.edge_dst[:E] if E else []
    flat = r.edge_values[:E * N] if E else []
    rows = [flat[e * N:(e + 1) * N] for e in range(E)]
    out = [[] for _ in range(S)]
    for e in range(E):
        out[src[e]].append(e)
    L, c0, c1 = int(r.sig_len), int(r.n_sig_vars), int(r.n_sig_vars) + int(r.n_until)
    sig = r.state_sig[:S * L] if S * L else []
    final = {v for v in range(1, S) if all(sig[v * L + c] == 1 for c in range(c0, c1))}
    if r.root_final:
        final.add(0)
    return Graph(S, src, dst, rows, out, frozenset(final))


def values_of(bounds, i):
    lb, ub = bounds[i]
    return frozenset(range(lb, ub + 1))


def traverse(g):
    """-> (valid set, alive set of edge indices)."""
    valid = set(g.final)
    while True:
        more = {g.src[e] for e in range(len(g.src)) if g.dst[e] in valid} - valid
        if not more:
            break
        valid |= more
    alive = {e for e in range(len(g.src)) if not ((g.src[e] in valid or g.src[e] == 0) and g.dst[e] not in valid)}
    return valid, alive


def clean_up(g, valid, alive):
    return {e for e in alive if not (g.src[e] in valid and g.dst[e] not in valid)}


def adversarial(g, valid, alive, i, bounds):
    """-> (valid, alive, valid[0])."""
    need = values_of(bounds, i)
    valid = set(valid)
    while True:
        lose = {s for s in valid if not need <= {g.rows[e][i] for e in g.out[s] if e in alive and g.dst[e] in valid}}
        if not lose:
            break
        valid -= lose
    return valid, clean_up(g, valid, alive), int(0 in valid)


def adversarial2(g, valid, alive, op, ava, bounds):
    """-> (valid, alive, valid[0])."""
    need = values_of(bounds, op)
    valid, alive = set(valid), set(alive)
    while True:
        lose, dead = set(), set()
        for s in valid:
            classes = {}
            for e in g.out[s]:
                if e in alive and g.dst[e] in valid:
                    classes.setdefault(g.rows[e][ava], []).append(e)
            complete = {a for a, es in classes.items() if need <= {g.rows[e][op] for e in es}}
            if not complete:
                lose.add(s)
            else:
                dead.update(e for a, es in classes.items() if a not in complete for e in es)
        if not lose and not dead:
            break
        valid -= lose
        alive -= dead
    if 0 in valid:
        alive = clean_up(g, valid, alive)
    return valid, alive, int(0 in valid)


def pack(g, valid, alive, ret):
    return Flags(bytes(int(v in valid) for v in range(g.n_states)), bytes(int(v in g.final) for v in range(g.n_states)),
                 bytes(int(e in alive) for e in range(len(g.src))), ret)


def run(g, bounds, adv=-1, adv2=None, start=None):
    """traverse [+ adversarial(adv)] [+ adversarial2(*adv2)] on one automaton, like postprocess(). `start` is the
    (valid, alive) of an earlier traverse(g), to spare its repetition."""
    valid, alive = start if start is not None else traverse(g)
    r1 = r2 = -1
    if adv >= 0:
        valid, alive, r1 = adversarial(g, valid, alive, adv, bounds)
    if adv2:
        valid, alive, r2 = adversarial2(g, valid, alive, adv2[0], adv2[1], bounds)
    return pack(g, valid, alive, (r1, r2))


def first_difference(got, want, src, dst, after_adv2):
    """"" if `got` and `want` (Flags) agree on everything the definitions determine, else what differs first."""
    if got.final != want.final:
        return "final flags differ"
    if got.valid != want.valid:
        return f"valid flags differ at state {next(v for v in range(len(want.valid)) if got.valid[v:v + 1] != want.valid[v:v + 1])}"
    if tuple(got.ret) != tuple(want.ret):
        return f"return values differ: {tuple(got.ret)} != {tuple(want.ret)}"
    if len(got.alive) != len(want.alive):
        return "edge counts differ"
    if got.alive == want.alive:
        return ""
    valid = want.valid
    for e in range(len(want.alive)):
        if after_adv2 and not (valid[src[e]] and (valid[0] or valid[dst[e]])):
            continue
        if bool(got.alive[e]) != bool(want.alive[e]):
            return f"edge_alive differs at edge {e} ({src[e]} -> {dst[e]}): {got.alive[e]} != {want.alive[e]}"
    return ""


def same_flags(got, want, src, dst, after_adv2):
    """The determined relation: valid and final bit-identical, the return values equal, edge_alive equal on all edges
    after traverse / adversarial, and after adversarial2 on the edges with valid[src] and (valid[0] or valid[dst])."""
    return not first_difference(got, want, src, dst, after_adv2)


def post_flags(post):
    """A PostResult as Flags (copies)."""
    S, E = int(post.n_states), int(post.n_edges)
    return Flags(bytes(post.state_valid[:S]), bytes(post.state_final[:S]), bytes(post.edge_alive[:E]) if E else b"",
                 (post.adver1, post.adver2))


def host_flags(a, ret):
    """The flags of a host Automaton as Flags."""
    v, f, al = a.flags()
    return Flags(v, f, al, ret)


class Tally:
    """What a fuzz exercised, counted on the yardstick's results: the floors that keep it from going trivial."""

    def __init__(self):
        self.models = self.traverse_partial = self.adv_runs = self.adv_partial = 0
        self.adv2_runs = self.adv2_partial = self.adv2_thinning = 0

    def traverse(self, g, t):
        self.models += 1
        self.traverse_partial += 0 < t.valid.count(1) < g.n_states

    def adv(self, t, f):
        self.adv_runs += 1
        self.adv_partial += 0 < f.valid.count(1) < t.valid.count(1)

    def adv2(self, g, t, f):
        self.adv2_runs += 1
        self.adv2_partial += 0 < f.valid.count(1) < t.valid.count(1)
        self.adv2_thinning += any(t.alive[e] and not f.alive[e] and f.valid[g.src[e]] and f.valid[g.dst[e]] for e in range(len(g.src)))

    def __iadd__(self, o):
        for k, v in vars(o).items():
            setattr(self, k, getattr(self, k) + v)
        return self

    def __repr__(self):
        return " ".join(f"{k}={v}" for k, v in vars(self).items())
