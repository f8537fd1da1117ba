"""The independent yardstick of the stream inference (tests only), in plain Python over quotient_ref.live_out_edges, whose
lists are already in canonical order (sorted by full row).

Definition (include/stcsp_engine.h, stcsp_engine_infer): an edge matches a step iff it carries every observed value;
B_0 = 1 on the live states (final[s] with end_final), B_{r+1}(s) = the sum of B_r(dst) over the matching live out-edges in
canonical order; count = B_len(root); an edge is feasible at step t iff its source is in F_t, it matches and its
destination has weight to go; the support of (t, v) is the set of values the feasible edges carry.

Two implementations that share nothing but the edge lists: dp() is the contract's recurrences in Python floats, one
operation at a time, so bit for bit the contract's; brute() enumerates every live path of the stream's length in
lexicographic order of the full rows, filters by the match and reads everything off the surviving paths. walk() is the
contract's draw in Python floats."""
import numpy as np

import quotient_ref as Q
from generate_ref import uniform

MISSING = -2 ** 31


class Yardstick:
    def __init__(self, r, valid, final, alive, mask):
        out = Q.live_out_edges(r, valid, alive)
        self.live = Q.canonical_numbers(out, bool(valid[0]))  # the states the root reaches
        self.out = {s: out.get(s, []) for s in self.live}     # state -> [(full row, destination)] in canonical order
        self.keep = [i for i, m in enumerate(mask) if m]
        self.final = final
        self.memo = {}

    def rows(self, stream):
        return np.asarray(stream).reshape(-1, len(self.keep)).tolist()

    def matches(self, lab, x):
        return all(xv == MISSING or lab[i] == xv for i, xv in zip(self.keep, x))

    def n_paths(self, length):
        level = dict.fromkeys(self.live, 1)
        for _ in range(length):
            level = {s: sum(level[d] for _, d in self.out[s]) for s in self.live}
        return level.get(0, 0)

    def backward(self, stream, end_final=False):
        """B[r][s] for r = 0 .. len (kept: dp() and walk() of one stream share it)."""
        key = (repr(stream), end_final)
        if key in self.memo:
            return self.memo[key]
        L = len(stream)
        B = [{s: (float(bool(self.final[s])) if end_final else 1.0) for s in self.live}]
        for r in range(1, L + 1):
            x, prev, level = stream[L - r], B[-1], {}
            for s in self.live:
                acc = 0.0
                for lab, d in self.out[s]:
                    if self.matches(lab, x):
                        acc = acc + prev[d]
                level[s] = acc
            B.append(level)
        self.memo = {key: B}
        return B

    def dp(self, stream, end_final=False):
        """(count, supports [len][n_obs] sorted lists, n_states [len + 1]) of one stream, by the recurrences."""
        stream = self.rows(stream)
        L, n_obs = len(stream), len(self.keep)
        B = self.backward(stream, end_final)
        count = B[L].get(0, 0.0)
        F = {0} if count > 0.0 else set()
        supports, n_states = [], [len(F)]
        for t in range(L):
            togo, nxt, sets = B[L - t - 1], set(), [set() for _ in range(n_obs)]
            for s in F:
                for lab, d in self.out[s]:
                    if self.matches(lab, stream[t]) and togo[d] > 0.0:
                        nxt.add(d)
                        for c, i in enumerate(self.keep):
                            sets[c].add(lab[i])
            supports.append([sorted(x) for x in sets])
            F = nxt
            n_states.append(len(F))
        return count, supports, n_states

    def walk(self, stream, q, end_final=False, seed=0, rank=None):
        """(rows, end_final) of draw q of a feasible stream: the sample of (seed, q), or the rank-th consistent path."""
        stream = self.rows(stream)
        L = len(stream)
        B = self.backward(stream, end_final)
        assert B[L].get(0, 0.0) > 0.0
        s, rows = 0, []
        tau = float(rank) if rank is not None else 0.0
        for t in range(L):
            r = L - t
            nxt = B[r - 1]
            if rank is None:
                tau = uniform(seed, q, t) * B[r][s]
            acc, pick, last = 0.0, None, None
            for lab, d in self.out[s]:
                if not self.matches(lab, stream[t]):
                    continue
                w = nxt[d]
                if w > 0.0:
                    last = (lab, d, acc)
                total = acc + w
                if total > tau:
                    pick = (lab, d, acc)
                    break
                acc = total
            if pick is None:
                pick = last
            lab, d, before = pick
            if rank is not None:
                tau = tau - before
            rows.append([lab[i] for i in self.keep])
            s = d
        return rows, int(bool(self.final[s]))

    def paths(self, length):
        """Every live path of `length` edges from the root as (full rows, states visited), in lexicographic order of the full
        rows (depth first over the sorted edge lists)."""
        found = []

        def go(s, acc, states):
            if len(acc) == length:
                found.append((tuple(acc), tuple(states)))
                return
            for lab, d in self.out[s]:
                acc.append(lab)
                states.append(d)
                go(d, acc, states)
                acc.pop()
                states.pop()

        if self.live:
            go(0, [], [0])
        return found

    def brute(self, stream, end_final=False, paths=None):
        """(count, supports, n_states, the consistent paths projected, their end_final) without the recurrences: the paths
        that match, in order. `paths`: self.paths(len(stream)), to share it among streams of one length."""
        stream = self.rows(stream)
        L, n_obs = len(stream), len(self.keep)
        paths = self.paths(L) if paths is None else paths
        ok = [(rows, states) for rows, states in paths
              if all(self.matches(lab, x) for lab, x in zip(rows, stream)) and (not end_final or self.final[states[-1]])]
        supports = [[sorted({rows[t][i] for rows, _ in ok}) for i in self.keep] for t in range(L)]
        n_states = [len({states[t] for _, states in ok}) for t in range(L + 1)]
        proj = [[[lab[i] for i in self.keep] for lab in rows] for rows, _ in ok]
        return float(len(ok)), supports, n_states, proj, [int(bool(self.final[states[-1]])) for _, states in ok]

    def sample_prefix(self, rng, length):
        """A random walk of up to `length` steps from the root, projected."""
        rows, s = [], 0
        while self.live and len(rows) < length and self.out.get(s):
            lab, s = self.out[s][rng.randint(len(self.out[s]))]
            rows.append([lab[i] for i in self.keep])
        return rows


def blank(stream, rate, rng):
    """A copy of the stream with every entry MISSING with probability `rate` (0: none, 1: all)."""
    s = np.array(stream, dtype=np.int32)
    if s.size:
        s[rng.random_sample(s.shape) < rate] = MISSING
    return s


def make_streams(y, bounds, seed, length, n=3, rates=(0.0, 0.3, 1.0)):
    """Seeded streams of `length` steps for the automaton behind `y`: sampled prefixes and prefixes with one entry overwritten
    by a random in-domain value, each at every MISSING rate; a row with a value no edge carries; and the empty stream.
    bounds = [(lb, ub)] of every variable."""
    rng = np.random.RandomState(seed)
    n_obs = len(y.keep)
    lo = [max(bounds[v][0], -10 ** 6) for v in y.keep]
    hi = [min(bounds[v][1], 10 ** 6) for v in y.keep]
    base = []
    for _ in range(n):
        w = y.sample_prefix(rng, length)
        if len(w) != length:
            w = [[int(rng.randint(lo[c], hi[c] + 1)) for c in range(n_obs)] for _ in range(length)]
        base.append(w)
        if n_obs and length:
            m = [list(row) for row in w]
            c = int(rng.randint(n_obs))
            m[int(rng.randint(length))][c] = int(rng.randint(lo[c], hi[c] + 1))
            base.append(m)
    if n_obs and length:
        m = [list(row) for row in base[0]]
        c = int(rng.randint(n_obs))
        m[int(rng.randint(length))][c] = hi[c] + 1000
        base.append(m)
    streams = [np.zeros((0, n_obs), np.int32)]
    for w in base:
        for rate in rates:
            streams.append(blank(np.array(w, dtype=np.int64).reshape(length, n_obs), rate, rng))
    return streams


def bits(x):
    """A double by its bits."""
    return np.float64(x).view(np.uint64).item() if not isinstance(x, np.ndarray) else x.astype(np.float64).view(np.uint64).tolist()


def unpack(result):
    """(count, supports, n_states, draws, end_final) of infer_streams() -> one tuple of plain Python values per stream, the
    count by its bits."""
    count, supports, n_states, draws, fin = result
    return [(bits(c), s, np.asarray(k).tolist(), np.asarray(d).tolist(), np.asarray(f).tolist())
            for c, s, k, d, f in zip(count, supports, n_states, draws, fin)]
