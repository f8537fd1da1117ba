"""The independent yardstick of the stream repair (tests only), in plain Python over quotient_ref.live_out_edges, whose
lists are already in canonical order (sorted by full row).

Definition (include/stcsp_engine.h, stcsp_engine_repair): the cost of a step is the sum of the weights of the observed
variables whose value the edge does not carry; G_0 = 0 on the live states (on the final ones with end_final),
G_{r+1}(s) = min over the live out-edges of cost + G_r(dst); the repaired stream follows, per step, the first edge in
canonical order that attains G_r(s).

Two implementations that share nothing but the edge lists: dp() is the contract's recurrence, brute() enumerates every
live path of the stream's length, costs each and keeps the first of least cost in lexicographic order."""
import numpy as np

import quotient_ref as Q

MISSING = -2 ** 31
INF = None


class Yardstick:
    def __init__(self, r, valid, final, alive, mask):
        out = Q.live_out_edges(r, valid, alive)
        self.live = Q.canonical_numbers(out, bool(valid[0]))  # the states the root reaches
        self.out = {s: out.get(s, []) for s in self.live}     # state -> [(full row, destination)] in canonical order
        self.keep = [i for i, m in enumerate(mask) if m]
        self.final = final

    def cost(self, lab, x, weights):
        return sum(w for i, xv, w in zip(self.keep, x, weights) if xv != MISSING and lab[i] != xv)

    def n_paths(self, length):
        """The number of live paths of `length` steps from the root (0 without a live root)."""
        level = dict.fromkeys(self.live, 1)
        for _ in range(length):
            level = {s: sum(level[d] for _, d in self.out[s]) for s in self.live}
        return level.get(0, 0)

    def answer(self, stream, s, rows):
        """(repaired rows, end_final, n_changed) of a path given as its full rows and its last state."""
        proj = [[lab[i] for i in self.keep] for lab in rows]
        changed = sum(1 for x, p in zip(stream, proj) for xv, pv in zip(x, p) if xv != MISSING and xv != pv)
        return proj, int(bool(self.final[s])), changed

    def dp(self, stream, weights=None, end_final=False):
        """(distance, repaired rows, end_final, n_changed) of one stream (rows of len(keep) values); distance -1: none."""
        stream = np.asarray(stream).reshape(-1, len(self.keep)).tolist()
        weights = [1] * len(self.keep) if weights is None else list(weights)
        L = len(stream)
        if not self.live:
            return -1, [[0] * len(self.keep)] * L, 0, 0
        G = [{s: (0 if not end_final or self.final[s] else INF) for s in self.live}]
        for r in range(1, L + 1):
            x, prev, level, seen = stream[L - r], G[-1], {}, {}

            def cost(lab):  # (one evaluation per distinct projected label and step)
                key = tuple(lab[i] for i in self.keep)
                if key not in seen:
                    seen[key] = self.cost(lab, x, weights)
                return seen[key]

            for s in self.live:
                terms = [cost(lab) + prev[d] for lab, d in self.out[s] if prev[d] is not INF]
                level[s] = min(terms) if terms else INF
            G.append(level)
        if G[L][0] is INF:
            return -1, [[0] * len(self.keep)] * L, 0, 0
        s, rows = 0, []
        for t in range(L):
            r = L - t
            for lab, d in self.out[s]:
                if G[r - 1][d] is not INF and self.cost(lab, stream[t], weights) + G[r - 1][d] == G[r][s]:
                    rows.append(lab)
                    s = d
                    break
            else:
                raise AssertionError("a finite minimum is attained")
        return (G[L][0],) + self.answer(stream, s, rows)

    def brute(self, stream, weights=None, end_final=False):
        """The same answer without the recurrence: every live path of the stream's length, depth first over the sorted edge
        lists, that is in lexicographic order of the full rows; the first path of least cost wins."""
        stream = np.asarray(stream).reshape(-1, len(self.keep)).tolist()
        weights = [1] * len(self.keep) if weights is None else list(weights)
        L = len(stream)
        best = [None, None, None]  # cost, rows, last state

        def walk(s, depth, acc, cost):
            if depth == L:
                if (not end_final or self.final[s]) and (best[0] is None or cost < best[0]):
                    best[:] = [cost, list(acc), s]
                return
            for lab, d in self.out[s]:
                acc.append(lab)
                walk(d, depth + 1, acc, cost + self.cost(lab, stream[depth], weights))
                acc.pop()

        if self.live:
            walk(0, 0, [], 0)
        if best[0] is None:
            return -1, [[0] * len(self.keep)] * L, 0, 0
        return (best[0],) + self.answer(stream, best[2], best[1])

    def sample_prefix(self, rng, length):
        """A random walk of up to `length` steps from the root, projected."""
        rows, s = [], 0
        while self.live and len(rows) < length and self.out.get(s):
            lab, s = self.out[s][rng.randint(len(self.out[s]))]
            rows.append([lab[i] for i in self.keep])
        return rows


def make_streams(y, bounds, seed, length, n=4):
    """Seeded streams of `length` steps for the automaton behind `y`: sampled prefixes as they are and with random entries
    overwritten by in-domain values; random in-domain rows; rows with a value no edge carries; rows with MISSING entries; an
    all-MISSING stream; and the empty stream. bounds = [(lb, ub)] of every variable."""
    rng = np.random.RandomState(seed)
    n_obs = len(y.keep)
    lo = [max(bounds[v][0], -10 ** 6) for v in y.keep]
    hi = [min(bounds[v][1], 10 ** 6) for v in y.keep]

    def random_rows():
        return [[int(rng.randint(lo[c], hi[c] + 1)) for c in range(n_obs)] for _ in range(length)]

    streams = [[], [[MISSING] * n_obs for _ in range(length)]]
    for _ in range(n):
        w = y.sample_prefix(rng, length)
        if len(w) == length:
            streams.append([list(row) for row in w])
            m = [list(row) for row in w]
            for _ in range(max(1, length * n_obs // 8)):
                if n_obs and length:
                    c = int(rng.randint(n_obs))
                    m[int(rng.randint(length))][c] = int(rng.randint(lo[c], hi[c] + 1))
            streams.append(m)
            if n_obs and length:
                m = [list(row) for row in m]
                m[int(rng.randint(length))][int(rng.randint(n_obs))] = MISSING
                streams.append(m)
        streams.append(random_rows())
    if n_obs and length:
        m = random_rows()
        c = int(rng.randint(n_obs))
        m[int(rng.randint(length))][c] = hi[c] + 1000
        streams.append(m)
    return [np.array(s, dtype=np.int64).reshape(len(s), n_obs).astype(np.int32) for s in streams]


def unpack(result):
    """(distance, values_list, end_final, n_changed) of repair_streams() -> one tuple of plain Python values per stream."""
    dist, values, fin, nchg = result
    return [(int(d), np.asarray(v).tolist(), int(f), int(c)) for d, v, f, c in zip(dist, values, fin, nchg)]
