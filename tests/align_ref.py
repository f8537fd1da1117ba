"""The independent yardstick of the stream alignment (tests only), in plain Python over the edge lists of
repair_ref.Yardstick, which are already in canonical order (sorted by full row).

Definition (include/stcsp_engine.h, stcsp_engine_align): the repair's shortest path over (time x automaton) with two more
arcs, a skip (drop the observed step, keep the state, skip_cost) and an insert (follow an edge, consume no step, gap_cost).

Three parts that share nothing but the edge lists and the step cost:
  distance()  Dijkstra with a heap over the product graph (t, s) from (0, root), with match, skip and insert arcs. This is
              not the recurrence: it runs forward and settles every node once.
  walk()      the contract's recurrence G[t][s], every level closed by repeated whole sweeps until nothing changes, and
              the four rules of the walk, for rows and ops.
  brute()     every solution prefix of up to len + distance / gap_cost steps, depth first, with the classical weighted edit
              distance (Needleman-Wunsch) of the stream against each; the minimum must be the distance."""
import heapq

import numpy as np

import repair_ref as R

MISSING = R.MISSING
M, D, I = 0, 1, 2
NONE = (-1, [], [], 0, 0, 0, 0)


class Yardstick(R.Yardstick):
    def _args(self, stream, weights):
        stream = np.asarray(stream).reshape(-1, len(self.keep)).tolist()
        return stream, ([1] * len(self.keep) if weights is None else list(weights))

    def base(self, s, end_final):
        return not end_final or bool(self.final[s])

    def distance(self, stream, weights=None, skip_cost=1, gap_cost=1, end_final=False):
        stream, weights = self._args(stream, weights)
        m = len(stream)
        if not self.live:
            return -1
        done, heap = set(), [(0, 0, 0)]
        while heap:
            d, t, s = heapq.heappop(heap)
            if (t, s) in done:
                continue
            done.add((t, s))
            if t == m and self.base(s, end_final):
                return d
            for lab, dst in self.out[s]:
                heapq.heappush(heap, (d + gap_cost, t, dst))
                if t < m:
                    heapq.heappush(heap, (d + self.cost(lab, stream[t], weights), t + 1, dst))
            if t < m:
                heapq.heappush(heap, (d + skip_cost, t + 1, s))
        return -1

    def close(self, level, gap_cost):
        changed = True
        while changed:
            changed = False
            for s in self.live:
                for _, d in self.out[s]:
                    if level[d] is not None and (level[s] is None or gap_cost + level[d] < level[s]):
                        level[s] = gap_cost + level[d]
                        changed = True
        return level

    def table(self, stream, weights, skip_cost, gap_cost, end_final):
        m = len(stream)
        G = [None] * (m + 1)
        G[m] = self.close({s: (0 if self.base(s, end_final) else None) for s in self.live}, gap_cost)
        for t in range(m - 1, -1, -1):
            nxt, level = G[t + 1], {}
            for s in self.live:
                terms = [self.cost(lab, stream[t], weights) + nxt[d] for lab, d in self.out[s] if nxt[d] is not None]
                if nxt[s] is not None:
                    terms.append(skip_cost + nxt[s])
                level[s] = min(terms) if terms else None
            G[t] = self.close(level, gap_cost)
        return G

    def walk(self, stream, weights=None, skip_cost=1, gap_cost=1, end_final=False):
        """(distance, emitted rows, ops, n_changed, n_skipped, n_inserted, end_final) of one stream; distance -1: NONE."""
        stream, weights = self._args(stream, weights)
        m = len(stream)
        if not self.live:
            return NONE
        G = self.table(stream, weights, skip_cost, gap_cost, end_final)
        if G[0][0] is None:
            return NONE
        t, s, rows, ops, changed = 0, 0, [], [], 0
        while not (t == m and G[m][s] == 0 and self.base(s, end_final)):
            want, step = G[t][s], None
            if t < m:
                for lab, d in self.out[s]:
                    if G[t + 1][d] is not None and self.cost(lab, stream[t], weights) + G[t + 1][d] == want:
                        step = (M, lab, d)
                        break
                if step is None and G[t + 1][s] is not None and skip_cost + G[t + 1][s] == want:
                    step = (D, None, s)
            if step is None:
                for lab, d in self.out[s]:
                    if G[t][d] is not None and gap_cost + G[t][d] == want:
                        step = (I, lab, d)
                        break
            assert step is not None, "a finite value is attained by a rule"
            op, lab, s = step
            ops.append(op)
            if op != D:
                row = [lab[i] for i in self.keep]
                rows.append(row)
                if op == M:
                    changed += sum(1 for xv, pv in zip(stream[t], row) if xv != MISSING and xv != pv)
            t += op != I
        return G[0][0], rows, ops, changed, ops.count(D), ops.count(I), int(bool(self.final[s]))

    def n_prefixes(self, longest):
        """The number of live paths of 0 .. longest steps from the root."""
        return sum(self.n_paths(t) for t in range(longest + 1))

    def brute(self, stream, distance, weights=None, skip_cost=1, gap_cost=1, end_final=False, limit=5000):
        """The least classical edit distance of the stream to a solution prefix of at most len + distance / gap_cost steps
        (a longer one costs more in inserts alone); -1 if none ends where it may. At most `limit` prefixes: the caller
        picks streams for which that holds."""
        stream, weights = self._args(stream, weights)
        m = len(stream)
        if not self.live:
            return -1
        longest = m + max(distance, 0) // gap_cost
        assert self.n_prefixes(longest) <= limit, "too many prefixes for the brute force: pick a shorter stream"
        best = [None]

        def visit(s, depth, col):  # col[j]: stream[:j] against the prefix walked so far
            if self.base(s, end_final) and (best[0] is None or col[m] < best[0]):
                best[0] = col[m]
            if depth == longest:
                return
            for lab, d in self.out[s]:
                new = [col[0] + gap_cost]
                for j in range(1, m + 1):
                    new.append(min(col[j] + gap_cost, new[j - 1] + skip_cost, col[j - 1] + self.cost(lab, stream[j - 1], weights)))
                visit(d, depth + 1, new)

        visit(0, 0, [j * skip_cost for j in range(m + 1)])
        return -1 if best[0] is None else best[0]


def unpack(result):
    """What align_streams() returns -> one tuple of plain Python values per stream, in the order of Yardstick.walk()."""
    dist, rows, ops, nchg, nskip, nins, fin = result
    return [(int(d), np.asarray(v).tolist(), np.asarray(o).tolist(), int(c), int(a), int(b), int(f))
            for d, v, o, c, a, b, f in zip(dist, rows, ops, nchg, nskip, nins, fin)]


def same(a, b):
    """Two results of align_streams(), every output of every stream."""
    return unpack(a) == unpack(b)


def recomputed_cost(y, stream, got, weights, skip_cost, gap_cost):
    """The distance recomputed from the outputs of one stream: the matched steps' costs and the prices of the D and I ops."""
    dist, rows, ops, nchg, nskip, nins, fin = got
    stream, weights = y._args(stream, weights)
    t = k = total = 0
    for op in ops:
        if op == M:
            total += sum(w for xv, pv, w in zip(stream[t], rows[k], weights) if xv != MISSING and xv != pv)
        total += skip_cost * (op == D) + gap_cost * (op == I)
        t += op != I
        k += op != D
    assert t == len(stream) and k == len(rows), "#M + #D == len and #M + #I == out_len"
    return total


def damaged(rng, prefix, lo, hi, deleted=0.02, duplicated=0.02, overwritten=0.05):
    """A solution prefix [len, n_obs] with steps deleted, steps duplicated and entries overwritten by in-domain values."""
    rows = []
    for row in np.asarray(prefix).tolist():
        u = rng.rand()
        if u < deleted:
            continue
        rows.append(list(row))
        if u > 1 - duplicated:
            rows.append(list(row))
    for row in rows:
        for c in range(len(row)):
            if rng.rand() < overwritten:
                row[c] = int(rng.randint(lo[c], hi[c] + 1))
    return np.array(rows, dtype=np.int64).reshape(len(rows), np.asarray(prefix).shape[1]).astype(np.int32)
