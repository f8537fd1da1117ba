"""The independent yardstick of the stream generator (tests only): counting, unranking and sampling of solution prefixes in
plain Python over quotient_ref.live_out_edges, whose lists are already sorted by row, with Python floats for the weights
and the targets.

Definition (include/stcsp_engine.h, stcsp_engine_generate): W_0(s) = 1 (or final[s]), W_{t+1}(s) = the sum of W_t(dst) over
the live out-edges of s in canonical order; a stream follows, per step, the first edge whose running sum exceeds the
target. Every floating-point step is one Python float operation, so the result is bit for bit the contract's."""
import numpy as np

import quotient_ref as Q

M64 = (1 << 64) - 1


def mix(x):
    """The splitmix64 finaliser of the header."""
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & M64
    return x ^ (x >> 31)


def uniform(seed, stream, t):
    z = mix((mix((mix((seed + 0x9e3779b97f4a7c15) & M64) + stream) & M64) + t) & M64)
    return float(z >> 11) * 2.0 ** -53


class Yardstick:
    def __init__(self, r, valid, final, alive, mask, horizon, end_final=False):
        out = Q.live_out_edges(r, valid, alive)
        self.live = Q.canonical_numbers(out, bool(valid[0]))  # the states the root reaches
        self.out = {s: out.get(s, []) for s in self.live}     # state -> [(full row, destination)] in canonical order
        self.keep = [i for i, m in enumerate(mask) if m]
        self.final = final
        self.horizon = horizon
        self.W = [{s: (float(bool(final[s])) if end_final else 1.0) for s in self.live}]
        for _ in range(horizon):
            prev, level = self.W[-1], {}
            for s in self.live:
                acc = 0.0
                for _, d in self.out[s]:
                    acc = acc + prev[d]
                level[s] = acc
            self.W.append(level)
        self.count = np.array([w.get(0, 0.0) for w in self.W], dtype=np.float64)

    def max_out_degree(self):
        return max((len(e) for e in self.out.values()), default=0)

    def n_edges(self):
        return sum(len(e) for e in self.out.values())

    def stream(self, length, seed=0, index=0, rank=None):
        """(rows [length][n_obs], end_final, full rows) of one stream: the sample of (seed, index), or the rank-th path."""
        assert 0 <= length <= self.horizon and self.count[length] > 0
        s, rows, full = 0, [], []
        tau = float(rank) if rank is not None else 0.0
        for t in range(length):
            r = length - t
            nxt = self.W[r - 1]
            if rank is None:
                tau = uniform(seed, index, t) * self.W[r][s]
            acc, pick, last = 0.0, None, None
            for lab, d in self.out[s]:
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
            full.append(lab)
            s = d
        return rows, int(bool(self.final[s])), full

    def streams(self, n, length, seed=0, ranks=None):
        """(values int32 [n, length, n_obs], end_final uint8 [n])"""
        res = [self.stream(length, seed, i, None if ranks is None else int(ranks[i])) for i in range(n)]
        values = np.array([x[0] for x in res], dtype=np.int32).reshape(n, length, len(self.keep))
        return values, np.array([x[1] for x in res], dtype=np.uint8)

    def enumerate(self, length, end_final=False):
        """Every live path of `length` steps as its sequence of full rows, in lexicographic order (depth first over the
        sorted edge lists); with end_final only those that end in a final state. Independent of the weights."""
        paths = []

        def walk(s, depth, acc):
            if depth == length:
                if not end_final or self.final[s]:
                    paths.append(tuple(acc))
                return
            for lab, d in self.out[s]:
                acc.append(lab)
                walk(d, depth + 1, acc)
                acc.pop()

        if self.live:
            walk(0, 0, [])
        return paths
