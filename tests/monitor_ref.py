"""The independent yardstick of the stream monitor (tests only): sets of states over the automaton of the CPU oracle, in
plain Python, and the seeded stream generators every monitor test draws from.

Definition (include/stcsp_engine.h, stcsp_engine_monitor_check): S_0 = {root} if the root is live, S_{t+1} = the live
states reached from S_t over a live edge whose projected label equals step t; accepted_len = the largest L with S_L not
empty, n_end = |S_accepted_len|, end_final = some state of it is final. None of the three depends on state numbers."""
import numpy as np

import quotient_ref as Q


class Yardstick:
    def __init__(self, r, valid, final, alive, mask):
        out = Q.live_out_edges(r, valid, alive)
        self.live = Q.canonical_numbers(out, bool(valid[0]))  # state -> number, the states the root reaches
        self.keep = [i for i, m in enumerate(mask) if m]
        self.final = final
        self.trans = {}   # (state, projected label) -> set of destinations
        self.edges = []   # (source, projected label, destination) of every live edge, in a reproducible order
        for s in sorted(self.live, key=self.live.get):
            for lab, d in out.get(s, ()):
                p = tuple(lab[i] for i in self.keep)
                self.trans.setdefault((s, p), set()).add(d)
                self.edges.append((s, p, d))
        self.out = {}
        for s, p, d in self.edges:
            self.out.setdefault(s, []).append((p, d))

    def check(self, stream):
        """(accepted_len, n_end, end_final, largest set met) of one stream (rows of len(keep) values)."""
        cur = {0} if self.live else set()
        t, largest = 0, len(cur)
        for row in np.asarray(stream).tolist():  # [len, n_obs]
            nxt = set()
            for s in cur:
                nxt |= self.trans.get((s, tuple(row)), set())
            if not nxt:
                break
            cur = nxt
            t += 1
            largest = max(largest, len(cur))
        return t, len(cur), int(any(self.final[s] for s in cur)), largest

    def check_all(self, streams):
        res = [self.check(s) for s in streams]
        acc = np.array([x[0] for x in res], dtype=np.int32)
        nend = np.array([x[1] for x in res], dtype=np.int32)
        fin = np.array([x[2] for x in res], dtype=np.uint8)
        return acc, nend, fin, max([x[3] for x in res], default=len({0} if self.live else ()))


def make_streams(y, bounds, seed, n_walks=12, max_len=200):
    """Seeded streams for the automaton behind yardstick `y`. Returns (streams, kinds, mutated index or -1):
       walk     random walks on the live automaton from the root, projected: must be accepted whole;
       mutated  the same walks with one step overwritten by another edge's label or by an out-of-domain value;
       random   rows drawn from the variables' bounds;
    lengths from 0 (always present) to max_len. bounds = [(lb, ub)] of every variable."""
    rng = np.random.RandomState(seed)
    n_obs = len(y.keep)
    streams, kinds, where = [np.zeros((0, n_obs), np.int32)], ["walk"], [-1]
    walks = []
    for i in range(n_walks):
        length = int(rng.randint(0, max_len + 1)) if i else max_len
        rows, s = [], 0
        while y.live and len(rows) < length and y.out.get(s):
            p, s = y.out[s][rng.randint(len(y.out[s]))]
            rows.append(p)
        w = np.array(rows, dtype=np.int32).reshape(len(rows), n_obs)
        walks.append(w)
        streams.append(w), kinds.append("walk"), where.append(-1)
    for w in walks:
        if not len(w) or not n_obs:
            continue
        m = w.copy()
        at = int(rng.randint(len(m)))
        if rng.randint(2) and y.edges:
            m[at] = y.edges[rng.randint(len(y.edges))][1]
        else:
            col = int(rng.randint(n_obs))
            m[at, col] = min(bounds[y.keep[col]][1], 10 ** 6) + 1000
        streams.append(m), kinds.append("mutated"), where.append(at)
    for _ in range(max(2, n_walks // 2)):
        length = int(rng.randint(0, max_len + 1))
        cols = [rng.randint(max(bounds[v][0], -10 ** 6), min(bounds[v][1], 10 ** 6) + 1, size=length) for v in y.keep]
        streams.append(np.stack(cols, axis=1).astype(np.int32) if cols else np.zeros((length, 0), np.int32))
        kinds.append("random"), where.append(-1)
    return streams, kinds, where


def hidden_signature_mask(model, r):
    """Every variable observable but the first signature variable (the first variable when there is none)."""
    mask = [1] * model.n_vars
    sig = [v for v in range(model.n_vars) if r.var_is_signature[v]]
    mask[sig[0] if sig else 0] = 0
    return mask


def masks(model, r):
    return {"default": Q.default_mask(model.var_names), "all": [1] * model.n_vars, "hidden": hidden_signature_mask(model, r)}
