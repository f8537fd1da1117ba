"""The independent yardstick of the posterior marginals (tests only), in plain Python over the automaton of the CPU oracle,
on the mask, order and match rules of tests/infer_ref.py (whose Yardstick it extends).

Definition (include/stcsp_engine.h, stcsp_engine_posterior): the weight of an edge is the product, in variable order, of the
weights of the observable values it carries (a value that is not listed weighs 1); B_0 = 1 on the live states (final[s] with
end_final), B_{r+1}(s) = the sum of w(e) * B_r(dst) over the matching live out-edges of positive weight whose destination has
weight to go, in canonical order; mass = B_len(root); exact = mass < 2^53. For an exact stream A_0(root) = 1,
A_{t+1}(d) = the sum of A_t(src) * w over the edges feasible at t, and m(t, v, a) = the sum of A_t(src) * w * B(dst) over the
feasible edges that carry a.

Two implementations that share nothing but the edge lists: dp() is the contract's recurrences, B in Python floats one
operation at a time (bit for bit the contract's), A and the marginals in Python ints; brute() enumerates every live path and
multiplies the weights of its edges as Python ints."""
import numpy as np

import infer_ref as I

MISSING = I.MISSING
bits = I.bits


class Yardstick(I.Yardstick):
    def __init__(self, r, valid, final, alive, mask, weights=None):
        """weights: None, or per observable variable (mask order) a dict value -> int weight or None."""
        super().__init__(r, valid, final, alive, mask)
        self.weights = [w or {} for w in weights] if weights is not None else [{} for _ in self.keep]

    def weight(self, lab):
        """(the double of the contract, the exact integer)"""
        acc, exact = 1.0, 1
        for c, i in enumerate(self.keep):
            w = self.weights[c].get(lab[i], 1)
            acc = acc * float(w)
            exact *= w
        return acc, exact

    def backward_w(self, stream, end_final=False):
        L = len(stream)
        B = [{s: (float(bool(self.final[s])) if end_final else 1.0) for s in self.live}]
        for r in range(1, L + 1):
            x, prev, level = stream[L - r], B[-1], {}
            for s in self.live:
                acc = 0.0
                for lab, d in self.out[s]:
                    if not self.matches(lab, x):
                        continue
                    w = self.weight(lab)[0]
                    if not w > 0.0 or not prev[d] > 0.0:
                        continue
                    term = w * prev[d]
                    acc = acc + term
                level[s] = acc
            B.append(level)
        return B

    def dp(self, stream, end_final=False):
        """(mass, exact, final_mass, marginals [len][n_obs] of sorted (value, mass) lists) of one stream, by the recurrences."""
        stream = self.rows(stream)
        L, n_obs = len(stream), len(self.keep)
        B = self.backward_w(stream, end_final)
        mass = B[L].get(0, 0.0)
        exact = int(mass < 2.0 ** 53)
        if not exact:
            return mass, 0, 0, [[[] for _ in range(n_obs)] for _ in range(L)]
        A = {0: 1} if mass > 0.0 else {}
        marginals = []
        for t in range(L):
            togo, nxt, bins = B[L - t - 1], {}, [{} for _ in range(n_obs)]
            for s, a in A.items():
                for lab, d in self.out[s]:
                    w = self.weight(lab)
                    if self.matches(lab, stream[t]) and w[0] > 0.0 and togo[d] > 0.0:
                        assert w[0] == w[1] and togo[d] == int(togo[d])  # the exactness argument
                        nxt[d] = nxt.get(d, 0) + a * w[1]
                        for c, i in enumerate(self.keep):
                            bins[c][lab[i]] = bins[c].get(lab[i], 0) + a * w[1] * int(togo[d])
            marginals.append([sorted(b.items()) for b in bins])
            A = nxt
        return mass, 1, sum(a for s, a in A.items() if self.final[s]), marginals

    def brute(self, stream, end_final=False, paths=None):
        """(mass as an int, final_mass, marginals) without the recurrences: over the paths that match, the products of their
        edges' weights as Python ints. `paths`: self.paths(len(stream)), to share it among streams of one length."""
        stream = self.rows(stream)
        L, n_obs = len(stream), len(self.keep)
        paths = self.paths(L) if paths is None else paths
        mass = final_mass = 0
        bins = [[{} for _ in range(n_obs)] for _ in range(L)]
        for rows, states in paths:
            if not all(self.matches(lab, x) for lab, x in zip(rows, stream)):
                continue
            w = 1
            for lab in rows:
                w *= self.weight(lab)[1]
            if not w:
                continue
            if self.final[states[-1]]:
                final_mass += w
            elif end_final:
                continue
            mass += w
            for t, lab in enumerate(rows):
                for c, i in enumerate(self.keep):
                    bins[t][c][lab[i]] = bins[t][c].get(lab[i], 0) + w
        return mass, final_mass, [[sorted(b.items()) for b in row] for row in bins]


def unpack(result):
    """(mass, exact, final_mass, marginals) of posterior_streams() -> one tuple of plain Python values per stream, the mass by
    its bits."""
    mass, exact, final_mass, marginals = result
    return [(bits(m), int(e), int(f), [[[(int(a), int(b)) for a, b in cell] for cell in row] for row in g])
            for m, e, f, g in zip(mass, exact, final_mass, marginals)]


def expected(y, stream, end_final=False):
    """What unpack() gives for one stream, by the yardstick's recurrences."""
    mass, exact, final_mass, marginals = y.dp(stream, end_final)
    return bits(mass), exact, final_mass, marginals
