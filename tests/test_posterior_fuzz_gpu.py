"""Posterior marginals on two table-driven random automata of tests/test_services_fuzz.py, on the device: table:17:60:3:60:10
(65 live states, one variable of 60 values: the W = 2 kernels) and table:37:16x16:3:60:10:3 (262 live states). Device == host
twin on the engine's own automaton == the plain Python yardstick of tests/posterior_ref.py on the CPU oracle's, every output
with `==`, the masses by their bits; under every mask of that file, with and without END_FINAL, unweighted and under a
positive weight set and one with a 0 and a 2^31 - 1. Each automaton is solved once. Run on the GPU box: pytest -m gpu."""
import functools

import pytest

import infer_ref as I
import monitor_ref as M
import observer_ref as OR
import posterior_ref as P
from test_posterior_gpu import check, first_weights
from test_services_fuzz import MASKS, TEXT

pytestmark = pytest.mark.gpu

AUTOMATA = {"table:17:60:3:60:10": 65, "table:37:16x16:3:60:10:3": 262}


@functools.lru_cache(maxsize=None)
def device(stcsp, RefOracle, name):
    """(model, engine, Result, the host's automaton with the device's flags, the oracle's Result and flags, and the oracle that owns
    them) of one automaton."""
    m = stcsp.Model(text=TEXT[name])
    e = stcsp.Engine(m)
    r = e.solve()
    assert not r.truncated
    post = e.postprocess()
    o = RefOracle(m)
    ro = o.solve()
    return m, e, r, e.automaton(r).import_flags(post), ro, o.automaton(ro).traverse().flags(), o


@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("name", list(AUTOMATA))
def test_device_against_twin_and_yardstick(stcsp, RefOracle, name, mask_name):
    m, e, r, host, ro, flags, _ = device(stcsp, RefOracle, name)
    mask = {**M.masks(m, r), "colour": OR.only(m, "c")}[mask_name]
    arg = None if mask_name == "default" else mask
    info = e.generator(arg, 0)
    assert info.n_states == AUTOMATA[name]
    plain = I.Yardstick(ro, *flags, mask)
    streams = [s for L in (4, 9) for s in I.make_streams(plain, m.var_bounds(), 3 + L, L, n=2)]
    few = range(len(streams)) if info.n_edges <= 2000 else range(1, 5)  # the plain Python recurrences then take a few streams only
    for weights in (None,) + (first_weights(sum(mask), streams) if sum(mask) else ()):
        y = P.Yardstick(ro, *flags, mask, weights)
        for end_final in (False, True):
            dev = check(e, host, streams, arg, y, few=few, end_final=end_final, weights=weights)
            if weights is None:  # (b) and the count, against the device's own infer
                count, supports = e.infer_streams(streams, end_final=end_final)[:2]
                assert [d[0] for d in dev] == I.bits(count)
                assert all([[k for k, _ in cell] for cell in row] == sets for d, sup in zip(dev, supports) if d[1] for row, sets in zip(d[3], sup))
