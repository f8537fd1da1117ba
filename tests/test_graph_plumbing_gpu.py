"""What components(), optimise() and ctl() share on the device (csrc/automaton.hip: one live-edge CSR group, one launch batch, one
fixpoint; dev_csr.hpp: the CSR kernels and the walk step), asked in turn on ONE engine: optimise(mean) and ctl run the component pass
and then build their own CSR into the same group, ctl under another state filter, so every call finds the group as another service
left it. Every answer must equal the host twin's on the same automaton, array by array, and the answer of an engine that was asked
nothing else, by what does not depend on the numbering of states and edges. Run on the GPU box: pytest -m gpu."""
import pytest

import components_ref as R
import ctl_ref as T
from fuzz_models import table_by_name
from test_ctl_gpu import loops
from test_optimise import rows_of
from test_optimise_gpu import FANOUT, same as same_optimise
from test_repair_gpu import counter
from test_services_fuzz import TABLES

pytestmark = pytest.mark.gpu

NO_LIVE_ROOT = "table:1:20:3:60:0"  # of TABLES: no goal, `w until g` never ends
assert NO_LIVE_ROOT in TABLES

# name -> (text, interval domains, the CTL queries: an EU and an EX witness walk where there are worlds)
MODELS = {
    "no_live_root": (table_by_name(NO_LIVE_ROOT), False, ("EG true", "EX true")),  # E > 0 and not one live edge
    "loops:1": (loops(1), False, ("E[x >= 0 U x == 0]", "EX x == 0")),  # one state, one edge
    "loops:129": (loops(129), True, ("E[x > 100 U x < 3]", "EX x >= 70")),  # a segment of 129 > 64, three set words
    "FANOUT": (FANOUT, False, ("E[t == 0 U b == 3]", "EX a == 9")),  # 100 out-edges per state
    "row:255": (counter(255), False, ("EF c1 == 127", "EX x == 1")),  # k_s_scan: 255 lanes own a state
    "row:256": (counter(256), False, ("EF c2 == 1", "EX x == 1")),  # ... all 256
    "row:257": (counter(257), False, ("EF c2 == 2", "EX x == 1")),  # ... chunks of two states, 129 lanes
}


def solved(stcsp, name):
    text, interval, _ = MODELS[name]
    m = stcsp.Model(text=text)
    e = stcsp.Engine(m, flags=stcsp.F_INTERVAL_DOMAINS if interval else 0)
    r = e.solve()
    assert not r.truncated
    post = e.postprocess()
    return m, e, r, e.automaton(r).import_flags(post)


def requests(m, name):
    """(service, arguments) in the order asked: optimise(mean) and ctl, components, then both again, ctl with its other query first."""
    w = [(i * 7 + 3) % 5 - 2 for i in range(m.n_vars)]
    opt = ("optimise", (w,), dict(horizon=6, lengths=[6, 0, 3], mean=True, state_best=True))
    eu, ex = MODELS[name][2]
    return [opt, ("ctl", (eu,), dict(witness=True)), ("components", ("all",), {}), opt, ("ctl", (ex,), dict(witness=True)), ("ctl", (eu,), dict(witness=True))]


SAME = {"optimise": same_optimise, "ctl": T.same, "components": R.same}


def content(service, res):
    """What an answer says whatever the numbering of the states and the order of the exported edges."""
    if service == "optimise":
        return (res["best"].tolist(), sorted(res["state_best"].tolist()), res["omega_mean"], sorted(res["comp_mean"]), res["largest_cyclic"],
                [(n, rows_of(rows)) for n, rows, _ in res["witnesses"]])
    if service == "ctl":
        return (res["n_worlds"], res["n_initial"], res["n_initial_sat"], int(res["edge_world"].sum()), int(res["edge_sat"].sum()), T.witness_rows(res))
    return (tuple(int(res[k]) for k in ("n_states", "n_components", "n_cyclic", "n_accepting", "n_bottom", "n_omega", "root_omega", "n_lassos")),
            sorted(res["comp_size"].tolist()), sorted((rows_of(stem), rows_of(loop)) for _, stem, loop in res["lassos"]))


@pytest.mark.parametrize("name", list(MODELS))
def test_services_in_turn_on_one_engine(stcsp, name):
    m, e, r, a = solved(stcsp, name)
    got = []
    for service, args, kw in requests(m, name):
        dev = getattr(e, service)(*args, **kw)
        assert SAME[service](dev, getattr(a, service)(*args, **kw)), f"{name}: {service}{args[-1:]} after {[s for s, _ in got]}: device and host twin differ"
        got.append((service, content(service, dev)))
    assert got[0] == got[3] and got[1] == got[5], f"{name}: the same call, asked again after the other services, answers differently"
    for i, (service, args, kw) in enumerate(requests(m, name)[:3] + requests(m, name)[4:5]):
        _, fresh, _, fa = solved(stcsp, name)
        alone = getattr(fresh, service)(*args, **kw)
        assert SAME[service](alone, getattr(fa, service)(*args, **kw))
        assert (service, content(service, alone)) == got[i if i < 3 else 4], f"{name}: {service}{args[-1:]} on one engine in turn and on a fresh engine differ"
    # the corner the model is in the list for
    comps, worlds = got[2][1], got[1][1][0]
    states, edges = r.n_states, a.n_live_edges
    if name == "no_live_root":
        assert r.n_edges > 0 and (edges, comps[0][0], worlds) == (0, 0, 0)
    elif name.startswith("loops:"):
        assert (states, edges, worlds) == (1, int(name[6:]), int(name[6:])) and len(got[1][1][5][1]) == 1 and len(got[4][1][5][1]) == 2
    elif name == "FANOUT":
        assert edges == 100 * comps[0][0] and worlds == edges
    else:
        n = int(name[4:])
        assert (states, comps[0][0], edges, worlds) == (n, n, 2 * n, 2 * n) and [len(s) for s, _ in comps[2]] == [n - 1]
