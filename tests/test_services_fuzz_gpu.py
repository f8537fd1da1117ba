"""The automaton services on table-driven random automata, on the device: the list of tests/test_services_fuzz.py through the
existing device checks of generate, repair, infer, monitor, quotient, observer, components, optimise and compare -- device ==
host twin on the engine's own automaton == the plain Python yardstick on the CPU oracle's, everything with `==`, doubles by
their bits. One engine per automaton, shared by the services: the helpers of the other files that solve a model of their own
are handed that engine here. Two-digit models run with default flags, one-variable models of 33..128 values under the wide
kernels, the one of 200 values with F_INTERVAL_DOMAINS. Run on the GPU box: pytest -m gpu."""
import functools

import numpy as np
import pytest

import compare_ref as CMP
import components_ref as CR
import monitor_ref as M
import observer_ref as OR
import quotient_ref as Q
import test_compare_gpu as TCmpg
import test_components_gpu as TCg
import test_generate_gpu as TGg
import test_infer_gpu as TIg
import test_monitor_gpu as TMg
import test_observer_gpu as TObg
import test_optimise_gpu as TOg
import test_quotient_gpu as TQg
import test_repair_gpu as TRg
from test_compare import oracle_observer
from test_optimise import big_weights, small_weights
from test_services_fuzz import MASKS, OBSERVABLES, TABLES, TEXT, check_floors, digits_of, mutant, oracle_shape, shape_line, shape_of

pytestmark = pytest.mark.gpu

SERVICES = ("generate", "repair", "infer", "monitor", "quotient", "observer", "components", "optimise-small", "optimise-big", "compare")
# the services in two orders on two of the automata: 65 live states under the W = 2 kernels, 262 under the default ones
ORDERS = {"forward": SERVICES, "backward": SERVICES[::-1]}
ORDERED = ("table:17:60:3:60:10", "table:37:16x16:3:60:10:3")


def values_of(name):
    """The largest domain of the model: what chooses the engine's kernels."""
    return max(int(b) for b in name.removeprefix("mutant:").split(":")[2].split("x"))


@functools.lru_cache(maxsize=None)
def device(stcsp, name):
    """(model, engine, Result, PostResult, the host's automaton with the device's flags) of one automaton: solved and
    post-processed once, under the kernels its domains ask for."""
    m = stcsp.Model(text=TEXT[name])
    width = values_of(name)
    e = stcsp.Engine(m, flags=stcsp.F_INTERVAL_DOMAINS if width > 128 else 0)
    expect = (0,) if width > 128 else (2, 4) if width > 32 else (1,)  # intervals, the W = 2 / 4 kernels, one word
    assert e.kernel_choice()["domain_form"] in expect, f"{name}: domain form {e.kernel_choice()['domain_form']}"
    r = e.solve()
    assert not r.truncated
    post = e.postprocess()
    return m, e, r, post, e.automaton(r).import_flags(post)


_by_model = {}  # id(model) -> name: the helpers that take a model are given the one device() made


def model_of(stcsp, name):
    m = device(stcsp, name)[0]
    _by_model[id(m)] = name
    return m


@pytest.fixture(autouse=True)
def one_engine_per_automaton(stcsp, monkeypatch):
    """The lookup: where a helper of another file would solve the model again, it gets the shared engine; where it takes a name,
    it finds the text under it (tests/test_services_fuzz.py); and the colour-only mask is among monitor_ref.masks()."""
    plain = M.masks
    monkeypatch.setattr(M, "masks", lambda model, r: {**plain(model, r), "colour": OR.only(model, "c")})

    def solved(stcsp, m, adversarial=-1, **opts):
        assert adversarial == -1 and not opts
        return device(stcsp, _by_model[id(m)])[1:]
    for module in (TGg, TRg, TIg, TMg):
        monkeypatch.setattr(module, "solved", solved)

    def device_classes(stcsp, m, adversarial=-1, **opts):
        _, e, r, post, _ = device(stcsp, _by_model[id(m)])
        return e, r, Q.post_flags(post)
    monkeypatch.setattr(TQg, "device_classes", device_classes)

    def device_case(stcsp, name, interval=False):
        m, e, r, post, host = device(stcsp, name)
        return m, e, r, Q.post_flags(post), host
    monkeypatch.setattr(TCg, "device_case", device_case)
    monkeypatch.setattr(TOg, "device_case", device_case)
    monkeypatch.setattr(TObg, "solved", lambda stcsp, name, **opts: device(stcsp, name))
    monkeypatch.setattr(TObg, "text_of", lambda stcsp, name: TEXT[name])

    def device_observer(stcsp, name, names):
        """(engine, its observer under the named variables): built anew, so that it is the engine's last one."""
        m, e = device(stcsp, name)[:2]
        e.generator(TCmpg.mask_of(m, names), 0)
        return e, e.observer()
    monkeypatch.setattr(TCmpg, "device_observer", device_observer)


def check_service(stcsp, RefOracle, service, name):
    """One existing device check on one table automaton, on the automaton's shared engine."""
    m = model_of(stcsp, name)
    large = oracle_shape(stcsp, RefOracle, name)["edges"] > 500
    if service == "generate":
        TGg.check_device(stcsp, RefOracle, m, name, horizon=24, masks=MASKS, n=40)
    elif service == "repair":
        TRg.check_device(stcsp, RefOracle, m, name, masks=MASKS, lengths=(6,) if large else (5, 12))
    elif service == "infer":
        TIg.check_device(stcsp, RefOracle, m, name, masks=MASKS, lengths=(6,) if large else (4, 9), engine=device(stcsp, name)[1:])
    elif service == "monitor":
        TMg.check_device(stcsp, RefOracle, m, name, masks=MASKS, n_walks=8, max_len=60)
    elif service == "quotient":
        TQg.check_device(stcsp, RefOracle, m, name)
    elif service == "observer":
        for which in ("default", "all", "only:c", M.hidden_signature_mask(m, device(stcsp, name)[2])):
            TObg.check_device(stcsp, RefOracle, name, which)
    elif service == "components":
        dev = TCg.check_device(stcsp, name, RefOracle=RefOracle)
        assert CR.same(TCg.check_device(stcsp, name, no_trim=True, RefOracle=RefOracle), dev)
    elif service.startswith("optimise"):
        weights = small_weights if service == "optimise-small" else big_weights
        TOg.check_device(stcsp, name, weights(m.n_vars), RefOracle=RefOracle)
    else:
        for which in OBSERVABLES:
            names = digits_of(name) if which == "digits" else which
            e, ol, orr, dev = TCmpg.check_device(stcsp, name, mutant(name), names)
            expect = CMP.product(oracle_observer(stcsp, RefOracle, name, names)[2], oracle_observer(stcsp, RefOracle, mutant(name), names)[2])
            assert CMP.same(dev, expect), f"{name} | mutant [{names}]: device and yardstick differ"


def test_the_engines_shapes_keep_the_floors(stcsp, RefOracle):
    """The floors of tests/test_services_fuzz.py on the engine's own export, and the oracle's live state counts."""
    shapes = {}
    for name in TABLES:
        m, e, r, post, host = device(stcsp, name)
        e.generator(OR.only(m, "c"), 0)
        shapes[name] = shape_of(r, *Q.post_flags(post), e.observer())
        print(shape_line(name, shapes[name]))
        want = oracle_shape(stcsp, RefOracle, name)
        assert all(shapes[name][k] == want[k] for k in want if k != "removed"), f"{name}: engine {shapes[name]} oracle {want}"
    check_floors(shapes)


@pytest.mark.parametrize("service", SERVICES)
@pytest.mark.parametrize("name", TABLES)
def test_device_against_twin_and_yardstick(stcsp, RefOracle, name, service):
    check_service(stcsp, RefOracle, service, name)


def answer(stcsp, service, name):
    """What one service answers on the shared engine, as a flat list of arrays and numbers: enough to see a disturbance."""
    m, e, r, post, host = device(stcsp, name)
    colour = OR.only(m, "c")
    rows = host.generate(6, 5, seed=2, observable=colour, horizon=5)[0] if host.n_live_states else np.zeros((6, 5, 1), np.int32)
    streams = list(rows) + [rows[0][:2], np.zeros((0, 1), np.int32)]
    if service == "generate":
        info = e.generator(colour, 12)
        return [info.count] + (list(e.generate(20, 12, seed=3)) if info.count[12] > 0 else [])
    if service in ("repair", "infer", "monitor"):
        e.generator(colour, 0)
        e.monitor(colour)
        if service == "monitor":
            return list(e.check_streams(streams)[:3])
        if service == "repair":
            dist, values, fin, nchg = e.repair_streams(streams, end_final=True)
            return [dist, fin, nchg] + list(values)
        count, supports, n_states, draws, fin = e.infer_streams(streams, draws=1, seed=1)
        return [count, fin] + list(n_states) + list(draws) + [np.array(str(supports))]
    if service == "quotient":
        return list(e.quotient(None)[:2])
    if service in ("observer", "compare"):
        e.generator(colour, 0)
        obs = e.observer()
        if service == "observer":
            return [obs[k] for k in TObg.ARRAYS]
        me, other = device(stcsp, mutant(name))[:2]
        other.generator(OR.only(me, "c"), 0)
        cmp = e.compare(other.observer())
        return [cmp[k] for k in CMP.ARRAYS] + [np.int64(cmp["n_pairs"])]
    if service == "components":
        res = e.components("all")
        return [res[k] for k in ("state_component", "state_omega", "comp_size", "comp_depth", "comp_flags")] + [x for lasso in res["lassos"] for x in lasso[1:]]
    res = e.optimise((small_weights if service == "optimise-small" else big_weights)(m.n_vars), horizon=9, lengths=[9], mean=True, state_best=True)
    return [res["best"], res["state_best"], res["state_component"], np.array(res["comp_mean"]), np.array(res["omega_mean"])] + list(res["witnesses"][0][1:])


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("name", ORDERED)
def test_services_share_one_engine_in_any_order(stcsp, RefOracle, name, order):
    """Every service's whole check, one after the other on one engine, forwards and backwards; what the first one answered before
    the others ran it answers again after the last."""
    first = ORDERS[order][0]
    before = answer(stcsp, first, name)
    for service in ORDERS[order]:
        check_service(stcsp, RefOracle, service, name)
    after = answer(stcsp, first, name)
    assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after)), f"{name}: {first} after {order}"
