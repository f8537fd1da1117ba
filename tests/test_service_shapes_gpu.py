"""The automaton services on the exports of every kernel family, on the device: the catalogue of tests/service_shapes.py through
the existing device checks of generate, repair, infer, monitor, quotient, observer, components, optimise and compare -- device
== host twin on the engine's own export == the plain Python yardstick on the CPU oracle's automaton, everything with `==`,
doubles by their bits. One engine per shape, created with the shape's prefix_k, flags and tuning switches and asserted to have
chosen the shape's kernels, so the arrays the services index (labels of N values, keys of KL words, the until flags behind the
signature) were written by that family; it is shared by the services through the lookups of tests/test_services_fuzz_gpu.py.
Every masked service runs under six masks, three of which reach the high variable indices. Beside them postprocess() against
tests/postproc_ref.py, the services in two orders on two shapes, and the INT_MIN contract of include/stcsp_engine.h on a
model whose labels take both ends of int32. Run on the GPU box: pytest -m gpu."""
import contextlib
import functools
import os

import numpy as np
import pytest

import compare_ref as CMP
import components_ref as CR
import generate_ref as G
import infer_ref as I
import kernel_matrix as km
import monitor_ref as M
import observer_ref as OR
import postproc_ref as PR
import quotient_ref as Q
import repair_ref as R
import service_shapes as S
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
from test_service_shapes import compare_names, oracle_figures  # (and the lookup of the texts by name)

pytestmark = pytest.mark.gpu

SERVICES = ("generate", "repair", "infer", "monitor", "quotient", "observer", "components", "optimise-small", "optimise-big", "compare")
ORDERS = {"forward": SERVICES, "backward": SERVICES[::-1]}
ORDERED = ("until_dr4_plain_kr2", "until_dr8_cs_kr2")  # KR = 2 with 63 until flags; N = 148
SWITCHES = ("STCSP_LITE", "STCSP_IMG_LDS", "STCSP_BIG", "STCSP_LITE_SHAPE", "STCSP_SMALL_POOLS", "STCSP_FORCE_CANDIDATES")
ENDS = "ends_of_int32"
X = S.INT_MIN  # STCSP_REPAIR_MISSING == STCSP_INFER_MISSING


@contextlib.contextmanager
def switches(env):
    """The engine's tuning switches of a kernel-matrix row, for as long as the engine is created and solves."""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def shape_of_key(key):
    return S.BY_NAME[key.split(":")[-1]]


def new_engine(stcsp, key):
    """(model, engine) of a shape or of its mutant; for a shape itself the kernels are asserted."""
    if key == ENDS:
        m = stcsp.Model(text=S.ENDS)
        e = stcsp.Engine(m, flags=stcsp.F_INTERVAL_DOMAINS)
        assert e.kernel_choice()["domain_form"] == km.INTERVALS
        return m, e
    s = shape_of_key(key)
    m = stcsp.Model(text=S.TEXT[key], prefix_k=s.prefix_k)
    e = stcsp.Engine(m, **({"flags": s.flags} if s.flags else {}))
    if key == S.key_of(s.name):
        k = e.kernel_choice()
        if s.row:
            assert k == km.choice(km.ROW[s.row]), f"{s.name}: {k}"
        else:
            assert (k["key_regs"], k["dom_regs"], k["domain_form"]) == s.regs, f"{s.name}: {k}"
    return m, e


@functools.lru_cache(maxsize=None)
def device(stcsp, key):
    """(model, engine, Result, PostResult, the host's automaton with the device's flags): solved and post-processed once."""
    with switches({} if key == ENDS else shape_of_key(key).env):
        m, e = new_engine(stcsp, key)
        r = e.solve()
        assert not r.truncated
        post = e.postprocess()
    return m, e, r, post, e.automaton(r).import_flags(post)


_by_model = {}  # id(model) -> key: the helpers that take a model are given the one device() made


def model_of(stcsp, key):
    m = device(stcsp, key)[0]
    _by_model[id(m)] = key
    return m


@pytest.fixture(autouse=True)
def one_engine_per_shape(stcsp, monkeypatch):
    """The lookups of tests/test_services_fuzz_gpu.py: where a helper of another file would solve the model again it gets the
    shared engine, and where it takes a name it finds the text under it."""
    def solved(stcsp, m, adversarial=-1, **opts):
        assert adversarial == -1 and not opts
        return device(stcsp, _by_model[id(m)])[1:]
    for module in (TGg, TRg, TIg, TMg):
        monkeypatch.setattr(module, "solved", solved)

    def device_classes(stcsp, m, adversarial=-1, **opts):
        _, e, r, post, _ = device(stcsp, _by_model[id(m)])
        return e, r, Q.post_flags(post)
    monkeypatch.setattr(TQg, "device_classes", device_classes)

    def device_case(stcsp, key, interval=False):
        m, e, r, post, host = device(stcsp, key)
        return m, e, r, Q.post_flags(post), host
    monkeypatch.setattr(TCg, "device_case", device_case)
    monkeypatch.setattr(TOg, "device_case", device_case)
    monkeypatch.setattr(TObg, "solved", lambda stcsp, key, **opts: device(stcsp, key))
    monkeypatch.setattr(TObg, "text_of", lambda stcsp, key: S.TEXT[key])

    def device_observer(stcsp, key, names):
        """(engine, its observer under the named variables): built anew, so that it is the engine's last one."""
        m, e = device(stcsp, key)[:2]
        e.generator(TCmpg.mask_of(m, names), 0)
        return e, e.observer()
    monkeypatch.setattr(TCmpg, "device_observer", device_observer)


@pytest.fixture
def masks(monkeypatch):
    plain = M.masks

    def use(name):
        monkeypatch.setattr(M, "masks", S.masks_for(plain, S.BY_NAME[name]))
    return use


def check_service(stcsp, RefOracle, service, name):
    """One existing device check on one shape, on the shape's shared engine, under all six masks where the service takes one."""
    s = S.BY_NAME[name]
    key, k = S.key_of(name), s.prefix_k
    m = model_of(stcsp, key)
    large, huge = S.large(oracle_figures(stcsp, RefOracle, name)), S.huge(oracle_figures(stcsp, RefOracle, name))
    if service == "generate":
        TGg.check_device(stcsp, RefOracle, m, name, horizon=24, masks=S.MASKS, n=40)
    elif service == "repair":
        TRg.check_device(stcsp, RefOracle, m, name, masks=S.MASKS, lengths=(2,) if huge else (6,) if large else (5, 12))
    elif service == "infer":
        TIg.check_device(stcsp, RefOracle, m, name, masks=S.MASKS, lengths=(3,) if huge else (6,) if large else (4, 9), engine=device(stcsp, key)[1:])
    elif service == "monitor":
        TMg.check_device(stcsp, RefOracle, m, name, masks=S.MASKS, n_walks=8, max_len=60)
    elif service == "quotient":
        TQg.check_device(stcsp, RefOracle, m, name)
    elif service == "observer":
        for which, mask in M.masks(m, device(stcsp, key)[2]).items():
            TObg.check_device(stcsp, RefOracle, key, which if which in ("default", "all") else mask, prefix_k=k)
    elif service == "components":
        dev = TCg.check_device(stcsp, key, RefOracle=RefOracle, prefix_k=k)
        assert CR.same(TCg.check_device(stcsp, key, no_trim=True, RefOracle=RefOracle, prefix_k=k), dev)
    elif service.startswith("optimise"):
        weights = small_weights if service == "optimise-small" else big_weights
        TOg.check_device(stcsp, key, weights(m.n_vars), RefOracle=RefOracle, prefix_k=k)
    else:
        model_of(stcsp, S.mutant_key(name))
        for which in ("behaviour", "all"):
            names = compare_names(name, which)
            e, ol, orr, dev = TCmpg.check_device(stcsp, key, S.mutant_key(name), names)
            expect = CMP.product(oracle_observer(stcsp, RefOracle, key, names, k)[2], oracle_observer(stcsp, RefOracle, S.mutant_key(name), names, k)[2])
            assert CMP.same(dev, expect), f"{name} | mutant [{which}]: device and yardstick differ"
            assert dev["witness_len"][0] >= 0 and dev["witness_len"][1] == -1


def test_the_engines_exports_have_the_shapes(stcsp, RefOracle):
    """Every shape's kernels (asserted where its engine is made), and the figures of the catalogue on the engine's own export."""
    figs = {}
    for name in S.NAMES:
        m, e, r, post, host = device(stcsp, S.key_of(name))
        figs[name] = S.figures(m, r, *Q.post_flags(post), CR)
        print(S.line(name, figs[name]))
        want = oracle_figures(stcsp, RefOracle, name)
        assert all(figs[name][k] == want[k] for k in want if k != "removed"), f"{name}: engine {figs[name]} oracle {want}"
    S.check_floors(figs)


@pytest.mark.parametrize("service", SERVICES)
@pytest.mark.parametrize("name", S.NAMES)
def test_device_against_twin_and_yardstick(stcsp, RefOracle, masks, name, service):
    masks(name)
    check_service(stcsp, RefOracle, service, name)


@pytest.mark.parametrize("name", S.NAMES)
def test_postprocess_against_the_yardstick(stcsp, name):
    """The traverse, and `adversarial` over one narrow variable (the last behaviour variable, of at most eight values), on an engine of its own against
    tests/postproc_ref.py: the passes read the until flags behind the signature, at the key's stride."""
    s = S.BY_NAME[name]
    with switches(s.env):
        m, e = new_engine(stcsp, S.key_of(name))
        r = e.solve()
    g = PR.graph(r)
    start = PR.traverse(g)
    narrow = m.var_names.index(s.behaviour.split(",")[-1])
    lo, hi = m.var_bounds()[narrow]
    assert hi - lo < 8
    for adv in (-1, narrow):
        want = PR.run(g, m.var_bounds(), adv, None, start)
        post = e.postprocess(adversarial=adv)
        got = PR.post_flags(post)
        assert (post.n_states, post.n_edges) == (r.n_states, r.n_edges)
        assert PR.same_flags(got, want, g.src, g.dst, False), f"{name} adv={adv}: {PR.first_difference(got, want, g.src, g.dst, False)}"
        assert (post.adver1, post.adver2) == want.ret, f"{name} adv={adv}"
    e.close()


def answer(stcsp, service, name):
    """What one service answers on the shared engine, as a flat list of arrays and numbers: enough to see a disturbance."""
    m, e, r, post, host = device(stcsp, S.key_of(name))
    mask = S.extra_masks(S.BY_NAME[name], m.var_names)["behaviour"]
    n_obs = sum(mask)
    rows = host.generate(6, 5, seed=2, observable=mask, horizon=5)[0]
    streams = list(rows) + [rows[0][:2], np.zeros((0, n_obs), np.int32)]
    if service == "generate":
        info = e.generator(mask, 12)
        return [info.count] + list(e.generate(20, 12, seed=3))
    if service in ("repair", "infer", "monitor"):
        e.generator(mask, 0)
        e.monitor(mask)
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
        e.generator(mask, 0)
        obs = e.observer()
        if service == "observer":
            return [obs[k] for k in TObg.ARRAYS]
        other = device(stcsp, S.mutant_key(name))[1]
        other.generator(mask, 0)
        cmp = e.compare(other.observer())
        return [cmp[k] for k in CMP.ARRAYS] + [np.int64(cmp["n_pairs"])]
    if service == "components":
        res = e.components("all")
        return [res[k] for k in ("state_component", "state_omega", "comp_size", "comp_depth", "comp_flags")] + [x for lasso in res["lassos"] for x in lasso[1:]]
    res = e.optimise((small_weights if service == "optimise-small" else big_weights)(m.n_vars), horizon=9, lengths=[9], mean=True, state_best=True)
    return [res["best"], res["state_best"], res["state_component"], np.array(res["comp_mean"]), np.array(res["omega_mean"])] + list(res["witnesses"][0][1:])


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("name", ORDERED)
def test_services_share_one_engine_in_any_order(stcsp, RefOracle, masks, name, order):
    """Every service's whole check, one after the other on one engine, forwards and backwards; what the first one answered before
    the others ran it answers again after the last."""
    masks(name)
    first = ORDERS[order][0]
    before = answer(stcsp, first, name)
    for service in ORDERS[order]:
        check_service(stcsp, RefOracle, service, name)
    after = answer(stcsp, first, name)
    assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after)), f"{name}: {first} after {order}"


# ------------------------------------------------------------------------------------------------ INT_MIN in rows: the contract
def ends_weights(n):
    """3 * INT_MIN and -5 * (INT_MIN + 1) leave 32 bits; nine steps of them stay far inside the optimiser's exact range."""
    return [1, 3, -5, 1] + [0] * (n - 4)


def test_int_min_is_a_value_on_output_and_unobserved_on_input(stcsp):
    """include/stcsp_engine.h beside STCSP_REPAIR_MISSING: in an input row of repair and infer INT_MIN is "not observed" and
    matches any value; output rows carry INT_MIN wherever an edge has it; the monitor has no MISSING and takes INT_MIN as the
    value it is. Device == host twin == yardstick, the latter two on the engine's own export: the CPU oracle does not finish a
    variable over the whole int range."""
    m, e, r, post, a = device(stcsp, ENDS)
    flags = Q.post_flags(post)
    mask = [int(n in ("v", "u")) for n in m.var_names]
    val = Q.result_arrays(r)[2]
    assert {S.INT_MIN, S.INT_MIN + 1, -1, S.INT_MAX} <= set(val[[k for k in range(r.n_edges) if flags[2][k]]].ravel().tolist())
    lo, hi = [S.INT_MIN, S.INT_MIN + 1], [S.INT_MAX, -1]   # (v, u) at s == 0 and at s == 1
    # generate: every stream alternates the two rows, INT_MIN among its values
    e.generator(mask, 5)
    dev = e.generate(4, 5, 0)
    twin = a.generate(4, 5, 0, observable=mask, horizon=5)
    yv, yf = G.Yardstick(r, *flags, mask, 5).streams(4, 5, 0)
    assert np.array_equal(dev[0], twin[0]) and np.array_equal(dev[0], yv) and np.array_equal(dev[1], yf)
    assert all(s.tolist() == [lo, hi, lo, hi, lo] for s in dev[0])
    # monitor: INT_MIN is matched as a value: accepted where the edge has it, rejected where the edge has INT_MAX
    e.generator(mask, 0)
    e.monitor(mask)
    streams = [np.array([lo, hi, lo], np.int32), np.array([lo, lo], np.int32), np.array([[S.INT_MIN, -1]], np.int32)]
    dev, twin, yard = e.check_streams(streams), a.check_streams(streams, mask), M.Yardstick(r, *flags, mask).check_all(streams)
    assert dev[0].tolist() == [3, 1, 0] and TMg.same(dev, twin) and TMg.same(dev, yard)
    # repair: an observed INT_MAX at s == 0 is repaired to the value INT_MIN; INT_MIN in the input costs nothing anywhere
    yr = R.Yardstick(r, *flags, mask)
    streams = [np.array([[S.INT_MAX, S.INT_MIN + 1], hi], np.int32), np.array([[X, S.INT_MIN + 1], [X, -1], [X, X]], np.int32),
               np.array([hi, hi], np.int32)]
    for kw in (dict(), dict(end_final=True), dict(weights=[3, 2])):
        dev = e.repair_streams(streams, **kw)
        assert TRg.same(dev, a.repair_streams(streams, mask, **kw)) and R.unpack(dev) == [yr.dp(s, **kw) for s in streams], kw
    got = R.unpack(e.repair_streams(streams))
    assert [g[0] for g in got] == [1, 0, 2] and got[0][1] == [lo, hi] and got[1][1] == [lo, hi, lo] and got[2][1] == [lo, hi]
    # infer: the support of an unobserved v at s == 0 is {INT_MIN}, and the draws carry it
    yi = I.Yardstick(r, *flags, mask)
    streams = [np.array([[X, S.INT_MIN + 1], [X, X]], np.int32), np.array([[X, X]], np.int32), np.array([[S.INT_MAX, X]], np.int32)]
    for end_final in (False, True):
        dev = e.infer_streams(streams, end_final=end_final, draws=1, seed=1)
        assert TIg.same(dev, a.infer_streams(streams, mask, end_final=end_final, draws=1, seed=1))
        for i, (s, got) in enumerate(zip(streams, I.unpack(dev))):
            count, supports, n_states = yi.dp(s, end_final)
            assert got[:3] == (I.bits(count), supports, n_states), f"stream {i} end_final={end_final}"
            expect = yi.walk(s, i, end_final, 1) if count > 0 else ([[X] * 2] * len(s), 0)
            assert (got[3][0], got[4][0]) == expect
    count, supports, n_states, draws, dfin = e.infer_streams(streams, draws=1, seed=1)
    assert count.tolist() == [4.0, 2.0, 0.0] and supports[0][0][0] == [S.INT_MIN] and supports[0][1][0] == [S.INT_MAX]
    assert draws[0][0].tolist() == [lo, hi] and draws[1][0].tolist() == [lo] and draws[2][0].tolist() == [[X, X]]


def test_services_on_the_ends_of_int32(stcsp):
    """Monitor, quotient, observer and optimise through their own device checks, against the twin and against the yardsticks on the
    engine's export; the optimiser's costs 3 * INT_MIN and -5 * (INT_MIN + 1) need 64 bits."""
    m = model_of(stcsp, ENDS)
    _, e, r, post, a = device(stcsp, ENDS)
    valid, final, alive = Q.post_flags(post)
    TMg.check_device(stcsp, None, m, ENDS, oracle=False, masks=("default", "all", "hidden"), n_walks=8, max_len=40)
    TQg.check_device(stcsp, None, m, ENDS, oracle=False)
    for name, mask in {"default": Q.default_mask(m.var_names), "all": [1] * m.n_vars}.items():
        cls, n_classes = e.quotient(None if name == "default" else "all")[:2]
        part, yn = Q.yardstick(m, r, valid, final, alive, mask)[:2]
        assert n_classes == yn and Q.engine_partition(r, valid, alive, cls) == part, name
    for which in ("default", "all", "only:v", "only:u"):
        mask, dev = TObg.check_device(stcsp, None, ENDS, which, oracle=False)[3:]
        expect = OR.subset_construction(M.Yardstick(r, valid, final, alive, mask))
        assert OR.normalised(dev, OR.numbers_of(r, valid, alive)) == expect, which
    w = ends_weights(m.n_vars)
    TOg.check_device(stcsp, ENDS, w)
    res = e.optimise(w, horizon=2, lengths=[1, 2])
    first = 3 * S.INT_MIN - 5 * (S.INT_MIN + 1)   # s == 0, f == 0
    second = 1 + 3 * S.INT_MAX + 5                # s == 1, f == 0
    assert res["best"].tolist() == [0, first, first + second] and abs(3 * S.INT_MIN) > 2 ** 32
    assert res["witnesses"][0][1].tolist()[0][1:3] == [S.INT_MIN, S.INT_MIN + 1]
