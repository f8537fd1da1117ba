"""Fair CTL over the infinite solutions on the device (stcsp_engine_ctl, dev_ctl.hpp) through the C ABI: device == host twin on
the engine's own automaton, array by array and witness by witness, == the yardstick of tests/ctl_ref.py on the CPU oracle's
automaton wherever the oracle runs in seconds. Run on the GPU box: pytest -m gpu."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import ctl_ref as T
import quotient_ref as Q
import service_shapes as S
from fuzz_models import table_by_name, until_chain
from test_components import text_of
from test_ctl import ALONE, MALFORMED, NESTED, at_the_node_limit, atoms_for, case, slot_chain
from test_services_fuzz import TABLES

pytestmark = pytest.mark.gpu

# a saturating counter with a stay-for-ever branch: c counts up to 5 and holds there while b == 0; once b == 1 it stands still
COUNTER5 = ("var c:[0,5]; var b:[0,1]; first c == 0; first b == 0; "
            "next c == if (b eq 1) then c else (if (c lt 5) then (c + 1) else c); next b >= b;")
NEGATIVE = "var x:[-70,50]; x >= -70;"  # 121 values, W = 4 words of domain, negative values on the edges
CRAFTED = {"COUNTER5": COUNTER5, "NEGATIVE": NEGATIVE, "CHAIN70": until_chain(70)}


def loops(n):
    """One state with n self-loops: x is free."""
    return f"var x:[0,{n - 1}]; x >= 0;"


def text_for(stcsp, name):
    if name.startswith("loops:"):
        return loops(int(name[6:]))
    if name.startswith("table:"):
        return table_by_name(name)
    return CRAFTED[name] if name in CRAFTED else text_of(stcsp, name)


@functools.lru_cache(maxsize=None)
def device_case(stcsp, name, interval=False):
    """(model, engine, Result, (valid, final, alive), the host's automaton with the device's flags): solved and post-processed once.
    More than 128 values per variable need interval domains."""
    interval = interval or (name.startswith("loops:") and int(name[6:]) > 128)
    m = stcsp.Model(text=text_for(stcsp, name))
    e = stcsp.Engine(m, flags=stcsp.F_INTERVAL_DOMAINS if interval else 0)
    r = e.solve()
    assert not r.truncated
    post = e.postprocess()
    return m, e, r, Q.post_flags(post), e.automaton(r).import_flags(post)


@functools.lru_cache(maxsize=None)
def oracle_worlds(stcsp, RefOracle, name):
    if name in CRAFTED or name.startswith("loops:"):
        m = stcsp.Model(text=text_for(stcsp, name))
        o = RefOracle(m)
        r = o.solve()
        flags = o.automaton(r).traverse().flags()
        return m, r, flags, T.Worlds(r, *flags), o
    m, r, _, flags, w, o = case(stcsp, RefOracle, name)
    return m, r, flags, w, o


def check_device(stcsp, name, text, RefOracle=None, interval=False, got=None):
    """Device == twin, exactly: the verdict arrays and the witness; with RefOracle also == the yardstick on the oracle's automaton, by
    canonical state numbers and full rows."""
    m, e, r, (valid, final, alive), a = got or device_case(stcsp, name, interval)
    dev = e.ctl(text, witness=True)
    twin = a.ctl(text, witness=True)
    assert T.same(dev, twin), f"{name}: {text}: device and host twin differ"
    assert dev["seconds"] > 0 and dev["rounds"][2] >= 0
    plain = e.ctl(text)
    assert plain["witness"][0] == "none" and np.array_equal(plain["edge_sat"], dev["edge_sat"])
    if RefOracle is not None:
        om, orr, (ov, of, oa), w, _ = oracle_worlds(stcsp, RefOracle, name)
        ref = w.result(T.parse(text, om.var_names), witness=True)
        assert T.signature(r, valid, alive, dev) == T.signature(orr, ov, oa, ref), f"{name}: {text}: device and yardstick differ"
        assert T.witness_rows(dev) == ref["witness"], f"{name}: {text}"
    return dev


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129])
def test_world_counts_around_the_word_boundaries(stcsp, RefOracle, n):
    """n self-loops on one state: n worlds, all initial. The last world's bit is the last bit of the last set word for n = 64 and 128
    and the first of a new word for 65 and 129; n = 100 and 129 give the witness walk a segment of more than 64 and 128 candidates."""
    name = f"loops:{n}"
    top = n - 1
    for text in ("true", f"x == {top}", f"!x == {top}", f"EX x == {top}", f"AX x < {top}", f"EG x == {top}", f"AG EF x == {top}", f"E[x < {top} U x == {top}]",
                 f"EF x == {top}", f"AF x == {top}", f"A[x >= 0 U x == {top}]", f"!EX x == {top}", "!EG true", f"EX x >= {n}"):
        dev = check_device(stcsp, name, text, RefOracle)
        assert (dev["n_worlds"], dev["n_initial"]) == (n, n)
    assert check_device(stcsp, name, f"AG EF x == {top}")["holds"]
    assert int(check_device(stcsp, name, f"x == {top}")["edge_sat"].sum()) == 1
    assert check_device(stcsp, name, "!false")["n_initial_sat"] == n  # the tail bits past n_worlds stay 0 under !


def test_witness_ties(stcsp, RefOracle):
    """All candidates of a step tie on the distance: the least full row wins, at both steps, over a segment of 100 candidates."""
    dev = check_device(stcsp, "loops:100", "EX x >= 0", RefOracle)
    assert dev["witness"][0] == "witness" and dev["witness"][1][:, 0].tolist() == [0, 0]
    dev = check_device(stcsp, "loops:100", "EX x >= 70", RefOracle)
    assert dev["witness"][1][:, 0].tolist() == [0, 70]
    dev = check_device(stcsp, "loops:129", "E[x > 100 U x < 3]", RefOracle)
    assert dev["witness"][1][:, 0].tolist() == [0]  # the initial world of distance 0 with the least row
    dev = check_device(stcsp, "loops:129", "E[x > 100 U (x < 3 & false)] | true", RefOracle)
    assert dev["witness"][0] == "none"
    dev = check_device(stcsp, "loops:129", "AG x < 128", RefOracle)
    assert dev["witness"][0] == "counterexample" and dev["witness"][1][:, 0].tolist() == [128]
    dev = check_device(stcsp, "loops:129", "AX x < 128", RefOracle)
    assert dev["witness"][0] == "counterexample" and dev["witness"][1][:, 0].tolist() == [0, 128]


@pytest.mark.parametrize("name", ["FUSE", "FUSE_UNTIL", "random:0"])
def test_no_worlds(stcsp, RefOracle, name):
    for text in ("true", "false", "EG true", "AG EF false"):
        dev = check_device(stcsp, name, text, RefOracle)
        assert (dev["n_worlds"], dev["n_initial"], dev["n_initial_sat"]) == (0, 0, 0) and dev["vacuous"] and dev["holds"]
        assert not dev["edge_world"].any() and dev["witness"][0] == "none"


def test_an_eg_that_needs_outer_rounds(stcsp, RefOracle):
    """COUNTER5 under EG (c < 5 & b == 0): every world is final, so a round of Emerson-Lei removes exactly the worlds whose successors
    inside the set are all gone: c == 4 first, then c == 3, .. -- one layer per outer round, five layers and the round that confirms.
    The set ends empty. A pass that stops after one round keeps c <= 3."""
    dev = check_device(stcsp, "COUNTER5", "EG (c < 5 & b == 0)", RefOracle)
    assert dev["rounds"][1] >= 3 and not dev["edge_sat"].any() and dev["n_worlds"] > 0
    dev = check_device(stcsp, "COUNTER5", "EG c < 5", RefOracle)  # staying below 5 for ever: raise b in time
    assert dev["possible"] and dev["rounds"][1] >= 2
    for text in ("AF c == 5", "AF (c == 5 | b == 1)", "EG (c < 3 & b == 0) | EG c < 2", "E[c < 4 U EG (c < 5 & b == 0)]"):
        check_device(stcsp, "COUNTER5", text, RefOracle)


def test_an_eu_chain_of_more_than_64_levels(stcsp, RefOracle):
    m, e, r, flags, a = device_case(stcsp, "CHAIN70")
    dev = check_device(stcsp, "CHAIN70", "E[y == 0 U y == 1]", RefOracle)
    ref = oracle_worlds(stcsp, RefOracle, "CHAIN70")[3].result(T.parse("E[y == 0 U y == 1]", m.var_names), witness=True)
    assert dev["witness"][0] == "witness" and len(dev["witness"][1]) == len(ref["witness"][1]) > 64
    assert dev["rounds"][0] > 64
    for text in ("AF y == 1", "AG (y == 1 -> AG y == 1)", "EF x == 70", "AG x < 70", "A[y == 0 U x == 70]"):
        check_device(stcsp, "CHAIN70", text, RefOracle)


def raw(stcsp, e, words, flags=0):
    prog = np.asarray(words, np.int32)
    rq, out = stcsp.CtlRequest(prog.ctypes.data_as(C.POINTER(C.c_int32)), prog.size, flags), stcsp.CtlResult()
    return e._f("ctl")(e._h, C.byref(rq), C.byref(out))


def test_the_limits_on_the_device(stcsp):
    """A step predicate at the node limit and one past it; nesting at the slot limit and one past it; the stack of 64."""
    m, e, r, flags, a = device_case(stcsp, "LADDER")
    under, at, over = at_the_node_limit(stcsp)
    for words in (under, at, [stcsp.CTL_TRUE] * 64 + [stcsp.CTL_AND] * 63, slot_chain(stcsp, 14)):
        assert T.same(e.ctl(words, witness=True), a.ctl(words, witness=True))
    assert e.ctl(under)["holds"] and not e.ctl(at)["possible"] and e.ctl(slot_chain(stcsp, 14))["holds"]
    # 128 atoms that all matter: m >= 0 & .. & m >= 0 & m == 3 is m == 3
    im = m.var_names.index("m")
    words = [stcsp.CTL_CMP_CONST, im, 5, 0] + [stcsp.CTL_CMP_CONST, im, 5, 0, stcsp.CTL_AND] * 126 + [stcsp.CTL_CMP_CONST, im, 0, 3, stcsp.CTL_AND]
    assert np.array_equal(e.ctl(words)["edge_sat"], e.ctl("m == 3")["edge_sat"]) and e.ctl("m == 3")["edge_sat"].any()
    for words in (over, [stcsp.CTL_TRUE] * 65 + [stcsp.CTL_AND] * 64, slot_chain(stcsp, 15)):
        with pytest.raises(stcsp.StcspError) as ex:
            e.ctl(words)
        assert ex.value.code == -2 and "ctl:" in str(ex.value)
    for words in MALFORMED:
        assert raw(stcsp, e, words) == -1, words
    with pytest.raises(stcsp.StcspError) as ex:
        e.ctl([stcsp.CTL_CMP_CONST, 1000, 0, 0])
    assert ex.value.code == -1 and "out of range" in str(ex.value)


MODELS = ["LADDER", "LADDER_UNTIL", "TRAP", "juggling_b4_f4_nosym", "juggling_b4_f5", "digitinvader3", TABLES[4], TABLES[5], TABLES[10], TABLES[11]]


@pytest.mark.parametrize("name", MODELS)
def test_device_on_the_models(stcsp, RefOracle, name):
    om, _, _, w, _ = oracle_worlds(stcsp, RefOracle, name)
    p, q = atoms_for(w, om.var_names)
    for f in ALONE + NESTED:
        check_device(stcsp, name, f.format(p=p, q=q), RefOracle, interval=name == TABLES[10])  # (a variable of 200 values)


def test_interval_domains_and_negative_values(stcsp, RefOracle):
    om, _, _, w, _ = oracle_worlds(stcsp, RefOracle, "juggling_b4_f5")
    p, q = atoms_for(w, om.var_names)
    for f in ALONE[5:] + NESTED[:6]:
        check_device(stcsp, "juggling_b4_f5", f.format(p=p, q=q), RefOracle, interval=True)
    for interval in (False, True):
        for text in ("x < -64", "EF x < -64", "EX x < -69", "AG x >= -70", "E[x < 0 U x > -1]", "AX x > -70", "x <= -70 | x >= 50", "x != -2147483648"):
            dev = check_device(stcsp, "NEGATIVE", text, RefOracle, interval=interval)
            assert dev["n_worlds"] == 121
        assert int(e_sat(stcsp, "NEGATIVE", "x < -64", interval)) == 6 and int(e_sat(stcsp, "NEGATIVE", "x > -2147483648", interval)) == 121


def e_sat(stcsp, name, text, interval):
    return device_case(stcsp, name, interval)[1].ctl(text)["edge_sat"].sum()


def test_rows_and_keys_of_more_than_64_words(stcsp):
    """N = 148 variables under a key of 65 words: the row stride is N, and atoms read variables past index 64 and the last one."""
    from test_service_shapes_gpu import device
    m, e, r, post, a = device(stcsp, S.key_of("until_dr8_cs_kr2"))
    assert m.n_vars == 148
    names = m.var_names
    got = (m, e, r, Q.post_flags(post), a)
    _, _, val = Q.result_arrays(r)
    world = a.ctl("true")["edge_world"].astype(bool)
    assert world.any()
    for v in (0, 63, 64, 65, 127, 128, 147):
        k = int(np.bincount(val[world][:, v] - val[world][:, v].min()).argmax() + val[world][:, v].min())
        for f in ("{p}", "EF {p}", "AG {p}", "EG {p}", "A[{p} U p == 3]", "E[g0 == 0 U {p}]", f"{names[v]} <= {names[147 - v]}"):
            dev = check_device(stcsp, "until_dr8_cs_kr2", f.format(p=f"{names[v]} == {k}"), got=got)
        assert np.array_equal(e.ctl(f"{names[v]} == {k}")["edge_sat"].astype(bool), world & (val[:, v] == k))


def test_twin_alone_on_a_larger_instance(stcsp):
    name = "partialorder_14"
    m, e, r, flags, a = device_case(stcsp, name)
    names = m.var_names
    p = f"{names[0]} == 0"
    for text in (f"AG EF {p}", f"EG {p}", f"EG !{p}", f"EF {p}"):
        dev = check_device(stcsp, name, text)
        assert dev["n_worlds"] > 100000


def test_the_byte_budget(stcsp):
    m, e, r, flags, a = device_case(stcsp, "digitinvader3")
    saved = os.environ.get("STCSP_CTL_BYTES")
    try:
        os.environ["STCSP_CTL_BYTES"] = "4096"
        with pytest.raises(stcsp.StcspError) as ex:
            e.ctl("AG EF true")
        assert ex.value.code == -4 and "STCSP_CTL_BYTES" in str(ex.value) and "4096" in str(ex.value) and "need" in str(ex.value)
        os.environ["STCSP_CTL_BYTES"] = str(1 << 20)
        assert e.ctl("AG EF true")["holds"]
    finally:
        os.environ.pop("STCSP_CTL_BYTES", None)
        if saved is not None:
            os.environ["STCSP_CTL_BYTES"] = saved
    assert e.ctl("AG EF true")["holds"]


def test_error_paths(stcsp):
    m = stcsp.Model.from_name("partialorder_10")
    e = stcsp.Engine(m)
    ok = [stcsp.CTL_TRUE]
    assert raw(stcsp, e, ok) == -6  # before any solve
    e.solve()
    assert raw(stcsp, e, ok) == -6  # before postprocess
    with pytest.raises(stcsp.StcspError) as ex:
        e.ctl("true")
    assert ex.value.code == -6 and "postprocess" in str(ex.value)
    e.postprocess()
    assert raw(stcsp, e, ok) == 0 and raw(stcsp, e, []) == -1
    out = stcsp.CtlResult()
    assert e._f("ctl")(e._h, None, C.byref(out)) == -1
    e.solve()  # a new solve ends the flags' validity
    assert raw(stcsp, e, ok) == -6
    t = stcsp.Engine(m, max_search_nodes=2000, batch_nodes=256)  # truncated solve
    assert t.solve().truncated == 1
    t.postprocess()
    with pytest.raises(stcsp.StcspError) as ex:
        t.ctl("true")
    assert ex.value.code == -6 and "truncated" in str(ex.value)
    s = stcsp.Engine(m, flags=stcsp.F_STEPPED)  # the sharded pipeline
    with pytest.raises(stcsp.StcspError) as ex:
        s.ctl("true")
    assert ex.value.code == -2 and "stcsp_automaton_ctl" in str(ex.value)
    with pytest.raises(stcsp.CtlSyntaxError):
        s.ctl("nonsense ==")


@pytest.mark.parametrize("first", [True, False])
def test_other_services_are_not_disturbed(stcsp, first):
    """monitor, generator, repair, infer, observer, compare and optimise give the same with a ctl() call between build and use, before
    or after the first use; a components() result is replaced by an equal one."""
    import components_ref as R
    m = stcsp.Model.from_name("juggling_b4_f5")
    e = stcsp.Engine(m)
    e.solve()
    e.postprocess()
    mask = [int(n == "A") for n in m.var_names]
    e.monitor(mask)
    e.generator(mask, 6)
    obs = e.observer()
    streams = [obs["edge_values"][:1], np.zeros((0, 1), np.int32)]
    weights = [1] * m.n_vars
    formula = f"AG EF {m.var_names[0]} == 0"

    def use():
        acc, nend, fin, _ = e.check_streams(streams)
        values, gfin = e.generate(5, 6, ranks=[0, 1, 2, 3, 4])
        cmp = e.compare(obs)
        opt = e.optimise(weights, horizon=4, lengths=[4])
        inf = e.infer_streams(streams)
        return [acc, nend, fin, values, gfin, e.repair_streams(streams)[0], cmp["witness_len"], np.int64(cmp["n_pairs"]), opt["best"], inf[0]]
    comps = e.components("all")
    if first:
        res = e.ctl(formula, witness=True)
        before = use()
    else:
        before = use()
        res = e.ctl(formula, witness=True)
    assert res["n_worlds"] == 224
    after = use()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    again = e.observer()
    assert all(np.array_equal(obs[k], again[k]) for k in ("member_off", "member", "state_final", "edge_src", "edge_dst", "edge_values"))
    assert R.same(e.components("all"), comps)
    assert T.same(e.ctl(formula, witness=True), res)
