"""The observer (subset construction), host side (include/stcsp_host.h: stcsp_automaton_observer / stcsp_automaton_from_observer):
the CPU twin of the device pass against an independent yardstick -- the plain Python subset construction of tests/observer_ref.py,
run on the automaton of the CPU oracle -- and the properties the builder's automaton must have. The device pass itself:
tests/test_observer_gpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import monitor_ref as M
import observer_ref as R
import quotient_ref as Q
from fuzz_models import random_model
from test_monitor import NO_LIVE_ROOT
from test_quotient import COUNTDOWN, COUNTER, DUPLICATES, PROBES

WITNESSES = {"counter": COUNTER, "countdown": COUNTDOWN, "duplicates": DUPLICATES}
SMALL = {**WITNESSES, "crafted3": R.CRAFTED % (3, 3), "juggling_b4_f4": None, "digitinvader1": None}


def model_of(stcsp, name, prefix_k=2):
    if name.startswith("crafted"):
        k = int(name[7:])
        return stcsp.Model(text=R.CRAFTED % (k, k), prefix_k=prefix_k)
    if name in PROBES:
        return stcsp.Model(text=PROBES[name]["text"], prefix_k=prefix_k)
    return stcsp.Model(text=SMALL[name], prefix_k=prefix_k) if SMALL.get(name) else stcsp.Model.from_name(name, prefix_k)


def masks_of(model, r):
    """default, all, the hidden-signature mask and one single-variable mask (the first variable that is no `_V`)."""
    first = next(n for n in model.var_names if not n.startswith("_V"))
    return {**M.masks(model, r), "only:" + first: R.only(model, first)}


@functools.lru_cache(maxsize=4)
def _oracle(stcsp, RefOracle, name, adversarial, prefix_k=2):
    m = model_of(stcsp, name, prefix_k)
    o = RefOracle(m)
    r = o.solve()
    a = o.automaton(r).traverse()
    if adversarial is not None:
        a.adversarial(adversarial)
    return m, o, r, a


def twin_against_yardstick(stcsp, RefOracle, name, which, adversarial=None, prefix_k=2):
    """Twin == yardstick: member sets by canonical number, final flags, edges (src, row, dst), levels. Returns what a test needs."""
    m, o, r, a = _oracle(stcsp, RefOracle, name, adversarial, prefix_k)
    mask = which if isinstance(which, list) else R.resolve_mask(m, which)
    valid, final, alive = a.flags()
    y = M.Yardstick(r, valid, final, alive, mask)
    expect = R.subset_construction(y)
    obs = a.observer(mask)
    R.check_shape(obs)
    assert R.normalised(obs, R.numbers_of(r, valid, alive)) == expect, f"{name} [{which}]"
    assert obs["n_observable"] == sum(mask) and obs["n_labels"] == len({p for _, p, _ in y.edges})
    return m, r, a, y, mask, obs, expect


@pytest.mark.parametrize("name,which", list(R.TABLE))
def test_twin_matches_yardstick_on_the_table(stcsp, RefOracle, name, which):
    m, r, a, y, mask, obs, (sets, final, edges, levels) = twin_against_yardstick(stcsp, RefOracle, name, which)
    assert (len(y.live), len(y.edges), len(sets), len(edges), max(map(len, sets)), levels) == R.TABLE[(name, which)]
    assert (obs["n_states"], obs["n_edges"], obs["max_set"], obs["levels"]) == R.TABLE[(name, which)][2:]


@pytest.mark.parametrize("name", ["until", "arr", "at", "misc", "adversarial", "counter", "countdown", "duplicates"])
def test_twin_matches_yardstick_on_probes_and_witnesses(stcsp, RefOracle, name):
    m, o, r, a = _oracle(stcsp, RefOracle, name, None)
    for which, mask in masks_of(m, r).items():
        twin_against_yardstick(stcsp, RefOracle, name, mask)
    if name == "adversarial":  # -a: valid states cut off from the root are outside the live automaton
        for which, mask in masks_of(m, r).items():
            y = twin_against_yardstick(stcsp, RefOracle, name, mask, adversarial=5)[3]
            assert len(y.live) == PROBES["adversarial"]["adver1_live_states"]


def test_hand_derived_observers(stcsp, RefOracle):
    """COUNTER, only x: the four states offer x = 0 and x = 1 and move on: {S}, {c1}, {c2}, {c3}, the last one loops: 4 sets, 8 edges.
    The crafted model var x:[0,k]; var h:[0,k]; next h == h; x <= h, only x: the root picks h, which then stays. After x the
    system is in one of the states with h >= x, after more rows in those with h >= the largest row so far: the root and one set
    per value of that maximum, k + 2 sets; every set offers x = 0 .. k (some h = k state is in it): (k + 2)(k + 1) edges."""
    obs = twin_against_yardstick(stcsp, RefOracle, "counter", "only:x")[5]
    assert (obs["n_states"], obs["n_edges"], obs["max_set"]) == (4, 8, 1)
    for k in (1, 3, 6):
        SMALL[f"crafted{k}"] = R.CRAFTED % (k, k)
        obs = twin_against_yardstick(stcsp, RefOracle, f"crafted{k}", "only:x")[5]
        assert (obs["n_states"], obs["n_edges"], obs["max_set"], obs["levels"]) == (k + 2, (k + 2) * (k + 1), k + 1, 2)


@pytest.mark.parametrize("name", ["juggling_b4_f5", "digitinvader3", "partialorder_10", "countdown"])
def test_under_all_every_set_is_a_singleton(stcsp, RefOracle, name):
    m, r, a, y, mask, obs, _ = twin_against_yardstick(stcsp, RefOracle, name, "all")
    assert obs["max_set"] == 1 and obs["n_states"] == len(y.live) == a.n_live_states and obs["n_edges"] == a.n_live_edges
    assert a.from_observer(obs, "all").renumber().canonical() == a.renumber().canonical()


def walk(obs, stream, steps):
    """The observer state a stream reaches after `steps` rows."""
    nxt = {(s, tuple(r)): d for s, r, d in zip(obs["edge_src"].tolist(), obs["edge_values"].tolist(), obs["edge_dst"].tolist())}
    s = 0
    for row in np.asarray(stream).tolist()[:steps]:
        s = nxt[(s, tuple(row))]
    return s


@pytest.mark.parametrize("name,which", [("juggling_b4_f5", "only:B0"), ("digitinvader3", "only:D1"), ("partialorder_10", "only:succ"),
                                        ("duplicates", "only:x"), ("until", "hidden"), ("digitinvader1", "default")])
def test_language_preserved(stcsp, RefOracle, name, which):
    m, o, r, a = _oracle(stcsp, RefOracle, name, None)
    mask = masks_of(m, r)[which] if which == "hidden" else R.resolve_mask(m, which)
    m, r, a, y, mask, obs, _ = twin_against_yardstick(stcsp, RefOracle, name, mask)
    streams, kinds, _ = M.make_streams(y, m.var_bounds(), seed=7, n_walks=10, max_len=60)
    acc, nend, fin, _ = a.check_streams(streams, mask)
    q = a.from_observer(obs, mask)
    qacc, qnend, qfin, largest = q.check_streams(streams, mask)
    assert np.array_equal(qacc, acc) and np.array_equal(qfin, fin) and (qnend == 1).all() and largest == 1
    sizes = np.diff(obs["member_off"])
    assert [int(sizes[walk(obs, s, int(n))]) for s, n in zip(streams, acc)] == nend.tolist()
    assert "mutated" in kinds and (acc < [len(s) for s in streams]).any()  # some stream is rejected


def distinct_prefixes(y, length):
    """Brute force: the distinct projected streams of every length up to `length` over the paths from the root."""
    counts, paths = [1], {(0, ())}
    for _ in range(length):
        paths = {(d, word + (p,)) for s, word in paths for p, d in y.out.get(s, ())}
        counts.append(len({w for _, w in paths}))
    return counts


@pytest.mark.parametrize("name", ["counter", "countdown", "duplicates", "crafted3", "juggling_b4_f4", "digitinvader1"])
def test_paths_of_the_observer_are_the_distinct_streams(stcsp, RefOracle, name):
    m, o, r, a = _oracle(stcsp, RefOracle, name, None)
    hidden = 0
    for which, mask in masks_of(m, r).items():
        m, r, a, y, mask, obs, _ = twin_against_yardstick(stcsp, RefOracle, name, mask)
        expect = distinct_prefixes(y, 4)
        assert a.from_observer(obs, mask).count_streams(4).tolist() == expect, f"{name} [{which}]"
        hidden += a.count_streams(4).tolist() != expect
    assert hidden or name not in ("duplicates", "crafted3")  # there the paths outnumber the streams


@pytest.mark.parametrize("name,which", [("juggling_b4_f5", "only:B0"), ("digitinvader3", "only:D0"), ("partialorder_10", "only:succ"),
                                        ("crafted6", "only:x"), ("countdown", "only:x")])
def test_idempotent_and_foldable(stcsp, RefOracle, name, which):
    """The observer of the observer has the same states; folded by the bisimulation under the same mask it has the classes of the
    coarsest partition of the yardstick's observer (what --observer --quotient writes)."""
    SMALL.setdefault("crafted6", R.CRAFTED % (6, 6))
    m, r, a, y, mask, obs, (sets, final, edges, _) = twin_against_yardstick(stcsp, RefOracle, name, which)
    q = a.from_observer(obs, mask)
    again = q.observer(mask)
    assert (again["n_states"], again["n_edges"], again["max_set"]) == (obs["n_states"], obs["n_edges"], 1)
    assert np.array_equal(again["edge_values"], obs["edge_values"]) and np.array_equal(again["edge_src"], obs["edge_src"])
    pairs = {}
    for s, p, d in edges:
        pairs.setdefault(s, []).append((p, d))
    cls, _ = Q.coarsest_partition(range(len(sets)), final, pairs)
    hc, hn, _ = q.bisimulation(mask)
    assert hn == len(set(cls.values())) <= obs["n_states"]
    folded = q.quotient(hc, mask).renumber()
    assert folded.n_live_states == hn


@pytest.mark.parametrize("block", range(2))
def test_twin_matches_yardstick_on_fuzz_models(stcsp, RefOracle, block):
    grown = 0
    for seed in [s for s in range(60) if s % 2 == block]:
        text = random_model(seed)
        SMALL[f"fuzz{seed}"] = text
        m, o, r, a = _oracle(stcsp, RefOracle, f"fuzz{seed}", None)
        for which, mask in masks_of(m, r).items():
            obs = twin_against_yardstick(stcsp, RefOracle, f"fuzz{seed}", mask)[5]
            grown += obs["max_set"] > 1
    assert grown >= 1  # the generator produces automata that a mask makes nondeterministic


def test_output_formats_are_stable(stcsp, RefOracle, tmp_path):
    """The device-less road of `stcsp --observer`: the twin's observer through order_by_label / renumber / write_dot / write_binary
    is byte for byte the same from two builds, and survives the binary round trip."""
    from canon import canon
    m, r, a, y, mask, obs, _ = twin_against_yardstick(stcsp, RefOracle, "digitinvader3", "only:D1")
    files = []
    for i in range(2):
        q = a.from_observer(a.observer(mask), mask).order_by_label().renumber()
        q.write_dot(str(tmp_path / f"o{i}.dot"))
        q.write_binary(str(tmp_path / f"o{i}.bin"))
        files.append(((tmp_path / f"o{i}.dot").read_bytes(), (tmp_path / f"o{i}.bin").read_bytes()))
    assert files[0] == files[1]
    text, ns, ne = canon(str(tmp_path / "o0.dot"))
    assert text == q.canonical() and (ns, ne) == (obs["n_states"], obs["n_edges"])
    back = stcsp.Automaton.read_binary(str(tmp_path / "o0.bin"))
    assert back.canonical() == q.canonical()
    assert back.observer(mask)["n_states"] == obs["n_states"]  # the twin is the road for read_binary


def test_limits_and_refusals(stcsp, RefOracle):
    m, r, a, y, mask, obs, _ = twin_against_yardstick(stcsp, RefOracle, "juggling_b4_f5", "only:B0")
    assert a.observer(mask, max_states=obs["n_states"])["n_states"] == obs["n_states"]
    with pytest.raises(stcsp.StcspError) as ex:
        a.observer(mask, max_states=obs["n_states"] - 1)
    assert ex.value.code == -4
    other = a.observer("all")
    with pytest.raises(stcsp.StcspError) as ex:  # an observer under another mask does not fit
        a.from_observer(other, mask)
    assert ex.value.code == -1
    bad = dict(obs)
    bad["member"] = obs["member"].copy()
    bad["member"][-1] = r.n_states  # no such state
    with pytest.raises(stcsp.StcspError):
        a.from_observer(bad, mask)


def test_an_automaton_without_live_root_has_the_empty_observer(stcsp, RefOracle):
    SMALL["dead"] = NO_LIVE_ROOT
    m, r, a, y, mask, obs, _ = twin_against_yardstick(stcsp, RefOracle, "dead", "default")
    assert (obs["n_states"], obs["n_edges"], obs["levels"], obs["max_set"]) == (0, 0, 0, 0)
    assert a.from_observer(obs, mask).renumber().canonical().endswith("EMPTY\n")


def test_observer_abi(stcsp):
    """The new symbols are exported and the two new structs have the sizes of include/stcsp_engine.h (LP64)."""
    hip = C.CDLL(str(stcsp.CSRC / "libstcsp_hip.so"))
    assert hasattr(hip, "stcsp_engine_observer")
    host = stcsp.host_lib()
    for n in ("stcsp_automaton_observer", "stcsp_observer_get", "stcsp_observer_free", "stcsp_automaton_from_observer"):
        assert hasattr(host, n), n
    assert C.sizeof(stcsp.ObserverOptions) == 16  # int64, int32[2]
    assert C.sizeof(stcsp.ObserverResult) == 136  # 2 x int64, 6 pointers, 3 x int64, 2 x int32, 5 x double
    assert stcsp.ObserverResult.n_labels.offset == 64 and stcsp.ObserverResult.levels.offset == 92 and stcsp.ObserverResult.seconds.offset == 96
