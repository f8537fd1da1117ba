"""Bisimulation quotient, host side (include/stcsp_host.h: stcsp_automaton_bisimulation / stcsp_automaton_quotient): the CPU
twin of the device pass against an independent yardstick -- the plain Python partition refinement of tests/quotient_ref.py,
run on the automaton of the CPU oracle. The device pass itself: tests/test_quotient_gpu.py."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import quotient_ref as Q
from fuzz_models import random_model

PROBES = json.loads((Path(__file__).resolve().parent / "golden" / "reference_probes.json").read_text())
SMALLEST_GOLDENS = ["juggling_b4_f4", "juggling_b5_f5", "juggling_b6_f6", "juggling_b4_f4_nosym", "digitinvader1", "juggling_b4_f5"]
FUZZ_SEEDS = range(220)

# A free x beside a hidden counter c that runs 0, 1, 2, 3, 3, 3, ...  (`next c` adds the look-ahead variable _V0).
COUNTER = "var x:[0,1]; var c:[0,3]; first c == 0; next c == if (c lt 3) then (c + 1) else 3;"
# ... where x must be 1 once the counter has reached 3.
COUNTDOWN = COUNTER + " (c eq 3) -> (x eq 1);"
# ... with a second hidden variable h that is free while c < 3 and 0 afterwards.
DUPLICATES = COUNTER + " var h:[0,1]; (c eq 3) -> (h eq 0);"


def masks(model):
    return {"default": Q.default_mask(model.var_names), "all": [1] * model.n_vars}


def oracle_automaton(stcsp, RefOracle, model, adversarial=None):
    o = RefOracle(model)
    r = o.solve()
    a = o.automaton(r).traverse()
    if adversarial is not None:
        a.adversarial(adversarial)
    return o, r, a


def check_host_twin(stcsp, RefOracle, model, what):
    """Host twin == yardstick as partitions of the canonical state numbers, for the default mask and for `all`; the
    quotient automaton has the yardstick's state and edge counts. Returns {mask name: (live, classes)}."""
    o, r, a = oracle_automaton(stcsp, RefOracle, model)
    valid, final, alive = a.flags()
    res = {}
    for name, mask in masks(model).items():
        part, n_classes, out, num, cls = Q.yardstick(model, r, valid, final, alive, mask)
        hc, hn, rounds = a.bisimulation(None if name == "default" else "all")
        assert hn == n_classes, f"{what} [{name}]"
        assert Q.engine_partition(r, valid, alive, hc) == part, f"{what} [{name}]"
        assert 1 <= rounds <= len(num) + 1
        # classes are numbered by their least member
        firsts = [int(np.flatnonzero(hc == c)[0]) for c in range(hn)]
        assert firsts == sorted(firsts), f"{what} [{name}]"
        q = a.quotient(hc, mask).renumber()
        assert (q.n_live_states, q.n_live_edges) == Q.quotient_counts(out, num, cls, mask), f"{what} [{name}]"
        res[name] = (len(num), n_classes)
    return res


@pytest.mark.parametrize("name", SMALLEST_GOLDENS)
def test_host_twin_matches_yardstick_on_goldens(stcsp, RefOracle, name):
    check_host_twin(stcsp, RefOracle, stcsp.Model.from_name(name), name)


@pytest.mark.parametrize("probe", ["until", "arr", "at", "misc", "adversarial"])
def test_host_twin_matches_yardstick_on_probes(stcsp, RefOracle, probe):
    check_host_twin(stcsp, RefOracle, stcsp.Model(text=PROBES[probe]["text"]), probe)


@pytest.mark.parametrize("block", range(4))
def test_host_twin_matches_yardstick_on_fuzz_models(stcsp, RefOracle, block):
    folded = 0
    seeds = [s for s in FUZZ_SEEDS if s % 4 == block]
    for seed in seeds:
        text = random_model(seed)
        res = check_host_twin(stcsp, RefOracle, stcsp.Model(text=text), f"seed {seed}\n{text}")
        folded += res["default"][1] < res["default"][0]
    assert folded >= 1  # the generator produces automata with something to fold


def test_host_twin_after_adversarial_pass(stcsp, RefOracle):
    """After adversarialTraverse valid states can be cut off from the root: they are outside the live automaton."""
    m = stcsp.Model(text=PROBES["adversarial"]["text"])
    o, r, a = oracle_automaton(stcsp, RefOracle, m, adversarial=5)
    valid, final, alive = a.flags()
    for name, mask in masks(m).items():
        part, n_classes, out, num, cls = Q.yardstick(m, r, valid, final, alive, mask)
        hc, hn, _ = a.bisimulation(mask)
        assert hn == n_classes and Q.engine_partition(r, valid, alive, hc) == part
        assert len(num) == PROBES["adversarial"]["adver1_live_states"]


def test_hand_derived_counts(stcsp, RefOracle):
    """COUNTER: the live automaton has four states -- the root S, then the states whose signature says that c will be 1,
    2 and 3; the last one loops. Every state offers x = 0 and x = 1, so eight edges, and every state is final (no until).

    Only x observable: every state accepts every word over x, so ONE class with two edges (x = 0, x = 1, both loops).
    Every variable observable (and also the default mask, which hides only _V0): the label of S's edges carries c = 0, and
    those of the other three c = 1, 2, 3: no two states offer the same labels, nothing folds: four classes, eight edges.

    COUNTDOWN, only x observable: the looping state offers x = 1 only, the others x = 0 and x = 1; a state's language is
    fixed by its distance to the loop (3, 2, 1, 0 steps): four classes again, but they need one round per step to separate.

    DUPLICATES, only x observable: before c reaches 3 every state has four edges (x, h free) that project on two labels,
    the looping state has two. As SETS of (label, class) they agree: one class, two edges. A sum over the edges that
    counted the duplicated pairs twice would split it."""
    expect = {
        (COUNTER, "x"): (4, 1, 2), (COUNTER, "default"): (4, 4, 8), (COUNTER, "all"): (4, 4, 8),
        (COUNTDOWN, "x"): (4, 4, 7), (DUPLICATES, "x"): (4, 1, 2), (DUPLICATES, "all"): (4, 4, 14),
    }
    for (text, which), (live, classes, edges) in expect.items():
        m = stcsp.Model(text=text)
        mask = {"x": [int(n == "x") for n in m.var_names], "default": Q.default_mask(m.var_names), "all": [1] * m.n_vars}[which]
        o, r, a = oracle_automaton(stcsp, RefOracle, m)
        valid, final, alive = a.flags()
        part, n_classes, out, num, cls = Q.yardstick(m, r, valid, final, alive, mask)
        assert (len(num), n_classes) + Q.quotient_counts(out, num, cls, mask)[1:] == (live, classes, edges), (text, which)
        hc, hn, rounds = a.bisimulation(mask)
        assert (int((hc >= 0).sum()), hn) == (live, classes), (text, which)
        q = a.quotient(hc, mask).renumber()
        assert (q.n_live_states, q.n_live_edges) == (classes, edges), (text, which)
        if text == COUNTDOWN:
            assert rounds >= 4


def test_a_shipped_family_folds(stcsp, RefOracle):
    """Default mask, shipped instances: the symmetry-broken juggling instances and digitinvader fold a state (the root has
    a twin inside the cycle it enters); the _nosym juggling instances do not fold at all -- every state of theirs is told
    apart by the labels of its own out-edges, which carry the signature values."""
    res = {n: check_host_twin(stcsp, RefOracle, stcsp.Model.from_name(n), n)["default"]
           for n in ["juggling_b4_f4", "juggling_b5_f5", "digitinvader1", "juggling_b4_f4_nosym"]}
    assert res["juggling_b4_f4"] == (5, 4) and res["juggling_b5_f5"] == (6, 5)
    assert res["digitinvader1"][1] < res["digitinvader1"][0]
    assert res["juggling_b4_f4_nosym"] == (25, 25)


@pytest.mark.parametrize("name", ["juggling_b4_f5", "digitinvader2", "partialorder_10"])
def test_identity_partition_gives_the_same_automaton(stcsp, RefOracle, name):
    m = stcsp.Model.from_name(name)
    o, r, a = oracle_automaton(stcsp, RefOracle, m)
    hc, _, _ = a.bisimulation("all")
    live = hc >= 0
    identity = np.where(live, np.cumsum(live) - 1, -1).astype(np.int32)  # every live state its own class
    q = a.quotient(identity, "all").renumber()
    assert q.canonical() == a.renumber().canonical()


def test_quotient_of_a_partition_without_root_is_empty_and_bad_partitions_are_refused(stcsp, RefOracle):
    m = stcsp.Model(text=COUNTER)
    o, r, a = oracle_automaton(stcsp, RefOracle, m)
    none = np.full(r.n_states, -1, dtype=np.int32)
    assert a.quotient(none).renumber().canonical().endswith("EMPTY\n")
    bad = np.zeros(r.n_states, dtype=np.int32)
    bad[-1] = 2  # class 1 has no member
    with pytest.raises(stcsp.StcspError):
        a.quotient(bad)


def test_quotient_survives_the_output_formats(stcsp, RefOracle, tmp_path):
    """write_dot / write_binary / order_by_label / renumber work on a quotient unchanged."""
    from canon import canon
    m = stcsp.Model.from_name("digitinvader2")
    o, r, a = oracle_automaton(stcsp, RefOracle, m)
    hc, hn, _ = a.bisimulation()
    q = a.quotient(hc).order_by_label().renumber()
    q.write_dot(str(tmp_path / "q.dot"))
    q.write_binary(str(tmp_path / "q.bin"))
    text, ns, ne = canon(str(tmp_path / "q.dot"))
    assert text == q.canonical() and ns == hn
    assert stcsp.Automaton.read_binary(str(tmp_path / "q.bin")).canonical() == q.canonical()


def test_quotient_abi(stcsp):
    """The new symbols are exported and the two new structs have the sizes of include/stcsp_engine.h (LP64)."""
    hip = C.CDLL(str(stcsp.CSRC / "libstcsp_hip.so"))
    assert hasattr(hip, "stcsp_engine_quotient")
    host = stcsp.host_lib()
    for n in ("stcsp_automaton_bisimulation", "stcsp_automaton_quotient", "stcsp_automaton_set_observable"):
        assert hasattr(host, n), n
    assert C.sizeof(stcsp.QuotientOptions) == 16    # pointer + int32[2]
    assert C.sizeof(stcsp.QuotientResult) == 48     # 3 x int64, pointer, int32 (+ 4 padding), double
    assert stcsp.QuotientResult.seconds.offset == 40 and stcsp.QuotientResult.rounds.offset == 32
