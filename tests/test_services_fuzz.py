"""The automaton services on table-driven random automata, host side: the existing checks of generate, repair, infer, compare,
components, optimise, monitor, quotient and observer -- each host twin against its own plain Python yardstick on the automaton of
the CPU oracle -- over a fixed list of fuzz_models.table_automaton models: joins, cycles through several components, dead ends
the traverse removes, non-final states beside final ones and real nondeterminism under a mask, at live state counts on both
sides of 64, 256 and 1024. This file is where the shapes are sized: test_the_shapes_keep_their_floors prints one line per
automaton (pytest -s) and asserts the floors that keep the fuzz from degenerating. The same list on the device:
tests/test_services_fuzz_gpu.py."""
import functools

import pytest

import compare_ref as CMP
import components_ref as CR
import monitor_ref as M
import observer_ref as OR
import test_compare as TCmp
import test_components as TC
import test_generate as TG
import test_infer as TI
import test_monitor as TM
import test_observer as TOb
import test_optimise as TO
import test_quotient as TQ
import test_repair as TR
from fuzz_models import table_by_name, table_mutant

# table:<seed>:<digits>:<letters>:<keep %>:<goal %>[:unrooted][:<colours>]. The seeds were chosen on the CPU oracle alone so that the
# floors below hold; the comment is the live state count and what the automaton is in the list for.
TABLES = [
    "table:1:8:3:70:20",                 # 9: small enough for the brute force of compare
    "table:1:20:3:60:10",                # 16: the same
    "table:1:20:3:60:0",                 # 0: no goal, `w until g` never ends: no live root
    "table:3:30:2:70:20:unrooted",       # 13: one variable, nine edges out of the root
    "table:9:50:3:60:10",                # 58: below 64, one variable of 50 values (W = 2); 2,714 observer states under the colour
    "table:17:60:3:60:10",               # 65: above 64, one variable of 60 values (W = 2)
    "table:4:8x9:3:65:10",               # 64: a full wavefront, two digits
    "table:1:8x9:3:65:10",               # 66: above 64, two digits
    "table:1:100:2:80:5:3",              # 122: one variable of 100 values (W = 4)
    "table:1:128:2:80:5:3",              # 147: one variable of 128 values (W = 4, the last bit of the last word)
    "table:2:200:2:80:5:3",              # 251: below 256, one variable of 200 values (interval domains)
    "table:37:16x16:3:60:10:3",          # 262: above 256
    "table:1:12x12:3:60:10:unrooted:4",  # 190: 24 edges out of the root
    "table:2:24x25:3:55:8:4",            # 690
    "table:38:32x32:2:78:4:4",           # 1021: below 1024
    "table:28:32x32:2:79:5:4",           # 1029: above 1024, more live states than the table has entries (the until flag doubles some)
]
MUTANT_SEED = 5
MASKS = ("default", "all", "hidden", "colour")
SERVICES = ("generate", "repair", "infer", "components", "optimise", "monitor", "quotient", "observer")
OBSERVABLES = ("x", "c", "digits")  # what compare observes: the letter, the colour, the state


def mutant(name):
    return "mutant:" + name


TEXT = {name: table_by_name(name) for name in TABLES}
TEXT.update({mutant(name): table_mutant(TEXT[name], MUTANT_SEED) for name in TABLES})
# the lookup: the helpers of the other files that take a name find the text under it
for texts in (TC.CRAFTED, TCmp.TEXTS, TOb.SMALL):
    texts.update(TEXT)


@pytest.fixture(autouse=True)
def colour_among_the_masks(monkeypatch):
    """Every check that walks monitor_ref.masks() meets the colour-only mask as well."""
    plain = M.masks
    monkeypatch.setattr(M, "masks", lambda model, r: {**plain(model, r), "colour": OR.only(model, "c")})


def digits_of(name):
    return "s1,s0" if "x" in name.split(":")[2] else "s"


def shape_of(r, valid, final, alive, observer):
    """The figures of one automaton (a Result with its flags, and its observer dict under the colour mask)."""
    ref = CR.yardstick(r, valid, final, alive)
    live = sorted(ref["num"])
    return dict(live=len(live), edges=ref["counts"]["n_edges"], components=ref["counts"]["n_components"], largest=ref["counts"]["largest"],
                cyclic=max([len(ms) for c, ms in ref["members"].items() if ref["flags"][c] & CR.CYCLIC], default=0),
                final=sum(1 for s in live if final[s]), nonfinal=sum(1 for s in live if not final[s]), removed=r.n_states - len(live),
                root_edges=len(ref["out"].get(0, ())) if live else 0, obs_states=observer["n_states"], obs_largest=observer["max_set"])


def shape_line(name, s):
    return (f"{name}: live {s['live']} edges {s['edges']} components {s['components']} largest {s['largest']} (cyclic {s['cyclic']}) "
            f"non-final {s['nonfinal']} removed {s['removed']} root edges {s['root_edges']} observer {s['obs_states']} largest set {s['obs_largest']}")


def check_floors(shapes):
    """shapes: {name: shape_of()} over TABLES."""
    assert list(shapes) == TABLES
    all_shapes = list(shapes.values())
    third = -(-len(all_shapes) // 3)
    for boundary in (64, 256, 1024):
        assert any(boundary - 8 <= s["live"] < boundary for s in all_shapes), f"no automaton within 8 states below {boundary}"
        assert any(boundary < s["live"] <= boundary + 8 for s in all_shapes), f"no automaton within 8 states above {boundary}"
    assert sum(s["cyclic"] >= 16 and s["components"] >= 3 for s in all_shapes) >= third
    assert sum(s["final"] > 0 and s["nonfinal"] > 0 and s["removed"] >= 1 for s in all_shapes) >= third
    assert sum(s["obs_largest"] >= 3 for s in all_shapes) >= third
    assert any(s["obs_states"] > s["live"] for s in all_shapes)
    assert any("unrooted" in name and s["root_edges"] >= 8 for name, s in shapes.items())
    assert any(s["live"] == 0 for s in all_shapes)


@functools.lru_cache(maxsize=None)
def oracle_shape(stcsp, RefOracle, name):
    m, r, a, (valid, final, alive), ref, _ = TC.oracle_case(stcsp, RefOracle, name)
    return shape_of(r, valid, final, alive, a.observer(OR.only(m, "c")))


def test_the_shapes_keep_their_floors(stcsp, RefOracle):
    shapes = {name: oracle_shape(stcsp, RefOracle, name) for name in TABLES}
    for name, s in shapes.items():
        print(shape_line(name, s))
    check_floors(shapes)


def test_the_generator_reads_nothing_and_repeats_itself():
    assert all(table_by_name(name) == text for name, text in TEXT.items() if not name.startswith("mutant:"))
    for name in TABLES:
        extra = TEXT[mutant(name)][len(TEXT[name]):]
        assert TEXT[mutant(name)].startswith(TEXT[name]) and extra.count("\n") == 1 and " ne " in extra


def check_service(stcsp, RefOracle, service, name):
    """One existing host check on one table automaton. The plain Python recurrences grow with edges x length: the stream counts
    and lengths are capped here as those checks cap them on the shipped instances."""
    text = TEXT[name]
    large = oracle_shape(stcsp, RefOracle, name)["edges"] > 500
    if service == "generate":
        TG.check_sampling(stcsp, RefOracle, text, name, horizon=24, n=12, lengths=(24, 1, 8), mask_names=MASKS)
    elif service == "repair":
        TR.check_twin(stcsp, RefOracle, text, name, mask_names=MASKS, most=12 if large else 100)
    elif service == "infer":
        TI.check_twin(stcsp, RefOracle, text, name, mask_names=MASKS, n=2 if large else 5, most=6 if large else None)
    elif service == "components":
        TC.check_host_twin(stcsp, RefOracle, name)
    elif service == "optimise":
        TO.check_host_twin(stcsp, RefOracle, name)
    elif service == "monitor":
        TM.check_host_twin(stcsp, RefOracle, stcsp.Model(text=text), name, n_walks=8, max_len=60)
    elif service == "quotient":
        TQ.check_host_twin(stcsp, RefOracle, stcsp.Model(text=text), name)
    else:
        for which in ("default", "all", "only:c"):
            TOb.twin_against_yardstick(stcsp, RefOracle, name, which)
        m, o, r, a = TOb._oracle(stcsp, RefOracle, name, None)
        TOb.twin_against_yardstick(stcsp, RefOracle, name, M.hidden_signature_mask(m, r))


@pytest.mark.parametrize("name", TABLES)
@pytest.mark.parametrize("service", SERVICES)
def test_host_twin_against_yardstick(stcsp, RefOracle, service, name):
    check_service(stcsp, RefOracle, service, name)


@pytest.mark.parametrize("name", TABLES)
@pytest.mark.parametrize("which", OBSERVABLES)
def test_compare_with_the_mutant(stcsp, RefOracle, which, name):
    """Automaton against mutant: twin == product yardstick, the swapped operands, the prefix witnesses against the monitor, and on
    the automata of at most 20 live states the witnesses against the enumerated languages. The mutant only forbids: no stream is
    a prefix of it alone."""
    names = digits_of(name) if which == "digits" else which
    sl, sr, twin = TCmp.twin_against_yardstick(stcsp, RefOracle, name, mutant(name), names)
    assert CMP.same(stcsp.compare_observers(sr[2], sl[2]), CMP.swapped(twin))
    TCmp.check_prefix_witnesses(stcsp, (sl, sr), twin)
    assert twin["witness_len"][1] == -1
    print(f"{name} | mutant [{names}]: observers {sl[2]['n_states']} | {sr[2]['n_states']} pairs {twin['n_pairs']} witness lengths {twin['witness_len'].tolist()}")
    if oracle_shape(stcsp, RefOracle, name)["live"] <= 20:
        CMP.check_by_brute_force(sl[2], sr[2], twin, max(7, int(twin["witness_len"].max()) + 1))
