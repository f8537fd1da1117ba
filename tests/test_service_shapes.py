"""The automaton services on the export shapes of every kernel family, host side: the existing checks of generate, repair,
infer, components, optimise, monitor, quotient, observer and compare -- each host twin against its own plain Python yardstick on
the automaton of the CPU oracle -- over the catalogue of tests/service_shapes.py: keys of up to 126 words, up to 63 until
flags, up to 263 variables per label, K = 1, 2 and 3, interval domains under long keys. Beside the default mask, `all` and
the hidden-signature mask, every shape runs under three masks that reach the high indices (the last variable alone, every
variable from index 64 on, the behaviour variables with the last padding variable). test_the_shapes_keep_their_floors prints
one line per shape (pytest -s) and asserts the floors. The same list on the device: tests/test_service_shapes_gpu.py."""
import functools

import pytest

import compare_ref as CMP
import components_ref as CR
import monitor_ref as M
import service_shapes as S
import test_compare as TCmp
import test_components as TC
import test_generate as TG
import test_infer as TI
import test_monitor as TM
import test_observer as TOb
import test_optimise as TO
import test_quotient as TQ
import test_repair as TR

SERVICES = ("generate", "repair", "infer", "monitor", "observer")    # the services that take a mask: one case per group of masks
UNMASKED = ("components", "optimise", "quotient")                   # (the quotient's check takes the default mask and `all`)

# the lookup: the helpers of the other files that take a name find the text under it
for texts in (TC.CRAFTED, TCmp.TEXTS, TOb.SMALL):
    texts.update(S.TEXT)


@pytest.fixture
def masks(monkeypatch):
    """monitor_ref.masks() gives the masks of one shape: those of one group, or all six."""
    plain = M.masks

    def use(name, names=S.MASKS):
        monkeypatch.setattr(M, "masks", S.masks_for(plain, S.BY_NAME[name], names))
    return use


@functools.lru_cache(maxsize=None)
def oracle_figures(stcsp, RefOracle, name):
    s = S.BY_NAME[name]
    m, r, a, (valid, final, alive), ref, _ = TC.oracle_case(stcsp, RefOracle, S.key_of(name), None, s.prefix_k)
    return S.figures(m, r, valid, final, alive, CR)


def test_the_shapes_keep_their_floors(stcsp, RefOracle):
    figs = {name: oracle_figures(stcsp, RefOracle, name) for name in S.NAMES}
    for name, f in figs.items():
        print(S.line(name, f))
    S.check_floors(figs)


def test_the_catalogue_names_its_rows_and_its_masks(stcsp):
    for s in S.SHAPES:
        m = stcsp.Model(text=S.TEXT[S.key_of(s.name)], prefix_k=s.prefix_k)
        extra = S.extra_masks(s, m.var_names)
        n = m.n_vars
        assert sum(extra["last"]) == 1 and extra["last"][n - 1] == 1
        assert sum(extra["high"]) == n - S.high_from(n) > 0 and (n <= 64 or not any(extra["high"][:64]))
        assert 2 <= sum(extra["behaviour"]) <= 3 and (s.pad is None or extra["behaviour"][m.var_names.index(s.pad)])
        if s.pad:  # the last padding variable: none of that family comes after it
            assert not any(v.startswith(s.pad.rstrip("0123456789")) for v in m.var_names[m.var_names.index(s.pad) + 1:])
        assert S.TEXT[S.mutant_key(s.name)].startswith(S.TEXT[S.key_of(s.name)]) and s.mutant.count(";") == 1
        assert (s.row is None) == (s.regs is not None)


def check_service(stcsp, RefOracle, service, name, mask_names):
    """One existing host check on one shape under some of the masks (monitor_ref.masks() is already narrowed to them). The plain
    Python recurrences grow with edges x length: stream counts and lengths are capped as tests/test_services_fuzz.py caps them."""
    s = S.BY_NAME[name]
    key, k = S.key_of(name), s.prefix_k
    text = S.TEXT[key]
    large, huge = S.large(oracle_figures(stcsp, RefOracle, name)), S.huge(oracle_figures(stcsp, RefOracle, name))
    if service == "generate":
        TG.check_sampling(stcsp, RefOracle, text, name, horizon=24, n=12, lengths=(24, 1, 8), mask_names=mask_names, prefix_k=k)
    elif service == "repair":
        TR.check_twin(stcsp, RefOracle, text, name, mask_names=mask_names, most=6 if huge else 12 if large else 100, prefix_k=k)
    elif service == "infer":
        TI.check_twin(stcsp, RefOracle, text, name, mask_names=mask_names, n=2 if large else 5, most=6 if large else None, prefix_k=k)
    elif service == "components":
        TC.check_host_twin(stcsp, RefOracle, key, prefix_k=k)
    elif service == "optimise":
        TO.check_host_twin(stcsp, RefOracle, key, prefix_k=k)
    elif service == "monitor":
        TM.check_host_twin(stcsp, RefOracle, stcsp.Model(text=text, prefix_k=k), name, n_walks=8, max_len=60)
    elif service == "quotient":
        TQ.check_host_twin(stcsp, RefOracle, stcsp.Model(text=text, prefix_k=k), name)
    else:
        m, o, r, a = TOb._oracle(stcsp, RefOracle, key, None, k)
        for which, mask in M.masks(m, r).items():
            TOb.twin_against_yardstick(stcsp, RefOracle, key, which if which in ("default", "all") else mask, prefix_k=k)


@pytest.mark.parametrize("name", S.NAMES)
@pytest.mark.parametrize("group", list(S.MASK_GROUPS))
@pytest.mark.parametrize("service", SERVICES)
def test_host_twin_against_yardstick(stcsp, RefOracle, masks, service, group, name):
    masks(name, S.MASK_GROUPS[group])
    check_service(stcsp, RefOracle, service, name, S.MASK_GROUPS[group])


@pytest.mark.parametrize("name", S.NAMES)
@pytest.mark.parametrize("service", UNMASKED)
def test_host_twin_against_yardstick_on_whole_rows(stcsp, RefOracle, service, name):
    check_service(stcsp, RefOracle, service, name, ())


def compare_names(name, which):
    """What compare observes: the behaviour variables with the last padding variable, or every variable."""
    s = S.BY_NAME[name]
    if which == "behaviour":
        return S.behaviour_names(s)
    return ",".join(stcsp_names(name))


@functools.lru_cache(maxsize=None)
def stcsp_names(name):
    s = S.BY_NAME[name]
    return tuple(S.st.Model(text=S.TEXT[S.key_of(name)], prefix_k=s.prefix_k).var_names)


@pytest.mark.parametrize("name", S.NAMES)
@pytest.mark.parametrize("which", ["behaviour", "all"])
def test_compare_with_the_mutant(stcsp, RefOracle, which, name):
    """Shape against mutant: twin == product yardstick, the swapped operands, the prefix witnesses against the monitor. The mutant
    only forbids: no stream is a prefix of it alone, and some stream of the shape is none of the mutant's."""
    k = S.BY_NAME[name].prefix_k
    names = compare_names(name, which)
    sl, sr, twin = TCmp.twin_against_yardstick(stcsp, RefOracle, S.key_of(name), S.mutant_key(name), names, k)
    assert CMP.same(stcsp.compare_observers(sr[2], sl[2]), CMP.swapped(twin))
    TCmp.check_prefix_witnesses(stcsp, (sl, sr), twin)
    assert twin["witness_len"][1] == -1 and twin["witness_len"][0] >= 0
    print(f"{name} | mutant [{which}]: observers {sl[2]['n_states']} | {sr[2]['n_states']} pairs {twin['n_pairs']} witness lengths {twin['witness_len'].tolist()}")
