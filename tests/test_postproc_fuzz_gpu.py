"""The device post-search graph passes (stcsp_engine_postprocess: k_trav_*, k_adv_*, k_adv2_* of dev_postproc.hpp)
against the plain yardstick tests/postproc_ref.py on the engine's own export: random models (tests/fuzz_models.py: Gen,
UntilGen, WideGen), the game family at cover-word boundaries up to kPostMaxWidth values, two long cascades, a model
without a solution, and the seeds where adversarial2 invalidates the root and leaves edge flags that no definition
determines. No oracle: the yardstick reads the same Result the device passes ran on, so state numbering is free.

Per model: the traverse, adversarial(i) for every variable, adversarial2(op, ava) for every ordered pair, and both on
one automaton for one seeded choice; flags under postproc_ref.same_flags(), adver1 / adver2 against the yardstick's
return values. The floors are those of tests/test_postproc.py; an MI355X run produced its figures for Gen and UntilGen
(every pair ran: no model reaches PAIR_WORK) and, for WideGen under the engine's node cap, 137 models, adversarial partial
9, adversarial2 partial 33, thinning 7. Kernels with a wrong last cover word, without the thinning of adversarial2 or
without the traverse's root rule fail these tests. Run on the GPU box: pytest -m gpu."""
import importlib

import pytest

import postproc_ref as ref
from fuzz_models import NO_SOLUTION, WIDE_SLOW_SEEDS, Gen, UntilGen, WideGen, adv_chain, game_model, until_chain

pytestmark = pytest.mark.gpu

_inst = importlib.import_module("stcsp-solver_amd").instances

WIDE_CAP = 20000  # max_search_nodes for the WideGen models, as in tests/test_postproc.py
PAIR_WORK = 1000000  # pairs x edges per model beyond which the pairs are thinned by a seeded choice
GAME_COUNTS = {0: (4, 4, 8), 1: (0, 0, 8)}  # valid states after adversarial(o), adversarial2(o, a), adversarial2(a, o)


def check_engine(stcsp, text, tally, choice, ctx, variables=None, **opts):
    """Every pass of the device on the engine's automaton of `text` against the yardstick (`variables`: the indices to
    take the passes over, default all). Returns the yardstick's flags by pass and the PostResult rounds by pass, or
    None when the engine refused the model as unsupported or stopped at its node cap."""
    m = stcsp.Model(text=text)
    try:
        e = stcsp.Engine(m, **opts)
    except stcsp.StcspError as ex:
        assert ex.code == -2, f"{ctx}: {ex}\n{text}"
        return None
    r = e.solve()
    if r.truncated:
        e.close()
        return None
    bounds = m.var_bounds()
    g = ref.graph(r)
    start = ref.traverse(g)
    seen = {"graph": g, "rounds": {}}

    def compare(adv=-1, adv2=None):
        want = ref.run(g, bounds, adv, adv2, start)
        post = e.postprocess(adversarial=adv, adversarial2=adv2)
        assert (post.n_states, post.n_edges) == (r.n_states, r.n_edges), ctx
        got = ref.post_flags(post)
        assert ref.same_flags(got, want, g.src, g.dst, bool(adv2)), \
            f"{ctx} adv={adv} adv2={adv2}: {ref.first_difference(got, want, g.src, g.dst, bool(adv2))}\n{text}"
        assert (post.adver1, post.adver2) == want.ret, f"{ctx} adv={adv} adv2={adv2}\n{text}"
        seen[(adv, adv2)] = want
        seen["rounds"][(adv, adv2)] = tuple(post.rounds)
        return want

    over = list(range(m.n_vars)) if variables is None else list(variables)
    pairs = [(op, ava) for op in over for ava in over]
    keep = max(4, PAIR_WORK // max(1, len(g.src)))
    if variables is None and len(pairs) > keep:  # a large export: a seeded choice of the pairs bounds the yardstick's time
        for k in range(keep):
            j = k + choice.below(len(pairs) - k)
            pairs[k], pairs[j] = pairs[j], pairs[k]
        pairs = pairs[:keep]
    t = compare()
    tally.traverse(g, t)
    for i in over:
        tally.adv(t, compare(adv=i))
    for p in pairs:
        tally.adv2(g, t, compare(adv2=p))
    compare(adv=over[choice.below(len(over))], adv2=(over[choice.below(len(over))], over[choice.below(len(over))]))  # -a -z
    e.close()
    return seen


BLOCKS = {"Gen": (Gen, 3, {}), "UntilGen": (UntilGen, 3, {}), "WideGen": (WideGen, 2, {"max_search_nodes": WIDE_CAP})}


@pytest.fixture(scope="module")
def block_tally(stcsp):
    """(generator name, block) -> the Tally of its fuzz over seeds [100 block, 100 block + 100) (WideGen: up to 150),
    run once."""
    done = {}

    def get(name, block):
        if (name, block) not in done:
            gen, _, opts = BLOCKS[name]
            tally = ref.Tally()
            for seed in range(block * 100, min((block + 1) * 100, 150 if name == "WideGen" else 300)):
                if name == "WideGen" and seed in WIDE_SLOW_SEEDS:
                    continue
                check_engine(stcsp, gen(seed).model(), tally, _inst.SplitMix64(0xAD5E0000 + seed), f"{name} seed {seed}", **opts)
            done[name, block] = tally
        return done[name, block]
    return get


@pytest.mark.parametrize("name,block", [(name, b) for name, (_, n, _) in BLOCKS.items() for b in range(n)])
def test_device_passes_match_yardstick_on_random_models(block_tally, name, block):
    assert block_tally(name, block).adv2_runs > 0


def test_device_fuzz_floors(block_tally):
    """The sums over the blocks above: the floors of tests/test_postproc.py."""
    total = {}
    for name, (_, n, _) in BLOCKS.items():
        total[name] = ref.Tally()
        for b in range(n):
            total[name] += block_tally(name, b)
        print(name, total[name])
    t = total["Gen"]
    assert t.adv_partial >= 50 and t.adv2_partial >= 280 and t.adv2_thinning >= 45, t
    t = total["UntilGen"]
    assert t.traverse_partial >= 8 and t.adv_partial >= 45 and t.adv2_partial >= 230 and t.adv2_thinning >= 40, t
    t = total["WideGen"]
    assert t.models >= 100 and t.adv_partial >= 5 and t.adv2_partial >= 20 and t.adv2_thinning >= 4, t


def game(stcsp, W, alo, shift=0, **opts):
    # at 4096 values the passes run over o, a and s only: the yardstick is plain Python over 3 W edges per state
    seen = check_engine(stcsp, game_model(W, alo, shift), ref.Tally(), _inst.SplitMix64(W), f"game W={W} alo={alo} shift={shift}",
                        variables=(0, 1, 2) if W >= 4096 else None, **opts)
    assert seen is not None
    assert len(seen[-1, None].valid) == 8 and seen[-1, None].valid.count(1) == 8
    assert (seen[0, None].valid.count(1), seen[-1, (0, 1)].valid.count(1), seen[-1, (1, 0)].valid.count(1)) == GAME_COUNTS[alo]
    return seen


@pytest.mark.parametrize("alo", [0, 1])
@pytest.mark.parametrize("W", [31, 32, 33, 63, 64, 65, 96, 127, 128])
def test_device_passes_game_family_bitset(stcsp, W, alo):
    """One, two, three and four cover words per state, full and partial last words."""
    seen = game(stcsp, W, alo)
    if alo == 0:  # edges between kept states are thinned
        t, f, g = seen[-1, None], seen[-1, (0, 1)], seen["graph"]
        assert sum(t.alive[e] and not f.alive[e] and f.valid[g.src[e]] and f.valid[g.dst[e]] for e in range(len(g.src))) > 1


@pytest.mark.parametrize("alo", [0, 1])
@pytest.mark.parametrize("W", [129, 1024, 4096])
def test_device_passes_game_family_interval(stcsp, W, alo):
    """Interval domains: up to kPostMaxWidth = 4096 values, i.e. 128 cover words per state and 4096 avatar classes."""
    game(stcsp, W, alo, flags=stcsp.F_INTERVAL_DOMAINS, time_limit_s=30.0)  # (a solve that ran out of time fails the test)


@pytest.mark.parametrize("alo", [0, 1])
@pytest.mark.parametrize("W", [33, 129])
def test_device_passes_game_family_shifted(stcsp, W, alo):
    """o's domain starts at -5: the cover bit of a value is value - lb."""
    game(stcsp, W, alo, shift=-5, flags=stcsp.F_INTERVAL_DOMAINS if W > 128 else 0)


def test_device_adversarial_long_cascade(stcsp):
    """The cover of a sweep is computed from the flags of the sweep before, so a sweep takes one level off the chain:
    at least 120 rounds, and the call succeeds, i.e. the sweeps stay within the driver's bound of S + 8 rounds."""
    seen = check_engine(stcsp, adv_chain(120), ref.Tally(), _inst.SplitMix64(1), "adv_chain(120)")
    assert seen[-1, None].valid.count(1) >= 121 and seen[0, None].valid.count(1) == 0 and seen[0, None].ret == (0, -1)
    assert seen["rounds"][0, None][1] >= 120


def test_device_traverse_long_cascade(stcsp):
    seen = check_engine(stcsp, until_chain(120), ref.Tally(), _inst.SplitMix64(2), "until_chain(120)")
    assert seen[-1, None].final.count(1) < seen[-1, None].valid.count(1) and seen[-1, None].valid.count(1) >= 121


def test_device_passes_without_a_solution(stcsp):
    """No edge at all: every pass runs its state kernels only."""
    seen = check_engine(stcsp, NO_SOLUTION, ref.Tally(), _inst.SplitMix64(3), "no solution")
    assert len(seen["graph"].src) == 0
    assert all(f.alive == b"" for k, f in seen.items() if k not in ("graph", "rounds"))


@pytest.mark.parametrize("gen,seed,pairs", [(Gen, 97, [(0, 2), (0, 3)]), (UntilGen, 97, [(0, 2), (0, 3)]), (UntilGen, 286, [(3, 5)])])
def test_device_adversarial2_invalidated_root(stcsp, gen, seed, pairs):
    """adversarial2 invalidates the root here, the clean-up is skipped, and whether an edge from a kept state into an
    invalidated one was thinned depends on the visiting order: same_flags() leaves exactly those edges out. The root
    must be invalid, or the relation was widened somewhere else."""
    seen = check_engine(stcsp, gen(seed).model(), ref.Tally(), _inst.SplitMix64(seed), f"{gen.__name__} seed {seed}")
    for p in pairs:
        assert seen[-1, p].valid[0] == 0 and seen[-1, p].ret == (-1, 0)
        assert seen[-1, p].valid.count(1) > 0
