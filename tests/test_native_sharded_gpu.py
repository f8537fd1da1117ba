"""stcsp_engine_solve_sharded (include/stcsp_sharded.h): the superstep loop inside the engine library, no Python and no
torch between two bursts of k_expand.  The in-process transport (ranks = host threads, records by hipMemcpyAsync) runs
2, 3 and 4 shards on one GPU; the RCCL transport (libstcsp_rccl.so) runs with a communicator of size 1 -- all one GPU
allows.  Same checks as the torch-driven loop: the reference's canonical automaton and `dom`, node conservation, what is
donated is adopted, and a failing rank ends every rank.

Below them the record shapes the scalar frontier model cannot take (wide and interval domains, more than 32 until constraints,
big scopes): redistribution between engines that really moves nodes, and the donate / adopt round-trip law with a plain Python
decoder of the transfer record (tests/xfer_ref.py)."""
import importlib
from collections import namedtuple

import pytest

from conftest import finish
from node_seam import DeviceWords, one_expansion_per_round  # (they moved to the node-level seam, which shares them)

pytestmark = pytest.mark.gpu

SHARE = dict(budget_rounds=1, share_per_rank=2)


def run_local(stcsp, model, world, knobs=None, flags=0, **opts):
    engines = [stcsp.Engine(model, rank=r, world=world, flags=flags | (stcsp.F_STEPPED if world == 1 else 0), **opts) for r in range(world)]
    g = stcsp.LocalGroup(world)
    stats = g.solve(engines, **(knobs or {}))
    results = [e.export() for e in engines]
    h, merged = stcsp.merge_shards(results)
    a = stcsp.Automaton(model, merged).traverse().renumber()
    nodes = [e.counters().search_nodes for e in engines]
    return a, merged, stats, nodes, engines, g


@pytest.mark.parametrize("world,name", [(2, "juggling_b4_f5"), (3, "digitinvader3"), (2, "partialorder_10"), (4, "partialorder_12"),
                                        (2, "juggling_b4_f4_nosym")])
def test_native_sharded_matches_golden(stcsp, golden, world, name):
    m = stcsp.Model.from_name(name)
    a, merged, stats, nodes, engines, g = run_local(stcsp, m, world)
    gold = golden[name]
    assert (a.n_live_states, a.n_live_edges, a.canonical_sha256()) == (gold["states"], gold["edges"], gold["canonical_sha256"])
    assert merged.counters.dominance == gold["dom"]
    if gold["fail"] == 0:
        assert sum(nodes) == gold["search"]
    assert sum(s["nodes_donated"] for s in stats) == sum(s["nodes_adopted"] for s in stats)
    assert sum(s["candidates_sent"] for s in stats) == sum(s["candidates_received"] for s in stats) > 0


@pytest.mark.parametrize("world", [2, 3])
def test_native_sharded_redistribution_no_leaf(stcsp, FrontierModel, world):
    """A refutation-only member of the synthetic family (no leaf is ever reached: without redistribution every shard but
    the root's would stay idle): every shard searches, the sum is the unsharded tree."""
    inst = stcsp.instances
    m = stcsp.Model(text=inst.synthetic(24, 8, 125, 4, 7))
    f = FrontierModel(m)
    r1 = f.solve()
    a, merged, stats, nodes, engines, g = run_local(stcsp, m, world, knobs=SHARE)
    assert all(n > 0 for n in nodes), nodes
    assert sum(nodes) == r1.counters.search_nodes
    assert sum(s["nodes_donated"] for s in stats) == sum(s["nodes_adopted"] for s in stats) > 0


def test_native_sharded_headline_two_shards(stcsp, golden):
    name = "partialorder_14"
    m = stcsp.Model.from_name(name)
    a, merged, stats, nodes, engines, g = run_local(stcsp, m, 2)
    gold = golden[name]
    assert (a.n_live_states, a.n_live_edges, a.canonical_sha256()) == (gold["states"], gold["edges"], gold["canonical_sha256"])
    assert sum(nodes) == gold["search"] and all(n > 0 for n in nodes)


def test_native_sharded_wide_domains(stcsp, RefOracle):
    from test_wide_gpu import WIDE
    m = stcsp.Model(text=WIDE["hull_next_sum"])
    o = RefOracle(m)
    ro = o.solve()
    ao, _ = finish(o, ro)
    a, merged, stats, nodes, engines, g = run_local(stcsp, m, 2, knobs=SHARE)
    assert a.canonical_sha256() == ao.canonical_sha256() and merged.counters.dominance == ro.counters.dominance


@pytest.mark.parametrize("call,rank", [("commit", 1), ("expand_local", 0), ("donate", 0), ("adopt", 1)])
def test_native_sharded_failure_ends_every_rank(stcsp, monkeypatch, call, rank):
    """An engine call that fails on ONE rank: every rank returns an error at the same superstep (threads all end)."""
    inst = stcsp.instances
    m = stcsp.Model(text=inst.synthetic(24, 8, 125, 4, 7)) if call in ("donate", "adopt") else stcsp.Model.from_name("partialorder_10")
    monkeypatch.setenv("STCSP_FAULT", f"{call},{rank},{1 if call in ('donate', 'adopt') else 2}")
    engines = [stcsp.Engine(m, rank=r, world=2) for r in range(2)]
    monkeypatch.delenv("STCSP_FAULT")
    g = stcsp.LocalGroup(2)
    with pytest.raises(stcsp.StcspError):
        g.solve(engines, **SHARE)
    assert all(ex is not None for ex in g.errors), g.errors
    assert "injected fault" in str(g.errors[rank]) and "failed in" in str(g.errors[1 - rank])


@pytest.mark.parametrize("name", ["juggling_b4_f5", "partialorder_12"])
def test_native_sharded_rccl_world1(stcsp, golden, monkeypatch, name):
    """The RCCL transport (ncclAllGather for the count table, grouped ncclSend / ncclRecv on the engine's stream) with a
    communicator of size 1. A single shard owns every state and would commit every leaf in place: STCSP_FORCE_CANDIDATES
    sends them all through the exchange (RCCL send / recv to itself) and k_commit instead."""
    m = stcsp.Model.from_name(name)
    monkeypatch.setenv("STCSP_FORCE_CANDIDATES", "1")
    e = stcsp.Engine(m, rank=0, world=1, flags=stcsp.F_STEPPED)
    monkeypatch.delenv("STCSP_FORCE_CANDIDATES")
    t = stcsp.RcclTransport(stcsp.rccl_unique_id(), 0, 1, 0)
    st = stcsp.solve_sharded_native(e, t.ptr)
    r = e.export()
    h, merged = stcsp.merge_shards([r])
    a = stcsp.Automaton(m, merged).traverse().renumber()
    gold = golden[name]
    assert (a.n_live_states, a.n_live_edges, a.canonical_sha256()) == (gold["states"], gold["edges"], gold["canonical_sha256"])
    assert st["candidates_sent"] == st["candidates_received"] == e.counters().leaves > 0  # every leaf travelled
    t.close()


@pytest.mark.parametrize("name,flags", [("juggling_b4_f6", ["-s"]), ("digitinvader4", ["-s", "-a"]), ("partialorder_11", ["-s"])])
def test_cli_shards_writes_the_same_files(stcsp, tmp_path, name, flags):
    """`stcsp --shards=N` (N host threads, one engine each, in-process transport) against the unsharded command line: the
    same statistics fields and byte-identical solutions.dot (the writer orders edges by label)."""
    import subprocess
    exe = stcsp.CSRC / "stcsp"
    src = tmp_path / f"{name}.csp"
    src.write_text(stcsp.instances.by_name(name))
    outs = []
    for extra in ([], ["--shards=2"], ["--shards=3"]):
        d = tmp_path / ("one" if not extra else extra[0].replace("=", ""))
        d.mkdir()
        r = subprocess.run([str(exe), *flags, *extra, str(src)], cwd=d, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        line = r.stdout.strip().split("\n")[-1]
        head = r.stdout[: r.stdout.rfind(line)]
        fields = line.split("\t")
        outs.append((head, fields[1:6], (d / "solutions.dot").read_bytes()))
    assert outs[0][0] == outs[1][0] == outs[2][0]          # "adver1: ..." part
    assert outs[0][1][:3] == outs[1][1][:3] == outs[2][1][:3]  # var con dom
    assert outs[0][2] == outs[1][2] == outs[2][2]


def test_native_sharded_resolve_on_the_same_engines(stcsp, golden):
    """The -t loop of the reference re-solves one model (src/solver.cpp:295-349): the same engines and the same transport group
    run the sharded search again and again (the table's generation, the plan mirror and the transport's barriers all start over)."""
    name = "digitinvader3"
    m = stcsp.Model.from_name(name)
    engines = [stcsp.Engine(m, rank=r, world=3) for r in range(3)]
    g = stcsp.LocalGroup(3)
    gold = golden[name]
    for _ in range(3):
        g.solve(engines, budget_rounds=1, share_per_rank=2)
        h, merged = stcsp.merge_shards([e.export() for e in engines])
        a = stcsp.Automaton(m, merged).traverse().renumber()
        assert (a.n_live_states, a.n_live_edges, a.canonical_sha256()) == (gold["states"], gold["edges"], gold["canonical_sha256"])
        assert sum(e.counters().search_nodes for e in engines) == gold["search"]


# ------------------------------------------------------------------------------------- the strides the scalar model cannot follow
# The mixed runs (tests/test_mixed_shards_gpu.py) put the scalar frontier model beside the engine; it takes W = 1, no interval
# domains, at most 32 until constraints and no big scope. The records of every other shape travel between engines only: one row
# each, wide enough (free booleans) that open nodes really move, and below the record-level law for the same rows.
def engine_rows():
    import kernel_matrix as km
    from mixed_rows import free_booleans
    from test_many_until import many_until
    Row = namedtuple("Row", "text k flags cell untils")
    iv = importlib.import_module("stcsp-solver_amd").F_INTERVAL_DOMAINS
    return {
        # name           model text                                                       K  flags  kernel-matrix row of the same cell  untils
        "w2_dr8": Row(km.walker(40) + km.pad(54) + free_booleans(5), 2, 0, "block8_w2", 1),           # N = 65: 260 words
        "w4_dr4": Row(km.walker(100) + km.pad(21) + free_booleans(5), 2, 0, "wide_w4_dr4", 1),        # N = 32: 256 words
        "intervals_dr4": Row(km.walker(200) + km.pad(22) + free_booleans(5), 2, iv, "wide_w0_dr4", 1),  # N = 33: 132 words
        "until_uw2": Row(many_until(40, free=6), 2, 0, "until_dr4_plain_kr1", 40),
        "until_uw3_u70": Row(many_until(70, free=6), 2, 0, "until_dr4_cs_kr2", 70),
        "until_uw3_u97": Row(many_until(97, free=6), 2, 0, "until_dr4_cs_kr2", 97),
        "until_uw4": Row(many_until(124, free=6), 2, 0, "until_dr4_cs_kr2", 124),
        "big_scope_w1": Row(km.scoped(65, "sum")() + free_booleans(5), 1, 0, "big_scope_dr4_plain_kr1", 0),
        "big_scope_w2": Row(km.scoped(65, "sum", top=40)() + free_booleans(5), 1, 0, "big_scope_dr4_w2_kr1", 0),
    }


ENGINE_ROWS = engine_rows()
_oracle = {}


def oracle_of(stcsp, RefOracle, name):
    """The oracle's run of a row, once: (model, canonical automaton, counters)."""
    if name not in _oracle:
        row = ENGINE_ROWS[name]
        m = stcsp.Model(text=row.text, prefix_k=row.k)
        o = RefOracle(m, time_limit_s=60.0)
        ro = o.solve()
        assert not ro.truncated
        ao, _ = finish(o, ro)
        _oracle[name] = (m, ao.canonical(), ro.counters.dominance, ro.counters.search_nodes, ro.counters.fails)
    return _oracle[name]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", list(ENGINE_ROWS))
def test_native_sharded_moves_nodes_of_every_stride(stcsp, RefOracle, monkeypatch, name, world):
    import kernel_matrix as km
    row = ENGINE_ROWS[name]
    m, canonical, dom, search_nodes, fails = oracle_of(stcsp, RefOracle, name)
    one_expansion_per_round(monkeypatch)
    a, merged, stats, nodes, engines, g = run_local(stcsp, m, world, knobs=SHARE, flags=row.flags)
    donated, adopted = [s["nodes_donated"] for s in stats], [s["nodes_adopted"] for s in stats]
    print(f"{name} world {world}: donated {donated} adopted {adopted} nodes {nodes}")
    assert all(e.kernel_choice() == km.choice(km.ROW[row.cell]) for e in engines)
    assert a.canonical() == canonical
    assert merged.counters.dominance == dom
    if fails == 0 and merged.counters.fails == 0:
        assert sum(nodes) == search_nodes
    assert sum(donated) == sum(adopted) > 0
    for e in engines:
        e.close()
    g.close()


def stepped_to_the_end(e, cands, on_open=None):
    """The plain world-1 loop of the stepping calls: expand, hand the own outbox back through commit, until nothing is left.
    `on_open(left)` runs after every expand_local that leaves open nodes."""
    while True:
        left = e.expand_local()
        if left and on_open:
            on_open(left)
        ptr, n = e.outbox(0)
        if left == 0 and n == 0:
            break
        e.commit(cands.load(ptr, n * (e.candidate_bytes() // 4)), n)
    e.finish()
    return e.export()


@pytest.mark.parametrize("name", list(ENGINE_ROWS))
def test_transfer_records_round_trip(stcsp, RefOracle, monkeypatch, name):
    """The record-level law of k_donate[_until] / k_adopt[_until] on one stepped engine: what is donated, adopted and donated
    again is the same multiset of records (header and block; the padding is unspecified), every record decodes by
    tests/xfer_ref.py into non-empty domains inside the initial ones with nothing beyond the last expire word, and the search
    that goes on from the adopted nodes is the undisturbed one. Once while the frontier is still the root's (the issue of a
    budget of one round and four open nodes), then in every superstep until each expire word past the first has been seen
    non-zero (they fill as the counter passes the flags of the until constraints 32, 64 and 96)."""
    import kernel_matrix as km
    import xfer_ref as xr
    row = ENGINE_ROWS[name]
    m, canonical, dom, search_nodes, fails = oracle_of(stcsp, RefOracle, name)
    one_expansion_per_round(monkeypatch)
    lib = stcsp.hip_lib()
    e = stcsp.Engine(m, rank=0, world=1, flags=row.flags | stcsp.F_STEPPED)
    choice = e.kernel_choice()
    assert choice == km.choice(km.ROW[row.cell])
    form, N, K, bounds = choice["domain_form"], m.n_vars, row.k, m.var_bounds()
    nsw = e.node_bytes() // 4
    assert nsw == xr.stride(N, K, form)
    uw = xr.expire_words(row.untils)
    first, again, cands = DeviceWords(lib), DeviceWords(lib), DeviceWords(lib)
    seen = [False] * uw  # expire word j non-zero in some record
    trips = moved = 0

    def round_trip(left):
        nonlocal trips, moved
        if trips >= 4 and all(seen[1:]):
            e.set_expand_budget(0, 0)  # enough: run every later frontier dry
            return
        ptr, n = e.donate(left)  # (asks for `left`: the engine sizes its buffer by what is asked for)
        assert n == left
        e.adopt(first.load(ptr, n * nsw), n)
        ptr, n2 = e.donate(n)
        assert n2 == n
        e.adopt(again.load(ptr, n * nsw), n)
        a, b = first.host().reshape(n, nsw), again.host().reshape(n, nsw)
        assert sorted(xr.payload(r, N, K, form) for r in a) == sorted(xr.payload(r, N, K, form) for r in b)
        for rec in a:
            d = xr.decode(rec, N, K, form, row.untils)
            xr.check(d, bounds, K, form, row.untils)
            for j, x in enumerate(d["expire"]):
                seen[j] = seen[j] or x != 0
        trips += 1
        moved += n

    e.set_expand_budget(1, 4)
    e.begin()
    r = stepped_to_the_end(e, cands, round_trip)
    print(f"{name}: {trips} round trips, {moved} records, expire words seen non-zero {seen}")
    assert trips >= 1 and moved >= 4
    assert all(seen[1:]), seen
    assert r.n_until_cons == row.untils
    h, merged = stcsp.merge_shards([r])  # (a stepped engine exports a shard: the raw edge log)
    assert stcsp.Automaton(m, merged).traverse().renumber().canonical() == canonical and merged.counters.dominance == dom
    work = lambda c: (c.search_nodes, c.fails, c.leaves, c.gac_calls, c.revisions, c.wave_revisions, c.sweeps, c.skipped_revisions)  # noqa: E731
    disturbed = work(e.counters())
    for buf in (first, again, cands):
        buf.free()
    e.close()
    e2 = stcsp.Engine(m, rank=0, world=1, flags=row.flags | stcsp.F_STEPPED)
    calls = 0

    def same_schedule(left):  # hands control back where the first engine did, and moves nothing
        nonlocal calls
        if calls >= trips:
            e2.set_expand_budget(0, 0)
        calls += 1

    e2.set_expand_budget(1, 4)
    e2.begin()
    stepped_to_the_end(e2, cands, same_schedule)
    undisturbed = work(e2.counters())
    print(f"{name}: (nodes, fails, leaves, gac calls, revisions, wave revisions, sweeps, skipped) disturbed {disturbed} undisturbed {undisturbed}")
    # every node is expanded once, from the same block and the same dirty seed wherever it has been in between: the same tree and
    # the same work (an adopt that lost the seed would revise every item of the node: more revisions and sweeps)
    assert disturbed == undisturbed
    if fails == 0 and undisturbed[1] == 0:
        assert disturbed[0] == search_nodes
    cands.free()
    e2.close()
