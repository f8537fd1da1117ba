"""The N>1 path: world_size-2 (and 3) runs of the sharded driver over gloo. On CPU the compute
backend is the oracle's frontier model (tests only); the GPU variant runs two HIP-engine shards
on one GPU with the all-to-all staged through host memory."""
import json
import socket
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(world, name, kind, tmp_path, timeout=300, env=None, prefix_k=None):
    import os
    port = free_port()
    out = tmp_path / "merged.json"
    extra = [] if prefix_k is None else [str(prefix_k)]
    procs = [subprocess.Popen([sys.executable, str(REPO / "tests" / "_sharded_worker.py"), str(r), str(world), str(port),
                               name, kind, str(out), *extra], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              env=dict(os.environ, STCSP_TEST_STACKS_AFTER=str(timeout * 5 // 6), **(env or {})))
             for r in range(world)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            tails = [q.communicate()[0][-4000:] for q in procs]  # what every rank wrote, its stacks at 5/6 of the limit included
            raise AssertionError(f"{kind} run of {name} did not end in {timeout} s; the ranks wrote:\n" + "\n----\n".join(tails)) from None
        logs.append(o)
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    return json.loads(out.read_text())


@pytest.mark.parametrize("world,name", [(2, "juggling_b4_f5"), (2, "digitinvader2"), (3, "juggling_b4_f4_nosym"),
                                        (2, "partialorder_10")])
def test_sharded_driver_gloo_cpu(oracle_lib, golden, tmp_path, world, name):
    r = launch(world, name, "fmodel", tmp_path)
    g = golden[name]
    assert (r["states"], r["edges"], r["sha"]) == (g["states"], g["edges"], g["canonical_sha256"])
    assert r["dom"] == g["dom"]
    if g["fail"] == 0:
        assert r["table"] == g["node"]


# A model without next/first/fby/until has an EMPTY signature: one state per constraint set, and the
# leaf of set 0 must return to the root key [tag 0], which lives on shard 0 whatever its hash says
# (device_types.hpp key_owner). world = 1 gives 1 state / 5 edges; a second "root" on another shard
# would give 2 states / 10 edges.
NOSIG = "var x:[0,1];\nvar y:[0,2];\nx <= y;\n"
# the synthetic family at the shapes the reference-faithful oracle finishes:
# 16 variables x |D| = 8, m = 95 / 88 / 80 point constraints + 4 next-coupled pairs; these instances
# exercise failing branches (most shipped examples never fail)
SYNTH_SMALL = ["synth:16,8,95,4,20261003", "synth:16,8,88,4,20261003", "synth:16,8,80,4,20261003"]


def reference_of(st, RefOracle, spec):
    """Canonical automaton of `spec` by oracle/ref_dfs.cpp (the reference's algorithm restated)."""
    sys.path.insert(0, str(REPO / "tests"))
    from _sharded_worker import load_model
    m = load_model(st, spec)
    o = RefOracle(m)
    r = o.solve()
    a = o.automaton(r).traverse().renumber()
    return a.canonical(), a.canonical_sha256(), r.counters.dominance


@pytest.mark.parametrize("world", [2, 3, 4])
def test_sharded_empty_signature_gloo_cpu(stcsp, oracle_lib, RefOracle, tmp_path, world):
    f = tmp_path / "nosig.csp"
    f.write_text(NOSIG)
    canon, sha, dom = reference_of(stcsp, RefOracle, f"file:{f}")
    r = launch(world, f"file:{f}", "fmodel", tmp_path)
    assert (r["states"], r["edges"]) == (1, 5)
    assert r["sha"] == sha and r["canonical"] == canon
    assert r["table"] == 1  # no second root on another shard


@pytest.mark.parametrize("world,spec", [(2, SYNTH_SMALL[0]), (3, SYNTH_SMALL[1]), (2, SYNTH_SMALL[2])])
def test_sharded_synthetic_gloo_cpu(stcsp, oracle_lib, RefOracle, tmp_path, world, spec):
    canon, sha, dom = reference_of(stcsp, RefOracle, spec)
    r = launch(world, spec, "fmodel", tmp_path)
    assert r["sha"] == sha
    assert r["dom"] == dom


# Frontier redistribution (the branch case of the search, src/solveralgorithm.cpp:911-939, is the
# work that moves). NO_LEAF instances never reach a leaf (pure refutation, like BASELINE config 4 at 64 x 32): without
# redistribution every shard but the root's would stay idle for ever. SHARE: tiny instances must share early.
NO_LEAF = ["synth:24,8,125,4,7", "synth:16,8,95,4,20261003"]
SHARE = {"STCSP_TEST_BUDGET_ROUNDS": "1", "STCSP_TEST_SHARE": "2"}


def test_plan_transfers_is_deterministic_and_balancing():
    import importlib
    sh = importlib.import_module("stcsp-solver_amd.sharded")
    assert sh.plan_transfers([0, 0, 0]) == [[0] * 3] * 3
    assert sh.plan_transfers([10, 9, 11]) == [[0] * 3] * 3          # balanced enough
    p = sh.plan_transfers([100, 0, 0, 0])                            # scatter from the root's shard
    assert p[0] == [0, 25, 25, 25] and all(sum(r) == 0 for r in p[1:])
    p = sh.plan_transfers([90, 10, 0])
    left = [90, 10, 0]
    after = [left[r] - sum(p[r]) + sum(p[q][r] for q in range(3)) for r in range(3)]
    assert sum(after) == 100 and max(after) - min(after) <= 2
    assert sh.plan_transfers([5, 0]) == [[0, 2], [0, 0]]


@pytest.mark.parametrize("world,spec", [(2, NO_LEAF[0]), (3, NO_LEAF[0]), (4, NO_LEAF[0])])
def test_frontier_redistribution_no_leaf_gloo_cpu(stcsp, oracle_lib, FrontierModel, RefOracle, tmp_path, world, spec):
    """Every shard gets work although nobody ever reaches a leaf; the search tree is the unsharded one (open
    nodes are self-contained: whoever expands one produces the same children), so the counts add up exactly."""
    from _sharded_worker import load_model
    m = load_model(stcsp, spec)
    f = FrontierModel(m)
    r1 = f.solve()
    assert r1.counters.leaves == 0 and r1.counters.search_nodes > 100
    r = launch(world, spec, "fmodel", tmp_path, env=SHARE)
    assert all(n > 0 for n in r["rank_nodes"]), r["rank_nodes"]
    assert sum(r["rank_nodes"]) == r1.counters.search_nodes
    assert r["fails"] == r1.counters.fails
    assert sum(r["donated"]) == sum(r["adopted"]) > 0
    canon, sha, dom = reference_of(stcsp, RefOracle, spec)
    assert r["sha"] == sha


@pytest.mark.parametrize("world,name", [(2, "juggling_b4_f5"), (3, "digitinvader2"), (2, "partialorder_10"), (3, SYNTH_SMALL[2])])
def test_frontier_redistribution_parity_gloo_cpu(stcsp, oracle_lib, RefOracle, golden, tmp_path, world, name):
    """Redistribution switched on aggressively on terminating instances (incl. `first` sets that travel):
    automaton parity with the reference's recorded values / the reference-faithful oracle."""
    r = launch(world, name, "fmodel", tmp_path, env=SHARE)
    if name in golden:
        g = golden[name]
        assert (r["states"], r["edges"], r["sha"]) == (g["states"], g["edges"], g["canonical_sha256"])
        assert r["dom"] == g["dom"]
    else:
        canon, sha, dom = reference_of(stcsp, RefOracle, name)
        assert r["sha"] == sha and r["dom"] == dom
    assert sum(r["donated"]) == sum(r["adopted"])
    if name in ("partialorder_10", SYNTH_SMALL[2]):
        assert sum(r["donated"]) > 0  # (the small juggling / digitinvader frontiers may never hold enough to share)


def launch_expect_failure(world, name, tmp_path, env, timeout=120):
    """All ranks must END (non-zero) -- none may be left waiting in a collective."""
    import os
    port = free_port()
    procs = [subprocess.Popen([sys.executable, str(REPO / "tests" / "_sharded_worker.py"), str(r), str(world), str(port),
                               name, "fmodel", str(tmp_path / "merged.json")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              env=dict(os.environ, **env))
             for r in range(world)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("a rank hung after a peer's engine failed")
        logs.append(o)
    return [p.returncode for p in procs], logs


@pytest.mark.parametrize("world,fault", [(2, "donate,0"), (3, "donate,0"), (2, "commit,1,3"), (2, "expand_local,1,4"), (3, "adopt,2"),
                                         (2, "finish,0")])
def test_engine_failure_ends_every_rank_gloo_cpu(stcsp, oracle_lib, tmp_path, world, fault):
    """ADVICE r02 / VERDICT r02 weak #5(iii): an engine error on one rank (a donate shortfall, a failed commit, ...) used to
    raise there only, with the peers blocked in the next all-to-all. Now the ranks agree on a status word before every
    exchange: every rank raises ShardedSolveError and exits."""
    rcs, logs = launch_expect_failure(world, NO_LEAF[0] if "commit" not in fault else "partialorder_10", tmp_path,
                                      dict(SHARE, STCSP_TEST_FAULT=fault))
    assert all(rc != 0 for rc in rcs), (rcs, logs)
    assert all("ShardedSolveError" in lg for lg in logs), logs
    bad = int(fault.split(",")[1])
    assert "injected fault" in logs[bad]


@pytest.mark.gpu
@pytest.mark.parametrize("world,spec", [(2, NO_LEAF[0]), (3, NO_LEAF[0])])
def test_frontier_redistribution_no_leaf_hip_one_gpu(stcsp, oracle_lib, FrontierModel, tmp_path, world, spec):
    """The same with HIP-engine shards on one GPU (k_donate / k_adopt, budgeted expand_local)."""
    from _sharded_worker import load_model
    m = load_model(stcsp, spec)
    f = FrontierModel(m)
    r1 = f.solve()
    r = launch(world, spec, "hip", tmp_path, env=SHARE)
    assert all(n > 0 for n in r["rank_nodes"]), r["rank_nodes"]
    assert sum(r["rank_nodes"]) == r1.counters.search_nodes
    assert r["fails"] == r1.counters.fails
    assert sum(r["donated"]) == sum(r["adopted"]) > 0


@pytest.mark.gpu
def test_synthetic_64x32_time_boxed_two_hip_shards_one_gpu(tmp_path):
    """BASELINE config 4 (64 vars x |D| = 32, frontier sharded) through solve_sharded, time-boxed, with two HIP-engine
    shards on one GPU and the production sharing knobs: both shards search, what one donates the other adopts."""
    r = launch(2, "synth:64,32,602,6,20261003", "hip", tmp_path, env={"STCSP_TEST_TIME_LIMIT": "1.0"}, timeout=600)
    assert all(n > 100000 for n in r["rank_nodes"]), r["rank_nodes"]
    assert sum(r["donated"]) == sum(r["adopted"]) > 0
    assert r["states"] <= 1  # nobody reaches a leaf on this instance


@pytest.mark.gpu
@pytest.mark.parametrize("world,name", [(2, "juggling_b4_f5"), (3, "digitinvader3"), (2, "partialorder_12"), (3, SYNTH_SMALL[2])])
def test_frontier_redistribution_parity_hip_one_gpu(stcsp, oracle_lib, RefOracle, golden, tmp_path, world, name):
    r = launch(world, name, "hip", tmp_path, env=SHARE)
    if name in golden:
        g = golden[name]
        assert (r["states"], r["edges"], r["sha"]) == (g["states"], g["edges"], g["canonical_sha256"])
        assert r["dom"] == g["dom"]
    else:
        canon, sha, dom = reference_of(stcsp, RefOracle, name)
        assert r["sha"] == sha and r["dom"] == dom
    assert sum(r["donated"]) == sum(r["adopted"])
    if name in ("partialorder_12", SYNTH_SMALL[2]):
        assert sum(r["donated"]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_empty_signature_hip_one_gpu(stcsp, oracle_lib, RefOracle, tmp_path, world):
    f = tmp_path / "nosig.csp"
    f.write_text(NOSIG)
    canon, sha, dom = reference_of(stcsp, RefOracle, f"file:{f}")
    r = launch(world, f"file:{f}", "hip", tmp_path)
    assert (r["states"], r["edges"], r["table"]) == (1, 5, 1)
    assert r["canonical"] == canon


@pytest.mark.gpu
@pytest.mark.parametrize("world,spec", [(2, SYNTH_SMALL[0]), (3, SYNTH_SMALL[0]), (2, SYNTH_SMALL[1]), (3, SYNTH_SMALL[1]),
                                        (2, SYNTH_SMALL[2]), (3, SYNTH_SMALL[2])])
def test_sharded_synthetic_hip_one_gpu(stcsp, oracle_lib, RefOracle, tmp_path, world, spec):
    """The synthetic family (BASELINE config 4) through the sharded pipeline with 2 and 3 HIP shards on
    one GPU, at the shapes oracle/ref_dfs.cpp terminates on: canonical text equal to the oracle's."""
    canon, sha, dom = reference_of(stcsp, RefOracle, spec)
    r = launch(world, spec, "hip", tmp_path)
    assert r["sha"] == sha
    if r["canonical"] is not None:
        assert r["canonical"] == canon
    assert r["dom"] == dom


@pytest.mark.gpu
@pytest.mark.parametrize("world,name", [(2, "juggling_b4_f5"), (2, "partialorder_10"), (3, "digitinvader3")])
def test_sharded_hip_engine_one_gpu(golden, tmp_path, world, name):
    r = launch(world, name, "hip", tmp_path)
    g = golden[name]
    assert (r["states"], r["edges"], r["sha"]) == (g["states"], g["edges"], g["canonical_sha256"])
    assert r["dom"] == g["dom"]


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"STCSP_STREAM_EXPORT": "0"}, {"STCSP_STREAM_CHUNK": "16"}],
                         ids=["host-export", "tiny-chunks"])
def test_sharded_hip_export_paths_one_gpu(golden, tmp_path, env):
    """A shard's export (states + RAW leaf-edge log) leaves the device during the supersteps like an unsharded
    result does; the host-side export it replaces and chunks of 16 records give the same merge."""
    name = "partialorder_10"
    r = launch(2, name, "hip", tmp_path, env=env)
    g = golden[name]
    assert (r["states"], r["edges"], r["sha"]) == (g["states"], g["edges"], g["canonical_sha256"])
    assert r["dom"] == g["dom"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["juggling_b4_f5", "digitinvader3", "partialorder_12"])
def test_sharded_pipeline_rccl_world1(golden, tmp_path, name):
    """The N>1 code path with the RCCL ("nccl") backend and device-resident candidate exchange,
    as far as one GPU allows: process group of size 1, STCSP_F_STEPPED engine."""
    r = launch(1, name, "hip-nccl", tmp_path)
    g = golden[name]
    assert (r["states"], r["edges"], r["sha"]) == (g["states"], g["edges"], g["canonical_sha256"])
    assert r["dom"] == g["dom"]
    print(f"{name}: sharded pipeline on one GPU: {r['rounds']} supersteps, {r['stepped_ms']:.2f} ms")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["partialorder_14", "digitinvader9"])
def test_sharded_headline_workloads_two_hip_shards_one_gpu(golden, tmp_path, name):
    """BASELINE's metric instance (partialorder_14 "at 1/2/4/8") and config 5 (digitinvader9 -a on 8 GPUs) through the sharded
    pipeline with two HIP-engine shards on one GPU: the reference's canonical automaton and `dom`, what one shard donates the
    other adopts; digitinvader9 also through the merged -a pass (adver1 == 0 and an empty body, as the reference prints)."""
    env = {"STCSP_TEST_ADVERSARIAL": "1"} if name == "digitinvader9" else {}
    r = launch(2, name, "hip", tmp_path, env=env, timeout=900)
    g = golden[name]
    assert (r["states"], r["edges"], r["sha"]) == (g["states"], g["edges"], g["canonical_sha256"])
    assert r["dom"] == g["dom"]
    assert r["nodes"] == g["search"] and sum(r["rank_nodes"]) == g["search"]
    assert all(n > 0 for n in r["rank_nodes"])
    assert sum(r["donated"]) == sum(r["adopted"])
    if name == "digitinvader9":
        assert r["adver1"] == 0 and r["adv_empty"]


@pytest.mark.gpu
def test_bursts_that_end_at_planner_stops_with_a_second_engine_on_the_gpu(golden, tmp_path):
    """The regime of round 3's late-workgroup race: bursts of launches that run past a planner stop (tiny pools: every pool
    grows again and again; outboxes of 64 candidates: PS_OUTBOX_FULL after a few nodes per region) while a second engine process
    shares the GPU. Exactly one launch may be admitted per planned round (Plan::gate): parity, and nothing lost or duplicated."""
    name = "partialorder_12"
    r = launch(2, name, "hip", tmp_path, env={"STCSP_SMALL_POOLS": "1", "STCSP_CAND_CAP": "64", **SHARE}, timeout=900)
    g = golden[name]
    assert (r["states"], r["edges"], r["sha"]) == (g["states"], g["edges"], g["canonical_sha256"])
    assert r["dom"] == g["dom"] and r["nodes"] == g["search"]
    assert sum(r["donated"]) == sum(r["adopted"]) > 0
