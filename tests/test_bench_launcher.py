"""bench.py's own N-rank launcher (`python bench.py --gpus N` without torchrun): the parent starts N rank processes
BEFORE touching any GPU, waits, prints rank 0's line. On CPU the ranks run the oracle's frontier model over gloo,
injected by tests/bench_cpu_entry.py (bench.py has no switch for it), so the launcher, the rendezvous, the sharded
pipeline, the N>1 output line and the exit codes are exercised without GPUs."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


def run_bench(*argv, timeout=300, entry="bench.py"):
    return subprocess.run([sys.executable, str(REPO / entry), *argv], capture_output=True, text=True, timeout=timeout)


CPU_ENTRY = "tests/bench_cpu_entry.py"


def last_json(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert lines, stdout
    return json.loads(lines[-1])


@pytest.mark.parametrize("world", [2, 3])
def test_bench_starts_its_own_ranks(oracle_lib, golden, world):
    r = run_bench("--gpus", str(world), "--workload", "partialorder_10", "--steps", "1", "--warmup", "0", "--full",
                  "--scalable-workload", "juggling_b4_f5", "--synthetic-seconds", "0", entry=CPU_ENTRY)
    assert r.returncode == 0, r.stderr[-2000:]
    d = last_json(r.stdout)
    assert d["n_gpus"] == world
    assert d["config"]["sharding"] == f"state-owner x{world}"
    assert d["parity"]["ok"] and d["parity"]["canonical_sha256"] == golden["partialorder_10"]["canonical_sha256"]
    sh = d["config"]["sharded"]
    assert len(sh["rank_search_nodes_per_step"]) == world and all(n > 0 for n in sh["rank_search_nodes_per_step"])
    assert sum(sh["rank_search_nodes_per_step"]) == d["config"]["nodes_per_step"] == 55636
    assert sum(sh["nodes_donated"]) == sum(sh["nodes_adopted"])
    extra = sh["scalable_workloads"]["juggling_b4_f5"]
    assert extra["nodes"] == 327 and len(extra["rank_search_nodes"]) == world
    assert "TEST ONLY" in d["config"]["engine"]


def test_bench_time_boxed_synthetic_through_the_sharded_pipeline(oracle_lib):
    """The N>1 line carries the time-boxed synthetic workload through solve_sharded (here a 24 x 8 member of the family
    that never reaches a leaf either: the CPU stand-in manages ~3 k nodes/s on 64 x 32): every rank gets work."""
    r = run_bench("--gpus", "2", "--workload", "juggling_b4_f5", "--steps", "1", "--warmup", "0", "--full",
                  "--scalable-workload", "", "--synthetic-seconds", "20.0", "--synthetic-shape", "24,8,125,4,7",
                  "--budget-rounds", "1", "--share-per-rank", "2", entry=CPU_ENTRY)
    assert r.returncode == 0, r.stderr[-2000:]
    d = last_json(r.stdout)
    s = d["config"]["sharded"]["scalable_workloads"]["synthetic"]
    assert s["time_box_s"] == 20.0 and s["leaves"] == 0
    assert all(n > 0 for n in s["rank_search_nodes"]), s
    assert sum(s["nodes_donated"]) == sum(s["nodes_adopted"]) > 0


def test_bench_refuses_more_gpus_than_visible():
    """No GPU in the CPU container: --gpus 2 must exit non-zero with a message (not print an n_gpus = 1 line)."""
    from conftest import visible_gpus
    if visible_gpus() >= 2:
        pytest.skip("this box has the GPUs")
    r = run_bench("--gpus", "2", "--steps", "1", "--warmup", "0", timeout=120)
    assert r.returncode != 0
    assert "sees" in r.stderr and not any(ln.startswith("{") for ln in r.stdout.splitlines())


def test_bench_world_mismatch_is_an_error():
    import os
    r = subprocess.run([sys.executable, str(REPO / CPU_ENTRY), "--gpus", "1"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr


def test_bench_has_no_switch_that_replaces_the_engine():
    """The benchmark script must not be able to put the checker in the product's place by itself."""
    src = (REPO / "bench.py").read_text()
    assert "--test-engine" not in src and "fmodel" not in src
    r = run_bench("--test-engine", "fmodel", timeout=120)
    assert r.returncode != 0 and "unrecognized arguments" in r.stderr


def test_bench_dump_outputs(golden, tmp_path):
    """--dump-outputs writes the last timed step's automaton (here the shards merged on rank 0) in a numbering that does not
    depend on scheduling: one and two shards number their states differently and still write the same arrays."""
    import numpy as np
    import bench
    dumps = []
    for world in (1, 2):
        out = tmp_path / f"dump{world}"
        r = run_bench("--gpus", str(world), "--workload", "partialorder_10", "--steps", "3", "--warmup", "0", "--full",
                      "--scalable-workload", "", "--synthetic-seconds", "0", "--dump-outputs", str(out), entry=CPU_ENTRY)
        assert r.returncode == 0, r.stderr[-2000:]
        d = last_json(r.stdout)
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["parity"]["ok"]
        assert sum(p.stat().st_size for p in out.glob("*.npy")) <= bench.DUMP_BYTES
        dumps.append({p.stem: np.load(p) for p in out.glob("*.npy")})
    a, b = dumps
    assert sorted(a) == sorted(b) == sorted(["state_cid", "state_sig", "state_fail", "edge_src", "edge_dst", "edge_values",
                                             "var_is_signature", "scalars"])
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    g = golden["partialorder_10"]
    assert a["state_cid"].shape == (g["states"],) and a["edge_values"].shape[0] == g["edges"]
    r = run_bench("--steps", "0", entry=CPU_ENTRY, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


def test_bench_plain_run_is_lean(golden, tmp_path):
    """Without --full the run stops after the timed steps and --dump-outputs: no parity check, no scalable workloads (the
    default partialorder_18 and the 2 s synthetic box would show in the line), and the dumped arrays equal --full's."""
    import numpy as np
    dumps = {}
    for world, full in ((1, True), (1, False), (2, False)):
        out = tmp_path / f"dump{world}{'full' if full else ''}"
        r = run_bench("--gpus", str(world), "--workload", "partialorder_10", "--steps", "2", "--warmup", "1",
                      "--dump-outputs", str(out), *(["--full", "--scalable-workload", "", "--synthetic-seconds", "0"] if full else []),
                      entry=CPU_ENTRY)
        assert r.returncode == 0, r.stderr[-2000:]
        d = last_json(r.stdout)
        assert d["metric"] == "search-tree nodes/sec on partialorder_10.csp" and d["unit"] == "search-tree nodes/s"
        assert d["higher_is_better"] is True and d["dtype"] == "u32" and d["value"] > 0 and d["ms_per_step"] > 0
        assert d["config"]["nodes_per_step"] == 55636
        assert ("parity" in d) == full and ("scalable_workloads" in d["config"]["sharded"]) == full
        if full:
            assert d["parity"]["ok"] and d["parity"]["canonical_sha256"] == golden["partialorder_10"]["canonical_sha256"]
        dumps[(world, full)] = {p.stem: np.load(p) for p in out.glob("*.npy")}
    ref = dumps[(1, True)]
    for key in ((1, False), (2, False)):
        assert sorted(dumps[key]) == sorted(ref)
        assert all(np.array_equal(dumps[key][k], ref[k]) for k in ref), key


def test_dump_outputs_size_cap(tmp_path, monkeypatch):
    """Over the cap, the same seeded rows are kept from run to run and their indices are written beside them."""
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    rng = np.random.default_rng(1)
    out = {"state_cid": np.arange(3000, dtype=np.float64), "state_sig": rng.random((3000, 4), dtype=np.float32),
           "state_fail": np.zeros(3000, np.float32), "edge_src": np.arange(20000, dtype=np.float64),
           "edge_dst": np.arange(20000, dtype=np.float64), "edge_values": rng.random((20000, 5), dtype=np.float32),
           "var_is_signature": np.ones(5, np.float32), "scalars": np.zeros(10)}
    for run in ("a", "b"):
        bench.dump_outputs({k: v.copy() for k, v in out.items()}, str(tmp_path / run))
    a = {p.name: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy")) <= 200_000
    assert all(np.array_equal(a[n], np.load(tmp_path / "b" / n)) for n in a)
    for kind, n in (("state", 3000), ("edge", 20000)):
        idx = a[f"{kind}_index.npy"].astype(np.int64)
        assert 0 < idx.size < n and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["edge_src.npy"], a["edge_index.npy"]) and np.array_equal(a["edge_values.npy"], out["edge_values"][a["edge_index.npy"].astype(np.int64)])
