"""Stream monitor: the device pass (stcsp_engine_monitor_build / stcsp_engine_monitor_check) against its host twin
(stcsp_automaton_check_streams) on the same automaton and the same streams, one core. Accepted walks on the
live automaton; median of `reps` device calls after a warm-up; the walk kernels' own time comes from HIP events around them.
Usage: tools/monitor_timing.py [--walks N] [--steps L] [instance ...]"""
import importlib, statistics, sys, time
import numpy as np
sys.path.insert(0, '.')
st = importlib.import_module("stcsp-solver_amd")
REPS = 7
args = sys.argv[1:]
WALKS = int(args.pop(args.index("--walks") + 1)) if "--walks" in args else 100_000
STEPS = int(args.pop(args.index("--steps") + 1)) if "--steps" in args else 64
args = [a for a in args if not a.startswith("--")]


def walks(r, valid, alive, keep, rng):
    """WALKS random walks of STEPS steps from the root over live edges, projected on `keep`: [WALKS * STEPS, len(keep)] (vectorised)."""
    E, N = r.n_edges, r.n_vars
    src = np.ctypeslib.as_array(r.edge_src, shape=(E,))
    dst = np.ctypeslib.as_array(r.edge_dst, shape=(E,))
    val = np.ctypeslib.as_array(r.edge_values, shape=(E * N,)).reshape(E, N)
    ok = (np.frombuffer(alive, np.uint8) != 0) & (np.frombuffer(valid, np.uint8)[src] != 0) & (np.frombuffer(valid, np.uint8)[dst] != 0)
    idx = np.flatnonzero(ok)
    idx = idx[np.argsort(src[idx], kind="stable")]
    start = np.searchsorted(src[idx], np.arange(r.n_states))
    deg = np.searchsorted(src[idx], np.arange(r.n_states), side="right") - start
    state = np.zeros(WALKS, np.int64)
    rows = np.zeros((WALKS, STEPS, len(keep)), np.int32)
    for t in range(STEPS):
        assert (deg[state] > 0).all(), "a live state without a live out-edge: walks of this length do not exist"
        e = idx[start[state] + (rng.random_sample(WALKS) * deg[state]).astype(np.int64)]
        rows[:, t, :] = val[e][:, keep]
        state = dst[e]
    return rows.reshape(WALKS * STEPS, len(keep))


for name in args or ["partialorder_14", "digitinvader9"]:
    m = st.Model.from_name(name)
    e = st.Engine(m)
    r = e.solve()
    post = e.postprocess()
    a = e.automaton(r).import_flags(post)
    valid, final, alive = a.flags()
    for mask in (None, "all"):
        keep = [v for v, n in enumerate(m.var_names) if mask == "all" or not n.startswith("_V")]
        values = walks(r, valid, alive, keep, np.random.RandomState(1))
        offsets = np.arange(WALKS + 1, dtype=np.int64) * STEPS
        e.monitor(mask)
        builds = [e.monitor(mask).seconds for _ in range(REPS)]
        info = e.monitor_info
        out = {}
        for force in (False, True):
            e.check_streams((values, offsets), force_sets=force)
            runs = []
            for _ in range(REPS):
                acc, nend, fin, fb = e.check_streams((values, offsets), force_sets=force)
                mr = e.monitor_result
                runs.append((mr.seconds, mr.seconds_labels, mr.seconds_walk))
            assert (acc == STEPS).all() and fb == 0
            out[force] = (acc, nend, fin, [statistics.median(x[i] for x in runs) for i in range(3)], mr.walk_kernel)
        t = time.perf_counter(); hacc, hnend, hfin, largest = a.check_streams((values, offsets), mask); host_s = time.perf_counter() - t
        for force in (False, True):
            assert (out[force][0] == hacc).all() and (out[force][1] == hnend).all() and (out[force][2] == hfin).all()
        steps, row_bytes = WALKS * STEPS, 4 * len(keep)
        print(f"{name:16s} mask {str(mask):4s} live {info.n_states} edges {info.n_edges} labels {info.n_labels} pairs {info.n_pairs} "
              f"max destinations {info.max_destinations} tables {info.table_bytes / 1e6:.1f} MB  build {statistics.median(builds) * 1e3:.3f} ms "
              f"(min {min(builds) * 1e3:.3f}, max {max(builds) * 1e3:.3f})", flush=True)
        for force in (False, True):
            total, lab, walk = out[force][3]
            print(f"    walk kernel {out[force][4]} ({'forced state sets' if force else 'chosen'}): check {total * 1e3:.2f} ms  k_m_steps {lab * 1e3:.3f} ms = "
                  f"{steps / lab / 1e9:.2f} G steps/s, {steps * (row_bytes + 4) / lab / 1e9:.1f} GB/s over {row_bytes} B rows  walk {walk * 1e3:.3f} ms = "
                  f"{steps / walk / 1e9:.3f} G steps/s, {steps * row_bytes / walk / 1e9:.1f} GB/s against the label rows", flush=True)
        print(f"    host twin {host_s * 1e3:.0f} ms (largest set {largest})  = {host_s / out[False][3][0]:.0f} x the device check", flush=True)
