"""Optimal solution streams: the device pass (stcsp_engine_optimise) against its host twin (stcsp_automaton_optimise, one core)
on the same automaton, both from flags in place to the result on the host. Median of REPS calls after a
warm-up; the results are compared array by array. Kernel time is the HIP-event time of the launches.
Usage: tools/optimise_timing.py [instance:horizon | instance:horizon:w (with witnesses for every length) | instance:mean ...]
The twin's Karp table takes (n + 1) * n * 8 bytes for a component of n states: a job whose table would pass TWIN_TABLE_BYTES
is timed on the device alone."""
import importlib, statistics, sys, time
import numpy as np
sys.path.insert(0, '.')
st = importlib.import_module("stcsp-solver_amd")
REPS = 7
TWIN_TABLE_BYTES = 4 << 30
JOBS = ["partialorder_14:64", "partialorder_14:64:w", "partialorder_18:64", "partialorder_18:64:w", "digitinvader5:mean", "digitinvader7:mean",
        "digitinvader9:mean", "juggling_b5_f6:mean"]


def same(a, b):
    keys = ("n_states", "n_components", "largest_cyclic", "omega_component", "omega_mean", "comp_mean")
    return (all(a[k] == b[k] for k in keys) and np.array_equal(a["best"], b["best"]) and len(a["witnesses"]) == len(b["witnesses"])
            and (a["state_component"] is None or np.array_equal(a["state_component"], b["state_component"]))
            and all(np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) for x, y in zip(a["witnesses"], b["witnesses"])))


solved = {}
for job in sys.argv[1:] or JOBS:
    name, what, *rest = job.split(":")
    if name not in solved:
        m = st.Model.from_name(name)
        e = st.Engine(m)
        r = e.solve()
        solved.clear()  # one engine at a time
        solved[name] = (m, e, e.automaton(r).import_flags(e.postprocess()))
    m, e, a = solved[name]
    w = [(i * 7 + 3) % 5 - 2 for i in range(m.n_vars)]
    kw = dict(mean=True) if what == "mean" else dict(horizon=int(what), lengths=list(range(int(what) + 1)) if rest else [])
    e.optimise(w, **kw)
    runs = [e.optimise(w, **kw) for _ in range(REPS)]
    d = runs[0]
    dev_ms = statistics.median(x["seconds"] for x in runs) * 1e3
    ker_ms = statistics.median(x["seconds_kernels"] for x in runs) * 1e3
    launches = int(d["rounds"].sum())
    head = (f"{job:24s} live states {d['n_states']} edges {a.n_live_edges} largest cyclic {d['largest_cyclic']} | launches {launches} | "
            f"device {dev_ms:.3f} ms (kernels {ker_ms:.3f} ms, {ker_ms / max(dev_ms, 1e-9) * 100:.0f} %, {ker_ms / max(launches, 1) * 1e3:.1f} us per launch)")
    nmax = int(e.components()["comp_size"].max(initial=0)) if what == "mean" else 0
    if (nmax + 1) * nmax * 8 > TWIN_TABLE_BYTES:
        print(f"{head} | host twin: not run, its Karp table would take {(nmax + 1) * nmax * 8 / 2**30:.1f} GiB", flush=True)
        continue
    twins = []
    for _ in range(REPS if what != "mean" or nmax < 5000 else 1):
        t = time.perf_counter(); h = a.optimise(w, **kw); twins.append((time.perf_counter() - t) * 1e3)
    assert same(d, h), f"{job}: device and host twin differ"
    print(f"{head} | host twin {statistics.median(twins):.3f} ms ({len(twins)} run{'s' if len(twins) > 1 else ''})", flush=True)
