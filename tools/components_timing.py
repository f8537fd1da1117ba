"""Strongly connected components and lassos: the device pass (stcsp_engine_components) against its host twin
(stcsp_automaton_components) on the same automaton, both from flags in place to the result on the host.
Median of REPS runs after a warm-up, with and without 64 lassos; the results are compared array by array. Kernel time is the
HIP-event time of the launches; the host's share per sweep is what is left of the wall time, divided by the sweeps.
Usage: tools/components_timing.py [instance ...]"""
import importlib, statistics, sys, time
import numpy as np
sys.path.insert(0, '.')
st = importlib.import_module("stcsp-solver_amd")
REPS = 7


def same(a, b):
    keys = ("n_states", "n_components", "n_cyclic", "n_accepting", "n_bottom", "n_omega", "root_omega", "n_lassos")
    arrays = ("state_component", "state_omega", "comp_size", "comp_depth", "comp_flags")
    return (all(a[k] == b[k] for k in keys) and all(np.array_equal(a[k], b[k]) for k in arrays)
            and all(x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) for x, y in zip(a["lassos"], b["lassos"])))


for name in sys.argv[1:] or ["partialorder_14", "partialorder_18", "digitinvader5", "digitinvader9", "juggling_b5_f6"]:
    m = st.Model.from_name(name)
    e = st.Engine(m)
    r = e.solve()
    a = e.automaton(r).import_flags(e.postprocess())
    for lassos in (0, 64):
        e.components(lassos)
        runs = [e.components(lassos) for _ in range(REPS)]
        d = runs[0]
        dev_ms = statistics.median(x["seconds"] for x in runs) * 1e3
        ker_ms = statistics.median(x["seconds_kernels"] for x in runs) * 1e3
        twins = []
        for _ in range(REPS):
            t = time.perf_counter(); h = a.components(lassos); twins.append((time.perf_counter() - t) * 1e3)
        assert same(d, h), f"{name}: device and host twin differ"
        trim, colour, sweeps = (int(x) for x in d["rounds"])
        print(f"{name:16s} lassos {d['n_lassos']:2d} live states {d['n_states']} edges {a.n_live_edges} components {d['n_components']} "
              f"largest {int(d['comp_size'].max(initial=0))} | trim rounds {trim} colouring rounds {colour} sweeps {sweeps} | "
              f"device {dev_ms:.3f} ms (kernels {ker_ms:.3f} ms, host share per sweep {(dev_ms - ker_ms) / max(sweeps, 1) * 1e3:.1f} us) "
              f"host twin {statistics.median(twins):.3f} ms", flush=True)
