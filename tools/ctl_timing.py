"""Fair CTL over the infinite solutions: the device pass (stcsp_engine_ctl) against its host twin (stcsp_automaton_ctl, one core) on
the same automaton, both from flags in place to the result on the host. Median of REPS calls after a
warm-up; the results are compared array by array. Kernel time is the HIP-event time of the launches, the component pass included.
Usage: tools/ctl_timing.py [instance ...]
Per instance the formulas AG EF p, EG p and A[p U q], p and q atoms NAME == VALUE on the model's first two visible variables with the
value their first step shows."""
import importlib, statistics, sys, time
import numpy as np
sys.path.insert(0, '.')
st = importlib.import_module("stcsp-solver_amd")
REPS = 7
INSTANCES = ["partialorder_14", "digitinvader9", "juggling_b5_f6"]
FORMULAS = ["AG EF {p}", "EG {p}", "A[{p} U {q}]"]


def same(a, b):
    return (all(a[k] == b[k] for k in ("n_worlds", "n_initial", "n_initial_sat")) and np.array_equal(a["edge_world"], b["edge_world"])
            and np.array_equal(a["edge_sat"], b["edge_sat"]))


for name in sys.argv[1:] or INSTANCES:
    m = st.Model.from_name(name)
    e = st.Engine(m)
    r = e.solve()
    a = e.automaton(r).import_flags(e.postprocess())
    shown = [i for i, n in enumerate(m.var_names) if not n.startswith("_V")]
    first = e.ctl("EX true", witness=True)["witness"][1]
    row = first[0] if len(first) else np.zeros(m.n_vars, np.int32)
    p, q = (f"{m.var_names[v]} == {int(row[v])}" for v in (shown[0], shown[min(1, len(shown) - 1)]))
    for f in FORMULAS:
        text = f.format(p=p, q=q)
        e.ctl(text)
        runs = [e.ctl(text) for _ in range(REPS)]
        d = runs[0]
        dev_ms = statistics.median(x["seconds"] for x in runs) * 1e3
        ker_ms = statistics.median(x["seconds_kernels"] for x in runs) * 1e3
        sweeps, outer, launches = (int(x) for x in d["rounds"])
        twins = []
        for _ in range(REPS):
            t = time.perf_counter(); h = a.ctl(text); twins.append((time.perf_counter() - t) * 1e3)
        assert same(d, h), f"{name}: {text}: device and host twin differ"
        print(f"{name:18s} {text:40s} worlds {d['n_worlds']} holds at {d['n_initial_sat']} of {d['n_initial']} | sweeps {sweeps}, EG rounds {outer}, "
              f"launches {launches} | device {dev_ms:.3f} ms (kernels {ker_ms:.3f} ms, {ker_ms / max(launches, 1) * 1e3:.1f} us per launch) | "
              f"host twin {statistics.median(twins):.3f} ms", flush=True)
