"""Observer (subset construction): the device pass (stcsp_engine_observer) against its host twin (stcsp_automaton_observer) on the
same automaton, one core. Per instance the default mask and two single-variable masks; the device time is
the median of `reps` calls after a warm-up (the first call after a generator build also orders the out-edges: reported apart),
the kernels' own time comes from HIP events around them.
Usage: tools/observer_timing.py [instance ...]"""
import importlib, statistics, sys, time
import numpy as np
sys.path.insert(0, '.')
st = importlib.import_module("stcsp-solver_amd")
REPS = 7
ARRAYS = ("member_off", "member", "state_final", "edge_src", "edge_dst", "edge_values")
args = [a for a in sys.argv[1:] if not a.startswith("--")]

for name in args or ["partialorder_14", "digitinvader9"]:
    m = st.Model.from_name(name)
    e = st.Engine(m)
    r = e.solve()
    post = e.postprocess()
    a = e.automaton(r).import_flags(post)
    plain = [n for n in m.var_names if not n.startswith("_V")]
    for which in (None, plain[0], plain[-1]):
        mask = None if which is None else [int(n == which) for n in m.var_names]
        e.generator(mask, 0)
        t = time.perf_counter(); dev = e.observer(); first = time.perf_counter() - t
        runs = []
        for _ in range(REPS):
            dev = e.observer()
            runs.append([dev[k] for k in ("seconds", "seconds_items", "seconds_intern", "seconds_commit")])
        total, items, intern, commit = (statistics.median(x[i] for x in runs) for i in range(4))
        t = time.perf_counter(); twin = a.observer(mask); host_s = time.perf_counter() - t
        assert all(np.array_equal(dev[k], twin[k]) for k in ARRAYS), "device and host twin differ"
        print(f"{name} [{'default' if which is None else 'only:' + which}]: {a.n_live_states} live states -> {dev['n_states']} sets, {dev['n_edges']} edges, "
              f"largest set {dev['max_set']}, {dev['levels']} levels, {dev['n_labels']} labels, {dev['table_bytes'] / 1e6:.2f} MB")
        print(f"    device {total * 1e3:.2f} ms (first call, with the ordered out-edges: {first * 1e3:.2f} ms): k_o_items {items * 1e3:.3f} ms, "
              f"k_o_succ<INTERN> {intern * 1e3:.3f} ms, <WRITE> + <VERIFY> {commit * 1e3:.3f} ms; host twin {host_s * 1e3:.2f} ms = {host_s / total:.2f}x")
