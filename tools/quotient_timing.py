"""Bisimulation quotient: the device pass (stcsp_engine_quotient) against its host twin (stcsp_automaton_bisimulation) on the same
automaton, both from flags in place to state_class on the host. Median of `reps` device runs after a warm-up.
Usage: tools/quotient_timing.py [instance ...]"""
import importlib, statistics, sys, time
sys.path.insert(0, '.')
st = importlib.import_module("stcsp-solver_amd")
REPS = 7
for name in sys.argv[1:] or ["partialorder_14", "digitinvader9", "juggling_b6_f6", "juggling_b6_f6_nosym"]:
    m = st.Model.from_name(name)
    e = st.Engine(m)
    r = e.solve()
    a = e.automaton(r).import_flags(e.postprocess())
    for mask in (None, "all"):
        e.quotient(mask)
        runs = [e.quotient(mask) for _ in range(REPS)]
        cls, n_classes, rounds, _ = runs[0]
        dev_ms = statistics.median(x[3] for x in runs) * 1e3
        t = time.perf_counter(); hc, hn, hrounds = a.bisimulation(mask); host_ms = (time.perf_counter() - t) * 1e3
        live, edges = int((cls >= 0).sum()), a.n_live_edges
        assert hn == n_classes and (hc == cls).all()
        # bytes one refinement round has to move: 12 B per edge (src, dst, label id), 44 B per state (signature and pair count written,
        # class + signature read, new class written)
        print(f"{name:22s} mask {str(mask):4s} live states {live} edges {edges} classes {n_classes} class edges {e.quotient_result.n_class_edges} "
              f"rounds {rounds} device {dev_ms:.3f} ms (min {min(x[3] for x in runs)*1e3:.3f}, max {max(x[3] for x in runs)*1e3:.3f}) "
              f"host twin {host_ms:.1f} ms  round bytes {(12 * r.n_edges + 44 * r.n_states) / 1e6:.2f} MB", flush=True)
