"""Stream generator: the device pass (stcsp_engine_generator_build / stcsp_engine_generate) against its host twin
(stcsp_automaton_generate) on the same automaton, one core. Sampled streams; median of `reps` device
calls after a warm-up; the generate kernel's own time comes from HIP events around it. The twin's time includes its build.
Usage: tools/generate_timing.py [--streams N] [--steps L] [instance ...]"""
import importlib, statistics, sys, time
import numpy as np
sys.path.insert(0, '.')
st = importlib.import_module("stcsp-solver_amd")
REPS = 7
args = sys.argv[1:]
STREAMS = int(args.pop(args.index("--streams") + 1)) if "--streams" in args else 100_000
STEPS = int(args.pop(args.index("--steps") + 1)) if "--steps" in args else 64
args = [a for a in args if not a.startswith("--")]

for name in args or ["partialorder_14", "digitinvader9"]:
    m = st.Model.from_name(name)
    e = st.Engine(m)
    r = e.solve()
    post = e.postprocess()
    a = e.automaton(r).import_flags(post)
    e.generator(None, STEPS)
    builds = [e.generator(None, STEPS).seconds for _ in range(REPS)]
    info = e.generator_info
    e.generate(STREAMS, STEPS, seed=1)
    runs = []
    for _ in range(REPS):
        values, fin = e.generate(STREAMS, STEPS, seed=1)
        runs.append((e.generate_result.seconds, e.generate_result.seconds_kernel))
    total, kernel = (statistics.median(x[i] for x in runs) for i in range(2))
    t = time.perf_counter(); hv, hf, hcount = a.generate(STREAMS, STEPS, seed=1, horizon=STEPS); host_s = time.perf_counter() - t
    assert np.array_equal(values, hv) and np.array_equal(fin, hf) and np.array_equal(info.count, hcount)
    print(f"{name:16s} live {info.n_states} edges {info.n_edges} max out-degree {info.max_out_degree} count[{STEPS}] {info.count[STEPS]:.4g} "
          f"tables {info.table_bytes / 1e6:.1f} MB  build {statistics.median(builds) * 1e3:.3f} ms (min {min(builds) * 1e3:.3f}, max {max(builds) * 1e3:.3f})", flush=True)
    print(f"    generate {total * 1e3:.2f} ms = {STREAMS / total / 1e6:.2f} M streams/s with the copy back; k_g_generate {kernel * 1e3:.3f} ms = "
          f"{STREAMS / kernel / 1e6:.2f} M streams/s, {STREAMS * STEPS / kernel / 1e9:.3f} G steps/s", flush=True)
    print(f"    host twin {host_s * 1e3:.0f} ms (build included) = {host_s / total:.0f} x the device call", flush=True)
