"""Stream repair: the device pass (stcsp_engine_repair) against its host twin (stcsp_automaton_repair_streams) on the same
automaton and streams, one core. Streams: sampled by the generator, 5 % of the entries overwritten by
random in-domain values under a fixed numpy seed. Median of `reps` device calls after a warm-up; the relax, cost and walk times
come from HIP events around the kernels. Relaxations = streams x steps x live edges; the bytes per relaxation are the kernel
table's claim (4 lid + 4 dst streamed, 4 cost + 4 G gathered = 16 B, plus 4 B written per state and level). The host twin is
timed on --host-streams streams (default 2) and scaled to the request: it is linear in the streams.
Usage: tools/repair_timing.py [--streams N] [--steps L] [--host-streams K] [instance ...]
STCSP_REPAIR_WAVE_SEGMENT=<d> in the environment moves the out-degree above which a wavefront relaxes a state."""
import importlib, os, statistics, sys, time
import numpy as np
sys.path.insert(0, '.')
st = importlib.import_module("stcsp-solver_amd")
REPS = 7
args = sys.argv[1:]


def opt(name, default):
    return int(args.pop(args.index(name) + 1)) if name in args else default


STREAMS, STEPS, HOST = opt("--streams", 256), opt("--steps", 64), opt("--host-streams", 2)
args = [a for a in args if not a.startswith("--")]

for name in args or ["partialorder_14", "digitinvader9"]:
    m = st.Model.from_name(name)
    e = st.Engine(m)
    r = e.solve()
    post = e.postprocess()
    a = e.automaton(r).import_flags(post)
    bounds = m.var_bounds()
    for mask_name, mask in (("default", None), ("all", "all")):
        info = e.generator(mask, STEPS)
        keep = [v for v in range(m.n_vars) if mask == "all" or not m.var_names[v].startswith("_V")]
        values = e.generate(STREAMS, STEPS, seed=1)[0]
        rng = np.random.RandomState(20)
        hit = rng.rand(*values.shape) < 0.05
        noise = np.stack([rng.randint(bounds[v][0], bounds[v][1] + 1, size=values.shape[:2]) for v in keep], axis=2).astype(np.int32)
        streams = list(np.where(hit, noise, values))
        e.generator(mask, 0)  # a fresh build: the first repair pays for the label ids
        t = time.perf_counter(); dev = e.repair_streams(streams); first = time.perf_counter() - t
        runs = []
        for _ in range(REPS):
            dev = e.repair_streams(streams)
            res = e.repair_result
            runs.append((res.seconds, res.seconds_relax, res.seconds_cost, res.seconds_walk))
        total, relax, cost, walk = (statistics.median(x[i] for x in runs) for i in range(4))
        relaxations = STREAMS * STEPS * info.n_edges
        bytes_claimed = relaxations * 16 + STREAMS * STEPS * r.n_states * 4
        t = time.perf_counter(); hst = a.repair_streams(streams[:HOST], mask); host_s = (time.perf_counter() - t) * STREAMS / HOST
        assert all(np.array_equal(dev[i][:HOST], hst[i]) for i in (0, 2, 3)) and all(np.array_equal(x, z) for x, z in zip(dev[1][:HOST], hst[1]))
        print(f"{name:16s} [{mask_name}] live {info.n_states} edges {info.n_edges} max out-degree {info.max_out_degree} labels {res.n_labels} "
              f"streams {STREAMS} x {STEPS} steps, {res.n_batches} batch(es), tables {res.table_bytes / 1e6:.1f} MB, wave segment "
              f"{os.environ.get('STCSP_REPAIR_WAVE_SEGMENT', 'default')}, mean distance {np.mean(dev[0]):.1f}", flush=True)
        print(f"    repair {total * 1e3:.2f} ms (first call, with the label ids: {first * 1e3:.2f} ms): k_r_cost {cost * 1e3:.3f} ms, k_r_level0 + k_r_relax "
              f"{relax * 1e3:.3f} ms = {relaxations / relax / 1e9:.2f} G relaxations/s = {bytes_claimed / relax / 1e9:.0f} GB/s of the "
              f"{bytes_claimed / 1e9:.2f} GB the kernel table claims, k_r_walk {walk * 1e3:.3f} ms", flush=True)
        print(f"    host twin {host_s * 1e3:.0f} ms ({HOST} streams timed, scaled to {STREAMS}) = {host_s / total:.0f} x the device call", flush=True)
