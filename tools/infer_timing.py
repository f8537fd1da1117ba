"""Stream inference: the device pass (stcsp_engine_infer) against its host twin (stcsp_automaton_infer_streams) on the same
automaton and streams, one core. Streams: sampled by the generator, 30 % of the entries set to MISSING
under a fixed numpy seed. Median of `reps` device calls after a warm-up; the match, backward, forward, support and walk times come
from HIP events around the kernels. Edge visits = streams x steps x live edges; the bytes per edge visit of k_i_backward are the
kernel table's claim (4 lid + 4 dst streamed, 1 match gathered, 8 B of B gathered for a matching edge: at most 17 B, plus 8 B
written per state and level), so the achieved bytes per second quoted are an upper bound. The host twin is timed on
--host-streams streams (default 2) and scaled to the request: it is linear in the streams.
Usage: tools/infer_timing.py [--streams N] [--steps L] [--draws D] [--host-streams K] [instance ...]
STCSP_REPAIR_WAVE_SEGMENT=<d> in the environment moves the out-degree above which a wavefront sweeps a state forward."""
import importlib, os, statistics, sys, time
import numpy as np
sys.path.insert(0, '.')
st = importlib.import_module("stcsp-solver_amd")
REPS = 7
args = sys.argv[1:]


def opt(name, default):
    return int(args.pop(args.index(name) + 1)) if name in args else default


STREAMS, STEPS, DRAWS, HOST = opt("--streams", 256), opt("--steps", 64), opt("--draws", 1), opt("--host-streams", 2)
args = [a for a in args if not a.startswith("--")]

for name in args or ["partialorder_14", "digitinvader9"]:
    m = st.Model.from_name(name)
    e = st.Engine(m)
    r = e.solve()
    post = e.postprocess()
    a = e.automaton(r).import_flags(post)
    for mask_name, mask in (("default", None), ("all", "all")):
        info = e.generator(mask, STEPS)
        values = e.generate(STREAMS, STEPS, seed=1)[0]
        rng = np.random.RandomState(20)
        streams = list(np.where(rng.rand(*values.shape) < 0.3, st.INFER_MISSING, values).astype(np.int32))
        e.generator(mask, 0)  # a fresh build: the first infer pays for the label ids and the dictionaries
        t = time.perf_counter(); dev = e.infer_streams(streams, draws=DRAWS, seed=2); first = time.perf_counter() - t
        runs = []
        for _ in range(REPS):
            dev = e.infer_streams(streams, draws=DRAWS, seed=2)
            res = e.infer_result
            runs.append((res.seconds, res.seconds_match, res.seconds_backward, res.seconds_forward, res.seconds_support, res.seconds_walk))
        total, match, back, fwd, sup, walk = (statistics.median(x[i] for x in runs) for i in range(6))
        visits = STREAMS * STEPS * info.n_edges
        bytes_claimed = visits * 17 + STREAMS * STEPS * r.n_states * 8
        t = time.perf_counter(); hst = a.infer_streams(streams[:HOST], mask, draws=DRAWS, seed=2); host_s = (time.perf_counter() - t) * STREAMS / HOST
        assert np.array_equal(dev[0][:HOST].view(np.uint64), hst[0].view(np.uint64)) and dev[1][:HOST] == hst[1]
        assert all(np.array_equal(x, z) for k in (2, 3, 4) for x, z in zip(dev[k][:HOST], hst[k]))
        print(f"{name:16s} [{mask_name}] live {info.n_states} edges {info.n_edges} max out-degree {info.max_out_degree} labels {res.n_labels} "
              f"streams {STREAMS} x {STEPS} steps, {DRAWS} draw(s), {res.n_batches} batch(es), tables {res.table_bytes / 1e6:.1f} MB, wave segment "
              f"{os.environ.get('STCSP_REPAIR_WAVE_SEGMENT', 'default')}, median log2 count {np.median(np.log2(dev[0])):.1f}", flush=True)
        print(f"    infer {total * 1e3:.2f} ms (first call, with label ids and dictionaries: {first * 1e3:.2f} ms): k_i_match {match * 1e3:.3f} ms, "
              f"k_i_level0 + k_i_backward + k_i_root {back * 1e3:.3f} ms = {visits / back / 1e9:.2f} G edge visits/s <= {bytes_claimed / back / 1e9:.0f} GB/s of the "
              f"{bytes_claimed / 1e9:.2f} GB the kernel table claims at most, k_i_forward + k_i_count {fwd * 1e3:.3f} ms, k_i_support {sup * 1e3:.3f} ms, "
              f"k_i_walk {walk * 1e3:.3f} ms", flush=True)
        print(f"    host twin {host_s * 1e3:.0f} ms ({HOST} streams timed, scaled to {STREAMS}) = {host_s / total:.0f} x the device call", flush=True)
