"""Posterior marginals: the device pass (stcsp_engine_posterior) against stcsp_engine_infer on the same build and request, and
against its host twin (stcsp_automaton_posterior_streams) on one core. Streams: the inputs of
tools/infer_timing.py -- sampled by the generator, 30 % of the entries set to MISSING under a fixed numpy seed. Median of `reps`
device calls after a warm-up; the label-weight + match, backward, forward and bins times come from HIP events around the kernels.
The host twin is timed on --host-streams streams (default 2) and scaled to the request: it is linear in the streams. A stream whose
mass is 2^53 or more has no forward pass (exact 0); the line says how many of the request's streams are exact. --weighted puts the
weights 2 and 3 on the least and the largest value the first variable takes.
Usage: tools/posterior_timing.py [--streams N] [--steps L] [--host-streams K] [--weighted] [instance ...]
STCSP_REPAIR_WAVE_SEGMENT=<d> in the environment moves the out-degree above which a wavefront sweeps a state forward."""
import importlib, os, statistics, sys, time
import numpy as np
sys.path.insert(0, '.')
st = importlib.import_module("stcsp-solver_amd")
REPS = 7
args = sys.argv[1:]


def opt(name, default):
    return int(args.pop(args.index(name) + 1)) if name in args else default


STREAMS, STEPS, HOST = opt("--streams", 256), opt("--steps", 64), opt("--host-streams", 2)
WEIGHTED = "--weighted" in args
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
        streams = list(np.where(rng.rand(*values.shape) < 0.3, st.POSTERIOR_MISSING, values).astype(np.int32))
        weights = None
        if WEIGHTED and info.n_observable:
            weights = [{int(values[:, :, 0].min()): 2, int(values[:, :, 0].max()): 3}] + [None] * (info.n_observable - 1)
        e.generator(mask, 0)  # a fresh build: the first call pays for the label ids and the dictionaries
        t = time.perf_counter(); dev = e.posterior_streams(streams, weights=weights); first = time.perf_counter() - t
        runs, infer = [], []
        for _ in range(REPS):
            dev = e.posterior_streams(streams, weights=weights)
            res = e.posterior_result
            runs.append((res.seconds, res.seconds_weights, res.seconds_backward, res.seconds_forward, res.seconds_bins))
            e.infer_streams(streams)
            infer.append(e.infer_result.seconds)
        total, wts, back, fwd, bins = (statistics.median(x[i] for x in runs) for i in range(5))
        t = time.perf_counter(); hst = a.posterior_streams(streams[:HOST], mask, weights=weights); host_s = (time.perf_counter() - t) * STREAMS / HOST
        assert np.array_equal(dev[0][:HOST].view(np.uint64), hst[0].view(np.uint64)) and dev[2][:HOST] == hst[2] and dev[3][:HOST] == hst[3]
        print(f"{name:16s} [{mask_name}] live {info.n_states} edges {info.n_edges} max out-degree {info.max_out_degree} labels {res.n_labels} "
              f"streams {STREAMS} x {STEPS} steps, {'weighted' if weights else 'all weights 1'}, {int(dev[1].sum())} exact, {res.n_batches} batch(es), tables "
              f"{res.table_bytes / 1e6:.1f} MB, wave segment {os.environ.get('STCSP_REPAIR_WAVE_SEGMENT', 'default')}, median log2 mass "
              f"{np.median(np.log2(dev[0])):.1f}", flush=True)
        print(f"    posterior {total * 1e3:.2f} ms (first call, with label ids and dictionaries: {first * 1e3:.2f} ms): k_p_label_weight + k_i_match "
              f"{wts * 1e3:.3f} ms, k_i_level0 + k_i_backward<true> + k_p_root {back * 1e3:.3f} ms = {STREAMS * STEPS * info.n_edges / back / 1e9:.2f} G edge visits/s, "
              f"k_p_forward(_long) + k_p_final {fwd * 1e3:.3f} ms, k_p_bins {bins * 1e3:.3f} ms", flush=True)
        print(f"    the same request through stcsp_engine_infer (no draws): {statistics.median(infer) * 1e3:.2f} ms = {statistics.median(infer) / total:.2f} x the "
              f"posterior call", flush=True)
        print(f"    host twin {host_s * 1e3:.0f} ms ({HOST} streams timed, scaled to {STREAMS}) = {host_s / total:.0f} x the device call", flush=True)
