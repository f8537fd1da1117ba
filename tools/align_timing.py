"""Stream alignment: the device pass (stcsp_engine_align) on both of its roads -- the fused kernel, and with
STCSP_ALIGN_FUSED=0 one launch per level and closure sweep -- against the repair (stcsp_engine_repair) on the same streams
and against its host twin (stcsp_automaton_align_streams) on one core. Streams: sampled by the
generator, then 2 % of the steps deleted, 2 % duplicated and 5 % of the entries overwritten by random in-domain values under
a fixed numpy seed. Median of `reps` device calls after a warm-up; the level, cost and walk times come from HIP events around
the kernels. The host twin is timed on --host-streams streams (default 2) and scaled to the request: it is linear in the
streams.
Usage: tools/align_timing.py [--streams N] [--steps L] [--host-streams K] [--costs SKIP:GAP] [instance ...]"""
import importlib, os, statistics, sys, time
import numpy as np
sys.path[:0] = ['.', 'tests']
st = importlib.import_module("stcsp-solver_amd")
from align_ref import damaged, same  # (the corruption the tests use, and the comparison of two results output by output)
REPS = 7
args = sys.argv[1:]


def opt(name, default, kind=int):
    return kind(args.pop(args.index(name) + 1)) if name in args else default


STREAMS, STEPS, HOST = opt("--streams", 256), opt("--steps", 64), opt("--host-streams", 2)
SKIP, GAP = (int(c) for c in opt("--costs", "1:1", str).split(":"))
args = [a for a in args if not a.startswith("--")]


def median_call(call, result, fields):
    call()
    runs = []
    for _ in range(REPS):
        call()
        runs.append([getattr(result(), f) for f in fields])
    return [statistics.median(x[i] for x in runs) for i in range(len(fields))]


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
        lo, hi = [bounds[v][0] for v in keep], [bounds[v][1] for v in keep]
        rng = np.random.RandomState(20)
        streams = [damaged(rng, s, lo, hi) for s in e.generate(STREAMS, STEPS, seed=1)[0]]
        e.generator(mask, 0)
        kw = dict(skip_cost=SKIP, gap_cost=GAP)
        print(f"{name:16s} [{mask_name}] states {r.n_states} live {info.n_states} edges {info.n_edges} max out-degree {info.max_out_degree} "
              f"streams {STREAMS} of about {STEPS} steps, costs {SKIP}:{GAP}", flush=True)
        rep_total, rep_relax = median_call(lambda: e.repair_streams(streams), lambda: e.repair_result, ("seconds", "seconds_relax"))
        rep_dist = e.repair_streams(streams)[0]
        answers = {}
        for road in ("fused", "general"):
            if road == "general":
                os.environ["STCSP_ALIGN_FUSED"] = "0"
            total, levels, cost, walk = median_call(lambda: e.align_streams(streams, **kw), lambda: e.align_result,
                                                    ("seconds", "seconds_levels", "seconds_cost", "seconds_walk"))
            os.environ.pop("STCSP_ALIGN_FUSED", None)
            res = e.align_result
            answers[road] = e.align_streams(streams, **kw)
            print(f"    align, path_kernel {res.path_kernel} ({road} asked): {total * 1e3:.2f} ms: cost {cost * 1e3:.3f} ms, levels {levels * 1e3:.3f} ms, "
                  f"walk {walk * 1e3:.3f} ms; {res.n_batches} batch(es), tables {res.table_bytes / 1e6:.1f} MB", flush=True)
        dev = answers["fused"]
        assert same(dev, answers["general"])
        print(f"    repair on the same streams: {rep_total * 1e3:.2f} ms, k_r_level0 + k_r_relax {rep_relax * 1e3:.3f} ms; mean distance: repair "
              f"{np.mean(rep_dist):.1f}, align {np.mean(dev[0]):.1f} (skipped {np.mean(dev[4]):.2f}, inserted {np.mean(dev[5]):.2f} per stream)", flush=True)
        t = time.perf_counter(); hst = a.align_streams(streams[:HOST], mask, **kw); host_s = (time.perf_counter() - t) * STREAMS / HOST
        assert same([out[:HOST] for out in dev], hst)
        print(f"    host twin {host_s * 1e3:.0f} ms ({HOST} streams timed, scaled to {STREAMS})", flush=True)
