"""Turn the raw output of tools/profile_r05.sh ($STCSP_PROFILE_RAW, default profile_raw/r05/) into the summaries committed under profiles/: for every
library tag of the job (before / after / ...) the instruction counters per node and the average k_expand launch of the timed
steps, partialorder_14. usage: tools/profile_r05_summaries.py tag="what that library is" [tag=...]"""
import csv, glob, importlib, json, os, subprocess, sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
RAW = os.environ.get("STCSP_PROFILE_RAW", os.path.join(REPO, "profile_raw", "r05"))
OUT = os.path.join(REPO, "profiles")
st = importlib.import_module("stcsp-solver_amd")
SHA = st.engine_source_sha()
HEAD = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
tags = dict(a.split("=", 1) for a in sys.argv[1:])
COUNTERS = ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_INSTS_SMEM", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR")


def newest(pattern):
    return sorted(glob.glob(pattern, recursive=True), key=os.path.getmtime)[-1]


def bench_line(path):
    for line in open(path):
        if line.startswith("{"):
            return json.loads(line)
    raise SystemExit(f"no JSON line in {path}")


pmc = {"_source": f"tools/profile_r05.sh (engine source sha {SHA} = the `after` library, git parent {HEAD}): per library one pass `rocprofv3 --pmc "
                  "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_SMEM SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVES SQ_WAVE_CYCLES -- python3 bench.py "
                  "--full --steps 1 --warmup 0 --no-cpu-baseline --no-other-workloads` (two solves of partialorder_14: the timed one and the "
                  "compacting-export comparison), sums over all k_expand dispatches divided by the nodes of both solves; all libraries in one job on one box",
       "engine_source_sha": SHA, "git_head": HEAD, "libraries": tags, "per_library": {}}
trace = {"_source": "tools/profile_r05.sh: per library `STCSP_STREAM_EXPORT=0 rocprofv3 --kernel-trace --stats -- python3 bench.py --full --steps 5 --warmup 2 "
                    "--no-cpu-baseline --no-other-workloads` (the kernel by itself, no comparison solve): k_expand dispatch durations of the timed steps",
         "engine_source_sha": SHA, "git_head": HEAD, "libraries": tags, "per_library": {}}
for tag in tags:
    c = json.loads(subprocess.check_output([sys.executable, os.path.join(REPO, "tools", "pmc_summary.py"), os.path.join(RAW, "pmc_" + tag), "k_expand"]))
    b = bench_line(os.path.join(RAW, f"pmc_{tag}.json"))
    nodes = b["config"]["nodes_per_step"] * 2
    pmc["per_library"][tag] = {"nodes_of_the_pass": nodes, "dispatches": c["SQ_WAVE_CYCLES"]["dispatches"],
                               "per_node": {k: c[k]["sum"] / nodes for k in COUNTERS},
                               "instructions_per_node": sum(c[k]["sum"] for k in COUNTERS) / nodes,
                               "wave_cycles_per_node_x4": c["SQ_WAVE_CYCLES"]["sum"] * 4 / nodes, "sums": c}
    sb = bench_line(os.path.join(RAW, f"stats_{tag}.json"))
    rows = list(csv.DictReader(open(newest(os.path.join(RAW, "stats_" + tag, "**", "*_kernel_trace.csv")))))
    d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "k_expand" in r["Kernel_Name"]]
    timed = d[-sb["roofline"]["launches"]:]
    trace["per_library"][tag] = {"k_expand_dispatches": len(d), "avg_us_all": sum(d) / len(d), "timed_dispatches": len(timed),
                                 "avg_us_timed_steps": sum(timed) / len(timed), "kernel_ms_per_timed_solve": sum(timed) / sb["steps"] / 1e3,
                                 "bench_avg_launch_us_hip_events": sb["roofline"]["avg_launch_us"], "bench_value": sb["value"],
                                 "bench_search_only_nodes_per_s": sb["search_only_nodes_per_s"]}
    p, t = pmc["per_library"][tag], trace["per_library"][tag]
    print(tag, {k: round(v, 1) for k, v in p["per_node"].items()}, "instructions", round(p["instructions_per_node"], 1), "wave cycles",
          round(p["wave_cycles_per_node_x4"]), "| trace avg us", round(t["avg_us_timed_steps"], 2), "events", round(t["bench_avg_launch_us_hip_events"], 2))
json.dump(pmc, open(os.path.join(OUT, "r05_p14_pmc.json"), "w"), indent=1)
json.dump(trace, open(os.path.join(OUT, "r05_p14_kernel_trace_summary.json"), "w"), indent=1)
