"""Comparison of two observable languages: the device pass (stcsp_engine_compare) against its host twin (stcsp_compare_observers) on
the same two observers, one core. Two engines in one process; the device time is the median of `reps`
calls after a warm-up (the first call also moves the left observer to the device: reported apart), the kernels' own time comes
from HIP events around them.
Usage: tools/compare_timing.py [left:right:NAME[,NAME...] ...]      (an empty list of names: the variables of the left model's default
mask that the right model has too)"""
import importlib, statistics, sys, time
import numpy as np
sys.path.insert(0, '.')
st = importlib.import_module("stcsp-solver_amd")
REPS = 7
KEYS = ("n_pairs", "n_pair_edges", "levels")
ARRAYS = ("witness_off", "witness_len", "witness_left", "witness_right", "witness_values")
ROWS = ["digitinvader5:digitinvader4:D1", "digitinvader3:digitinvader4:I,GAMEOVER", "partialorder_14:partialorder_13:", "juggling_b4_f5:juggling_b4_f5_nosym:A"]


def observer_of(name, names):
    m = st.Model.from_name(name)
    e = st.Engine(m)
    e.solve()
    e.postprocess()
    e.generator([int(n in names.split(",")) for n in m.var_names], 0)
    return e, e.observer()


for row in [a for a in sys.argv[1:] if not a.startswith("--")] or ROWS:
    left, right, names = row.split(":")
    if not names:
        there = st.Model.from_name(right).var_names
        names = ",".join(n for n in st.Model.from_name(left).var_names if not n.startswith("_V") and n in there)
    (e, ol), (_, orr) = observer_of(left, names), observer_of(right, names)
    t = time.perf_counter(); dev = e.compare(orr); first = time.perf_counter() - t
    runs = []
    for _ in range(REPS):
        dev = e.compare(orr)
        runs.append([dev[k] for k in ("seconds", "seconds_expand", "seconds_number")])
    total, expand, number = (statistics.median(x[i] for x in runs) for i in range(3))
    t = time.perf_counter(); twin = st.compare_observers(ol, orr); host_s = time.perf_counter() - t
    assert all(dev[k] == twin[k] for k in KEYS) and all(np.array_equal(dev[k], twin[k]) for k in ARRAYS), "device and host twin differ"
    print(f"{left} | {right} [{names}]: {ol['n_states']}/{ol['n_edges']} x {orr['n_states']}/{orr['n_edges']} -> {dev['n_pairs']} pairs, "
          f"{dev['n_pair_edges']} edges, {dev['levels']} levels, witnesses {dev['witness_len'].tolist()}, {dev['table_bytes'] / 1e6:.2f} MB")
    print(f"    device {total * 1e3:.2f} ms (first call: {first * 1e3:.2f} ms): k_c_expand {expand * 1e3:.3f} ms, k_c_collect + k_c_number {number * 1e3:.3f} ms, "
          f"host share {(total - expand - number) * 1e3:.2f} ms = {(total - expand - number) / dev['levels'] * 1e6 if dev['levels'] else 0:.0f} us per level; "
          f"host twin {host_s * 1e3:.2f} ms = {host_s / total:.2f}x")
