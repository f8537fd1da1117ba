"""Node-level strength of the production expansion kernels, one parent at a time (tests/node_seam.py), against the plain bounds
model (tests/bounds_ref.py): process_node_wide at W = 2 and W = 4 (dev_wide.hpp), the interval revisions (dev_interval.hpp), and the
W = 1 kernels as a calibration of the seam itself -- there the union of a parent's children must equal Engine.propagate (k_probe),
stcsp_fmodel_propagate (oracle/frontier_model.cpp) and the yardstick in gac mode on the same blocks.

Per parent of every row: the verdict (fail / branch / leaf) is the yardstick's; a branch's two children differ in the branch variable
at point 0 alone, split it at the yardstick's mid, carry seed 1 + that word, and their union is the yardstick's fixpoint word for
word; a leaf's labels are the fixpoint's time-0 values, its advanced block is the fixpoint moved one point on (the fresh last point
only has to lie inside the declared domains) and its expire words follow the until rule. A row marked exact must report no skipped
revision; the rows built to overrun a scan budget (and the one row where the device is weaker by a stated choice) must report some
and are held to soundness: a superset of the fixpoint, no consistent parent wiped out, leaves exact.

A whole solve cannot see propagation that is too weak -- it reaches the same automaton over more nodes; this does."""
import numpy as np
import pytest

import bounds_ref as br
import node_seam as ns
import xfer_ref as xr

pytestmark = pytest.mark.gpu

_runs = {}
_engine_error = []  # an engine call failed on the device: no later row starts anything there


def run_row(stcsp, name):
    """Every batch of a row through the seam, once: (model, bounds, [(yardstick entries, outcomes)], skipped revisions)."""
    if _engine_error:
        pytest.fail(f"not run: an engine call failed earlier in this session ({_engine_error[0]})")
    if name not in _runs:
        try:
            _runs[name] = _run_row(stcsp, name)
        except stcsp.StcspError as ex:
            _engine_error.append(f"{name}: {ex}")
            raise
    return _runs[name]


def _run_row(stcsp, name):
    r = ns.ROWS[name]
    m = stcsp.Model(text=r.text, prefix_k=r.k)
    assert [m.constraint_string(i) for i in range(m.n_constraints)] == [br.show(c) for c in r.cons]
    bounds = ns.declared(r, m)
    nu = ns.n_untils(r)
    seam = ns.Seam(stcsp, m, r.k, r.form, r.flags, nu, ns.sig_vars(r), r.names.index("mk"))
    choice = seam.e.kernel_choice()
    assert (choice["domain_form"], choice["family"]) == (r.form, r.family), choice  # the row cannot drift onto another kernel
    batches = []
    for b in range(r.batches):
        entries, _ = ns.yardstick(r, bounds, b)
        parents = [(ns.expire_list(ex, nu), ns.to_record_domains(d, bounds, r.form)) for ex, d, _, _, _ in entries]
        batches.append((entries, seam.step(parents)))
    skipped = seam.skipped
    seam.close()
    return m, bounds, batches, skipped


def union(a, b, form):
    if form == xr.INTERVALS:
        return [(min(x[0], y[0]), max(x[1], y[1])) for x, y in zip(a, b)]
    return [x | y for x, y in zip(a, b)]


def covers(big, small, form) -> bool:
    if form == xr.INTERVALS:
        return all(x[0] <= y[0] and y[1] <= x[1] for x, y in zip(big, small))
    return all(x & y == y for x, y in zip(big, small))


def inside_declared(doms, bounds, form) -> bool:
    if form == xr.INTERVALS:
        return all(lo <= d[0] <= d[1] <= hi for d, (lo, hi) in zip(doms, bounds))
    return all(d != 0 and d >> (hi - lo + 1) == 0 for d, (lo, hi) in zip(doms, bounds))


def check_parent(r, bounds, entry, out, exact, where):
    expire, doms, ok, fp, cls = entry
    N, K, form = len(r.names), r.k, r.form
    want = ns.to_record_domains(fp, bounds, form) if ok else None
    if exact:
        assert out.verdict == cls[0], (where, out.verdict, cls)
    else:
        assert not (ok and out.verdict == "fail"), (where, "a consistent parent was wiped out")
        if cls[0] == "leaf":
            assert out.verdict == "leaf", (where, out.verdict)
    if out.verdict == "branch":
        a, b = out.children
        diff = [i for i in range(N * K) if a["domains"][i] != b["domains"][i]]
        assert len(diff) == 1 and diff[0] < N, (where, diff)  # the branch variable at point 0 alone
        v = diff[0]
        assert a["seed"] == b["seed"] == 1 + v, (where, a["seed"], b["seed"], v)
        assert a["expire"] == b["expire"] == ns.expire_list(expire, ns.n_untils(r)), where
        lower, upper = sorted((a["domains"], b["domains"]), key=lambda d: d[v])
        whole = union(lower, upper, form)
        if form == xr.INTERVALS:
            lo_, hi_ = whole[v]
            mid = lo_ + (hi_ - lo_) // 2
            assert (lower[v], upper[v]) == ((lo_, mid), (mid + 1, hi_)), (where, lower[v], upper[v])
        else:  # bit positions differ from values by the declared lower bound: the same midpoint
            lo_, hi_ = bounds[v][0] + (whole[v] & -whole[v]).bit_length() - 1, bounds[v][0] + whole[v].bit_length() - 1
            mid = lo_ + (hi_ - lo_) // 2
            below = (2 << (mid - bounds[v][0])) - 1
            assert (lower[v], upper[v]) == (whole[v] & below, whole[v] & ~below), (where, hex(lower[v]), hex(upper[v]), mid)
        if exact:
            assert cls[1:] == (v, mid), (where, cls, v, mid)
            assert whole == want, (where, [(i, whole[i], want[i]) for i in range(N * K) if whole[i] != want[i]])
        elif ok:
            assert covers(whole, want, form), (where, "the device block lost a value of the fixpoint")
    if out.verdict == "leaf":
        c = out.candidate
        if ok:
            assert cls[0] == "leaf" or not exact
        if ok and cls[0] == "leaf":
            assert c["labels"] == [br.d_lo(fp[v]) for v in range(N)], (where, c["labels"])
            moved = want[N:]  # points 1 .. K-1 of the fixpoint are points 0 .. K-2 of the advanced block
            if exact:
                assert c["domains"][: N * (K - 1)] == moved, (where, c["domains"], moved)
            else:
                assert covers(c["domains"][: N * (K - 1)], moved, form), where
            assert inside_declared(c["domains"][N * (K - 1):], bounds, form), (where, c["domains"][N * (K - 1):])
            assert c["expire"] == ns.expire_list(br.next_expire(r.cons, r.names, fp, expire), ns.n_untils(r)), (where, c["expire"])


@pytest.mark.parametrize("name", list(ns.ROWS))
def test_one_expansion_equals_the_bounds_model(stcsp, name):
    r = ns.ROWS[name]
    m, bounds, batches, skipped = run_row(stcsp, name)
    mix = {}
    for b, (entries, outs) in enumerate(batches):
        for i, (entry, out) in enumerate(zip(entries, outs)):
            mix[out.verdict] = mix.get(out.verdict, 0) + 1
    print(f"{name}: device verdicts {mix}, skipped revisions {skipped}")
    if r.exact:
        assert skipped == 0, f"{name} is an exact row: {skipped} skipped revisions"
    else:
        assert skipped > 0, f"{name} is built to overrun a budget and overran none"
    for b, (entries, outs) in enumerate(batches):
        for i, (entry, out) in enumerate(zip(entries, outs)):
            check_parent(r, bounds, entry, out, r.exact, f"{name} batch {b} parent {i}")


@pytest.mark.parametrize("name", ["w1_partialorder_10", "w1_synth80"])
def test_seam_agrees_with_probe_kernel_and_scalar_model(stcsp, oracle_lib, FrontierModel, name):
    """The seam itself, independently of the new yardstick: on the same blocks the union of the children the production kernel
    stores == Engine.propagate (k_probe) == stcsp_fmodel_propagate == the yardstick in gac mode, and so are the four verdicts."""
    from test_propagate_gpu import fmodel_propagate
    r = ns.ROWS[name]
    m, bounds, batches, skipped = run_row(stcsp, name)
    assert skipped == 0
    e = stcsp.Engine(m)
    seen = {"fail": 0, "branch": 0, "leaf": 0}
    for b, (entries, outs) in enumerate(batches):
        blocks = np.array([ns.to_record_domains(d, bounds, 1) for _, d, _, _, _ in entries], dtype=np.uint32)
        got, outcome, probe_skipped = e.propagate(blocks, 0, 0)
        scalar, ok = fmodel_propagate(oracle_lib, FrontierModel, m, blocks)
        assert probe_skipped == 0
        for i, ((expire, doms, y_ok, fp, cls), out) in enumerate(zip(entries, outs)):
            where = f"{name} batch {b} parent {i}"
            assert expire == 0
            assert (out.verdict != "fail") == bool(outcome[i] != 0) == bool(ok[i] != 0) == y_ok, (where, out.verdict, outcome[i], ok[i], y_ok)
            seen[out.verdict] += 1
            if not y_ok:
                continue
            want = ns.to_record_domains(fp, bounds, 1)
            assert [int(x) for x in got[i]] == [int(x) for x in scalar[i]] == want, where
            if out.verdict == "branch":
                assert union(out.children[0]["domains"], out.children[1]["domains"], 1) == want, where
            else:
                assert out.candidate["labels"] == [br.d_lo(fp[v]) for v in range(len(r.names))], where
    print(f"{name}: {seen}")
    assert seen["branch"] > 0 and seen["fail"] > 0
    e.close()
