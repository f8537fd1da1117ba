"""stcsp-solver_amd -- MI355X-native stream-CSP propagation + search engine.

Host-side Python mirror of the C-ABI in include/stcsp_engine.h / include/stcsp_host.h (ctypes,
no torch types in any signature).  The package name contains a hyphen (it mirrors the upstream
repository name), so import it with::

    import importlib; stcsp = importlib.import_module("stcsp-solver_amd")

The HIP engine library is REQUIRED for `Engine`: there is no CPU fallback anywhere in this
package; a missing / unloadable libstcsp_hip.so raises immediately.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
CSRC = PKG_DIR / "csrc"
REPO = PKG_DIR.parent

from . import instances  # noqa: E402  (pure python, no native deps)


# ------------------------------------------------------------------ ctypes mirrors
class Node(C.Structure):
    _fields_ = [("token", C.c_int32), ("num", C.c_int32), ("var", C.c_int32), ("arr", C.c_int32),
                ("left", C.c_int32), ("right", C.c_int32)]


class Problem(C.Structure):
    _fields_ = [("n_vars", C.c_int32), ("prefix_k", C.c_int32),
                ("var_lb", C.POINTER(C.c_int32)), ("var_ub", C.POINTER(C.c_int32)),
                ("var_names", C.POINTER(C.c_char_p)),
                ("n_arrays", C.c_int32), ("array_off", C.POINTER(C.c_int32)), ("array_data", C.POINTER(C.c_int32)),
                ("n_nodes", C.c_int32), ("nodes", C.POINTER(Node)),
                ("n_constraints", C.c_int32), ("constraint_root", C.POINTER(C.c_int32))]


class Options(C.Structure):
    _fields_ = [("device", C.c_int32), ("rank", C.c_int32), ("world", C.c_int32), ("batch_nodes", C.c_int32),
                ("max_search_nodes", C.c_int64), ("time_limit_s", C.c_double), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


class Counters(C.Structure):
    _fields_ = [("search_nodes", C.c_int64), ("gac_calls", C.c_int64), ("fails", C.c_int64),
                ("dominance", C.c_int64), ("leaves", C.c_int64), ("revisions", C.c_int64),
                ("evaluations", C.c_int64), ("levels", C.c_int64),
                ("seconds_search", C.c_double), ("seconds_export", C.c_double),
                ("seconds_expand_kernel", C.c_double), ("expand_launches", C.c_int64),
                ("wave_revisions", C.c_int64), ("sweeps", C.c_int64), ("skipped_revisions", C.c_int64),
                ("translation_stops", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class KernelChoice(C.Structure):
    """stcsp_kernel_choice (include/stcsp_engine.h): the expansion, probe and commit kernel by their template arguments."""
    _fields_ = [(n, C.c_int32) for n in (
        "family", "dom_regs", "domain_form", "key_regs", "image_in_lds", "compact_sweeps", "lite", "big_workgroup",
        "one_register_shape", "expand_threads", "probe_family", "probe_image_in_lds", "probe_compact_sweeps", "probe_lite",
        "commit_family", "commit_key_regs")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# KernelChoice.family / .probe_family / .commit_family (STCSP_KF_* / STCSP_KP_* / STCSP_KC_*)
KF_VARIANT, KF_PREFIX, KF_WIDE_DOMAINS, KF_LONG_KEY, KF_LARGE_BLOCK, KF_UNTIL_HEAVY, KF_BIG_SCOPE = range(7)
KP_PROBE, KP_PROBE_BIG = 0, 1
KC_COMMIT, KC_COMMIT_UNTIL = 0, 1


class Result(C.Structure):
    _fields_ = [("n_states", C.c_int64), ("sig_len", C.c_int32), ("n_sig_vars", C.c_int32),
                ("n_until", C.c_int32), ("n_until_cons", C.c_int32),
                ("state_cid", C.POINTER(C.c_int32)), ("state_sig", C.POINTER(C.c_int32)),
                ("state_fail", C.POINTER(C.c_uint8)),
                ("n_edges", C.c_int64), ("edge_src", C.POINTER(C.c_int64)), ("edge_dst", C.POINTER(C.c_int64)),
                ("edge_values", C.POINTER(C.c_int32)),
                ("n_vars", C.c_int32), ("n_constraint_sets", C.c_int32),
                ("var_is_signature", C.POINTER(C.c_uint8)),
                ("root_final", C.c_int32), ("truncated", C.c_int32),
                ("counters", Counters)]


class PostOptions(C.Structure):
    _fields_ = [("adversarial_var", C.c_int32), ("adversarial2_op", C.c_int32), ("adversarial2_ava", C.c_int32),
                ("reserved", C.c_int32)]


class PostResult(C.Structure):
    _fields_ = [("n_states", C.c_int64), ("n_edges", C.c_int64),
                ("state_valid", C.POINTER(C.c_uint8)), ("state_final", C.POINTER(C.c_uint8)),
                ("edge_alive", C.POINTER(C.c_uint8)),
                ("adver1", C.c_int32), ("adver2", C.c_int32), ("rounds", C.c_int32 * 3), ("seconds", C.c_double)]


class QuotientOptions(C.Structure):
    _fields_ = [("observable", C.POINTER(C.c_uint8)), ("reserved", C.c_int32 * 2)]


class QuotientResult(C.Structure):
    _fields_ = [("n_states", C.c_int64), ("n_classes", C.c_int64), ("n_class_edges", C.c_int64),
                ("state_class", C.POINTER(C.c_int32)), ("rounds", C.c_int32), ("seconds", C.c_double)]


class MonitorOptions(C.Structure):
    _fields_ = [("observable", C.POINTER(C.c_uint8)), ("reserved", C.c_int32 * 2)]


class MonitorInfo(C.Structure):
    _fields_ = [("n_states", C.c_int64), ("n_edges", C.c_int64), ("n_labels", C.c_int64), ("n_pairs", C.c_int64),
                ("table_bytes", C.c_int64), ("n_observable", C.c_int32), ("max_destinations", C.c_int32),
                ("set_capacity", C.c_int32), ("root_live", C.c_int32), ("seconds", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class MonitorStreams(C.Structure):
    _fields_ = [("n_streams", C.c_int64), ("offsets", C.POINTER(C.c_int64)), ("values", C.POINTER(C.c_int32)),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class MonitorResult(C.Structure):
    _fields_ = [("n_streams", C.c_int64), ("accepted_len", C.POINTER(C.c_int32)), ("n_end", C.POINTER(C.c_int32)),
                ("end_final", C.POINTER(C.c_uint8)), ("n_host_fallback", C.c_int64), ("walk_kernel", C.c_int32),
                ("reserved", C.c_int32), ("seconds", C.c_double), ("seconds_labels", C.c_double), ("seconds_walk", C.c_double)]


MON_FORCE_SETS = 1  # check_streams(force_sets=True): the state-set kernel under a deterministic mask too (tests, measurements)


class GeneratorOptions(C.Structure):
    _fields_ = [("observable", C.POINTER(C.c_uint8)), ("horizon", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


class GeneratorInfo(C.Structure):
    _fields_ = [("n_states", C.c_int64), ("n_edges", C.c_int64), ("table_bytes", C.c_int64), ("_count", C.POINTER(C.c_double)),
                ("n_observable", C.c_int32), ("horizon", C.c_int32), ("max_out_degree", C.c_int32), ("root_live", C.c_int32),
                ("seconds", C.c_double)]
    count = None  # numpy float64 [horizon + 1], a copy (Engine.generator() sets it)

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if not n.startswith("_")}


class GenerateRequest(C.Structure):
    _fields_ = [("n_streams", C.c_int64), ("ranks", C.POINTER(C.c_uint64)), ("seed", C.c_uint64), ("len", C.c_int32),
                ("reserved", C.c_int32)]


class GenerateResult(C.Structure):
    _fields_ = [("n_streams", C.c_int64), ("values", C.POINTER(C.c_int32)), ("end_final", C.POINTER(C.c_uint8)), ("len", C.c_int32),
                ("n_observable", C.c_int32), ("seconds", C.c_double), ("seconds_kernel", C.c_double)]


GEN_END_FINAL = 1  # generator(end_final=True): only the prefixes that end in a final state


class RepairRequest(C.Structure):
    _fields_ = [("n_streams", C.c_int64), ("offsets", C.POINTER(C.c_int64)), ("values", C.POINTER(C.c_int32)),
                ("weights", C.POINTER(C.c_int32)), ("flags", C.c_int32), ("reserved", C.c_int32)]


class RepairResult(C.Structure):
    _fields_ = [("n_streams", C.c_int64), ("distance", C.POINTER(C.c_int32)), ("values", C.POINTER(C.c_int32)),
                ("end_final", C.POINTER(C.c_uint8)), ("n_changed", C.POINTER(C.c_int32)), ("n_labels", C.c_int64), ("table_bytes", C.c_int64),
                ("n_batches", C.c_int32), ("n_observable", C.c_int32), ("seconds", C.c_double), ("seconds_relax", C.c_double),
                ("seconds_walk", C.c_double), ("seconds_cost", C.c_double)]


REPAIR_END_FINAL = 1          # repair_streams(end_final=True): the repaired stream must end in a final state
REPAIR_MISSING = -2 ** 31     # a value of a row that was not observed


def _repair_weights(weights, n_obs):
    """None or one non-negative int32 per observable variable -> contiguous int32 array or None."""
    import numpy as np
    if weights is None:
        return None
    w = np.asarray(weights, dtype=np.int64)
    if w.shape != (n_obs,):
        raise ValueError(f"weights must have one entry per observable variable ({n_obs})")
    if (np.abs(w) >= 2 ** 31).any():
        raise StcspError(-1, "a weight does not fit an int32")
    return np.ascontiguousarray(w, dtype=np.int32) if n_obs else np.zeros(1, np.int32)


class AlignRequest(C.Structure):
    _fields_ = [("n_streams", C.c_int64), ("offsets", C.POINTER(C.c_int64)), ("values", C.POINTER(C.c_int32)),
                ("weights", C.POINTER(C.c_int32)), ("skip_cost", C.c_int32), ("gap_cost", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


class AlignResult(C.Structure):
    _fields_ = [("n_streams", C.c_int64), ("distance", C.POINTER(C.c_int32)), ("out_offsets", C.POINTER(C.c_int64)),
                ("values", C.POINTER(C.c_int32)), ("op_offsets", C.POINTER(C.c_int64)), ("ops", C.POINTER(C.c_uint8)),
                ("n_changed", C.POINTER(C.c_int32)), ("n_skipped", C.POINTER(C.c_int32)), ("n_inserted", C.POINTER(C.c_int32)),
                ("end_final", C.POINTER(C.c_uint8)), ("n_labels", C.c_int64), ("table_bytes", C.c_int64), ("n_batches", C.c_int32),
                ("n_observable", C.c_int32), ("path_kernel", C.c_int32), ("reserved", C.c_int32), ("seconds", C.c_double),
                ("seconds_levels", C.c_double), ("seconds_walk", C.c_double), ("seconds_cost", C.c_double)]


ALIGN_END_FINAL = 1                      # align_streams(end_final=True): the aligned prefix must end in a final state
ALIGN_MATCH, ALIGN_SKIP, ALIGN_INSERT = 0, 1, 2   # the ops of an alignment: M, D, I
ALIGN_FUSED, ALIGN_GENERAL = 1, 2        # AlignResult.path_kernel


def _align_costs(skip_cost, gap_cost):
    for c in (skip_cost, gap_cost):
        if not -2 ** 31 <= int(c) < 2 ** 31:
            raise StcspError(-1, "a cost does not fit an int32")
    return int(skip_cost), int(gap_cost)


def _align_unpack(n, n_obs, dist, out_off, values, op_off, ops, nchg, nskip, nins, fin):
    """The arrays of an alignment -> (distance int32, list of emitted rows int32 [out_len, n_observable], list of ops uint8,
    n_changed, n_skipped, n_inserted int32, end_final uint8)."""
    rows = [values[int(out_off[i]) * n_obs:int(out_off[i + 1]) * n_obs].reshape(-1, n_obs) for i in range(n)]
    return dist, rows, [ops[int(op_off[i]):int(op_off[i + 1])] for i in range(n)], nchg, nskip, nins, fin


def _repair_unpack(values, offsets, n_obs):
    return [values[int(offsets[i]) * n_obs:int(offsets[i + 1]) * n_obs].reshape(-1, n_obs) for i in range(len(offsets) - 1)]



class InferRequest(C.Structure):
    _fields_ = [("n_streams", C.c_int64), ("offsets", C.POINTER(C.c_int64)), ("values", C.POINTER(C.c_int32)),
                ("ranks", C.POINTER(C.c_uint64)), ("seed", C.c_uint64), ("flags", C.c_int32), ("draws", C.c_int32)]


class InferResult(C.Structure):
    _fields_ = [("n_streams", C.c_int64), ("count", C.POINTER(C.c_double)), ("feasible", C.POINTER(C.c_uint8)),
                ("support_off", C.POINTER(C.c_int64)), ("support_val", C.POINTER(C.c_int32)), ("n_states", C.POINTER(C.c_int32)),
                ("values", C.POINTER(C.c_int32)), ("end_final", C.POINTER(C.c_uint8)), ("n_labels", C.c_int64), ("table_bytes", C.c_int64),
                ("n_batches", C.c_int32), ("n_observable", C.c_int32), ("draws", C.c_int32), ("reserved", C.c_int32),
                ("seconds", C.c_double), ("seconds_match", C.c_double), ("seconds_backward", C.c_double), ("seconds_forward", C.c_double),
                ("seconds_support", C.c_double), ("seconds_walk", C.c_double)]


INFER_END_FINAL = 1           # infer_streams(end_final=True): only the completions that end in a final state
INFER_MISSING = -2 ** 31      # a value of a row that was not observed (== REPAIR_MISSING)


def _infer_ranks(ranks, n, draws):
    """None or [n][draws] ranks -> contiguous uint64 array or None."""
    import numpy as np
    if ranks is None:
        return None
    rk = np.ascontiguousarray(ranks, dtype=np.uint64).reshape(-1)
    if rk.size != n * draws:
        raise ValueError("ranks must have `draws` entries per stream")
    return rk if rk.size else np.zeros(1, np.uint64)


def _infer_unpack(count, soff, sval, nst, dvals, dfin, offsets, n_obs, draws):
    """The flat outputs of an infer call -> (count float64 [n], supports, n_states, draws, end_final): per stream a
    [len][n_obs] list of lists of ints, an int32 array [len + 1], an int32 array [draws, len, n_obs], a uint8 array [draws]."""
    n = len(offsets) - 1
    soff = soff.tolist()
    sval = sval.tolist()
    supports, n_states, out, fin = [], [], [], []
    for i in range(n):
        a, b = int(offsets[i]), int(offsets[i + 1])
        supports.append([[sval[soff[t * n_obs + v]:soff[t * n_obs + v + 1]] for v in range(n_obs)] for t in range(a, b)])
        n_states.append(nst[a + i:b + i + 1].copy())
        out.append(dvals[a * draws * n_obs:b * draws * n_obs].reshape(draws, b - a, n_obs).copy())
        fin.append(dfin[i * draws:(i + 1) * draws].copy())
    return count, supports, n_states, out, fin


class PosteriorRequest(C.Structure):
    _fields_ = [("n_streams", C.c_int64), ("offsets", C.POINTER(C.c_int64)), ("values", C.POINTER(C.c_int32)),
                ("weight_off", C.POINTER(C.c_int64)), ("weight_val", C.POINTER(C.c_int32)), ("weight_w", C.POINTER(C.c_int32)),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class PosteriorResult(C.Structure):
    _fields_ = [("n_streams", C.c_int64), ("mass", C.POINTER(C.c_double)), ("exact", C.POINTER(C.c_uint8)), ("feasible", C.POINTER(C.c_uint8)),
                ("final_mass", C.POINTER(C.c_uint64)), ("marg_off", C.POINTER(C.c_int64)), ("marg_val", C.POINTER(C.c_int32)),
                ("marg_mass", C.POINTER(C.c_uint64)), ("n_labels", C.c_int64), ("table_bytes", C.c_int64), ("n_batches", C.c_int32),
                ("n_observable", C.c_int32), ("seconds", C.c_double), ("seconds_weights", C.c_double), ("seconds_backward", C.c_double),
                ("seconds_forward", C.c_double), ("seconds_bins", C.c_double)]


POSTERIOR_END_FINAL = 1       # posterior_streams(end_final=True): only the completions that end in a final state
POSTERIOR_MISSING = -2 ** 31  # a value of a row that was not observed (== INFER_MISSING)


def _posterior_weights(weights, n_obs):
    """None, or per observable variable a dict value -> weight or None -> the CSR (weight_off int64 [n_obs + 1], weight_val int32,
    weight_w int32) of the contract, or (None, None, None). An item list [(value, weight), ...] is taken in its order, so that a
    request that is out of order can be written down."""
    import numpy as np
    if weights is None:
        return None, None, None
    if len(weights) != n_obs:
        raise ValueError(f"weights must have one entry per observable variable ({n_obs})")
    off, val, w = [0], [], []
    for d in weights:
        items = [] if d is None else sorted(d.items()) if isinstance(d, dict) else list(d)
        for value, weight in items:
            if not (-2 ** 31 <= int(value) < 2 ** 31 and -2 ** 31 <= int(weight) < 2 ** 31):
                raise StcspError(-1, "a weighted value or a weight does not fit an int32")
            val.append(int(value))
            w.append(int(weight))
        off.append(len(val))
    return np.array(off, np.int64), np.array(val + [0], np.int32), np.array(w + [0], np.int32)


def _posterior_unpack(mass, exact, fmass, moff, mval, mmass, offsets, n_obs):
    """The flat outputs of a posterior call -> (mass float64 [n], exact uint8 [n], final_mass list of ints, marginals):
    marginals[i][t][v] is the list of (value, mass) pairs of Python ints, in value order."""
    n = len(offsets) - 1
    moff = moff.tolist()
    pairs = list(zip(mval.tolist(), mmass.tolist()))
    marginals = []
    for i in range(n):
        a, b = int(offsets[i]), int(offsets[i + 1])
        marginals.append([[pairs[moff[t * n_obs + v]:moff[t * n_obs + v + 1]] for v in range(n_obs)] for t in range(a, b)])
    return mass, exact, [int(x) for x in fmass.tolist()], marginals


class ObserverOptions(C.Structure):
    _fields_ = [("max_states", C.c_int64), ("reserved", C.c_int32 * 2)]


class ObserverResult(C.Structure):
    _fields_ = [("n_states", C.c_int64), ("n_edges", C.c_int64), ("member_off", C.POINTER(C.c_int64)), ("member", C.POINTER(C.c_int32)),
                ("state_final", C.POINTER(C.c_uint8)), ("edge_src", C.POINTER(C.c_int32)), ("edge_dst", C.POINTER(C.c_int32)),
                ("edge_values", C.POINTER(C.c_int32)), ("n_labels", C.c_int64), ("max_set", C.c_int64), ("table_bytes", C.c_int64),
                ("n_observable", C.c_int32), ("levels", C.c_int32), ("seconds", C.c_double), ("seconds_build", C.c_double),
                ("seconds_items", C.c_double), ("seconds_intern", C.c_double), ("seconds_commit", C.c_double)]


OBSERVER_SCALARS = ("n_states", "n_edges", "n_labels", "max_set", "table_bytes", "n_observable", "levels", "seconds", "seconds_build",
                    "seconds_items", "seconds_intern", "seconds_commit")


def _copy_array(ptr, n, dtype):
    """A copy of the n elements at a ctypes pointer as a numpy array; n == 0: an empty one (the pointer is not read)."""
    import numpy as np
    return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, dtype)


def _observable_mask(n_vars, observable):
    """None (the default mask), "all", or a sequence of n_vars flags -> uint8 array or None."""
    import numpy as np
    if observable is None:
        return None
    m = np.ones(n_vars, dtype=np.uint8) if isinstance(observable, str) and observable == "all" else np.ascontiguousarray(observable, dtype=np.uint8)
    if m.shape != (n_vars,):
        raise ValueError(f"observable must have one flag per variable ({n_vars})")
    return m


def _stream_head(values, offsets):
    """The (n_streams, offsets, values) head of MonitorStreams, RepairRequest, InferRequest and PosteriorRequest, from pack_streams()."""
    return len(offsets) - 1, offsets.ctypes.data_as(C.POINTER(C.c_int64)), values.ctypes.data_as(C.POINTER(C.c_int32)) if values.size else None


def _observer_unpack(res):
    """An ObserverResult -> dict: copies of its arrays as numpy arrays (member_off int64 [n_states + 1], member int32, state_final
    uint8 [n_states], edge_src / edge_dst int32 [n_edges], edge_values int32 [n_edges, n_observable]) and its scalars."""
    import numpy as np
    ns, ne, no = res.n_states, res.n_edges, res.n_observable
    arr = _copy_array
    d = {k: getattr(res, k) for k in OBSERVER_SCALARS}
    d["member_off"] = arr(res.member_off, ns + 1, np.int64)
    d["member"] = arr(res.member, int(d["member_off"][-1]), np.int32)
    d["state_final"] = arr(res.state_final, ns, np.uint8)
    d["edge_src"] = arr(res.edge_src, ne, np.int32)
    d["edge_dst"] = arr(res.edge_dst, ne, np.int32)
    d["edge_values"] = arr(res.edge_values, ne * no, np.int32).reshape(ne, no)
    return d


def _observer_pack(obs):
    """The dict of _observer_unpack() -> (ObserverResult, the arrays it points into)."""
    import numpy as np
    keep = {k: np.ascontiguousarray(obs[k], dtype=t) for k, t in (("member_off", np.int64), ("member", np.int32), ("state_final", np.uint8),
                                                                     ("edge_src", np.int32), ("edge_dst", np.int32), ("edge_values", np.int32))}
    for k in list(keep):
        if keep[k].size == 0:
            keep[k] = np.zeros(1, keep[k].dtype)
    res = ObserverResult()
    res.n_states, res.n_edges, res.n_observable = int(obs["n_states"]), int(obs["n_edges"]), int(obs["n_observable"])
    res.member_off = keep["member_off"].ctypes.data_as(C.POINTER(C.c_int64))
    res.member = keep["member"].ctypes.data_as(C.POINTER(C.c_int32))
    res.state_final = keep["state_final"].ctypes.data_as(C.POINTER(C.c_uint8))
    res.edge_src = keep["edge_src"].ctypes.data_as(C.POINTER(C.c_int32))
    res.edge_dst = keep["edge_dst"].ctypes.data_as(C.POINTER(C.c_int32))
    res.edge_values = keep["edge_values"].ctypes.data_as(C.POINTER(C.c_int32))
    return res, keep


class CompareRequest(C.Structure):
    _fields_ = [("right", C.POINTER(ObserverResult)), ("max_pairs", C.c_int64), ("reserved", C.c_int32 * 2)]


class CompareResult(C.Structure):
    _fields_ = [("n_pairs", C.c_int64), ("n_pair_edges", C.c_int64), ("witness_off", C.c_int64 * 5), ("witness_values", C.POINTER(C.c_int32)),
                ("witness_len", C.c_int32 * 4), ("witness_left", C.c_int32 * 4), ("witness_right", C.c_int32 * 4), ("table_bytes", C.c_int64),
                ("n_observable", C.c_int32), ("levels", C.c_int32), ("seconds", C.c_double), ("seconds_expand", C.c_double),
                ("seconds_number", C.c_double)]


COMPARE_SCALARS = ("n_pairs", "n_pair_edges", "table_bytes", "n_observable", "levels", "seconds", "seconds_expand", "seconds_number")


def _compare_unpack(res):
    """A CompareResult -> dict: its scalars, witness_off int64 [5] (in rows), witness_len / witness_left / witness_right int32 [4]
    and witness_values int32 [witness_off[4], n_observable], all copies."""
    import numpy as np
    d = {k: getattr(res, k) for k in COMPARE_SCALARS}
    d["witness_off"] = np.array(res.witness_off[:], np.int64)
    for k in ("witness_len", "witness_left", "witness_right"):
        d[k] = np.array(getattr(res, k)[:], np.int32)
    rows, no = int(d["witness_off"][4]), res.n_observable
    d["witness_values"] = (np.ctypeslib.as_array(res.witness_values, shape=(rows * no,)).copy() if rows * no else np.zeros(0, np.int32)).reshape(rows, no)
    return d


def compare_observers(left, right, max_pairs=0):
    """The comparison of two observers (the dicts of Engine.observer() / Automaton.observer(), or any deterministic automata in that
    form; `right` with its columns in the order of `left`) by the host twin of Engine.compare(): the product of the two, the four
    inclusions P(L) in P(R), P(R) in P(L), F(L) in F(R), F(R) in F(L) and their shortest witnesses. Returns the dict of
    _compare_unpack(); StcspError -1 for a malformed operand, -4 beyond max_pairs (0: the default). Contract: include/stcsp_engine.h,
    stcsp_engine_compare."""
    lib = host_lib()
    lres, lkeep = _observer_pack(left)
    rres, rkeep = _observer_pack(right)
    h = C.c_void_p()
    rc = lib.stcsp_compare_observers(C.byref(lres), C.byref(rres), max_pairs, C.byref(h))
    del lkeep, rkeep
    if rc != 0:
        raise StcspError(rc, "compare_observers failed: more pairs than max_pairs" if rc == -4 else "compare_observers failed: a malformed operand")
    try:
        return _compare_unpack(lib.stcsp_comparison_get(h).contents)
    finally:
        lib.stcsp_comparison_free(h)


class ComponentsOptions(C.Structure):
    _fields_ = [("max_lassos", C.c_int64), ("flags", C.c_int32), ("reserved", C.c_int32)]


class ComponentsResult(C.Structure):
    _fields_ = [("n_states", C.c_int64), ("n_components", C.c_int64), ("n_cyclic", C.c_int64), ("n_accepting", C.c_int64),
                ("n_bottom", C.c_int64), ("n_omega", C.c_int64), ("state_component", C.POINTER(C.c_int32)),
                ("state_omega", C.POINTER(C.c_uint8)), ("comp_size", C.POINTER(C.c_int32)), ("comp_depth", C.POINTER(C.c_int32)),
                ("comp_flags", C.POINTER(C.c_int32)), ("n_lassos", C.c_int64), ("lasso_component", C.POINTER(C.c_int32)),
                ("lasso_off", C.POINTER(C.c_int64)), ("lasso_stem_len", C.POINTER(C.c_int32)), ("lasso_values", C.POINTER(C.c_int32)),
                ("n_vars", C.c_int32), ("root_omega", C.c_int32), ("rounds", C.c_int32 * 3), ("reserved", C.c_int32),
                ("seconds", C.c_double), ("seconds_kernels", C.c_double)]


SCC_LASSO_BOTTOM, SCC_NO_TRIM = 1, 2                       # ComponentsOptions.flags
SCC_CYCLIC, SCC_FINAL, SCC_BOTTOM, SCC_ACCEPTING = 1, 2, 4, 8  # comp_flags
COMPONENTS_SCALARS = ("n_states", "n_components", "n_cyclic", "n_accepting", "n_bottom", "n_omega", "n_lassos", "n_vars", "root_omega",
                      "seconds", "seconds_kernels")


def _components_options(lassos, no_trim):
    """lassos: 0 (none), "all", "bottom" (all of the bottom accepting components) or a positive count."""
    if lassos not in ("all", "bottom") and (not isinstance(lassos, int) or lassos < 0):
        raise ValueError('lassos is 0, "bottom", "all" or a positive count')
    return ComponentsOptions(-1 if lassos in ("all", "bottom") else lassos, (SCC_LASSO_BOTTOM if lassos == "bottom" else 0) | (SCC_NO_TRIM if no_trim else 0))


def _components_unpack(res, n_states):
    """A ComponentsResult -> dict: its scalars, rounds int32 [3], copies of state_component int32 / state_omega uint8 [n_states of the
    Result], comp_size / comp_depth / comp_flags int32 [n_components], and "lassos": a list of (component, stem, loop), stem and loop
    int32 arrays of full label rows [steps, n_vars]."""
    import numpy as np
    arr = _copy_array
    d = {k: getattr(res, k) for k in COMPONENTS_SCALARS}
    d["rounds"] = np.array(res.rounds[:], np.int32)
    d["state_component"] = arr(res.state_component, n_states, np.int32)
    d["state_omega"] = arr(res.state_omega, n_states, np.uint8)
    for k in ("comp_size", "comp_depth", "comp_flags"):
        d[k] = arr(getattr(res, k), res.n_components, np.int32)
    nl, nv = res.n_lassos, res.n_vars
    off = arr(res.lasso_off, nl + 1, np.int64) if nl else np.zeros(1, np.int64)
    comp, stem = arr(res.lasso_component, nl, np.int32), arr(res.lasso_stem_len, nl, np.int32)
    values = arr(res.lasso_values, int(off[-1]) * nv, np.int32).reshape(int(off[-1]), nv)
    d["lassos"] = [(int(comp[i]), values[off[i]:off[i] + stem[i]].copy(), values[off[i] + stem[i]:off[i + 1]].copy()) for i in range(nl)]
    return d


class OptimiseRequest(C.Structure):
    _fields_ = [("weights", C.POINTER(C.c_int32)), ("lengths", C.POINTER(C.c_int32)), ("horizon", C.c_int32), ("n_lengths", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class OptimiseResult(C.Structure):
    _fields_ = [("n_states", C.c_int64), ("best", C.POINTER(C.c_int64)), ("state_best", C.POINTER(C.c_int64)), ("n_witnesses", C.c_int64),
                ("witness_off", C.POINTER(C.c_int64)), ("witness_values", C.POINTER(C.c_int32)), ("witness_states", C.POINTER(C.c_int32)),
                ("n_components", C.c_int64), ("state_component", C.POINTER(C.c_int32)), ("comp_mean_num", C.POINTER(C.c_int64)),
                ("comp_mean_den", C.POINTER(C.c_int64)), ("omega_mean_num", C.c_int64), ("omega_mean_den", C.c_int64),
                ("omega_component", C.c_int32), ("n_vars", C.c_int32), ("horizon", C.c_int32), ("largest_cyclic", C.c_int32),
                ("rounds", C.c_int32 * 2), ("seconds", C.c_double), ("seconds_kernels", C.c_double)]


OPT_MAXIMISE, OPT_END_FINAL, OPT_MEAN, OPT_STATE_BEST = 1, 2, 4, 8  # OptimiseRequest.flags
OPT_NONE = 2**63 - 1                                                # best / state_best: no such path


def _optimise_request(weights, names, horizon, lengths, maximise, end_final, mean, state_best):
    """(OptimiseRequest, the arrays it points into). weights: a dict name -> int (the other variables 0) or one int per variable."""
    import numpy as np
    if isinstance(weights, dict):
        unknown = sorted(set(weights) - set(names))
        if unknown:
            raise ValueError(f"no variable named {unknown[0]!r}")
        weights = [weights.get(n, 0) for n in names]
    w = np.ascontiguousarray(weights, dtype=np.int32)
    if w.shape != (len(names),):
        raise ValueError(f"weights must have one entry per variable ({len(names)})")
    ln = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
    rq = OptimiseRequest(w.ctypes.data_as(C.POINTER(C.c_int32)), ln.ctypes.data_as(C.POINTER(C.c_int32)) if ln.size else None, horizon, ln.size,
                         (OPT_MAXIMISE if maximise else 0) | (OPT_END_FINAL if end_final else 0) | (OPT_MEAN if mean else 0) |
                         (OPT_STATE_BEST if state_best else 0), 0)
    return rq, (w, ln)


def _optimise_unpack(res, lengths, n_states):
    """An OptimiseResult -> dict: n_states, n_components, n_vars, horizon, largest_cyclic, seconds, seconds_kernels; rounds int32 [2];
    best int64 [horizon + 1] (OPT_NONE = no such prefix); state_best int64 [n_states of the Result] or None; "witnesses": a list of
    (length, rows int32 [steps, n_vars], states int32 [steps]: the state every step enters), empty arrays where best[length] is
    OPT_NONE; with mean: state_component int32 [n_states of the Result], "comp_mean": a list of (num, den) per component ((0, 0) when it
    is not cyclic), "omega_mean": (num, den) ((0, 0): no infinite solution) and omega_component; else None, [], (0, 0) and -1."""
    import numpy as np
    arr = _copy_array
    d = {k: getattr(res, k) for k in ("n_states", "n_components", "n_vars", "horizon", "largest_cyclic", "omega_component", "seconds", "seconds_kernels")}
    d["rounds"] = np.array(res.rounds[:], np.int32)
    d["best"] = arr(res.best, res.horizon + 1, np.int64)
    d["state_best"] = arr(res.state_best, n_states, np.int64) if res.state_best else None
    nw, nv = res.n_witnesses, res.n_vars
    off = arr(res.witness_off, nw + 1, np.int64) if nw else np.zeros(1, np.int64)
    values = arr(res.witness_values, int(off[-1]) * nv, np.int32).reshape(int(off[-1]), nv)
    states = arr(res.witness_states, int(off[-1]), np.int32)
    d["witnesses"] = [(int(lengths[i]), values[off[i]:off[i + 1]].copy(), states[off[i]:off[i + 1]].copy()) for i in range(nw)]
    d["state_component"] = arr(res.state_component, n_states, np.int32) if res.state_component else None
    num, den = arr(res.comp_mean_num, res.n_components, np.int64), arr(res.comp_mean_den, res.n_components, np.int64)
    d["comp_mean"] = [(int(p), int(q)) for p, q in zip(num, den)]
    d["omega_mean"] = (int(res.omega_mean_num), int(res.omega_mean_den))
    return d


F_KEEP_RAW_EDGES = 1
F_NO_EXPORT = 2
F_PROFILE = 4
F_STEPPED = 8
F_INTERVAL_DOMAINS = 16  # every variable held as an interval (any width in [INT_MIN, INT_MAX]); include/stcsp_engine.h
GID_SHIFT = 40

class CtlRequest(C.Structure):
    _fields_ = [("program", C.POINTER(C.c_int32)), ("n_words", C.c_int32), ("flags", C.c_int32)]


class CtlResult(C.Structure):
    _fields_ = [("n_worlds", C.c_int64), ("n_initial", C.c_int64), ("n_initial_sat", C.c_int64), ("n_edges", C.c_int64),
                ("edge_world", C.POINTER(C.c_uint8)), ("edge_sat", C.POINTER(C.c_uint8)), ("witness_values", C.POINTER(C.c_int32)),
                ("witness_kind", C.c_int32), ("witness_len", C.c_int32), ("n_vars", C.c_int32), ("rounds", C.c_int32 * 3),
                ("seconds", C.c_double), ("seconds_kernels", C.c_double)]


# the tokens of a CTL program and the comparisons of its atoms (include/stcsp_engine.h, STCSP_CTL_*)
CTL_TRUE, CTL_FALSE, CTL_CMP_CONST, CTL_CMP_VAR = 1, 2, 3, 4
CTL_NOT, CTL_AND, CTL_OR, CTL_IMPLIES = 10, 11, 12, 13
CTL_EX, CTL_EF, CTL_EG, CTL_EU, CTL_AX, CTL_AF, CTL_AG, CTL_AU = 20, 21, 22, 23, 24, 25, 26, 27
CTL_OPS = ("==", "!=", "<", "<=", ">", ">=")  # op k of an atom
CTL_WITNESS = 1
CTL_KINDS = ("none", "witness", "counterexample")
CTL_MAX_NODES, CTL_MAX_SLOTS = 256, 16


class CtlSyntaxError(ValueError):
    """A formula stcsp_ctl_parse() refuses: .position is the 0-based offset into the text, .message what is wrong there."""

    def __init__(self, position, message):
        super().__init__(f"{position}: {message}")
        self.position, self.message = position, message


def _ctl_parse_names(names, text):
    import numpy as np
    lib = host_lib()
    enc = [n.encode() for n in names]
    arr = (C.c_char_p * max(len(enc), 1))(*enc)
    p = Problem()
    p.n_vars = len(enc)
    p.var_names = C.cast(arr, C.POINTER(C.c_char_p))
    words, n, pos = C.POINTER(C.c_int32)(), C.c_int32(), C.c_int32()
    msg = C.create_string_buffer(256)
    rc = lib.stcsp_ctl_parse(text.encode(), C.byref(p), C.byref(words), C.byref(n), C.byref(pos), msg, len(msg))
    if rc == -1:
        raise CtlSyntaxError(pos.value, msg.value.decode())
    if rc != 0:
        raise StcspError(rc, "ctl_parse failed")
    try:
        return _copy_array(words, n.value, np.int32)
    finally:
        lib.stcsp_host_free(words)


def ctl_parse(model, text):
    """Formula text -> the postfix program of Engine.ctl() / Automaton.ctl(), an int32 array (grammar: include/stcsp_host.h,
    stcsp_ctl_parse). `model` is a Model, or a list of variable names. CtlSyntaxError with a position and a message for a
    formula that does not parse or names an unknown variable."""
    return _ctl_parse_names(model.var_names if isinstance(model, Model) else list(model), text)


def _ctl_request(formula, names, witness):
    import numpy as np
    prog = _ctl_parse_names(names, formula) if isinstance(formula, str) else np.ascontiguousarray(formula, dtype=np.int32).reshape(-1)
    rq = CtlRequest(prog.ctypes.data_as(C.POINTER(C.c_int32)), prog.size, CTL_WITNESS if witness else 0)
    return rq, prog


def _ctl_unpack(res):
    """A CtlResult -> dict: n_worlds, n_initial, n_initial_sat, n_vars, seconds, seconds_kernels; "holds" (n_initial_sat == n_initial),
    "possible" (n_initial_sat > 0), "vacuous" (n_initial == 0); rounds int32 [3]; copies of edge_world / edge_sat uint8 [n_edges of the
    Result]; "witness": (kind, rows) with kind "none", "witness" or "counterexample" and rows an int32 array of full rows [len, n_vars]."""
    import numpy as np
    d = {k: getattr(res, k) for k in ("n_worlds", "n_initial", "n_initial_sat", "n_vars", "seconds", "seconds_kernels")}
    d["holds"], d["possible"], d["vacuous"] = res.n_initial_sat == res.n_initial, res.n_initial_sat > 0, res.n_initial == 0
    d["rounds"] = np.array(res.rounds[:], np.int32)
    d["edge_world"] = _copy_array(res.edge_world, res.n_edges, np.uint8)
    d["edge_sat"] = _copy_array(res.edge_sat, res.n_edges, np.uint8)
    rows = _copy_array(res.witness_values, res.witness_len * res.n_vars, np.int32).reshape(res.witness_len, res.n_vars)
    d["witness"] = (CTL_KINDS[res.witness_kind], rows)
    return d


ENGINE_SYMBOLS = [
    "stcsp_engine_create", "stcsp_engine_solve", "stcsp_engine_export", "stcsp_engine_destroy",
    "stcsp_engine_last_error", "stcsp_engine_begin", "stcsp_engine_expand_local",
    "stcsp_engine_candidate_bytes", "stcsp_engine_outbox", "stcsp_engine_commit", "stcsp_engine_finish",
    "stcsp_engine_counters", "stcsp_engine_sets_blob", "stcsp_engine_sets_import", "stcsp_engine_postprocess",
    "stcsp_engine_propagate", "stcsp_engine_set_expand_budget", "stcsp_engine_node_bytes", "stcsp_engine_donate",
    "stcsp_engine_adopt", "stcsp_engine_expand_variant", "stcsp_engine_kernel_choice", "stcsp_engine_quotient",
    "stcsp_engine_monitor_build", "stcsp_engine_monitor_check", "stcsp_engine_generator_build", "stcsp_engine_generate",
    "stcsp_engine_repair", "stcsp_engine_align", "stcsp_engine_infer", "stcsp_engine_posterior", "stcsp_engine_observer", "stcsp_engine_compare",
    "stcsp_engine_components", "stcsp_engine_optimise", "stcsp_engine_ctl",
]
# include/stcsp_sharded.h: the superstep loop + in-process transport (libstcsp_hip.so), the RCCL transport (libstcsp_rccl.so)
SHARDED_SYMBOLS_HIP = ["stcsp_engine_solve_sharded", "stcsp_local_group_create", "stcsp_local_group_transport", "stcsp_local_group_destroy"]
SHARDED_SYMBOLS_RCCL = ["stcsp_rccl_unique_id", "stcsp_transport_rccl_create", "stcsp_transport_rccl_destroy"]
HOST_SYMBOLS = [
    "stcsp_model_load_file", "stcsp_model_load_text", "stcsp_model_problem", "stcsp_model_free",
    "stcsp_host_last_error", "stcsp_model_constraint_string",
    "stcsp_automaton_build", "stcsp_automaton_free", "stcsp_automaton_traverse",
    "stcsp_automaton_adversarial", "stcsp_automaton_adversarial2", "stcsp_automaton_renumber",
    "stcsp_automaton_import_flags", "stcsp_automaton_flags", "stcsp_automaton_order_by_label", "stcsp_automaton_write_binary", "stcsp_automaton_read_binary",
    "stcsp_automaton_write_dot", "stcsp_automaton_canonical", "stcsp_automaton_num_states",
    "stcsp_automaton_num_live_states", "stcsp_automaton_num_live_edges",
    "stcsp_merge_shards", "stcsp_merged_result", "stcsp_merged_free", "stcsp_host_free",
    "stcsp_automaton_bisimulation", "stcsp_automaton_set_observable", "stcsp_automaton_quotient",
    "stcsp_automaton_check_streams", "stcsp_automaton_num_observable", "stcsp_automaton_generate", "stcsp_automaton_count_streams",
    "stcsp_automaton_repair_streams", "stcsp_automaton_align_streams", "stcsp_automaton_infer_streams", "stcsp_automaton_posterior_streams",
    "stcsp_automaton_observer", "stcsp_observer_get", "stcsp_observer_free", "stcsp_automaton_from_observer",
    "stcsp_compare_observers", "stcsp_comparison_get", "stcsp_comparison_free", "stcsp_automaton_num_vars", "stcsp_automaton_var_name",
    "stcsp_automaton_components", "stcsp_components_get", "stcsp_components_free",
    "stcsp_automaton_optimise", "stcsp_optimise_get", "stcsp_optimise_free",
    "stcsp_ctl_parse", "stcsp_automaton_ctl", "stcsp_ctl_get", "stcsp_ctl_free",
]


class StcspError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"stcsp error {code}: {msg}")
        self.code = code


def engine_source_sha() -> str:
    """sha256 (first 16 hex digits) over the sources libstcsp_hip.so is built from: ties a committed PMC figure to the
    engine it was measured on (bench.py quotes profiles/*_traffic.json only when this matches)."""
    h = hashlib.sha256()
    for f in sorted(list(CSRC.glob("*.hip")) + list(CSRC.glob("dev_*.hpp")) + [CSRC / "device_types.hpp", CSRC / "cset.cpp", CSRC / "cset.hpp", CSRC / "sharded_native.hpp", CSRC / "automaton.hpp", CSRC / "hip_host.hpp"]):
        h.update(f.name.encode())
        h.update(f.read_bytes())
    return h.hexdigest()[:16]


# ------------------------------------------------------------------ library loading / building
def build(verbose: bool = False) -> None:
    """Compile every native library in-tree (hipcc cross-compiles gfx950 without a GPU)."""
    cmd = ["make", "-C", str(CSRC), "all"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout, r.stderr)
    if r.returncode != 0:
        raise RuntimeError("native build failed")
    global _host, _hip
    _host = _hip = None


_host = None
_hip = None


def host_lib() -> C.CDLL:
    global _host
    if _host is None:
        path = CSRC / "libstcsp_host.so"
        if not path.exists():
            raise RuntimeError(f"{path} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(str(path))
        lib.stcsp_model_load_file.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        lib.stcsp_model_load_text.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        lib.stcsp_model_problem.argtypes = [C.c_void_p]
        lib.stcsp_model_problem.restype = C.POINTER(Problem)
        lib.stcsp_model_free.argtypes = [C.c_void_p]
        lib.stcsp_host_last_error.restype = C.c_char_p
        lib.stcsp_model_constraint_string.argtypes = [C.c_void_p, C.c_int]
        lib.stcsp_model_constraint_string.restype = C.c_void_p
        lib.stcsp_automaton_build.argtypes = [C.POINTER(Problem), C.POINTER(Result), C.POINTER(C.c_void_p)]
        lib.stcsp_automaton_free.argtypes = [C.c_void_p]
        lib.stcsp_automaton_traverse.argtypes = [C.c_void_p]
        lib.stcsp_automaton_adversarial.argtypes = [C.c_void_p, C.c_int]
        lib.stcsp_automaton_adversarial2.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.stcsp_automaton_renumber.argtypes = [C.c_void_p]
        lib.stcsp_automaton_order_by_label.argtypes = [C.c_void_p]
        lib.stcsp_automaton_import_flags.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.stcsp_automaton_flags.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.stcsp_automaton_write_dot.argtypes = [C.c_void_p, C.c_char_p]
        lib.stcsp_automaton_write_binary.argtypes = [C.c_void_p, C.c_char_p]
        lib.stcsp_automaton_read_binary.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        lib.stcsp_automaton_canonical.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        lib.stcsp_automaton_canonical.restype = C.c_void_p
        for f in ("stcsp_automaton_num_states", "stcsp_automaton_num_live_states", "stcsp_automaton_num_live_edges"):
            getattr(lib, f).argtypes = [C.c_void_p]
            getattr(lib, f).restype = C.c_int64
        lib.stcsp_automaton_bisimulation.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        lib.stcsp_automaton_set_observable.argtypes = [C.c_void_p, C.c_void_p]
        lib.stcsp_automaton_quotient.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
        lib.stcsp_automaton_check_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        lib.stcsp_automaton_num_observable.argtypes = [C.c_void_p, C.c_void_p]
        lib.stcsp_automaton_generate.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_uint64, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
        lib.stcsp_automaton_count_streams.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        lib.stcsp_automaton_repair_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.stcsp_automaton_align_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_void_p),
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.stcsp_automaton_infer_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                      C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.stcsp_automaton_posterior_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                                          C.POINTER(C.c_void_p)]
        lib.stcsp_automaton_observer.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
        lib.stcsp_observer_get.argtypes = [C.c_void_p]
        lib.stcsp_observer_get.restype = C.POINTER(ObserverResult)
        lib.stcsp_observer_free.argtypes = [C.c_void_p]
        lib.stcsp_automaton_from_observer.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(ObserverResult), C.POINTER(C.c_void_p)]
        lib.stcsp_compare_observers.argtypes = [C.POINTER(ObserverResult), C.POINTER(ObserverResult), C.c_int64, C.POINTER(C.c_void_p)]
        lib.stcsp_comparison_get.argtypes = [C.c_void_p]
        lib.stcsp_comparison_get.restype = C.POINTER(CompareResult)
        lib.stcsp_comparison_free.argtypes = [C.c_void_p]
        lib.stcsp_automaton_components.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]
        lib.stcsp_components_get.argtypes = [C.c_void_p]
        lib.stcsp_components_get.restype = C.POINTER(ComponentsResult)
        lib.stcsp_components_free.argtypes = [C.c_void_p]
        lib.stcsp_automaton_optimise.argtypes = [C.c_void_p, C.POINTER(OptimiseRequest), C.POINTER(C.c_void_p)]
        lib.stcsp_optimise_get.argtypes = [C.c_void_p]
        lib.stcsp_optimise_get.restype = C.POINTER(OptimiseResult)
        lib.stcsp_optimise_free.argtypes = [C.c_void_p]
        lib.stcsp_ctl_parse.argtypes = [C.c_char_p, C.POINTER(Problem), C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.c_char_p, C.c_size_t]
        lib.stcsp_automaton_ctl.argtypes = [C.c_void_p, C.POINTER(CtlRequest), C.POINTER(C.c_void_p)]
        lib.stcsp_ctl_get.argtypes = [C.c_void_p]
        lib.stcsp_ctl_get.restype = C.POINTER(CtlResult)
        lib.stcsp_ctl_free.argtypes = [C.c_void_p]
        lib.stcsp_automaton_num_vars.argtypes = [C.c_void_p]
        lib.stcsp_automaton_var_name.argtypes = [C.c_void_p, C.c_int]
        lib.stcsp_automaton_var_name.restype = C.c_char_p
        lib.stcsp_merge_shards.argtypes = [C.POINTER(C.POINTER(Result)), C.c_int, C.POINTER(C.c_void_p)]
        lib.stcsp_merged_result.argtypes = [C.c_void_p]
        lib.stcsp_merged_result.restype = C.POINTER(Result)
        lib.stcsp_merged_free.argtypes = [C.c_void_p]
        lib.stcsp_host_free.argtypes = [C.c_void_p]
        _host = lib
    return _host


def bind_engine_api(lib: C.CDLL, prefix: str = "stcsp_engine") -> None:
    """Attach argtypes to an engine-shaped API (the HIP engine, or -- in tests only -- an
    oracle exposing the same shape under another prefix)."""
    g = lambda n: getattr(lib, f"{prefix}_{n}")  # noqa: E731
    g("create").argtypes = [C.POINTER(Problem), C.POINTER(Options), C.POINTER(C.c_void_p)]
    g("solve").argtypes = [C.c_void_p, C.POINTER(Result)]
    g("destroy").argtypes = [C.c_void_p]
    g("destroy").restype = None
    for n in ("export",):
        if hasattr(lib, f"{prefix}_{n}"):
            g(n).argtypes = [C.c_void_p, C.POINTER(Result)]
    if hasattr(lib, f"{prefix}_last_error"):
        g("last_error").argtypes = [C.c_void_p]
        g("last_error").restype = C.c_char_p
    if hasattr(lib, f"{prefix}_begin"):
        g("begin").argtypes = [C.c_void_p]
        g("expand_local").argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        g("candidate_bytes").argtypes = [C.c_void_p]
        g("outbox").argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        g("commit").argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        g("finish").argtypes = [C.c_void_p]
    if hasattr(lib, f"{prefix}_donate"):
        g("set_expand_budget").argtypes = [C.c_void_p, C.c_int64, C.c_int64]
        g("node_bytes").argtypes = [C.c_void_p]
        g("donate").argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        g("adopt").argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    if hasattr(lib, f"{prefix}_counters"):
        g("counters").argtypes = [C.c_void_p, C.POINTER(Counters)]
    if hasattr(lib, f"{prefix}_expand_variant"):
        g("expand_variant").argtypes = [C.c_void_p]
        g("kernel_choice").argtypes = [C.c_void_p, C.POINTER(KernelChoice)]
        g("sets_blob").argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_int64)]
        g("sets_import").argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int64]
    if hasattr(lib, f"{prefix}_postprocess"):
        g("postprocess").argtypes = [C.c_void_p, C.POINTER(PostOptions), C.POINTER(PostResult)]
    if hasattr(lib, f"{prefix}_quotient"):
        g("quotient").argtypes = [C.c_void_p, C.POINTER(QuotientOptions), C.POINTER(QuotientResult)]
    if hasattr(lib, f"{prefix}_monitor_build"):
        g("monitor_build").argtypes = [C.c_void_p, C.POINTER(MonitorOptions), C.POINTER(MonitorInfo)]
        g("monitor_check").argtypes = [C.c_void_p, C.POINTER(MonitorStreams), C.POINTER(MonitorResult)]
    if hasattr(lib, f"{prefix}_generator_build"):
        g("generator_build").argtypes = [C.c_void_p, C.POINTER(GeneratorOptions), C.POINTER(GeneratorInfo)]
        g("generate").argtypes = [C.c_void_p, C.POINTER(GenerateRequest), C.POINTER(GenerateResult)]
    if hasattr(lib, f"{prefix}_repair"):
        g("repair").argtypes = [C.c_void_p, C.POINTER(RepairRequest), C.POINTER(RepairResult)]
    if hasattr(lib, f"{prefix}_align"):
        g("align").argtypes = [C.c_void_p, C.POINTER(AlignRequest), C.POINTER(AlignResult)]
    if hasattr(lib, f"{prefix}_infer"):
        g("infer").argtypes = [C.c_void_p, C.POINTER(InferRequest), C.POINTER(InferResult)]
    if hasattr(lib, f"{prefix}_posterior"):
        g("posterior").argtypes = [C.c_void_p, C.POINTER(PosteriorRequest), C.POINTER(PosteriorResult)]
    if hasattr(lib, f"{prefix}_observer"):
        g("observer").argtypes = [C.c_void_p, C.POINTER(ObserverOptions), C.POINTER(ObserverResult)]
    if hasattr(lib, f"{prefix}_compare"):
        g("compare").argtypes = [C.c_void_p, C.POINTER(CompareRequest), C.POINTER(CompareResult)]
    if hasattr(lib, f"{prefix}_components"):
        g("components").argtypes = [C.c_void_p, C.POINTER(ComponentsOptions), C.POINTER(ComponentsResult)]
    if hasattr(lib, f"{prefix}_optimise"):
        g("optimise").argtypes = [C.c_void_p, C.POINTER(OptimiseRequest), C.POINTER(OptimiseResult)]
    if hasattr(lib, f"{prefix}_ctl"):
        g("ctl").argtypes = [C.c_void_p, C.POINTER(CtlRequest), C.POINTER(CtlResult)]
    if hasattr(lib, f"{prefix}_propagate"):
        g("propagate").argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(C.c_uint32), C.c_int64, C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int64)]


def hip_lib() -> C.CDLL:
    """The HIP engine. Fails loudly when the extension is missing or cannot be loaded."""
    global _hip
    if _hip is None:
        path = Path(os.environ.get("STCSP_HIP_LIB", CSRC / "libstcsp_hip.so"))  # override: tuning builds
        if not path.exists():
            raise RuntimeError(f"HIP engine library {path} is missing -- build it (make -C {CSRC}); "
                               "there is no CPU fallback")
        lib = C.CDLL(str(path))
        bind_engine_api(lib)
        _hip = lib
    return _hip


# ------------------------------------------------------------------ model (front end)
class Model:
    """A built stCSP model = what solverSolve() receives (reference src/solver.h:22-49)."""

    def __init__(self, text: str | None = None, path: str | None = None, prefix_k: int = 2):
        lib = host_lib()
        h = C.c_void_p()
        if path is not None:
            rc = lib.stcsp_model_load_file(os.fsencode(path), prefix_k, C.byref(h))
        else:
            rc = lib.stcsp_model_load_text(text.encode(), prefix_k, C.byref(h))
        if rc != 0:
            raise StcspError(rc, lib.stcsp_host_last_error().decode())
        self._h = h
        self.problem = lib.stcsp_model_problem(h)

    @classmethod
    def from_name(cls, name: str, prefix_k: int = 2) -> "Model":
        return cls(text=instances.by_name(name), prefix_k=prefix_k)

    @property
    def n_vars(self):
        return self.problem.contents.n_vars

    @property
    def n_constraints(self):
        return self.problem.contents.n_constraints

    @property
    def var_names(self):
        p = self.problem.contents
        return [p.var_names[i].decode() for i in range(p.n_vars)]

    def var_bounds(self):
        p = self.problem.contents
        return [(p.var_lb[i], p.var_ub[i]) for i in range(p.n_vars)]

    def constraint_string(self, i: int) -> str:
        lib = host_lib()
        p = lib.stcsp_model_constraint_string(self._h, i)
        s = C.string_at(p).decode()
        lib.stcsp_host_free(p)
        return s

    def close(self):
        if self._h:
            host_lib().stcsp_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_streams(streams, n_obs: int):
    """A list of 2-D int arrays ([len, n_obs] each; an empty stream may be any empty array), or a pair (values, offsets)
    with offsets in steps -> (values int32 [total_steps * n_obs], offsets int64 [n_streams + 1]), both contiguous."""
    import numpy as np
    if isinstance(streams, tuple) and len(streams) == 2:
        values = np.ascontiguousarray(streams[0], dtype=np.int32).reshape(-1)
        offsets = np.ascontiguousarray(streams[1], dtype=np.int64).reshape(-1)
        if offsets.size == 0:
            raise ValueError("offsets must have n_streams + 1 entries")
        if values.size != max(int(offsets[-1]), 0) * n_obs and not (offsets[-1] < 0):
            raise ValueError(f"values must hold offsets[-1] * {n_obs} entries")
        return values, offsets
    rows = []
    offsets = np.zeros(len(streams) + 1, dtype=np.int64)
    for i, s in enumerate(streams):
        a = np.asarray(s, dtype=np.int32)
        if a.size == 0 and (a.ndim != 2 or a.shape[1] != n_obs):
            a = a.reshape(0, n_obs)
        if a.ndim != 2 or a.shape[1] != n_obs:
            raise ValueError(f"stream {i}: expected rows of {n_obs} observable values")
        rows.append(a)
        offsets[i + 1] = offsets[i] + a.shape[0]
    values = np.concatenate(rows, axis=0).reshape(-1) if rows else np.zeros(0, dtype=np.int32)
    return np.ascontiguousarray(values, dtype=np.int32), offsets


# ------------------------------------------------------------------ automaton (post-processing)
class Automaton:
    def __init__(self, model: Model, result: Result):
        lib = host_lib()
        h = C.c_void_p()
        rc = lib.stcsp_automaton_build(model.problem, C.byref(result), C.byref(h))
        if rc != 0:
            raise StcspError(rc, "automaton build failed")
        self._h = h
        self._model = model
        self._n_edges = result.n_edges

    def traverse(self):
        host_lib().stcsp_automaton_traverse(self._h)
        return self

    def adversarial(self, var_index: int = 5) -> int:
        return host_lib().stcsp_automaton_adversarial(self._h, var_index)

    def adversarial2(self, opponent: int = 5, avatar: int = 6) -> int:
        return host_lib().stcsp_automaton_adversarial2(self._h, opponent, avatar)

    def renumber(self):
        host_lib().stcsp_automaton_renumber(self._h)
        return self

    def order_by_label(self):
        """Scheduling-independent output order (reproducible solutions.dot / binary files)."""
        host_lib().stcsp_automaton_order_by_label(self._h)
        return self

    def import_flags(self, post: "PostResult"):
        """Adopt the flags of Engine.postprocess() (device passes) instead of traverse()/adversarial*()."""
        rc = host_lib().stcsp_automaton_import_flags(self._h, post.state_valid, post.state_final, post.edge_alive)
        if rc != 0:
            raise StcspError(rc, "import_flags failed")
        return self

    def flags(self):
        """(valid, final, alive) as bytes objects."""
        lib = host_lib()
        ns = lib.stcsp_automaton_num_states(self._h)
        ne = self._n_edges
        v, f, a = C.create_string_buffer(max(ns, 1)), C.create_string_buffer(max(ns, 1)), C.create_string_buffer(max(ne, 1))
        lib.stcsp_automaton_flags(self._h, v, f, a)
        return v.raw[:ns], f.raw[:ns], a.raw[:ne]

    def write_dot(self, path: str):
        rc = host_lib().stcsp_automaton_write_dot(self._h, os.fsencode(path))
        if rc != 0:
            raise StcspError(rc, f"cannot write {path}")

    def write_binary(self, path: str):
        rc = host_lib().stcsp_automaton_write_binary(self._h, os.fsencode(path))
        if rc != 0:
            raise StcspError(rc, f"cannot write {path}")

    @classmethod
    def read_binary(cls, path: str) -> "Automaton":
        h = C.c_void_p()
        rc = host_lib().stcsp_automaton_read_binary(os.fsencode(path), C.byref(h))
        if rc != 0:
            raise StcspError(rc, f"cannot read {path}")
        a = cls.__new__(cls)
        a._h, a._model, a._n_edges = h, None, 0
        return a

    def _mask(self, observable):
        """None (the default mask), "all", or a sequence of n_vars flags -> uint8 array or None."""
        if observable is None:
            return None
        return _observable_mask(len(self._model.var_names) if self._model is not None else len(observable), observable)

    def bisimulation(self, observable=None):
        """The largest bisimulation of the live automaton under the labels projected on `observable` (None: every
        variable whose name does not start with "_V"; "all"; or one flag per variable), by the host twin of
        Engine.quotient(). Returns (state_class int32 ndarray, -1 outside the live automaton; n_classes; rounds)."""
        import numpy as np
        lib = host_lib()
        m = self._mask(observable)
        cls = np.full(max(self.n_states, 1), -1, dtype=np.int32)
        n = C.c_int64()
        rounds = lib.stcsp_automaton_bisimulation(self._h, m.ctypes.data if m is not None else None, cls.ctypes.data, C.byref(n))
        if rounds < 0:
            raise StcspError(rounds, "bisimulation failed")
        return cls[:self.n_states], n.value, rounds

    def quotient(self, state_class, observable=None) -> "Automaton":
        """The quotient automaton under a partition of the live states (bisimulation() or Engine.quotient()): one
        state per class, one edge per distinct (source class, projected label, destination class). `observable` is
        the mask the partition was computed with (as in bisimulation())."""
        import numpy as np
        lib = host_lib()
        cls = np.ascontiguousarray(state_class, dtype=np.int32)
        if cls.shape != (self.n_states,):
            raise ValueError("state_class must have one entry per state")
        m = self._mask(observable)
        lib.stcsp_automaton_set_observable(self._h, m.ctypes.data if m is not None else None)
        h = C.c_void_p()
        rc = lib.stcsp_automaton_quotient(self._h, cls.ctypes.data, int(cls.max(initial=-1)) + 1, C.byref(h))
        if rc != 0:
            raise StcspError(rc, "quotient failed: state_class is not a partition of the live states")
        q = Automaton.__new__(Automaton)
        q._h, q._model, q._n_edges = h, self._model, 0
        return q

    def _observed(self, observable, streams=None):
        """What every stream service of the host twin starts from: (host library, pointer to the mask or None, n_observable,
        values, offsets, number of streams), the streams packed as in pack_streams(); None, None, 0 without streams."""
        lib = host_lib()
        m = self._mask(observable)
        mp = m.ctypes.data_as(C.c_void_p) if m is not None else None  # (the pointer keeps the array alive)
        n_obs = lib.stcsp_automaton_num_observable(self._h, mp)
        if streams is None:
            return lib, mp, n_obs, None, None, 0
        values, offsets = pack_streams(streams, n_obs)
        return lib, mp, n_obs, values, offsets, len(offsets) - 1

    def check_streams(self, streams, observable=None):
        """Check observed streams against the live automaton by the host twin of Engine.check_streams() (contract:
        include/stcsp_engine.h, stcsp_engine_monitor_check), on the automaton's current flags. `streams` as in
        pack_streams(); `observable` as in bisimulation(). Returns (accepted_len int32, n_end int32, end_final uint8,
        max_set_size): one entry per stream, and the largest state set met."""
        import numpy as np
        lib, mp, n_obs, values, offsets, n = self._observed(observable, streams)
        acc, nend, fin = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8)
        largest = C.c_int64()
        rc = lib.stcsp_automaton_check_streams(self._h, mp, n, offsets.ctypes.data,
                                               values.ctypes.data if values.size else None, acc.ctypes.data, nend.ctypes.data,
                                               fin.ctypes.data, C.byref(largest))
        if rc != 0:
            raise StcspError(rc, "check_streams failed: malformed offsets")
        return acc[:n], nend[:n], fin[:n], largest.value

    def generate(self, n, length, seed=0, ranks=None, observable=None, horizon=None, end_final=False):
        """Sample (ranks=None) or unrank `n` solution prefixes of `length` steps by the host twin of Engine.generate()
        (contract: include/stcsp_engine.h, stcsp_engine_generate), on the automaton's current flags. `observable` as in
        bisimulation(); `horizon` defaults to `length`. Returns (values int32 [n, length, n_observable], end_final uint8 [n],
        count float64 [horizon + 1])."""
        import numpy as np
        lib, mp, n_obs = self._observed(observable)[:3]
        horizon = length if horizon is None else horizon
        rk = None
        if ranks is not None:
            rk = np.ascontiguousarray(ranks, dtype=np.uint64)
            if rk.shape != (n,):
                raise ValueError("ranks must have one entry per stream")
        values = np.zeros((max(n, 0), max(length, 0), n_obs), np.int32)
        fin = np.zeros(max(n, 1), np.uint8)
        count = np.zeros(max(horizon, 0) + 1, np.float64)
        rc = lib.stcsp_automaton_generate(self._h, mp, horizon, GEN_END_FINAL if end_final else 0, n, length, seed,
                                          rk.ctypes.data if rk is not None and rk.size else None, count.ctypes.data,
                                          values.ctypes.data if values.size else None, fin.ctypes.data)
        if rc != 0:
            raise StcspError(rc, "generate failed: a length without a prefix or beyond the horizon, a rank that is not below count[length] < 2^53, "
                                 "or a count that overflows a double")
        return values, fin[:n], count

    def repair_streams(self, streams, observable=None, weights=None, end_final=False):
        """The nearest solution prefix of every observed stream by the host twin of Engine.repair_streams() (contract:
        include/stcsp_engine.h, stcsp_engine_repair), on the automaton's current flags. `streams` as in pack_streams(), a
        value REPAIR_MISSING = not observed; `observable` as in bisimulation(); `weights`: one non-negative int per observable
        variable (None: all 1). Returns (distance int32, list of repaired streams int32 [len, n_observable], end_final uint8,
        n_changed int32); distance -1 = no solution prefix of that length (its repaired stream is all 0)."""
        import numpy as np
        lib, mp, n_obs, values, offsets, n = self._observed(observable, streams)
        w = _repair_weights(weights, n_obs)
        dist, nchg, fin = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8)
        out = np.zeros(max(values.size, 1), np.int32)
        rc = lib.stcsp_automaton_repair_streams(self._h, mp, REPAIR_END_FINAL if end_final else 0, w.ctypes.data if w is not None else None, n,
                                                offsets.ctypes.data, values.ctypes.data if values.size else None, dist.ctypes.data,
                                                out.ctypes.data, fin.ctypes.data, nchg.ctypes.data)
        if rc != 0:
            raise StcspError(rc, "repair_streams failed: malformed offsets, a negative weight, or (sum of the weights) x (longest stream) above 2^31 - 2")
        return dist[:n], _repair_unpack(out[:values.size], offsets, n_obs), fin[:n], nchg[:n]

    def align_streams(self, streams, observable=None, weights=None, skip_cost=1, gap_cost=1, end_final=False):
        """The weighted edit distance of every observed stream to the solution language and the aligned solution prefix, by the
        host twin of Engine.align_streams() (contract: include/stcsp_engine.h, stcsp_engine_align), on the automaton's current
        flags. `streams`, `observable` and `weights` as in repair_streams(); `skip_cost` drops an observed step, `gap_cost`
        inserts a solution step the recorder missed. Returns (distance int32, list of emitted rows int32 [out_len,
        n_observable], list of ops uint8 (ALIGN_MATCH / ALIGN_SKIP / ALIGN_INSERT), n_changed, n_skipped, n_inserted int32,
        end_final uint8); distance -1 = no alignment (its rows and ops are empty)."""
        import numpy as np
        lib, mp, n_obs, values, offsets, n = self._observed(observable, streams)
        w = _repair_weights(weights, n_obs)
        skip_cost, gap_cost = _align_costs(skip_cost, gap_cost)
        dist, nchg, nskip, nins = (np.zeros(max(n, 1), np.int32) for _ in range(4))
        fin = np.zeros(max(n, 1), np.uint8)
        out_off, op_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        pv, po = C.c_void_p(), C.c_void_p()
        rc = lib.stcsp_automaton_align_streams(self._h, mp, ALIGN_END_FINAL if end_final else 0, w.ctypes.data if w is not None else None,
                                               skip_cost, gap_cost, n, offsets.ctypes.data, values.ctypes.data if values.size else None,
                                               dist.ctypes.data, out_off.ctypes.data, C.byref(pv), op_off.ctypes.data, C.byref(po),
                                               fin.ctypes.data, nchg.ctypes.data, nskip.ctypes.data, nins.ctypes.data)
        if rc != 0:
            raise StcspError(rc, "align_streams failed: malformed offsets, a negative weight, a cost below 1, or max(sum of the weights, skip) x "
                                 "(longest stream) + gap x (states) above 2^31 - 2")
        try:
            rows = _copy_array(C.cast(pv, C.POINTER(C.c_int32)), int(out_off[n]) * n_obs, np.int32)
            ops = _copy_array(C.cast(po, C.POINTER(C.c_uint8)), int(op_off[n]), np.uint8)
        finally:
            lib.stcsp_host_free(pv)
            lib.stcsp_host_free(po)
        return _align_unpack(n, n_obs, dist[:n], out_off, rows, op_off, ops, nchg[:n], nskip[:n], nins[:n], fin[:n])

    def infer_streams(self, streams, observable=None, end_final=False, draws=0, seed=0, ranks=None):
        """What the unobserved entries of partially observed streams can be, by the host twin of Engine.infer_streams()
        (contract: include/stcsp_engine.h, stcsp_engine_infer), on the automaton's current flags. `streams` as in
        pack_streams(), a value INFER_MISSING = not observed; `observable` as in bisimulation(); `draws` completions per
        stream, sampled with `seed` or, with `ranks` ([n][draws]), unranked. Returns (count float64 [n], supports, n_states,
        draws, end_final): per stream the supports as a [len][n_observable] list of sorted lists of ints, |F_t| as int32
        [len + 1], the draws as int32 [draws, len, n_observable] and their end_final as uint8 [draws]."""
        import numpy as np
        lib, mp, n_obs, values, offsets, n = self._observed(observable, streams)
        steps = max(int(offsets[n]), 0) if n else 0
        rk = _infer_ranks(ranks, n, draws)
        count = np.zeros(max(n, 1), np.float64)
        soff = np.zeros(steps * n_obs + 1, np.int64)
        nst = np.zeros(steps + n + 1, np.int32)
        dvals = np.zeros(max(steps * max(draws, 0) * n_obs, 1), np.int32)
        dfin = np.zeros(max(n * max(draws, 0), 1), np.uint8)
        sval = C.c_void_p()
        rc = lib.stcsp_automaton_infer_streams(self._h, mp, INFER_END_FINAL if end_final else 0, n, offsets.ctypes.data,
                                               values.ctypes.data if values.size else None, draws, rk.ctypes.data if rk is not None else None,
                                               seed, count.ctypes.data, soff.ctypes.data, C.byref(sval), nst.ctypes.data, dvals.ctypes.data,
                                               dfin.ctypes.data)
        if rc != 0:
            raise StcspError(rc, "infer_streams failed: malformed offsets, a negative number of draws, a rank that is not below its stream's "
                                 "count < 2^53, or draws from a count that overflows a double")
        total = int(soff[-1])
        vals = np.ctypeslib.as_array(C.cast(sval, C.POINTER(C.c_int32)), shape=(max(total, 1),))[:total].copy()
        lib.stcsp_host_free(sval)
        return _infer_unpack(count[:n], soff, vals, nst, dvals, dfin, offsets, n_obs, max(draws, 0))

    def posterior_streams(self, streams, observable=None, end_final=False, weights=None):
        """How many solution prefixes give each value of the unobserved entries of partially observed streams, by the host twin
        of Engine.posterior_streams() (contract: include/stcsp_engine.h, stcsp_engine_posterior), on the automaton's current
        flags. `streams` as in pack_streams(), a value POSTERIOR_MISSING = not observed; `observable` as in bisimulation();
        `weights`: per observable variable, in mask order, a dict value -> non-negative int weight or None (None: all 1).
        Returns (mass float64 [n], exact uint8 [n], final_mass list of ints, marginals): marginals[i][t][v] is the list of
        (value, mass) pairs of Python ints in value order; empty for a stream that is not exact or not feasible."""
        import numpy as np
        lib, mp, n_obs, values, offsets, n = self._observed(observable, streams)
        steps = max(int(offsets[n]), 0) if n else 0
        woff, wval, ww = _posterior_weights(weights, n_obs)
        mass, exact, fmass = np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint64)
        moff = np.zeros(steps * n_obs + 1, np.int64)
        mval, mmass = C.c_void_p(), C.c_void_p()
        rc = lib.stcsp_automaton_posterior_streams(self._h, mp, POSTERIOR_END_FINAL if end_final else 0, n, offsets.ctypes.data,
                                                   values.ctypes.data if values.size else None, woff.ctypes.data if woff is not None else None,
                                                   wval.ctypes.data if woff is not None else None, ww.ctypes.data if woff is not None else None,
                                                   mass.ctypes.data, exact.ctypes.data, fmass.ctypes.data, moff.ctypes.data, C.byref(mval),
                                                   C.byref(mmass))
        if rc != 0:
            raise StcspError(rc, "posterior_streams failed: malformed offsets, or weights that are not strictly increasing values with weights >= 0")
        total = int(moff[-1])
        vals = np.ctypeslib.as_array(C.cast(mval, C.POINTER(C.c_int32)), shape=(max(total, 1),))[:total].copy()
        masses = np.ctypeslib.as_array(C.cast(mmass, C.POINTER(C.c_uint64)), shape=(max(total, 1),))[:total].copy()
        lib.stcsp_host_free(mval)
        lib.stcsp_host_free(mmass)
        return _posterior_unpack(mass[:n], exact[:n], fmass[:n], moff, vals, masses, offsets, n_obs)

    def observer(self, observable=None, max_states=0):
        """The observer (subset construction) of the live automaton under `observable` (as in bisimulation()) by the host twin
        of Engine.observer() (contract: include/stcsp_engine.h, stcsp_engine_observer), on the automaton's current flags.
        Returns a dict of numpy arrays and scalars (see _observer_unpack()); StcspError -4 beyond max_states (0: the default)."""
        lib = host_lib()
        m = self._mask(observable)
        h = C.c_void_p()
        rc = lib.stcsp_automaton_observer(self._h, m.ctypes.data if m is not None else None, max_states, C.byref(h))
        if rc != 0:
            raise StcspError(rc, "observer failed: more sets than max_states" if rc == -4 else "observer failed")
        try:
            return _observer_unpack(lib.stcsp_observer_get(h).contents)
        finally:
            lib.stcsp_observer_free(h)

    def components(self, lassos=0, no_trim=False):
        """The strongly connected components, omega-liveness and lasso solutions of the live automaton by the host twin of
        Engine.components() (contract: include/stcsp_engine.h, stcsp_engine_components), on the automaton's current flags.
        lassos as there; no_trim is accepted and means nothing here. Returns the dict of _components_unpack()."""
        lib = host_lib()
        co = _components_options(lassos, no_trim)
        h = C.c_void_p()
        rc = lib.stcsp_automaton_components(self._h, co.max_lassos, co.flags, C.byref(h))
        if rc != 0:
            raise StcspError(rc, "components failed: two live out-edges of one state carry the same full row" if rc == -5 else "components failed")
        try:
            return _components_unpack(lib.stcsp_components_get(h).contents, int(lib.stcsp_automaton_num_states(self._h)))
        finally:
            lib.stcsp_components_free(h)

    def optimise(self, weights, horizon=0, lengths=(), maximise=False, end_final=False, mean=False, state_best=False):
        """The best solution prefixes and the least long-run mean cost under a linear objective by the host twin of Engine.optimise()
        (contract: include/stcsp_engine.h, stcsp_engine_optimise), on the automaton's current flags. Arguments as there. Returns the
        dict of _optimise_unpack()."""
        lib = host_lib()
        names = [lib.stcsp_automaton_var_name(self._h, i).decode() for i in range(lib.stcsp_automaton_num_vars(self._h))]
        rq, keep = _optimise_request(weights, names, horizon, lengths, maximise, end_final, mean, state_best)
        h = C.c_void_p()
        rc = lib.stcsp_automaton_optimise(self._h, C.byref(rq), C.byref(h))
        if rc != 0:
            raise StcspError(rc, {-1: "optimise failed: a negative horizon, a length outside 0 .. horizon, or costs beyond 2^62",
                                  -2: "optimise failed: nmax^2 * cmax exceeds 2^62 (the largest cyclic component, the largest edge cost)",
                                  -4: "optimise failed: no memory for the tables",
                                  -5: "optimise failed: two live out-edges of one state carry the same full row"}.get(rc, "optimise failed"))
        try:
            return _optimise_unpack(lib.stcsp_optimise_get(h).contents, keep[1], int(lib.stcsp_automaton_num_states(self._h)))
        finally:
            lib.stcsp_optimise_free(h)

    def ctl(self, formula, witness=False):
        """A fair CTL query over the infinite solutions by the host twin of Engine.ctl() (contract: include/stcsp_engine.h,
        stcsp_engine_ctl), on the automaton's current flags. formula: text (grammar: ctl_parse()) or a postfix program. Returns
        the dict of _ctl_unpack()."""
        lib = host_lib()
        names = [lib.stcsp_automaton_var_name(self._h, i).decode() for i in range(lib.stcsp_automaton_num_vars(self._h))]
        rq, keep = _ctl_request(formula, names, witness)
        h = C.c_void_p()
        rc = lib.stcsp_automaton_ctl(self._h, C.byref(rq), C.byref(h))
        if rc != 0:
            raise StcspError(rc, {-1: "ctl failed: a malformed program",
                                  -2: f"ctl failed: the lowered formula is over a limit ({CTL_MAX_NODES} atoms and operators, {CTL_MAX_SLOTS} sets, a predicate stack of 64)",
                                  -5: "ctl failed: a fixpoint did not converge, or two worlds out of one state carry the same full row"}.get(rc, "ctl failed"))
        try:
            return _ctl_unpack(lib.stcsp_ctl_get(h).contents)
        finally:
            lib.stcsp_ctl_free(h)

    def from_observer(self, obs, observable=None) -> "Automaton":
        """The observer `obs` (the dict of Engine.observer() or observer() for this automaton under `observable`) as an
        Automaton: one state per set, one edge per (set, projected row), carrying the least full label that projects on it."""
        lib = host_lib()
        m = self._mask(observable)
        res, keep = _observer_pack(obs)
        h = C.c_void_p()
        rc = lib.stcsp_automaton_from_observer(self._h, m.ctypes.data if m is not None else None, C.byref(res), C.byref(h))
        del keep
        if rc != 0:
            raise StcspError(rc, "from_observer failed: the observer does not belong to this automaton and mask")
        q = Automaton.__new__(Automaton)
        q._h, q._model, q._n_edges = h, self._model, 0
        return q

    def count_streams(self, horizon, end_final=False):
        """count[t], t = 0 .. horizon: the number of solution prefixes of length t (float64; exact below 2^53)."""
        import numpy as np
        count = np.zeros(max(horizon, 0) + 1, np.float64)
        rc = host_lib().stcsp_automaton_count_streams(self._h, horizon, GEN_END_FINAL if end_final else 0, count.ctypes.data)
        if rc != 0:
            raise StcspError(rc, "count_streams failed")
        return count

    def canonical(self) -> str:
        lib = host_lib()
        n = C.c_size_t()
        p = lib.stcsp_automaton_canonical(self._h, C.byref(n))
        s = C.string_at(p, n.value).decode()
        lib.stcsp_host_free(p)
        return s

    def canonical_sha256(self) -> str:
        return hashlib.sha256(self.canonical().encode()).hexdigest()

    @property
    def n_states(self):
        return host_lib().stcsp_automaton_num_states(self._h)

    @property
    def n_live_states(self):
        return host_lib().stcsp_automaton_num_live_states(self._h)

    @property
    def n_live_edges(self):
        return host_lib().stcsp_automaton_num_live_edges(self._h)

    def close(self):
        if self._h:
            host_lib().stcsp_automaton_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------ engine
class EngineBase:
    """Common driver for an engine-shaped C-ABI (create / solve / destroy + stepping calls)."""

    _prefix = "stcsp_engine"

    def __init__(self, lib: C.CDLL, model: Model, **opts):
        self._lib = lib
        self._model = model
        o = Options()
        o.device = opts.get("device", 0)
        o.rank = opts.get("rank", 0)
        o.world = opts.get("world", 1)
        o.batch_nodes = opts.get("batch_nodes", 0)
        o.max_search_nodes = opts.get("max_search_nodes", 0)
        o.time_limit_s = opts.get("time_limit_s", 0.0)
        o.flags = opts.get("flags", 0)
        self.options = o
        h = C.c_void_p()
        rc = self._f("create")(model.problem, C.byref(o), C.byref(h))
        if rc != 0:
            raise StcspError(rc, self._last_error(None))
        self._h = h
        self.result = Result()

    def _f(self, name):
        return getattr(self._lib, f"{self._prefix}_{name}")

    def _last_error(self, h):
        if hasattr(self._lib, f"{self._prefix}_last_error"):
            m = self._f("last_error")(h)
            return m.decode() if m else ""
        return ""

    def _check(self, rc):
        if rc != 0:
            raise StcspError(rc, self._last_error(self._h))

    def solve(self) -> Result:
        self._check(self._f("solve")(self._h, C.byref(self.result)))
        return self.result

    def export(self) -> Result:
        self._check(self._f("export")(self._h, C.byref(self.result)))
        return self.result

    # sharded stepping interface
    def begin(self):
        self._check(self._f("begin")(self._h))

    def expand_local(self) -> int:
        left = C.c_int64()
        self._check(self._f("expand_local")(self._h, C.byref(left)))
        return left.value

    def candidate_bytes(self) -> int:
        return self._f("candidate_bytes")(self._h)

    def outbox(self, peer: int):
        p = C.c_void_p()
        n = C.c_int64()
        self._check(self._f("outbox")(self._h, peer, C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def commit(self, ptr: int, count: int):
        self._check(self._f("commit")(self._h, C.c_void_p(ptr), count))

    def finish(self):
        self._check(self._f("finish")(self._h))

    def set_expand_budget(self, max_rounds: int, min_open: int):
        self._check(self._f("set_expand_budget")(self._h, max_rounds, min_open))

    def node_bytes(self) -> int:
        return self._f("node_bytes")(self._h)

    def donate(self, want: int):
        """Remove up to `want` of the oldest open nodes; returns (pointer, count) of their transfer records."""
        ptr, n = C.c_void_p(), C.c_int64()
        self._check(self._f("donate")(self._h, want, C.byref(ptr), C.byref(n)))
        return (ptr.value or 0), n.value

    def adopt(self, ptr: int, count: int):
        self._check(self._f("adopt")(self._h, C.c_void_p(ptr), count))

    def counters(self) -> Counters:
        c = Counters()
        self._check(self._f("counters")(self._h, C.byref(c)))
        return c

    def expand_variant(self) -> int:
        """The expansion kernel of the current program: bit 0 LITE, bit 1 the one-register LITE shape, bit 2 image in LDS."""
        v = self._f("expand_variant")(self._h)
        self._check(min(v, 0))
        return v

    def kernel_choice(self) -> dict:
        """The expansion, probe and commit kernel of the current program, by their template arguments (KernelChoice's fields)."""
        k = KernelChoice()
        self._check(self._f("kernel_choice")(self._h, C.byref(k)))
        return k.as_dict()

    def sets_blob(self):
        """This shard's constraint-set registry as a list of int32 words."""
        p = C.POINTER(C.c_int32)()
        n = C.c_int64()
        self._check(self._f("sets_blob")(self._h, C.byref(p), C.byref(n)))
        return [p[i] for i in range(n.value)]

    def sets_count(self) -> int:
        """Number of constraint sets this shard knows (word 0 of the registry blob)."""
        p = C.POINTER(C.c_int32)()
        n = C.c_int64()
        self._check(self._f("sets_blob")(self._h, C.byref(p), C.byref(n)))
        return p[0] if n.value else 0

    def sets_import(self, words):
        arr = (C.c_int32 * len(words))(*words)
        self._check(self._f("sets_import")(self._h, arr, len(words)))

    def postprocess(self, adversarial: int = -1, adversarial2: tuple | None = None) -> PostResult:
        """graphTraverse [+ adversarialTraverse(var)] [+ adversarialTraverse2(op, ava)] on the device."""
        po = PostOptions(adversarial, adversarial2[0] if adversarial2 else -1, adversarial2[1] if adversarial2 else -1, 0)
        out = PostResult()
        self._check(self._f("postprocess")(self._h, C.byref(po), C.byref(out)))
        return out

    def quotient(self, observable=None):
        """Bisimulation quotient of the live automaton on the device, after postprocess(): the classes of the states
        under the labels projected on `observable` (None: every variable whose name does not start with "_V"; "all";
        or one flag per variable). Returns (state_class int32 ndarray with -1 outside the live automaton, n_classes,
        rounds, seconds); the whole QuotientResult of the call is kept in self.quotient_result."""
        import numpy as np
        qo = QuotientOptions()
        m = _observable_mask(self._model.n_vars, observable)  # (alive until the call returns)
        if m is not None:
            qo.observable = m.ctypes.data_as(C.POINTER(C.c_uint8))
        out = QuotientResult()
        self._check(self._f("quotient")(self._h, C.byref(qo), C.byref(out)))
        self.quotient_result = out
        cls = np.ctypeslib.as_array(out.state_class, shape=(max(self.result.n_states, 1),))[:self.result.n_states].copy()
        return cls, out.n_classes, out.rounds, out.seconds

    def monitor(self, observable=None) -> MonitorInfo:
        """Build the stream monitor's look-up structures on the device for one mask, after postprocess() (`observable`
        as in quotient()). They stay valid until the next solve / postprocess / monitor. Returns the MonitorInfo."""
        mo = MonitorOptions()
        m = _observable_mask(self._model.n_vars, observable)  # (alive until the call returns)
        if m is not None:
            mo.observable = m.ctypes.data_as(C.POINTER(C.c_uint8))
        info = MonitorInfo()
        self._check(self._f("monitor_build")(self._h, C.byref(mo), C.byref(info)))
        self.monitor_info = info
        return info

    def check_streams(self, streams, force_sets: bool = False):
        """Check observed streams against the live automaton on the device, after monitor(). `streams`: a list of 2-D
        int arrays, one row of the observable variables' values per step, or (values, offsets) as in pack_streams().
        Returns (accepted_len int32, n_end int32, end_final uint8, n_host_fallback); the whole MonitorResult of the
        call is kept in self.monitor_result. Always exact: see include/stcsp_engine.h."""
        import numpy as np
        if getattr(self, "monitor_info", None) is None:
            raise StcspError(-6, "check_streams() needs monitor() first")
        values, offsets = pack_streams(streams, self.monitor_info.n_observable)
        n = len(offsets) - 1
        ms = MonitorStreams(*_stream_head(values, offsets), MON_FORCE_SETS if force_sets else 0, 0)
        out = MonitorResult()
        self._check(self._f("monitor_check")(self._h, C.byref(ms), C.byref(out)))
        self.monitor_result = out
        if n == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8), 0
        return (np.ctypeslib.as_array(out.accepted_len, shape=(n,)).copy(), np.ctypeslib.as_array(out.n_end, shape=(n,)).copy(),
                np.ctypeslib.as_array(out.end_final, shape=(n,)).copy(), out.n_host_fallback)

    def generator(self, observable=None, horizon=64, end_final=False) -> GeneratorInfo:
        """Build the stream generator's structures on the device for one mask and horizon, after postprocess() (`observable`
        as in quotient()). They stay valid until the next solve / postprocess / generator. Returns the GeneratorInfo; its
        .count is a numpy float64 array [horizon + 1]: the number of solution prefixes of every length."""
        import numpy as np
        go = GeneratorOptions()
        go.horizon = horizon
        go.flags = GEN_END_FINAL if end_final else 0
        m = _observable_mask(self._model.n_vars, observable)  # (alive until the call returns)
        if m is not None:
            go.observable = m.ctypes.data_as(C.POINTER(C.c_uint8))
        info = GeneratorInfo()
        self.generator_info = None
        self._check(self._f("generator_build")(self._h, C.byref(go), C.byref(info)))
        info.count = np.ctypeslib.as_array(info._count, shape=(info.horizon + 1,)).copy()
        self.generator_info = info
        return info

    def _needs_generator(self, who):
        if getattr(self, "generator_info", None) is None:
            raise StcspError(-6, f"{who}() needs generator() first")

    def _generator_streams(self, who, streams):
        """What every stream service on the generator's structures starts from: (n_observable of its mask, values, offsets,
        number of streams), the streams packed as in pack_streams()."""
        self._needs_generator(who)
        n_obs = self.generator_info.n_observable
        values, offsets = pack_streams(streams, n_obs)
        return n_obs, values, offsets, len(offsets) - 1

    def generate(self, n, length, seed=0, ranks=None):
        """`n` solution prefixes of `length` steps from the device, after generator(): sampled with `seed` (uniform over the
        paths of that length), or the ranks[i]-th in lexicographic order. Returns (values int32 [n, length, n_observable],
        end_final uint8 [n]); the whole GenerateResult of the call is kept in self.generate_result."""
        import numpy as np
        self._needs_generator("generate")
        rq = GenerateRequest(n, None, seed, length, 0)
        if ranks is not None:
            rk = np.ascontiguousarray(ranks, dtype=np.uint64)
            if rk.shape != (n,):
                raise ValueError("ranks must have one entry per stream")
            if n == 0:
                rk = np.zeros(1, np.uint64)
            rq.ranks = rk.ctypes.data_as(C.POINTER(C.c_uint64))
        out = GenerateResult()
        self._check(self._f("generate")(self._h, C.byref(rq), C.byref(out)))
        self.generate_result = out
        n_obs = out.n_observable
        cells = n * length * n_obs
        values = np.ctypeslib.as_array(out.values, shape=(cells,)).copy() if cells else np.zeros(0, np.int32)
        fin = np.ctypeslib.as_array(out.end_final, shape=(n,)).copy() if n else np.zeros(0, np.uint8)
        return values.reshape(n, length, n_obs), fin

    def repair_streams(self, streams, weights=None, end_final=False):
        """The nearest solution prefix of every observed stream, on the device, after generator() (its mask; its horizon does
        not limit the streams). `streams` as for check_streams(), a value REPAIR_MISSING = not observed; `weights`: one
        non-negative int per observable variable (None: all 1). Returns (distance int32, list of repaired streams int32
        [len, n_observable], end_final uint8, n_changed int32); distance -1 = no solution prefix of that length. The whole
        RepairResult of the call is kept in self.repair_result. Contract: include/stcsp_engine.h, stcsp_engine_repair."""
        import numpy as np
        n_obs, values, offsets, n = self._generator_streams("repair_streams", streams)
        w = _repair_weights(weights, n_obs)
        rq = RepairRequest(*_stream_head(values, offsets), w.ctypes.data_as(C.POINTER(C.c_int32)) if w is not None else None,
                           REPAIR_END_FINAL if end_final else 0, 0)
        out = RepairResult()
        self._check(self._f("repair")(self._h, C.byref(rq), C.byref(out)))
        self.repair_result = out
        if n == 0:
            return np.zeros(0, np.int32), [], np.zeros(0, np.uint8), np.zeros(0, np.int32)
        rows = np.ctypeslib.as_array(out.values, shape=(values.size,)).copy() if values.size else np.zeros(0, np.int32)
        return (np.ctypeslib.as_array(out.distance, shape=(n,)).copy(), _repair_unpack(rows, offsets, n_obs),
                np.ctypeslib.as_array(out.end_final, shape=(n,)).copy(), np.ctypeslib.as_array(out.n_changed, shape=(n,)).copy())

    def align_streams(self, streams, weights=None, skip_cost=1, gap_cost=1, end_final=False):
        """The weighted edit distance of every observed stream to the solution language and the aligned solution prefix, on the
        device, after generator() (its mask; its horizon does not limit the streams). `streams` and `weights` as for
        repair_streams(); `skip_cost` drops an observed step as spurious, `gap_cost` inserts a solution step the recorder
        missed. Returns what Automaton.align_streams() returns; the whole AlignResult of the call is kept in
        self.align_result. Contract: include/stcsp_engine.h, stcsp_engine_align."""
        import numpy as np
        n_obs, values, offsets, n = self._generator_streams("align_streams", streams)
        w = _repair_weights(weights, n_obs)
        skip_cost, gap_cost = _align_costs(skip_cost, gap_cost)
        rq = AlignRequest(*_stream_head(values, offsets), w.ctypes.data_as(C.POINTER(C.c_int32)) if w is not None else None,
                          skip_cost, gap_cost, ALIGN_END_FINAL if end_final else 0, 0)
        out = AlignResult()
        self._check(self._f("align")(self._h, C.byref(rq), C.byref(out)))
        self.align_result = out
        arr = _copy_array
        out_off, op_off = arr(out.out_offsets, n + 1, np.int64), arr(out.op_offsets, n + 1, np.int64)
        return _align_unpack(n, n_obs, arr(out.distance, n, np.int32), out_off, arr(out.values, int(out_off[n]) * n_obs, np.int32), op_off,
                             arr(out.ops, int(op_off[n]), np.uint8), arr(out.n_changed, n, np.int32), arr(out.n_skipped, n, np.int32),
                             arr(out.n_inserted, n, np.int32), arr(out.end_final, n, np.uint8))

    def infer_streams(self, streams, end_final=False, draws=0, seed=0, ranks=None):
        """What the unobserved entries of partially observed streams can be, on the device, after generator() (its mask; its
        horizon does not limit the streams). `streams` as for check_streams(), a value INFER_MISSING = not observed; `draws`
        completions per stream, sampled with `seed` or, with `ranks` ([n][draws]), unranked. Returns (count float64 [n],
        supports, n_states, draws, end_final) as Automaton.infer_streams() does; the whole InferResult of the call is kept in
        self.infer_result. Contract: include/stcsp_engine.h, stcsp_engine_infer."""
        import numpy as np
        n_obs, values, offsets, n = self._generator_streams("infer_streams", streams)
        steps = max(int(offsets[n]), 0) if n else 0
        rk = _infer_ranks(ranks, n, draws)
        rq = InferRequest(*_stream_head(values, offsets), rk.ctypes.data_as(C.POINTER(C.c_uint64)) if rk is not None else None, seed,
                          INFER_END_FINAL if end_final else 0, draws)
        out = InferResult()
        self._check(self._f("infer")(self._h, C.byref(rq), C.byref(out)))
        self.infer_result = out
        arr = _copy_array
        soff = arr(out.support_off, steps * n_obs + 1, np.int64)
        return _infer_unpack(arr(out.count, n, np.float64), soff, arr(out.support_val, int(soff[-1]), np.int32), arr(out.n_states, steps + n, np.int32),
                             arr(out.values, steps * draws * n_obs, np.int32), arr(out.end_final, n * draws, np.uint8), offsets, n_obs, draws)

    def posterior_streams(self, streams, end_final=False, weights=None):
        """How many solution prefixes give each value of the unobserved entries of partially observed streams, on the device,
        after generator() (its mask; its horizon does not limit the streams). `streams` as for check_streams(), a value
        POSTERIOR_MISSING = not observed; `weights`: per observable variable, in mask order, a dict value -> non-negative int
        weight or None (None: all 1). Returns (mass float64 [n], exact, final_mass, marginals) as Automaton.posterior_streams()
        does; the whole PosteriorResult of the call is kept in self.posterior_result. Contract: include/stcsp_engine.h,
        stcsp_engine_posterior."""
        import numpy as np
        n_obs, values, offsets, n = self._generator_streams("posterior_streams", streams)
        steps = max(int(offsets[n]), 0) if n else 0
        woff, wval, ww = _posterior_weights(weights, n_obs)
        rq = PosteriorRequest(*_stream_head(values, offsets),
                              woff.ctypes.data_as(C.POINTER(C.c_int64)) if woff is not None else None,
                              wval.ctypes.data_as(C.POINTER(C.c_int32)) if woff is not None else None,
                              ww.ctypes.data_as(C.POINTER(C.c_int32)) if woff is not None else None, POSTERIOR_END_FINAL if end_final else 0, 0)
        out = PosteriorResult()
        self._check(self._f("posterior")(self._h, C.byref(rq), C.byref(out)))
        self.posterior_result = out
        arr = _copy_array
        moff = arr(out.marg_off, steps * n_obs + 1, np.int64)
        total = int(moff[-1])
        return _posterior_unpack(arr(out.mass, n, np.float64), arr(out.exact, n, np.uint8), arr(out.final_mass, n, np.uint64), moff,
                                 arr(out.marg_val, total, np.int32), arr(out.marg_mass, total, np.uint64), offsets, n_obs)

    def observer(self, max_states=0):
        """The observer (subset construction) of the live automaton on the device, after generator() (its mask; its horizon plays
        no part): the deterministic automaton over the sets of states the system can be in after an observed prefix. Returns a
        dict of numpy arrays and scalars (see _observer_unpack()); members are state indices of the last Result. StcspError -4
        beyond max_states (0: the default) or the byte budget. Contract: include/stcsp_engine.h, stcsp_engine_observer."""
        self._needs_generator("observer")
        oo = ObserverOptions(max_states)
        out = ObserverResult()
        self._check(self._f("observer")(self._h, C.byref(oo), C.byref(out)))
        return _observer_unpack(out)

    def compare(self, right, max_pairs=0):
        """The comparison of the observer that the last observer() built on this engine (left) with `right`, an observer dict (of
        another engine's observer(), of Automaton.observer(), or any deterministic automaton in that form, its columns in the order
        of this engine's observable variables), on the device: the product of the two, the four inclusions P(L) in P(R), P(R) in
        P(L), F(L) in F(R), F(R) in F(L) and their shortest witnesses. Returns the dict of _compare_unpack(). StcspError -6 without
        a valid observer, -1 for a malformed operand, -4 beyond max_pairs (0: the default) or the byte budget. Contract:
        include/stcsp_engine.h, stcsp_engine_compare."""
        res, keep = _observer_pack(right)
        rq = CompareRequest(C.pointer(res), max_pairs)
        out = CompareResult()
        rc = self._f("compare")(self._h, C.byref(rq), C.byref(out))
        del keep
        self._check(rc)
        return _compare_unpack(out)

    def components(self, lassos=0, no_trim=False):
        """The strongly connected components of the live automaton on the device, after postprocess(): which states belong
        together in the long run, which components are cyclic, final, bottom and accepting, which states start an infinite
        solution (state_omega, root_omega), and lasso solutions stem . loop^omega. lassos: 0 (none), "all", "bottom" (the bottom
        accepting components only) or a count; no_trim (tests, measurements) lets the colouring rounds find every component.
        Returns the dict of _components_unpack(); it touches no other service's state. Contract: include/stcsp_engine.h,
        stcsp_engine_components."""
        co = _components_options(lassos, no_trim)
        out = ComponentsResult()
        self._check(self._f("components")(self._h, C.byref(co), C.byref(out)))
        return _components_unpack(out, self.result.n_states)

    def optimise(self, weights, horizon=0, lengths=(), maximise=False, end_final=False, mean=False, state_best=False):
        """Which solution is best, on the device, after postprocess(). The cost of a step is sum_v weights[v] * value of v on the edge;
        weights is a dict name -> int (the other variables 0) or one int per variable. Finite horizon: best[L], L = 0 .. horizon, the
        least (maximise: the greatest) total cost of a solution prefix of L steps (end_final: that ends in a final state), OPT_NONE
        where there is none; for every L in `lengths` the lexicographically least prefix that attains it; state_best: the same for
        L = horizon from every live state. mean: per strongly connected component (numbered as components() numbers them) the least
        mean cost per step of a cycle in it, as an exact fraction, and the least over the accepting components, which is the infimum
        of the long-run mean cost of an infinite solution. Returns the dict of _optimise_unpack(); it touches no other service's state
        but, with mean, the result of an earlier components(). Contract: include/stcsp_engine.h, stcsp_engine_optimise."""
        rq, keep = _optimise_request(weights, self._model.var_names, horizon, lengths, maximise, end_final, mean, state_best)
        out = OptimiseResult()
        self._check(self._f("optimise")(self._h, C.byref(rq), C.byref(out)))
        return _optimise_unpack(out, keep[1], self.result.n_states)

    def ctl(self, formula, witness=False):
        """A fair CTL query over the infinite solutions on the device, after postprocess(): does `formula` hold on the first steps of
        the solutions, where does it hold, and with witness=True a shortest witness (top EX / EU / EF) or counterexample (top AX / AG).
        Only infinite solutions are quantified over; a model without one has 0 worlds and every query on it is vacuous. formula:
        text (grammar: ctl_parse()) or a postfix program. Returns the dict of _ctl_unpack(); it replaces the result of an earlier
        components() and touches no other service's state. Contract: include/stcsp_engine.h, stcsp_engine_ctl."""
        rq, keep = _ctl_request(formula, self._model.var_names, witness)
        out = CtlResult()
        self._check(self._f("ctl")(self._h, C.byref(rq), C.byref(out)))
        return _ctl_unpack(out)

    def automaton(self, result: Result | None = None) -> Automaton:
        return Automaton(self._model, result if result is not None else self.result)

    def close(self):
        if getattr(self, "_h", None):
            self._f("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine(EngineBase):
    """The MI355X engine (HIP, gfx950).  Replaces solverSolve's search (reference
    src/solveralgorithm.cpp:966-971)."""

    def __init__(self, model: Model, **opts):
        super().__init__(hip_lib(), model, **opts)

    def propagate(self, blocks, set_index: int = 0, expire: int = 0):
        """Kernel-granularity check: run the device code of one search node on each row of `blocks`
        (numpy uint32 [count, N*K]). Returns (propagated blocks, outcome per block, skipped revisions)."""
        import numpy as np
        b = np.ascontiguousarray(blocks, dtype=np.uint32).copy()
        count = b.shape[0]
        outcome = np.zeros(count, dtype=np.int32)
        skipped = C.c_int64(0)
        self._check(self._f("propagate")(self._h, set_index, expire, b.ctypes.data_as(C.POINTER(C.c_uint32)), count,
                                         outcome.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(skipped)))
        return b, outcome, skipped.value


# ------------------------------------------------------------------ native sharded solve (include/stcsp_sharded.h)
class ShardedOptions(C.Structure):
    _fields_ = [("budget_rounds", C.c_int64), ("share_per_rank", C.c_int64), ("max_supersteps", C.c_int64)]


class ShardedStats(C.Structure):
    _fields_ = [("supersteps", C.c_int64), ("nodes_donated", C.c_int64), ("nodes_adopted", C.c_int64),
                ("candidates_sent", C.c_int64), ("candidates_received", C.c_int64), ("seconds_collectives", C.c_double),
                ("seconds_expand", C.c_double), ("seconds_pack", C.c_double), ("seconds_commit", C.c_double)]


def _bind_sharded(lib):
    if getattr(lib, "_stcsp_sharded_bound", False):
        return
    lib.stcsp_engine_solve_sharded.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(ShardedOptions), C.POINTER(ShardedStats)]
    lib.stcsp_local_group_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    lib.stcsp_local_group_transport.argtypes = [C.c_void_p, C.c_int32]
    lib.stcsp_local_group_transport.restype = C.c_void_p
    lib.stcsp_local_group_destroy.argtypes = [C.c_void_p]
    lib.stcsp_local_group_destroy.restype = None
    lib._stcsp_sharded_bound = True


def solve_sharded_native(engine: "Engine", transport: int, budget_rounds: int = 8, share_per_rank: int = 64) -> dict:
    """stcsp_engine_solve_sharded: the whole superstep loop of this rank inside the engine library (no Python, no torch
    between two bursts of k_expand); `transport` = pointer to a stcsp_transport (LocalGroup.transport(r), RcclTransport.ptr)."""
    lib = hip_lib()
    _bind_sharded(lib)
    o = ShardedOptions(budget_rounds, share_per_rank, 0)
    st = ShardedStats()
    engine._check(lib.stcsp_engine_solve_sharded(engine._h, C.c_void_p(transport), C.byref(o), C.byref(st)))
    return {n: getattr(st, n) for n, _ in st._fields_}


class LocalGroup:
    """stcsp_local_group: `world` transports for `world` engines of ONE process, one host thread each (same or different
    GPUs; records move with hipMemcpy[Peer]Async)."""

    def __init__(self, world: int):
        lib = hip_lib()
        _bind_sharded(lib)
        self._lib, self.world = lib, world
        h = C.c_void_p()
        rc = lib.stcsp_local_group_create(world, C.byref(h))
        if rc != 0:
            raise StcspError(rc, "local group")
        self._h = h

    def transport(self, rank: int) -> int:
        return self._lib.stcsp_local_group_transport(self._h, rank)

    def solve(self, engines, **knobs):
        """Run stcsp_engine_solve_sharded on every engine, one thread per rank; returns the per-rank stats (raises the
        first rank's error after ALL threads have ended)."""
        import threading
        out, errs = [None] * self.world, [None] * self.world

        def run(r):
            try:
                out[r] = solve_sharded_native(engines[r], self.transport(r), **knobs)
            except Exception as ex:  # noqa: BLE001
                errs[r] = ex

        ts = [threading.Thread(target=run, args=(r,)) for r in range(self.world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        self.errors = errs
        for ex in errs:
            if ex is not None:
                raise ex
        return out

    def close(self):
        if self._h:
            self._lib.stcsp_local_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_rccl = None


def rccl_lib() -> C.CDLL:
    """libstcsp_rccl.so: the stcsp_transport over RCCL (one process per GPU)."""
    global _rccl
    if _rccl is None:
        path = CSRC / "libstcsp_rccl.so"
        if not path.exists():
            raise RuntimeError(f"{path} is missing -- build it (make -C {CSRC})")
        lib = C.CDLL(str(path))
        lib.stcsp_rccl_unique_id.argtypes = [C.c_void_p]
        lib.stcsp_transport_rccl_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        lib.stcsp_transport_rccl_destroy.argtypes = [C.c_void_p]
        lib.stcsp_transport_rccl_destroy.restype = None
        _rccl = lib
    return _rccl


RCCL_ID_BYTES = 128


def rccl_unique_id() -> bytes:
    buf = C.create_string_buffer(RCCL_ID_BYTES)
    rc = rccl_lib().stcsp_rccl_unique_id(buf)
    if rc != 0:
        raise StcspError(rc, "ncclGetUniqueId failed")
    return buf.raw


class RcclTransport:
    def __init__(self, unique_id: bytes, rank: int, world: int, device: int):
        lib = rccl_lib()
        h = C.c_void_p()
        rc = lib.stcsp_transport_rccl_create(C.create_string_buffer(unique_id, RCCL_ID_BYTES), rank, world, device, C.byref(h))
        if rc != 0:
            raise StcspError(rc, "ncclCommInitRank failed")
        self._lib, self.ptr = lib, h.value

    def close(self):
        if self.ptr:
            self._lib.stcsp_transport_rccl_destroy(C.c_void_p(self.ptr))
            self.ptr = None


def merge_shards(results):
    """stcsp_merge_shards over a list of Result structs; returns (handle, Result)."""
    lib = host_lib()
    arr = (C.POINTER(Result) * len(results))(*[C.pointer(r) for r in results])
    h = C.c_void_p()
    rc = lib.stcsp_merge_shards(arr, len(results), C.byref(h))
    if rc != 0:
        raise StcspError(rc, "merge failed")
    return h, lib.stcsp_merged_result(h).contents


def solve_to_canonical(model: Model, engine: EngineBase, adversarial: bool = False):
    """solverSolve's tail (reference src/solveralgorithm.cpp:972-997) on top of an engine."""
    res = engine.solve()
    a = engine.automaton(res)
    a.traverse()
    adv = a.adversarial(5) if adversarial else None
    a.renumber()
    return a, adv
