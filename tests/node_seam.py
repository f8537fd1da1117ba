"""The node-level seam of the production expansion kernels (tests only): put any block in front of k_expand and read back what
one expansion made of it, through the stepping calls alone -- a stepped world-1 engine, donate / adopt with the record layout of
tests/xfer_ref.py, set_expand_budget, and one expansion per slot, round and launch.

`encode` is the inverse of xfer_ref.decode. `Seam.step(parents)` adopts crafted parents (seed 0: every item dirty) into an empty
frontier, runs ONE round, and returns per parent the verdict (fail / branch / leaf), the two children of a branch with their seeds,
and the candidate record of a leaf (edge labels, time-advanced block, new expire words, signature). Children and candidates find
their parent through a marker variable: an unconstrained variable (no item, no signature word: mixed_rows.free_booleans) that the
parent fixes to its own index at every point of its block, so a batch holds at most as many parents as the marker has values.

The step invariant -- a step is one expansion per parent -- is asserted on the engine's own counters, never worked around:
search_nodes grows by len(parents) and fails + leaves + children / 2 == len(parents). One documented second pass: a leaf under a
constraint set with `first` constraints asks the host for the set's translation and is parked again, propagated, with seed
kSeedNone (dev_kernels.hpp OC_MISS); those records -- and only those -- are adopted once more and must all come back as candidates.

ROWS holds the models of tests/test_node_seam.py (CPU) and tests/test_node_seam_gpu.py: text, the constraints the front end must
normalise it to (tests/bounds_ref.py reads that list, never the text), K, domain form, kernel family and how parents are drawn.

Plain Python and ctypes; the GPU is touched by Seam and DeviceWords alone."""
import ctypes as C
import importlib
import os
import random
import time
from collections import namedtuple

import numpy as np

import bounds_ref as br
import xfer_ref as xr

st = importlib.import_module("stcsp-solver_amd")
INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1
SEED_NONE = (1 << 12) - 1  # kSeedNone (device_types.hpp)
CAND_HDR = 8               # kCandHdr
SEAM_ENV = {"STCSP_CHAIN_SMALL": "1", "STCSP_CHAIN_BIG": "1",  # one expansion per slot and round,
            "STCSP_BURST": "1",                                 # one round per launch burst,
            "STCSP_FORCE_CANDIDATES": "1"}                      # every leaf a candidate record (a single shard owns every state)


def one_expansion_per_round(monkeypatch):
    """One expansion per slot and round: the frontier is wide when expand_local hands control back (test_many_until_sharded)."""
    monkeypatch.setenv("STCSP_CHAIN_SMALL", "1")
    monkeypatch.setenv("STCSP_CHAIN_BIG", "1")


class DeviceWords:
    """A device buffer of the test's own (the engine's runtime, reached through the engine library: no second runtime in the
    process). The engine reads adopted and committed records after the call returns, so they must not stay in the buffers
    the engine reuses; `load` copies them here. `load` may free and replace the buffer, which is safe only because every call
    of it comes after an engine call that waits for the engine's stream -- donate(), outbox() and expand_local() all
    synchronise before they return (engine.hip), so no adopt or commit kernel is still reading the old buffer."""
    H2D, D2H, D2D = 1, 2, 3  # hipMemcpyHostToDevice, ...DeviceToHost, ...DeviceToDevice (hip_runtime_api.h: enum hipMemcpyKind)

    def __init__(self, lib):
        self.lib, self.ptr, self.cap = lib, None, 0
        lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        lib.hipFree.argtypes = [C.c_void_p]

    def _room(self, n_words: int):
        if n_words > self.cap:
            self.free()
            p = C.c_void_p()
            assert self.lib.hipMalloc(C.byref(p), n_words * 2 * 4) == 0
            self.ptr, self.cap = p.value, n_words * 2

    def load(self, src: int, n_words: int):
        self._room(n_words)
        if n_words:
            assert self.lib.hipMemcpy(self.ptr, src, n_words * 4, self.D2D) == 0
        self.n = n_words
        return self.ptr or 0

    def put(self, words):
        """Host words (uint32) into the buffer: crafted records. Same rule as `load` for when it may be called."""
        a = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        self._room(len(a))
        if len(a):
            assert self.lib.hipMemcpy(self.ptr, a.ctypes.data, len(a) * 4, self.H2D) == 0
        self.n = len(a)
        return self.ptr or 0

    def host(self):
        out = np.zeros(self.n, dtype=np.uint32)
        if self.n:
            assert self.lib.hipMemcpy(out.ctypes.data, self.ptr, self.n * 4, self.D2H) == 0
        return out

    def free(self):
        if self.ptr:
            assert self.lib.hipFree(self.ptr) == 0
        self.ptr, self.cap = None, 0


# ------------------------------------------------------------------ record coding
def to_mask(values, lb: int) -> int:
    m = 0
    for x in values:
        m |= 1 << (x - lb)
    return m


def from_mask(mask: int, lb: int) -> set:
    return {lb + i for i in range(mask.bit_length()) if (mask >> i) & 1}


def to_record_domains(domains, bounds, form):
    """Yardstick domains (sets / pairs, index p * N + v) as xfer_ref.decode gives them: masks over the declared domain, or pairs."""
    n = len(bounds)
    if form == xr.INTERVALS:
        return [tuple(d) for d in domains]
    return [to_mask(d, bounds[i % n][0]) for i, d in enumerate(domains)]


def from_record_domains(doms, bounds, form):
    n = len(bounds)
    if form == xr.INTERVALS:
        return [tuple(d) for d in doms]
    return [from_mask(d, bounds[i % n][0]) for i, d in enumerate(doms)]


def encode(gid: int, tag: int, seed: int, expire, domains, n_vars: int, k: int, form: int) -> list:
    """The inverse of xfer_ref.decode: the words of one transfer record, padding (zero) included. `expire`: 1 to 4 words;
    `domains`: index p * N + v, a mask over the declared domain (bitset forms) or a (lo, hi) pair (intervals)."""
    nk = n_vars * k
    assert len(domains) == nk and 1 <= len(expire) <= 4
    w = [0] * xr.stride(n_vars, k, form)
    w[0], w[1], w[2], w[3], w[4] = gid & 0xFFFFFFFF, gid >> 32, tag & 0xFFFFFFFF, expire[0], seed
    for j, x in enumerate(expire[1:]):
        w[xr.XFER_EXPIRE + j] = x
    for i, d in enumerate(domains):
        at = xr.XFER_HDR + i
        if form == xr.INTERVALS:
            w[at], w[at + nk] = d[0] & 0xFFFFFFFF, d[1] & 0xFFFFFFFF
        else:
            assert d >> (32 * form) == 0
            for c in range(form):
                w[at + c * nk] = (d >> (32 * c)) & 0xFFFFFFFF
    return w


def decode_candidate(rec, n_vars: int, k: int, form: int, sig_len: int, n_until_cons: int) -> dict:
    """A candidate record (device_types.hpp:229-230): [0,1] source gid, [2] next set tag, [3] expire word 0, [4,5] key hash,
    [8..) signature, N edge-label values (int32), the time-advanced block, expire words 1 .. UW-1."""
    w = [int(x) & 0xFFFFFFFF for x in rec]
    s32 = lambda x: x - (1 << 32) if x >> 31 else x  # noqa: E731
    at = CAND_HDR + sig_len
    nkc = n_vars * k * xr.chunks(form)
    block = [0] * xr.XFER_HDR + w[at + n_vars: at + n_vars + nkc]
    uw = xr.expire_words(n_until_cons)
    return dict(gid=w[0] | w[1] << 32, tag=w[2], signature=[s32(x) for x in w[CAND_HDR: at]], labels=[s32(x) for x in w[at: at + n_vars]],
                expire=[w[3]] + w[at + n_vars + nkc: at + n_vars + nkc + uw - 1],
                domains=xr.decode(block, n_vars, k, form, 0)["domains"])


def cand_stride(n_vars: int, k: int, form: int, sig_len: int, n_until_cons: int) -> int:
    return (CAND_HDR + sig_len + n_vars + n_vars * k * xr.chunks(form) + xr.expire_words(n_until_cons) - 1 + 3) & ~3


# ------------------------------------------------------------------ the harness
Outcome = namedtuple("Outcome", "verdict children candidate")  # children: [(seed, domains)] x 2 in record form; candidate: decode_candidate


class Seam:
    """A stepped world-1 engine behind begin(), its frontier empty, ready for `step`. `sig_vars`: indices of the variables on
    the left of an arc (the signature, in variable order); `marker`: index of the marker variable."""

    def __init__(self, stcsp, model, k: int, form: int, flags: int, n_until_cons: int, sig_vars, marker: int):
        saved = {key: os.environ.get(key) for key in SEAM_ENV}
        os.environ.update(SEAM_ENV)
        try:
            self.e = stcsp.Engine(model, rank=0, world=1, flags=flags | stcsp.F_STEPPED)
        finally:
            for key, val in saved.items():
                if val is None:
                    os.environ.pop(key, None)
                else:
                    os.environ[key] = val
        e = self.e
        self.N, self.K, self.form, self.untils, self.marker = model.n_vars, k, form, n_until_cons, marker
        self.bounds = model.var_bounds()
        self.sig_vars = list(sig_vars)
        self.sig_len = len(self.sig_vars) + n_until_cons
        self.nsw = e.node_bytes() // 4
        assert self.nsw == xr.stride(self.N, k, form)
        self.csw = e.candidate_bytes() // 4
        assert self.csw == cand_stride(self.N, k, form, self.sig_len, n_until_cons), (self.csw, self.sig_len)
        lib = stcsp.hip_lib()
        self.parents_buf, self.kids, self.cands = DeviceWords(lib), DeviceWords(lib), DeviceWords(lib)
        self.skipped = 0
        e.set_expand_budget(1, 1)
        e.begin()
        # 1. the header of every crafted parent: the root's gid and the root set's tag, from a donated record
        recs = self._donate_all()
        if not len(recs):
            e.expand_local()
            recs = self._donate_all()
            assert len(recs), "neither the root nor a child of it was donated"
            self._drain_outbox()
        d = xr.decode(recs[0], self.N, k, form, n_until_cons)
        self.gid, self.tag = d["gid"], d["tag"]
        assert all(xr.decode(r, self.N, k, form, n_until_cons)["tag"] == self.tag for r in recs)
        # 2. the frontier is empty now (everything was donated away)

    def _donate_all(self):
        out = []
        while True:
            ptr, n = self.e.donate(4096)
            if n == 0:
                break
            self.kids.load(ptr, n * self.nsw)
            out.append(self.kids.host().reshape(n, self.nsw))
        return np.concatenate(out) if out else np.zeros((0, self.nsw), dtype=np.uint32)

    def _drain_outbox(self):
        ptr, n = self.e.outbox(0)
        recs = np.zeros((0, self.csw), dtype=np.uint32)
        if n:
            self.cands.load(ptr, n * self.csw)
            recs = self.cands.host().reshape(n, self.csw)
        self.e.commit(ptr, 0)  # hands nothing over: empties the outbox
        return recs

    def _counters(self):
        c = self.e.counters()
        return {f: getattr(c, f) for f in ("search_nodes", "gac_calls", "fails", "leaves", "skipped_revisions", "translation_stops")}

    def _expand(self, words, n):
        self.e.adopt(self.parents_buf.put(words), n)
        self.e.expand_local()
        return self._donate_all(), self._drain_outbox()

    def craft(self, index: int, expire, domains) -> list:
        """The record of parent `index` of a batch: `domains` in record form, the marker fixed to `index` at every point."""
        doms = list(domains)
        lo, hi = self.bounds[self.marker]
        assert 0 <= index <= hi - lo
        for p in range(self.K):
            doms[p * self.N + self.marker] = (lo + index, lo + index) if self.form == xr.INTERVALS else 1 << index
        words = encode(self.gid, self.tag, 0, list(expire), doms, self.N, self.K, self.form)
        xr.check(xr.decode(words, self.N, self.K, self.form, self.untils), self.bounds, self.K, self.form, self.untils)
        return words

    def _index_of(self, dom) -> int:
        lo = self.bounds[self.marker][0]
        if self.form == xr.INTERVALS:
            assert dom[0] == dom[1], dom
            return dom[0] - lo
        assert dom and dom & (dom - 1) == 0, hex(dom)
        return dom.bit_length() - 1

    def step(self, parents) -> list:
        """`parents`: [(expire words, domains in record form)]. One expansion each; returns one Outcome per parent and adds the
        step's skipped revisions to `self.skipped`."""
        n = len(parents)
        assert 0 < n <= self.bounds[self.marker][1] - self.bounds[self.marker][0] + 1
        words = [w for i, (expire, doms) in enumerate(parents) for w in self.craft(i, expire, doms)]
        before = self._counters()
        kids, cands = self._expand(words, n)                                    # 3. adopt, 4. one round, 5. donate, 6. / 7. outbox
        parked = [r for r in kids if int(r[4]) == SEED_NONE]
        kids = [r for r in kids if int(r[4]) != SEED_NONE]
        mid = self._counters()
        assert mid["gac_calls"] - before["gac_calls"] == n, (before, mid)
        assert mid["gac_calls"] - mid["search_nodes"] - (before["gac_calls"] - before["search_nodes"]) == len(parked), (before, mid, len(parked))
        if parked:  # leaves that waited for the translation of their set: expanded once more, from their fixpoint
            assert mid["translation_stops"] > before["translation_stops"]
            more_kids, more = self._expand(np.concatenate(parked), len(parked))
            assert len(more_kids) == 0 and len(more) == len(parked), (len(more_kids), len(more), len(parked))
            cands = np.concatenate([cands, more])
        after = self._counters()
        delta = {f: after[f] - before[f] for f in after}
        assert delta["search_nodes"] == n, delta
        assert len(kids) % 2 == 0 and delta["fails"] + delta["leaves"] + len(kids) // 2 == n, (delta, len(kids))
        assert delta["leaves"] == len(cands), (delta, len(cands))
        self.skipped += delta["skipped_revisions"]
        children = [[] for _ in range(n)]
        for r in kids:
            d = xr.decode(r, self.N, self.K, self.form, self.untils)
            xr.check(d, self.bounds, self.K, self.form, self.untils)
            assert (d["gid"], d["tag"]) == (self.gid, self.tag)
            children[self._index_of(d["domains"][self.marker])].append(d)
        leaf = [None] * n
        for r in cands:
            d = decode_candidate(r, self.N, self.K, self.form, self.sig_len, self.untils)
            assert d["gid"] == self.gid
            i = d["labels"][self.marker] - self.bounds[self.marker][0]
            assert 0 <= i < n and leaf[i] is None, i
            leaf[i] = d
        out = []
        for i in range(n):
            assert len(children[i]) in (0, 2) and not (children[i] and leaf[i]), (i, len(children[i]))
            if children[i]:
                out.append(Outcome("branch", children[i], None))
            else:
                out.append(Outcome("leaf", None, leaf[i]) if leaf[i] else Outcome("fail", None, None))
        assert sum(o.verdict == "fail" for o in out) == delta["fails"]
        return out

    def close(self):
        """The frontier and the outbox are empty: the search ends like any stepped one."""
        self.e.set_expand_budget(0, 0)
        assert self.e.expand_local() == 0
        self.e.finish()
        for buf in (self.parents_buf, self.kids, self.cands):
            buf.free()
        self.e.close()


# ------------------------------------------------------------------ rows
# style of a variable's words in a crafted parent:
#   "small"  / "wide": a few words of either point are restricted (`touch` of the time-0 words, half as many later ones), the
#            others keep the declared domain; a restricted word gets a sub-interval of at most 2 * `sub` values, half of them
#            ending on or straddling a 32-value chunk edge of the declared domain (bits 31 / 32, 63 / 64, 95 / 96) or, with a
#            `hint` range, drawn inside the hint
#   "always" every word restricted so (the default above 40 values: the yardstick enumerates whole products)
#   "keep"   the declared domain, always (auxiliary variables of the full int range)
#   "free"   an unconstrained variable: whole, a huge sub-interval, or one value
#   "pin"    one value, always
Row = namedtuple("Row", "name text k form flags family exact cons names style hint sub leafy batches size arrays strength design touch search")
ROWS = {}
V, C_ = (lambda n: ("v", n)), (lambda n: ("c", n))
P = lambda t: ("point", t)  # noqa: E731


def row(name, text, cons, names, k=2, form=2, family=None, exact=True, style=None, hint=None, sub=8, leafy=0.2, batches=3, size=48,
        arrays=None, strength="bounds", design=False, touch=0.45, search=False):
    flags = st.F_INTERVAL_DOMAINS if form == xr.INTERVALS else 0
    family = st.KF_WIDE_DOMAINS if family is None else family
    ROWS[name] = Row(name, text, k, form, flags, family, exact, cons, names, style or {}, hint or {}, sub, leafy, batches, size, arrays or {},
                     strength, design, touch, search)


def _add(a, b):
    return ("+", a, b)


def _mul(a, b):
    return ("*", a, b)


# ---- W = 2 (at most 64 values; the marker has 64)
row("w2_sum64", "var x:[-1,62]; var y:[0,40]; var s:[0,3]; var mk:[0,63]; x + s <= y; x >= 2 * s - 1;",
    [P(("<=", _add(V("x"), V("s")), V("y"))), P((">=", V("x"), ("-", _mul(C_(2), V("s")), C_(1))))], ["x", "y", "s", "mk"],
    style={"y": "wide"}, sub=12)
row("w2_fby_shift", "var v:[5,60]; var u:[0,3]; var w:[0,63]; var mk:[0,63]; w == (2 fby v); v >= 20 * u;",
    [P(("==", V("_V0"), C_(2))), P(("==", ("first", V("_V1")), ("first", V("_V0")))), ("arc", "v", "_V1"), P(("==", V("w"), V("_V1"))),
     P((">=", V("v"), _mul(C_(20), V("u"))))], ["v", "u", "w", "mk", "_V0", "_V1"], sub=10,
    style={"v": "wide", "w@1": "wide", "w@0": "keep", "_V1": "keep", "_V0": "keep"}, touch=0.6)
row("w2_until", "var x:[0,50]; var g:[0,1]; var y:[0,1]; var h:[0,1]; var mk:[0,63]; y == (x ge 25); g until y; h until g; x != 30;",
    [P(("==", V("y"), ("ge", V("x"), C_(25)))), ("until", "g", "y"), ("until", "h", "g"), P(("!=", V("x"), C_(30)))],
    ["x", "g", "y", "h", "mk"], hint={"x": (20, 34)}, sub=6, leafy=0.3)
row("w2_next_sum_k3", "var x:[0,20]; var y:[0,20]; var z:[0,40]; var mk:[0,63]; z == next (x + y); x + y <= 30;",
    [P(("==", V("_V0"), _add(V("x"), V("y")))), ("arc", "_V1", "_V0"), P(("==", V("z"), V("_V1"))), P(("<=", _add(V("x"), V("y")), C_(30)))],
    ["x", "y", "z", "mk", "_V0", "_V1"], k=3, sub=6, style={"z": "wide"})
row("w2_interpreted5", "var a:[0,63]; var b:[0,63]; var c:[0,63]; var d:[0,63]; var e:[0,63]; var mk:[0,63]; a + b <= c * d + e; a >= b - e;",
    [P(("<=", _add(V("a"), V("b")), _add(_mul(V("c"), V("d")), V("e")))), P((">=", V("a"), ("-", V("b"), V("e"))))],
    ["a", "b", "c", "d", "e", "mk"], style={"c": "pin", "d": "pin", "e": "pin"}, hint={"c": (3, 9), "d": (4, 7), "a": (10, 63), "b": (5, 45)}, sub=10)
# ---- W = 4 (at most 128 values)
row("w4_edge128", "var x:[-1,126]; var y:[0,5]; var t:[0,120]; var mk:[0,127]; x + y <= t; t <= x + 60;",
    [P(("<=", _add(V("x"), V("y")), V("t"))), P(("<=", V("t"), _add(V("x"), C_(60))))], ["x", "y", "t", "mk"], form=4, sub=12, style={"t": "wide"})
row("w4_fby_shift", "var v:[10,126]; var u:[0,3]; var w:[-1,126]; var mk:[0,127]; w == (-1 fby v); v >= 30 * u + 10;",
    [P(("==", V("_V0"), C_(-1))), P(("==", ("first", V("_V1")), ("first", V("_V0")))), ("arc", "v", "_V1"), P(("==", V("w"), V("_V1"))),
     P((">=", V("v"), _add(_mul(C_(30), V("u")), C_(10))))], ["v", "u", "w", "mk", "_V0", "_V1"], form=4, sub=10,
    style={"v": "wide", "w@1": "wide", "w@0": "keep", "_V1": "keep", "_V0": "keep"})
row("w4_interpreted5", "var a:[0,99]; var b:[0,99]; var c:[0,99]; var d:[0,99]; var e:[0,99]; var mk:[0,127]; a + b <= c * d + e; a >= b - e;",
    [P(("<=", _add(V("a"), V("b")), _add(_mul(V("c"), V("d")), V("e")))), P((">=", V("a"), ("-", V("b"), V("e"))))],
    ["a", "b", "c", "d", "e", "mk"], form=4, style={"c": "pin", "d": "pin", "e": "pin"}, hint={"c": (3, 12), "d": (4, 9), "a": (20, 99), "b": (10, 70)}, sub=10)
# ---- intervals (any width; the marker has 301 values, batches stay at 64 parents)
IV = xr.INTERVALS
row("iv_wide", "var x:[-100,400]; var y:[0,300]; var s:[0,3]; var mk:[0,300]; x + s <= y; x >= 2 * s - 1;",
    [P(("<=", _add(V("x"), V("s")), V("y"))), P((">=", V("x"), ("-", _mul(C_(2), V("s")), C_(1))))], ["x", "y", "s", "mk"], form=IV,
    hint={"x": (120, 170), "y": (125, 175)}, sub=12)
row("iv_def_div_mod", "var f:[-2147483648,2147483647]; var v:[-1000,1000]; var a:[-3,3]; var b:[-3,3]; var c:[1,4]; var mk:[0,300]; "
    "v == a * b + c; v / c >= a; (v % c) != 1; a -> b;",
    [P(("==", V("v"), _add(_mul(V("a"), V("b")), V("c")))), P((">=", ("/", V("v"), V("c")), V("a"))), P(("!=", ("%", V("v"), V("c")), C_(1))),
     P(("->", V("a"), V("b")))], ["f", "v", "a", "b", "c", "mk"], form=IV, style={"f": "free", "v": "wide"}, hint={"v": (-10, 14)}, sub=9)
row("iv_next_def_k3", "var x:[0,200]; var y:[0,200]; var z:[0,400]; var mk:[0,300]; z == next (x + y); x + y <= 300;",
    [P(("==", V("_V0"), _add(V("x"), V("y")))), ("arc", "_V1", "_V0"), P(("==", V("z"), V("_V1"))), P(("<=", _add(V("x"), V("y")), C_(300)))],
    ["x", "y", "z", "mk", "_V0", "_V1"], k=3, form=IV, sub=6, style={"z": "wide", "_V0": "wide", "_V1": "wide"},
    hint={"x": (120, 145), "y": (120, 145), "z": (240, 290), "_V0": (240, 290), "_V1": (240, 290)}, touch=0.15)
row("iv_until", "var x:[0,500]; var g:[0,1]; var y:[0,1]; var h:[0,1]; var mk:[0,300]; y == (x ge 250); g until y; h until g; x != 300;",
    [P(("==", V("y"), ("ge", V("x"), C_(250)))), ("until", "g", "y"), ("until", "h", "g"), P(("!=", V("x"), C_(300)))],
    ["x", "g", "y", "h", "mk"], form=IV, hint={"x": (244, 304)}, sub=6, leafy=0.3, touch=0.6)
row("iv_int_edges", "var a:[2147482700,2147483647]; var b:[-2147483648,-2147482800]; var s:[0,3]; var mk:[0,300]; "
    "a + s > 0; b - s < 0; a - 2147483600 >= 9 * s; b + 2147483647 <= 40 - s;",
    [P((">", _add(V("a"), V("s")), C_(0))), P(("<", ("-", V("b"), V("s")), C_(0))), P((">=", ("-", V("a"), C_(2147483600)), _mul(C_(9), V("s")))),
     P(("<=", _add(V("b"), C_(2147483647)), ("-", C_(40), V("s"))))], ["a", "b", "s", "mk"], form=IV,
    hint={"a": (INT_MAX - 60, INT_MAX), "b": (INT_MIN, INT_MIN + 60)}, sub=12)
# the device is weaker here by a stated choice (DESIGN, "Node-level seam"): `z == _V1` with _V1 of the whole int range is an image
# pass over 2^32 values, which is skipped, and a bound scan from INT_MIN, which gives up after kIvScanLanes candidates
row("iv_aux_full_next", "var x:[-6,6]; var y:[-3,3]; var z:[-9,200]; var mk:[0,300]; z == next (x / y); next x == x % 5 + y;",
    [P(("==", V("_V0"), ("/", V("x"), V("y")))), ("arc", "_V1", "_V0"), P(("==", V("z"), V("_V1"))), ("arc", "_V2", "x"),
     P(("==", V("_V2"), _add(("%", V("x"), C_(5)), V("y"))))], ["x", "y", "z", "mk", "_V0", "_V1", "_V2"], form=IV, exact=False, design=True,
    style={"_V0": "keep", "_V1": "keep", "z": "wide"}, hint={"z": (-8, 8)}, sub=6)
# budget rows: a bound that has to move past more candidates than one revision scans
row("iv_scan_serial", "var a:[0,5000]; var s:[0,3]; var mk:[0,300]; a >= 100 * s + 70;",
    [P((">=", V("a"), _add(_mul(C_(100), V("s")), C_(70))))], ["a", "s", "mk"], form=IV, exact=False, style={"a": "low", "s": "small"}, batches=2)
row("iv_scan_lanes", "var a:[0,5000]; var s:[0,3]; var mk:[0,300]; a >= 1000 * s + 1100;",
    [P((">=", V("a"), _add(_mul(C_(1000), V("s")), C_(1100))))], ["a", "s", "mk"], form=IV, exact=False, style={"a": "low", "s": "pin"}, batches=2)


# ---- W = 1: the seam itself against Engine.propagate, stcsp_fmodel_propagate and the yardstick in gac mode
def _partialorder(n):
    names = ["succ", "giveTo"] + [f"seen{i}" for i in range(n)] + ["mk"]
    text = "var succ:[0,1]; var giveTo:[0,9]; " + "".join(f"var seen{i}:[0,1]; " for i in range(n)) + "var mk:[0,31]; first giveTo < 4; "
    cons = [P(("<", ("first", V("giveTo")), C_(4)))]
    for i in range(n):
        text += f"first seen{i} == 0; next seen{i} == seen{i} or (giveTo eq {i}); "
        cons += [P(("==", ("first", V(f"seen{i}")), C_(0))), ("arc", f"_V{i}", f"seen{i}"),
                 P(("==", V(f"_V{i}"), ("or", V(f"seen{i}"), ("eq", V("giveTo"), C_(i)))))]
    conj = V("seen0")
    for i in range(1, n):
        conj = ("and", conj, V(f"seen{i}"))
    text += "first succ == 0; succ >= (" + " and ".join(f"seen{i}" for i in range(n)) + "); next succ >= succ;"
    cons += [P(("==", ("first", V("succ")), C_(0))), P((">=", V("succ"), conj)), ("arc", f"_V{n}", "succ"), P((">=", V(f"_V{n}"), V("succ")))]
    return text, cons, names + [f"_V{i}" for i in range(n + 1)]


def _synthetic(n_vars, dom, n_point, n_next, seed, tight=300):
    """instances.synthetic, replayed from the same generator: its text plus one unconstrained marker, and the trees and arrays."""
    rng = st.instances.SplitMix64(seed)
    pairs, cons, arrays, names = set(), [], {}, [f"x{i}" for i in range(n_vars)] + ["mk"]
    lines = [f"var x{i}:[0,{dom - 1}];" for i in range(n_vars)] + ["var mk:[0,31];"]
    body = []

    def table(k):
        arrays[f"T{k}"] = [0 if rng.below(1000) < tight else 1 for _ in range(dom * dom)]
        lines.append(f"arr T{k} : {{" + ", ".join(map(str, arrays[f"T{k}"])) + "};")

    k = 0
    while k < n_point:
        a, b = rng.below(n_vars), rng.below(n_vars)
        if a == b or (a, b) in pairs or (b, a) in pairs:
            continue
        pairs.add((a, b))
        table(k)
        body.append(f"T{k}[x{a} * {dom} + x{b}] == 1;")
        cons.append(P(("==", ("arr", f"T{k}", _add(_mul(V(f"x{a}"), C_(dom)), V(f"x{b}"))), C_(1))))
        k += 1
    used = set()
    while len(used) < n_next:
        a, b = rng.below(n_vars), rng.below(n_vars)
        if b in used:
            continue
        aux = f"_V{len(used)}"
        used.add(b)
        table(k)
        body.append(f"T{k}[x{a} * {dom} + next x{b}] == 1;")
        cons += [("arc", aux, f"x{b}"), P(("==", ("arr", f"T{k}", _add(_mul(V(f"x{a}"), C_(dom)), V(aux))), C_(1)))]
        names.append(aux)
        k += 1
    return "\n".join(lines + body) + "\n", cons, names, arrays


def _many_until(u, top=31):
    """test_many_until.many_until(u) with the marker in place of its free booleans."""
    from test_many_until import many_until
    text = many_until(u).replace("g0 until", "var mk:[0,31]; g0 until", 1)
    names = ["p", "_V0"] + [f"y{b}" for b in range(32)] + [f"g{a}" for a in range((u + 31) // 32)] + ["mk"]
    cons = [P(("==", ("first", V("p")), C_(0))), ("arc", "_V0", "p"),
            P(("==", V("_V0"), ("if", ("lt", V("p"), C_(top)), _add(V("p"), C_(1)), C_(0))))]
    cons += [P(("==", V(f"y{b}"), ("eq", V("p"), C_(b * top // 31)))) for b in range(32)]
    cons += [("until", f"g{i // 32}", f"y{(i + 5 * (i // 32)) % 32}") for i in range(u)]
    return text, cons, names


_t, _c, _n = _partialorder(10)
row("w1_partialorder_10", _t, _c, _n, form=1, family=st.KF_VARIANT, strength="gac", size=32, leafy=0.3, touch=0.2)
_t, _c, _n, _a = _synthetic(16, 8, 80, 4, 20261003)
row("w1_synth80", _t, _c, _n, form=1, family=st.KF_VARIANT, strength="gac", size=32, arrays=_a, leafy=0.15, touch=0.12, search=True)
_t, _c, _n = _many_until(40)
row("w1_until_uw2", _t, _c, _n, form=1, family=st.KF_UNTIL_HEAVY, strength="gac", size=32, leafy=0.3, touch=0.05, style={"p": "wide", "_V0": "keep"})


def n_untils(r: Row) -> int:
    return sum(c[0] == "until" for c in r.cons)


def sig_vars(r: Row) -> list:
    return sorted({r.names.index(c[1]) for c in r.cons if c[0] == "arc"})


def declared(r: Row, model=None) -> list:
    """The declared bounds per variable, from the model the front end built."""
    m = model or st.Model(text=r.text, prefix_k=r.k)
    assert m.var_names == r.names, (m.var_names, r.names)
    return m.var_bounds()


# ------------------------------------------------------------------ parents
EDGES = (31, 32, 63, 64, 95, 96)


def _sub_interval(rng, lo, hi, sub, hint):
    n = hi - lo + 1
    w = min(n, rng.choice([1, 1, 2, 3, 5, sub, 2 * sub]))
    if hint:
        h0, h1 = max(lo, hint[0]), min(hi, hint[1])
        a = rng.randint(h0, max(h0, h1 - w + 1))
    else:
        edges = [e for e in EDGES if e < n]
        if edges and rng.random() < 0.5:  # ends on the edge bit, starts on it, or straddles it
            a = lo + rng.choice(edges) - rng.randrange(w)
        else:
            a = lo + rng.randrange(n - w + 1)
    a = min(max(a, lo), hi - w + 1)
    return a, a + w - 1


def _draw(rng, r: Row, name, p, lo, hi, leaf_word):
    """A style or a hint may be given for one point alone, as "name@p"."""
    n = hi - lo + 1
    style = r.style.get(f"{name}@{p}", r.style.get(name, "wide" if n <= 40 else "always"))
    hint = r.hint.get(f"{name}@{p}", r.hint.get(name))
    if style == "keep":
        return lo, hi
    if style == "free":
        k = rng.randrange(3)
        if k == 0 and not leaf_word:
            return lo, hi
        if k == 1 and not leaf_word:
            a = rng.randint(lo, hi - 1)
            return a, rng.randint(a + 1, hi)
        a = rng.choice([lo, hi, rng.randint(lo, hi)])
        return a, a
    if style == "low":  # [lo, something]: the bound that must move is the declared one
        return (lo, rng.choice([150, 200, 1500, 4000, hi])) if not leaf_word else (rng.choice([70, 170, 1100, 2100, 3100, 4100, 3000]),) * 2
    if style == "pin" or leaf_word:
        a = rng.randint(max(lo, hint[0]), min(hi, hint[1])) if hint else rng.randint(lo, hi)
        return a, a
    if style != "always" and rng.random() >= (r.touch if p == 0 else r.touch / 2):
        return lo, hi
    return _sub_interval(rng, lo, hi, r.sub, hint)


def _as_domain(r: Row, a, b):
    return (a, b) if r.form == xr.INTERVALS else set(range(a, b + 1))


_found = {}


def search_leaves(r: Row, bounds, want=6, budget=3000) -> list:
    """Time-0 assignments of consistent leaves of the declared block, by a depth-first search over the yardstick's fixpoints
    (smallest domain first): for a model so tight that a guided walk reaches none (the synthetic family is near its phase
    transition). Only the parents of such a row are drawn from it; what a parent's fixpoint is remains the yardstick's word."""
    if r.name not in _found:
        N, mk = len(r.names), r.names.index("mk")
        found, nodes = [], [0]
        start = [set(range(bounds[i % N][0], bounds[i % N][1] + 1)) for i in range(N * r.k)]
        for p in range(r.k):
            start[p * N + mk] = {bounds[mk][0]}

        def dfs(doms):
            if len(found) >= want or nodes[0] > budget:
                return
            nodes[0] += 1
            ok, fp = br.propagate(r.cons, r.names, doms, 0, r.k, r.strength, r.arrays)
            if not ok:
                return
            open_ = [v for v in range(N) if len(fp[v]) > 1]
            if not open_:
                found.append([min(fp[v]) for v in range(N)])
                return
            v = min(open_, key=lambda v: len(fp[v]))
            for a in sorted(fp[v]):
                d = list(fp)
                d[v] = {a}
                dfs(d)

        dfs(start)
        _found[r.name] = found
    return _found[r.name]


def make_parents(r: Row, bounds, count: int, seed: int) -> list:
    """[(expire as one integer, domains)]: yardstick domains (sets / pairs; the marker's words hold the parent's index, which
    `craft` writes again). A fifth or so are `leafy`: every declared time-0 variable fixed, and the auxiliary ones to a value of the
    yardstick's fixpoint of that block, so that leaves are met."""
    rng = random.Random(seed)
    N, nu = len(r.names), n_untils(r)
    mk = r.names.index("mk")
    out = []
    while len(out) < count:
        leafy = rng.random() < r.leafy
        doms = []
        for p in range(r.k):
            for v, name in enumerate(r.names):
                lo, hi = bounds[v]
                if v == mk:
                    doms.append(_as_domain(r, lo + len(out), lo + len(out)))  # the parent's index in its batch
                elif (name.startswith("_V") and not any(key.split("@")[0] == name for key in (*r.style, *r.hint)) and rng.random() < 0.7):
                    doms.append(_as_domain(r, lo, hi))
                else:
                    doms.append(_as_domain(r, *_draw(rng, r, name, p, lo, hi, False)))
        expire = rng.getrandbits(nu) if nu else 0
        if nu > 32 and rng.random() < 0.5:
            expire |= (1 << 3) | (1 << 37)  # bits of both words
        if leafy:  # fix the time-0 variables one after the other, mostly to a value the yardstick still holds possible
            pool = search_leaves(r, bounds) if r.search else []
            if pool:
                leaf = rng.choice(pool)
                for v in range(N):
                    if v != mk:
                        doms[v] = {leaf[v]}
            wild = rng.random() < 0.25  # ... a quarter of them with a value or two drawn from the parent's own domains instead
            start = list(doms)
            for attempt in range(12):  # (a tight model: the walk may run into a wipe-out; the last attempt stays, failed or not)
                doms = list(start)
                for v in range(N):
                    if v == mk:
                        continue
                    ok, fp = br.propagate(r.cons, r.names, doms, expire, r.k, r.strength, r.arrays)
                    d = doms[v] if not ok or (wild and rng.random() < 2 / N) else fp[v]
                    if br.d_size(d) > 1:
                        a = rng.choice(list(br.d_values(d))) if br.d_size(d) <= 4096 else rng.choice([br.d_lo(d), br.d_hi(d), rng.randint(br.d_lo(d), br.d_hi(d))])
                        doms[v] = _as_domain(r, a, a)
                    elif d is not doms[v]:
                        doms[v] = _as_domain(r, br.d_lo(d), br.d_lo(d))
                if wild or br.propagate(r.cons, r.names, doms, expire, r.k, r.strength, r.arrays)[0]:
                    break
        out.append((expire, doms))
    return out


def expire_list(expire: int, n_until_cons: int) -> list:
    return [(expire >> (32 * j)) & 0xFFFFFFFF for j in range(xr.expire_words(n_until_cons))]


_yard = {}


def yardstick(r: Row, bounds, batch: int):
    """The parents of one batch of a row and what the yardstick makes of each: [(expire, domains, ok, fixpoint, class)], once."""
    key = (r.name, batch)
    if key not in _yard:
        t0 = time.perf_counter()
        out = []
        for expire, doms in make_parents(r, bounds, r.size, 20261021 + 1000 * batch + sum(map(ord, r.name))):
            ok, fp = br.propagate(r.cons, r.names, doms, expire, r.k, r.strength, r.arrays)
            out.append((expire, doms, ok, fp, br.classify(ok, fp, len(r.names))))
        _yard[key] = (out, time.perf_counter() - t0)
    return _yard[key]
