"""Worker for the multi-process tests of the sharded driver (one process per shard)."""
import ctypes as C
import importlib
import json
import os
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))


def load_model(st, spec, prefix_k=2):
    """`spec`: an instance name, "file:<path to a .csp>" or "synth:n,d,m,s,seed" (instances.synthetic)."""
    if spec.startswith("file:"):
        return st.Model(text=Path(spec[5:]).read_text(), prefix_k=prefix_k)
    if spec.startswith("synth:"):
        n, d, m, s, seed = (int(x) for x in spec[6:].split(","))
        return st.Model(text=st.instances.synthetic(n, d, m, s, seed), prefix_k=prefix_k)
    return st.Model.from_name(spec, prefix_k=prefix_k)


class Faulty:
    """Fault injection for the failure-protocol tests: the wrapped engine raises at the n-th call of one method
    (STCSP_TEST_FAULT="method,rank[,n]"); everything else passes through."""

    def __init__(self, eng, method, nth):
        self._eng, self._method, self._nth, self._seen = eng, method, nth, 0

    def __getattr__(self, name):
        attr = getattr(self._eng, name)
        if name != self._method:
            return attr

        def boom(*a, **k):
            self._seen += 1
            if self._seen >= self._nth:
                raise RuntimeError(f"injected fault in {name}")
            return attr(*a, **k)

        return boom


class Tally:
    """Counts the candidate records an engine commits and the ones it addressed to itself, so that a run can say how many
    came from its peers; everything else passes through."""

    def __init__(self, eng, rank):
        self._eng, self._rank, self.committed, self.to_self = eng, rank, 0, 0

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def outbox(self, peer):
        ptr, n = self._eng.outbox(peer)
        if peer == self._rank:
            self.to_self += n
        return ptr, n

    def commit(self, ptr, count):
        self.committed += count
        return self._eng.commit(ptr, count)


def mixed_layout(backend_kind, world):
    """"mixed:<layout>": one letter per rank, `h` the HIP engine on GPU 0 (staged through the host), `f` the frontier model."""
    layout = backend_kind[len("mixed:"):]
    if len(layout) != world or set(layout) - set("hf") or layout.count("h") > 1:
        raise ValueError(f"mixed layout {layout!r}: one letter of 'h' / 'f' per rank ({world}), at most one 'h'")
    return layout


def agree_on_strides(dist, torch, eng, world):
    """Every rank's (candidate_bytes, node_bytes): unequal record strides would desynchronise the all-to-all, so every rank
    raises together, with both numbers."""
    mine = torch.tensor([eng.candidate_bytes(), eng.node_bytes()], dtype=torch.int64)
    everyone = torch.empty(2 * world, dtype=torch.int64)
    dist.all_gather_into_tensor(everyone, mine)
    strides = everyone.view(world, 2).tolist()
    if any(s != strides[0] for s in strides):
        raise RuntimeError(f"record strides differ between the ranks: (candidate_bytes, node_bytes) = {strides}")
    return strides


def run(rank, world, port, name, backend_kind, out_path, prefix_k=2):
    # redistribution knobs for the tests (small instances must share early to exercise the path)
    budget = dict(budget_rounds=int(os.environ.get("STCSP_TEST_BUDGET_ROUNDS", "8")),
                  share_per_rank=int(os.environ.get("STCSP_TEST_SHARE", "64")))
    stats = {}
    if os.environ.get("STCSP_TEST_STACKS_AFTER"):
        # the launcher kills every rank at its time limit; shortly before, a rank that is still here writes where it stands
        # (which engine call, which collective), which is what tells a rank alone in a collective from a busy engine
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["STCSP_TEST_STACKS_AFTER"]), exit=False, file=sys.stdout)
    import torch
    import torch.distributed as dist

    st = importlib.import_module("stcsp-solver_amd")
    sh = importlib.import_module("stcsp-solver_amd.sharded")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if backend_kind == "hip-nccl":
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda:0"))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    m = load_model(st, name, prefix_k)
    mine_kind = backend_kind
    if backend_kind.startswith("mixed:"):
        mine_kind = {"h": "hip", "f": "fmodel"}[mixed_layout(backend_kind, world)[rank]]
        if mine_kind == "hip":  # one expansion per slot and round: the frontier is wide when expand_local hands control back
            os.environ["STCSP_CHAIN_SMALL"] = os.environ["STCSP_CHAIN_BIG"] = "1"
    tally = None
    if mine_kind == "fmodel":
        # CPU stand-in for the HIP engine (tests only): oracle/frontier_model.cpp
        lib = C.CDLL(str(REPO / "oracle" / "libstcsp_oracle.so"))
        st.bind_engine_api(lib, "stcsp_fmodel")

        class FModel(st.EngineBase):
            _prefix = "stcsp_fmodel"

            def __init__(self, model, **o):
                super().__init__(lib, model, **o)

        eng = FModel(m, rank=rank, world=world)
        if os.environ.get("STCSP_TEST_PRETRANSLATE") == str(rank):
            # this rank translates constraint sets ahead of need, with the HIP engine's limits, as that engine does when it is
            # created: it starts from a larger set registry than its peers
            lib.stcsp_fmodel_pretranslate.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
            assert lib.stcsp_fmodel_pretranslate(eng._h, 65536, 16384, None, None, None) > 0
        fault = os.environ.get("STCSP_TEST_FAULT")
        if fault:
            f = fault.split(",")
            if int(f[1]) == rank:
                eng = Faulty(eng, f[0], int(f[2]) if len(f) > 2 else 1)
        device = torch.device("cpu")
        if backend_kind != mine_kind:
            strides = agree_on_strides(dist, torch, eng, world)
            eng = tally = Tally(eng, rank)
        rounds = sh.solve_sharded(eng, rank, world, device, stats=stats, **budget)
    elif backend_kind == "hip-nccl":
        # the production N>1 code path on one GPU: RCCL process group of size 1, candidates stay in
        # HBM (all_to_all_single on views of the engine's outbox), STCSP_F_STEPPED forces the
        # candidate/commit pipeline although world == 1
        import time
        assert world == 1
        eng = st.Engine(m, device=0, rank=0, world=1, flags=st.F_STEPPED)
        device = torch.device("cuda:0")
        rounds = sh.solve_sharded(eng, rank, world, device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rounds = sh.solve_sharded(eng, rank, world, device)
        torch.cuda.synchronize()
        stepped_ms = (time.perf_counter() - t0) * 1e3
    else:
        # the real HIP engine, every shard on GPU 0, all-to-all staged through host (gloo)
        eng = st.Engine(m, device=0, rank=rank, world=world, time_limit_s=float(os.environ.get("STCSP_TEST_TIME_LIMIT", "0")))
        device = torch.device("cuda:0")
        if backend_kind != mine_kind:
            strides = agree_on_strides(dist, torch, eng, world)
            eng = tally = Tally(eng, rank)
        rounds = sh.solve_sharded(eng, rank, world, device, stage_through_host=True, stats=stats, **budget)
    # every rank's own search-node count (tensor collective)
    ctr = eng.counters()
    row = [ctr.search_nodes, stats.get("nodes_donated", 0), stats.get("nodes_adopted", 0), ctr.skipped_revisions, ctr.fails,
           tally.committed if tally else 0, tally.to_self if tally else 0]
    choice = eng.kernel_choice() if mine_kind != "fmodel" else {}  # (the frontier model has no kernels)
    fields = [n for n, _ in st.KernelChoice._fields_]
    row += [choice.get(n, -1) for n in fields]
    mine = torch.tensor(row, dtype=torch.int64)
    everyone = torch.empty(len(row) * world, dtype=torch.int64)
    if backend_kind == "hip-nccl":
        mine, everyone = mine.cuda(), everyone.cuda()
    dist.all_gather_into_tensor(everyone, mine)
    everyone = everyone.cpu().view(world, len(row)).tolist()
    merged = sh.gather_and_merge(st, eng, rank, world, device)
    if rank == 0:
        h, res = merged
        a = st.Automaton(m, res).traverse().renumber()
        out = dict(states=a.n_live_states, edges=a.n_live_edges, sha=a.canonical_sha256(), rounds=rounds,
                   table=res.n_states, dom=res.counters.dominance, nodes=res.counters.search_nodes,
                   sets=res.n_constraint_sets, fails=res.counters.fails, rank_nodes=[e[0] for e in everyone],
                   donated=[e[1] for e in everyone], adopted=[e[2] for e in everyone], canonical=a.canonical() if a.n_states <= 4096 else None)
        # per rank: what it was, its own counters, and (HIP ranks) the kernels it chose
        kinds = [mine_kind] * world if backend_kind == mine_kind else [{"h": "hip", "f": "fmodel"}[c] for c in mixed_layout(backend_kind, world)]
        out.update(backend=kinds, rank_skipped_revisions=[e[3] for e in everyone], rank_fails=[e[4] for e in everyone],
                   kernel_choice=[dict(zip(fields, e[7:])) if k != "fmodel" else None for k, e in zip(kinds, everyone)])
        if tally:
            out.update(strides=strides, candidates_committed=[e[5] for e in everyone], candidates_to_self=[e[6] for e in everyone])
        if backend_kind == "hip-nccl":
            out["stepped_ms"] = stepped_ms
        if os.environ.get("STCSP_TEST_ADVERSARIAL"):
            # solverSolve's tail with -a (solveralgorithm.cpp:972-985) on the merged automaton
            b = st.Automaton(m, res).traverse()
            out["adver1"] = b.adversarial(5)
            b.renumber()
            out["adv_empty"] = b.canonical().endswith("EMPTY\n")
        Path(out_path).write_text(json.dumps(out))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    rank, world, port, name, kind, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5], sys.argv[6]
    run(rank, world, port, name, kind, out, prefix_k=int(sys.argv[7]) if len(sys.argv) > 7 else 2)
