"""Plain Python decoder of the transfer record of an open search node, from the layout in stcsp-solver_amd/csrc/device_types.hpp:

    [0,1] source state gid   [2] constraint-set tag   [3] until-expire word 0   [4] dirty seed
    [5..7] until-expire words 1..3 (0 beyond UW)      [8 .. 8 + N*K*W) the block, then padding to a multiple of 4 words

The block is chunk-major: word (c, p, v) = c * N*K + p * N + v. Bitset domains (W = 1, 2, 4): chunk c holds the values
lb[v] + 32 c .. lb[v] + 32 c + 31 of variable v at time point p, one bit each. Interval domains: chunk 0 is the lower bound
and chunk 1 the upper bound, as int32. No GPU, no numpy tricks: a record is a sequence of 32-bit words."""
XFER_HDR = 8
XFER_EXPIRE = 5
INTERVALS = 0  # KernelChoice.domain_form of interval domains (1, 2, 4 = W otherwise)


def chunks(form: int) -> int:
    return 2 if form == INTERVALS else form


def stride(n_vars: int, k: int, form: int) -> int:
    return (XFER_HDR + n_vars * k * chunks(form) + 3) & ~3


def expire_words(n_until_cons: int) -> int:
    return 1 if n_until_cons <= 32 else (n_until_cons + 31) // 32


def payload(rec, n_vars: int, k: int, form: int) -> tuple:
    """The words of a record that are specified: header and block, without the padding."""
    return tuple(int(w) for w in rec[: XFER_HDR + n_vars * k * chunks(form)])


def decode(rec, n_vars: int, k: int, form: int, n_until_cons: int) -> dict:
    w = [int(x) & 0xFFFFFFFF for x in rec]
    nk = n_vars * k
    uw = expire_words(n_until_cons)
    doms = []
    for p in range(k):
        for v in range(n_vars):
            at = XFER_HDR + p * n_vars + v
            if form == INTERVALS:
                lo, hi = w[at], w[at + nk]
                doms.append((lo - (1 << 32) if lo >> 31 else lo, hi - (1 << 32) if hi >> 31 else hi))
            else:
                doms.append(sum(w[at + c * nk] << (32 * c) for c in range(form)))
    return dict(gid=w[0] | w[1] << 32, tag=w[2], seed=w[4], expire=[w[3]] + w[XFER_EXPIRE: XFER_EXPIRE + uw - 1],
                beyond=w[XFER_EXPIRE + uw - 1: XFER_HDR], domains=doms)


def check(d: dict, bounds, k: int, form: int, n_until_cons: int) -> None:
    """What holds for every open node whatever the search did: every domain non-empty and inside the variable's initial one, no
    expire bit beyond the until constraints, header words past the last expire word zero, a seed that names a block word."""
    n = len(bounds)
    assert len(d["domains"]) == n * k
    for i, dom in enumerate(d["domains"]):
        lo, hi = bounds[i % n]
        if form == INTERVALS:
            assert lo <= dom[0] <= dom[1] <= hi, (i, dom, (lo, hi))
        else:
            assert dom != 0 and dom >> (hi - lo + 1) == 0, (i, hex(dom), (lo, hi))
    assert all(x == 0 for x in d["beyond"]), d["beyond"]
    bits = sum(e << (32 * j) for j, e in enumerate(d["expire"]))
    assert bits >> n_until_cons == 0, (hex(bits), n_until_cons)
    seed_none = (1 << 12) - 1  # kSeedNone: 32 - kSetBits = 12 bits of seed
    # 0: revise everything; 1 + a word of chunk 0: what the parent bisected; N*K + 1: a fresh state under its parent's set
    assert d["seed"] == seed_none or d["seed"] <= n * k + 1, d["seed"]
