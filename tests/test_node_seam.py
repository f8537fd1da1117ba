"""The CPU side of the node-level seam (tests/node_seam.py): the record coding, the rows' stated constraint lists against the front
end, every crafted parent against xfer_ref.check, and the seeded parents of every exact row against the thresholds that keep the
GPU comparison from being degenerate -- judged by the yardstick alone. Prints the mix and the yardstick's time per row (the table
of DESIGN, "Node-level seam"). No GPU."""
import random

import pytest

import bounds_ref as br
import node_seam as ns
import xfer_ref as xr

FORMS = (1, 2, 4, xr.INTERVALS)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("uw", [1, 2, 3, 4])
def test_encode_then_decode_is_the_identity(form, uw):
    rng = random.Random(100 * form + uw)
    n_until_cons = {1: 7, 2: 40, 3: 70, 4: 124}[uw]
    for n_vars, k in ((1, 1), (3, 2), (5, 3), (33, 2)):
        doms = []
        for _ in range(n_vars * k):
            if form == xr.INTERVALS:
                a = rng.choice([ns.INT_MIN, -5, 0, ns.INT_MAX - 3])
                doms.append((a, rng.randint(a, ns.INT_MAX)))
            else:
                doms.append(rng.randint(1, (1 << (32 * form)) - 1) | 1 << (32 * form - 1) * rng.randrange(2))
        expire = [rng.getrandbits(32) for _ in range(uw)]
        expire[-1] &= (1 << (n_until_cons - 32 * (uw - 1))) - 1
        gid, tag, seed = rng.getrandbits(40), rng.getrandbits(32), rng.choice([0, 1, n_vars * k + 1, ns.SEED_NONE])
        words = ns.encode(gid, tag, seed, expire, doms, n_vars, k, form)
        assert len(words) == xr.stride(n_vars, k, form) and all(0 <= w < 1 << 32 for w in words)
        d = xr.decode(words, n_vars, k, form, n_until_cons)
        assert (d["gid"], d["tag"], d["seed"], d["expire"], d["domains"]) == (gid, tag, seed, expire, doms)
        assert all(x == 0 for x in d["beyond"])
        # and the other way round: the record of what was decoded is the record
        assert ns.encode(d["gid"], d["tag"], d["seed"], d["expire"], d["domains"], n_vars, k, form) == words


def test_masks_are_relative_to_the_declared_lower_bound():
    assert ns.to_mask({-1, 0, 62}, -1) == 1 | 2 | 1 << 63
    assert ns.from_mask(1 << 127 | 1 << 32, -1) == {31, 126}
    bounds = [(-1, 126), (0, 3)]
    doms = [{-1, 126}, {2}, {30, 31}, {0, 3}]
    rec = ns.to_record_domains(doms, bounds, 4)
    assert rec == [1 | 1 << 127, 4, 3 << 31, 9] and ns.from_record_domains(rec, bounds, 4) == doms


def test_candidate_decoder_reads_the_documented_layout():
    n, k, form, sig, nu = 3, 2, 2, 2, 40  # [8 header][2 signature][3 labels][3 * 2 * 2 block][1 expire word]
    assert ns.cand_stride(n, k, form, sig, nu) == (8 + 2 + 3 + 12 + 1 + 3) & ~3
    rec = [0] * ns.cand_stride(n, k, form, sig, nu)
    rec[0], rec[1], rec[2], rec[3] = 5, 1, 77, 0x80000001
    rec[8:10] = [9, 0xFFFFFFFF]
    rec[10:13] = [0xFFFFFFFE, 4, 0]
    rec[13:25] = [1, 2, 4, 8, 16, 32, 1, 0, 0, 0, 0, 3]  # chunk 0 of the six words, then chunk 1
    rec[25] = 0x21
    d = ns.decode_candidate(rec, n, k, form, sig, nu)
    assert (d["gid"], d["tag"], d["signature"], d["labels"], d["expire"]) == (5 | 1 << 32, 77, [9, -1], [-2, 4, 0], [0x80000001, 0x21])
    assert d["domains"] == [1 | 1 << 32, 2, 4, 8, 16, 32 | 3 << 32]


@pytest.mark.parametrize("name", list(ns.ROWS))
def test_rows_state_what_the_front_end_normalises_to(stcsp, name):
    """The yardstick reads the row's own list of trees, arcs and untils, never the text: here the list is held against the parsed
    text, constraint by constraint, and the variable order (auxiliary variables included) with it."""
    r = ns.ROWS[name]
    m = stcsp.Model(text=r.text, prefix_k=r.k)
    assert m.var_names == r.names
    assert [m.constraint_string(i) for i in range(m.n_constraints)] == [br.show(c) for c in r.cons]
    bounds = m.var_bounds()
    widest = max(hi - lo + 1 for lo, hi in bounds)
    assert {1: widest <= 32, 2: 32 < widest <= 64, 4: 64 < widest <= 128, xr.INTERVALS: widest > 128}[r.form], (r.form, widest)
    lo, hi = bounds[r.names.index("mk")]
    assert r.names.index("mk") == max(i for i, v in enumerate(r.names) if not v.startswith("_V"))  # declared last
    assert hi - lo + 1 >= r.size and r.size <= 64 and 2 <= r.batches <= 4
    assert all("mk" not in br.scope_of(c[1]) for c in r.cons if c[0] == "point") and all("mk" not in c[1:] for c in r.cons if c[0] != "point")


def test_three_quarters_of_the_rows_are_exact():
    rows = list(ns.ROWS.values())
    assert sum(r.exact for r in rows) * 4 >= 3 * len(rows)
    for form in FORMS:
        assert sum(1 for r in rows if r.form == form and not r.exact and not r.design) <= 2
    assert [r.name for r in rows if r.design] == ["iv_aux_full_next"]  # the one row that is weaker by a stated choice, by name


@pytest.mark.parametrize("name", list(ns.ROWS))
def test_parents_are_well_formed_and_the_sample_is_not_degenerate(stcsp, name):
    r = ns.ROWS[name]
    m = stcsp.Model(text=r.text, prefix_k=r.k)
    bounds = ns.declared(r, m)
    nu, N = ns.n_untils(r), len(r.names)
    mix = {"fail": 0, "branch": 0, "leaf": 0, "moved": 0}
    seconds = 0.0
    both_words = False
    for b in range(r.batches):
        entries, t = ns.yardstick(r, bounds, b)
        seconds += t
        assert len(entries) == r.size
        for i, (expire, doms, ok, fp, cls) in enumerate(entries):
            words = ns.encode(1 << 32 | 7, 12345, 0, ns.expire_list(expire, nu), ns.to_record_domains(doms, bounds, r.form), N, r.k, r.form)
            d = xr.decode(words, N, r.k, r.form, nu)
            xr.check(d, bounds, r.k, r.form, nu)  # no empty domain, no bit outside the declared domain, no foreign expire bit
            assert ns.from_record_domains(d["domains"], bounds, r.form) == [x if br.is_pair(x) else set(x) for x in doms]
            assert all(br.d_lo(doms[p * N + r.names.index("mk")]) == bounds[r.names.index("mk")][0] + i for p in range(r.k))
            both_words = both_words or (nu > 32 and expire & 0xFFFFFFFF and expire >> 32)
            mix[cls[0]] += 1
            mix["moved"] += cls[0] == "branch" and fp != doms
    total = r.size * r.batches
    print(f"{name}: {total} parents, fail {mix['fail']} branch {mix['branch']} leaf {mix['leaf']}, branch parents pruned {mix['moved']}, "
          f"yardstick {seconds:.2f} s")
    if nu > 32:
        assert both_words
    if r.exact:
        assert mix["fail"] * 100 >= 15 * total, mix
        assert mix["branch"] * 100 >= 15 * total, mix
        assert mix["leaf"] >= 3, mix
        assert mix["moved"] * 100 >= 30 * mix["branch"], mix
    else:
        assert mix["branch"] + mix["leaf"] > 0 and mix["leaf"] > 0, mix
