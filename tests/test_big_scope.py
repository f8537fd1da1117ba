"""Constraints over more than 64 variables (the reference revises any scope, src/solveralgorithm.cpp:435-523): up to 256 are
compiled; 257 and more are refused with STCSP_E_UNSUPPORTED naming 256. Without a GPU the engine stops at "no HIP device" before it
compiles anything, so the compiler is observed through the scalar frontier model, which links the product's cset.cpp and
compiles the flat program when it is created. Scope = the distinct variables of the whole constraint."""
import ctypes as C

import pytest


def wide_and(n: int) -> str:
    """`d >= (x0 and ... and x_(n-1))` over a chain x_i <= x_(i+1): a scope of n + 1 variables."""
    t = "var d:[0,1]; " + "".join(f"var x{i}:[0,1]; " for i in range(n))
    t += "".join(f"x{i} <= x{i + 1}; " for i in range(n - 1))
    return t + "d >= (" + " and ".join(f"x{i}" for i in range(n)) + ");"


def const_sum(n: int) -> str:
    """A sum over 6 booleans and n - 6 constants (a product small enough for a tuple bitmap while n <= 64)."""
    t = "".join(f"var b{i}:[0,1]; " for i in range(6)) + "".join(f"var z{i}:[0,0]; " for i in range(n - 6))
    return t + "(" + " + ".join([f"b{i}" for i in range(6)] + [f"z{i}" for i in range(n - 6)]) + ") <= 3;"


def sum_le(n: int) -> str:
    """`x0 <= (x1 + ... + x_(n-1))` over n booleans."""
    t = "".join(f"var x{i}:[0,1]; " for i in range(n))
    return t + "x0 <= (" + " + ".join(f"x{i}" for i in range(1, n)) + ");"


def sizes(oracle_lib, f):
    out = (C.c_longlong * 11)()
    assert oracle_lib.stcsp_fmodel_program_sizes(f._h, out, 11) == 11
    return list(out)


@pytest.mark.parametrize("scope", [65, 70, 100, 200, 256])
def test_scopes_up_to_256_are_not_refused(stcsp, FrontierModel, scope):
    FrontierModel(stcsp.Model(text=wide_and(scope - 1))).close()
    FrontierModel(stcsp.Model(text=sum_le(scope))).close()


def test_scope_of_257_is_refused_naming_256(stcsp, FrontierModel):
    for text in (wide_and(256), sum_le(257)):
        with pytest.raises(stcsp.StcspError) as ex:
            FrontierModel(stcsp.Model(text=text))
        assert ex.value.code == -2 and "256" in str(ex.value) and "64" not in str(ex.value)


def test_scope_of_64_compiles_as_before(stcsp, oracle_lib, FrontierModel):
    """Section byte sizes [sets, sweep records, itemrows, wavefront items, scope, strides, code, cons, tables, transitions, direct
    tables], as the parent compiled them."""
    f = FrontierModel(stcsp.Model(text=wide_and(63)))
    assert sizes(oracle_lib, f) == [80, 2016, 2080, 96, 752, 0, 1504, 3528, 992, 0, 0]
    f.close()
    f = FrontierModel(stcsp.Model(text=const_sum(64)))  # tabulated: 64 strides, a two-word bitmap
    assert sizes(oracle_lib, f) == [80, 32, 520, 96, 256, 256, 524, 56, 8, 0, 0]
    f.close()


def test_big_scope_gets_no_tuple_table(stcsp, oracle_lib, FrontierModel):
    """The same sum over 65 variables has a product of 64 tuples but is interpreted: no strides, no table words."""
    f = FrontierModel(stcsp.Model(text=const_sum(65)))
    s = sizes(oracle_lib, f)
    assert s[4] == 65 * 4 and s[5] == 0 and s[8] == 0
    f.close()


def verdict(stcsp, text, prefix_k=2, **opts):
    """None when the engine takes the model (it may still find no device), else the refusal."""
    try:
        stcsp.Engine(stcsp.Model(text=text, prefix_k=prefix_k), **opts).close()
    except stcsp.StcspError as ex:
        return None if ex.code != -2 else ex
    return None


def test_big_scope_with_interval_domains_is_refused(stcsp):
    """(An interval block of 256 words holds 128 variables at K = 1.)"""
    ex = verdict(stcsp, wide_and(70), prefix_k=1, flags=stcsp.F_INTERVAL_DOMAINS)
    assert ex is not None and "interval" in str(ex) and "71" in str(ex)
    assert verdict(stcsp, wide_and(63), prefix_k=1, flags=stcsp.F_INTERVAL_DOMAINS) is None


def test_big_scope_with_more_than_32_until_constraints_is_refused(stcsp):
    text = wide_and(70) + "".join(f"var g{i}:[0,1]; g{i} until d; " for i in range(33))
    ex = verdict(stcsp, text)
    assert ex is not None and "until" in str(ex) and "32" in str(ex)
    assert verdict(stcsp, wide_and(70) + "".join(f"var g{i}:[0,1]; g{i} until d; " for i in range(32))) is None
