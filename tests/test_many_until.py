"""More than 32 `until` constraints (the reference keeps one Constraint::expire per until constraint and one sticky flag per
until in the signature, src/constraint.h:43, src/solveralgorithm.cpp:820-835): the only limit on their number is the
state key's, 1 + n_sig + n_until_cons <= 126 words. Checked before any device is looked at (no GPU needed)."""
import pytest

N_SIG = 1  # the counter's `next` auxiliary variable


def many_until(u: int, top: int = 31, pad: int = 0, free: int = 0) -> str:
    """u `until` constraints whose flags expire at different times. A counter p runs over [0, top] and wraps; y_b is 1 when
    p is at b * top // 31 (b < 32). Until i (its ordinal) is `g_(i // 32) until y_((i + 5 (i // 32)) % 32)`, so g_1, g_2
    and g_3 are only held by ordinals of 32 and above: a node that sets one of them to 0 before its flags expire is refuted
    there. top > 31: a domain of more than 32 values (W = 2 or 4). pad: constant variables that grow the block. free:
    unconstrained booleans (a bushier search)."""
    t = f"var p:[0,{top}]; first p == 0; next p == (if (p lt {top}) then (p + 1) else 0); "
    t += "".join(f"var y{b}:[0,1]; y{b} == (p eq {b * top // 31}); " for b in range(32))
    t += "".join(f"var g{a}:[0,1]; " for a in range((u + 31) // 32))
    t += "".join(f"var z{i}:[0,0]; " for i in range(pad))
    t += "".join(f"var h{i}:[0,1]; " for i in range(free))
    t += "".join(f"g{i // 32} until y{(i + 5 * (i // 32)) % 32}; " for i in range(u))
    return t


def verdict(stcsp, text, **opts):
    """None when the engine takes the model (it may still find no device), else the refusal."""
    try:
        stcsp.Engine(stcsp.Model(text=text), **opts).close()
    except stcsp.StcspError as ex:
        return None if ex.code != -2 else ex
    return None


@pytest.mark.parametrize("u", [33, 64, 65, 97, 125 - N_SIG])
def test_many_until_constraints_are_not_refused(stcsp, u):
    assert verdict(stcsp, many_until(u)) is None


@pytest.mark.parametrize("flags", [0, "intervals"])
def test_many_until_constraints_any_domain_form(stcsp, flags):
    opts = {"flags": stcsp.F_INTERVAL_DOMAINS} if flags else {}
    assert verdict(stcsp, many_until(40, top=100), **opts) is None
    assert verdict(stcsp, many_until(70, pad=100)) is None  # a block of more than 256 words


def test_key_of_127_words_is_refused_naming_the_signature_limit(stcsp):
    ex = verdict(stcsp, many_until(126 - N_SIG))
    assert ex is not None and "125" in str(ex) and "126" in str(ex)
    assert "32" not in str(ex)
