"""The block limit of the bitset engines, checked before any device is looked at (no GPU needed): N*K*W <= 512 words is
accepted for its size, 513 and more is refused with STCSP_E_UNSUPPORTED naming the limit. Interval blocks keep theirs."""
import pytest


def chain(n: int) -> str:
    return "".join(f"var x{i}:[0,1]; " for i in range(n)) + "".join(f"x{i} <= x{i + 1}; " for i in range(n - 1))


def size_verdict(stcsp, text, prefix_k=2, **opts):
    """None when the engine takes the model's block (it may still find no device), else the refusal."""
    try:
        stcsp.Engine(stcsp.Model(text=text, prefix_k=prefix_k), **opts).close()
    except stcsp.StcspError as ex:
        return None if ex.code != -2 else ex
    return None


@pytest.mark.parametrize("n,k", [(129, 2), (256, 2), (512, 1), (170, 3)])
def test_blocks_up_to_512_words_are_not_refused(stcsp, n, k):
    assert size_verdict(stcsp, chain(n), prefix_k=k) is None


@pytest.mark.parametrize("n,k", [(257, 2), (513, 1), (171, 3)])
def test_blocks_over_512_words_are_refused(stcsp, n, k):
    ex = size_verdict(stcsp, chain(n), prefix_k=k)
    assert ex is not None and "512" in str(ex) and "register-resident block" in str(ex)


def test_wide_domains_count_in_the_block(stcsp):
    """W = 4 (65..128 values) for the whole block: 64 variables fit at K = 2, 65 do not."""
    wide = "var y:[0,99]; first y == 0; next y == (if (y lt 99) then (y + 1) else 0); "
    assert size_verdict(stcsp, wide + chain(62)) is None  # y, its `next` aux and 62 booleans: 64 * 2 * 4 = 512
    ex = size_verdict(stcsp, wide + chain(63))
    assert ex is not None and "512" in str(ex)


def test_interval_blocks_keep_their_256_word_limit(stcsp):
    ex = size_verdict(stcsp, chain(129), flags=stcsp.F_INTERVAL_DOMAINS)
    assert ex is not None and "block limit" in str(ex) and "256" in str(ex)
