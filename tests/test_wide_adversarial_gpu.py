"""adversarialTraverse / adversarialTraverse2 on the device (dev_postproc.hpp) for variables of 33..128 values: the cover
sets are CW = ceil(width / 32) words per state (per state and `ava` value), the last one compared with the partial full
mask. Against the host twins (postproc.cpp), like tests/test_postproc_gpu.py, and on the command line against --shards=2,
which runs the host passes."""
import re
import subprocess

import pytest

from test_postproc_gpu import host_and_device
from test_wide_gpu import WIDE

pytestmark = pytest.mark.gpu


def game(w: int) -> str:
    """Variables 5 and 6 (the CLI's -a / -z indices) take w values: a misses its lowest value and c its highest (the top bit of
    the last, partial cover word) in state s = 1, so whether a state keeps every value decides the passes."""
    return ("var d0:[0,0]; var d1:[0,0]; var d2:[0,0]; var d3:[0,0]; var s:[0,1]; "
            f"var a:[0,{w - 1}]; var c:[0,{w - 1}]; var e:[0,1]; "
            f"first s == 0; next s == (if (e eq 1) then (a ge {w // 2}) else s); a >= s; c + s <= {w - 1};")


def widths(m):
    return [k for k, (lo, hi) in enumerate(m.var_bounds()) if hi - lo + 1 > 32]


@pytest.mark.parametrize("name", sorted(WIDE))
def test_wide_device_adversarial_passes_match_host(stcsp, name):
    m = stcsp.Model(text=WIDE[name])
    e = stcsp.Engine(m)
    r = e.solve()
    wide = widths(m)
    assert wide
    for v in wide:
        other = 0 if v != 0 else m.n_vars - 1
        host_and_device(stcsp, e, r, adv=v)
        host_and_device(stcsp, e, r, adv2=(v, other))
        host_and_device(stcsp, e, r, adv2=(other, v))
        host_and_device(stcsp, e, r, adv2=(v, v))
    host_and_device(stcsp, e, r, adv=wide[0], adv2=(wide[-1], wide[0]))


@pytest.mark.parametrize("w", [32, 33, 64, 65, 96, 128])
def test_wide_device_adversarial_word_boundaries(stcsp, w):
    m = stcsp.Model(text=game(w))
    e = stcsp.Engine(m)
    r = e.solve()
    assert r.n_states >= 2
    results = set()
    for v in (5, 6, 4, 7):
        _, _, post = host_and_device(stcsp, e, r, adv=v)
        results.add(post.adver1)
    for op, ava in [(5, 6), (6, 5), (5, 7), (7, 5), (6, 6), (4, 6)]:
        _, _, post = host_and_device(stcsp, e, r, adv2=(op, ava))
        results.add(post.adver2)
    host_and_device(stcsp, e, r, adv=5, adv2=(5, 6))
    assert results == {0, 1}  # (the passes keep some roots and lose others: the masks are looked at)


@pytest.mark.parametrize("w,flags", [(65, ["-s", "-a"]), (128, ["-s", "-z"]), (33, ["-s", "-a", "-z"])])
def test_cli_wide_adversarial_matches_sharded_host_passes(stcsp, tmp_path, w, flags):
    exe = stcsp.CSRC / "stcsp"
    src = tmp_path / "game.csp"
    src.write_text(game(w))
    outs = []
    for extra in ([], ["--shards=2"]):
        d = tmp_path / ("one" if not extra else "two")
        d.mkdir()
        r = subprocess.run([str(exe), *flags, *extra, str(src)], cwd=d, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        line = r.stdout.strip().split("\n")[-1]
        outs.append((re.findall(r"adver\d: -?\d+", r.stdout), line.split("\t")[1:4], (d / "solutions.dot").read_bytes()))
    assert len(outs[0][0]) == ("-a" in flags) + ("-z" in flags)
    assert outs[0] == outs[1]
