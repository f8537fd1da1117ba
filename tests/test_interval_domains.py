"""Interval domains without a GPU: the option flag is the same number in the C header and in Python, the command line knows
--intervals, and the front end gives the aux variables of `/` and `%` under next the whole int range (the models the flag is for)."""
import re
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]


def test_flag_matches_the_header(stcsp):
    text = (REPO / "include" / "stcsp_engine.h").read_text()
    value = int(re.search(r"#define STCSP_F_INTERVAL_DOMAINS (\d+)", text).group(1))
    assert value == stcsp.F_INTERVAL_DOMAINS == 16
    others = [int(v) for v in re.findall(r"#define STCSP_F_\w+ (\d+)", text)]
    assert others.count(value) == 1  # a bit of its own


def test_cli_documents_intervals():
    src = (REPO / "stcsp-solver_amd" / "csrc" / "stcsp_main.cpp").read_text()
    assert "--intervals" in src.split("#include")[0]  # the usage comment
    assert '"--intervals"' in src
    assert "--intervals" in (REPO / "README.md").read_text()


def test_div_under_next_gives_int_range_aux(stcsp):
    m = stcsp.Model(text="var x:[-3,3]; var y:[-2,2]; var z:[-9,9]; z == next (x / y) + next (x % y);")
    wide = [b for b in m.var_bounds() if b == (-(2 ** 31), 2 ** 31 - 1)]
    assert len(wide) >= 2
