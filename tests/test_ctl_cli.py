"""stcsp --ctl='FORMULA' (csrc/stcsp_main.cpp): argument and parse errors, which need no device, and on the GPU box the printed
verdict and witness on LADDER by the device road and by the host twin (--shards=2)."""
import re
import subprocess

import pytest

import ctl_ref as T
from test_components import LADDER


def exe_of(stcsp):
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    return exe


def run(stcsp, tmp_path, *opts):
    (tmp_path / "m.csp").write_text(LADDER)
    return subprocess.run([str(exe_of(stcsp)), *opts, str(tmp_path / "m.csp")], capture_output=True, text=True, timeout=600, cwd=tmp_path)


@pytest.mark.parametrize("formula, line", [
    ("AG EF", "--ctl: 5: the formula ends where an operand is expected"),
    ("z == 1", "--ctl: 0: unknown variable 'z'"),
    ("m == 1 )", "--ctl: 7: unexpected ')' after the formula"),
    ("E[m == 1 t == 0]", "--ctl: 9: expected U"),
    ("", "--ctl: 0: the formula ends where an operand is expected"),
    ("m == 99999999999", "--ctl: 5: the integer is outside int32"),
])
def test_a_formula_that_does_not_parse_ends_the_run(stcsp, tmp_path, formula, line):
    """Status 1 and `--ctl: <position>: <message>` before anything is solved: no device is needed, nothing is written."""
    p = run(stcsp, tmp_path, "-s", f"--ctl={formula}")
    assert p.returncode == 1 and p.stderr.splitlines() == [line] and p.stdout == ""
    assert not (tmp_path / "solutions.dot").exists()


def test_ctl_without_a_formula(stcsp, tmp_path):
    p = run(stcsp, tmp_path, "--ctl")
    assert p.returncode == 1 and p.stderr.startswith("--ctl takes a formula") and p.stdout == ""


@pytest.mark.gpu
def test_cli_verdict_and_witness(stcsp, tmp_path):
    """The device road and the twin road (--shards=2) print the same lines; they parse back to the twin's result; stdout and the
    written automaton are those of the run without the option."""
    m = stcsp.Model(text=LADDER)
    e = stcsp.Engine(m)
    r = e.solve()
    a = e.automaton(r).import_flags(e.postprocess())
    shown = [i for i, n in enumerate(m.var_names) if not n.startswith("_V")]
    plain = run(stcsp, tmp_path, "-s")
    assert plain.returncode == 0 and "ctl:" not in plain.stderr
    dot = (tmp_path / "solutions.dot").read_bytes()
    cases = [("AG EF m == 3", "yes", None), ("EF m == 3", "yes", "witness"), ("AG m < 3", "no", "counterexample")]
    for formula, verdict, kind in cases:
        twin = a.ctl(formula, witness=True)
        for opts in ((), ("--shards=2",)) if kind else ((),):
            p = run(stcsp, tmp_path, "-s", f"--ctl={formula}", *opts)
            assert p.returncode == 0, p.stderr
            assert (tmp_path / "solutions.dot").read_bytes() == dot and p.stdout.split()[:3] == plain.stdout.split()[:3]
            lines = [line for line in p.stderr.splitlines() if line.startswith("ctl: ")]
            head = re.fullmatch(r"ctl: (\d+) steps on infinite solutions, holds at (\d+) of (\d+) first steps: (yes|no|vacuous)", lines[0])
            assert head and [int(head.group(i)) for i in (1, 2, 3)] == [twin["n_worlds"], twin["n_initial_sat"], twin["n_initial"]]
            assert head.group(4) == verdict
            if kind is None:
                assert len(lines) == 1 and twin["witness"][0] == "none"
                continue
            assert twin["witness"][0] == kind and len(lines) == 3
            assert lines[1] == "ctl: # " + " ".join(m.var_names[i] for i in shown)
            assert lines[2].startswith(f"ctl: {kind}:")
            rows = [tuple(map(int, row.split())) for row in lines[2][len(f"ctl: {kind}:"):].split(";")]
            assert rows == [tuple(int(row[i]) for i in shown) for row in twin["witness"][1]]
    fuse = "var c:[0,3]; first c == 0; next c == c + 1;"
    (tmp_path / "f.csp").write_text(fuse)
    p = subprocess.run([str(exe_of(stcsp)), "--ctl=AG false", str(tmp_path / "f.csp")], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert p.returncode == 0 and "ctl: 0 steps on infinite solutions, holds at 0 of 0 first steps: vacuous" in p.stderr
    assert T.parse("AG false", ["c"]) == ("AG", ("false",))
