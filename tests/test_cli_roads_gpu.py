"""Every service of the `stcsp` command line on its two host roads. The adversarial variable `a` of OVER_CAP has 5000 values,
more than the device passes take, so `-a --intervals` sends an unsharded run down the fallback road (the host passes, then every
service by its host twin), the road no other service test reaches; `--shards=2` takes the sharded road (the same twins on the
merged automaton). Both roads must answer alike: the exit code, stdout, solutions.dot and the service's own stderr lines. The
statistics line carries times and is not compared.

OVER_CAP fixes `a` by `s`, so the adversary, who chooses `a`, leaves no live state ("adver1: 0"): there the services answer for
the empty language, and --sample fails alike on both roads (no prefix of that length). FREE is the same model with `a`
unconstrained; all its 3 states and 15000 edges survive -a, and there every service must also succeed and print answers."""
import re
import subprocess

import pytest

from test_interval_domains_gpu import OVER_CAP

pytestmark = pytest.mark.gpu

FREE = ("var d0:[0,0]; var d1:[0,0]; var d2:[0,0]; var d3:[0,0]; var s:[0,1]; var a:[0,4999]; var c:[0,1]; "
        "first s == 0; next s == 1 - s; c == s;")
MODELS = {"over_cap": OVER_CAP, "free": FREE}

# three streams of at most four steps over s a c, one with values that were not observed, an infeasible stream (s starts at 0) and
# an empty one; --check= does not read "?"
STREAMS = "# s a c\n0 3 0\n1 20 1\n0 3 0\n1 20 1\n\n0 ? 0\n1 20 ?\n\n0 3 0\n\n1 3 0\n0 3 0\n\n\n"
CHECKED = STREAMS.replace("?", "3", 1).replace("?", "1", 1)

CASES = {  # service -> (its arguments, the prefixes of its own stderr lines)
    "check": (["--check=../checked.txt"], ()),
    "count": (["--count=3"], ()),
    "sample": (["--sample=3:3:1"], ()),
    "repair": (["--repair=../streams.txt"], ()),
    "align": (["--align=../streams.txt", "--align-costs=2:3"], ()),
    "infer": (["--infer=../streams.txt", "--infer-draws=2:1"], ()),
    "posterior": (["--posterior=../streams.txt", "--posterior-weights=a=3:2,s=1:0"], ()),
    "components": (["--components=all"], ("components:",)),
    "optimise": (["--optimise=min:a=1:3:mean"], ("optimise:",)),
    "observer": (["--observer"], ("observer:",)),
    "compare": (["--observer", "--compare=../first.bin"], ("observer:", "compare:")),
    "quotient": (["--quotient"], ("quotient:",)),
}
STATISTICS = re.compile(r"\d+\.\d+\t\d+\t\d+\t\d+\t\d+\t\d+\t\d+\.\d+\t\d+\.\d+\n\Z")


@pytest.fixture(scope="module", params=list(MODELS))
def bench(request, stcsp, tmp_path_factory):
    """The CLI, the name of the model and the directory of the model, the streams and the binary automaton of a first run
    (--compare= reads it)."""
    exe = stcsp.CSRC / "stcsp"
    if not exe.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    d = tmp_path_factory.mktemp(request.param)
    (d / "m.csp").write_text(MODELS[request.param])
    (d / "streams.txt").write_text(STREAMS)
    (d / "checked.txt").write_text(CHECKED)
    r = subprocess.run([str(exe), "--intervals", "--binary=first.bin", "m.csp"], cwd=d, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and (d / "first.bin").exists(), r.stderr
    return exe, request.param, d


@pytest.mark.parametrize("service", list(CASES))
def test_fallback_and_sharded_roads_answer_alike(bench, service):
    exe, model, d = bench
    args, prefixes = CASES[service]
    seen = []
    for road, extra in (("fallback", []), ("sharded", ["--shards=2"])):
        cwd = d / f"{service}_{road}"
        cwd.mkdir()
        r = subprocess.run([str(exe), "-s", "-a", "--intervals", *extra, *args, "../m.csp"], cwd=cwd, capture_output=True, text=True, timeout=300)
        own = [line for line in r.stderr.splitlines() if line.startswith(prefixes)] if prefixes else []
        print(road, r.returncode, repr(r.stdout[:2000]), repr(r.stderr[:2000]))
        dot = cwd / "solutions.dot"
        seen.append((r.returncode, STATISTICS.sub("", r.stdout), dot.read_bytes() if dot.exists() else None, own))
    assert seen[0] == seen[1]
    if model == "free":
        rc, out, dot, own = seen[0]
        assert rc == 0 and dot
        if prefixes:
            assert own, "the service printed nothing of its own"
        else:
            assert out.count("\n") >= 4, "the service printed no answers"
