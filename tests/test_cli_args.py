"""The `stcsp` command line before it needs a device: exit code, stdout and stderr of the argument errors, of a model that
cannot be loaded and of a streams file that cannot be read, on the unsharded road and on --shards=2. The texts are the ones the
command line printed before its services were brought onto one road; they are pinned so that no road loses or rewords one."""
import subprocess
import sys

import pytest

MODEL = "var s:[0,1]; var a:[0,4]; var c:[0,1];\nfirst s == 0; next s == 1 - s; a == 2 * s + 1; c == s;\n"
EXCLUDE = "--check, --repair, --align, --infer, --posterior, --sample and --count exclude each other\n"
HEADER = 'the first line must be "# name name ..."\n'
STREAM_OPTIONS = ("check", "repair", "align", "infer", "posterior")


@pytest.fixture(scope="module")
def exe(stcsp):
    path = stcsp.CSRC / "stcsp"
    if not path.exists():
        subprocess.run(["make", "-C", str(stcsp.CSRC), "stcsp"], check=True, capture_output=True)
    return path


@pytest.fixture()
def cli(exe, tmp_path):
    (tmp_path / "c.csp").write_text(MODEL)
    (tmp_path / "s.txt").write_text("# s a\n0 1\n1 3\n")

    def run(*args):
        r = subprocess.run([str(exe), *args], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout, r.stderr

    run.dir = tmp_path
    return run


@pytest.mark.parametrize("args, rc, out, err", [
    ((), 0, "No constraints!\n", ""),
    (("--repair=s.txt", "--check=s.txt", "c.csp"), 1, "", EXCLUDE),
    (("--compare=f.bin", "c.csp"), 1, "", "--compare needs --observer: the observers of the two models are compared\n"),
    (("--components=0", "c.csp"), 1, "", "--components takes nothing, bottom, all or a positive count\n"),
    (("--align-costs=0:1", "c.csp"), 1, "", "--align-costs=SKIP:GAP takes two integers of at least 1\n"),
    (("--infer-draws=x",), 1, "", "Invalid argument: --infer-draws=x\n"),
    (("--sample=1",), 1, "", "Invalid argument: --sample=1\n"),
    (("--count=-1",), 1, "", "Invalid argument: --count=-1\n"),
    (("--shards=65",), 1, "", "Invalid argument: --shards=65\n"),
    (("-k",), 1, "", "Option -k needs a value\n"),
    (("-k0", "c.csp"), 1, "", "Invalid argument: -k 0\n"),
    (("-q", "c.csp"), 1, "", "Unknown argument: q\n"),
])
def test_argument_errors(cli, args, rc, out, err):
    assert cli(*args) == (rc, out, err)


@pytest.mark.parametrize("shards", [(), ("--shards=2",)])
def test_model_that_cannot_be_loaded(cli, shards):
    """A file that is not there is reported on stderr, a syntax error on stdout (as the reference's yyerror does)."""
    assert cli(*shards, "nofile.csp") == (1, "", "cannot open nofile.csp\n")
    (cli.dir / "bad.csp").write_text("var s:[0,1];\nfirst s == ;\n")
    assert cli(*shards, "bad.csp") == (1, "Line 2: syntax error\n", "")


@pytest.mark.parametrize("shards", [(), ("--shards=2",)])
@pytest.mark.parametrize("option", STREAM_OPTIONS)
@pytest.mark.parametrize("text, err", [
    (None, "cannot read f.txt\n"),
    ("0 1\n", "f.txt: " + HEADER),
    ("", "f.txt: " + HEADER),
    ("# s zz\n0 1\n", "f.txt: unknown variable zz\n"),
    ("# s s\n0 1\n", "f.txt: repeated variable s\n"),
    ("# s a\n0 1\n\n0\n", "f.txt:4: expected 2 values\n"),
    ("# s a\n0 x1\n", "f.txt:2: not an int32: x1\n"),
    ("# s a\n0 99999999999\n", "f.txt:2: not an int32: 99999999999\n"),
])
def test_streams_file_that_cannot_be_read(cli, option, shards, text, err):
    if text is not None:
        (cli.dir / "f.txt").write_text(text)
    assert cli(*shards, f"--{option}=f.txt", "c.csp") == (1, "", err)


def device_available():
    """torch.cuda.is_available(), asked in a child process: torch ships its own HIP runtime, which must not start in the
    test process (tests/conftest.py, visible_gpus)."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True, text=True, check=True,
                       timeout=300)
    return r.stdout.split()[-1] == "True"


@pytest.fixture(scope="module")
def no_device():
    return not device_available()


@pytest.mark.parametrize("shards", [(), ("--shards=2",)])
@pytest.mark.parametrize("option", STREAM_OPTIONS)
def test_question_mark_is_a_value_for_all_but_check(cli, no_device, option, shards):
    """--check refuses "?" while it reads the file; the other four take it as "not observed" and go on to the solve, which ends
    at the missing device on a machine without one."""
    (cli.dir / "f.txt").write_text("# s a\n0 ?\n")
    rc, out, err = cli(*shards, f"--{option}=f.txt", "c.csp")
    if option == "check":
        assert (rc, out, err) == (1, "", "f.txt:2: not an int32: ?\n")
    elif no_device:
        assert (rc, out, err) == (1, "", "no HIP device available\n")
    else:
        assert rc == 0 and "not an int32" not in err, err


@pytest.mark.parametrize("shards", [(), ("--shards=2",)])
def test_valid_run_without_a_device(cli, no_device, shards):
    if not no_device:
        pytest.skip("there is a device: the run would succeed")
    assert cli(*shards, "--repair=s.txt", "c.csp") == (1, "", "no HIP device available\n")
