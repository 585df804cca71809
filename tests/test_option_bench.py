"""The per-option benchmark scripts under tools/gpu/ (X_bench.py, over
tools/gpu/optbench.py), replayed on the CPU.

Each committed profiles/X_bench.json keeps the per-process results (`runs`)
beside the `summary` and `comparisons` computed from them.  Here every script's
driver runs with subprocess.run replaced by a stub that hands those results
back one by one as tagged lines, and the document it writes has to be the
committed one, byte for byte: same keys in the same order, same rounding, same
note.  (profiles/depth_bench.json was merged by hand from two sessions; its
script replays tests/golden/depth_bench_runs.json, a round of that file's
processes with the split process's `none` set given back, into
tests/golden/depth_bench_doc.json.)

The stub also records what the driver asks of every worker -- the arguments,
the time limit, the SID_* variables -- and the sequence is pinned here; a
worker that fails, prints no tagged line or runs past its time limit has to end
the script before another one starts."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools", "gpu")
GOLDEN = os.path.join(ROOT, "tests", "golden")
PARENT = "/nonexistent/parent"
VARS = ("SID_LIB_PATH", "SID_DH_FORM", "SID_DEPTH_SPLIT")
CHECK = "+check"   # "--check" in the first round

# per tool: the default --step-timeout, the configs, and a round's processes for one config in order:
# (tree, the arguments after --warmup W, the SID_* variables the process sees)
STARTS = {
    "select_bench": (600, "C2,C3", [(PARENT, "--selects all", {}),
                                    (ROOT, "--selects all,het,hom " + CHECK, {})]),
    "regions_bench": (600, "C2,C3", [(PARENT, "--sets none", {}),
                                     (ROOT, "--sets none,sparse,whole " + CHECK, {})]),
    "context_bench": (600, "C2,C3", [(PARENT, "--sels none,het", {}),
                                     (ROOT, "--sels none,het,hetctx " + CHECK, {})]),
    "windows_bench": (400, "C2,C3", [(PARENT, "--sels none", {}),
                                     (ROOT, "--sels none,win,hetwin " + CHECK, {})]),
    "variants_bench": (600, "C2,C3", [(PARENT, "--sets none,het", {}),
                                      (ROOT, "--sets none,variants,het " + CHECK, {})]),
    "depth_bench": (600, "C2,C3", [(PARENT, "--sets none", {}),
                                   (ROOT, "--sets none,half,tight,variants,both", {}),
                                   (ROOT, "--sets none,both_split --split", {})]),
    "vcf_bench": (300, "C2,C3", [(PARENT, "--sets csv", {}),
                                 (ROOT, "--sets csv,vcf", {})]),
    "depth_hist_bench": (300, "C2,C3,D200", [(PARENT, "--sels none", {}),
                                             (ROOT, "--sels none,win,dh " + CHECK, {"SID_DH_FORM": "0"}),
                                             (ROOT, "--sels none,dh " + CHECK, {"SID_DH_FORM": "1"})]),
}
TOOLS_ALL = tuple(STARTS) + ("bgzf_bench",)


def load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case(name):
    """(the expected document's path, the worker results to hand back, the driver's arguments)."""
    if name == "depth_bench":
        path = os.path.join(GOLDEN, "depth_bench_doc.json")
        with open(os.path.join(GOLDEN, "depth_bench_runs.json")) as f:
            results = json.load(f)
    else:
        path = os.path.join(ROOT, "profiles", name + ".json")
        with open(path) as f:
            results = [{k: v for k, v in r.items() if k not in ("build", "round")} for r in json.load(f)["runs"]]
    with open(path) as f:
        doc = json.load(f)
    argv = ["--parent", PARENT, "--sites", str(doc["sites"]), "--steps", str(doc["steps"]), "--warmup",
            str(doc["warmup"]), "--rounds", str(doc.get("rounds_asked", doc["rounds"]))]
    if name == "bgzf_bench":
        argv += ["--level", str(doc["summary"]["level"]), "--chunk-bytes", str(doc["chunk_bytes"])]
    return path, results, argv


class Stub:
    """subprocess.run for the drivers: start k answers with outcomes[k] -- a dict is a worker's result, printed as
    the tool's tagged line; a (status, stdout) pair is returned as it is; an exception is raised."""

    def __init__(self, name, outcomes):
        self.script, self.tag = os.path.join(TOOLS, name + ".py"), name.upper() + " "
        self.outcomes, self.starts = list(outcomes), []

    def __call__(self, cmd, **kw):
        assert cmd[0] == sys.executable and cmd[1] == self.script
        assert kw.pop("capture_output") is True and kw.pop("text") is True
        env = kw.pop("env")
        self.starts.append((cmd[2:], kw.pop("timeout"), {v: env[v] for v in VARS if v in env}))
        assert not kw and "HSA_ENABLE_SDMA" in env
        o = self.outcomes[len(self.starts) - 1]
        if isinstance(o, BaseException):
            raise o
        status, out = o if isinstance(o, tuple) else (0, "a line before\n" + self.tag + json.dumps(o) + "\nand after\n")
        return subprocess.CompletedProcess(cmd, status, out, "stderr of the worker\n")


def drive(name, outcomes, argv, out, monkeypatch):
    """The script's main() over the stub, with the variables a caller might have set."""
    stub = Stub(name, outcomes)
    monkeypatch.setattr(subprocess, "run", stub)
    monkeypatch.setattr(sys, "argv", [stub.script] + argv + ["--out", str(out)])
    monkeypatch.setenv("SID_LIB_PATH", "/nonexistent/libsid.so")
    monkeypatch.setenv("SID_DH_FORM", "7")
    monkeypatch.delenv("SID_DEPTH_SPLIT", raising=False)
    return stub, load(name).main


def expected_starts(name, argv):
    a = dict(zip(argv[::2], argv[1::2]))
    common = ["--sites", a["--sites"], "--steps", a["--steps"], "--warmup", a["--warmup"]]
    if name == "bgzf_bench":
        args = ["--sites", a["--sites"], "--level", a["--level"], "--steps", a["--steps"], "--warmup", a["--warmup"],
                "--chunk-bytes", a["--chunk-bytes"]]
        return [(["--worker", tree] + args + more, 300, {"SID_DH_FORM": "7"})
                for _ in range(int(a["--rounds"])) for tree, more in ((PARENT, ["--plain-only"]), (ROOT, []))]
    timeout, configs, procs = STARTS[name]
    keep = {} if name == "depth_hist_bench" else {"SID_DH_FORM": "7"}   # (its driver sets or clears the form)
    return [(["--worker", tree, "--config", config] + common +
             [x for x in tail.split() if x != CHECK] + (["--check"] if CHECK in tail and rnd == 0 else []),
             timeout, {**keep, **env})
            for rnd in range(int(a["--rounds"])) for config in configs.split(",") for tree, tail, env in procs]


@pytest.mark.parametrize("name", TOOLS_ALL)
def test_replay_writes_the_committed_document(name, tmp_path, monkeypatch, capsys):
    path, results, argv = case(name)
    stub, main = drive(name, results, argv, tmp_path / "doc.json", monkeypatch)
    assert main() == 0
    with open(path) as f:
        want = f.read()
    got = (tmp_path / "doc.json").read_text()
    assert json.loads(got) == json.loads(want)
    assert got == want   # key order, rounding and layout too
    assert len(stub.starts) == len(results)
    assert stub.starts == expected_starts(name, argv)
    lines = capsys.readouterr().out.splitlines()
    assert lines[-1] == f"wrote {tmp_path / 'doc.json'}"
    assert [ln.startswith("round ") for ln in lines].count(True) == len(results)   # a progress line a process


def test_every_tool_is_replayed():
    have = sorted(f[:-3] for f in os.listdir(TOOLS) if f.endswith("_bench.py"))
    assert have == sorted(TOOLS_ALL)


@pytest.mark.parametrize("name", ["select_bench", "bgzf_bench"])
@pytest.mark.parametrize("how", ["exit", "no_line", "timeout"])
def test_a_failing_worker_ends_the_script(name, how, tmp_path, monkeypatch, capsys):
    """The third start fails: nothing is started after it and no document is written."""
    path, results, argv = case(name)
    bad = {"exit": (134, Stub(name, []).tag + json.dumps(results[2]) + "\n"), "no_line": (0, "nothing tagged\n"),
           "timeout": subprocess.TimeoutExpired(["worker"], 300)}[how]
    stub, main = drive(name, results[:2] + [bad] + results[3:], argv, tmp_path / "doc.json", monkeypatch)
    if how == "timeout":
        with pytest.raises(subprocess.TimeoutExpired):
            main()
    else:
        with pytest.raises(SystemExit) as ei:
            main()
        assert name in str(ei.value.code) and f"(exit {bad[0]})" in str(ei.value.code)
        assert "stderr of the worker" in capsys.readouterr().err
    assert len(stub.starts) == 3 and stub.starts == expected_starts(name, argv)[:3]
    assert not (tmp_path / "doc.json").exists()


@pytest.mark.parametrize("name", TOOLS_ALL + ("optbench",))
def test_imports_without_a_device(name):
    """Loading a script or the shared module imports neither torch nor sid_amd."""
    code = ("import importlib.util, sys; s = importlib.util.spec_from_file_location('m', sys.argv[1]); "
            "m = importlib.util.module_from_spec(s); s.loader.exec_module(m); "
            "assert 'torch' not in sys.modules and 'sid_amd' not in sys.modules")
    p = subprocess.run([sys.executable, "-c", code, os.path.join(TOOLS, name + ".py")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


@pytest.mark.parametrize("name", TOOLS_ALL)
def test_help(name, tmp_path):
    p = subprocess.run([sys.executable, os.path.join(TOOLS, name + ".py"), "--help"], capture_output=True, text=True,
                       cwd=tmp_path)
    assert p.returncode == 0 and "--parent" in p.stdout and "--step-timeout" in p.stdout
