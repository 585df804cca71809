"""tools/gpu/bench_region_stats.py (over tools/gpu/optbench.py) replayed on the
CPU, as tests/test_option_bench.py replays its siblings: the driver runs with
subprocess.run replaced by a stub that hands the per-process results of
profiles/region_stats_bench.json back one by one, and the document it writes
has to be the committed one, byte for byte.  The sequence of worker starts --
arguments, time limit, SID_RS_FORM -- is pinned, and a failing worker ends the
script before another one starts."""
import json
import os
import subprocess
import sys

import pytest

from test_option_bench import CHECK, PARENT, ROOT, TOOLS, load

NAME = "bench_region_stats"
DOC = os.path.join(ROOT, "profiles", "region_stats_bench.json")
PROCS = [(PARENT, "--sels none", {}),
         (ROOT, "--sels none,reg_a,rs_a,reg_b,rs_b,dh " + CHECK, {"SID_RS_FORM": "0"}),
         (ROOT, "--sels none,reg_a,rs_a " + CHECK, {"SID_RS_FORM": "1"})]


class Stub:
    """subprocess.run for the driver: start k answers with outcomes[k] (a dict: the worker's tagged line; a
    (status, stdout) pair as it is)."""

    def __init__(self, outcomes):
        self.script, self.tag = os.path.join(TOOLS, NAME + ".py"), NAME.upper() + " "
        self.outcomes, self.starts = list(outcomes), []

    def __call__(self, cmd, **kw):
        assert cmd[0] == sys.executable and cmd[1] == self.script
        assert kw.pop("capture_output") is True and kw.pop("text") is True
        env = kw.pop("env")
        self.starts.append((cmd[2:], kw.pop("timeout"), {v: env[v] for v in ("SID_LIB_PATH", "SID_RS_FORM") if v in env}))
        assert not kw and "HSA_ENABLE_SDMA" in env
        o = self.outcomes[len(self.starts) - 1]
        status, out = o if isinstance(o, tuple) else (0, "a line before\n" + self.tag + json.dumps(o) + "\nand after\n")
        return subprocess.CompletedProcess(cmd, status, out, "stderr of the worker\n")


def case():
    with open(DOC) as f:
        doc = json.load(f)
    results = [{k: v for k, v in r.items() if k not in ("build", "round")} for r in doc["runs"]]
    argv = ["--parent", PARENT, "--sites", str(doc["sites"]), "--steps", str(doc["steps"]), "--warmup",
            str(doc["warmup"]), "--rounds", str(doc["rounds_asked"])]
    return doc, results, argv


def drive(outcomes, argv, out, monkeypatch):
    stub = Stub(outcomes)
    monkeypatch.setattr(subprocess, "run", stub)
    monkeypatch.setattr(sys, "argv", [stub.script] + argv + ["--out", str(out)])
    monkeypatch.setenv("SID_LIB_PATH", "/nonexistent/libsid.so")
    monkeypatch.setenv("SID_RS_FORM", "7")
    return stub, load(NAME).main


def expected_starts(doc, argv, n):
    a = dict(zip(argv[::2], argv[1::2]))
    common = ["--sites", a["--sites"], "--steps", a["--steps"], "--warmup", a["--warmup"]]
    return [(["--worker", tree, "--config", config] + common + [x for x in tail.split() if x != CHECK] +
             (["--check"] if CHECK in tail and rnd == 0 else []), 300, env)
            for rnd in range(doc["rounds"]) for config in ("C2", "C3") for tree, tail, env in PROCS][:n]


def test_replay_writes_the_committed_document(tmp_path, monkeypatch, capsys):
    doc, results, argv = case()
    argv[-1] = str(doc["rounds"])   # (the rounds that ran: a replay has no time budget to run out of)
    stub, main = drive(results, argv, tmp_path / "doc.json", monkeypatch)
    assert main() == 0
    got = json.loads((tmp_path / "doc.json").read_text())
    got["rounds_asked"] = doc["rounds_asked"]
    assert got == doc
    assert json.dumps(got, indent=1) + "\n" == open(DOC).read()   # key order, rounding and layout too
    assert len(stub.starts) == len(results) and stub.starts == expected_starts(doc, argv, len(results))
    lines = capsys.readouterr().out.splitlines()
    assert lines[-1] == f"wrote {tmp_path / 'doc.json'}"
    assert [ln.startswith("round ") for ln in lines].count(True) == len(results)   # a progress line a process


def test_the_document_states_what_the_design_rests_on():
    doc, results, argv = case()
    assert doc["tool"] == "tools/gpu/bench_region_stats.py" and doc["rounds"] >= 1
    for config in ("C2", "C3"):
        c = doc["summary"][config]
        assert c["rows_check"]["this_f0"]["equal"] is True and c["rows_check"]["this_f1"]["equal"] is True
        assert c["both_forms_give_the_same_rows"] is True
        assert c["this_f0_rs_a"]["rows"] == 1 and c["this_f0_rs_b"]["rows"] > 1000
        cost = doc["comparisons"][config]["stage_cost"]
        assert {"set_a", "set_b", "set_a_forms"} <= set(cost)


@pytest.mark.parametrize("how", ["exit", "no_line"])
def test_a_failing_worker_ends_the_script(how, tmp_path, monkeypatch, capsys):
    doc, results, argv = case()
    bad = {"exit": (134, NAME.upper() + " " + json.dumps(results[2]) + "\n"), "no_line": (0, "nothing tagged\n")}[how]
    stub, main = drive(results[:2] + [bad] + results[3:], argv, tmp_path / "doc.json", monkeypatch)
    with pytest.raises(SystemExit) as ei:
        main()
    assert NAME in str(ei.value.code) and f"(exit {bad[0]})" in str(ei.value.code)
    assert len(stub.starts) == 3 and stub.starts == expected_starts(doc, argv, 3)
    assert not (tmp_path / "doc.json").exists()


def test_imports_without_a_device_and_help(tmp_path):
    code = ("import importlib.util, sys; s = importlib.util.spec_from_file_location('m', sys.argv[1]); "
            "m = importlib.util.module_from_spec(s); s.loader.exec_module(m); "
            "assert 'torch' not in sys.modules and 'sid_amd' not in sys.modules")
    script = os.path.join(TOOLS, NAME + ".py")
    p = subprocess.run([sys.executable, "-c", code, script], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0 and "--parent" in p.stdout and "--budget-s" in p.stdout
