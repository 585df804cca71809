"""tools/gpu/strip_steps.py without a device: its bench.py processes replaced
by canned result lines.  The order of the starts (parent and this tree
alternating, then the other configs, the timed run, the --full run), the
document it writes, and that a failing process ends it before anything else
starts.  CPU only."""
import importlib.util
import json
import os
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def tool():
    spec = importlib.util.spec_from_file_location("strip_steps", os.path.join(ROOT, "tools", "gpu", "strip_steps.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def line(ms):
    return json.dumps({"ms_per_step": ms, "value": 5e10 / ms, "spot_check": {"ranks_equal": True},
                       "device_path": {"ms_per_step": 2.17, "stages_ms": {"parse": 1.27}, "more": 1},
                       "pcie": {"ingest_s": ms / 1e3, "h2d_s_last_step": ms / 1e3 - 5e-4, "h2d_GBps_last_step": 50.0,
                                "chunks": 34, "tile_overflows_last_step": 0, "text_bytes": 4_000_000_000,
                                "ceiling": {"frac": 72.4 / ms}}})


def timing(k):
    return json.dumps({"engine_phase": "ingest", "s": 0.05, "strip_threads": 14, "strip_busy_s": 0.6 + k / 100,
                       "strip_busy_min_s": 0.04, "strip_busy_max_s": 0.05 + k / 1000, "chunks_stripped": 33,
                       "strip_bytes": 1_400_000_000 + k, "h2d_bytes": 2_600_000_000 - k})


def drive(tool, monkeypatch, tmp_path, argv, fail_at=None):
    starts = []

    def run(cmd, cwd=None, env=None, timeout=None, **kw):
        starts.append((os.path.basename(cwd), cmd[4:], timeout, (env or {}).get("SID_ENGINE_TIMING")))
        if fail_at is not None and len(starts) == fail_at:
            return types.SimpleNamespace(returncode=134, stdout="", stderr="boom\n")
        ms = 73.0 + len(starts) if os.path.basename(cwd) == "parent" else 53.0 + len(starts)
        err = "".join('{"engine_phase": "emit"}\n' + timing(k) + "\n" for k in range(5))
        return types.SimpleNamespace(returncode=0, stdout="noise\n" + line(ms) + "\n", stderr=err)

    monkeypatch.setattr(tool.subprocess, "run", run)
    out = tmp_path / "doc.json"
    monkeypatch.setattr(tool.sys, "argv", ["strip_steps.py", "--parent", str(tmp_path / "parent"), "--out", str(out)] + argv)
    return starts, out


def test_starts_and_document(tool, monkeypatch, tmp_path):
    starts, out = drive(tool, monkeypatch, tmp_path, ["--rounds", "2", "--steps", "3", "--warmup", "1", "--full"])
    tool.main()
    base = ["--steps", "3", "--warmup", "1"]
    this = os.path.basename(ROOT)
    assert starts == [("parent", base, 240, None), (this, base, 240, None)] * 2 + \
        [(t, base + ["--config", c], 240, None) for c in ("C3", "C5") for t in ("parent", this)] + \
        [(this, base, 240, "1"), (this, base + ["--full", "--no-cpu"], 720, None)]
    doc = json.loads(out.read_text())
    assert [r["ms_per_step"] for r in doc["C2"]["parent"]] == [74.0, 76.0]
    assert doc["C2"]["ms_per_step"]["this"] == {"min": 55.0, "max": 57.0, "runs": [55.0, 57.0]}
    assert doc["C2"]["parent"][0]["pcie_ceiling_frac"] == 72.4 / 74.0 and "h2d_bytes_last_step" not in doc["C2"]["this"][0]
    assert doc["C3"]["this"]["ms_per_step"] == 59.0 and doc["C5"]["parent"]["ms_per_step"] == 80.0
    timed = doc["C2"]["this_timed"]   # (the last `steps` ingest lines of the five)
    assert timed["strip_threads"] == 14 and timed["strip_bytes"] == {"min": 1_400_000_002, "max": 1_400_000_004}
    assert timed["h2d_bytes"] == {"min": 2_599_999_996, "max": 2_599_999_998}
    assert timed["strip_busy_max_s"] == {"min": 0.05 + 2 / 1000, "max": 0.05 + 4 / 1000}
    assert doc["full"]["spot_check"] == {"ranks_equal": True}
    assert doc["full"]["device_path"] == {"ms_per_step": 2.17, "stages_ms": {"parse": 1.27}}


def test_a_failing_process_ends_the_script(tool, monkeypatch, tmp_path):
    starts, out = drive(tool, monkeypatch, tmp_path, ["--rounds", "2"], fail_at=3)
    with pytest.raises(SystemExit) as ei:
        tool.main()
    assert "exit status 134" in str(ei.value.code) and len(starts) == 3
    assert len(json.loads(out.read_text())["C2"]["parent"]) == 1   # (what was measured so far is kept)


def test_help_needs_no_device(tmp_path):
    p = subprocess.run([os.sys.executable, os.path.join(ROOT, "tools", "gpu", "strip_steps.py"), "--help"],
                       capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0 and "--parent" in p.stdout
