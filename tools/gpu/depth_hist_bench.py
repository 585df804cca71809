#!/usr/bin/env python3
"""depth_hist_bench.py -- what --depth-hist (sid_engine_set_depth_hist) costs,
against another build of the project (its parent commit), and which of the
stage's two aggregation forms is faster.

Inputs: the C2 text (seed 2, -m local) and the C3 text (seed 3, -R -m
likelihood_ratio), --sites synthetic 30x sites each, and D200, a 200x text
(seed 5, -m local) of the same number of read bases (--sites * 30 / 200 sites).
The engine runs

  none     no option
  dh       the depth histogram                 (this tree only)
  win      --windows 100000, the peer summary  (this tree only)

  device   text and records in HBM (device_sink 1): the stage times of
           sid_engine_profile_read (HIP event pairs around every stage), per step
  pcie     pinned host text in, records into the pinned host arena
           (device_sink 2 + host_hold_bytes): the step's wall time

The histogram's stage runs inside a stage the engine already brackets -- the
tile parse's (`parse`) for -m local, the length stage (`fmt_len`) for the Lynch
pass 2 and for a chunk on the two-pass path -- so its time is parse + fmt_len
with the option minus the same sum of the plain run, same build, same process
(stage_ms; the window stage's likewise, for the peer).  The aggregation form
(SID_DH_FORM: 0 an LDS atomic a lane, 1 a wave's distinct depths one by one) is
read once per process, so each form has processes of its own: this_f0, this_f1.

Every (tree, form, config) is a process of its own (a fresh HIP runtime, the
tree's own sid_amd and libsid.so) under its own time limit.  The processes
alternate parent / this tree for --rounds rounds in one session; the spread of
a figure is its min .. max over the rounds.  A process that fails or runs past
--step-timeout ends the whole script; a round that would start past --budget-s
is not started and the file says how many rounds ran.

Once per configuration and form (this tree, first round) the rows are checked:
their sites add up to the run's, their records to the plain run's record count
(its newlines), the records with the option equal the records without, the
device-sink and PCIe runs give the same rows, the four column sums equal the
window rows', and (in the driver) both forms give the same rows.

    python tools/gpu/depth_hist_bench.py --parent DIR [--out profiles/depth_hist_bench.json]

DIR is a checkout of the parent commit built with `make` (build/libsid.so).
Needs an MI355X; there is no CPU fallback."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HSA_ENABLE_SDMA", "1")   # as bench.py: the copy engines for host<->device copies

CONFIGS = {"C2": dict(method="local", R=False, seed=2, depth=30.0),
           "C3": dict(method="likelihood_ratio", R=True, seed=3, depth=30.0),
           "D200": dict(method="local", R=False, seed=5, depth=200.0)}
W = 100_000
SELS = {"none": {}, "dh": {"depth_hist": True}, "win": {"window": W}}
STAGES = ("index", "parse", "call", "hist", "fmt_len", "fmt_write")
TAG = "DEPTH_HIST_BENCH "


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--parent", default=None, help="a built checkout of the parent commit (none: this tree only)")
    p.add_argument("--sites", type=int, default=50_000_000)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--configs", default="C2,C3,D200")
    p.add_argument("--no-check", action="store_true", help="skip the check of the rows")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_hist_bench.json"))
    p.add_argument("--step-timeout", type=int, default=300, help="seconds a (tree, form, config) process may take")
    p.add_argument("--budget-s", type=int, default=0, help="start no round past this many seconds (0: no limit)")
    # one (tree, form, config) process
    p.add_argument("--worker", default=None, metavar="TREE")
    p.add_argument("--config", default="C2")
    p.add_argument("--sels", default="none")
    p.add_argument("--check", action="store_true")
    return p.parse_args(argv)


def config_sites(config, sites):
    return int(sites * 30.0 / CONFIGS[config]["depth"])


# ------------------------------------------------------------------ worker --
def worker(a):
    sys.path.insert(0, a.worker)
    import ctypes as C
    import numpy as np
    import torch
    import sid_amd
    assert os.path.dirname(os.path.abspath(sid_amd.__file__)).startswith(os.path.abspath(a.worker))
    cfg = CONFIGS[a.config]
    n = config_sites(a.config, a.sites)
    dev = torch.device("cuda", 0)
    cap = int(n * (2.72 * cfg["depth"] + 2) * 1.03) + (64 << 20)
    text = torch.empty(cap, dtype=torch.uint8, device=dev)
    ctx = sid_amd.Context(0)
    ln = ctx.synth_text_device(cfg["seed"], cfg["depth"], 0, n, text.data_ptr(), cap - 512)
    text[ln:ln + 512].zero_()
    torch.cuda.synchronize(dev)
    ctx.close()
    host = text[:ln].cpu().pin_memory()
    out = {"config": a.config, "sites": n, "text_bytes": ln, "steps": a.steps, "warmup": a.warmup,
           "form": os.environ.get("SID_DH_FORM", "default"), "version": sid_amd.lib().sid_version().decode(), "sels": {}}

    def step(eng):
        st = eng.ingest()
        eng.estimate()
        _, st2 = eng.emit()
        return st, st2

    def timed(eng, steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            st, st2 = step(eng)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / steps * 1e3, st, st2

    rows, drows, wrows, digest, newlines = None, None, None, {}, None
    for name in a.sels.split(","):
        kw = SELS[name]
        r = {}
        eng = sid_amd.Engine(method=cfg["method"], estimate_prior=cfg["R"], devices=1, device_sink=1, **kw)
        eng.source_device_text(text.data_ptr(), ln, keep=text)
        eng.profile(False)
        for _ in range(a.warmup):
            step(eng)
        r["device_ms_per_step"], st, st2 = timed(eng, a.steps)
        eng.profile(True)
        step(eng)
        eng.profile_read()
        for _ in range(a.steps):
            step(eng)
        prof = eng.profile_read()
        eng.profile(False)
        if name == "dh":
            drows = eng.depth_hist()
        eng.close()
        r["device_stages_ms"] = {k[:-3]: v / a.steps for k, v in prof.items() if k.endswith("_ms")}
        r["device_bytes_out"] = st2.bytes_out
        r["chunks_tiled"] = st.chunks_tiled
        r["tile_overflows"] = st.tile_overflows
        eng = sid_amd.Engine(method=cfg["method"], estimate_prior=cfg["R"], devices=1, device_sink=2,
                             host_hold_bytes=int(n * 48) + (64 << 20), **kw)
        eng.source_host_ptr(host.data_ptr(), ln, keep=host)
        for _ in range(a.warmup):
            step(eng)
        r["pcie_ms_per_step"], st, st2 = timed(eng, a.steps)
        r["pcie_bytes_out"] = st2.bytes_out
        r["pcie_chunks"] = st.chunks
        if name == "dh":
            rows = eng.depth_hist()
            r["rows"] = len(rows)
            r["rows_csv_bytes"] = len(sid_amd.depth_hist_format(rows))
            r["rows_digest"] = hashlib.blake2b(repr(rows).encode()).hexdigest()
            r["modal_depth"] = max(rows, key=lambda x: x[1])[0] if rows else None
        if name == "win":
            wrows = eng.windows()
        if a.check and name in ("none", "dh"):
            h, nl = hashlib.blake2b(), 0
            for j in range(st.chunks):
                p, m = eng.records(j)
                raw = C.string_at(p, m) if m else b""
                h.update(raw)
                nl += int(np.count_nonzero(np.frombuffer(raw, np.uint8) == 10))
            digest[name] = h.hexdigest()
            if name == "none":
                newlines = nl
        eng.close()
        out["sels"][name] = r
    if a.check and rows is not None:
        sums = tuple(sum(x[k] for x in rows) for k in (1, 2, 3, 4))
        wsums = tuple(sum(x[k] for x in wrows) for k in (3, 4, 5, 6)) if wrows is not None else None
        ordered = all(x[0] < y[0] for x, y in zip(rows, rows[1:])) and all(x[2] == x[3] + x[4] for x in rows)
        chk = {"rows": len(rows), "sites_sum": sums[0], "sites": n, "records_sum": sums[1],
               "records_of_the_plain_run": newlines, "rows_in_order": ordered,
               "device_sink_rows_equal_pcie_rows": drows == rows,
               "records_equal_with_and_without": digest.get("dh") == digest.get("none"),
               "column_sums_equal_the_window_rows": None if wsums is None else sums == wsums}
        chk["equal"] = bool(sums[0] == n and sums[1] == newlines and ordered and drows == rows and
                            digest.get("dh") == digest.get("none") and wsums in (None, sums))
        out["rows_check"] = chk
    print(TAG + json.dumps(out), flush=True)
    return 0


# ------------------------------------------------------------------ driver --
def spread(xs):
    xs = list(xs)
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def rng(e, k):
    return [round(e[k]["min"], 3), round(e[k]["max"], 3)]


def comparisons(summary, sites):
    out = {}
    keys = ["device_ms_per_step", "pcie_ms_per_step"] + [s + "_ms" for s in STAGES]
    for config, c in summary.items():
        o = {}
        if "parent_none" in c:
            p = c["parent_none"]
            for b in ("this_f0", "this_f1"):
                if b + "_none" in c:
                    t = c[b + "_none"]
                    o[b + "_unchanged_without_the_option"] = {
                        "met": all(rng(t, k)[0] <= rng(p, k)[1] and rng(p, k)[0] <= rng(t, k)[1] for k in keys),
                        "this": {k: rng(t, k) for k in keys}, "parent": {k: rng(p, k) for k in keys}}
        scale = 50_000_000 / config_sites(config, sites)
        cost = {}
        for b, form in (("this_f0", "lds_atomic_per_lane"), ("this_f1", "wave_ballot_per_distinct_depth")):
            if b + "_dh" in c:
                e = c[b + "_dh"]
                cost[form] = {"stage_ms_per_step": rng(e, "stage_ms"),
                              "stage_ms_per_50M_sites": [round(x * scale, 3) for x in rng(e, "stage_ms")],
                              "pcie_ms_per_step": rng(e, "pcie_ms_per_step"),
                              "pcie_ms_per_step_without": rng(c[b + "_none"], "pcie_ms_per_step"),
                              "pcie_change_ms_median": round(e["pcie_ms_per_step"]["median"] -
                                                             c[b + "_none"]["pcie_ms_per_step"]["median"], 3)}
        if "this_f0_win" in c:
            cost["window_stage_peer"] = {"stage_ms_per_step": rng(c["this_f0_win"], "stage_ms"),
                                         "pcie_ms_per_step": rng(c["this_f0_win"], "pcie_ms_per_step")}
        o["stage_cost"] = cost
        out[config] = o
    return out


def main():
    a = parse_args()
    if a.worker:
        return worker(a)
    t_start = time.time()
    runs = []
    # (tree name, tree, SID_DH_FORM, selections)
    procs = ([("parent", os.path.abspath(a.parent), None, "none")] if a.parent else []) + \
            [("this_f0", ROOT, "0", "none,win,dh"), ("this_f1", ROOT, "1", "none,dh")]
    rounds_run, round_s = 0, 0.0
    for rnd in range(a.rounds):
        if a.budget_s and rnd and time.time() - t_start + round_s > a.budget_s:
            print(f"round {rnd} not started: past the budget of {a.budget_s} s", flush=True)
            break
        t_round = time.time()
        for config in a.configs.split(","):
            for name, tree, form, sels in procs:
                check = name != "parent" and rnd == 0 and not a.no_check
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", tree, "--config", config, "--sites",
                       str(a.sites), "--steps", str(a.steps), "--warmup", str(a.warmup), "--sels", sels] + \
                      (["--check"] if check else [])
                env = dict(os.environ)
                env.pop("SID_LIB_PATH", None)   # each tree loads its own build/libsid.so
                env.pop("SID_DH_FORM", None)
                if form is not None:
                    env["SID_DH_FORM"] = form
                # (a process of its own under its own time limit; a failure or a timeout ends the script)
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, env=env)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith(TAG)]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit(f"depth_hist_bench: {name} {config} failed (exit {p.returncode})")
                r = json.loads(line[0][len(TAG):])
                r["build"], r["round"] = name, rnd
                base = r["sels"]["none"]["device_stages_ms"]
                for s in ("dh", "win"):   # the stages that can hold the summary's kernels, against the plain run's
                    if s in r["sels"]:
                        g = r["sels"][s]["device_stages_ms"]
                        r["sels"][s]["stage_ms"] = g["parse"] + g["fmt_len"] - base["parse"] - base["fmt_len"]
                runs.append(r)
                print(f"round {rnd} {config} {name}: " + ", ".join(
                    f"{s}: device {v['device_ms_per_step']:.2f} ms (parse {v['device_stages_ms']['parse']:.3f}, "
                    f"len {v['device_stages_ms']['fmt_len']:.3f}), pcie {v['pcie_ms_per_step']:.1f} ms" +
                    (f", stage {v['stage_ms']:.3f} ms" if "stage_ms" in v else "") + (f", {v['rows']} rows" if "rows" in v else "")
                    for s, v in r["sels"].items()) + (f"; check {r['rows_check']['equal']}" if "rows_check" in r else ""),
                      flush=True)
        rounds_run += 1
        round_s = time.time() - t_round

    def series(build, config, s, get):
        return [get(r["sels"][s]) for r in runs if r["build"] == build and r["config"] == config and s in r["sels"]]

    summary = {}
    for config in a.configs.split(","):
        c = {}
        for build, _, _, _ in procs:
            for s in SELS:
                if not series(build, config, s, lambda v: 0):
                    continue
                e = {"device_ms_per_step": spread(series(build, config, s, lambda v: v["device_ms_per_step"])),
                     "pcie_ms_per_step": spread(series(build, config, s, lambda v: v["pcie_ms_per_step"])),
                     "bytes_out": series(build, config, s, lambda v: v["pcie_bytes_out"])[0]}
                for stg in STAGES:
                    e[stg + "_ms"] = spread(series(build, config, s, lambda v: v["device_stages_ms"][stg]))
                if s != "none":
                    e["stage_ms"] = spread(series(build, config, s, lambda v: v["stage_ms"]))
                if s == "dh":
                    for k in ("rows", "rows_csv_bytes", "rows_digest", "modal_depth"):
                        e[k] = series(build, config, s, lambda v: v[k])[0]
                c[f"{build}_{s}"] = e
        checks = {r["build"]: r["rows_check"] for r in runs if r["config"] == config and "rows_check" in r}
        if checks:
            c["rows_check"] = checks
            d = {c[b + "_dh"]["rows_digest"] for b in ("this_f0", "this_f1") if b + "_dh" in c}
            c["both_forms_give_the_same_rows"] = len(d) == 1
        summary[config] = c
    doc = {"tool": "tools/gpu/depth_hist_bench.py", "sites": a.sites, "steps": a.steps, "warmup": a.warmup,
           "rounds": rounds_run, "rounds_asked": a.rounds, "window": W,
           "note": "ms per step; device: text and records in HBM (device_sink 1), stages from HIP event pairs in a "
                   "profiled run of the same steps; pcie: pinned host text in, records into the pinned host arena "
                   "(device_sink 2), wall time.  stage_ms: parse + fmt_len (the stages that hold the summary's "
                   "kernels) with the option minus the plain run's, same process.  this_f0 / this_f1: this tree with "
                   "SID_DH_FORM 0 (an LDS atomic a lane) / 1 (a wave's distinct depths one by one).  The processes "
                   "alternate parent / this tree within every round; the spread of a figure is its min .. max over "
                   "the rounds.  D200 has sites * 30 / 200 sites; stage_ms_per_50M_sites scales its figure",
           "comparisons": comparisons(summary, a.sites), "summary": summary, "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
