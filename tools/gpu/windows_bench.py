#!/usr/bin/env python3
"""windows_bench.py -- what --windows W (sid_opts.window) costs, against another
build of the project (its parent commit).

Over the C2 text (seed 2, -m local) and the C3 text (seed 3, -R -m
likelihood_ratio), 50M synthetic 30x sites each, the engine runs

  none     no option
  win      --windows 100000                  (this tree only)
  hetwin   --only het --windows 100000       (this tree only)

  device   text and records in HBM (device_sink 1): the stage times of
           sid_engine_profile_read (HIP event pairs around every stage), per step
  pcie     pinned host text in, records into the pinned host arena
           (device_sink 2 + host_hold_bytes): the step's wall time

The window stage runs inside a stage the engine already brackets -- the tile
parse's (`parse`) for -m local, the length stage (`fmt_len`) for the Lynch
pass 2 -- so its time is that stage's with the option minus the same stage's
of the plain run, same build, same process (window_ms).  With --only het the
difference also holds the marking stage that selects (the selection goes the
context's way under --windows: the unselected parse and tables).

Every (tree, config) pair is a process of its own (a fresh HIP runtime, the
tree's own sid_amd and libsid.so).  The pairs alternate parent / this tree for
--rounds rounds in one session; the spread of a figure is its min .. max over
the rounds.  Each timed window is warmed up by --warmup steps and holds --steps.
A process that fails or runs past --step-timeout ends the whole script.

Once per configuration (this tree, first round) the rows are checked: their
sites add up to the run's, their records to the plain run's record count (its
newlines), the rows with --only het equal the rows without, the records with
the option equal the records without (win against none), and every row is a
window of its chrom in ascending order.

    python tools/gpu/windows_bench.py --parent DIR [--out profiles/windows_bench.json]

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

CONFIGS = {"C2": dict(method="local", R=False, seed=2), "C3": dict(method="likelihood_ratio", R=True, seed=3)}
DEPTH = 30.0
W = 100_000
SELS = {"none": {}, "win": {"window": W}, "hetwin": {"select": "het", "window": W}}
STAGES = ("index", "parse", "call", "hist", "fmt_len", "fmt_write")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--parent", default=None, help="a built checkout of the parent commit (none: this tree only)")
    p.add_argument("--parent-all", action="store_true",
                   help="the parent runs every selection this tree runs (a parent that has them all)")
    p.add_argument("--sites", type=int, default=50_000_000)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--configs", default="C2,C3")
    p.add_argument("--no-check", action="store_true", help="skip the check of the rows")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows_bench.json"))
    p.add_argument("--step-timeout", type=int, default=400, help="seconds a (tree, config) process may take")
    # one (tree, config) process
    p.add_argument("--worker", default=None, metavar="TREE")
    p.add_argument("--config", default="C2")
    p.add_argument("--sels", default="none")
    p.add_argument("--check", action="store_true")
    return p.parse_args(argv)


# ------------------------------------------------------------------ worker --
def worker(a):
    sys.path.insert(0, a.worker)
    import ctypes as C
    import numpy as np
    import torch
    import sid_amd
    assert os.path.dirname(os.path.abspath(sid_amd.__file__)).startswith(os.path.abspath(a.worker))
    cfg = CONFIGS[a.config]
    n = a.sites
    dev = torch.device("cuda", 0)
    cap = int(n * (2.72 * DEPTH + 2) * 1.03) + (64 << 20)
    text = torch.empty(cap, dtype=torch.uint8, device=dev)
    ctx = sid_amd.Context(0)
    ln = ctx.synth_text_device(cfg["seed"], DEPTH, 0, n, text.data_ptr(), cap - 512)
    text[ln:ln + 512].zero_()
    torch.cuda.synchronize(dev)
    ctx.close()
    host = text[:ln].cpu().pin_memory()
    out = {"config": a.config, "sites": n, "text_bytes": ln, "steps": a.steps, "warmup": a.warmup,
           "version": sid_amd.lib().sid_version().decode(), "sels": {}}

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

    rows, digest, newlines = {}, {}, None
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
        if "window" in kw:
            r["device_rows"] = len(eng.windows())
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
        if "window" in kw:
            rows[name] = eng.windows()
            r["rows"] = len(rows[name])
            r["rows_csv_bytes"] = len(sid_amd.windows_format(rows[name]))
        if a.check and name in ("none", "win"):
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
    if a.check and "win" in rows:
        rw = rows["win"]
        ordered = all(r[1] % W == 0 and r[2] == r[1] + W and r[4] == r[5] + r[6] for r in rw) and \
            all(a_[0] != b_[0] or a_[1] < b_[1] for a_, b_ in zip(rw, rw[1:]))
        out["rows_check"] = {"rows": len(rw), "sites_sum": sum(r[3] for r in rw), "sites": n,
                             "records_sum": sum(r[4] for r in rw), "records_of_the_plain_run": newlines,
                             "het_sum": sum(r[5] for r in rw), "windows_in_order": ordered,
                             "rows_equal_with_only_het": rows.get("hetwin") == rw,
                             "records_equal_with_and_without": digest.get("win") == digest.get("none"),
                             "equal": bool(sum(r[3] for r in rw) == n and sum(r[4] for r in rw) == newlines and ordered and
                                           rows.get("hetwin") == rw and digest.get("win") == digest.get("none"))}
    print("WINDOWS_BENCH " + json.dumps(out), flush=True)
    return 0


# ------------------------------------------------------------------ driver --
def spread(xs):
    xs = list(xs)
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def comparisons(summary):
    def rng(e, k):
        return [round(e[k]["min"], 3), round(e[k]["max"], 3)]

    out = {}
    keys = ["device_ms_per_step", "pcie_ms_per_step"] + [s + "_ms" for s in STAGES]
    for config, c in summary.items():
        if "parent_none" not in c:
            continue
        o = {}
        p, t = c["parent_none"], c["this_none"]
        o["unchanged_without_the_option"] = {
            "met": all(rng(t, k)[0] <= rng(p, k)[1] and rng(p, k)[0] <= rng(t, k)[1] for k in keys),
            "this": {k: rng(t, k) for k in keys}, "parent": {k: rng(p, k) for k in keys}}
        w, h = c["this_win"], c["this_hetwin"]
        o["window_cost"] = {
            "window_ms": {"win": rng(w, "window_ms"), "hetwin": rng(h, "window_ms")},
            "device_ms_per_step": {"win": rng(w, "device_ms_per_step"), "hetwin": rng(h, "device_ms_per_step"),
                                   "none": rng(t, "device_ms_per_step"), "parent_none": rng(p, "device_ms_per_step")},
            "pcie_ms_per_step": {"win": rng(w, "pcie_ms_per_step"), "hetwin": rng(h, "pcie_ms_per_step"),
                                 "none": rng(t, "pcie_ms_per_step"), "parent_none": rng(p, "pcie_ms_per_step")}}
        pw, pp = rng(w, "pcie_ms_per_step"), rng(p, "pcie_ms_per_step")
        o["pcie_step_with_windows_overlaps_parent_unselected"] = {
            "met": pw[0] <= pp[1] and pp[0] <= pw[1], "win": pw, "parent_none": pp,
            "apart_by_ms": round(max(pw[0] - pp[1], pp[0] - pw[1], 0.0), 3)}
        width = (p["pcie_ms_per_step"]["max"] - p["pcie_ms_per_step"]["min"]) + \
                (h["pcie_ms_per_step"]["max"] - h["pcie_ms_per_step"]["min"])
        o["pcie_step_only_het_windows_below_parent_unselected_by_more_than_both_ranges"] = {
            "met": h["pcie_ms_per_step"]["max"] < p["pcie_ms_per_step"]["min"] - width,
            "hetwin": rng(h, "pcie_ms_per_step"), "parent_none": pp, "combined_width": round(width, 3)}
        out[config] = o
    return out


def main():
    a = parse_args()
    if a.worker:
        return worker(a)
    runs = []
    trees = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("this", ROOT)]
    for rnd in range(a.rounds):
        for config in a.configs.split(","):
            for name, tree in trees:
                check = name == "this" and rnd == 0 and not a.no_check
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", tree, "--config", config, "--sites",
                       str(a.sites), "--steps", str(a.steps), "--warmup", str(a.warmup), "--sels",
                       "none,win,hetwin" if name == "this" or a.parent_all else "none"] + (["--check"] if check else [])
                env = dict(os.environ)
                env.pop("SID_LIB_PATH", None)   # each tree loads its own build/libsid.so
                # (a process of its own under its own time limit; a failure or a timeout ends the script)
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, env=env)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("WINDOWS_BENCH ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit(f"windows_bench: {name} {config} failed (exit {p.returncode})")
                r = json.loads(line[0][len("WINDOWS_BENCH "):])
                r["build"], r["round"] = name, rnd
                stage = "parse" if config == "C2" else "fmt_len"   # the stage that holds the window kernels
                for s in ("win", "hetwin"):
                    if s in r["sels"]:
                        r["sels"][s]["window_ms"] = (r["sels"][s]["device_stages_ms"][stage] -
                                                     r["sels"]["none"]["device_stages_ms"][stage])
                runs.append(r)
                print(f"round {rnd} {config} {name}: " + ", ".join(
                    f"{s}: device {v['device_ms_per_step']:.2f} ms (parse {v['device_stages_ms']['parse']:.3f}, "
                    f"len {v['device_stages_ms']['fmt_len']:.3f}, write {v['device_stages_ms']['fmt_write']:.3f}), "
                    f"pcie {v['pcie_ms_per_step']:.1f} ms, {v['pcie_bytes_out']} B" + (f", {v['rows']} rows" if "rows" in v else "")
                    for s, v in r["sels"].items()) + (f"; check {r['rows_check']['equal']}" if "rows_check" in r else ""),
                      flush=True)

    def series(build, config, s, get):
        return [get(r["sels"][s]) for r in runs if r["build"] == build and r["config"] == config and s in r["sels"]]

    summary = {}
    for config in a.configs.split(","):
        c = {}
        for build, _ in trees:
            for s in SELS:
                if not series(build, config, s, lambda v: 0):
                    continue
                e = {"device_ms_per_step": spread(series(build, config, s, lambda v: v["device_ms_per_step"])),
                     "pcie_ms_per_step": spread(series(build, config, s, lambda v: v["pcie_ms_per_step"])),
                     "bytes_out": series(build, config, s, lambda v: v["pcie_bytes_out"])[0]}
                for stg in STAGES:
                    e[stg + "_ms"] = spread(series(build, config, s, lambda v: v["device_stages_ms"][stg]))
                if s != "none":
                    e["window_ms"] = spread(series(build, config, s, lambda v: v["window_ms"]))
                    e["rows"] = series(build, config, s, lambda v: v["rows"])[0]
                    e["rows_csv_bytes"] = series(build, config, s, lambda v: v["rows_csv_bytes"])[0]
                c[f"{build}_{s}"] = e
        checks = [r["rows_check"] for r in runs if r["config"] == config and "rows_check" in r]
        if checks:
            c["rows_check"] = checks[0]
        summary[config] = c
    doc = {"tool": "tools/gpu/windows_bench.py", "sites": a.sites, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "depth": DEPTH, "window": W,
           "note": "ms per step; device: text and records in HBM (device_sink 1), stages from HIP event pairs in a "
                   "profiled run of the same steps; pcie: pinned host text in, records into the pinned host arena "
                   "(device_sink 2), wall time.  window_ms: the stage that holds the window kernels (C2: parse, "
                   "the tile parse; C3: fmt_len) with the option minus the plain run's, same process (hetwin: the "
                   "selecting marks included).  parent / this tree alternate within every round; the spread of a "
                   "figure is its min .. max over the rounds",
           "comparisons": comparisons(summary), "summary": summary, "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
