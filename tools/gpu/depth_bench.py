#!/usr/bin/env python3
"""depth_bench.py -- what the depth bounds (--min-depth / --max-depth,
sid_engine_set_depth) cost and save, against another build of the project (its
parent commit).

Over the C2 text (seed 2, -m local) and the C3 text (seed 3, -R -m
likelihood_ratio), 50M synthetic 30x sites each (one chrom, positions 1..n),
the engine runs without a selection, with bounds that keep about half the
records (half: min 30 of the generator's 30x mean), with bounds that keep a few
percent (tight: min 40), with --variants, and with --variants and the half
bounds together -- the latter once with the two tests in one kernel (both) and
once, in a process of its own under SID_DEPTH_SPLIT=1, as two kernels one
after the other (both_split):

  device   text and records in HBM (device_sink 1): the stage times of
           sid_engine_profile_read (HIP event pairs around every stage), per step
  pcie     pinned host text in, records into the pinned host arena
           (device_sink 2 + host_hold_bytes): the step's wall time

What the brackets separate.  The bounds add no per-site state to the parse, so
the only new device work is the marking kernel: on C3 (the Lynch pass 2 marks)
it is the `fmt_len` stage with the option minus without it, on C2 (-m local,
one pass) the tile parse's `parse` bracket holds it; mark_ms is that
difference, of the same build in the same process.

Every (tree, config) pair is a process of its own (a fresh HIP runtime, the
tree's own sid_amd and libsid.so); the parent tree, which has no such option,
runs without a selection.  The pairs alternate parent / this tree for --rounds
rounds in one session, so the spread between rounds of the same code stands
beside every difference between the two.

    python tools/gpu/depth_bench.py --parent DIR [--out profiles/depth_bench.json]

DIR is a checkout of the parent commit built with `make` (build/libsid.so).
Needs an MI355X; there is no CPU fallback."""
import argparse
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
STAGES = ("index", "parse", "call", "hist", "fmt_len", "fmt_write")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--parent", default=None, help="a built checkout of the parent commit (none: this tree only)")
    p.add_argument("--sites", type=int, default=50_000_000)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--configs", default="C2,C3")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_bench.json"))
    p.add_argument("--step-timeout", type=int, default=600, help="seconds a (tree, config) process may take")
    # one (tree, config) process
    p.add_argument("--worker", default=None, metavar="TREE")
    p.add_argument("--config", default="C2")
    p.add_argument("--sets", default="none")
    p.add_argument("--split", action="store_true", help="SID_DEPTH_SPLIT=1: two kernels for variants + bounds")
    return p.parse_args(argv)


# ------------------------------------------------------------------ worker --
HALF, TIGHT = (30, 0), (40, 0)


def worker(a):
    if a.split:
        os.environ["SID_DEPTH_SPLIT"] = "1"
    sys.path.insert(0, a.worker)
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
           "version": sid_amd.lib().sid_version().decode(), "sets": {}}
    KW = {"none": {}, "variants": {"variants": 1},
          "half": dict(min_depth=HALF[0], max_depth=HALF[1]), "tight": dict(min_depth=TIGHT[0], max_depth=TIGHT[1]),
          "both": dict(variants=1, min_depth=HALF[0], max_depth=HALF[1])}
    KW["both_split"] = KW["both"]

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

    for name in a.sets.split(","):
        kw = KW[name]
        r = {}
        # text and records in HBM: the kernels, per stage
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
        eng.close()
        r["device_stages_ms"] = {k[:-3]: v / a.steps for k, v in prof.items() if k.endswith("_ms")}
        r["device_chunks_per_step"] = prof["chunks"] / a.steps
        r["device_bytes_out"] = st2.bytes_out
        r["chunks_tiled"] = st.chunks_tiled
        r["tile_overflows"] = st.tile_overflows
        # the PCIe path: host text in, records into the pinned host arena
        eng = sid_amd.Engine(method=cfg["method"], estimate_prior=cfg["R"], devices=1, device_sink=2,
                             host_hold_bytes=int(n * 48) + (64 << 20), **kw)
        eng.source_host_ptr(host.data_ptr(), ln, keep=host)
        for _ in range(a.warmup):
            step(eng)
        r["pcie_ms_per_step"], st, st2 = timed(eng, a.steps)
        r["pcie_bytes_out"] = st2.bytes_out
        r["pcie_chunks"] = st.chunks
        eng.close()
        out["sets"][name] = r
    print("DEPTH_BENCH " + json.dumps(out), flush=True)
    return 0


# ------------------------------------------------------------------ driver --
def spread(xs):
    xs = list(xs)
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


OPTS = ("half", "tight", "variants", "both", "both_split")


def comparisons(summary):
    """The comparisons the change is judged by, each stated with its ranges (min .. max over the rounds)."""
    def rng(e, k):
        return [round(e[k]["min"], 3), round(e[k]["max"], 3)]

    out = {}
    for config, c in summary.items():
        o = {}
        n = c["this_none"]
        keys = ["device_ms_per_step", "pcie_ms_per_step"] + [s + "_ms" for s in STAGES]
        if "parent_none" in c:
            p = c["parent_none"]
            o["1_without_the_option_within_parent_spread"] = {
                "met": all(rng(n, k)[0] <= rng(p, k)[1] and rng(p, k)[0] <= rng(n, k)[1] for k in keys),
                "overlap": {k: rng(n, k)[0] <= rng(p, k)[1] and rng(p, k)[0] <= rng(n, k)[1] for k in keys},
                "this": {k: rng(n, k) for k in keys}, "parent": {k: rng(p, k) for k in keys}}
        have = [s for s in OPTS if f"this_{s}" in c]
        o["2_marking_stage_ms"] = {"stage": "parse" if config == "C2" else "fmt_len",
                                   **{s: rng(c[f"this_{s}"], "mark_ms") for s in have}}
        o["3_writer_device_path_and_pcie"] = {
            k: {"none": rng(n, k), **{s: rng(c[f"this_{s}"], k) for s in have}}
            for k in ("fmt_write_ms", "device_ms_per_step", "pcie_ms_per_step")}
        o["kept_bytes"] = {"none": n["bytes_out"], **{s: c[f"this_{s}"]["bytes_out"] for s in have}}
        o["kept_share"] = {s: round(c[f"this_{s}"]["bytes_out"] / max(n["bytes_out"], 1), 6) for s in have}
        out[config] = o
    return out


def main():
    a = parse_args()
    if a.worker:
        return worker(a)
    runs = []
    trees = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("this", ROOT), ("this_split", ROOT)]
    for rnd in range(a.rounds):
        for config in a.configs.split(","):
            for name, tree in trees:
                sets = {"parent": "none", "this": "none,half,tight,variants,both", "this_split": "none,both_split"}[name]
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", tree, "--config", config, "--sites",
                       str(a.sites), "--steps", str(a.steps), "--warmup", str(a.warmup), "--sets", sets] + \
                      (["--split"] if name == "this_split" else [])
                env = dict(os.environ)
                env.pop("SID_LIB_PATH", None)   # each tree loads its own build/libsid.so
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, env=env)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("DEPTH_BENCH ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit(f"depth_bench: {name} {config} failed (exit {p.returncode})")
                r = json.loads(line[0][len("DEPTH_BENCH "):])
                r["build"], r["round"] = name, rnd
                stage = "parse" if config == "C2" else "fmt_len"
                for s, v in r["sets"].items():   # (the marking stage: with the option minus without, same process)
                    if s != "none":
                        v["mark_ms"] = v["device_stages_ms"][stage] - r["sets"]["none"]["device_stages_ms"][stage]
                if name == "this_split":   # (its own unselected run was only the subtrahend)
                    r["build"] = "this"
                    del r["sets"]["none"]
                runs.append(r)
                print(f"round {rnd} {config} {name}: " + ", ".join(
                    f"{s}: device {v['device_ms_per_step']:.2f} ms (parse {v['device_stages_ms']['parse']:.3f}, "
                    f"len {v['device_stages_ms']['fmt_len']:.3f}, write {v['device_stages_ms']['fmt_write']:.3f}), "
                    f"pcie {v['pcie_ms_per_step']:.1f} ms, {v['pcie_bytes_out']} B"
                    for s, v in r["sets"].items()), flush=True)

    def series(build, config, s, get):
        return [get(r["sets"][s]) for r in runs if r["build"] == build and r["config"] == config and s in r["sets"]]

    summary = {}
    for config in a.configs.split(","):
        c = {}
        for build in ("parent", "this"):
            for s in ("none",) + OPTS:
                if not series(build, config, s, lambda v: 0):
                    continue
                e = {"device_ms_per_step": spread(series(build, config, s, lambda v: v["device_ms_per_step"])),
                     "pcie_ms_per_step": spread(series(build, config, s, lambda v: v["pcie_ms_per_step"])),
                     "bytes_out": series(build, config, s, lambda v: v["pcie_bytes_out"])[0]}
                for stg in STAGES:
                    e[stg + "_ms"] = spread(series(build, config, s, lambda v: v["device_stages_ms"][stg]))
                if s != "none":
                    e["mark_ms"] = spread(series(build, config, s, lambda v: v["mark_ms"]))
                c[f"{build}_{s}"] = e
        summary[config] = c
    doc = {"tool": "tools/gpu/depth_bench.py", "sites": a.sites, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "depth": DEPTH,
           "bounds": {"half": list(HALF), "tight": list(TIGHT)},
           "note": "ms per step; device: text and records in HBM (device_sink 1), stages from HIP event pairs in a "
                   "profiled run of the same steps; pcie: pinned host text in, records into the pinned host arena "
                   "(device_sink 2), wall time.  mark_ms: the parse (C2) / fmt_len (C3) stage with the option minus "
                   "without, same process: the marking kernel(s); both: variants and bounds in one kernel, "
                   "both_split: SID_DEPTH_SPLIT=1, two kernels.  parent / this tree alternate within "
                   "every round; the spread of a figure is its min .. max over the rounds",
           "comparisons": comparisons(summary), "summary": summary, "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
