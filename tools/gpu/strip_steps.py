"""strip_steps.py -- what the strip crews (sid_engine_cfg.strip)
do to bench.py's step, against a built checkout of the parent commit.

Every measurement is `python bench.py --gpus 1 --steps S --warmup W [--config
C]` as a process of its own in its tree, under its own time limit; the parent
and this tree alternate within every round of C2, then one round each of the
--also configs, then on this tree one C2 run with SID_ENGINE_TIMING set (the
crews' busy time -- summed, and the least and most busy thread's --,
chunks_stripped, strip_bytes and h2d_bytes of every step, from the engine's
stderr lines) and, with --full, one `--full --no-cpu` run (spot_check,
device_path).  A process that fails or prints no result line ends the script
before anything else starts.  Writes one JSON file (profiles/strip_bench.json).

  python tools/gpu/strip_steps.py --parent ../parent [--rounds 3] [--also C3,C5] [--full]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KEEP = ("ms_per_step", "value")
PCIE = ("ingest_s", "h2d_s_last_step", "h2d_GBps_last_step", "chunks", "tile_overflows_last_step", "text_bytes")


def bench(tree, args, timeout, env=None):
    """One bench.py process in `tree`: (its result line as a dict, its stderr)."""
    cmd = [sys.executable, "bench.py", "--gpus", "1"] + args
    r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})))
    line = next((l for l in reversed(r.stdout.splitlines()) if l.startswith("{")), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stderr[-3000:])
        raise SystemExit(f"strip_steps: {' '.join(cmd)} in {tree}: exit status {r.returncode}")
    return json.loads(line), r.stderr


def brief(out):
    b = {k: out[k] for k in KEEP}
    b.update({k: out["pcie"].get(k) for k in PCIE})
    b["pcie_ceiling_frac"] = out["pcie"]["ceiling"].get("frac")
    return b


def spread(runs, key="ms_per_step"):
    v = [r[key] for r in runs]
    return {"min": min(v), "max": max(v), "runs": v}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--parent", required=True, help="a built checkout of the parent commit")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--also", default="C3,C5", help="configs measured for one round more (none: '')")
    p.add_argument("--full", action="store_true", help="one --full --no-cpu run of this tree")
    p.add_argument("--step-timeout", type=int, default=240, help="seconds a bench.py process may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "strip_bench.json"))
    a = p.parse_args()
    trees = {"parent": os.path.abspath(a.parent), "this": ROOT}
    base = ["--steps", str(a.steps), "--warmup", str(a.warmup)]
    res = {"command": "bench.py --gpus 1 " + " ".join(base), "rounds": a.rounds, "C2": {"parent": [], "this": []}}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for rnd in range(a.rounds):
        for name in ("parent", "this"):
            out, _ = bench(trees[name], base, a.step_timeout)
            res["C2"][name].append(brief(out))
            print(f"round {rnd} C2 {name}: {out['ms_per_step']:.2f} ms/step", flush=True)
            save()
    res["C2"]["ms_per_step"] = {k: spread(v) for k, v in res["C2"].items() if k in trees}
    for config in [c for c in a.also.split(",") if c]:
        res[config] = {}
        for name in ("parent", "this"):
            out, _ = bench(trees[name], base + ["--config", config], a.step_timeout)
            res[config][name] = brief(out)
            print(f"{config} {name}: {out['ms_per_step']:.2f} ms/step", flush=True)
            save()
    # the crews' own figures: the engine's SID_ENGINE_TIMING line of every ingest
    out, err = bench(trees["this"], base, a.step_timeout, env={"SID_ENGINE_TIMING": "1"})
    steps = [json.loads(l) for l in err.splitlines() if l.startswith('{"engine_phase": "ingest"')]
    timed = steps[-a.steps:]
    res["C2"]["this_timed"] = {
        "note": "SID_ENGINE_TIMING=1 (a stream sync more per step); per timed step, min .. max; strip_busy_s: the "
                "crew's threads summed, strip_busy_min_s / _max_s: the least and the most busy thread of a step; "
                "h2d_bytes: the engine's count of the bytes its copies moved",
        "ms_per_step": out["ms_per_step"], "strip_threads": timed[-1]["strip_threads"],
        **{k: {"min": min(s[k] for s in timed), "max": max(s[k] for s in timed)}
           for k in ("strip_busy_s", "strip_busy_min_s", "strip_busy_max_s", "chunks_stripped", "strip_bytes",
                     "h2d_bytes")}}
    save()
    if a.full:
        out, _ = bench(trees["this"], base + ["--full", "--no-cpu"], 3 * a.step_timeout)
        res["full"] = {"ms_per_step": out["ms_per_step"], "spot_check": out.get("spot_check"),
                       "device_path": {k: out["device_path"].get(k) for k in ("ms_per_step", "stages_ms")}}
        save()
    print(json.dumps(res["C2"]["ms_per_step"]))


if __name__ == "__main__":
    main()
