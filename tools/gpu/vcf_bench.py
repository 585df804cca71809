#!/usr/bin/env python3
"""vcf_bench.py -- what the VCF format (--vcf, sid_engine_set_format) costs,
against this build's CSV and against another build of the project (its parent
commit).

Over the C2 text (seed 2, -m local) and the C3 text (seed 3, -R -m
likelihood_ratio), 50M synthetic 30x sites each (one chrom, positions 1..n),
the engine runs with the CSV format (csv: every build) and with the VCF format
(vcf: this build):

  device   text and records in HBM (device_sink 1): the stage times of
           sid_engine_profile_read (HIP event pairs around every stage), per step
  pcie     pinned host text in, records into the pinned host arena
           (device_sink 2 + host_hold_bytes): the step's wall time

What the brackets separate.  The VCF stage is a length kernel and a writer in
place of the CSV's.  On C3 (the Lynch pass 2) the length kernel is the `fmt_len`
stage and the writer the `fmt_write` stage.  On C2 (-m local, one pass) the CSV
has no length kernel at all -- its lengths come out of the tile parse -- so the
VCF length kernel shows as the `parse` bracket with the option minus without
it (len_ms), of the same build in the same process; the writer is `fmt_write`.
write_gbps is the records' bytes over the writer's time.

Every (tree, config) pair is a process of its own (a fresh HIP runtime, the
tree's own sid_amd and libsid.so); the parent tree, which has no such option,
runs the CSV only.  The pairs alternate parent / this tree for --rounds rounds
in one session, so the spread between rounds of the same code stands beside
every difference between the two.

    python tools/gpu/vcf_bench.py --parent DIR [--out profiles/vcf_bench.json]

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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_bench.json"))
    p.add_argument("--step-timeout", type=int, default=300, help="seconds a (tree, config) process may take")
    # one (tree, config) process
    p.add_argument("--worker", default=None, metavar="TREE")
    p.add_argument("--config", default="C2")
    p.add_argument("--sets", default="csv")
    return p.parse_args(argv)


# ------------------------------------------------------------------ worker --
def worker(a):
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
    KW = {"csv": {}, "vcf": dict(format="vcf")}
    ARENA = {"csv": 48, "vcf": 72}   # host arena bytes a site: the whole run's records fit

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
                             host_hold_bytes=int(n * ARENA[name]) + (64 << 20), **kw)
        eng.source_host_ptr(host.data_ptr(), ln, keep=host)
        for _ in range(a.warmup):
            step(eng)
        r["pcie_ms_per_step"], st, st2 = timed(eng, a.steps)
        r["pcie_bytes_out"] = st2.bytes_out
        r["pcie_chunks"] = st.chunks
        r["pcie_chunks_held"] = st.chunks_held
        eng.close()
        out["sets"][name] = r
    print("VCF_BENCH " + json.dumps(out), flush=True)
    return 0


# ------------------------------------------------------------------ driver --
def spread(xs):
    xs = list(xs)
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def comparisons(summary):
    """The comparisons the change is judged by, each stated with its ranges (min .. max over the rounds)."""
    def rng(e, k):
        return [round(e[k]["min"], 3), round(e[k]["max"], 3)]

    out = {}
    for config, c in summary.items():
        o = {}
        n = c["this_csv"]
        keys = ["device_ms_per_step", "pcie_ms_per_step"] + [s + "_ms" for s in STAGES]
        if "parent_csv" in c:
            p = c["parent_csv"]
            o["1_without_the_option_within_parent_spread"] = {
                "met": all(rng(n, k)[0] <= rng(p, k)[1] and rng(p, k)[0] <= rng(n, k)[1] for k in keys),
                "overlap": {k: rng(n, k)[0] <= rng(p, k)[1] and rng(p, k)[0] <= rng(n, k)[1] for k in keys},
                "this": {k: rng(n, k) for k in keys}, "parent": {k: rng(p, k) for k in keys}}
        if "this_vcf" in c:
            v = c["this_vcf"]
            o["2_vcf_against_csv"] = {
                "bytes_out": {"csv": n["bytes_out"], "vcf": v["bytes_out"],
                              "ratio": round(v["bytes_out"] / max(n["bytes_out"], 1), 4),
                              "vcf_bytes_per_site": round(v["bytes_out"] / c["sites"], 2),
                              "text_bytes_per_site": round(c["text_bytes"] / c["sites"], 2)},
                "length_stage": "parse, with the option minus without (C2: the CSV's lengths come out of the parse)"
                                if config == "C2" else "fmt_len",
                "len_ms": {"csv": rng(n, "len_ms"), "vcf": rng(v, "len_ms")},
                "fmt_write_ms": {"csv": rng(n, "fmt_write_ms"), "vcf": rng(v, "fmt_write_ms")},
                "write_gbps": {"csv": rng(n, "write_gbps"), "vcf": rng(v, "write_gbps")},
                "device_ms_per_step": {"csv": rng(n, "device_ms_per_step"), "vcf": rng(v, "device_ms_per_step")},
                "pcie_ms_per_step": {"csv": rng(n, "pcie_ms_per_step"), "vcf": rng(v, "pcie_ms_per_step")}}
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
                sets = {"parent": "csv", "this": "csv,vcf"}[name]
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", tree, "--config", config, "--sites",
                       str(a.sites), "--steps", str(a.steps), "--warmup", str(a.warmup), "--sets", sets]
                env = dict(os.environ)
                env.pop("SID_LIB_PATH", None)   # each tree loads its own build/libsid.so
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, env=env)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("VCF_BENCH ")]
                if p.returncode != 0 or not line:   # (a failure ends the script: nothing more starts on the GPU)
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit(f"vcf_bench: {name} {config} failed (exit {p.returncode})")
                r = json.loads(line[0][len("VCF_BENCH "):])
                r["build"], r["round"] = name, rnd
                stage = "parse" if config == "C2" else "fmt_len"
                for s, v in r["sets"].items():
                    # the length stage: C3's fmt_len bracket; C2's parse bracket less the CSV's, same process
                    v["len_ms"] = v["device_stages_ms"][stage] - (r["sets"]["csv"]["device_stages_ms"][stage]
                                                                  if config == "C2" else 0.0)
                    v["write_gbps"] = v["device_bytes_out"] / max(v["device_stages_ms"]["fmt_write"], 1e-9) / 1e6
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
            for s in ("csv", "vcf"):
                if not series(build, config, s, lambda v: 0):
                    continue
                e = {"device_ms_per_step": spread(series(build, config, s, lambda v: v["device_ms_per_step"])),
                     "pcie_ms_per_step": spread(series(build, config, s, lambda v: v["pcie_ms_per_step"])),
                     "len_ms": spread(series(build, config, s, lambda v: v["len_ms"])),
                     "write_gbps": spread(series(build, config, s, lambda v: v["write_gbps"])),
                     "bytes_out": series(build, config, s, lambda v: v["pcie_bytes_out"])[0],
                     "pcie_chunks_held": series(build, config, s, lambda v: v.get("pcie_chunks_held", 0))[0]}
                for stg in STAGES:
                    e[stg + "_ms"] = spread(series(build, config, s, lambda v: v["device_stages_ms"][stg]))
                c[f"{build}_{s}"] = e
        first = [r for r in runs if r["config"] == config][0]
        c["sites"], c["text_bytes"] = first["sites"], first["text_bytes"]
        summary[config] = c
    doc = {"tool": "tools/gpu/vcf_bench.py", "sites": a.sites, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "depth": DEPTH,
           "note": "ms per step; device: text and records in HBM (device_sink 1), stages from HIP event pairs in a "
                   "profiled run of the same steps; pcie: pinned host text in, records into the pinned host arena "
                   "(device_sink 2), wall time.  len_ms: C3's fmt_len stage; C2's parse stage with the format minus "
                   "the CSV's, same process (the CSV's lengths come out of the tile parse).  write_gbps: the "
                   "records' bytes over fmt_write.  parent / this tree alternate within every round; the spread of "
                   "a figure is its min .. max over the rounds",
           "comparisons": comparisons(summary), "summary": summary, "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
