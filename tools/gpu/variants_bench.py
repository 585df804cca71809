#!/usr/bin/env python3
"""variants_bench.py -- what keeping the reference byte and the selection of
the variants (--variants, sid_opts.variants) cost and save, against another
build of the project (its parent commit).

Over the C2 text (seed 2, -m local) and the C3 text (seed 3, -R -m
likelihood_ratio), 50M synthetic 30x sites each (one chrom, positions 1..n),
the engine runs without a selection, with the option, and with --only het on
the same text:

  device   text and records in HBM (device_sink 1): the stage times of
           sid_engine_profile_read (HIP event pairs around every stage), per step
  pcie     pinned host text in, records into the pinned host arena
           (device_sink 2 + host_hold_bytes): the step's wall time

What the brackets separate.  C3 (the Lynch pass 1 parses, pass 2 marks): the
`parse` stage with the option minus without it is the byte store of the tile
parse and its compaction (store_ms); the `fmt_len` stage's difference is the
marking kernel (mark_ms).  C2 (-m local, one pass): both sit inside the tile
parse's `parse` bracket, so its difference is their sum (parse_delta_ms).  All
differences are of the same build in the same process.

The synthetic generator draws the reference base uniformly from A, C, G, T and
makes no hom-alt sites: the option keeps about the hets plus the sites where
errors won the call.  kept_share is the kept records' bytes over all records'.

Every (tree, config) pair is a process of its own (a fresh HIP runtime, the
tree's own sid_amd and libsid.so); the parent tree, which has no such option,
runs without a selection and with --only het.  The pairs alternate parent /
this tree for --rounds rounds in one session, so the spread between rounds of
the same code stands beside every difference between the two.

Once per configuration (this tree, first round) the het records of the run with
the option are compared, chunk by chunk, with the records of the --only het
run (every het on an A, C, G or T reference is a variant); the hom records it
keeps are counted.  (What is kept is checked line by line by the tests.)

    python tools/gpu/variants_bench.py --parent DIR [--out profiles/variants_bench.json]

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
STAGES = ("index", "parse", "call", "hist", "fmt_len", "fmt_write")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--parent", default=None, help="a built checkout of the parent commit (none: this tree only)")
    p.add_argument("--sites", type=int, default=50_000_000)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--configs", default="C2,C3")
    p.add_argument("--no-check", action="store_true", help="skip the comparison of the records")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "variants_bench.json"))
    p.add_argument("--step-timeout", type=int, default=600, help="seconds a (tree, config) process may take")
    # one (tree, config) process
    p.add_argument("--worker", default=None, metavar="TREE")
    p.add_argument("--config", default="C2")
    p.add_argument("--sets", default="none")
    p.add_argument("--check", action="store_true")
    return p.parse_args(argv)


# ------------------------------------------------------------------ worker --
def by_label(raw, np):
    """(the het records' bytes, the hom records' bytes) of a chunk's records."""
    a = np.frombuffer(raw, np.uint8)
    if a.size == 0:
        return b"", b""
    nl = np.flatnonzero(a == 10)
    ls = np.concatenate(([0], nl[:-1] + 1))
    commas = np.flatnonzero(a == 44)
    c2 = commas[np.searchsorted(commas, ls) + 1]   # "chr1,<pos>,het,": the second comma of the line
    het = a[c2 + 2] == ord("e")
    per = np.repeat(het, nl + 1 - ls)
    return a[per].tobytes(), a[~per].tobytes()


def worker(a):
    sys.path.insert(0, a.worker)
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
           "version": sid_amd.lib().sid_version().decode(), "sets": {}}
    KW = {"none": {}, "variants": {"variants": 1}, "het": {"select": "het"}}

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

    recs = {}
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
        if a.check and name != "none":
            import ctypes as C
            d = []
            for j in range(st.chunks):
                p, m = eng.records(j)
                raw = C.string_at(p, m) if m else b""
                het, hom = by_label(raw, np)
                d.append((hashlib.blake2b(het).hexdigest(), len(het), hom.count(b"\n")))
            recs[name] = d
        eng.close()
        out["sets"][name] = r
    if a.check and "variants" in recs and "het" in recs:
        v, h = recs["variants"], recs["het"]
        out["records_check"] = {
            "chunks": len(v),
            "het_records_equal_only_het": len(v) == len(h) and all(x[:2] == y[:2] for x, y in zip(v, h)),
            "only_het_has_no_hom": all(y[2] == 0 for y in h),
            "het_bytes": sum(x[1] for x in v), "hom_records_kept": sum(x[2] for x in v)}
    print("VARIANTS_BENCH " + json.dumps(out), flush=True)
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
        n, v, h = c["this_none"], c["this_variants"], c["this_het"]
        keys = ["device_ms_per_step", "pcie_ms_per_step"] + [s + "_ms" for s in STAGES]
        if "parent_none" in c:
            p = c["parent_none"]
            o["1_without_the_option_within_parent_spread"] = {
                "met": all(rng(n, k)[0] <= rng(p, k)[1] and rng(p, k)[0] <= rng(n, k)[1] for k in keys),
                "this": {k: rng(n, k) for k in keys}, "parent": {k: rng(p, k) for k in keys}}
        o["2_parse_stage_with_and_without"] = {"with": rng(v, "parse_ms"), "without": rng(n, "parse_ms"),
                                               "delta_ms": rng(v, "parse_delta_ms"),
                                               "holds": "the byte store and the marking kernel" if config == "C2"
                                                        else "the byte store (tile parse + compaction)"}
        o["3_marking_stage"] = ({"mark_ms": rng(v, "mark_ms"), "stage": "fmt_len"} if config != "C2" else
                                {"inside": "parse_delta_ms (the tile parse's bracket holds the marking kernel too)"})
        o["4_writer_and_pcie_against_only_het"] = {
            "fmt_write_ms": {"variants": rng(v, "fmt_write_ms"), "het": rng(h, "fmt_write_ms"),
                             "none": rng(n, "fmt_write_ms")},
            "pcie_ms_per_step": {"variants": rng(v, "pcie_ms_per_step"), "het": rng(h, "pcie_ms_per_step"),
                                 "none": rng(n, "pcie_ms_per_step")},
            "device_ms_per_step": {"variants": rng(v, "device_ms_per_step"), "het": rng(h, "device_ms_per_step"),
                                   "none": rng(n, "device_ms_per_step")}}
        o["kept_share"] = {"variants": round(v["bytes_out"] / max(n["bytes_out"], 1), 6),
                           "het": round(h["bytes_out"] / max(n["bytes_out"], 1), 6)}
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
                       str(a.sites), "--steps", str(a.steps), "--warmup", str(a.warmup), "--sets",
                       "none,variants,het" if name == "this" else "none,het"] + (["--check"] if check else [])
                env = dict(os.environ)
                env.pop("SID_LIB_PATH", None)   # each tree loads its own build/libsid.so
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, env=env)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("VARIANTS_BENCH ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit(f"variants_bench: {name} {config} failed (exit {p.returncode})")
                r = json.loads(line[0][len("VARIANTS_BENCH "):])
                r["build"], r["round"] = name, rnd
                if "variants" in r["sets"]:
                    v, n0 = r["sets"]["variants"], r["sets"]["none"]
                    v["parse_delta_ms"] = v["device_stages_ms"]["parse"] - n0["device_stages_ms"]["parse"]
                    v["mark_ms"] = v["device_stages_ms"]["fmt_len"] - n0["device_stages_ms"]["fmt_len"]
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
        for build, _ in trees:
            for s in ("none", "variants", "het"):
                if not series(build, config, s, lambda v: 0):
                    continue
                e = {"device_ms_per_step": spread(series(build, config, s, lambda v: v["device_ms_per_step"])),
                     "pcie_ms_per_step": spread(series(build, config, s, lambda v: v["pcie_ms_per_step"])),
                     "bytes_out": series(build, config, s, lambda v: v["pcie_bytes_out"])[0]}
                for stg in STAGES:
                    e[stg + "_ms"] = spread(series(build, config, s, lambda v: v["device_stages_ms"][stg]))
                if s == "variants":
                    e["parse_delta_ms"] = spread(series(build, config, s, lambda v: v["parse_delta_ms"]))
                    e["mark_ms"] = spread(series(build, config, s, lambda v: v["mark_ms"]))
                c[f"{build}_{s}"] = e
        checks = [r["records_check"] for r in runs if r["config"] == config and "records_check" in r]
        if checks:
            c["records_check"] = checks[0]
        summary[config] = c
    doc = {"tool": "tools/gpu/variants_bench.py", "sites": a.sites, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "depth": DEPTH,
           "note": "ms per step; device: text and records in HBM (device_sink 1), stages from HIP event pairs in a "
                   "profiled run of the same steps; pcie: pinned host text in, records into the pinned host arena "
                   "(device_sink 2), wall time.  parse_delta_ms / mark_ms: the parse / fmt_len stage with the option "
                   "minus without, same process (C2: the parse bracket holds the byte store and the marking kernel; "
                   "C3: parse holds the store, fmt_len the marking kernel).  parent / this tree alternate within "
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
