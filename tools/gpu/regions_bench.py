#!/usr/bin/env python3
"""regions_bench.py -- what the selection by region (--regions,
sid_opts.regions) costs and saves, against another build of the project (its
parent commit).

Over the C2 text (seed 2, -m local) and the C3 text (seed 3, -R -m
likelihood_ratio), 50M synthetic 30x sites each (one chrom, positions 1..n),
the engine runs without a set and with two sets made from the text's own
coordinates with a fixed seed:

  sparse   an interval of 200-400 positions in every 12,000: 2-3 % of the sites
  whole    the chrom alone: every site

  device   text and records in HBM (device_sink 1): the stage times of
           sid_engine_profile_read (HIP event pairs around every stage), per step
  pcie     pinned host text in, records into the pinned host arena
           (device_sink 2 + host_hold_bytes): the step's wall time

The region kernel runs inside a stage the engine already brackets -- the tile
parse's (`parse`) for -m local, the length stage (`fmt_len`) for the Lynch
pass 2 -- so its time is that stage's with a set minus the same stage's
without one, same build, same round (region_ms).

Every (tree, config) pair is a process of its own (a fresh HIP runtime, the
tree's own sid_amd and libsid.so); the parent tree, which has no region sets,
runs without one only.  The pairs alternate parent / this tree for --rounds
rounds in one session, so the spread between rounds of the same code stands
beside every difference between the two.  Each timed window is warmed up by
--warmup steps of the same shape and holds --steps steps.

Once per configuration (this tree, first round) the records of the runs with
a set are compared with the unfiltered run's records filtered by position,
chunk by chunk (the chunks are cut by input bytes: the same in every run).

    python tools/gpu/regions_bench.py --parent DIR [--out profiles/regions_bench.json]

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
PERIOD, LEN_LO, LEN_HI, SET_SEED = 12_000, 200, 400, 1234


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
    p.add_argument("--no-check", action="store_true", help="skip the comparison of the filtered records")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions_bench.json"))
    p.add_argument("--step-timeout", type=int, default=600, help="seconds a (tree, config) process may take")
    # one (tree, config) process
    p.add_argument("--worker", default=None, metavar="TREE")
    p.add_argument("--config", default="C2")
    p.add_argument("--sets", default="none")
    p.add_argument("--check", action="store_true")
    return p.parse_args(argv)


# ------------------------------------------------------------------ worker --
def sparse_intervals(n, np):
    """(starts, ends), BED convention, over positions 1..n: one interval per PERIOD positions."""
    rng = np.random.default_rng(SET_SEED)
    k = np.arange(0, n, PERIOD, dtype=np.int64)
    s = k + rng.integers(0, PERIOD - LEN_HI, k.size)
    e = np.minimum(s + rng.integers(LEN_LO, LEN_HI + 1, k.size), n)
    return s, e


def filtered_digest(raw, starts, ends, np):
    """(bytes, digest) of the records of `raw` (all of chrom chr1) whose position lies in an interval."""
    a = np.frombuffer(raw, np.uint8)
    if a.size == 0:
        return 0, hashlib.blake2b(b"").hexdigest()
    nl = np.flatnonzero(a == 10)
    ls = np.concatenate(([0], nl[:-1] + 1))
    # "chr1,<pos>,": the digits from byte 5 of the line to the next comma
    commas = np.flatnonzero(a == 44)
    c2 = commas[np.searchsorted(commas, ls + 5)]
    nd = c2 - (ls + 5)
    pos = np.zeros(ls.size, np.int64)
    for d in range(int(nd.max())):
        m = nd > d
        pos[m] = pos[m] * 10 + (a[ls[m] + 5 + d].astype(np.int64) - 48)
    j = np.searchsorted(starts, pos, side="left") - 1        # the last start < pos
    keep = (j >= 0) & (pos <= ends[np.maximum(j, 0)])
    sel = a[np.repeat(keep, nl + 1 - ls)]
    return int(sel.size), hashlib.blake2b(sel.tobytes()).hexdigest()


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
    sp_s, sp_e = sparse_intervals(n, np)

    def make_set(name):
        if name == "none":
            return None
        if name == "whole":
            return sid_amd.Regions(b"chr1\n")
        return sid_amd.Regions(b"".join(b"chr1\t%d\t%d\n" % (s, e) for s, e in zip(sp_s.tolist(), sp_e.tolist())))

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

    digests = {}
    for name in a.sets.split(","):
        rg = make_set(name)
        kw = {} if rg is None else {"regions": rg}
        r = {"intervals": 0 if rg is None else len(rg)}
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
        if a.check:
            import ctypes as C
            d = []
            for j in range(st.chunks):
                p, m = eng.records(j)
                raw = C.string_at(p, m) if m else b""
                if name == "none":
                    d.append({"sparse": filtered_digest(raw, sp_s, sp_e, np), "whole": (m, hashlib.blake2b(raw).hexdigest())})
                else:
                    d.append((m, hashlib.blake2b(raw).hexdigest()))
            digests[name] = d
        eng.close()
        if rg is not None:
            rg.close()
        out["sets"][name] = r
    if a.check:
        chk = {}
        for name in ("sparse", "whole"):
            if name in digests and "none" in digests:
                want = [tuple(x[name]) for x in digests["none"]]
                got = [tuple(x) for x in digests[name]]
                chk[name] = {"equal": want == got, "chunks": len(got), "bytes": sum(x[0] for x in got),
                             "records_all_bytes": out["sets"]["none"]["pcie_bytes_out"]}
                if want != got:
                    chk[name]["first_bad_chunk"] = next(j for j, (w, g) in enumerate(zip(want, got)) if w != g)
        out["filtered_bytes_check"] = chk
    print("REGIONS_BENCH " + json.dumps(out), flush=True)
    return 0


# ------------------------------------------------------------------ driver --
def spread(xs):
    xs = list(xs)
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def comparisons(summary):
    """The four comparisons against the parent build, each stated with its ranges (min .. max over the rounds)."""
    def rng(e, k):
        return [round(e[k]["min"], 3), round(e[k]["max"], 3)]

    def overlap_or_lower(x, y):   # x not above y: the ranges overlap, or x lies below
        return x[0] <= y[1]

    out = {}
    for config, c in summary.items():
        if "parent_none" not in c:
            continue
        p, n, s, w = c["parent_none"], c["this_none"], c["this_sparse"], c["this_whole"]
        keys = ["device_ms_per_step", "pcie_ms_per_step", "parse_ms", "fmt_len_ms", "fmt_write_ms"]
        o = {"1_no_set_within_parent_spread": {
                 "met": all(rng(n, k)[0] <= rng(p, k)[1] and rng(p, k)[0] <= rng(n, k)[1] for k in keys),
                 "this": {k: rng(n, k) for k in keys}, "parent": {k: rng(p, k) for k in keys}},
             "2_sparse_device_path_not_slower": {
                 "met": overlap_or_lower(rng(s, "device_ms_per_step"), rng(p, "device_ms_per_step")),
                 "this_sparse": rng(s, "device_ms_per_step"), "parent": rng(p, "device_ms_per_step"),
                 "region_ms": rng(s, "region_ms")},
             "4_whole_set_cost_over_no_set": {
                 "device_ms": [round(w["device_ms_per_step"]["min"] - n["device_ms_per_step"]["max"], 3),
                               round(w["device_ms_per_step"]["max"] - n["device_ms_per_step"]["min"], 3)],
                 "this_whole": rng(w, "device_ms_per_step"), "this_none": rng(n, "device_ms_per_step"),
                 "region_ms": rng(w, "region_ms"), "pcie_this_whole": rng(w, "pcie_ms_per_step"),
                 "pcie_this_none": rng(n, "pcie_ms_per_step")}}
        if config == "C3":
            sp = p["pcie_ms_per_step"]["max"] - p["pcie_ms_per_step"]["min"]
            o["3_sparse_pcie_step_below_parent_by_more_than_the_spread"] = {
                "met": s["pcie_ms_per_step"]["max"] < p["pcie_ms_per_step"]["min"] - sp,
                "this_sparse": rng(s, "pcie_ms_per_step"), "parent": rng(p, "pcie_ms_per_step"), "spread": round(sp, 3)}
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
                       "none,sparse,whole" if name == "this" or a.parent_all else "none"] + (["--check"] if check else [])
                env = dict(os.environ)
                env.pop("SID_LIB_PATH", None)   # each tree loads its own build/libsid.so
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, env=env)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("REGIONS_BENCH ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit(f"regions_bench: {name} {config} failed (exit {p.returncode})")
                r = json.loads(line[0][len("REGIONS_BENCH "):])
                r["build"], r["round"] = name, rnd
                stage = "parse" if config == "C2" else "fmt_len"   # the stage that holds the region kernel
                for s, v in r["sets"].items():
                    if s != "none":
                        v["region_ms"] = v["device_stages_ms"][stage] - r["sets"]["none"]["device_stages_ms"][stage]
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
            for s in ("none", "sparse", "whole"):
                if not series(build, config, s, lambda v: 0):
                    continue
                e = {"device_ms_per_step": spread(series(build, config, s, lambda v: v["device_ms_per_step"])),
                     "pcie_ms_per_step": spread(series(build, config, s, lambda v: v["pcie_ms_per_step"])),
                     "bytes_out": series(build, config, s, lambda v: v["pcie_bytes_out"])[0],
                     "intervals": series(build, config, s, lambda v: v["intervals"])[0]}
                for stg in ("index", "parse", "call", "hist", "fmt_len", "fmt_write"):
                    e[stg + "_ms"] = spread(series(build, config, s, lambda v: v["device_stages_ms"][stg]))
                if s != "none":
                    e["region_ms"] = spread(series(build, config, s, lambda v: v["region_ms"]))
                c[f"{build}_{s}"] = e
        checks = [r["filtered_bytes_check"] for r in runs if r["config"] == config and "filtered_bytes_check" in r]
        if checks:
            c["filtered_bytes_check"] = checks[0]
        summary[config] = c
    doc = {"tool": "tools/gpu/regions_bench.py", "sites": a.sites, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "depth": DEPTH,
           "sets": {"sparse": f"an interval of {LEN_LO}-{LEN_HI} positions in every {PERIOD} (seed {SET_SEED})",
                    "whole": "chr1"},
           "note": "ms per step; device: text and records in HBM (device_sink 1), stages from HIP event pairs in a "
                   "profiled run of the same steps; pcie: pinned host text in, records into the pinned host arena "
                   "(device_sink 2), wall time.  region_ms: the stage that holds the region kernel (C2: parse, the "
                   "tile parse; C3: fmt_len) with the set minus without, same process.  parent / this tree "
                   "alternate within every round; the spread of a figure is its min .. max over the rounds",
           "comparisons": comparisons(summary), "summary": summary, "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
