#!/usr/bin/env python3
"""context_bench.py -- what --context N (sid_opts.context) costs and saves,
against another build of the project (its parent commit).

Over the C2 text (seed 2, -m local) and the C3 text (seed 3, -R -m
likelihood_ratio), 50M synthetic 30x sites each, the engine runs

  none     no selection
  het      --only het
  hetctx   --only het --context 2          (this tree only)

  device   text and records in HBM (device_sink 1): the stage times of
           sid_engine_profile_read (HIP event pairs around every stage), per step
  pcie     pinned host text in, records into the pinned host arena
           (device_sink 2 + host_hold_bytes): the step's wall time

The marking stage runs inside a stage the engine already brackets -- the tile
parse's (`parse`) for -m local, the length stage (`fmt_len`) for the Lynch
pass 2 -- and a context runs the unselected parse, so its time is that stage's
with the context minus the same stage's of the unselected run, same build,
same process (context_ms); the edge kernel's time is in the writer's stage.

Every (tree, config) pair is a process of its own (a fresh HIP runtime, the
tree's own sid_amd and libsid.so).  The pairs alternate parent / this tree for
--rounds rounds in one session; the spread of a figure is its min .. max over
the rounds.  Each timed window is warmed up by --warmup steps and holds --steps.

Once per configuration (this tree, first round) the context run's records are
compared, chunk by chunk, with the unselected run's records filtered by the
model: the label from each record's third field, the dilation over the record
indices of the whole run, cut at the chunks' ends.

    python tools/gpu/context_bench.py --parent DIR [--out profiles/context_bench.json]

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
N = 2
SELS = {"none": {}, "het": {"select": "het"}, "hetctx": {"select": "het", "context": N}}
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
    p.add_argument("--no-check", action="store_true", help="skip the comparison of the records")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_bench.json"))
    p.add_argument("--step-timeout", type=int, default=600, help="seconds a (tree, config) process may take")
    # one (tree, config) process
    p.add_argument("--worker", default=None, metavar="TREE")
    p.add_argument("--config", default="C2")
    p.add_argument("--sels", default="none")
    p.add_argument("--check", action="store_true")
    return p.parse_args(argv)


# ------------------------------------------------------------------ worker --
def line_table(raw, np):
    """(bytes as an array, line starts, line ends past the newline, het flags) of a chunk's records ("chr1,pos,label,...")."""
    a = np.frombuffer(raw, np.uint8)
    nl = np.flatnonzero(a == 10)
    ls = np.concatenate(([0], nl[:-1] + 1)) if nl.size else np.zeros(0, np.int64)
    commas = np.flatnonzero(a == 44)
    c2 = commas[np.searchsorted(commas, ls) + 1] if nl.size else ls   # the second comma: the label follows
    het = a[c2 + 2] == ord("e") if nl.size else np.zeros(0, bool)
    return a, ls, nl + 1, het


def model_digests(chunks, n, np):
    """Per chunk (bytes, digest) of the records within n records of a het one, over the whole run's record order."""
    tabs = [line_table(raw, np) for raw in chunks]
    het = np.concatenate([t[3] for t in tabs]) if tabs else np.zeros(0, bool)
    idx = np.flatnonzero(het)
    keep = np.zeros(het.size, bool)
    if idx.size:
        r = np.arange(het.size)
        k = np.searchsorted(idx, r)
        before = r - idx[np.maximum(k - 1, 0)]
        after = idx[np.minimum(k, idx.size - 1)] - r
        keep = ((k > 0) & (before <= n)) | ((k < idx.size) & (after <= n))
    out, at = [], 0
    for a, ls, le, h in tabs:
        kp = keep[at:at + h.size]
        at += h.size
        sel = a[np.repeat(kp, le - ls)] if h.size else a[:0]
        out.append((int(sel.size), hashlib.blake2b(sel.tobytes()).hexdigest()))
    return out, int(het.sum()), int(keep.sum())


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

    digests, model = {}, None
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
        eng.close()
        r["device_stages_ms"] = {k[:-3]: v / a.steps for k, v in prof.items() if k.endswith("_ms")}
        r["device_bytes_out"] = st2.bytes_out
        r["chunks_tiled"] = st.chunks_tiled
        eng = sid_amd.Engine(method=cfg["method"], estimate_prior=cfg["R"], devices=1, device_sink=2,
                             host_hold_bytes=int(n * 48) + (64 << 20), **kw)
        eng.source_host_ptr(host.data_ptr(), ln, keep=host)
        for _ in range(a.warmup):
            step(eng)
        r["pcie_ms_per_step"], st, st2 = timed(eng, a.steps)
        r["pcie_bytes_out"] = st2.bytes_out
        r["pcie_chunks"] = st.chunks
        if a.check and name in ("none", "hetctx"):
            raws = []
            for j in range(st.chunks):
                p, m = eng.records(j)
                raws.append(C.string_at(p, m) if m else b"")
            if name == "none":
                model = model_digests(raws, N, np)
            else:
                digests[name] = [(len(x), hashlib.blake2b(x).hexdigest()) for x in raws]
            del raws
        eng.close()
        out["sels"][name] = r
    if a.check and model and "hetctx" in digests:
        want, nhet, nkeep = model
        got = digests["hetctx"]
        chk = {"equal": want == got, "chunks": len(got), "bytes": sum(x[0] for x in got), "het_records": nhet,
               "kept_records": nkeep, "records_all_bytes": out["sels"]["none"]["pcie_bytes_out"],
               "bytes_out_stat": out["sels"]["hetctx"]["pcie_bytes_out"],
               "device_sink_bytes_out_stat": out["sels"]["hetctx"]["device_bytes_out"]}
        if want != got:
            chk["first_bad_chunk"] = next((j for j, (w, g) in enumerate(zip(want, got)) if w != g), min(len(want), len(got)))
        out["records_check"] = chk
    print("CONTEXT_BENCH " + json.dumps(out), flush=True)
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
        for s in ("none", "het"):
            p, t = c["parent_" + s], c["this_" + s]
            o[f"unchanged_without_the_option_{s}"] = {
                "met": all(rng(t, k)[0] <= rng(p, k)[1] and rng(p, k)[0] <= rng(t, k)[1] for k in keys),
                "this": {k: rng(t, k) for k in keys}, "parent": {k: rng(p, k) for k in keys}}
        x, h, u, pu = c["this_hetctx"], c["this_het"], c["this_none"], c["parent_none"]
        o["context_cost"] = {
            "context_ms": rng(x, "context_ms"),
            "writer_ms": {"hetctx": rng(x, "fmt_write_ms"), "het": rng(h, "fmt_write_ms"), "none": rng(u, "fmt_write_ms")},
            "device_ms_per_step": {"hetctx": rng(x, "device_ms_per_step"), "het": rng(h, "device_ms_per_step"),
                                   "none": rng(u, "device_ms_per_step"), "parent_none": rng(pu, "device_ms_per_step")},
            "pcie_ms_per_step": {"hetctx": rng(x, "pcie_ms_per_step"), "het": rng(h, "pcie_ms_per_step"),
                                 "none": rng(u, "pcie_ms_per_step"), "parent_none": rng(pu, "pcie_ms_per_step")},
            "device_path_slower_than_parent_unselected": rng(x, "device_ms_per_step")[0] > rng(pu, "device_ms_per_step")[1]}
        if config == "C3":
            width = (pu["pcie_ms_per_step"]["max"] - pu["pcie_ms_per_step"]["min"]) + \
                    (x["pcie_ms_per_step"]["max"] - x["pcie_ms_per_step"]["min"])
            o["pcie_step_below_parent_unselected_by_more_than_both_ranges"] = {
                "met": x["pcie_ms_per_step"]["max"] < pu["pcie_ms_per_step"]["min"] - width,
                "hetctx": rng(x, "pcie_ms_per_step"), "parent_none": rng(pu, "pcie_ms_per_step"),
                "combined_width": round(width, 3)}
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
                       "none,het,hetctx" if name == "this" or a.parent_all else "none,het"] + (["--check"] if check else [])
                env = dict(os.environ)
                env.pop("SID_LIB_PATH", None)   # each tree loads its own build/libsid.so
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, env=env)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("CONTEXT_BENCH ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit(f"context_bench: {name} {config} failed (exit {p.returncode})")
                r = json.loads(line[0][len("CONTEXT_BENCH "):])
                r["build"], r["round"] = name, rnd
                stage = "parse" if config == "C2" else "fmt_len"   # the stage that holds the marking kernels
                if "hetctx" in r["sels"]:
                    r["sels"]["hetctx"]["context_ms"] = (r["sels"]["hetctx"]["device_stages_ms"][stage] -
                                                         r["sels"]["none"]["device_stages_ms"][stage])
                runs.append(r)
                print(f"round {rnd} {config} {name}: " + ", ".join(
                    f"{s}: device {v['device_ms_per_step']:.2f} ms (parse {v['device_stages_ms']['parse']:.3f}, "
                    f"len {v['device_stages_ms']['fmt_len']:.3f}, write {v['device_stages_ms']['fmt_write']:.3f}), "
                    f"pcie {v['pcie_ms_per_step']:.1f} ms, {v['pcie_bytes_out']} B"
                    for s, v in r["sels"].items()) + (f"; check {r['records_check']['equal']}" if "records_check" in r else ""),
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
                if s == "hetctx":
                    e["context_ms"] = spread(series(build, config, s, lambda v: v["context_ms"]))
                c[f"{build}_{s}"] = e
        checks = [r["records_check"] for r in runs if r["config"] == config and "records_check" in r]
        if checks:
            c["records_check"] = checks[0]
        summary[config] = c
    doc = {"tool": "tools/gpu/context_bench.py", "sites": a.sites, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "depth": DEPTH, "context": N,
           "note": "ms per step; device: text and records in HBM (device_sink 1), stages from HIP event pairs in a "
                   "profiled run of the same steps; pcie: pinned host text in, records into the pinned host arena "
                   "(device_sink 2), wall time.  context_ms: the stage that holds the marking kernels (C2: parse, "
                   "the tile parse; C3: fmt_len) with --only het --context 2 minus the unselected run's, same "
                   "process.  parent / this tree alternate within every round; the spread of a figure is its "
                   "min .. max over the rounds",
           "comparisons": comparisons(summary), "summary": summary, "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
