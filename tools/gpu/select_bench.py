#!/usr/bin/env python3
"""select_bench.py -- what the selection by label (--only, sid_opts.select)
costs and saves, against another build of the project (its parent commit).

Over the C2 text (seed 2, -m local) and the C3 text (seed 3, -R -m
likelihood_ratio), 50M synthetic 30x sites each, the engine runs with select
all, het and hom:

  device   text and records in HBM (device_sink 1): the stage times of
           sid_engine_profile_read (HIP event pairs around every stage), per step
  pcie     pinned host text in, records into the pinned host arena
           (device_sink 2 + host_hold_bytes): the step's wall time

Every (tree, config) pair is a process of its own (a fresh HIP runtime, the
tree's own sid_amd and libsid.so); the parent tree, which has no selection,
runs select all only.  The pairs alternate parent / this tree for --rounds
rounds in one session, so the spread between rounds of the same code stands
beside every difference between the two.  Each timed window is warmed up by
--warmup steps of the same shape and holds --steps steps.

Once per configuration (this tree, first round) the het and hom records are
compared with the `all` run's records filtered by the label field, chunk by
chunk (the chunks are cut by input bytes: the same in every run).

    python tools/gpu/select_bench.py --parent DIR [--out profiles/select_bench.json]

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


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--parent", default=None, help="a built checkout of the parent commit (none: this tree only)")
    p.add_argument("--sites", type=int, default=50_000_000)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--configs", default="C2,C3")
    p.add_argument("--no-check", action="store_true", help="skip the comparison of the filtered records")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_bench.json"))
    p.add_argument("--step-timeout", type=int, default=600, help="seconds a (tree, config) process may take")
    # one (tree, config) process
    p.add_argument("--worker", default=None, metavar="TREE")
    p.add_argument("--config", default="C2")
    p.add_argument("--selects", default="all")
    p.add_argument("--check", action="store_true")
    return p.parse_args(argv)


# ------------------------------------------------------------------ worker --
def select_mask_lines(a, np):
    """Per line of the CSV bytes `a` (a uint8 array): (line starts, line ends
    past the newline, the label's second letter) -- the label is the field
    after the fifth comma from the line's right."""
    nl = np.flatnonzero(a == 10)
    commas = np.flatnonzero(a == 44)
    upto = np.searchsorted(commas, nl)          # commas before each newline
    fifth = commas[upto - 5]                    # the fifth from the right
    starts = np.concatenate(([0], nl[:-1] + 1))
    return starts, nl + 1, a[fifth + 2]         # 'e' of het, 'o' of hom


def filtered_digest(raw, want, np):
    """(bytes, digest) of the records of `raw` whose label is `want`."""
    a = np.frombuffer(raw, np.uint8)
    if a.size == 0:
        return 0, hashlib.blake2b(b"").hexdigest()
    starts, ends, second = select_mask_lines(a, np)
    keep = second == (ord("e") if want == "het" else ord("o"))
    mask = np.repeat(keep, ends - starts)
    sel = a[mask]
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
           "version": sid_amd.lib().sid_version().decode(), "selects": {}}

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
    for sel in a.selects.split(","):
        kw = {} if sel == "all" else {"select": sel}
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
        if a.check:
            import ctypes as C
            d = []
            for j in range(st.chunks):
                p, m = eng.records(j)
                raw = C.string_at(p, m) if m else b""
                if sel == "all":
                    d.append({w: filtered_digest(raw, w, np) for w in ("het", "hom")})
                else:
                    d.append((m, hashlib.blake2b(raw).hexdigest()))
            digests[sel] = d
        eng.close()
        out["selects"][sel] = r
    if a.check:
        chk = {}
        for sel in ("het", "hom"):
            if sel in digests and "all" in digests:
                want = [tuple(x[sel]) for x in digests["all"]]
                got = [tuple(x) for x in digests[sel]]
                chk[sel] = {"equal": want == got, "chunks": len(got), "bytes": sum(x[0] for x in got),
                            "records_all_bytes": out["selects"]["all"]["pcie_bytes_out"]}
                if want != got:
                    bad = next(j for j, (w, g) in enumerate(zip(want, got)) if w != g)
                    chk[sel]["first_bad_chunk"] = bad
        out["filtered_bytes_check"] = chk
    print("SELECT_BENCH " + json.dumps(out), flush=True)
    return 0


# ------------------------------------------------------------------ driver --
def spread(xs):
    xs = list(xs)
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


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
                       str(a.sites), "--steps", str(a.steps), "--warmup", str(a.warmup), "--selects",
                       "all,het,hom" if name == "this" else "all"] + (["--check"] if check else [])
                env = dict(os.environ)
                env.pop("SID_LIB_PATH", None)   # each tree loads its own build/libsid.so
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, env=env)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("SELECT_BENCH ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit(f"select_bench: {name} {config} failed (exit {p.returncode})")
                r = json.loads(line[0][len("SELECT_BENCH "):])
                r["build"], r["round"] = name, rnd
                runs.append(r)
                print(f"round {rnd} {config} {name}: " + ", ".join(
                    f"{s}: device {v['device_ms_per_step']:.2f} ms (write {v['device_stages_ms']['fmt_write']:.3f}, "
                    f"len {v['device_stages_ms']['fmt_len']:.3f}), pcie {v['pcie_ms_per_step']:.1f} ms"
                    for s, v in r["selects"].items()), flush=True)

    def series(build, config, sel, get):
        return [get(r["selects"][sel]) for r in runs if r["build"] == build and r["config"] == config
                and sel in r["selects"]]

    summary = {}
    for config in a.configs.split(","):
        c = {}
        for build, _ in trees:
            for sel in ("all", "het", "hom"):
                if not series(build, config, sel, lambda v: 0):
                    continue
                e = {"device_ms_per_step": spread(series(build, config, sel, lambda v: v["device_ms_per_step"])),
                     "pcie_ms_per_step": spread(series(build, config, sel, lambda v: v["pcie_ms_per_step"])),
                     "bytes_out": series(build, config, sel, lambda v: v["pcie_bytes_out"])[0]}
                for stg in ("index", "parse", "call", "hist", "fmt_len", "fmt_write"):
                    e[stg + "_ms"] = spread(series(build, config, sel, lambda v: v["device_stages_ms"][stg]))
                c[f"{build}_{sel}"] = e
        checks = [r["filtered_bytes_check"] for r in runs if r["config"] == config and "filtered_bytes_check" in r]
        if checks:
            c["filtered_bytes_check"] = checks[0]
        summary[config] = c
    doc = {"tool": "tools/gpu/select_bench.py", "sites": a.sites, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "depth": DEPTH,
           "note": "ms per step; device: text and records in HBM (device_sink 1), stages from HIP event pairs in a "
                   "profiled run of the same steps; pcie: pinned host text in, records into the pinned host arena "
                   "(device_sink 2), wall time.  parent / this tree alternate within every round; the spread of a "
                   "figure is its min .. max over the rounds",
           "summary": summary, "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
