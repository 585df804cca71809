"""optbench.py -- what the per-option benchmark scripts of this directory
(X_bench.py) share: plain functions, called by each script for what it needs.

A script measures what one option costs and saves against another build of the
project (its parent commit).  Its driver starts every measurement as a process
of its own (`python X_bench.py --worker TREE ...`: a fresh HIP runtime, the
tree's own sid_amd and libsid.so) under its own time limit, parent and this
tree alternating within every round; a process that fails, prints no tagged
line or runs past the limit ends the script before anything else starts.  The
worker makes the synthetic text on the device and runs the engine over it once
per option set, two ways:

  device   text and records in HBM (device_sink 1): the stage times of
           sid_engine_profile_read (HIP event pairs around every stage), per step
  pcie     pinned host text in, records into the pinned host arena
           (device_sink 2 + host_hold_bytes): the step's wall time

A script keeps its option sets, its check of the records or rows, its derived
figures and its comparisons.  torch and sid_amd are imported by the worker's
functions only: the drivers and --help need neither."""
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

DEPTH = 30.0
CONFIGS = {"C2": dict(method="local", R=False, seed=2, depth=DEPTH),
           "C3": dict(method="likelihood_ratio", R=True, seed=3, depth=DEPTH),
           "D200": dict(method="local", R=False, seed=5, depth=200.0)}   # depth_hist_bench.py's, on request
STAGES = ("index", "parse", "call", "hist", "fmt_len", "fmt_write")
KEYS = ["device_ms_per_step", "pcie_ms_per_step"] + [s + "_ms" for s in STAGES]
NOTE = ("ms per step; device: text and records in HBM (device_sink 1), stages from HIP event pairs in a "
        "profiled run of the same steps; pcie: pinned host text in, records into the pinned host arena "
        "(device_sink 2), wall time.  ")
NOTE_ROUNDS = ("parent / this tree alternate within every round; the spread of a figure is its min .. max over "
               "the rounds")


def tool(script):
    """select_bench of .../select_bench.py: the name in the messages; upper case and a space, the tag of its line."""
    return os.path.splitext(os.path.basename(script))[0]


def arg_parser(script, doc, sets=None, sites=50_000_000, steps=8, warmup=2, configs="C2,C3", step_timeout=600,
               process="(tree, config)"):
    """The arguments every script has; `sets` names the worker's list of option sets (--sets none,...)."""
    p = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--parent", default=None, help="a built checkout of the parent commit (none: this tree only)")
    p.add_argument("--sites", type=int, default=sites)
    p.add_argument("--steps", type=int, default=steps)
    p.add_argument("--warmup", type=int, default=warmup)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", tool(script) + ".json"))
    p.add_argument("--step-timeout", type=int, default=step_timeout, help=f"seconds a {process} process may take")
    p.add_argument("--worker", default=None, metavar="TREE", help=f"one {process} process")
    if sets:
        p.add_argument("--configs", default=configs)
        p.add_argument("--config", default="C2")
        p.add_argument(sets[0], default=sets[1])
    return p


def add_check_args(p, what):
    p.add_argument("--no-check", action="store_true", help="skip the " + what)
    p.add_argument("--check", action="store_true")


def add_parent_all(p):
    p.add_argument("--parent-all", action="store_true",
                   help="the parent runs every selection this tree runs (a parent that has them all)")


# ------------------------------------------------------------------ worker --
def load_tree(tree):
    """The tree's own sid_amd (and with it its build/libsid.so)."""
    sys.path.insert(0, tree)
    import sid_amd
    assert os.path.dirname(os.path.abspath(sid_amd.__file__)).startswith(os.path.abspath(tree))
    return sid_amd


def make_text(seed, depth, n, ctx=None):
    """(the device tensor, the text's length, its pinned host copy): n synthetic sites made on the device, with
    512 zero bytes behind them.  Without a `ctx` of the caller's, one is opened for the call."""
    import torch
    import sid_amd
    dev = torch.device("cuda", 0)
    cap = int(n * (2.72 * depth + 2) * 1.03) + (64 << 20)
    text = torch.empty(cap, dtype=torch.uint8, device=dev)
    own = ctx is None
    if own:
        ctx = sid_amd.Context(0)
    ln = ctx.synth_text_device(seed, depth, 0, n, text.data_ptr(), cap - 512)
    text[ln:ln + 512].zero_()
    torch.cuda.synchronize(dev)
    if own:
        ctx.close()
    return text, ln, text[:ln].cpu().pin_memory()


def config_sites(config, sites):
    """The same number of read bases in every config."""
    return int(sites * DEPTH / CONFIGS[config]["depth"])


def worker_start(a, key, **more):
    """What every (tree, config) worker begins with: (cfg, sites, text, length, host copy, the result so far)."""
    sid_amd = load_tree(a.worker)
    cfg = CONFIGS[a.config]
    n = config_sites(a.config, a.sites)
    text, ln, host = make_text(cfg["seed"], cfg["depth"], n)
    out = {"config": a.config, "sites": n, "text_bytes": ln, "steps": a.steps, "warmup": a.warmup, **more,
           "version": sid_amd.lib().sid_version().decode(), key: {}}
    return cfg, n, text, ln, host, out


def step(eng):
    st = eng.ingest()
    eng.estimate()
    _, st2 = eng.emit()
    return st, st2


def timed(eng, steps):
    """(ms per step over `steps` steps, the last step's two stats)."""
    import torch
    torch.cuda.synchronize(0)
    t0 = time.perf_counter()
    for _ in range(steps):
        st, st2 = step(eng)
    torch.cuda.synchronize(0)
    return (time.perf_counter() - t0) / steps * 1e3, st, st2


def device_pass(a, cfg, text, ln, kw, before_close=None, omit=()):
    """Text and records in HBM: the kernels, per stage.  Warm-up, the timed steps, then a profiled step discarded
    and the profiled steps read.  `before_close(eng, r)` reads what a script wants of the engine."""
    import sid_amd
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
    if before_close:
        before_close(eng, r)
    eng.close()
    r["device_stages_ms"] = {k[:-3]: v / a.steps for k, v in prof.items() if k.endswith("_ms")}
    r["device_chunks_per_step"] = prof["chunks"] / a.steps
    r["device_bytes_out"] = st2.bytes_out
    r["chunks_tiled"] = st.chunks_tiled
    r["tile_overflows"] = st.tile_overflows
    for k in omit:   # (a script whose documents never had the figure)
        del r[k]
    return r


def pcie_pass(a, cfg, host, ln, n, kw, r, site_bytes=48):
    """The PCIe path: host text in, records into the pinned host arena of `site_bytes` a site (the whole run's
    records fit).  Adds its figures to `r`; (the engine, still open with the last step's records, its stats)."""
    import sid_amd
    eng = sid_amd.Engine(method=cfg["method"], estimate_prior=cfg["R"], devices=1, device_sink=2,
                         host_hold_bytes=int(n * site_bytes) + (64 << 20), **kw)
    eng.source_host_ptr(host.data_ptr(), ln, keep=host)
    for _ in range(a.warmup):
        step(eng)
    r["pcie_ms_per_step"], st, st2 = timed(eng, a.steps)
    r["pcie_bytes_out"] = st2.bytes_out
    r["pcie_chunks"] = st.chunks
    return eng, st


def record_chunks(eng, chunks):
    """The bytes of every chunk's records, in order."""
    import ctypes as C
    for j in range(chunks):
        p, m = eng.records(j)
        yield C.string_at(p, m) if m else b""


def records_digest(eng, chunks):
    """(digest, newlines) of a run's records."""
    h, nl = hashlib.blake2b(), 0
    for raw in record_chunks(eng, chunks):
        h.update(raw)
        nl += raw.count(b"\n")
    return h.hexdigest(), nl


def chunk_digest(raw):
    return len(raw), hashlib.blake2b(raw).hexdigest()


def first_bad(want, got):
    return next((j for j, (w, g) in enumerate(zip(want, got)) if w != g), min(len(want), len(got)))


def emit(script, out):
    print(tool(script).upper() + " " + json.dumps(out), flush=True)
    return 0


# ------------------------------------------------------------------ driver --
def run_worker(script, args, timeout, label, env=None):
    """One worker process of `script` under its time limit; its tagged line's result.  SID_LIB_PATH is dropped (each
    tree loads its own build/libsid.so); `env` sets variables, or drops the ones it gives as None.  A failure ends
    the script, and so does the limit (subprocess.TimeoutExpired): nothing more starts on the GPU."""
    e = dict(os.environ)
    for k, v in {"SID_LIB_PATH": None, **(env or {})}.items():
        e.pop(k, None)
        if v is not None:
            e[k] = v
    p = subprocess.run([sys.executable, os.path.abspath(script)] + args, capture_output=True, text=True,
                       timeout=timeout, env=e)
    tag = tool(script).upper() + " "
    line = [ln for ln in p.stdout.splitlines() if ln.startswith(tag)]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{tool(script)}: {label} failed (exit {p.returncode})")
    return json.loads(line[0][len(tag):])


def trees(a):
    return ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("this", ROOT)]


def run_rounds(a, script, procs, derive, progress, budget_s=0):
    """Rounds x configs x processes, each process started by run_worker; (the runs, the rounds run).  `procs`:
    (name, tree, the worker's arguments after --warmup, checked in the first round, env) per process of a round.
    `derive(r, config)` adds the script's derived figures to a result, `progress(r)` is the text of its line.  A
    round that would start past `budget_s` seconds is not started."""
    runs, rounds_run, round_s, t_start = [], 0, 0.0, time.time()
    for rnd in range(a.rounds):
        if budget_s and rnd and time.time() - t_start + round_s > budget_s:
            print(f"round {rnd} not started: past the budget of {budget_s} s", flush=True)
            break
        t_round = time.time()
        for config in a.configs.split(","):
            for name, tree, args, checked, env in procs:
                check = checked and rnd == 0 and not a.no_check
                r = run_worker(script, ["--worker", tree, "--config", config, "--sites", str(a.sites), "--steps",
                                        str(a.steps), "--warmup", str(a.warmup)] + args + (["--check"] if check else []),
                               a.step_timeout, f"{name} {config}", env)
                r["build"], r["round"] = name, rnd
                derive(r, config)
                runs.append(r)
                print(f"round {rnd} {config} {name}: " + progress(r), flush=True)
        rounds_run += 1
        round_s = time.time() - t_round
    return runs, rounds_run


def set_line(v, stages=("parse", "fmt_len", "fmt_write"), nbytes=True):
    """A set's part of the progress line."""
    short = {"parse": "parse", "fmt_len": "len", "fmt_write": "write"}
    return (f"device {v['device_ms_per_step']:.2f} ms (" +
            ", ".join(f"{short[s]} {v['device_stages_ms'][s]:.3f}" for s in stages) +
            f"), pcie {v['pcie_ms_per_step']:.1f} ms" + (f", {v['pcie_bytes_out']} B" if nbytes else ""))


def check_note(r, key):
    return f"; check {r[key]['equal']}" if key in r else ""


def spread(xs, runs=True):
    xs = list(xs)
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), **({"runs": xs} if runs else {})}


def rng(e, k):
    return [round(e[k]["min"], 3), round(e[k]["max"], 3)]


def series(runs, key, build, config, s, get):
    return [get(r[key][s]) for r in runs if r["build"] == build and r["config"] == config and s in r[key]]


def summary_entry(ser, lead=(), mid=None):
    """A set's entry of the summary from `ser(get)`, its series over the rounds: the two wall times (and the `lead`
    figures), bytes_out (and the `mid` values), the six stage spreads.  The script adds its own after those."""
    e = {k: spread(ser(lambda v: v[k])) for k in ("device_ms_per_step", "pcie_ms_per_step") + tuple(lead)}
    e["bytes_out"] = ser(lambda v: v["pcie_bytes_out"])[0]
    e.update(mid or {})
    for stg in STAGES:
        e[stg + "_ms"] = spread(ser(lambda v: v["device_stages_ms"][stg]))
    return e


def summarise(a, runs, key, builds, sets, entry=lambda ser, s: summary_entry(ser), check_key=None):
    """{config: {build_set: entry(ser, set)}} over the sets that ran, and the first `check_key` of a config's runs."""
    summary = {}
    for config in a.configs.split(","):
        c = {}
        for build in builds:
            for s in sets:
                def ser(get):
                    return series(runs, key, build, config, s, get)
                if ser(lambda v: 0):
                    c[f"{build}_{s}"] = entry(ser, s)
        checks = [r[check_key] for r in runs if r["config"] == config and check_key in r]
        if checks:
            c[check_key] = checks[0]
        summary[config] = c
    return summary


def within_parent_spread(t, p, keys=KEYS, per_key=False):
    """The comparison "without the option, within the parent's spread": every figure's range overlaps the parent's."""
    over = {k: rng(t, k)[0] <= rng(p, k)[1] and rng(p, k)[0] <= rng(t, k)[1] for k in keys}
    return {"met": all(over.values()), **({"overlap": over} if per_key else {}),
            "this": {k: rng(t, k) for k in keys}, "parent": {k: rng(p, k) for k in keys}}


def doc_head(script, a):
    return {"tool": "tools/gpu/" + os.path.basename(script), "sites": a.sites, "steps": a.steps, "warmup": a.warmup,
            "rounds": a.rounds}


def write_doc(a, doc):
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0
