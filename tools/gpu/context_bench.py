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
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optbench as ob
from optbench import rng

N = 2
SELS = {"none": {}, "het": {"select": "het"}, "hetctx": {"select": "het", "context": N}}


def parse_args(argv=None):
    p = ob.arg_parser(__file__, __doc__, sets=("--sels", "none"))
    ob.add_parent_all(p)
    ob.add_check_args(p, "comparison of the records")
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
    import numpy as np
    cfg, n, text, ln, host, out = ob.worker_start(a, "sels")
    digests, model = {}, None
    for name in a.sels.split(","):
        kw = SELS[name]
        r = ob.device_pass(a, cfg, text, ln, kw, omit=("device_chunks_per_step", "tile_overflows"))
        eng, st = ob.pcie_pass(a, cfg, host, ln, n, kw, r)
        if a.check and name in ("none", "hetctx"):
            raws = list(ob.record_chunks(eng, st.chunks))
            if name == "none":
                model = model_digests(raws, N, np)
            else:
                digests[name] = [ob.chunk_digest(x) for x in raws]
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
            chk["first_bad_chunk"] = ob.first_bad(want, got)
        out["records_check"] = chk
    return ob.emit(__file__, out)


# ------------------------------------------------------------------ driver --
def comparisons(summary):
    out = {}
    for config, c in summary.items():
        if "parent_none" not in c:
            continue
        o = {}
        for s in ("none", "het"):
            o[f"unchanged_without_the_option_{s}"] = ob.within_parent_spread(c["this_" + s], c["parent_" + s])
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


def derive(r, config):
    stage = "parse" if config == "C2" else "fmt_len"   # the stage that holds the marking kernels
    if "hetctx" in r["sels"]:
        r["sels"]["hetctx"]["context_ms"] = (r["sels"]["hetctx"]["device_stages_ms"][stage] -
                                             r["sels"]["none"]["device_stages_ms"][stage])


def entry(ser, s):
    e = ob.summary_entry(ser)
    if s == "hetctx":
        e["context_ms"] = ob.spread(ser(lambda v: v["context_ms"]))
    return e


def main():
    a = parse_args()
    if a.worker:
        return worker(a)
    trees = ob.trees(a)
    runs, _ = ob.run_rounds(
        a, __file__, [(name, tree, ["--sels", "none,het,hetctx" if name == "this" or a.parent_all else "none,het"],
                       name == "this", None) for name, tree in trees],
        derive, progress=lambda r: ", ".join(f"{s}: " + ob.set_line(v) for s, v in r["sels"].items()) +
        ob.check_note(r, "records_check"))
    summary = ob.summarise(a, runs, "sels", [b for b, _ in trees], SELS, entry, check_key="records_check")
    return ob.write_doc(a, {
        **ob.doc_head(__file__, a), "depth": ob.DEPTH, "context": N,
        "note": ob.NOTE + "context_ms: the stage that holds the marking kernels (C2: parse, the tile parse; C3: "
                "fmt_len) with --only het --context 2 minus the unselected run's, same process.  " + ob.NOTE_ROUNDS,
        "comparisons": comparisons(summary), "summary": summary, "runs": runs})


if __name__ == "__main__":
    sys.exit(main())
