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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optbench as ob
from optbench import rng

HALF, TIGHT = (30, 0), (40, 0)
KW = {"none": {}, "variants": {"variants": 1},
      "half": dict(min_depth=HALF[0], max_depth=HALF[1]), "tight": dict(min_depth=TIGHT[0], max_depth=TIGHT[1]),
      "both": dict(variants=1, min_depth=HALF[0], max_depth=HALF[1])}
KW["both_split"] = KW["both"]
OPTS = ("half", "tight", "variants", "both", "both_split")


def parse_args(argv=None):
    p = ob.arg_parser(__file__, __doc__, sets=("--sets", "none"))
    p.add_argument("--split", action="store_true", help="SID_DEPTH_SPLIT=1: two kernels for variants + bounds")
    return p.parse_args(argv)


# ------------------------------------------------------------------ worker --
def worker(a):
    if a.split:
        os.environ["SID_DEPTH_SPLIT"] = "1"
    cfg, n, text, ln, host, out = ob.worker_start(a, "sets")
    for name in a.sets.split(","):
        r = ob.device_pass(a, cfg, text, ln, KW[name])
        eng, _ = ob.pcie_pass(a, cfg, host, ln, n, KW[name], r)
        eng.close()
        out["sets"][name] = r
    return ob.emit(__file__, out)


# ------------------------------------------------------------------ driver --
def comparisons(summary):
    """The comparisons the change is judged by, each stated with its ranges (min .. max over the rounds)."""
    out = {}
    for config, c in summary.items():
        o = {}
        n = c["this_none"]
        if "parent_none" in c:
            o["1_without_the_option_within_parent_spread"] = ob.within_parent_spread(n, c["parent_none"], per_key=True)
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


def derive(r, config):
    stage = "parse" if config == "C2" else "fmt_len"
    for s, v in r["sets"].items():   # (the marking stage: with the option minus without, same process)
        if s != "none":
            v["mark_ms"] = v["device_stages_ms"][stage] - r["sets"]["none"]["device_stages_ms"][stage]
    if r["build"] == "this_split":   # (its own unselected run was only the subtrahend)
        r["build"] = "this"
        del r["sets"]["none"]


def entry(ser, s):
    e = ob.summary_entry(ser)
    if s != "none":
        e["mark_ms"] = ob.spread(ser(lambda v: v["mark_ms"]))
    return e


def main():
    a = parse_args()
    if a.worker:
        return worker(a)
    args = {"parent": ["--sets", "none"], "this": ["--sets", "none,half,tight,variants,both"],
            "this_split": ["--sets", "none,both_split", "--split"]}
    procs = [(name, tree, args[name], False, None) for name, tree in ob.trees(a) + [("this_split", ob.ROOT)]]
    runs, _ = ob.run_rounds(a, __file__, procs, derive,
                            progress=lambda r: ", ".join(f"{s}: " + ob.set_line(v) for s, v in r["sets"].items()))
    summary = ob.summarise(a, runs, "sets", ("parent", "this"), ("none",) + OPTS, entry)
    return ob.write_doc(a, {
        **ob.doc_head(__file__, a), "depth": ob.DEPTH, "bounds": {"half": list(HALF), "tight": list(TIGHT)},
        "note": ob.NOTE + "mark_ms: the parse (C2) / fmt_len (C3) stage with the option minus without, same "
                "process: the marking kernel(s); both: variants and bounds in one kernel, both_split: "
                "SID_DEPTH_SPLIT=1, two kernels.  " + ob.NOTE_ROUNDS,
        "comparisons": comparisons(summary), "summary": summary, "runs": runs})


if __name__ == "__main__":
    sys.exit(main())
