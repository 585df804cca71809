#!/usr/bin/env python3
"""windows_bench.py -- what --windows W (sid_opts.window) costs, against another
build of the project (its parent commit).

Over the C2 text (seed 2, -m local) and the C3 text (seed 3, -R -m
likelihood_ratio), 50M synthetic 30x sites each, the engine runs

  none     no option
  win      --windows 100000                  (this tree only)
  hetwin   --only het --windows 100000       (this tree only)

  device   text and records in HBM (device_sink 1): the stage times of
           sid_engine_profile_read (HIP event pairs around every stage), per step
  pcie     pinned host text in, records into the pinned host arena
           (device_sink 2 + host_hold_bytes): the step's wall time

The window stage runs inside a stage the engine already brackets -- the tile
parse's (`parse`) for -m local, the length stage (`fmt_len`) for the Lynch
pass 2 -- so its time is that stage's with the option minus the same stage's
of the plain run, same build, same process (window_ms).  With --only het the
difference also holds the marking stage that selects (the selection goes the
context's way under --windows: the unselected parse and tables).

Every (tree, config) pair is a process of its own (a fresh HIP runtime, the
tree's own sid_amd and libsid.so).  The pairs alternate parent / this tree for
--rounds rounds in one session; the spread of a figure is its min .. max over
the rounds.  Each timed window is warmed up by --warmup steps and holds --steps.
A process that fails or runs past --step-timeout ends the whole script.

Once per configuration (this tree, first round) the rows are checked: their
sites add up to the run's, their records to the plain run's record count (its
newlines), the rows with --only het equal the rows without, the records with
the option equal the records without (win against none), and every row is a
window of its chrom in ascending order.

    python tools/gpu/windows_bench.py --parent DIR [--out profiles/windows_bench.json]

DIR is a checkout of the parent commit built with `make` (build/libsid.so).
Needs an MI355X; there is no CPU fallback."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optbench as ob
from optbench import rng

W = 100_000
SELS = {"none": {}, "win": {"window": W}, "hetwin": {"select": "het", "window": W}}


def parse_args(argv=None):
    p = ob.arg_parser(__file__, __doc__, sets=("--sels", "none"), step_timeout=400)
    ob.add_parent_all(p)
    ob.add_check_args(p, "check of the rows")
    return p.parse_args(argv)


# ------------------------------------------------------------------ worker --
def worker(a):
    cfg, n, text, ln, host, out = ob.worker_start(a, "sels")
    import sid_amd

    def device_rows(eng, r):
        r["device_rows"] = len(eng.windows())

    rows, digest, newlines = {}, {}, None
    for name in a.sels.split(","):
        kw = SELS[name]
        r = ob.device_pass(a, cfg, text, ln, kw, before_close=device_rows if "window" in kw else None,
                           omit=("device_chunks_per_step",))
        eng, st = ob.pcie_pass(a, cfg, host, ln, n, kw, r)
        if "window" in kw:
            rows[name] = eng.windows()
            r["rows"] = len(rows[name])
            r["rows_csv_bytes"] = len(sid_amd.windows_format(rows[name]))
        if a.check and name in ("none", "win"):
            digest[name], nl = ob.records_digest(eng, st.chunks)
            if name == "none":
                newlines = nl
        eng.close()
        out["sels"][name] = r
    if a.check and "win" in rows:
        rw = rows["win"]
        ordered = all(r[1] % W == 0 and r[2] == r[1] + W and r[4] == r[5] + r[6] for r in rw) and \
            all(a_[0] != b_[0] or a_[1] < b_[1] for a_, b_ in zip(rw, rw[1:]))
        out["rows_check"] = {"rows": len(rw), "sites_sum": sum(r[3] for r in rw), "sites": n,
                             "records_sum": sum(r[4] for r in rw), "records_of_the_plain_run": newlines,
                             "het_sum": sum(r[5] for r in rw), "windows_in_order": ordered,
                             "rows_equal_with_only_het": rows.get("hetwin") == rw,
                             "records_equal_with_and_without": digest.get("win") == digest.get("none"),
                             "equal": bool(sum(r[3] for r in rw) == n and sum(r[4] for r in rw) == newlines and ordered and
                                           rows.get("hetwin") == rw and digest.get("win") == digest.get("none"))}
    return ob.emit(__file__, out)


# ------------------------------------------------------------------ driver --
def comparisons(summary):
    out = {}
    for config, c in summary.items():
        if "parent_none" not in c:
            continue
        o = {}
        p, t = c["parent_none"], c["this_none"]
        o["unchanged_without_the_option"] = ob.within_parent_spread(t, p)
        w, h = c["this_win"], c["this_hetwin"]
        o["window_cost"] = {
            "window_ms": {"win": rng(w, "window_ms"), "hetwin": rng(h, "window_ms")},
            "device_ms_per_step": {"win": rng(w, "device_ms_per_step"), "hetwin": rng(h, "device_ms_per_step"),
                                   "none": rng(t, "device_ms_per_step"), "parent_none": rng(p, "device_ms_per_step")},
            "pcie_ms_per_step": {"win": rng(w, "pcie_ms_per_step"), "hetwin": rng(h, "pcie_ms_per_step"),
                                 "none": rng(t, "pcie_ms_per_step"), "parent_none": rng(p, "pcie_ms_per_step")}}
        pw, pp = rng(w, "pcie_ms_per_step"), rng(p, "pcie_ms_per_step")
        o["pcie_step_with_windows_overlaps_parent_unselected"] = {
            "met": pw[0] <= pp[1] and pp[0] <= pw[1], "win": pw, "parent_none": pp,
            "apart_by_ms": round(max(pw[0] - pp[1], pp[0] - pw[1], 0.0), 3)}
        width = (p["pcie_ms_per_step"]["max"] - p["pcie_ms_per_step"]["min"]) + \
                (h["pcie_ms_per_step"]["max"] - h["pcie_ms_per_step"]["min"])
        o["pcie_step_only_het_windows_below_parent_unselected_by_more_than_both_ranges"] = {
            "met": h["pcie_ms_per_step"]["max"] < p["pcie_ms_per_step"]["min"] - width,
            "hetwin": rng(h, "pcie_ms_per_step"), "parent_none": pp, "combined_width": round(width, 3)}
        out[config] = o
    return out


def derive(r, config):
    stage = "parse" if config == "C2" else "fmt_len"   # the stage that holds the window kernels
    for s in ("win", "hetwin"):
        if s in r["sels"]:
            r["sels"][s]["window_ms"] = (r["sels"][s]["device_stages_ms"][stage] -
                                         r["sels"]["none"]["device_stages_ms"][stage])


def entry(ser, s):
    e = ob.summary_entry(ser)
    if s != "none":
        e["window_ms"] = ob.spread(ser(lambda v: v["window_ms"]))
        e["rows"] = ser(lambda v: v["rows"])[0]
        e["rows_csv_bytes"] = ser(lambda v: v["rows_csv_bytes"])[0]
    return e


def main():
    a = parse_args()
    if a.worker:
        return worker(a)
    trees = ob.trees(a)
    runs, _ = ob.run_rounds(
        a, __file__, [(name, tree, ["--sels", "none,win,hetwin" if name == "this" or a.parent_all else "none"],
                       name == "this", None) for name, tree in trees],
        derive, progress=lambda r: ", ".join(
            f"{s}: " + ob.set_line(v) + (f", {v['rows']} rows" if "rows" in v else "")
            for s, v in r["sels"].items()) + ob.check_note(r, "rows_check"))
    summary = ob.summarise(a, runs, "sels", [b for b, _ in trees], SELS, entry, check_key="rows_check")
    return ob.write_doc(a, {
        **ob.doc_head(__file__, a), "depth": ob.DEPTH, "window": W,
        "note": ob.NOTE + "window_ms: the stage that holds the window kernels (C2: parse, the tile parse; C3: "
                "fmt_len) with the option minus the plain run's, same process (hetwin: the selecting marks "
                "included).  " + ob.NOTE_ROUNDS,
        "comparisons": comparisons(summary), "summary": summary, "runs": runs})


if __name__ == "__main__":
    sys.exit(main())
