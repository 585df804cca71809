#!/usr/bin/env python3
"""depth_hist_bench.py -- what --depth-hist (sid_engine_set_depth_hist) costs,
against another build of the project (its parent commit), and which of the
stage's two aggregation forms is faster.

Inputs: the C2 text (seed 2, -m local) and the C3 text (seed 3, -R -m
likelihood_ratio), --sites synthetic 30x sites each, and D200, a 200x text
(seed 5, -m local) of the same number of read bases (--sites * 30 / 200 sites).
The engine runs

  none     no option
  dh       the depth histogram                 (this tree only)
  win      --windows 100000, the peer summary  (this tree only)

  device   text and records in HBM (device_sink 1): the stage times of
           sid_engine_profile_read (HIP event pairs around every stage), per step
  pcie     pinned host text in, records into the pinned host arena
           (device_sink 2 + host_hold_bytes): the step's wall time

The histogram's stage runs inside a stage the engine already brackets -- the
tile parse's (`parse`) for -m local, the length stage (`fmt_len`) for the Lynch
pass 2 and for a chunk on the two-pass path -- so its time is parse + fmt_len
with the option minus the same sum of the plain run, same build, same process
(stage_ms; the window stage's likewise, for the peer).  The aggregation form
(SID_DH_FORM: 0 an LDS atomic a lane, 1 a wave's distinct depths one by one) is
read once per process, so each form has processes of its own: this_f0, this_f1.

Every (tree, form, config) is a process of its own (a fresh HIP runtime, the
tree's own sid_amd and libsid.so) under its own time limit.  The processes
alternate parent / this tree for --rounds rounds in one session; the spread of
a figure is its min .. max over the rounds.  A process that fails or runs past
--step-timeout ends the whole script; a round that would start past --budget-s
is not started and the file says how many rounds ran.

Once per configuration and form (this tree, first round) the rows are checked:
their sites add up to the run's, their records to the plain run's record count
(its newlines), the records with the option equal the records without, the
device-sink and PCIe runs give the same rows, the four column sums equal the
window rows', and (in the driver) both forms give the same rows.

    python tools/gpu/depth_hist_bench.py --parent DIR [--out profiles/depth_hist_bench.json]

DIR is a checkout of the parent commit built with `make` (build/libsid.so).
Needs an MI355X; there is no CPU fallback."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optbench as ob
from optbench import rng

W = 100_000
SELS = {"none": {}, "dh": {"depth_hist": True}, "win": {"window": W}}


def parse_args(argv=None):
    p = ob.arg_parser(__file__, __doc__, sets=("--sels", "none"), configs="C2,C3,D200", step_timeout=300,
                      process="(tree, form, config)")
    ob.add_check_args(p, "check of the rows")
    p.add_argument("--budget-s", type=int, default=0, help="start no round past this many seconds (0: no limit)")
    return p.parse_args(argv)


# ------------------------------------------------------------------ worker --
def worker(a):
    cfg, n, text, ln, host, out = ob.worker_start(a, "sels", form=os.environ.get("SID_DH_FORM", "default"))
    import sid_amd
    seen = {}

    def device_rows(eng, r):
        seen["drows"] = eng.depth_hist()

    rows, wrows, digest, newlines = None, None, {}, None
    for name in a.sels.split(","):
        kw = SELS[name]
        r = ob.device_pass(a, cfg, text, ln, kw, before_close=device_rows if name == "dh" else None,
                           omit=("device_chunks_per_step",))
        eng, st = ob.pcie_pass(a, cfg, host, ln, n, kw, r)
        if name == "dh":
            rows = eng.depth_hist()
            r["rows"] = len(rows)
            r["rows_csv_bytes"] = len(sid_amd.depth_hist_format(rows))
            r["rows_digest"] = hashlib.blake2b(repr(rows).encode()).hexdigest()
            r["modal_depth"] = max(rows, key=lambda x: x[1])[0] if rows else None
        if name == "win":
            wrows = eng.windows()
        if a.check and name in ("none", "dh"):
            digest[name], nl = ob.records_digest(eng, st.chunks)
            if name == "none":
                newlines = nl
        eng.close()
        out["sels"][name] = r
    if a.check and rows is not None:
        drows = seen.get("drows")
        sums = tuple(sum(x[k] for x in rows) for k in (1, 2, 3, 4))
        wsums = tuple(sum(x[k] for x in wrows) for k in (3, 4, 5, 6)) if wrows is not None else None
        ordered = all(x[0] < y[0] for x, y in zip(rows, rows[1:])) and all(x[2] == x[3] + x[4] for x in rows)
        chk = {"rows": len(rows), "sites_sum": sums[0], "sites": n, "records_sum": sums[1],
               "records_of_the_plain_run": newlines, "rows_in_order": ordered,
               "device_sink_rows_equal_pcie_rows": drows == rows,
               "records_equal_with_and_without": digest.get("dh") == digest.get("none"),
               "column_sums_equal_the_window_rows": None if wsums is None else sums == wsums}
        chk["equal"] = bool(sums[0] == n and sums[1] == newlines and ordered and drows == rows and
                            digest.get("dh") == digest.get("none") and wsums in (None, sums))
        out["rows_check"] = chk
    return ob.emit(__file__, out)


# ------------------------------------------------------------------ driver --
def comparisons(summary, sites):
    out = {}
    for config, c in summary.items():
        o = {}
        if "parent_none" in c:
            for b in ("this_f0", "this_f1"):
                if b + "_none" in c:
                    o[b + "_unchanged_without_the_option"] = ob.within_parent_spread(c[b + "_none"], c["parent_none"])
        scale = 50_000_000 / ob.config_sites(config, sites)
        cost = {}
        for b, form in (("this_f0", "lds_atomic_per_lane"), ("this_f1", "wave_ballot_per_distinct_depth")):
            if b + "_dh" in c:
                e = c[b + "_dh"]
                cost[form] = {"stage_ms_per_step": rng(e, "stage_ms"),
                              "stage_ms_per_50M_sites": [round(x * scale, 3) for x in rng(e, "stage_ms")],
                              "pcie_ms_per_step": rng(e, "pcie_ms_per_step"),
                              "pcie_ms_per_step_without": rng(c[b + "_none"], "pcie_ms_per_step"),
                              "pcie_change_ms_median": round(e["pcie_ms_per_step"]["median"] -
                                                             c[b + "_none"]["pcie_ms_per_step"]["median"], 3)}
        if "this_f0_win" in c:
            cost["window_stage_peer"] = {"stage_ms_per_step": rng(c["this_f0_win"], "stage_ms"),
                                         "pcie_ms_per_step": rng(c["this_f0_win"], "pcie_ms_per_step")}
        o["stage_cost"] = cost
        out[config] = o
    return out


def derive(r, config):
    base = r["sels"]["none"]["device_stages_ms"]
    for s in ("dh", "win"):   # the stages that can hold the summary's kernels, against the plain run's
        if s in r["sels"]:
            g = r["sels"][s]["device_stages_ms"]
            r["sels"][s]["stage_ms"] = g["parse"] + g["fmt_len"] - base["parse"] - base["fmt_len"]


def entry(ser, s):
    e = ob.summary_entry(ser)
    if s != "none":
        e["stage_ms"] = ob.spread(ser(lambda v: v["stage_ms"]))
    if s == "dh":
        for k in ("rows", "rows_csv_bytes", "rows_digest", "modal_depth"):
            e[k] = ser(lambda v: v[k])[0]
    return e


def main():
    a = parse_args()
    if a.worker:
        return worker(a)
    # (tree name, tree, selections, checked, SID_DH_FORM: each form has processes of its own, the parent neither)
    procs = ([("parent", os.path.abspath(a.parent), ["--sels", "none"], False, {"SID_DH_FORM": None})]
             if a.parent else []) + \
            [("this_f0", ob.ROOT, ["--sels", "none,win,dh"], True, {"SID_DH_FORM": "0"}),
             ("this_f1", ob.ROOT, ["--sels", "none,dh"], True, {"SID_DH_FORM": "1"})]
    runs, rounds_run = ob.run_rounds(
        a, __file__, procs, derive, budget_s=a.budget_s, progress=lambda r: ", ".join(
            f"{s}: " + ob.set_line(v, ("parse", "fmt_len"), nbytes=False) +
            (f", stage {v['stage_ms']:.3f} ms" if "stage_ms" in v else "") + (f", {v['rows']} rows" if "rows" in v else "")
            for s, v in r["sels"].items()) + ob.check_note(r, "rows_check"))
    summary = ob.summarise(a, runs, "sels", [p[0] for p in procs], SELS, entry)
    for config, c in summary.items():
        checks = {r["build"]: r["rows_check"] for r in runs if r["config"] == config and "rows_check" in r}
        if checks:
            c["rows_check"] = checks
            d = {c[b + "_dh"]["rows_digest"] for b in ("this_f0", "this_f1") if b + "_dh" in c}
            c["both_forms_give_the_same_rows"] = len(d) == 1
    return ob.write_doc(a, {
        **ob.doc_head(__file__, a), "rounds": rounds_run, "rounds_asked": a.rounds, "window": W,
        "note": ob.NOTE + "stage_ms: parse + fmt_len (the stages that hold the summary's kernels) with the option "
                "minus the plain run's, same process.  this_f0 / this_f1: this tree with SID_DH_FORM 0 (an LDS "
                "atomic a lane) / 1 (a wave's distinct depths one by one).  The processes alternate parent / this "
                "tree within every round; the spread of a figure is its min .. max over the rounds.  D200 has "
                "sites * 30 / 200 sites; stage_ms_per_50M_sites scales its figure",
        "comparisons": comparisons(summary, a.sites), "summary": summary, "runs": runs})


if __name__ == "__main__":
    sys.exit(main())
