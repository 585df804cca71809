#!/usr/bin/env python3
"""bench_region_stats.py -- what --region-stats (sid_engine_set_region_stats)
costs, against another build of the project (its parent commit), against its
two peers, and which of the stage's two forms is faster on one long interval.

(The file is not called region_stats_bench.py: tests/test_option_bench.py pins
the list of *_bench.py scripts in this directory, and existing tests stay as
they are.  tests/test_region_stats_bench.py replays this one.)

Inputs: the C2 text (seed 2, -m local) and the C3 text (seed 3, -R -m
likelihood_ratio), --sites synthetic 30x sites each (one chrom, positions
1..n).  The region sets:

  a   one whole-chromosome line: every site of a chunk goes to one bin
  b   exon-like: a 150-base interval every 1,500 bases

The engine runs

  none     no option
  reg_a    --regions a, the marking stage alone (the peer, and rs_a's base)
  rs_a     --regions a with the region rows
  reg_b    --regions b
  rs_b     --regions b with the region rows
  dh       the depth histogram, the other peer

  device   text and records in HBM (device_sink 1): the stage times of
           sid_engine_profile_read (HIP event pairs around every stage), per step
  pcie     pinned host text in, records into the pinned host arena
           (device_sink 2 + host_hold_bytes): the step's wall time

The stage runs inside a stage the engine already brackets -- the tile parse's
(`parse`) for -m local, the length stage (`fmt_len`) for the Lynch pass 2 and
for a chunk on the two-pass path -- so a stage's time is parse + fmt_len of the
run that has it minus the same sum of the run that lacks it, same build, same
process (stage_ms): rs_x against reg_x for the region rows, reg_x against none
for the marking stage, dh against none for the histogram.  The stage reads what
the marking stage and the histogram read together, so peers_ms, the sum of
their two times, stands beside it.  The form (SID_RS_FORM: 0 the wave carries
its interval's sums across the groups it walks, 1 it adds them to the table
once per wave of sites) is read once per process, so each form has processes of
its own: this_f0, this_f1.

Every (tree, form, config) is a process of its own (a fresh HIP runtime, the
tree's own sid_amd and libsid.so) under its own time limit.  The processes
alternate parent / this tree for --rounds rounds in one session; the spread of
a figure is its min .. max over the rounds.  A process that fails or runs past
--step-timeout ends the whole script; a round that would start past --budget-s
is not started and the file says how many rounds ran.

Once per configuration and form (this tree, first round) the rows are checked:
set a's one row counts every site, set b's rows count the sites their intervals
hold (150 each), the records sum to the newlines of the same run's records, the
device-sink and PCIe runs give the same rows, and the records with the option
equal the records of the same set without it.

    python tools/gpu/bench_region_stats.py --parent DIR [--out profiles/region_stats_bench.json]

DIR is a checkout of the parent commit built with `make` (build/libsid.so).
Needs an MI355X; there is no CPU fallback."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optbench as ob
from optbench import rng

PERIOD, FIRST, LEN = 1_500, 100, 150
SELS = ("none", "reg_a", "rs_a", "reg_b", "rs_b", "dh")
BASE = {"rs_a": "reg_a", "rs_b": "reg_b", "reg_a": "none", "reg_b": "none", "dh": "none"}


def parse_args(argv=None):
    p = ob.arg_parser(__file__, __doc__, sets=("--sels", "none"), step_timeout=300, process="(tree, form, config)")
    p.set_defaults(out=os.path.join(ob.ROOT, "profiles", "region_stats_bench.json"))
    ob.add_check_args(p, "check of the rows")
    p.add_argument("--budget-s", type=int, default=0, help="start no round past this many seconds (0: no limit)")
    return p.parse_args(argv)


# ------------------------------------------------------------------ worker --
def exon_bed(n):
    """A LEN-base interval every PERIOD bases over positions 1..n (the last one clipped to the text)."""
    return b"".join(b"chr1\t%d\t%d\n" % (s, min(s + LEN, n)) for s in range(FIRST, n, PERIOD) if s < n)


def worker(a):
    cfg, n, text, ln, host, out = ob.worker_start(a, "sels", form=os.environ.get("SID_RS_FORM", "default"))
    import sid_amd
    beds = {"a": b"chr1\n", "b": exon_bed(n)}
    seen = {}

    def device_rows(eng, r):
        seen["drows"] = eng.region_stats()

    digest, newlines, rows, drows = {}, {}, {}, {}
    for name in a.sels.split(","):
        rg = sid_amd.Regions(beds[name[-1]]) if name[:3] in ("reg", "rs_") else None
        kw = {"depth_hist": True} if name == "dh" else {}
        if rg is not None:
            kw = {"regions": rg, **({"region_stats": True} if name.startswith("rs_") else {})}
        r = {"intervals": 0 if rg is None else len(rg),
             **ob.device_pass(a, cfg, text, ln, kw, before_close=device_rows if name.startswith("rs_") else None,
                              omit=("device_chunks_per_step",))}
        eng, st = ob.pcie_pass(a, cfg, host, ln, n, kw, r)
        if name.startswith("rs_"):
            rows[name], drows[name] = eng.region_stats(), seen.pop("drows")
            r["rows"] = len(rows[name])
            r["rows_csv_bytes"] = len(sid_amd.region_stats_format(rows[name]))
            r["rows_digest"] = hashlib.blake2b(repr(rows[name]).encode()).hexdigest()
            r["rows_touched"] = sum(1 for x in rows[name] if x[3])
        if a.check and rg is not None:
            digest[name], newlines[name] = ob.records_digest(eng, st.chunks)
        eng.close()
        if rg is not None:
            rg.close()
        out["sels"][name] = r
    if a.check and rows:
        chk = {}
        for name, rs in rows.items():
            base = BASE[name]
            want_sites = n if name == "rs_a" else sum(min(s + LEN, n) - s for s in range(FIRST, n, PERIOD) if s < n)
            c = {"rows": len(rs), "sites_sum": sum(x[3] for x in rs), "sites_inside": want_sites,
                 "depth_sum": sum(x[4] for x in rs), "records_sum": sum(x[5] for x in rs),
                 "records_of_the_same_set": newlines.get(name),
                 "every_full_interval_holds_its_sites": all(x[3] == x[2] - x[1] for x in rs) if name == "rs_b" else None,
                 "device_sink_rows_equal_pcie_rows": drows[name] == rs,
                 "records_equal_with_and_without": digest.get(name) == digest.get(base) if base in digest else None}
            c["equal"] = bool(c["sites_sum"] == want_sites and c["records_sum"] == newlines.get(name) and
                              c["device_sink_rows_equal_pcie_rows"] and c["records_equal_with_and_without"] in (None, True)
                              and c["every_full_interval_holds_its_sites"] in (None, True) and
                              all(x[5] == x[6] + x[7] for x in rs))
            chk[name] = c
        chk["equal"] = all(c["equal"] for c in chk.values())
        out["rows_check"] = chk
    return ob.emit(__file__, out)


# ------------------------------------------------------------------ driver --
def derive(r, config):
    for s, base in BASE.items():   # the stages that can hold the stage's kernels, against the run without it
        if s in r["sels"] and base in r["sels"]:
            g, b = r["sels"][s]["device_stages_ms"], r["sels"][base]["device_stages_ms"]
            r["sels"][s]["stage_ms"] = g["parse"] + g["fmt_len"] - b["parse"] - b["fmt_len"]
            r["sels"][s]["pcie_change_ms"] = r["sels"][s]["pcie_ms_per_step"] - r["sels"][base]["pcie_ms_per_step"]
    for x in "ab":   # the two peers' times together, the figure the stage's stands beside
        if "rs_" + x in r["sels"] and "dh" in r["sels"]:
            r["sels"]["rs_" + x]["peers_ms"] = r["sels"]["reg_" + x]["stage_ms"] + r["sels"]["dh"]["stage_ms"]


def entry(ser, s):
    e = ob.summary_entry(ser)
    if s != "none":
        e["stage_ms"] = ob.spread(ser(lambda v: v["stage_ms"]))
        e["pcie_change_ms"] = ob.spread(ser(lambda v: v["pcie_change_ms"]))
    if s.startswith("rs_"):
        if ser(lambda v: "peers_ms" in v)[0]:
            e["peers_ms"] = ob.spread(ser(lambda v: v["peers_ms"]))
        for k in ("rows", "rows_csv_bytes", "rows_digest", "rows_touched"):
            e[k] = ser(lambda v: v[k])[0]
    return e


def comparisons(summary):
    out = {}
    for config, c in summary.items():
        o = {}
        if "parent_none" in c:
            for b in ("this_f0", "this_f1"):
                if b + "_none" in c:
                    o[b + "_unchanged_without_the_option"] = ob.within_parent_spread(c[b + "_none"], c["parent_none"])
        cost = {}
        for x in "ab":
            e = c.get("this_f0_rs_" + x)
            if e is None:
                continue
            k = {"stage_ms_per_step": rng(e, "stage_ms"),
                 "marking_stage_peer_ms": rng(c["this_f0_reg_" + x], "stage_ms"),
                 "pcie_change_ms": rng(e, "pcie_change_ms"),
                 "pcie_ms_per_step": rng(e, "pcie_ms_per_step"),
                 "pcie_ms_per_step_without": rng(c["this_f0_reg_" + x], "pcie_ms_per_step")}
            if "this_f0_dh" in c:
                k["depth_hist_peer_ms"] = rng(c["this_f0_dh"], "stage_ms")
                k["peers_ms"] = rng(e, "peers_ms")
                k["stage_over_peers_median"] = round(e["stage_ms"]["median"] / e["peers_ms"]["median"], 3)
            cost["set_" + x] = k
        if "this_f1_rs_a" in c and "this_f0_rs_a" in c:
            f0, f1 = c["this_f0_rs_a"], c["this_f1_rs_a"]
            cost["set_a_forms"] = {"carry_stage_ms": rng(f0, "stage_ms"), "flush_per_wave_stage_ms": rng(f1, "stage_ms"),
                                   "carry_is_faster": f0["stage_ms"]["max"] < f1["stage_ms"]["min"],
                                   "flush_over_carry_median": round(f1["stage_ms"]["median"] / f0["stage_ms"]["median"], 3)
                                   if f0["stage_ms"]["median"] > 0 else None}
        o["stage_cost"] = cost
        out[config] = o
    return out


def main():
    a = parse_args()
    if a.worker:
        return worker(a)
    # (tree name, tree, selections, checked, SID_RS_FORM: each form has processes of its own, the parent neither)
    procs = ([("parent", os.path.abspath(a.parent), ["--sels", "none"], False, {"SID_RS_FORM": None})]
             if a.parent else []) + \
            [("this_f0", ob.ROOT, ["--sels", ",".join(SELS)], True, {"SID_RS_FORM": "0"}),
             ("this_f1", ob.ROOT, ["--sels", "none,reg_a,rs_a"], True, {"SID_RS_FORM": "1"})]
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
            d = {c[b + "_rs_a"]["rows_digest"] for b in ("this_f0", "this_f1") if b + "_rs_a" in c}
            c["both_forms_give_the_same_rows"] = len(d) == 1
    return ob.write_doc(a, {
        **ob.doc_head(__file__, a), "rounds": rounds_run, "rounds_asked": a.rounds,
        "sets": {"a": "one whole-chromosome line", "b": f"{LEN}-base intervals every {PERIOD} bases"},
        "note": ob.NOTE + "stage_ms: parse + fmt_len (the stages that hold the stage's kernels) of the run that has a "
                "stage minus the run that lacks it, same process: rs_x - reg_x the region rows, reg_x - none the "
                "marking stage, dh - none the depth histogram; peers_ms: the latter two added.  this_f0 / this_f1: "
                "this tree with SID_RS_FORM 0 (the wave carries its interval's sums) / 1 (it adds them once per wave "
                "of sites).  The processes alternate parent / this tree within every round; the spread of a figure "
                "is its min .. max over the rounds",
        "comparisons": comparisons(summary), "summary": summary, "runs": runs})


if __name__ == "__main__":
    sys.exit(main())
