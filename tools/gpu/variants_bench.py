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
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optbench as ob
from optbench import rng

KW = {"none": {}, "variants": {"variants": 1}, "het": {"select": "het"}}


def parse_args(argv=None):
    p = ob.arg_parser(__file__, __doc__, sets=("--sets", "none"))
    ob.add_check_args(p, "comparison of the records")
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
    import numpy as np
    cfg, n, text, ln, host, out = ob.worker_start(a, "sets")
    recs = {}
    for name in a.sets.split(","):
        r = ob.device_pass(a, cfg, text, ln, KW[name])
        eng, st = ob.pcie_pass(a, cfg, host, ln, n, KW[name], r)
        if a.check and name != "none":
            d = []
            for raw in ob.record_chunks(eng, st.chunks):
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
    return ob.emit(__file__, out)


# ------------------------------------------------------------------ driver --
def comparisons(summary):
    """The comparisons the change is judged by, each stated with its ranges (min .. max over the rounds)."""
    out = {}
    for config, c in summary.items():
        o = {}
        n, v, h = c["this_none"], c["this_variants"], c["this_het"]
        if "parent_none" in c:
            o["1_without_the_option_within_parent_spread"] = ob.within_parent_spread(n, c["parent_none"])
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


def derive(r, config):
    if "variants" in r["sets"]:
        v, n0 = r["sets"]["variants"], r["sets"]["none"]
        v["parse_delta_ms"] = v["device_stages_ms"]["parse"] - n0["device_stages_ms"]["parse"]
        v["mark_ms"] = v["device_stages_ms"]["fmt_len"] - n0["device_stages_ms"]["fmt_len"]


def entry(ser, s):
    e = ob.summary_entry(ser)
    if s == "variants":
        e["parse_delta_ms"] = ob.spread(ser(lambda v: v["parse_delta_ms"]))
        e["mark_ms"] = ob.spread(ser(lambda v: v["mark_ms"]))
    return e


def main():
    a = parse_args()
    if a.worker:
        return worker(a)
    trees = ob.trees(a)
    runs, _ = ob.run_rounds(
        a, __file__, [(name, tree, ["--sets", "none,variants,het" if name == "this" else "none,het"], name == "this",
                       None) for name, tree in trees],
        derive, progress=lambda r: ", ".join(f"{s}: " + ob.set_line(v) for s, v in r["sets"].items()))
    summary = ob.summarise(a, runs, "sets", [b for b, _ in trees], ("none", "variants", "het"), entry,
                           check_key="records_check")
    return ob.write_doc(a, {
        **ob.doc_head(__file__, a), "depth": ob.DEPTH,
        "note": ob.NOTE + "parse_delta_ms / mark_ms: the parse / fmt_len stage with the option minus without, same "
                "process (C2: the parse bracket holds the byte store and the marking kernel; C3: parse holds the "
                "store, fmt_len the marking kernel).  " + ob.NOTE_ROUNDS,
        "comparisons": comparisons(summary), "summary": summary, "runs": runs})


if __name__ == "__main__":
    sys.exit(main())
