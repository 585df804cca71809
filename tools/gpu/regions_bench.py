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
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optbench as ob
from optbench import rng

PERIOD, LEN_LO, LEN_HI, SET_SEED = 12_000, 200, 400, 1234


def parse_args(argv=None):
    p = ob.arg_parser(__file__, __doc__, sets=("--sets", "none"))
    ob.add_parent_all(p)
    ob.add_check_args(p, "comparison of the filtered records")
    return p.parse_args(argv)


# ------------------------------------------------------------------ worker --
def sparse_intervals(n, np):
    """(starts, ends), BED convention, over positions 1..n: one interval per PERIOD positions."""
    gen = np.random.default_rng(SET_SEED)
    k = np.arange(0, n, PERIOD, dtype=np.int64)
    s = np.minimum(k + gen.integers(0, PERIOD - LEN_HI, k.size), n - 1)   # (the last one starts inside the text)
    e = np.minimum(s + gen.integers(LEN_LO, LEN_HI + 1, k.size), n)
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
    import numpy as np
    cfg, n, text, ln, host, out = ob.worker_start(a, "sets")
    import sid_amd
    sp_s, sp_e = sparse_intervals(n, np)

    def make_set(name):
        if name == "none":
            return None
        if name == "whole":
            return sid_amd.Regions(b"chr1\n")
        return sid_amd.Regions(b"".join(b"chr1\t%d\t%d\n" % (s, e) for s, e in zip(sp_s.tolist(), sp_e.tolist())))

    digests = {}
    for name in a.sets.split(","):
        rg = make_set(name)
        kw = {} if rg is None else {"regions": rg}
        r = {"intervals": 0 if rg is None else len(rg), **ob.device_pass(a, cfg, text, ln, kw)}
        eng, st = ob.pcie_pass(a, cfg, host, ln, n, kw, r)
        if a.check:
            digests[name] = [{"sparse": filtered_digest(raw, sp_s, sp_e, np), "whole": ob.chunk_digest(raw)}
                             if name == "none" else ob.chunk_digest(raw) for raw in ob.record_chunks(eng, st.chunks)]
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
                    chk[name]["first_bad_chunk"] = ob.first_bad(want, got)
        out["filtered_bytes_check"] = chk
    return ob.emit(__file__, out)


# ------------------------------------------------------------------ driver --
def comparisons(summary):
    """The four comparisons against the parent build, each stated with its ranges (min .. max over the rounds)."""
    def overlap_or_lower(x, y):   # x not above y: the ranges overlap, or x lies below
        return x[0] <= y[1]

    out = {}
    for config, c in summary.items():
        if "parent_none" not in c:
            continue
        p, n, s, w = c["parent_none"], c["this_none"], c["this_sparse"], c["this_whole"]
        keys = ["device_ms_per_step", "pcie_ms_per_step", "parse_ms", "fmt_len_ms", "fmt_write_ms"]
        o = {"1_no_set_within_parent_spread": ob.within_parent_spread(n, p, keys),
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


def derive(r, config):
    stage = "parse" if config == "C2" else "fmt_len"   # the stage that holds the region kernel
    for s, v in r["sets"].items():
        if s != "none":
            v["region_ms"] = v["device_stages_ms"][stage] - r["sets"]["none"]["device_stages_ms"][stage]


def entry(ser, s):
    e = ob.summary_entry(ser, mid={"intervals": ser(lambda v: v["intervals"])[0]})
    if s != "none":
        e["region_ms"] = ob.spread(ser(lambda v: v["region_ms"]))
    return e


def main():
    a = parse_args()
    if a.worker:
        return worker(a)
    trees = ob.trees(a)
    runs, _ = ob.run_rounds(
        a, __file__, [(name, tree, ["--sets", "none,sparse,whole" if name == "this" or a.parent_all else "none"],
                       name == "this", None) for name, tree in trees],
        derive, progress=lambda r: ", ".join(f"{s}: " + ob.set_line(v) for s, v in r["sets"].items()))
    summary = ob.summarise(a, runs, "sets", [b for b, _ in trees], ("none", "sparse", "whole"), entry,
                           check_key="filtered_bytes_check")
    return ob.write_doc(a, {
        **ob.doc_head(__file__, a), "depth": ob.DEPTH,
        "sets": {"sparse": f"an interval of {LEN_LO}-{LEN_HI} positions in every {PERIOD} (seed {SET_SEED})",
                 "whole": "chr1"},
        "note": ob.NOTE + "region_ms: the stage that holds the region kernel (C2: parse, the tile parse; C3: "
                "fmt_len) with the set minus without, same process.  " + ob.NOTE_ROUNDS,
        "comparisons": comparisons(summary), "summary": summary, "runs": runs})


if __name__ == "__main__":
    sys.exit(main())
