#!/usr/bin/env python3
"""vcf_bench.py -- what the VCF format (--vcf, sid_engine_set_format) costs,
against this build's CSV and against another build of the project (its parent
commit).

Over the C2 text (seed 2, -m local) and the C3 text (seed 3, -R -m
likelihood_ratio), 50M synthetic 30x sites each (one chrom, positions 1..n),
the engine runs with the CSV format (csv: every build) and with the VCF format
(vcf: this build):

  device   text and records in HBM (device_sink 1): the stage times of
           sid_engine_profile_read (HIP event pairs around every stage), per step
  pcie     pinned host text in, records into the pinned host arena
           (device_sink 2 + host_hold_bytes): the step's wall time

What the brackets separate.  The VCF stage is a length kernel and a writer in
place of the CSV's.  On C3 (the Lynch pass 2) the length kernel is the `fmt_len`
stage and the writer the `fmt_write` stage.  On C2 (-m local, one pass) the CSV
has no length kernel at all -- its lengths come out of the tile parse -- so the
VCF length kernel shows as the `parse` bracket with the option minus without
it (len_ms), of the same build in the same process; the writer is `fmt_write`.
write_gbps is the records' bytes over the writer's time.

Every (tree, config) pair is a process of its own (a fresh HIP runtime, the
tree's own sid_amd and libsid.so); the parent tree, which has no such option,
runs the CSV only.  The pairs alternate parent / this tree for --rounds rounds
in one session, so the spread between rounds of the same code stands beside
every difference between the two.

    python tools/gpu/vcf_bench.py --parent DIR [--out profiles/vcf_bench.json]

DIR is a checkout of the parent commit built with `make` (build/libsid.so).
Needs an MI355X; there is no CPU fallback."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optbench as ob
from optbench import rng

KW = {"csv": {}, "vcf": dict(format="vcf")}
ARENA = {"csv": 48, "vcf": 72}   # host arena bytes a site: the whole run's records fit


def parse_args(argv=None):
    return ob.arg_parser(__file__, __doc__, sets=("--sets", "csv"), step_timeout=300).parse_args(argv)


# ------------------------------------------------------------------ worker --
def worker(a):
    cfg, n, text, ln, host, out = ob.worker_start(a, "sets")
    for name in a.sets.split(","):
        r = ob.device_pass(a, cfg, text, ln, KW[name])
        eng, st = ob.pcie_pass(a, cfg, host, ln, n, KW[name], r, site_bytes=ARENA[name])
        r["pcie_chunks_held"] = st.chunks_held
        eng.close()
        out["sets"][name] = r
    return ob.emit(__file__, out)


# ------------------------------------------------------------------ driver --
def comparisons(summary):
    """The comparisons the change is judged by, each stated with its ranges (min .. max over the rounds)."""
    out = {}
    for config, c in summary.items():
        o = {}
        n = c["this_csv"]
        if "parent_csv" in c:
            o["1_without_the_option_within_parent_spread"] = ob.within_parent_spread(n, c["parent_csv"], per_key=True)
        if "this_vcf" in c:
            v = c["this_vcf"]
            o["2_vcf_against_csv"] = {
                "bytes_out": {"csv": n["bytes_out"], "vcf": v["bytes_out"],
                              "ratio": round(v["bytes_out"] / max(n["bytes_out"], 1), 4),
                              "vcf_bytes_per_site": round(v["bytes_out"] / c["sites"], 2),
                              "text_bytes_per_site": round(c["text_bytes"] / c["sites"], 2)},
                "length_stage": "parse, with the option minus without (C2: the CSV's lengths come out of the parse)"
                                if config == "C2" else "fmt_len",
                "len_ms": {"csv": rng(n, "len_ms"), "vcf": rng(v, "len_ms")},
                "fmt_write_ms": {"csv": rng(n, "fmt_write_ms"), "vcf": rng(v, "fmt_write_ms")},
                "write_gbps": {"csv": rng(n, "write_gbps"), "vcf": rng(v, "write_gbps")},
                "device_ms_per_step": {"csv": rng(n, "device_ms_per_step"), "vcf": rng(v, "device_ms_per_step")},
                "pcie_ms_per_step": {"csv": rng(n, "pcie_ms_per_step"), "vcf": rng(v, "pcie_ms_per_step")}}
        out[config] = o
    return out


def derive(r, config):
    stage = "parse" if config == "C2" else "fmt_len"
    for s, v in r["sets"].items():
        # the length stage: C3's fmt_len bracket; C2's parse bracket less the CSV's, same process
        v["len_ms"] = v["device_stages_ms"][stage] - (r["sets"]["csv"]["device_stages_ms"][stage]
                                                      if config == "C2" else 0.0)
        v["write_gbps"] = v["device_bytes_out"] / max(v["device_stages_ms"]["fmt_write"], 1e-9) / 1e6


def entry(ser, s):
    return ob.summary_entry(ser, lead=("len_ms", "write_gbps"),
                            mid={"pcie_chunks_held": ser(lambda v: v.get("pcie_chunks_held", 0))[0]})


def main():
    a = parse_args()
    if a.worker:
        return worker(a)
    runs, _ = ob.run_rounds(
        a, __file__, [(name, tree, ["--sets", "csv,vcf" if name == "this" else "csv"], False, None)
                      for name, tree in ob.trees(a)],
        derive, progress=lambda r: ", ".join(f"{s}: " + ob.set_line(v) for s, v in r["sets"].items()))
    summary = ob.summarise(a, runs, "sets", ("parent", "this"), ("csv", "vcf"), entry)
    for config, c in summary.items():
        first = [r for r in runs if r["config"] == config][0]
        c["sites"], c["text_bytes"] = first["sites"], first["text_bytes"]
    return ob.write_doc(a, {
        **ob.doc_head(__file__, a), "depth": ob.DEPTH,
        "note": ob.NOTE + "len_ms: C3's fmt_len stage; C2's parse stage with the format minus the CSV's, same "
                "process (the CSV's lengths come out of the tile parse).  write_gbps: the records' bytes over "
                "fmt_write.  " + ob.NOTE_ROUNDS,
        "comparisons": comparisons(summary), "summary": summary, "runs": runs})


if __name__ == "__main__":
    sys.exit(main())
