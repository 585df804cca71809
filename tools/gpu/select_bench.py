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
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optbench as ob


def parse_args(argv=None):
    p = ob.arg_parser(__file__, __doc__, sets=("--selects", "all"))
    ob.add_check_args(p, "comparison of the filtered records")
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
    import numpy as np
    cfg, n, text, ln, host, out = ob.worker_start(a, "selects")
    digests = {}
    for sel in a.selects.split(","):
        kw = {} if sel == "all" else {"select": sel}
        r = ob.device_pass(a, cfg, text, ln, kw)
        eng, st = ob.pcie_pass(a, cfg, host, ln, n, kw, r)
        if a.check:
            digests[sel] = [{w: filtered_digest(raw, w, np) for w in ("het", "hom")} if sel == "all" else
                            ob.chunk_digest(raw) for raw in ob.record_chunks(eng, st.chunks)]
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
                    chk[sel]["first_bad_chunk"] = ob.first_bad(want, got)
        out["filtered_bytes_check"] = chk
    return ob.emit(__file__, out)


# ------------------------------------------------------------------ driver --
def main():
    a = parse_args()
    if a.worker:
        return worker(a)
    trees = ob.trees(a)
    runs, _ = ob.run_rounds(
        a, __file__, [(name, tree, ["--selects", "all,het,hom" if name == "this" else "all"], name == "this", None)
                      for name, tree in trees],
        derive=lambda r, config: None,
        progress=lambda r: ", ".join(f"{s}: " + ob.set_line(v, ("fmt_write", "fmt_len"), nbytes=False)
                                     for s, v in r["selects"].items()))
    summary = ob.summarise(a, runs, "selects", [b for b, _ in trees], ("all", "het", "hom"),
                           check_key="filtered_bytes_check")
    return ob.write_doc(a, {**ob.doc_head(__file__, a), "depth": ob.DEPTH, "note": ob.NOTE + ob.NOTE_ROUNDS,
                            "summary": summary, "runs": runs})


if __name__ == "__main__":
    sys.exit(main())
