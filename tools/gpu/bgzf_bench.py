#!/usr/bin/env python3
"""bgzf_bench.py -- what BGZF input costs and saves: the inflate kernel alone,
and the PCIe step fed with compressed bytes against the same step fed with the
plain text, against the host's zlib, and against the parent commit's step.

Input: --sites synthetic 30x sites (seed 2, -m local: the C2 text), packed by
Python's zlib at --level into 0xff00-byte BGZF members (the ratio is reported).

  (a) kernel    sid_bgzf_inflate_device over the whole file resident in HBM:
                wall time of the call (member table upload, launch, sync), in
                GB/s of text produced; the text is compared with the input once
  (b) pcie      pinned host bytes in, records into the pinned host arena
                (device_sink 2 + host_hold_bytes), wall time per step:
                  bgzf    Engine.source_bgzf on the pinned compressed bytes
                  plain   the same build's step on the pinned plain text
                the records of both are compared once
      zlib      the host's zlib inflating the same members on one core (what
                `zcat` costs in front of the plain run)
  (c) parent    the plain-text step of another build (the parent commit)

Every (tree, round) pair is a process of its own (a fresh HIP runtime, the
tree's own sid_amd and libsid.so); parent and this tree alternate for --rounds
rounds in one session, so the spread between rounds of the same code stands
beside every difference between the two.

    python tools/gpu/bgzf_bench.py --parent DIR [--out profiles/bgzf_bench.json]

DIR is a checkout of the parent commit built with `make` (build/libsid.so).
Needs an MI355X; there is no CPU fallback."""
import hashlib
import json
import os
import statistics
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optbench as ob

SEED, PAYLOAD = 2, 0xff00


def parse_args(argv=None):
    p = ob.arg_parser(__file__, __doc__, sites=2_000_000, steps=10, warmup=3, step_timeout=300,
                      process="(tree, round)")
    p.add_argument("--level", type=int, default=6)
    p.add_argument("--chunk-bytes", type=int, default=0, help="engine chunk_bytes (0: its default)")
    p.add_argument("--plain-only", action="store_true")
    return p.parse_args(argv)


def bgzf_member(payload: bytes, level: int) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
    body = c.compress(payload) + c.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25) + body
            + struct.pack("<II", zlib.crc32(payload), len(payload)))


def worker(a):
    sid_amd = ob.load_tree(a.worker)
    import torch
    n = a.sites
    dev = torch.device("cuda", 0)
    ctx = sid_amd.Context(0)   # (kept for the inflate kernel)
    ln, host = ob.make_text(SEED, ob.DEPTH, n, ctx)[1:]   # (the device copy is dropped)
    out = {"sites": n, "text_bytes": ln, "steps": a.steps, "warmup": a.warmup,
           "version": sid_amd.lib().sid_version().decode()}

    def each_step_ms(eng):
        """(every step's ms after the warm-up, the last step's two stats)."""
        for _ in range(a.warmup):
            ob.step(eng)
        ms = [ob.timed(eng, 1) for _ in range(a.steps)]
        return [m[0] for m in ms], ms[-1][1], ms[-1][2]

    def records_digest(eng, chunks):
        return hashlib.blake2b(eng.records_bytes(chunks)).hexdigest()

    def engine():
        return sid_amd.Engine(method="local", devices=1, device_sink=2, host_hold_bytes=int(n * 48) + (64 << 20),
                              chunk_bytes=a.chunk_bytes)

    eng = engine()
    eng.source_host_ptr(host.data_ptr(), ln, keep=host)
    ms, st, st2 = each_step_ms(eng)
    out["plain"] = {"ms": ms, "chunks": st.chunks, "bytes_out": st2.bytes_out, "h2d_bytes": st.h2d_bytes,
                    "records": records_digest(eng, st.chunks)}
    eng.close()
    if not a.plain_only:
        raw = host.numpy().tobytes()
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:   # (zlib releases the interpreter lock)
            members = list(ex.map(lambda k: bgzf_member(raw[k:k + PAYLOAD], a.level), range(0, ln, PAYLOAD)))
        z = b"".join(members) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
        out["compress_s"] = time.perf_counter() - t0
        out["bgzf_bytes"], out["level"], out["ratio"] = len(z), a.level, ln / len(z)
        # the host's zlib, one core, member by member (zcat)
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            got = 0
            for m in members:
                got += len(zlib.decompress(m, 31))
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
        assert got == ln
        out["zlib_inflate_ms"] = best * 1e3
        # (a) the kernel alone
        idx = sid_amd.BgzfIndex(z)
        zh = torch.frombuffer(bytearray(z), dtype=torch.uint8).pin_memory()
        zd = zh.to(dev)
        od = torch.empty(ln + 65536, dtype=torch.uint8, device=dev)
        for _ in range(a.warmup):
            sid_amd.bgzf_inflate_device(ctx, zd, idx, od, cap=ln)
        kms = []
        for _ in range(a.steps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            sid_amd.bgzf_inflate_device(ctx, zd, idx, od, cap=ln)
            kms.append((time.perf_counter() - t0) * 1e3)
        assert bool((od[:ln].cpu() == host).all()), "device inflate differs from the text"
        out["kernel"] = {"ms": kms, "blocks": len(idx), "text_GBps": ln / (statistics.median(kms) * 1e-3) / 1e9}
        del zd, od
        # (b) the PCIe step on the compressed bytes
        eng = engine()
        eng.source_bgzf_host_ptr(zh.data_ptr(), len(z), keep=zh)
        ms, st, st2 = each_step_ms(eng)
        out["bgzf"] = {"ms": ms, "chunks": st.chunks, "bytes_out": st2.bytes_out, "h2d_bytes": st.h2d_bytes,
                       "bgzf_bytes": st.bgzf_bytes, "bgzf_blocks": st.bgzf_blocks,
                       "records": records_digest(eng, st.chunks)}
        eng.close()
        out["records_equal"] = out["bgzf"]["records"] == out["plain"]["records"]
    ctx.close()
    return ob.emit(__file__, out)


def main():
    a = parse_args()
    if a.worker:
        return worker(a)
    runs = []
    for rnd in range(a.rounds):
        for name, tree in ob.trees(a):
            r = ob.run_worker(__file__, ["--worker", tree, "--sites", str(a.sites), "--level", str(a.level), "--steps",
                                         str(a.steps), "--warmup", str(a.warmup), "--chunk-bytes", str(a.chunk_bytes)] +
                              (["--plain-only"] if name == "parent" else []), a.step_timeout, name)
            r["build"], r["round"] = name, rnd
            runs.append(r)
            msg = f"round {rnd} {name}: plain {statistics.median(r['plain']['ms']):.2f} ms"
            if "bgzf" in r:
                msg += (f", bgzf {statistics.median(r['bgzf']['ms']):.2f} ms, kernel "
                        f"{statistics.median(r['kernel']['ms']):.2f} ms ({r['kernel']['text_GBps']:.1f} GB/s of text), "
                        f"zlib {r['zlib_inflate_ms']:.0f} ms, ratio {r['ratio']:.2f}, records equal {r['records_equal']}")
            print(msg, flush=True)
    this = [r for r in runs if r["build"] == "this"]
    par = [r for r in runs if r["build"] == "parent"]
    tb = this[0]["text_bytes"]
    summary = {
        "text_bytes": tb, "bgzf_bytes": this[0]["bgzf_bytes"], "level": a.level, "ratio": this[0]["ratio"],
        "kernel_ms": ob.spread((statistics.median(r["kernel"]["ms"]) for r in this), runs=False),
        "pcie_bgzf_ms": ob.spread((statistics.median(r["bgzf"]["ms"]) for r in this), runs=False),
        "pcie_plain_ms": ob.spread((statistics.median(r["plain"]["ms"]) for r in this), runs=False),
        "zlib_inflate_ms": ob.spread((r["zlib_inflate_ms"] for r in this), runs=False),
        "records_equal": all(r["records_equal"] for r in this),
    }
    summary["kernel_text_GBps"] = tb / (summary["kernel_ms"]["median"] * 1e-3) / 1e9
    summary["pcie_bgzf_sites_per_s"] = a.sites / (summary["pcie_bgzf_ms"]["median"] * 1e-3)
    summary["pcie_plain_sites_per_s"] = a.sites / (summary["pcie_plain_ms"]["median"] * 1e-3)
    if par:
        summary["parent_pcie_plain_ms"] = ob.spread((statistics.median(r["plain"]["ms"]) for r in par), runs=False)
    doc = {**ob.doc_head(__file__, a), "depth": ob.DEPTH, "chunk_bytes": a.chunk_bytes,
           "note": "ms per step, wall time; every figure of a process is the median of its steps, its spread the "
                   "min .. max of those medians over the rounds.  kernel: sid_bgzf_inflate_device on the file in "
                   "HBM (table upload, launch and sync included).  pcie: pinned host bytes in, records into the "
                   "pinned host arena (device_sink 2).  zlib: one host core inflating the same members.  parent / "
                   "this tree alternate within every round",
           "summary": summary, "runs": runs}
    print(json.dumps(summary))
    return ob.write_doc(a, doc)


if __name__ == "__main__":
    sys.exit(main())
