"""--regions FILE (sid_opts.regions) on the device: through build/sid and through
sid_amd.Engine, every formatter (the tile parse and its writers, the two-pass
fallback, the Lynch pass 2, the generic kernels, sid_dtext_format,
--host-parse).

The expected stdout is always the oracle CLI's unfiltered stdout for the same
flags and input, filtered in Python (tests/regions_ref.py, not the library):
each record split from the right, line.rsplit(b",", 6), its chrom compared
byte for byte and start < pos <= end.  stderr and the exit status are the
oracle's own.  Every BED is built from the input's own (chrom, pos) list, and
every case asserts that its expected output keeps at least one record and
drops at least one -- but for the header-only and keep-everything cases, which
assert exactly that."""
import os

import numpy as np
import pytest

from regions_ref import RefSet, bed_points, bed_runs, bed_whole, filter_csv, text_sites
from test_select_gpu import FLAGS, SHAPES, Inputs, line, run

pytestmark = pytest.mark.gpu


def dense_text(n=6000, chrom=b"chr1", first=1) -> bytes:
    return b"".join(line(chrom, first + i, i % 97 == 0) for i in range(n))


class RInputs(Inputs):
    def __init__(self, sid, oracle, d):
        super().__init__(sid, oracle, d)
        self.dir = d
        rng = np.random.default_rng(7)
        extra = {
            "dense": dense_text(),
            # a chrom change every 37 sites (inside waves), names of 4, 8, 9 and 12 bytes, two that share 8 bytes
            "chroms37": b"".join(line([b"chrA", b"chrom_08", b"chrom_08b", b"chrom_08c", b"chromosome12"][(i // 37) % 5],
                                      1 + i % 37 + 40 * (i // 185), i % 5 == 0) for i in range(5000)),
            # positions that run backwards, repeat, and jump (gaps over 127 and over 10^6 positions)
            "order": b"".join(line(b"chr1", p, k % 7 == 0) for k, p in enumerate(
                list(range(3000, 0, -1)) + [5] * 300 + [200 * i for i in range(1, 1500)] +
                [3 * 10 ** 6 * i for i in range(1, 600)] + [int(x) for x in rng.integers(1, 10 ** 7, 1500)])),
            "contigs": b"".join(line(b"contig_%04d" % (c * 7 % 300) if c % 2 else b"ctg%d" % c, i, (c + i) % 9 == 0)
                                for c in range(300) for i in range(1, 31)),
            "wide": b"".join(line(b"chr%d" % (1 + i // 10000), 1 + 50 * (i % 10000), i % 11 == 0) for i in range(20000)),
        }
        for k, t in extra.items():
            self.texts[k] = t
            p = d / f"{k}.plp"
            p.write_bytes(t)
            self.paths[k] = str(p)
        self._sites = {}
        self._beds = {}

    def sites(self, name):
        if name not in self._sites:
            self._sites[name] = text_sites(self.text(name))
        return self._sites[name]

    def bed(self, key, text: bytes):
        """The BED `text` as a file (written once per key) -> (path, RefSet)."""
        if key not in self._beds:
            p = self.dir / f"{key}.bed"
            p.write_bytes(text)
            self._beds[key] = (str(p), RefSet(text), text)
        return self._beds[key][:2]

    def bed_text(self, key):
        return self._beds[key][2]


@pytest.fixture(scope="module")
def inputs(sid, oracle, tmp_path_factory):
    return RInputs(sid, oracle, tmp_path_factory.mktemp("regions"))


def std_bed(inputs, name, kind="mix"):
    """A BED of the input's own sites: runs of 70 in every 5th run, and every 61st site."""
    s = inputs.sites(name)
    if kind == "mix" and name == "edge":   # (few sites, fewer records under the Lynch methods: every second site)
        text = bed_points(s, lambda i: i % 2 == 0)
    elif kind == "mix":
        text = bed_runs(s, lambda i: (i // 70) % 5 == 2) + bed_points(s, lambda i: i % 61 == 0)
    elif kind == "second":
        text = bed_points(s, lambda i: i % 2 == 0)
    elif kind == "61st":
        text = bed_points(s, lambda i: i % 61 == 0)
    elif kind == "runs70":
        text = bed_runs(s, lambda i: (i // 70) % 9 == 3)
    elif kind == "last100":
        text = bed_runs(s, lambda i: i >= len(s) - 100)
    elif kind == "whole":
        text = bed_whole(s)
    else:
        raise KeyError(kind)
    return inputs.bed(f"{name}.{kind}", text)


def expect(inputs, flags, name, ref, select="all", mode="some"):
    b = inputs.ref(flags, name)
    assert b.returncode == 0, b.stderr[-300:]
    want, kept, dropped = filter_csv(b.stdout, ref, select)
    if mode == "header":
        assert kept == 0 and dropped > 0 and want == b.stdout.splitlines(keepends=True)[0]
    elif mode == "all":
        assert dropped == 0 and kept > 0 and want == b.stdout
    else:
        assert kept >= 1 and dropped >= 1, (flags, name, select, kept, dropped)
    return b, want


def check_cli(sid, inputs, flags, name, bed, extra=(), select="all", mode="some"):
    path, ref = bed
    b, want = expect(inputs, flags, name, ref, select, mode)
    sel = [] if select == "all" else ["--only", select]
    a = run(sid.CLI_PATH, list(extra) + ["--regions", path] + sel + list(flags) + [inputs.paths[name]])
    assert a.returncode == 0, (a.returncode, a.stderr[-400:])
    assert a.stdout == want, (flags, name, select, extra)
    assert a.stderr == b.stderr


ENGINE_KW = {(): dict(method="local"), ("-R", "-m", "likelihood_ratio"): dict(method="likelihood_ratio", estimate_prior=True),
             ("-m", "bayes"): dict(method="bayes"), ("-R", "-m", "local"): dict(method="local", estimate_prior=True)}


def check_engine(sid, inputs, flags, name, bed_key, select="all", mode="some", **kw):
    ref = inputs._beds[bed_key][1]
    b, want = expect(inputs, flags, name, ref, select, mode)
    rg = sid.Regions(inputs.bed_text(bed_key))
    eng = sid.Engine(regions=rg, select=select, **ENGINE_KW[tuple(flags)], **kw)
    rg.close()   # (the engine holds its own copy)
    eng.source_text(inputs.text(name))
    out, st = eng.run()
    eng.close()
    assert out == want, (flags, name, select, kw)
    assert st.bytes_out == len(want) - len(sid.HEADER)
    return st


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: " ".join(f) or "default")
def test_cli_flag_sets(sid, inputs, flags):
    for name in ("c1", "edge", "special"):
        check_cli(sid, inputs, flags, name, std_bed(inputs, name))
    check_cli(sid, inputs, flags, "deep", std_bed(inputs, "deep"), extra=["--chunk-bytes", "300000"])
    if tuple(flags) in ENGINE_KW:
        std_bed(inputs, "special")
        check_engine(sid, inputs, flags, "special", "special.mix", chunk_bytes=200_000)


@pytest.mark.parametrize("flags", [["-m", "quality"], ["-R", "-m", "quality"]], ids=lambda f: " ".join(f))
def test_cli_quality(sid, inputs, flags):
    check_cli(sid, inputs, flags, "quality", std_bed(inputs, "quality"))
    check_cli(sid, inputs, flags, "quality", std_bed(inputs, "quality"), extra=["--chunk-bytes", "65536"])


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_cli_engine_shapes(sid, inputs, shape):
    for flags in ([], ["-R", "-m", "likelihood_ratio"]):
        check_cli(sid, inputs, flags, "special", std_bed(inputs, "special"), extra=SHAPES[shape])


def edges_bed(inputs):
    """Intervals whose start, start+1, end and end+1 are all sites of `dense` (positions 1..6000, site i at
    position i + 1), laid inside a wave's window, across 64-slot, 512-slot, tile (~253 lines) and chunk
    boundaries (4096 B: ~50 lines; 65536 B: ~800 lines); one-position intervals among them."""
    marks = sorted(set([40, 64, 128, 192, 253, 254, 255, 256, 506, 507, 512, 1024, 1536, 2048, 5999, 6000] +
                       list(range(49, 6000, 101)) + list(range(800, 6000, 809))))
    out = []
    for b in marks:
        out.append(b"chr1\t%d\t%d\n" % (b - 1, b))          # position b alone
        out.append(b"chr1\t%d\t%d\n" % (b + 2, b + 6))      # b+3 .. b+6: an interval across the mark's neighbours
    out.append(b"chr1\t0\t1\nchr1\t0\t0\n")
    return inputs.bed("dense.edges", b"".join(out))


@pytest.mark.parametrize("extra", [[], ["--chunk-bytes", "4096"], ["--chunk-bytes", "65536"]], ids=lambda e: "-".join(e) or "one")
def test_interval_edges(sid, inputs, extra):
    bed = edges_bed(inputs)
    for flags in ([], ["-R", "-m", "likelihood_ratio"], ["-E", "-0.5"]):
        check_cli(sid, inputs, flags, "dense", bed, extra=extra)
    kw = {"chunk_bytes": int(extra[1])} if extra else {}
    check_engine(sid, inputs, [], "dense", "dense.edges", **kw)
    check_engine(sid, inputs, ["-m", "bayes"], "dense", "dense.edges", **kw)


@pytest.mark.parametrize("kind", ["second", "61st", "runs70", "last100"])
def test_placements(sid, inputs, kind):
    """Groups and chunks without a byte, and with every record."""
    bed = std_bed(inputs, "dense", kind)
    for flags, extra in (([], ["--chunk-bytes", "65536"]), ([], []), (["-m", "bayes"], ["--chunk-bytes", "65536"]),
                         (["-R", "-m", "local"], ["--chunk-bytes", "100000", "--hold-bytes", "1"])):
        check_cli(sid, inputs, flags, "dense", bed, extra=extra)
    check_engine(sid, inputs, [], "dense", f"dense.{kind}", chunk_bytes=65536)


def test_all_of_one_chunk_and_none_of_the_next(sid, inputs):
    s = inputs.sites("dense")
    inputs.bed("dense.half", bed_runs(s, lambda i: (i // 750) % 2 == 0))   # ~61 KB of text each
    for flags in ([], ["-R", "-m", "likelihood_ratio"]):
        check_cli(sid, inputs, flags, "dense", inputs.bed("dense.half", b""), extra=["--chunk-bytes", "60000"])
        check_engine(sid, inputs, flags, "dense", "dense.half", chunk_bytes=60000)


def test_chroms(sid, inputs):
    s = inputs.sites("chroms37")
    names = {c for c, _ in s}
    assert {b"chrom_08", b"chrom_08b", b"chrom_08c"} <= names
    # only some chroms, an absent one, and one that shares its first 8 bytes with input chroms
    some = bed_runs(s, lambda i: s[i][0] in (b"chrom_08b", b"chromosome12") and i % 37 > 5) + \
        bed_points(s, lambda i: s[i][0] == b"chrA" and i % 3 == 0) + \
        b"chrom_08d\t0\t1000\nchrB\nchromosome13\t0\t100000\n"
    bed = inputs.bed("chroms37.some", some)
    for flags in ([], ["-R", "-m", "likelihood_ratio"], ["-E", "-0.5"]):
        for extra in ([], ["--chunk-bytes", "4096"]):
            check_cli(sid, inputs, flags, "chroms37", bed, extra=extra)
    check_engine(sid, inputs, [], "chroms37", "chroms37.some")
    # a whole chromosome of several
    check_cli(sid, inputs, [], "chroms37", inputs.bed("chroms37.one", b"chrom_08b\n"))


def test_order_does_not_matter(sid, inputs):
    s = inputs.sites("order")
    bed = inputs.bed("order.mix", bed_points(s, lambda i: i % 5 == 0) + b"chr1\t100\t180\nchr1\t2000000\t9000000\n")
    for flags in ([], ["-m", "bayes"]):
        for extra in ([], ["--chunk-bytes", "65536"]):
            check_cli(sid, inputs, flags, "order", bed, extra=extra)
    check_engine(sid, inputs, [], "order", "order.mix")


def test_large_tables(sid, inputs):
    rng = np.random.default_rng(11)
    st = rng.integers(0, 2_000_000, 90_000)   # (the sites lie below 500,000: most intervals hold none)
    ln = rng.integers(0, 5, 90_000)
    ch = rng.integers(1, 3, 90_000)
    big = b"".join(b"chr%d\t%d\t%d\n" % (c, a, a + w) for c, a, w in zip(ch, st, ln))
    bed = inputs.bed("wide.big", big)
    assert bed[1].intervals >= 50_000
    for flags in ([], ["-R", "-m", "likelihood_ratio"]):
        check_cli(sid, inputs, flags, "wide", bed, extra=["--chunk-bytes", "300000"])
    check_engine(sid, inputs, [], "wide", "wide.big", chunk_bytes=300_000)
    s = inputs.sites("contigs")
    names = sorted({c for c, _ in s})
    assert len(names) == 300
    cb = b"".join(b"%s\t%d\t%d\n" % (c, k % 20, k % 20 + 7) for k, c in enumerate(names) if k % 3) + \
        b"".join(b"nocontig_%d\n" % k for k in range(50))
    bed = inputs.bed("contigs.many", cb)
    assert bed[1].chroms >= 200
    for flags in ([], ["-m", "bayes"]):
        check_cli(sid, inputs, flags, "contigs", bed)
    check_engine(sid, inputs, [], "contigs", "contigs.many")


@pytest.mark.parametrize("select", ["het", "hom"])
def test_combined_with_only(sid, inputs, select):
    for name in ("special", "dense"):
        bed = std_bed(inputs, name)
        for flags in ([], ["-R", "-m", "likelihood_ratio"], ["-E", "-0.5"]):
            if name == "dense" and flags == ["-E", "-0.5"]:
                continue   # (every site of `dense` is hom under a negative base: nothing to tell apart)
            check_cli(sid, inputs, flags, name, bed, select=select)
        check_cli(sid, inputs, [], name, bed, select=select, extra=["--host-parse"])
        check_cli(sid, inputs, ["-R", "-m", "local"], name, bed, select=select,
                  extra=["--chunk-bytes", "100000", "--hold-bytes", "1"])
        check_engine(sid, inputs, [], name, f"{name}.mix", select=select, chunk_bytes=100_000)


@pytest.mark.parametrize("which", ["empty", "absent"])
def test_header_only(sid, inputs, which):
    text = b"" if which == "empty" else b"# nothing here\nchrNone\t0\t100000\nchr1x\n"
    bed = inputs.bed(f"none.{which}", text)
    for flags in ([], ["-R", "-m", "likelihood_ratio"]):
        for extra in ([], ["--chunk-bytes", "65536"], ["--chunk-bytes", "65536", "--hold-bytes", "1"],
                      ["--chunk-bytes", "65536", "--host-hold", "100000"], ["--host-parse"]):
            check_cli(sid, inputs, flags, "dense", bed, extra=extra, mode="header")
    for kw in ({}, {"chunk_bytes": 65536}, {"chunk_bytes": 65536, "hold_bytes": 1},
               {"chunk_bytes": 65536, "host_hold_bytes": 1 << 20}):
        st = check_engine(sid, inputs, [], "dense", f"none.{which}", mode="header", **kw)
        assert st.bytes_out == 0 and st.sites == 6000
    rg = sid.Regions(text)
    eng = sid.Engine(regions=rg, device_sink=2, chunk_bytes=65536, host_hold_bytes=1 << 20)
    rg.close()
    eng.source_text(inputs.text("dense"))
    st = eng.ingest()
    eng.estimate()
    _, st2 = eng.emit()
    assert st.chunks >= 4 and st2.bytes_out == 0
    assert eng.records_bytes(st.chunks) == b""
    eng.close()


def test_keep_everything(sid, inputs):
    for name in ("special", "dense"):
        bed = std_bed(inputs, name, "whole")
        for flags in ([], ["-R", "-m", "likelihood_ratio"], ["-E", "-0.5"]):
            check_cli(sid, inputs, flags, name, bed, mode="all")
    st = check_engine(sid, inputs, [], "dense", "dense.whole", mode="all", chunk_bytes=100_000)
    assert st.chunks >= 3 and st.chunks_tiled == st.chunks


@pytest.mark.parametrize("method", ["local", "likelihood_ratio"])
def test_engine_host_arena_records(sid, inputs, method):
    flags = [] if method == "local" else ["-R", "-m", method]
    _, ref = std_bed(inputs, "special")
    b, want = expect(inputs, flags, "special", ref)
    text = inputs.text("special")
    rg = sid.Regions(inputs.bed_text("special.mix"))
    eng = sid.Engine(method=method, estimate_prior=method != "local", regions=rg, device_sink=2,
                     chunk_bytes=100_000, host_hold_bytes=len(text))
    rg.close()
    eng.source_text(text)
    st = eng.ingest()
    eng.estimate()
    _, st2 = eng.emit()
    got = eng.records_bytes(st.chunks)
    assert st.chunks >= 4 and st2.bytes_out == len(got)
    assert sid.HEADER + got == want
    eng.close()


def test_device_sink_counts_the_selected_bytes(sid, inputs):
    _, ref = std_bed(inputs, "dense")
    _, want = expect(inputs, [], "dense", ref)
    rg = sid.Regions(inputs.bed_text("dense.mix"))
    eng = sid.Engine(regions=rg, device_sink=1, chunk_bytes=65536)
    eng.source_text(inputs.text("dense"))
    _, st = eng.run()
    assert st.bytes_out == len(want) - len(sid.HEADER)
    eng.close()
    rg.close()


def test_dtext_format_honours_the_context(sid, gpu, inputs):
    """sid_dtext_format on a context with a set, and with a set plus a selection; the caller's codes stay."""
    import torch
    text = inputs.text("synth")
    ref = inputs.ref([], "synth")
    _, rs = std_bed(inputs, "synth")
    for select in ("all", "het"):
        rg = sid.Regions(inputs.bed_text("synth.mix"))
        ctx = sid.Context(0, method="local", select=select, regions=rg)
        rg.close()
        t = sid.DText(ctx, text)
        n = len(t)
        _, dcode, dhom, dhet = gpu.device_buffers(n)
        ctx.call_local(t.counts_ptr, n, dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr())
        torch.cuda.synchronize()
        before = dcode[:n].cpu().numpy().copy()
        want, kept, dropped = filter_csv(ref.stdout, rs, select)
        assert kept >= 1 and dropped >= 1
        assert sid.HEADER + t.format(dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr(), "p_value") == want
        assert (dcode[:n].cpu().numpy() == before).all()
        t.close()
        ctx.close()


def test_engine_reuse_and_engines_do_not_share_sets(sid, inputs):
    for method, flags in (("local", []), ("likelihood_ratio", ["-R", "-m", "likelihood_ratio"])):
        kw = dict(method=method, estimate_prior=method != "local", chunk_bytes=200_000)
        for name in ("synth", "synth2", "special"):
            std_bed(inputs, name)
        # one set for the three texts (the synthetic ones share their chrom names; `special` has its own,
        # so the chroms of the set that a run's sites hit change between the runs)
        both = inputs.bed_text("synth.mix") + inputs.bed_text("synth2.mix") + inputs.bed_text("special.mix")
        rs = inputs.bed("synth.both", both)[1]
        rg = sid.Regions(both)
        eng = sid.Engine(regions=rg, **kw)
        rg.close()
        for name in ("synth", "special", "synth2", "synth"):
            _, want = expect(inputs, flags, name, rs)
            eng.source_text(inputs.text(name))
            out, st = eng.run()
            assert out == want, (method, name)
            assert st.bytes_out == len(want) - len(sid.HEADER)
        rg2 = sid.Regions(inputs.bed_text("synth.mix"))
        other = sid.Engine(regions=rg2, **kw)
        rg2.close()
        other.source_text(inputs.text("synth"))
        assert other.run()[0] == expect(inputs, flags, "synth", inputs._beds["synth.mix"][1])[1]
        full = sid.Engine(**kw)
        full.source_text(inputs.text("synth"))
        assert full.run()[0] == inputs.ref(flags, "synth").stdout
        eng.source_text(inputs.text("synth2"))
        assert eng.run()[0] == expect(inputs, flags, "synth2", rs)[1]
        for e in (eng, other, full):
            e.close()


def test_malformed_line_in_the_last_chunk(sid, inputs):
    b = inputs.ref([], "bad_late")
    assert b.returncode != 0 and b.stdout == b""
    path, _ = inputs.bed("bad.bed", b"chr1\t0\t3000\n")
    for extra in ([], ["--chunk-bytes", "65536"], ["--chunk-bytes", "65536", "--hold-bytes", "1"], ["--host-parse"]):
        a = run(sid.CLI_PATH, extra + ["--regions", path, inputs.paths["bad_late"]])
        assert a.returncode == b.returncode, (extra, a.returncode, b.returncode)
        assert a.stdout == b""
        assert a.stderr == b.stderr


def test_cli_errors(sid, inputs, tmp_path):
    missing = str(tmp_path / "no_such.bed")
    a = run(sid.CLI_PATH, ["--regions", missing, inputs.paths["c1"]])
    assert (a.returncode, a.stdout, a.stderr) == (1, b"", b"sid: --regions: could not open %s\n" % missing.encode())
    a = run(sid.CLI_PATH, ["--regions", str(tmp_path), inputs.paths["c1"]])   # a directory opens, and cannot be read
    assert (a.returncode, a.stdout, a.stderr) == (1, b"", b"sid: --regions: could not open %s\n" % str(tmp_path).encode())
    bad = tmp_path / "bad.bed"
    bad.write_bytes(b"chr1\t0\t10\n# fine\nchr1\t7\n")
    for extra in ([], ["--host-parse"], ["-m", "bayes"]):
        a = run(sid.CLI_PATH, extra + ["--regions", str(bad), inputs.paths["c1"]])
        assert (a.returncode, a.stdout) == (1, b"")
        assert a.stderr == b"sid: --regions: %s:3: malformed region\n" % str(bad).encode()
    # given twice: the last wins
    p1, _ = inputs.bed("none.empty2", b"")
    p2, ref = std_bed(inputs, "c1")
    _, want = expect(inputs, [], "c1", ref)
    a = run(sid.CLI_PATH, ["--regions", p1, "--regions", p2, inputs.paths["c1"]])
    assert a.returncode == 0 and a.stdout == want
    with pytest.raises(sid.SidError):
        sid.Engine(regions="chr1")


def test_help_text_is_the_reference_s(sid, oracle):
    a, b = run(sid.CLI_PATH, ["-h"]), oracle.run_cli(["-h"])
    assert a.stdout == b.stdout and b"--regions" not in a.stdout
