"""The depth bounds (--min-depth / --max-depth, sid_engine_set_depth,
sid_set_depth) on the device: through build/sid and through sid_amd.Engine,
every parser (the tile parse's lane and quad shapes, its general routine, the
two-pass path), every formatter family and every record path of the engine.

The expected stdout is always the oracle CLI's unselected stdout for the same
flags and input, filtered in Python by tests/depth_ref.py (the rule restated
from the pileup text: the counts by oracle.read_bases, which lines print a
record), and with a selection by label, region, variant or a context also by
variants_ref / context_ref / regions_ref.  stderr and the exit status are the
oracle's own.  Every case that is no edge case asserts that its expected output
keeps at least one hom and one het record and drops at least one of each; the
edge cases (the header alone, everything kept) assert exactly that."""
import json

import numpy as np
import pytest

import bgzf_ref
import depth_ref as D
import variants_ref as V
from context_ref import dilate, selected
from regions_ref import RefSet, bed_runs, text_sites
from test_select_gpu import run

pytestmark = pytest.mark.gpu

# flag set -> (the CLI's flags, a Lynch method: no record below coverage 4, the Engine's options)
FLAGSETS = {
    "local": ([], False, dict(method="local")),
    "local_R": (["-R", "-m", "local"], False, dict(method="local", estimate_prior=True)),
    "lr": (["-R", "-m", "likelihood_ratio"], True, dict(method="likelihood_ratio", estimate_prior=True)),
    "bayes": (["-m", "bayes"], True, dict(method="bayes")),
    "quality": (["-m", "quality"], False, dict(method="quality")),
}
FOUR = ["local", "local_R", "lr", "bayes"]
ESTATE, EINVAL = 7, 1


FIX_DEPTHS = (34, 40, 41, 46)


def tiny_text() -> bytes:
    """12- to 14-byte lines of depth 1 .. 3, more a tile than any slot list: the tile parse overflows into the
    two-pass path.  Behind them every kind of record at the depths of depth_text."""
    bases = (b"G", b"GA", b"...", b".", b"..", b"GGG", b"G", b"G.", b"AAA")
    t = b"".join(b"c\t%d\t%s\t%d\t%s\t%s\n" % (i % 10, b"ACGT"[i % 4:i % 4 + 1], len(bases[i % 9]), bases[i % 9],
                                              b"I" * len(bases[i % 9])) for i in range(1, 30_000))
    return t + D.depth_text(1500, chrom=lambda i: b"chrB")


def parsers_text() -> bytes:
    rng = np.random.default_rng(65)
    parts = []
    # '+2AC' indels and '^]' carets on lines of every depth: the general routine
    for i in range(1, 701):
        r = b"ACGT"[i % 4:i % 4 + 1]
        b = V.bases_of(V.KINDS[i % 3] if i % 2 else "homref", r, D.DEPTHS[i % 7] if i % 7 > 1 else 29)
        if i % 3 == 0:
            b = b[:5] + b"+2AC" + b[5:]
        elif i % 3 == 1:
            b = b"^]" + b[:6] + b"^]" + b[6:]
        parts.append(V.vline(b"chr7", i, r, b))
    # four alleles in numbers, 34, 40, 41 or 46 read bases: no class table covers them (the fix-up), and
    # their depths lie across a bound of 40
    for i in range(1, 701):
        q = 6 + i % 3
        k = (FIX_DEPTHS[i % 4] - 3 * q - i % 2, q + i % 2, q, q)
        bases = bytearray(b"A" * k[0] + b"c" * k[1] + b"G" * k[2] + b"t" * k[3])
        rng.shuffle(bases)
        parts.append(V.vline(b"chr3", i, b"ACGTN"[i % 5:i % 5 + 1], bytes(bases)))
    return b"".join(parts) + D.depth_text(700, chrom=lambda i: b"chrB")


def geometry_text() -> bytes:
    at = lambda c, p, d, kind="homref", r=b"A": V.vline(c, p, r, V.bases_of(kind, r, d))
    parts = []
    # the first tile's slots: sites outside the bounds (8, 31) at slots 0, 63, 64, 127 and 128
    parts += [at(b"chr1", i + 1, 90 if i in (0, 63, 64, 127, 128) else 30, "hetref" if i % 5 == 0 else "homref")
              for i in range(400)]
    # 600 consecutive sites outside them: whole 512-slot groups without a record
    parts += [at(b"chr1", 401 + i, 4, "hetref" if i % 3 == 0 else "homref") for i in range(600)]
    # a chrom change every 37 sites, names of 4, 8, 9 and 12 bytes: compact words against header pairs
    names = [b"chrA", b"chrom_12", b"chrom_123", b"chromosome12"]
    parts.append(D.depth_text(1200, chrom=lambda i: names[i // 37 % 4]))
    # a 70-byte name: a 512-slot group's records pass the writers' LDS buffer
    parts.append(D.depth_text(700, chrom=lambda i: b"N" * 70))
    return b"".join(parts)


class Inputs:
    """The test inputs as files, and the oracle's run of each (flag set, input), computed once."""

    def __init__(self, sid, oracle, d):
        self.sid, self.oracle, self.dir = sid, oracle, d
        good = D.depth_text()
        texts = {"depth": good, "depthq": D.depth_text(mapq=True), "deep": D.deep_text(),
                 "deepq": D.deep_text(mapq=True), "tiny": tiny_text(), "parsers": parsers_text(),
                 "geom": geometry_text(),
                 "bad_late": good + good + b"chr1\t1\tAC\t3\t...\tIII\n" + D.depth_text(50)}
        self.texts, self.paths = texts, {}
        for k, t in texts.items():
            p = d / f"{k}.plp"
            p.write_bytes(t)
            self.paths[k] = str(p)
        self._ref, self._lines, self._beds = {}, {}, {}

    def ref(self, fs, name):
        if (fs, name) not in self._ref:
            self._ref[(fs, name)] = self.oracle.run_cli(FLAGSETS[fs][0] + [self.paths[name]])
        return self._ref[(fs, name)]

    def lines(self, fs, name):
        """(the oracle's run, its lines, its records' depths, one bool a record: a variant)."""
        if (fs, name) not in self._lines:
            b = self.ref(fs, name)
            assert b.returncode == 0, b.stderr[-300:]
            lines = b.stdout.splitlines(keepends=True)
            self._lines[(fs, name)] = (b, lines, D.record_depths(lines[1:], self.texts[name], FLAGSETS[fs][1]),
                                       V.flags(lines[1:], self.texts[name], FLAGSETS[fs][1]))
        return self._lines[(fs, name)]

    def bed(self, name):
        """A region set built from the input's own sites: runs of 40 sites in every 130."""
        if name not in self._beds:
            text = bed_runs(text_sites(self.texts[name]), lambda i: i % 130 < 40)
            p = self.dir / f"{name}.bed"
            p.write_bytes(text)
            self._beds[name] = (str(p), RefSet(text), text)
        return self._beds[name]


@pytest.fixture(scope="module")
def inputs(sid, oracle, tmp_path_factory):
    return Inputs(sid, oracle, tmp_path_factory.mktemp("depth"))


def expect(inputs, fs, name, bounds, select="all", bed=None, context=0, variants=False, mode="some"):
    """The oracle's run and its stdout filtered: the records within the bounds, and the other selections with
    them; asserts that the case is not vacuous."""
    b, lines, depths, var = inputs.lines(fs, name)
    recs = lines[1:]
    sel = [D.inside(d, *bounds) and s and (v or not variants)
           for d, s, v in zip(depths, selected(recs, select, bed[1] if bed else None), var)]
    keep = dilate(sel, context) if context else sel
    want = lines[0] + b"".join(ln for ln, k in zip(recs, keep) if k)
    n = D.tally(recs, keep)
    if mode == "header":
        assert not any(keep) and len(recs) > 0 and want == lines[0]
    elif mode == "all":
        assert all(keep) and n[(True, b"hom")] >= 1 and n[(True, b"het")] >= 1 and want == b.stdout
    elif mode == "variants":   # among the variants, the numbers kept and dropped
        assert variants and select == "all" and not bed and not context
        nv = D.tally([ln for ln, v in zip(recs, var) if v], [k for k, v in zip(keep, var) if v])
        assert nv[(True, b"hom")] >= 6 and nv[(True, b"het")] >= 12 and nv[(False, b"hom")] >= 13 and \
            nv[(False, b"het")] >= 24, (fs, name, bounds, nv)
    elif select == "all":
        assert min(n.values()) >= 1, (fs, name, bounds, n)
    else:   # with --only: the label's records kept and dropped, the other label's all dropped
        x, y = select.encode(), (b"hom" if select == "het" else b"het")
        assert n[(True, x)] >= 1 and n[(False, x)] >= 1 and n[(False, y)] >= 1 and (context or n[(True, y)] == 0), \
            (fs, name, bounds, n)
    if context:
        assert sum(keep) > sum(sel) >= 1   # (context records)
    return b, want


def cli_args(inputs, fs, name, bounds, select="all", bed=None, context=0, variants=False):
    return (["--min-depth", str(bounds[0]), "--max-depth", str(bounds[1])] + (["--variants"] if variants else []) +
            ([] if select == "all" else ["--only", select]) + (["--regions", bed[0]] if bed else []) +
            (["--context", str(context)] if context else []) + FLAGSETS[fs][0] + [inputs.paths[name]])


def check_cli(sid, inputs, fs, name, bounds, extra=(), mode="some", **sel):
    b, want = expect(inputs, fs, name, bounds, mode=mode, **sel)
    a = run(sid.CLI_PATH, list(extra) + cli_args(inputs, fs, name, bounds, **sel))
    assert a.returncode == 0, (a.returncode, a.stderr[-400:])
    assert a.stdout == want, (fs, name, bounds, extra, sel)
    assert a.stderr == b.stderr
    return a


def check_engine(sid, inputs, fs, name, bounds, select="all", bed=None, context=0, variants=False, mode="some",
                 source="text", **kw):
    b, want = expect(inputs, fs, name, bounds, select, bed, context, variants, mode)
    rg = sid.Regions(bed[2]) if bed else None
    eng = sid.Engine(min_depth=bounds[0], max_depth=bounds[1], variants=int(variants), regions=rg, select=select,
                     context=context, **FLAGSETS[fs][2], **kw)
    if rg:
        rg.close()
    if source == "bgzf":
        eng.source_bgzf(bgzf_ref.write(inputs.texts[name], payload=20_000)[0])
    else:
        eng.source_text(inputs.texts[name])
    out, st = eng.run()
    eng.close()
    assert out == want, (fs, name, bounds, select, context, variants, kw)
    assert st.bytes_out == len(want) - len(sid.HEADER)
    return st


@pytest.mark.parametrize("bounds", D.BOUNDS, ids=str)
@pytest.mark.parametrize("fs", sorted(FLAGSETS))
def test_flag_sets_cli_and_engine(sid, inputs, fs, bounds):
    name = "depthq" if fs == "quality" else "depth"
    check_cli(sid, inputs, fs, name, bounds, extra=["--chunk-bytes", "65536"])   # tile and chunk edges
    st = check_engine(sid, inputs, fs, name, bounds, chunk_bytes=20_000)
    assert st.chunks >= 5


@pytest.mark.parametrize("fs", sorted(FLAGSETS))
def test_deep_text_the_quad_shape_and_the_second_table(sid, inputs, fs):
    name = "deepq" if fs == "quality" else "deep"
    for bounds in D.DEEP_BOUNDS:
        st = check_engine(sid, inputs, fs, name, bounds, chunk_bytes=300_000)
        # (-m quality reads the qualities off the text by line offsets: always the two-pass parse, never a tile)
        assert st.chunks >= 2 and (st.chunks_tiled > 0) == (fs != "quality")
    check_cli(sid, inputs, fs, name, D.DEEP_BOUNDS[2], extra=["--chunk-bytes", "300000"])


def test_edge_cases(sid, inputs):
    for fs in FOUR:
        check_cli(sid, inputs, fs, "depth", (91, 0), mode="header")
        check_cli(sid, inputs, fs, "depth", (0, 0), mode="all")
        check_engine(sid, inputs, fs, "depth", (91, 0), mode="header", chunk_bytes=20_000)
    for fs in ("lr", "bayes"):   # no record below coverage 4 anyway
        for lo in (1, 4):
            check_cli(sid, inputs, fs, "depth", (lo, 0), mode="all")
            check_engine(sid, inputs, fs, "depth", (lo, 0), mode="all", chunk_bytes=20_000)
    st = check_engine(sid, inputs, "local", "depth", (91, 0), mode="header")
    assert st.bytes_out == 0 and st.sites == 3000


def test_two_pass_path_after_a_tile_overflow(sid, inputs):
    st = check_engine(sid, inputs, "local", "tiny", (2, 30), chunk_bytes=100_000)
    assert st.tile_overflows > 0
    check_engine(sid, inputs, "local", "tiny", (3, 0), chunk_bytes=100_000)
    check_engine(sid, inputs, "bayes", "tiny", (0, 30), chunk_bytes=100_000)
    check_cli(sid, inputs, "local_R", "tiny", (2, 30))


@pytest.mark.parametrize("bounds", [(8, 31), (0, 40), (41, 0), (30, 30)], ids=str)
def test_general_routine_and_fix_up(sid, inputs, bounds):
    for fs in FOUR:
        check_cli(sid, inputs, fs, "parsers", bounds)
    for fs in ("local", "bayes"):
        check_cli(sid, inputs, fs, "parsers", bounds, extra=["--chunk-bytes", "65536"])
        check_engine(sid, inputs, fs, "parsers", bounds, chunk_bytes=20_000)


def test_the_fix_up_s_sites_lie_across_the_bound(inputs):
    """(the case's own premise: four-allele sites of 40 read bases and fewer, and of 41 and more)"""
    d = D.depths(inputs.texts["parsers"])[700:1400]
    assert set(d) == set(FIX_DEPTHS) and all(d.count(x) == 175 for x in FIX_DEPTHS)


def test_geometry(sid, inputs):
    for bounds in ((8, 31), (30, 0)):
        for fs in FOUR:
            check_cli(sid, inputs, fs, "geom", bounds)
        for fs in ("local", "lr"):
            check_cli(sid, inputs, fs, "geom", bounds, extra=["--chunk-bytes", "65536"])
            check_engine(sid, inputs, fs, "geom", bounds, chunk_bytes=20_000)
    want = expect(inputs, "local", "geom", (8, 31))[1]
    for p in (1, 64, 65, 128, 129):   # the first tile's slots 0, 63, 64, 127, 128
        assert b"chr1,%d," % p not in want
    for p in (2, 63, 66, 127, 130, 400):
        assert b"chr1,%d," % p in want
    assert not any(b"chr1,%d," % p in want for p in range(401, 1001))


@pytest.mark.parametrize("fs", FOUR)
def test_engine_record_paths(sid, inputs, fs):
    """Pass 2 from the kept parse and from text read again, two lanes, a BGZF source, the host arena."""
    bounds = (8, 31)
    st = check_engine(sid, inputs, fs, "depth", bounds, chunk_bytes=20_000, hold_bytes=1)
    assert st.chunks >= 5 and (fs == "local" or st.chunks_reloaded == 0)
    st = check_engine(sid, inputs, fs, "depth", bounds, chunk_bytes=20_000, hold_bytes=1, retain_bytes=1)
    assert st.chunks_reloaded == st.chunks
    check_engine(sid, inputs, fs, "depth", bounds, chunk_bytes=20_000, lanes=2)
    check_engine(sid, inputs, fs, "depth", bounds, chunk_bytes=20_000, source="bgzf")
    check_engine(sid, inputs, fs, "depth", bounds, chunk_bytes=20_000, host_hold_bytes=3000)
    # the PCIe path without a writer: the expected records in the pinned host arena
    b, want = expect(inputs, fs, "depth", bounds)
    text = inputs.texts["depth"]
    eng = sid.Engine(min_depth=8, max_depth=31, device_sink=2, chunk_bytes=20_000, host_hold_bytes=len(text),
                     **FLAGSETS[fs][2])
    eng.source_text(text)
    st = eng.ingest()
    eng.estimate()
    _, st2 = eng.emit()
    got = eng.records_bytes(st.chunks)
    eng.close()
    assert st.chunks >= 4 and st2.bytes_out == len(got) == len(want) - len(sid.HEADER) and sid.HEADER + got == want


@pytest.mark.parametrize("fs", ["local", "local_R", "lr", "bayes", "quality"])
def test_composition(sid, inputs, fs):
    name = "depthq" if fs == "quality" else "depth"
    bed = inputs.bed(name)
    # (a context of 2 around four depths in seven keeps nearly everything: one depth in seven there)
    bounds, narrow = (8, 31), (30, 30)
    for sel in (dict(select="het"), dict(select="hom"), dict(bed=bed), dict(variants=True)):
        check_cli(sid, inputs, fs, name, bounds, **sel)
        check_cli(sid, inputs, fs, name, narrow, context=2, **sel)
    check_cli(sid, inputs, fs, name, narrow, context=2)   # the bounds alone select under a context
    # ... all of them, and over tile and chunk edges
    check_cli(sid, inputs, fs, name, bounds, extra=["--chunk-bytes", "65536"], select="hom", bed=bed, variants=True)
    check_cli(sid, inputs, fs, name, narrow, extra=["--chunk-bytes", "65536"], select="het", bed=bed, context=2)
    check_engine(sid, inputs, fs, name, bounds, variants=True, chunk_bytes=20_000)
    check_engine(sid, inputs, fs, name, narrow, bed=bed, context=2, chunk_bytes=20_000)
    check_engine(sid, inputs, fs, name, narrow, context=2, chunk_bytes=20_000)


@pytest.mark.parametrize("fs", ["local", "lr", "quality"])
def test_composition_with_variants_on_the_four_bounds(sid, inputs, fs):
    name = "depthq" if fs == "quality" else "depth"
    for bounds in D.BOUNDS:
        check_cli(sid, inputs, fs, name, bounds, variants=True, mode="variants")
        check_engine(sid, inputs, fs, name, bounds, variants=True, mode="variants", chunk_bytes=20_000)


@pytest.mark.parametrize("fs", ["local", "lr", "quality"])
def test_the_window_rows_do_not_change(sid, inputs, fs):
    name = "depthq" if fs == "quality" else "depth"
    rows = {}
    for bounds, more in (((0, 0), {}), ((8, 31), {}), ((8, 31), dict(select="het")), ((30, 30), dict(context=2))):
        for cb in (0, 20_000):
            eng = sid.Engine(window=100, min_depth=bounds[0], max_depth=bounds[1], chunk_bytes=cb, **more,
                             **FLAGSETS[fs][2])
            eng.source_text(inputs.texts[name])
            out, st = eng.run()
            rows[(bounds, tuple(more), cb)] = eng.windows()
            eng.close()
            if bounds != (0, 0):
                want = expect(inputs, fs, name, bounds, more.get("select", "all"), None, more.get("context", 0))[1]
            else:
                want = inputs.ref(fs, name).stdout
            assert out == want and st.bytes_out == len(want) - len(sid.HEADER), (bounds, more, cb)
    first = rows[((0, 0), (), 0)]
    assert len(first) == 30 and sum(r[3] for r in first) == 3000 and all(r == first for r in rows.values())


def test_setter_contract(sid, inputs):
    text = inputs.texts["depth"]
    for fs in ("local", "lr"):
        eng = sid.Engine(chunk_bytes=20_000, **FLAGSETS[fs][2])
        for lo, hi in ((-1, 0), (0, -1), (9, 8), (D.DEPTH_MAX + 1, 0), (0, D.DEPTH_MAX + 1)):
            with pytest.raises(sid.SidError) as ei:
                eng.set_depth(lo, hi)
            assert ei.value.status == EINVAL
        # two runs with different bounds, then none: each its own expected output
        for bounds in ((8, 31), (31, 0), (0, 0), (30, 30)):
            eng.set_depth(*bounds)
            eng.source_text(text)
            out, st = eng.run()
            want = inputs.ref(fs, "depth").stdout if bounds == (0, 0) else expect(inputs, fs, "depth", bounds)[1]
            assert out == want and st.bytes_out == len(want) - len(sid.HEADER), (fs, bounds)
        # between a successful ingest and its emit: SID_ESTATE, and the run keeps its bounds
        eng.source_text(text)
        eng.ingest()
        with pytest.raises(sid.SidError) as ei:
            eng.set_depth(0, 0)
        assert ei.value.status == ESTATE
        eng.estimate()
        out, _ = eng.emit()
        assert out == expect(inputs, fs, "depth", (30, 30))[1]
        eng.set_depth(0, 29)   # ... and after the emit it is allowed again
        eng.source_text(text)
        assert eng.run()[0] == expect(inputs, fs, "depth", (0, 29))[1]
        eng.close()
    # under a context the bounds alone switch its route on and off
    eng = sid.Engine(chunk_bytes=20_000, context=2)
    for bounds in ((0, 0), (30, 30), (0, 0), (90, 90)):
        eng.set_depth(*bounds)
        eng.source_text(text)
        out, st = eng.run()
        want = inputs.ref("local", "depth").stdout if bounds == (0, 0) else \
            expect(inputs, "local", "depth", bounds, context=2)[1]
        assert out == want and st.bytes_out == len(want) - len(sid.HEADER), bounds
    eng.close()
    for kw in (dict(min_depth=-1), dict(max_depth=-1), dict(min_depth=9, max_depth=8), dict(min_depth=D.DEPTH_MAX + 1)):
        with pytest.raises(sid.SidError) as ei:
            sid.Engine(**kw)
        assert ei.value.status == EINVAL
        with pytest.raises(sid.SidError) as ei:
            sid.Context(0, **kw)
        assert ei.value.status == EINVAL


def test_cli_errors(sid, inputs):
    p = inputs.paths["depth"]
    for opt in ("--min-depth", "--max-depth"):
        for arg in ("262141", "-1", "x", "", "12a", "1e3", "0x10", "9999999"):
            a = run(sid.CLI_PATH, [opt, arg, p])
            assert a.returncode == 1 and a.stdout == b""
            assert a.stderr == b"sid: %s: expected 0..262140, got %s\n" % (opt.encode(), arg.encode())
    for args in (["--min-depth", "9", "--max-depth", "8"], ["--max-depth", "8", "--min-depth", "9"],
                 ["--min-depth", "1", "--min-depth", "262140", "--max-depth", "31"]):
        a = run(sid.CLI_PATH, args + [p])
        assert a.returncode == 1 and a.stdout == b"" and a.stderr == b"sid: --min-depth above --max-depth\n"
    # given twice, the last wins; a maximum of 0 is no maximum
    want = expect(inputs, "local", "depth", (8, 31))[1]
    a = run(sid.CLI_PATH, ["--min-depth", "90", "--max-depth", "3", "--min-depth", "8", "--max-depth", "31", p])
    assert a.returncode == 0 and a.stdout == want
    a = run(sid.CLI_PATH, ["--min-depth", "31", "--max-depth", "0", p])
    assert a.returncode == 0 and a.stdout == expect(inputs, "local", "depth", (31, 0))[1]
    assert b"depth" not in run(sid.CLI_PATH, ["-h"]).stdout
    s = run(sid.CLI_PATH, ["--stats", "--min-depth", "8", "--max-depth", "31", p])
    assert s.returncode == 0 and s.stdout == want
    assert json.loads(s.stderr.splitlines()[-1])["bytes_out"] == len(want) - len(sid.HEADER)


def test_host_parse(sid, inputs):
    for fs in FOUR:
        check_cli(sid, inputs, fs, "depth", (8, 31), extra=["--host-parse"])
    check_cli(sid, inputs, "local", "geom", (30, 0), extra=["--host-parse", "--devices", "2"])
    check_cli(sid, inputs, "local", "depth", (30, 30), extra=["--host-parse"], select="het", context=2)
    check_cli(sid, inputs, "local", "depth", (30, 30), extra=["--host-parse"], context=2)
    check_cli(sid, inputs, "local", "depth", (8, 31), extra=["--host-parse"], variants=True)


def test_malformed_line_late_in_the_input(sid, inputs):
    b = inputs.ref("local", "bad_late")
    assert b.returncode != 0 and b.stdout == b""
    for extra in ([], ["--chunk-bytes", "65536"], ["--chunk-bytes", "65536", "--hold-bytes", "1"], ["--host-parse"]):
        a = run(sid.CLI_PATH, extra + ["--min-depth", "8", "--max-depth", "31", inputs.paths["bad_late"]])
        assert a.returncode == b.returncode, (extra, a.returncode, b.returncode)
        assert a.stdout == b""
        assert a.stderr == b.stderr


def test_resident_shard(sid, gpu, inputs):
    """sid_dtext_format on a Context with the bounds: -m local and -R -m likelihood_ratio, a range, a context,
    and the bounds set and taken back on the context."""
    import torch
    text = inputs.texts["depth"]
    for fs in ("local", "lr"):
        ctx = sid.Context(0, min_depth=8, max_depth=31, **FLAGSETS[fs][2])
        t = sid.DText(ctx, text)
        n = len(t)
        _, dcode, dhom, dhet = gpu.device_buffers(n)
        if fs == "local":
            ctx.call_local(t.counts_ptr, n, dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr())
        else:
            ctx.profile_reset(None)
            ctx.profile_accumulate(t.counts_ptr, n, None)
            ctx.lynch_prepare(False)
            ctx.lookup_sites(t.counts_ptr, n, dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr(), None)
        torch.cuda.synchronize()
        fmt = lambda *r: t.format(dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr(), "p_value", *r)
        assert sid.HEADER + fmt() == expect(inputs, fs, "depth", (8, 31))[1], fs
        if fs == "local":   # a range: sites [1000, 2500) (every line prints a record)
            b, lines, depths, _ = inputs.lines(fs, "depth")
            assert fmt(1000, 2500) == b"".join(ln for ln, d in zip(lines[1001:2501], depths[1000:2500])
                                               if D.inside(d, 8, 31))
        ctx.set_depth(31, 0)
        assert sid.HEADER + fmt() == expect(inputs, fs, "depth", (31, 0))[1], fs
        ctx.set_depth(0, 0)
        assert sid.HEADER + fmt() == inputs.ref(fs, "depth").stdout, fs
        t.close()
        ctx.close()
    ctx = sid.Context(0, method="local", context=2, min_depth=30, max_depth=30)
    t = sid.DText(ctx, text)
    n = len(t)
    _, dcode, dhom, dhet = gpu.device_buffers(n)
    ctx.call_local(t.counts_ptr, n, dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr())
    torch.cuda.synchronize()
    assert sid.HEADER + t.format(dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr(), "p_value") == \
        expect(inputs, "local", "depth", (30, 30), context=2)[1]
    t.close()
    ctx.close()


def test_without_the_bounds_nothing_changes(sid, inputs):
    for fs in ("local", "lr"):
        b = inputs.ref(fs, "depth")
        eng = sid.Engine(min_depth=0, max_depth=0, chunk_bytes=20_000, **FLAGSETS[fs][2])
        eng.source_text(inputs.texts["depth"])
        out, st = eng.run()
        eng.close()
        assert out == b.stdout and st.bytes_out == len(b.stdout) - len(sid.HEADER)
