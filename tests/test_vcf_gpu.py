"""The VCF format (--vcf, sid_engine_set_format, sid_set_format) on the device:
through build/sid and through sid_amd.Engine, every parser (the tile parse's
lane and quad shapes, its general routine, the two-pass path), every formatter
family, every selection and every record path of the engine.

The expected stdout is always the oracle CLI's unselected stdout for the same
flags and input, mapped record by record by tests/vcf_ref.py (sid.h's "VCF"
paragraph restated from the pileup text and that CSV) and filtered by the
other *_ref modules as the selections' own tests filter the CSV.  stderr and
the exit status are the oracle's own.

Non-vacuity: every unselected case asserts that its expected output holds a
record each of 0/0, 0/1, 1/1, 1/2 and REF N, and of ./. where the flag set can
print one -- likelihood_ratio and bayes print no record below coverage 4, so a
record without a counted base does not exist there.  A selected case (--only
het holds no 0/0 by definition) asserts instead that records are kept and
dropped and that the kept ones hold a REF N or two genotypes."""
import json

import pytest

import bgzf_ref
import depth_ref as D
import vcf_ref as F
from context_ref import dilate, selected
from test_depth_gpu import FLAGSETS, FOUR, Inputs
from test_select_gpu import run

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = 7, 1


class VcfInputs(Inputs):
    def __init__(self, sid, oracle, d):
        super().__init__(sid, oracle, d)
        self._vcf = {}
        self.version = sid.lib().sid_version()

    def header(self, fs):
        return F.header(self.version, b"probability" if fs == "bayes" else b"p_value")

    def vcf(self, fs, name):
        """The oracle's records as VCF lines, one per record."""
        if (fs, name) not in self._vcf:
            b = self.lines(fs, name)[0]
            self._vcf[(fs, name)] = F.vcf_lines(b.stdout, self.texts[name], FLAGSETS[fs][1])[1]
        return self._vcf[(fs, name)]


@pytest.fixture(scope="module")
def inputs(sid, oracle, tmp_path_factory):
    return VcfInputs(sid, oracle, tmp_path_factory.mktemp("vcf"))


def expect(inputs, fs, name, select="all", bed=None, context=0, variants=False, bounds=(0, 0), mode="some"):
    """(the oracle's run, the expected stdout): the header and the VCF lines of the records the options keep."""
    b, lines, depths, var = inputs.lines(fs, name)
    recs, vcf = lines[1:], inputs.vcf(fs, name)
    assert len(recs) == len(vcf) > 0
    sel = [D.inside(d, *bounds) and s and (v or not variants)
           for d, s, v in zip(depths, selected(recs, select, bed[1] if bed else None), var)]
    keep = dilate(sel, context) if context else sel
    body = b"".join(v for v, k in zip(vcf, keep) if k)
    plain = select == "all" and not bed and not variants and bounds == (0, 0)
    g, refn = F.kinds(body)
    if mode == "header":
        assert not any(keep)
    elif plain:
        assert all(keep)
        assert (F.ALL_KINDS - ({b"./."} if FLAGSETS[fs][1] else set())) <= g and refn, (fs, name, sorted(g), refn)
    else:
        assert 0 < sum(keep) < len(keep) and (refn or len(g) >= 2), (fs, name, sorted(g), refn)
        if context:
            assert sum(keep) > sum(sel) >= 1
    return b, inputs.header(fs) + body


def cli_args(inputs, fs, name, select="all", bed=None, context=0, variants=False, bounds=(0, 0)):
    return (["--vcf"] + (["--min-depth", str(bounds[0]), "--max-depth", str(bounds[1])] if bounds != (0, 0) else []) +
            (["--variants"] if variants else []) + ([] if select == "all" else ["--only", select]) +
            (["--regions", bed[0]] if bed else []) + (["--context", str(context)] if context else []) +
            FLAGSETS[fs][0] + [inputs.paths[name]])


def check_cli(sid, inputs, fs, name, extra=(), mode="some", **sel):
    b, want = expect(inputs, fs, name, mode=mode, **sel)
    a = run(sid.CLI_PATH, list(extra) + cli_args(inputs, fs, name, **sel))
    assert a.returncode == 0, (a.returncode, a.stderr[-400:])
    assert a.stdout == want, (fs, name, extra, sel)
    assert a.stderr == b.stderr
    return a


def check_engine(sid, inputs, fs, name, select="all", bed=None, context=0, variants=False, bounds=(0, 0), mode="some",
                 source="text", **kw):
    b, want = expect(inputs, fs, name, select, bed, context, variants, bounds, mode)
    rg = sid.Regions(bed[2]) if bed else None
    eng = sid.Engine(format="vcf", min_depth=bounds[0], max_depth=bounds[1], variants=int(variants), regions=rg,
                     select=select, context=context, **FLAGSETS[fs][2], **kw)
    if rg:
        rg.close()
    if source == "bgzf":
        eng.source_bgzf(bgzf_ref.write(inputs.texts[name], payload=20_000)[0])
    else:
        eng.source_text(inputs.texts[name])
    out, st = eng.run(header=inputs.header(fs))
    eng.close()
    assert out == want, (fs, name, select, context, variants, bounds, kw)
    assert st.bytes_out == len(want) - len(inputs.header(fs))
    return st


@pytest.mark.parametrize("fs", sorted(FLAGSETS))
def test_flag_sets_cli_and_engine(sid, inputs, fs):
    name = "depthq" if fs == "quality" else "depth"
    check_cli(sid, inputs, fs, name)
    check_cli(sid, inputs, fs, name, extra=["--chunk-bytes", "65536"])   # tile and chunk edges
    st = check_engine(sid, inputs, fs, name, chunk_bytes=20_000)
    assert st.chunks >= 5


@pytest.mark.parametrize("fs", ["local", "lr", "quality"])
def test_deep_text_the_quad_shape_and_the_second_table(sid, inputs, fs):
    name = "deepq" if fs == "quality" else "deep"
    st = check_engine(sid, inputs, fs, name, chunk_bytes=300_000)
    assert st.chunks >= 2 and (st.chunks_tiled > 0) == (fs != "quality")
    check_cli(sid, inputs, fs, name, extra=["--chunk-bytes", "300000"])


def test_two_pass_path_after_a_tile_overflow(sid, inputs):
    st = check_engine(sid, inputs, "local", "tiny", chunk_bytes=100_000)
    assert st.tile_overflows > 0
    check_engine(sid, inputs, "bayes", "tiny", chunk_bytes=100_000)
    check_cli(sid, inputs, "local_R", "tiny")


@pytest.mark.parametrize("name", ["parsers", "geom"])
def test_general_routine_fix_up_and_geometry(sid, inputs, name):
    for fs in FOUR:
        check_cli(sid, inputs, fs, name)
    for fs in ("local", "lr"):
        check_cli(sid, inputs, fs, name, extra=["--chunk-bytes", "65536"])
        check_engine(sid, inputs, fs, name, chunk_bytes=20_000)


def test_geometry_s_premises_and_its_empty_groups(sid, inputs):
    want = expect(inputs, "local", "geom")[1]
    assert want.count(b"N" * 70 + b"\t") == 700   # the 70-byte chrom: groups past the writer's LDS buffer
    for c in (b"chrA", b"chrom_12", b"chrom_123", b"chromosome12"):
        assert b"\n" + c + b"\t" in want
    # a selection that empties whole 512-slot groups (600 consecutive sites at depth 4) and the first tile's slots
    for fs in ("local", "lr"):
        check_cli(sid, inputs, fs, "geom", bounds=(8, 31))
        check_engine(sid, inputs, fs, "geom", bounds=(8, 31), chunk_bytes=20_000)


@pytest.mark.parametrize("fs", ["local", "local_R", "lr", "bayes", "quality"])
def test_selections(sid, inputs, fs):
    name = "depthq" if fs == "quality" else "depth"
    bed = inputs.bed(name)
    for sel in (dict(select="het"), dict(select="hom"), dict(bed=bed), dict(variants=True), dict(bounds=(8, 31))):
        check_cli(sid, inputs, fs, name, **sel)
    check_cli(sid, inputs, fs, name, extra=["--chunk-bytes", "65536"], select="het", bed=bed, variants=True,
              bounds=(8, 0))
    # grep -C 2 over at least three chunks
    assert len(inputs.texts[name]) > 3 * 65536
    check_cli(sid, inputs, fs, name, extra=["--chunk-bytes", "65536"], select="het", context=2)
    st = check_engine(sid, inputs, fs, name, select="het", context=2, chunk_bytes=20_000)
    assert st.chunks >= 3
    check_engine(sid, inputs, fs, name, select="hom", bed=bed, bounds=(30, 30), context=2, chunk_bytes=20_000)


@pytest.mark.parametrize("fs", FOUR)
def test_engine_record_paths(sid, inputs, fs):
    """Pass 2 from the kept parse and from text read again, lanes, devices, a BGZF source, a host arena too
    small for the run, and the three sink modes' bytes_out."""
    import torch
    st = check_engine(sid, inputs, fs, "depth", chunk_bytes=20_000, hold_bytes=1)
    assert st.chunks >= 5 and (fs == "local" or st.chunks_reloaded == 0)
    st = check_engine(sid, inputs, fs, "depth", chunk_bytes=20_000, hold_bytes=1, retain_bytes=1)
    assert st.chunks_reloaded == st.chunks
    check_engine(sid, inputs, fs, "depth", chunk_bytes=20_000, lanes=2)
    if torch.cuda.device_count() >= 2:
        check_engine(sid, inputs, fs, "depth", chunk_bytes=20_000, devices=2)
    check_engine(sid, inputs, fs, "depth", chunk_bytes=20_000, source="bgzf")
    # the arena holds a few chunks' lines: the others take the HBM hold, and nothing is lost
    check_engine(sid, inputs, fs, "depth", chunk_bytes=20_000, host_hold_bytes=30_000)
    b, want = expect(inputs, fs, "depth")
    head = inputs.header(fs)
    text = inputs.texts["depth"]
    for sink, hh in ((1, 0), (2, 2 * len(text)), (2, 30_000)):
        eng = sid.Engine(format="vcf", device_sink=sink, chunk_bytes=20_000, host_hold_bytes=hh, **FLAGSETS[fs][2])
        eng.source_text(text)
        st = eng.ingest()
        eng.estimate()
        out, st2 = eng.emit(header=head)
        assert st.chunks >= 4 and st2.bytes_out == len(want) - len(head), (fs, sink, hh)
        if sink == 2 and hh > 30_000:   # the PCIe path without a writer: the lines in the pinned host arena
            assert head + eng.records_bytes(st.chunks) == want
        eng.close()


def test_the_cli_s_host_arena_and_stats(sid, inputs):
    """--host-hold too small for the VCF lines: chunks beyond it fall back to the HBM hold; bytes_out is exact."""
    b, want = expect(inputs, "local", "depth")
    a = run(sid.CLI_PATH, ["--vcf", "--stats", "--chunk-bytes", "65536", "--host-hold", "40000", inputs.paths["depth"]])
    assert a.returncode == 0 and a.stdout == want
    assert json.loads(a.stderr.splitlines()[-1])["bytes_out"] == len(want) - len(inputs.header("local"))
    assert b"vcf" not in run(sid.CLI_PATH, ["-h"]).stdout


@pytest.mark.parametrize("fs", ["local", "lr", "quality"])
def test_the_window_rows_do_not_change(sid, inputs, fs):
    name = "depthq" if fs == "quality" else "depth"
    rows = {}
    for fmt in ("csv", "vcf"):
        for more in ({}, dict(select="het")):
            eng = sid.Engine(window=100, format=fmt, chunk_bytes=20_000, **more, **FLAGSETS[fs][2])
            eng.source_text(inputs.texts[name])
            out, st = eng.run(header=inputs.header(fs) if fmt == "vcf" else sid.HEADER)
            rows[(fmt, tuple(more))] = eng.windows()
            eng.close()
            if fmt == "vcf":
                assert out == expect(inputs, fs, name, **more)[1]
    first = rows[("csv", ())]
    assert len(first) == 30 and sum(r[3] for r in first) == 3000 and all(r == first for r in rows.values())


def test_malformed_line_late_in_the_input(sid, inputs):
    b = inputs.ref("local", "bad_late")
    assert b.returncode != 0 and b.stdout == b""
    for extra in ([], ["--chunk-bytes", "65536"], ["--chunk-bytes", "65536", "--hold-bytes", "1"], ["--host-parse"]):
        a = run(sid.CLI_PATH, extra + ["--vcf", inputs.paths["bad_late"]])
        assert a.returncode == b.returncode, (extra, a.returncode, b.returncode)
        assert a.stdout == b""
        assert a.stderr == b.stderr


def test_header_alone(sid, oracle, inputs):
    """An unknown -m prints the header alone -- now the VCF header; so does a selection that keeps nothing."""
    b = oracle.run_cli(["-m", "nonsense", inputs.paths["depth"]])
    a = run(sid.CLI_PATH, ["--vcf", "-m", "nonsense", inputs.paths["depth"]])
    assert a.returncode == b.returncode == 0 and a.stderr == b.stderr
    assert a.stdout == inputs.header("local") and b.stdout.count(b"\n") == 1
    for fs in FOUR:
        a = check_cli(sid, inputs, fs, "depth", bounds=(91, 0), mode="header")
        assert a.stdout == inputs.header(fs)
    st = check_engine(sid, inputs, "local", "depth", bounds=(91, 0), mode="header", chunk_bytes=20_000)
    assert st.bytes_out == 0 and st.sites == 3000


def test_host_parse(sid, inputs):
    for fs in FOUR:
        check_cli(sid, inputs, fs, "depth", extra=["--host-parse"])
    check_cli(sid, inputs, "local", "geom", extra=["--host-parse", "--devices", "2"])
    check_cli(sid, inputs, "local", "depth", extra=["--host-parse"], select="het", context=2)
    check_cli(sid, inputs, "lr", "depth", extra=["--host-parse"], variants=True, bounds=(8, 31))


def test_setter_contract(sid, inputs):
    text = inputs.texts["depth"]
    for fs in ("local", "lr"):
        head = inputs.header(fs)
        eng = sid.Engine(chunk_bytes=20_000, **FLAGSETS[fs][2])
        for v in (-1, 2, 7, 1 << 20):
            with pytest.raises(sid.SidError) as ei:
                eng.set_format(v)
            assert ei.value.status == EINVAL
        # the same engine: CSV, VCF, CSV again -- each run its own expected output
        for fmt in ("csv", "vcf", "csv", "vcf"):
            eng.set_format(fmt)
            eng.source_text(text)
            out, st = eng.run(header=head if fmt == "vcf" else sid.HEADER)
            want = expect(inputs, fs, "depth")[1] if fmt == "vcf" else inputs.ref(fs, "depth").stdout
            assert out == want and st.bytes_out == len(want) - len(head if fmt == "vcf" else sid.HEADER), (fs, fmt)
        # between a successful ingest and its emit: SID_ESTATE, and the run keeps its format
        eng.source_text(text)
        eng.ingest()
        with pytest.raises(sid.SidError) as ei:
            eng.set_format("csv")
        assert ei.value.status == ESTATE
        eng.estimate()
        out, _ = eng.emit(header=head)
        assert out == expect(inputs, fs, "depth")[1]
        eng.set_format("csv")   # ... and after the emit it is allowed again
        eng.source_text(text)
        assert eng.run()[0] == inputs.ref(fs, "depth").stdout
        eng.close()
    ctx = sid.Context(0)
    for v in (-1, 2):
        with pytest.raises(sid.SidError) as ei:
            ctx.set_format(v)
        assert ei.value.status == EINVAL
    ctx.close()


def test_resident_shard(sid, gpu, inputs):
    """sid_dtext_format honours the context's format: -m local and -R -m likelihood_ratio, a range, a
    selection, and the format set and taken back on the context."""
    import torch
    text = inputs.texts["depth"]
    for fs in ("local", "lr"):
        head = inputs.header(fs)
        ctx = sid.Context(0, format="vcf", **FLAGSETS[fs][2])
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
        assert head + fmt() == expect(inputs, fs, "depth")[1], fs
        if fs == "local":   # a range: sites [1000, 2500) (every line prints a record)
            assert fmt(1000, 2500) == b"".join(inputs.vcf(fs, "depth")[1000:2500])
        ctx.set_depth(8, 31)
        assert head + fmt() == expect(inputs, fs, "depth", bounds=(8, 31))[1], fs
        ctx.set_depth(0, 0)
        ctx.set_format("csv")
        assert sid.HEADER + fmt() == inputs.ref(fs, "depth").stdout, fs
        t.close()
        ctx.close()


def test_without_the_option_nothing_changes(sid, inputs):
    for fs in ("local", "lr"):
        b = inputs.ref(fs, "depth")
        eng = sid.Engine(format="csv", chunk_bytes=20_000, **FLAGSETS[fs][2])
        eng.source_text(inputs.texts["depth"])
        out, st = eng.run()
        eng.close()
        assert out == b.stdout and st.bytes_out == len(b.stdout) - len(sid.HEADER)
