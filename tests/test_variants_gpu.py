"""--variants (sid_opts.variants) on the device: through build/sid and through
sid_amd.Engine, every parser that keeps the reference byte (the tile parse's
lane and quad shapes, its general routine, the two-pass path), every formatter
family and every record path of the engine.

The expected stdout is always the oracle CLI's unselected stdout for the same
flags and input, filtered in Python by tests/variants_ref.py (the rule restated
from the pileup text: the third token, the counts by oracle.read_bases, which
lines print a record), and with a selection by label, region or a context also
by context_ref / regions_ref.  stderr and the exit status are the oracle's own.
Every case asserts that its expected output keeps at least one hom and one het
record and drops at least one of each -- a filter that is secretly `--only het`
cannot pass -- but for the header-only and keep-everything cases, which assert
exactly that."""
import json

import numpy as np
import pytest

import bgzf_ref
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
PLACEMENTS = ["none", "every", "second", "61st", "runs70", "last100"]


def tail(mapq=False) -> bytes:
    """Every kind of record (kept and dropped, hom and het) behind a text of one kind of line."""
    return V.base_text(1500, chrom=lambda i: b"chrB", mapq=mapq)


def geometry_text() -> bytes:
    hom = lambda c, p, r=b"A": V.vline(c, p, r, V.bases_of("homref", r))
    var = lambda c, p, k, r=b"A": V.vline(c, p, r, V.bases_of(k, r))
    parts = []
    # the first tile's slots: variants at lanes 0, 63 and 64 of its first wave of slots, and 127 / 128
    parts += [var(b"chr1", i + 1, "homalt" if i % 2 else "hetref") if i in (0, 63, 64, 127, 128) else hom(b"chr1", i + 1)
              for i in range(400)]
    # a chrom change every 37 sites, names of 4, 8, 9 and 12 bytes: compact words against header pairs
    names = [b"chrA", b"chrom_12", b"chrom_123", b"chromosome12"]
    parts.append(V.base_text(1200, chrom=lambda i: names[i // 37 % 4]))
    # position gaps over 127 (past a compact word's offset) and over 10^6
    pos = 1
    for i in range(600):
        pos += 1 if i % 5 else (130 if i % 10 else 1_000_003)
        parts.append(var(b"chrG", pos, "homalt", b"c") if i % 7 == 0 else hom(b"chrG", pos, b"c"))
    # a 70-byte name: a 512-slot group's records pass the writers' LDS buffer
    parts += [var(b"N" * 70, i, "hetalt", b"T") if i % 2 else hom(b"N" * 70, i, b"T") for i in range(1, 701)]
    # zero-padded positions: the formatter's tokeniser
    parts += [var(b"chrZ", b"%05d" % i, "homalt", b"g") if i % 4 == 0 else hom(b"chrZ", b"%05d" % i, b"g")
              for i in range(1, 81)]
    return b"".join(parts) + tail()


def refs_text() -> bytes:
    parts = []
    # 30 explicit G under references that are no base: hom,GG, which must be dropped
    for k, r in enumerate([b"N", b"n", b"R", b"*", b"A", b"a"]):
        parts += [V.vline(b"chrR%d" % k, i, r, b"G" * 30) for i in range(1, 41)]
    # depth 0 and all-'*' lines on A, C and G: "hom,TT" without a counted base
    for r in (b"A", b"C", b"G", b"T"):
        parts += [b"chr0\t%d\t%s\t0\t*\t*\n" % (i, r) for i in range(1, 31)]
        parts += [V.vline(b"chrS", i, r, b"*" * 12) for i in range(1, 31)]
    # lower-case references, every kind of site
    parts.append(V.base_text(900, chrom=lambda i: b"chrL").replace(b"\tA\t", b"\ta\t").replace(b"\tG\t", b"\tg\t"))
    return b"".join(parts) + tail()


def parsers_text() -> bytes:
    rng = np.random.default_rng(64)
    parts = []
    # '+2AC' indels and '^]' carets on variant lines: the general routine
    for i in range(1, 401):
        r = b"ACGT"[i % 4:i % 4 + 1]
        b = V.bases_of(V.KINDS[i % 3] if i % 2 else "homref", r)
        if i % 3 == 0:
            b = b[:10] + b"+2AC" + b[10:]
        elif i % 3 == 1:
            b = b"^]" + b[:20] + b"^]" + b[20:]
        parts.append(V.vline(b"chr7", i, r, b))
    # four alleles in numbers at 40x: no class table covers them (the fix-up)
    for i in range(1, 401):
        k = rng.integers(1, 4, 4) * 5 + rng.integers(0, 3, 4)
        bases = bytearray(b"A" * int(k[0]) + b"c" * int(k[1]) + b"G" * int(k[2]) + b"t" * int(k[3]))
        rng.shuffle(bases)
        parts.append(V.vline(b"chr3", i, b"ACGTN"[i % 5:i % 5 + 1], bytes(bases)))
    return b"".join(parts) + tail()


def tiny_text() -> bytes:
    """12-byte lines, more a tile than any slot list: the tile parse overflows into the two-pass path."""
    t = b"".join(b"c\t%d\t%s\t1\t%s\tI\n" % (i % 10, b"ACGN"[i % 4:i % 4 + 1], b"G." [i % 2:i % 2 + 1])
                 for i in range(1, 30_000))
    return t + tail()


class VInputs:
    """The test inputs as files, the oracle's run of each (flag set, input) and its filter, computed once."""

    def __init__(self, sid, oracle, d):
        self.sid, self.oracle, self.dir = sid, oracle, d
        good = V.base_text(3000)
        texts = {"base": V.base_text(), "baseq": V.base_text(mapq=True), "geom": geometry_text(), "refs": refs_text(),
                 "parsers": parsers_text(), "tiny": tiny_text(),
                 "deep": V.base_text(2500, depth=200),   # 200x: the quad shape from the second chunk on
                 "bad_late": good + good + b"chr1\t1\tAC\t3\t...\tIII\n" + V.base_text(50)}
        for k in PLACEMENTS:
            texts[k] = V.placement_text(k)
        self.texts, self.paths = texts, {}
        for k, t in texts.items():
            p = d / f"{k}.plp"
            p.write_bytes(t)
            self.paths[k] = str(p)
        self._ref, self._var, self._beds = {}, {}, {}

    def ref(self, fs, name):
        if (fs, name) not in self._ref:
            self._ref[(fs, name)] = self.oracle.run_cli(FLAGSETS[fs][0] + [self.paths[name]])
        return self._ref[(fs, name)]

    def lines_flags(self, fs, name):
        """(the oracle's run, its record lines, one bool a record: a variant)."""
        if (fs, name) not in self._var:
            b = self.ref(fs, name)
            assert b.returncode == 0, b.stderr[-300:]
            lines = b.stdout.splitlines(keepends=True)
            self._var[(fs, name)] = (b, lines, V.flags(lines[1:], self.texts[name], FLAGSETS[fs][1]))
        return self._var[(fs, name)]

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
    return VInputs(sid, oracle, tmp_path_factory.mktemp("variants"))


def expect(inputs, fs, name, select="all", bed=None, context=0, mode="some"):
    """The oracle's run and its stdout filtered: the variants, and the other selections with them; asserts
    that the case is not vacuous."""
    b, lines, var = inputs.lines_flags(fs, name)
    recs = lines[1:]
    sel = [v and s for v, s in zip(var, selected(recs, select, bed[1] if bed else None))]
    keep = dilate(sel, context) if context else sel
    want = lines[0] + b"".join(ln for ln, k in zip(recs, keep) if k)
    lab = [V.record_fields(ln)[2] for ln in recs]
    n = {(k, x): sum(1 for kk, ll in zip(keep, lab) if kk == k and ll == x) for k in (True, False) for x in (b"hom", b"het")}
    if mode == "header":
        assert not any(keep) and len(recs) > 0 and want == lines[0]
    elif mode == "all":
        assert all(keep) and n[(True, b"hom")] >= 1 and n[(True, b"het")] >= 1 and want == b.stdout
    elif select == "all":
        assert min(n.values()) >= 1, (fs, name, n)
    else:   # with --only: the label's records kept and dropped, the other label's all dropped
        x, y = select.encode(), (b"hom" if select == "het" else b"het")
        assert n[(True, x)] >= 1 and n[(False, x)] >= 1 and n[(False, y)] >= 1 and (context or n[(True, y)] == 0), (fs, name, n)
    if context:
        assert sum(keep) > sum(sel) >= 1   # (context records)
    return b, want


def cli_args(inputs, fs, name, select, bed, context):
    return (["--variants"] + ([] if select == "all" else ["--only", select]) + (["--regions", bed[0]] if bed else []) +
            (["--context", str(context)] if context else []) + FLAGSETS[fs][0] + [inputs.paths[name]])


def check_cli(sid, inputs, fs, name, extra=(), select="all", bed=None, context=0, mode="some"):
    b, want = expect(inputs, fs, name, select, bed, context, mode)
    a = run(sid.CLI_PATH, list(extra) + cli_args(inputs, fs, name, select, bed, context))
    assert a.returncode == 0, (a.returncode, a.stderr[-400:])
    assert a.stdout == want, (fs, name, extra, select, context)
    assert a.stderr == b.stderr
    return a


def check_engine(sid, inputs, fs, name, select="all", bed=None, context=0, mode="some", source="text", **kw):
    b, want = expect(inputs, fs, name, select, bed, context, mode)
    rg = sid.Regions(bed[2]) if bed else None
    eng = sid.Engine(variants=1, regions=rg, select=select, context=context, **FLAGSETS[fs][2], **kw)
    if rg:
        rg.close()
    if source == "bgzf":
        eng.source_bgzf(bgzf_ref.write(inputs.texts[name], payload=20_000)[0])
    else:
        eng.source_text(inputs.texts[name])
    out, st = eng.run()
    eng.close()
    assert out == want, (fs, name, select, context, kw)
    assert st.bytes_out == len(want) - len(sid.HEADER)
    return st


def test_the_base_input_is_the_issue_s(inputs):
    """The kept and dropped records of the base input by flag set, as the issue tabulates them."""
    for fs, want in (("local", (175, 176, 5638, 11)), ("local_R", (175, 176, 5638, 11)), ("lr", (87, 176, 4917, 11)),
                     ("bayes", (87, 176, 4917, 11))):
        b = inputs.ref(fs, "base")
        assert b.returncode == 0
        assert V.filter_csv(b.stdout, inputs.texts["base"], FLAGSETS[fs][1])[1:] == want
    lines = {V.record_fields(ln)[:2]: ln for ln in inputs.ref("local", "base").stdout.splitlines()[1:]}
    assert lines[(b"chr1", 20)].startswith(b"chr1,20,hom,TT,1,1,")   # no counted base, on reference G
    assert (b"chr1", 82) in lines                                       # coverage 2: a record under -m local alone
    assert b"chr1,82," not in inputs.ref("lr", "base").stdout


@pytest.mark.parametrize("fs", sorted(FLAGSETS))
def test_flag_sets_cli_and_engine(sid, inputs, fs):
    name = "baseq" if fs == "quality" else "base"
    check_cli(sid, inputs, fs, name)
    check_cli(sid, inputs, fs, name, extra=["--chunk-bytes", "65536"])   # tile and chunk edges
    st = check_engine(sid, inputs, fs, name)
    if fs == "local":
        assert st.chunks == 1 and st.chunks_tiled == 1 and st.tile_overflows == 0
    st = check_engine(sid, inputs, fs, name, chunk_bytes=65536)
    assert st.chunks >= 5


@pytest.mark.parametrize("kind", PLACEMENTS)
def test_placements(sid, inputs, kind):
    """Chunks and 512-slot groups without a variant, with only variants, and with a few."""
    mode = {"none": "header", "every": "all"}.get(kind, "some")
    for fs in FOUR:
        check_cli(sid, inputs, fs, kind, mode=mode)
    check_cli(sid, inputs, "local", kind, extra=["--chunk-bytes", "65536"], mode=mode)
    check_cli(sid, inputs, "lr", kind, extra=["--chunk-bytes", "65536", "--hold-bytes", "1"], mode=mode)
    st = check_engine(sid, inputs, "local", kind, mode=mode, chunk_bytes=100_000)
    if kind == "none":
        assert st.bytes_out == 0 and st.sites == 6000


@pytest.mark.parametrize("name", ["geom", "refs", "parsers"])
def test_geometry_reference_bytes_and_parsers(sid, inputs, name):
    for fs in FOUR:
        check_cli(sid, inputs, fs, name)
    for fs in ("local", "bayes"):
        check_cli(sid, inputs, fs, name, extra=["--chunk-bytes", "65536"])
        check_engine(sid, inputs, fs, name, chunk_bytes=20_000)


def test_reference_bytes_that_are_no_base_drop_their_hom_gg(inputs):
    """(the case's own premise: the oracle prints hom,GG on N, n, R and '*', and TT without a counted base)"""
    out = inputs.ref("local", "refs").stdout
    for k in range(4):
        assert b"chrR%d,7,hom,GG," % k in out
    assert b"chr0,7,hom,TT,1,1," in out and b"chrS,7,hom,TT,1,1," in out
    want = expect(inputs, "local", "refs")[1]
    assert b"chrR0," not in want and b"chrR3," not in want and b"chr0," not in want and b"chrS," not in want
    assert b"chrR4,7,hom,GG," in want and b"chrR5,7,hom,GG," in want   # ... and on A and a it is a variant


def test_quad_shape_and_tile_overflow(sid, inputs):
    for fs in ("local", "lr"):
        st = check_engine(sid, inputs, fs, "deep", chunk_bytes=300_000)   # 200x lines: the quad shape from chunk 2 on
        assert st.chunks >= 3 and st.chunks_tiled >= 2
        check_cli(sid, inputs, fs, "deep", extra=["--chunk-bytes", "300000"])
    st = check_engine(sid, inputs, "local", "tiny", chunk_bytes=100_000)   # into the two-pass path
    assert st.tile_overflows > 0
    check_engine(sid, inputs, "bayes", "tiny", chunk_bytes=100_000)
    check_cli(sid, inputs, "local_R", "tiny")


@pytest.mark.parametrize("fs", ["local", "local_R", "lr", "bayes"])
def test_engine_routes(sid, inputs, fs):
    """Pass 2 from the kept parse and from text read again, two lanes, a BGZF source, the host arena."""
    st = check_engine(sid, inputs, fs, "base", chunk_bytes=65536, hold_bytes=1)
    assert st.chunks >= 5 and (fs == "local" or st.chunks_reloaded == 0)
    st = check_engine(sid, inputs, fs, "base", chunk_bytes=65536, hold_bytes=1, retain_bytes=1)
    assert st.chunks_reloaded == st.chunks
    check_engine(sid, inputs, fs, "base", chunk_bytes=65536, lanes=2)
    check_engine(sid, inputs, fs, "base", chunk_bytes=65536, source="bgzf")
    check_engine(sid, inputs, fs, "base", chunk_bytes=65536, host_hold_bytes=3000)
    # the PCIe path without a writer: the expected records in the pinned host arena
    b, want = expect(inputs, fs, "base")
    text = inputs.texts["base"]
    eng = sid.Engine(variants=1, device_sink=2, chunk_bytes=100_000, host_hold_bytes=len(text), **FLAGSETS[fs][2])
    eng.source_text(text)
    st = eng.ingest()
    eng.estimate()
    _, st2 = eng.emit()
    got = eng.records_bytes(st.chunks)
    eng.close()
    assert st.chunks >= 4 and st2.bytes_out == len(got) and sid.HEADER + got == want


def test_host_parse(sid, inputs):
    for fs in FOUR:
        check_cli(sid, inputs, fs, "base", extra=["--host-parse"])
    check_cli(sid, inputs, "local", "refs", extra=["--host-parse", "--devices", "2"])
    check_cli(sid, inputs, "local", "base", extra=["--host-parse"], select="het", context=2)


def test_dtext_format(sid, gpu, inputs):
    """sid_dtext_format of a context with the option (the generic length / write kernels), a range included."""
    import torch
    text = inputs.texts["base"]
    for kw, sel, cx in ((dict(variants=1), "all", 0), (dict(variants=1, select="hom"), "hom", 0),
                        (dict(variants=1, context=2), "all", 2), (dict(variants=0), None, 0)):
        ctx = sid.Context(0, method="local", **kw)
        t = sid.DText(ctx, text)
        n = len(t)
        _, dcode, dhom, dhet = gpu.device_buffers(n)
        ctx.call_local(t.counts_ptr, n, dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr())
        torch.cuda.synchronize()
        want = inputs.ref("local", "base").stdout if sel is None else expect(inputs, "local", "base", sel, None, cx)[1]
        assert sid.HEADER + t.format(dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr(), "p_value") == want, kw
        if kw == dict(variants=1):   # a range: sites [1000, 5000)
            b, lines, var = inputs.lines_flags("local", "base")
            part = b"".join(ln for ln, k in zip(lines[1001:5001], var[1000:5000]) if k)
            assert t.format(dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr(), "p_value", 1000, 5000) == part
        t.close()
        ctx.close()


@pytest.mark.parametrize("fs", ["local", "local_R", "lr", "bayes", "quality"])
def test_composition(sid, inputs, fs):
    name = "baseq" if fs == "quality" else "base"
    bed = inputs.bed(name)
    for select in ("het", "hom"):
        check_cli(sid, inputs, fs, name, select=select)
    check_cli(sid, inputs, fs, name, bed=bed)
    check_cli(sid, inputs, fs, name, select="hom", bed=bed)
    check_cli(sid, inputs, fs, name, context=2)
    check_cli(sid, inputs, fs, name, select="het", bed=bed, context=2)
    # ... and over tile and chunk edges
    check_cli(sid, inputs, fs, name, extra=["--chunk-bytes", "65536"], select="hom", bed=bed)
    check_cli(sid, inputs, fs, name, extra=["--chunk-bytes", "65536"], select="het", bed=bed, context=2)
    check_engine(sid, inputs, fs, name, select="het", chunk_bytes=20_000)
    check_engine(sid, inputs, fs, name, bed=bed, context=2, chunk_bytes=20_000)


@pytest.mark.parametrize("fs", ["local", "lr", "quality"])
def test_the_window_rows_do_not_change(sid, inputs, fs):
    name = "baseq" if fs == "quality" else "base"
    rows = {}
    for variants, more in ((0, {}), (1, {}), (1, dict(select="het")), (1, dict(select="hom", context=2))):
        for cb in (0, 65536):
            eng = sid.Engine(window=100, variants=variants, chunk_bytes=cb, **more, **FLAGSETS[fs][2])
            eng.source_text(inputs.texts[name])
            out, st = eng.run()
            rows[(variants, tuple(more), cb)] = eng.windows()
            eng.close()
            if variants:
                want = expect(inputs, fs, name, more.get("select", "all"), None, more.get("context", 0))[1]
            else:
                want = inputs.ref(fs, name).stdout
            assert out == want and st.bytes_out == len(want) - len(sid.HEADER), (variants, more, cb)
    first = rows[(0, (), 0)]
    assert len(first) == 60 and sum(r[3] for r in first) == 6000 and all(r == first for r in rows.values())


def test_malformed_line_late_in_the_input(sid, inputs):
    b = inputs.ref("local", "bad_late")
    assert b.returncode != 0 and b.stdout == b""
    for extra in ([], ["--chunk-bytes", "65536"], ["--chunk-bytes", "65536", "--hold-bytes", "1"], ["--host-parse"]):
        a = run(sid.CLI_PATH, extra + ["--variants", inputs.paths["bad_late"]])
        assert a.returncode == b.returncode, (extra, a.returncode, b.returncode)
        assert a.stdout == b""
        assert a.stderr == b.stderr


def test_other_values_are_rejected(sid, inputs):
    for v in (2, -1):
        with pytest.raises(sid.SidError) as ei:
            sid.Engine(variants=v)
        assert ei.value.status == 1   # SID_EINVAL
        with pytest.raises(sid.SidError) as ei:
            sid.Context(0, variants=v)
        assert ei.value.status == 1
    with pytest.raises(sid.SidError) as ei:
        sid.Engine(select=3, variants=1)   # (--only keeps its three values)
    assert ei.value.status == 1
    a = run(sid.CLI_PATH, ["--variants=1", inputs.paths["base"]])   # the flag takes no argument
    assert a.returncode == 1 and a.stdout == b""


def test_without_the_option_nothing_changes(sid, inputs):
    """variants=0 is the run without the field, and --stats reports the selected bytes."""
    for fs in ("local", "lr"):
        b = inputs.ref(fs, "base")
        eng = sid.Engine(variants=0, chunk_bytes=65536, **FLAGSETS[fs][2])
        eng.source_text(inputs.texts["base"])
        out, st = eng.run()
        eng.close()
        assert out == b.stdout and st.bytes_out == len(b.stdout) - len(sid.HEADER)
    want = expect(inputs, "local", "base")[1]
    s = run(sid.CLI_PATH, ["--stats", "--variants", inputs.paths["base"]])
    assert s.returncode == 0 and s.stdout == want
    assert json.loads(s.stderr.splitlines()[-1])["bytes_out"] == len(want) - len(sid.HEADER)
