"""--region-stats FILE (sid_engine_set_region_stats) on the device: through
sid_amd.Engine, sid_dtext_region_stats and build/sid, every formatter family,
the wave shapes of the stage (one interval over everything, 64 intervals a
wave, two alternating, an edge at every lane offset, the chrom search's two
branches, two rounds of the wave search), every chunk layout and source, the
selections, and the errors.

The expected rows are always the Python model's (tests/region_stats_ref.py)
over the host parser's per-site counts, the oracle's codes and the intervals of
Regions.interval.  Every engine case asserts that the records and bytes_out are
byte-equal to the same configuration's without the option and that the rows
equal the model's."""
import os

import pytest

import bgzf_ref
import depth_hist_ref as DH
import region_stats_ref as RS
import windows_ref as WR
from regions_ref import bed_runs, text_sites
from test_select_gpu import BASES, line, run
from test_windows import quirks_text
from test_windows_gpu import METHODS, low_cov_text

pytestmark = pytest.mark.gpu


def ones_text(n=5000) -> bytes:
    """Sites at the even positions 2 .. 2n: under ones_bed every site has an interval of its own."""
    return b"".join(line(b"chrO", 2 * i, i % 7 == 0) for i in range(1, n + 1))


def ones_bed(n=5000) -> bytes:
    """n one-base intervals (2i - 1, 2i) on one chrom -- more than 4,096, two rounds of the wave search; they do
    not abut, so the merge keeps them apart."""
    return b"".join(b"chrO\t%d\t%d\n" % (2 * i - 1, 2 * i) for i in range(1, n + 1))


def long_line(chrom: bytes, pos: int, k: int) -> bytes:
    b = b"^I" * k + BASES
    return b"%s\t%d\tA\t30\t%s\t%s\n" % (chrom, pos, b, b"I" * 30)


class RInputs:
    def __init__(self, sid, oracle, d):
        self.sid, self.oracle, self.dir = sid, oracle, d
        mix = sid.synth_text(81, 2100, 30.0, sites_per_chrom=700) + quirks_text() + sid.synth_text(82, 2000, 30.0, sites_per_chrom=700)
        many = [b"c%02d_%s" % (k, b"x" * (k % 11)) for k in range(70)]   # 70 chroms, names of 4 to 14 bytes
        back = (b"".join(line(b"chr1", i, i % 9 == 0) for i in range(1, 3001)) +
                b"".join(line(b"chr2", i, i % 5 == 0) for i in range(1, 2001)) +
                b"".join(line(b"chr1", i, i % 4 == 0) for i in range(1, 3001)))
        self.texts = {
            "whole": b"".join(line(b"chr1", i, i % 61 == 0) for i in range(1, 40_001)),
            "ones": ones_text(),
            "alt": b"".join(line(b"chrA" if i % 2 else b"chromosome_B1", i, i % 6 == 0) for i in range(1, 8001)),
            "phase": b"".join(line(b"chr1", 100000 + i, i % 51 == 0) for i in range(6000)),
            "many": b"".join(line(many[(i // 13) % 70], i, i % 8 == 0) for i in range(1, 9101)),
            "mix": mix,
            "lowcov": low_cov_text() + b"".join(b"chr7\t%d\tA\t0\t*\t*\n" % i for i in range(1, 301)) +
                      sid.synth_text(83, 1500, 30.0, sites_per_chrom=700),
            "back": back,
            "deep": sid.synth_text(5, 1500, 200.0, sites_per_chrom=700) +
                    b"".join(line(b"chrD", i, False, b"." * 100 + b"g" * 100 if i % 7 == 0 else b"." * 200)
                             for i in range(1, 701)),
            "long": (b"".join(line(b"chrG", 1 + i, i % 9 == 0) for i in range(2000)) + long_line(b"chrG", 2001, 30_000) +
                     b"".join(line(b"chrG", 2002 + i, i % 7 == 0) for i in range(600))),
            "quality": sid.synth_text(4, 3000, 30.0, sites_per_chrom=700, mapq=True),
        }
        good = b"".join(line(b"chr1", i, i % 61 == 0) for i in range(1, 4001))
        self.texts["bad_late"] = good + good + b"chr1\t1\tAC\t3\t...\tIII\n" + good[:3000]
        assert max(len(x) for x in self.texts["long"].splitlines()) < 61_000
        runs = lambda name: bed_runs(text_sites(self.texts[name]), lambda i: (i // 70) % 5 == 2)
        self.beds = {
            "whole": b"chr1\n",
            "ones": ones_bed(),
            "alt": b"chromosome_B1\nchrA\nchromosome_B2\t0\t9\n",
            # 36 positions inside, the 37th outside: an edge at every lane offset and across the groups' edges
            "phase": b"".join(b"chr1\t%d\t%d\n" % (99999 + 37 * k, 99999 + 37 * k + 36) for k in range(170)),
            "many": b"".join(b"%s\t%d\t%d\n" % (c, 100 * k, 100 * k + 60) for k in range(95) for c in many[k % 3::3]),
            "mix": b"chr2\t0\t2\nchromosome_A\nchr1\t36\t74\nchromosom\t2\t3\nchrZ\t2147483640\t2147483647\nabsent\t1\t5\n" + runs("mix"),
            "lowcov": b"chr7\nchr6\t0\t1500\nchr6\t1600\t1700\n" + runs("lowcov"),
            "back": b"chr2\t500\t1500\nchr1\t0\t1000\nchr1\t2000\t2500\n",
            "deep": b"chrD\t100\t600\n" + runs("deep"),
            "long": b"chrG\t1990\t2010\nchrG\t0\t50\nchrG\t2500\t9000\n",
            "quality": runs("quality"),
            "bad_late": b"chr1\n",
        }
        self.paths = {}
        for k, t in self.texts.items():
            p = d / f"{k}.plp"
            p.write_bytes(t)
            self.paths[k] = str(p)
            (d / f"{k}.bed").write_bytes(self.beds[k])
            self.paths[k + ".bed"] = str(d / f"{k}.bed")
        self._rows, self._plain = {}, {}

    def regions(self, name):
        return self.sid.Regions(self.beds[name])

    def rows(self, name, mkey="local"):
        """The model's rows once per (input, method)."""
        if (name, mkey) not in self._rows:
            kw = dict(METHODS[mkey][0])
            r = self.regions(name)
            self._rows[(name, mkey)] = RS.site_rows(self.sid, self.oracle, r, self.texts[name], kw.pop("method"), **kw)
            assert len(self._rows[(name, mkey)]) == len(r)
            r.close()
        return self._rows[(name, mkey)]

    def plain(self, name, mkey, **kw):
        """The engine's records of the same configuration (the set selecting) without the option, once each."""
        key = (name, mkey, tuple(sorted((k, repr(v)) for k, v in kw.items())))
        if key not in self._plain:
            r = self.regions(name)
            eng = self.sid.Engine(regions=r, **METHODS[mkey][0], **kw)
            r.close()
            eng.source_text(self.texts[name])
            out, st = eng.run(**self.header(mkey, kw))
            with pytest.raises(self.sid.SidError) as ei:   # the option off: no rows
                eng.region_stats()
            assert ei.value.status == 7
            eng.close()
            self._plain[key] = (out, st.bytes_out)
        return self._plain[key]

    def header(self, mkey, kw):
        if kw.get("format") != "vcf":
            return {}
        return dict(header=self.sid.vcf_header(**METHODS[mkey][0]))


@pytest.fixture(scope="module")
def inputs(sid, oracle, tmp_path_factory):
    return RInputs(sid, oracle, tmp_path_factory.mktemp("region_stats"))


def check_rows(inputs, name, mkey, rows):
    want = inputs.rows(name, mkey)
    assert rows == want, (name, mkey, len(rows), len(want), next(((a, b) for a, b in zip(rows, want) if a != b), None))


def check_engine(sid, inputs, name, mkey="local", source="text", **kw):
    out0, bytes0 = inputs.plain(name, mkey, **kw)
    r = inputs.regions(name)
    eng = sid.Engine(region_stats=True, regions=r, **METHODS[mkey][0], **kw)
    r.close()
    f = None
    if source == "text":
        eng.source_text(inputs.texts[name])
    elif source == "bgzf":
        eng.source_bgzf(bgzf_ref.write(inputs.texts[name], payload=20000)[0])
    elif source == "file":
        f = open(inputs.paths[name], "rb")
        eng.source_file(f.fileno())
    out, st = eng.run(**inputs.header(mkey, kw))
    rows = eng.region_stats()
    eng.close()
    if f:
        f.close()
    if not kw.get("device_sink"):
        assert out == out0, (name, mkey, source, kw)
    assert st.bytes_out == bytes0, (name, mkey, source, kw)
    check_rows(inputs, name, mkey, rows)
    if not kw.get("device_sink") and kw.get("format") != "vcf" and set(kw) <= {"chunk_bytes", "lanes", "devices"}:
        # the set is the only selection: the records and the het records are the rows' columns summed
        assert sum(x[5] for x in rows) == out.count(b"\n") - 1
        assert sum(x[6] for x in rows) == out.count(b",het,")
    return st, rows


@pytest.mark.parametrize("mkey", ["local", "local_R", "lr", "bayes", "quality"])
def test_methods(sid, inputs, mkey):
    """Every formatter family on the hand-made keys (inside `mix`), on sites without a record and on -m
    local's depth-0 placeholders."""
    if mkey == "quality":
        for cb in (0, 20_000):
            check_engine(sid, inputs, "quality", mkey, chunk_bytes=cb)
        return
    for cb in (0, 20_000):
        check_engine(sid, inputs, "mix", mkey, chunk_bytes=cb)
        st, rows = check_engine(sid, inputs, "lowcov", mkey, chunk_bytes=cb)
    by = {x[:3]: x for x in rows}
    star = by[(b"chr7", 0, 2 ** 31 - 1)]
    low = by[(b"chr6", 0, 1500)]
    if mkey in ("local", "local_R"):
        assert star[3:] == (300, 0, 300, 0, 300)   # '*' lines: a "hom,TT" record each, depth 0
        assert low[3] == low[5] == 1500
    else:
        assert star[3:] == (300, 0, 0, 0, 0)       # sites counted, no record
        assert low[3] == 1500 and low[5] == 1000   # coverage 2 at every third site: no Lynch record
    mix = {x[:3]: x for x in inputs.rows("mix", mkey)}
    assert mix[(b"absent", 1, 5)][3:] == (0, 0, 0, 0, 0) and mix[(b"chromosome_A", 0, 2 ** 31 - 1)][3] == 2
    assert mix[(b"chromosom", 2, 3)][3] == 2 and mix[(b"chrZ", 2147483640, 2 ** 31 - 1)][3] == 2


@pytest.mark.parametrize("mkey", ["local", "lr"])
def test_wave_shapes(sid, inputs, mkey):
    # one interval over every site: the carry, across many blocks and the groups a block walks
    for cb in (0, 1 << 19):
        st, rows = check_engine(sid, inputs, "whole", mkey, chunk_bytes=cb)
    assert len(rows) == 1 and rows[0][3] == 40_000 and rows[0][4] > 0
    # 64 one-base intervals a wave (the fallback), 5,000 on one chrom (two rounds of the wave search), and
    # chunks that touch more intervals than the pinned block holds
    for cb in (0, 65536):
        st, rows = check_engine(sid, inputs, "ones", mkey, chunk_bytes=cb)
    assert len(rows) == 5000 and all(x[3] == 1 for x in rows)
    # two intervals alternating lane by lane; the third interval never met
    st, rows = check_engine(sid, inputs, "alt", mkey, chunk_bytes=0)
    assert [x[3] for x in rows] == [4000, 4000, 0]
    # an interval edge at every lane offset and across a 512-slot group's edge, by runs of 36
    for cb in (0, 20_000):
        st, rows = check_engine(sid, inputs, "phase", mkey, chunk_bytes=cb)
    assert [x[3] for x in rows[:162]] == [36] * 162 and rows[162][3] == 6 and rows[163][3] == 0
    # more than 64 chroms: the other branch of the chrom search
    for cb in (0, 20_000):
        st, rows = check_engine(sid, inputs, "many", mkey, chunk_bytes=cb)
    assert len({x[0] for x in rows}) == 70 and len(rows) > 2000 and sum(x[3] for x in rows) > 1500


def test_chunks_and_layouts(sid, gpu, inputs):
    import torch
    got = []
    for cb in (0, 20_000, 1 << 19):
        st, rows = check_engine(sid, inputs, "mix", chunk_bytes=cb)
        got.append(rows)
    assert got[0] == got[1] == got[2]
    # unsorted input: positions return to an earlier interval in a later chunk
    st, rows = check_engine(sid, inputs, "back", chunk_bytes=20_000)
    assert st.chunks >= 10 and [x[:4] for x in rows] == [(b"chr2", 500, 1500, 1000), (b"chr1", 0, 1000, 2000),
                                                         (b"chr1", 2000, 2500, 1000)]
    check_engine(sid, inputs, "back", "lr", chunk_bytes=20_000)
    check_engine(sid, inputs, "mix", chunk_bytes=20_000, lanes=2)
    if torch.cuda.device_count() >= 2:
        check_engine(sid, inputs, "mix", "lr", chunk_bytes=20_000, devices=2)
    # 200x lines: the quad shape from chunk 2 on; one 60 KB line inside an interval: the long-line layout
    st, _ = check_engine(sid, inputs, "deep", chunk_bytes=300_000)
    assert st.chunks >= 3 and st.chunks_tiled >= 2
    check_engine(sid, inputs, "deep", "lr", chunk_bytes=300_000)
    for cb in (0, 100_000):
        st, rows = check_engine(sid, inputs, "long", chunk_bytes=cb)
    assert [x[:4] for x in rows] == [(b"chrG", 0, 50, 50), (b"chrG", 1990, 2010, 20), (b"chrG", 2500, 9000, 101)]
    # budgets: nothing formatted in pass 1, the text read again in pass 2 -- every chunk counts once
    for mkey in ("local", "lr"):
        check_engine(sid, inputs, "mix", mkey, chunk_bytes=20_000, hold_bytes=1, retain_bytes=1)


@pytest.mark.parametrize("mkey", ["local", "lr"])
def test_sources_and_sinks(sid, inputs, mkey):
    for source in ("file", "bgzf"):
        for cb in (0, 65536):
            check_engine(sid, inputs, "mix", mkey, source=source, chunk_bytes=cb)
    for sink, more in ((1, {}), (2, {"host_hold_bytes": 1 << 22})):
        check_engine(sid, inputs, "mix", mkey, chunk_bytes=20_000, device_sink=sink, **more)


@pytest.mark.parametrize("mkey", ["local", "lr"])
def test_independence_of_selections_and_format(sid, inputs, mkey):
    """--only, --variants, the depth bounds, --context and --vcf change the records, not the rows."""
    full = len(inputs.plain("mix", mkey, chunk_bytes=20_000)[0])
    for sel in (dict(select="het"), dict(variants=1), dict(min_depth=25, max_depth=32), dict(select="het", context=2),
                dict(select="het", variants=1, min_depth=20, context=2)):
        check_engine(sid, inputs, "mix", mkey, chunk_bytes=20_000, **sel)
        assert len(inputs.plain("mix", mkey, chunk_bytes=20_000, **sel)[0]) < full   # (the selection selects)
    check_engine(sid, inputs, "mix", mkey, chunk_bytes=20_000, format="vcf")
    check_engine(sid, inputs, "mix", mkey, chunk_bytes=0, format="vcf", select="het")


def test_state_and_reuse(sid, inputs):
    L = sid.lib()
    eng = sid.Engine(chunk_bytes=20_000)   # no region set
    assert L.sid_engine_set_region_stats(eng.h, 1) == 1 and L.sid_engine_set_region_stats(eng.h, 2) == 1
    eng.close()
    with pytest.raises(sid.SidError) as ei:
        sid.Engine(region_stats=True)
    assert ei.value.status == 1
    r = inputs.regions("mix")
    eng = sid.Engine(regions=r, chunk_bytes=20_000)
    r.close()
    assert L.sid_engine_set_region_stats(eng.h, -1) == 1
    eng.set_region_stats(True)
    with pytest.raises(sid.SidError) as ei:   # before a run
        eng.region_stats()
    assert ei.value.status == 7
    eng.source_text(inputs.texts["mix"])
    eng.ingest()
    assert L.sid_engine_set_region_stats(eng.h, 0) == 7 and L.sid_engine_set_region_stats(eng.h, 1) == 7   # SID_ESTATE
    with pytest.raises(sid.SidError):   # before the emit
        eng.region_stats()
    eng.estimate()
    out, st = eng.emit()
    assert out == inputs.plain("mix", "local", chunk_bytes=20_000)[0]
    check_rows(inputs, "mix", "local", eng.region_stats())
    # a second run on the engine starts from zero; another text under the same set; then off, and on again
    eng.source_text(inputs.texts["mix"])
    with pytest.raises(sid.SidError):   # a new source: the last run's rows are gone
        eng.region_stats()
    out, st = eng.run()
    check_rows(inputs, "mix", "local", eng.region_stats())
    eng.source_text(b"")
    out, st = eng.run()
    assert out == sid.HEADER and eng.region_stats() == [x[:3] + (0, 0, 0, 0, 0) for x in inputs.rows("mix")]
    eng.set_region_stats(False)
    eng.source_text(inputs.texts["mix"])
    out, st = eng.run()
    assert out == inputs.plain("mix", "local", chunk_bytes=20_000)[0]
    with pytest.raises(sid.SidError) as ei:   # the option off
        eng.region_stats()
    assert ei.value.status == 7
    eng.set_region_stats(True)
    eng.source_text(inputs.texts["mix"])
    out, st = eng.run()
    check_rows(inputs, "mix", "local", eng.region_stats())
    eng.close()
    # beside the depth histogram and the windows, under a selection by label: all three see every site
    r = inputs.regions("mix")
    eng = sid.Engine(regions=r, region_stats=True, depth_hist=True, window=100, select="het", chunk_bytes=20_000)
    r.close()
    eng.source_text(inputs.texts["mix"])
    out, st = eng.run()
    assert out == inputs.plain("mix", "local", chunk_bytes=20_000, select="het")[0]
    check_rows(inputs, "mix", "local", eng.region_stats())
    assert sum(x[1] for x in eng.depth_hist()) == st.sites == sum(x[3] for x in eng.windows())
    eng.set_depth_hist(False)   # (the route stays: the region rows still need it)
    eng.source_text(inputs.texts["mix"])
    out, st = eng.run()
    assert out == inputs.plain("mix", "local", chunk_bytes=20_000, select="het")[0]
    check_rows(inputs, "mix", "local", eng.region_stats())
    eng.close()


def test_every_row_set_past_its_pinned_block(sid, oracle):
    """The region rows, the depth histogram and the windows together, each with more rows a chunk than its pinned
    block holds (256, 384 and 64), on the tile path, where the next chunk's stages run before this chunk's rows
    are read: 5,000 sites at even positions, site i of depth 1 + i % 500 (lines of up to 1 KB, so a 512 KiB chunk
    has more than 500 consecutive sites), an interval a site, a window a site."""
    def bases(i):
        d = 1 + i % 500
        return b"." * (d - d // 2) + b"G" * (d // 2) if i % 7 == 0 else b"." * d
    n = 5000
    text = b"".join(line(b"chrO", 2 * i, False, bases(i)) for i in range(1, n + 1))
    kw = dict(chunk_bytes=1 << 19)
    opts = {"win": dict(window=2), "dh": dict(depth_hist=True), "rs": dict(region_stats=True)}

    def engine_rows(**on):
        r = sid.Regions(ones_bed(n))
        eng = sid.Engine(regions=r, **kw, **on)
        r.close()
        eng.source_text(text)
        out, st = eng.run()
        rows = {"win": eng.windows() if "window" in on else None,
                "dh": eng.depth_hist() if "depth_hist" in on else None,
                "rs": eng.region_stats() if "region_stats" in on else None}
        eng.close()
        return out, st, rows

    sites, codes = WR.site_codes(sid, oracle, text, "local")
    ds = DH.depths(sid.parse_text(text).counts)
    r = sid.Regions(ones_bed(n))
    want = {"win": WR.rows(sites, codes, 2), "dh": DH.rows(ds, codes), "rs": RS.rows(RS.intervals(r), sites, codes, ds)}
    r.close()
    assert len(want["win"]) == n and len(want["dh"]) == 500 and len(want["rs"]) == n
    out, st, rows = engine_rows(**opts["win"], **opts["dh"], **opts["rs"])
    assert st.chunks >= 3 and st.chunks_tiled > 0, (st.chunks, st.chunks_tiled)
    for k in opts:
        assert rows[k] == want[k], (k, len(rows[k]), len(want[k]),
                                    next(((a, b) for a, b in zip(rows[k], want[k]) if a != b), None))
        assert engine_rows(**opts[k])[2][k] == rows[k], k   # the option alone
    assert out == engine_rows()[0]


def test_failing_run(sid, inputs):
    for more in ({}, {"hold_bytes": 1}):
        errs = []
        for on in (False, True):
            r = inputs.regions("bad_late")
            eng = sid.Engine(regions=r, region_stats=on, chunk_bytes=65536, **more)
            r.close()
            eng.source_text(inputs.texts["bad_late"])
            with pytest.raises(sid.SidError) as ei:
                eng.run()
            errs.append((ei.value.status, ei.value.offset))
            with pytest.raises(sid.SidError) as e2:
                eng.region_stats()
            assert e2.value.status == 7
            eng.close()
        assert errs[0] == errs[1] and errs[0][0] == 4   # the error as without the option


def test_dtext_region_stats(sid, gpu, inputs):
    import torch
    for name in ("mix", "ones", "phase"):
        text = inputs.texts[name]
        r = inputs.regions(name)
        ivs = RS.intervals(r)
        ctx = sid.Context(0, method="local", regions=r)   # (no switch on the context)
        r.close()
        t = sid.DText(ctx, text)
        n = len(t)
        _, dcode, dhom, dhet = gpu.device_buffers(n)
        ctx.call_local(t.counts_ptr, n, dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr())
        torch.cuda.synchronize()
        whole = sid.dtext_region_stats(ctx, t, dcode.data_ptr())
        assert whole == inputs.rows(name, "local")
        parts = []
        for a, b in ((0, n // 6), (n // 6, n // 2), (n // 2, n - 1), (n - 1, n)):
            parts.append(sid.dtext_region_stats(ctx, t, dcode.data_ptr(), a, b))
            assert [x[:3] for x in parts[-1]] == ivs
        tot = parts[0]
        for p in parts[1:]:
            tot = sid.region_stats_merge(tot, p)
        assert tot == whole   # site ranges sum to the whole
        assert sid.dtext_region_stats(ctx, t, dcode.data_ptr(), 5, 5) == [iv + (0, 0, 0, 0, 0) for iv in ivs]
        with pytest.raises(sid.SidError) as ei:
            sid.dtext_region_stats(ctx, t, dcode.data_ptr(), 0, n + 1)
        assert ei.value.status == 1
        t.close()
        ctx.close()
    ctx = sid.Context(0, method="local")   # a context without a set
    t = sid.DText(ctx, inputs.texts["phase"])
    _, dcode, _, _ = gpu.device_buffers(len(t))
    with pytest.raises(sid.SidError) as ei:
        sid.dtext_region_stats(ctx, t, dcode.data_ptr())
    assert ei.value.status == 1
    t.close()
    ctx.close()


def test_cli(sid, inputs, tmp_path):
    out = tmp_path / "r.csv"
    for mkey, name, extra in (("local", "mix", []), ("local", "ones", ["--chunk-bytes", "65536"]),
                              ("lr", "lowcov", ["--chunk-bytes", "20000"]), ("bayes", "mix", []),
                              ("local", "mix", ["--host-parse"]), ("lr", "lowcov", ["--host-parse"]),
                              ("quality", "quality", ["--chunk-bytes", "65536"])):
        args = extra + ["--regions", inputs.paths[name + ".bed"]] + METHODS[mkey][1]
        b = run(sid.CLI_PATH, args + [inputs.paths[name]])
        if out.exists():
            out.unlink()
        a = run(sid.CLI_PATH, args + ["--region-stats", str(out), inputs.paths[name]])
        assert (a.returncode, a.stdout, a.stderr) == (b.returncode, b.stdout, b.stderr), (mkey, name, extra)
        assert b.returncode == 0 and out.read_bytes() == RS.fmt(inputs.rows(name, mkey)), (mkey, name, extra)
    # the stage's other form (SID_RS_FORM=1, the measurement switch: no carry) gives the same rows
    for name in ("whole", "phase", "ones"):
        a = run(sid.CLI_PATH, ["--chunk-bytes", "65536", "--regions", inputs.paths[name + ".bed"], "--region-stats", str(out),
                               inputs.paths[name]], env=dict(os.environ, SID_RS_FORM="1"))
        assert a.returncode == 0 and out.read_bytes() == RS.fmt(inputs.rows(name, "local")), name
    # with --only het the records are the selected ones, the rows the same; --stats names the rows
    want = inputs.rows("mix", "local")
    for extra in ([], ["--host-parse"]):
        plain = run(sid.CLI_PATH, extra + ["--only", "het", "--regions", inputs.paths["mix.bed"], inputs.paths["mix"]])
        a = run(sid.CLI_PATH, extra + ["--stats", "--only", "het", "--regions", inputs.paths["mix.bed"], "--region-stats",
                                       "/nonexistent/x", "--region-stats", str(out), inputs.paths["mix"]])   # (the last wins)
        assert a.returncode == 0 and a.stdout == plain.stdout
        assert out.read_bytes() == RS.fmt(want)
        assert b'"region_rows": %d, "region_sites": %d' % (len(want), sum(x[3] for x in want)) in a.stderr
        s = run(sid.CLI_PATH, extra + ["--stats", inputs.paths["mix"]])
        assert s.returncode == 0 and b"region_rows" not in s.stderr   # only under the option
    # the refusals, each with exit status 1, nothing on stdout, before any input is read
    nodir = str(tmp_path / "no" / "dir.csv")
    over = tmp_path / "over.bed"
    over.write_bytes(b"".join(b"c\t%d\t%d\n" % (2 * i, 2 * i + 1) for i in range(RS.MAX + 1)))
    for extra in ([], ["--host-parse"]):
        a = run(sid.CLI_PATH, extra + ["--regions", inputs.paths["mix.bed"], "--region-stats", nodir, "/nonexistent/input.plp"])
        assert (a.returncode, a.stdout, a.stderr) == (1, b"", b"sid: --region-stats: could not open %s\n" % nodir.encode())
        a = run(sid.CLI_PATH, extra + ["--region-stats", str(out), "/nonexistent/input.plp"])
        assert (a.returncode, a.stdout, a.stderr) == (1, b"", b"sid: --region-stats: needs --regions\n")
        a = run(sid.CLI_PATH, extra + ["--regions", str(over), "--region-stats", str(out), "/nonexistent/input.plp"])
        assert (a.returncode, a.stdout, a.stderr) == (1, b"", b"sid: --region-stats: more than 1048576 intervals\n")
    # a malformed line in the last chunk: the failure as without the option, and no file
    fresh = tmp_path / "none.csv"
    for extra in ([], ["--chunk-bytes", "65536"], ["--host-parse"]):
        args = extra + ["--regions", inputs.paths["bad_late.bed"]]
        b = run(sid.CLI_PATH, args + [inputs.paths["bad_late"]])
        a = run(sid.CLI_PATH, args + ["--region-stats", str(fresh), inputs.paths["bad_late"]])
        assert (a.returncode, a.stdout, a.stderr) == (b.returncode, b"", b.stderr) and b.returncode != 0
        assert not fresh.exists()
    assert b"--region-stats" not in run(sid.CLI_PATH, ["-h"]).stdout   # -h stays the reference's
