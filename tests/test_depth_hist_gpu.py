"""--depth-hist FILE (sid_engine_set_depth_hist) on the device: through
sid_amd.Engine, build/sid and sid_dtext_depth_hist, every formatter family, the
edges of the stage's bins (the LDS range's last bin, the first direct bin, the
top bin, wrapped counts), the shapes of same-address contention, and every
record path of the engine.

The expected rows are always the Python model's (tests/depth_hist_ref.py) over
the host parser's per-site counts and the oracle's codes.  Every engine case
asserts that the records and bytes_out are byte-equal to the same
configuration's without the option, that the rows equal the model's, and that
sum(sites) == stats.sites and stats.depth_rows == len(rows)."""
import os

import pytest

import bgzf_ref
import depth_hist_ref as DH
import windows_ref as WR
from test_select_gpu import line, run
from test_windows import quirks_text
from test_windows_gpu import METHODS, low_cov_text

pytestmark = pytest.mark.gpu

# the wrapped sites: 65536 x A (the u16 count wraps to 0) plus three C = depth 3; 65536 x A alone = depth 0
# with no counted base
WRAP = (b"chrW\t1\tG\t65539\t" + b"A" * 65536 + b"CCC\t" + b"I" * 65539 + b"\n" +
        b"chrW\t2\tG\t65536\t" + b"A" * 65536 + b"\t" + b"I" * 65536 + b"\n")
BIG = [d for k in range(1, 18) for d in (2 ** k - 1, 2 ** k, 2 ** k + 1)] + [65535 * 2, 65535 * 4, 65535 * 4 - 1]


def ramp_text(top: int, mapq: bool = False) -> bytes:
    """One site at every depth 0 .. top, the neighbours of every power of two up to 2^17, 131070, 262140 (the
    top bin), 262139, and the wrapped sites; every third site het where its depth allows."""
    ds = list(range(0, top + 1)) + BIG
    t = b"".join(DH.depth_line(b"chrR", i + 1, d, i % 3 == 0, mapq) for i, d in enumerate(ds))
    if mapq:
        return t + b"".join(ln + b"\t" + b"5" * (65539 - 3 * k) + b"\n" for k, ln in enumerate(WRAP.splitlines()))
    return t + WRAP


def contention_text() -> bytes:
    one = b"".join(line(b"chrC", i, False) for i in range(1, 4097))                        # 4096 sites, one bin
    lanes = b"".join(DH.depth_line(b"chrL", i + 1, 10 + i % 64, i % 5 == 0) for i in range(64 * 24))   # 64 bins a wave
    two = b"".join(DH.depth_line(b"chrT", i + 1, 30 + i % 2) for i in range(2048))         # two depths alternating
    share = b"".join(line(b"chrS", i, i % 2 == 0) for i in range(1, 1025))                  # het and hom, one depth
    return one + lanes + two + share


class DInputs:
    def __init__(self, sid, oracle, d):
        self.sid, self.oracle, self.dir = sid, oracle, d
        self.texts = {
            "ramp": ramp_text(2200),
            "ramp_s": ramp_text(300),
            "ramp_q": ramp_text(300, mapq=True),
            "cont": contention_text(),
            "lowcov": low_cov_text() + b"".join(b"chr7\t%d\tA\t0\t*\t*\n" % i for i in range(1, 301)) +
                      sid.synth_text(83, 1500, 30.0, sites_per_chrom=700),
            "mix": sid.synth_text(81, 2100, 30.0, sites_per_chrom=700) + quirks_text() +
                   sid.synth_text(82, 2000, 30.0, sites_per_chrom=700),
            "tiny": b"".join(b"c\t%d\tA\t0\t*\n" % (i % 10) for i in range(1, 20_000)),
            "deep": sid.synth_text(5, 1500, 200.0, sites_per_chrom=700) +
                    b"".join(line(b"chrD", i, False, b"." * 100 + b"g" * 100 if i % 7 == 0 else b"." * 200)
                             for i in range(1, 701)),
            "quality": sid.synth_text(4, 3000, 30.0, sites_per_chrom=700, mapq=True),
            "synth": sid.synth_text(9, 5000, 30.0, sites_per_chrom=1000),
        }
        good = b"".join(line(b"chr1", i, i % 61 == 0) for i in range(1, 4001))
        self.texts["bad_late"] = good + good + b"chr1\t1\tAC\t3\t...\tIII\n" + good[:3000]
        self.paths = {}
        for k, t in self.texts.items():
            p = d / f"{k}.plp"
            p.write_bytes(t)
            self.paths[k] = str(p)
        self._rows, self._plain, self._codes = {}, {}, {}

    def rows(self, name, mkey):
        """The model's rows once per (input, method)."""
        if (name, mkey) not in self._rows:
            kw = dict(METHODS[mkey][0])
            self._rows[(name, mkey)] = DH.site_rows(self.sid, self.oracle, self.texts[name], kw.pop("method"), **kw)
        return self._rows[(name, mkey)]

    def plain(self, name, mkey, **kw):
        """The engine's records of the same configuration without the option, once each."""
        key = (name, mkey, tuple(sorted((k, repr(v)) for k, v in kw.items())))
        if key not in self._plain:
            eng = self.sid.Engine(**METHODS[mkey][0], **self.build(kw))
            eng.source_text(self.texts[name])
            out, st = eng.run(**self.header(mkey, kw))
            with pytest.raises(self.sid.SidError) as ei:   # the option off: no rows
                eng.depth_hist()
            assert ei.value.status == 7 and st.depth_rows == 0
            eng.close()
            self._plain[key] = (out, st.bytes_out)
        return self._plain[key]

    def build(self, kw):
        kw = dict(kw)
        if "bed" in kw:
            kw["regions"] = self.sid.Regions(kw.pop("bed"))
        return kw

    def header(self, mkey, kw):
        if kw.get("format") != "vcf":
            return {}
        return dict(header=self.sid.vcf_header(**METHODS[mkey][0]))


@pytest.fixture(scope="module")
def inputs(sid, oracle, tmp_path_factory):
    return DInputs(sid, oracle, tmp_path_factory.mktemp("depth_hist"))


def check_rows(inputs, name, mkey, rows, st):
    want = inputs.rows(name, mkey)
    assert rows == want, (name, mkey, len(rows), len(want), next(((a, b) for a, b in zip(rows, want) if a != b), None))
    assert sum(r[1] for r in rows) == st.sites
    assert st.depth_rows == len(rows)


def check_engine(sid, inputs, name, mkey="local", source="text", **kw):
    out0, bytes0 = inputs.plain(name, mkey, **kw)
    eng = sid.Engine(depth_hist=True, **METHODS[mkey][0], **inputs.build(kw))
    f = None
    if source == "text":
        eng.source_text(inputs.texts[name])
    elif source == "bgzf":
        eng.source_bgzf(bgzf_ref.write(inputs.texts[name], payload=20000)[0])
    elif source == "file":
        f = open(inputs.paths[name], "rb")
        eng.source_file(f.fileno())
    out, st = eng.run(**inputs.header(mkey, kw))
    rows = eng.depth_hist()
    eng.close()
    if f:
        f.close()
    if not kw.get("device_sink"):
        assert out == out0, (name, mkey, source, kw)
    assert st.bytes_out == bytes0, (name, mkey, source, kw)
    check_rows(inputs, name, mkey, rows, st)
    return st, rows


@pytest.mark.parametrize("mkey", ["local", "lr"])
def test_ramp(sid, inputs, mkey):
    """Every bin of the dense range and past it, the powers of two, the top bin, wrapped counts."""
    for cb in (0, 1 << 20):
        st, rows = check_engine(sid, inputs, "ramp", mkey, chunk_bytes=cb)
    ds = [r[0] for r in rows]
    assert ds[:2201] == list(range(2201)) and ds[-3:] == [131073, DH.DEPTH_MAX - 1, DH.DEPTH_MAX]
    assert set(BIG) <= set(ds)
    by = {r[0]: r for r in rows}
    assert by[0][1] == 2   # the ramp's site and the wrapped one without a counted base
    assert by[1023][1] == by[1024][1] == by[1025][1] == 2 and by[2200][1] == by[131070][1] == 1
    if mkey == "lr":
        assert [by[d][2] for d in (0, 1, 2, 3)] == [0, 0, 0, 0] and by[4][2] == by[4][1]


@pytest.mark.parametrize("mkey", ["local_R", "bayes", "quality"])
def test_short_ramp(sid, inputs, mkey):
    """(-m quality: some 13 s, nearly all of it the oracle's call over the sites of up to 262140 bases.)"""
    name = "ramp_q" if mkey == "quality" else "ramp_s"
    for cb in (0, 1 << 19):
        st, rows = check_engine(sid, inputs, name, mkey, chunk_bytes=cb)
    assert rows[-1][0] == DH.DEPTH_MAX and [r[0] for r in rows[:301]] == list(range(301))


@pytest.mark.parametrize("mkey", ["local", "lr"])
def test_contention(sid, inputs, mkey):
    for cb in (0, 20_000):
        st, rows = check_engine(sid, inputs, "cont", mkey, chunk_bytes=cb)
    by = {r[0]: r for r in rows}
    assert by[30][1] == 4096 + 24 + 1024 + 1024 and by[31][1] == 24 + 1024
    assert by[30][3] > 0 and by[30][4] >= 4096   # het and hom records in one bin
    assert [by[d][1] for d in range(10, 74) if d not in (30, 31)] == [24] * 62


@pytest.mark.parametrize("mkey", ["local", "lr", "bayes"])
def test_sites_without_a_record(sid, inputs, mkey):
    for cb in (0, 20_000):
        st, rows = check_engine(sid, inputs, "lowcov", mkey, chunk_bytes=cb)
    by = {r[0]: r for r in rows}
    if mkey == "local":
        assert by[0][1:] == (300, 300, 0, 300)   # '*' lines: a "hom,TT" record at depth 0
        assert by[2][1] == by[2][2] > 600
    else:
        assert by[0][1:] == (300, 0, 0, 0) and by[2][1] > 600 and by[2][2] == 0   # sites counted, no record


def test_edges_chunks_lanes_devices(sid, gpu, inputs):
    import torch
    for devices in ([1, torch.cuda.device_count()] if torch.cuda.device_count() >= 2 else [1]):
        for mkey in ("local", "lr"):
            st, _ = check_engine(sid, inputs, "mix", mkey, chunk_bytes=20_000, devices=devices)
            assert st.chunks >= 10
    st, _ = check_engine(sid, inputs, "mix", chunk_bytes=0)
    assert st.chunks == 1
    check_engine(sid, inputs, "mix", chunk_bytes=20_000, lanes=2)
    check_engine(sid, inputs, "mix", "lr", chunk_bytes=20_000, lanes=2)
    check_engine(sid, inputs, "quality", "quality", chunk_bytes=20_000)


def test_line_shapes(sid, inputs):
    st, rows = check_engine(sid, inputs, "tiny", chunk_bytes=100_000)   # tile overflow into the two-pass path
    assert st.tile_overflows > 0 and rows == [(0, 19_999, 19_999, 0, 19_999)]   # each chunk counted once
    st, _ = check_engine(sid, inputs, "deep", chunk_bytes=300_000)   # 200x lines: the quad shape from chunk 2 on
    assert st.chunks >= 3 and st.chunks_tiled >= 2
    check_engine(sid, inputs, "deep", "lr", chunk_bytes=300_000)


@pytest.mark.parametrize("mkey", ["local", "local_R", "lr"])
def test_budgets_count_every_chunk_once(sid, inputs, mkey):
    """hold_bytes=1: nothing formatted in pass 1; retain_bytes=1: the text read again in pass 2."""
    for more in (dict(hold_bytes=1), dict(retain_bytes=1), dict(hold_bytes=1, retain_bytes=1)):
        st, _ = check_engine(sid, inputs, "mix", mkey, chunk_bytes=20_000, **more)
        assert st.chunks >= 10
        if more.get("retain_bytes") and more.get("hold_bytes") and mkey != "local":
            assert st.chunks_reloaded == st.chunks


@pytest.mark.parametrize("mkey", ["local", "lr", "quality"])
def test_independence_of_selections_and_format(sid, inputs, mkey):
    """--only, --regions, --variants, the depth bounds, --context and --vcf change the records, not the rows."""
    name = "quality" if mkey == "quality" else "mix"
    bed = b"chr1\t10\t400\nchr2\t0\t50\nchromosome_A\nchr3\t100\t300\n"
    full = len(inputs.plain(name, mkey)[0])
    for sel in (dict(select="het"), dict(bed=bed), dict(variants=1), dict(min_depth=25, max_depth=32),
                dict(select="het", context=3), dict(select="het", bed=bed, variants=1, min_depth=20, context=3)):
        check_engine(sid, inputs, name, mkey, chunk_bytes=20_000, **sel)
        assert len(inputs.plain(name, mkey, chunk_bytes=20_000, **sel)[0]) < full   # (the selection selects)
    check_engine(sid, inputs, name, mkey, chunk_bytes=20_000, format="vcf")
    check_engine(sid, inputs, name, mkey, chunk_bytes=0, format="vcf", select="het")


@pytest.mark.parametrize("mkey", ["local", "lr"])
def test_independence_of_sinks_and_sources(sid, inputs, mkey):
    for sink, more in ((1, {}), (1, {"hold_bytes": 1}), (2, {"host_hold_bytes": 1 << 22}), (2, {"host_hold_bytes": 3000})):
        check_engine(sid, inputs, "mix", mkey, chunk_bytes=20_000, device_sink=sink, **more)
    check_engine(sid, inputs, "mix", mkey, chunk_bytes=20_000, host_hold_bytes=3000)
    for cb in (0, 65536):
        check_engine(sid, inputs, "mix", mkey, source="bgzf", chunk_bytes=cb)
        check_engine(sid, inputs, "mix", mkey, source="file", chunk_bytes=cb)
    # a synth source: the generator's text is the model's input
    for on_device in (False, True):
        eng = sid.Engine(depth_hist=True, chunk_bytes=65536, **METHODS[mkey][0])
        eng.source_synth(9, 5000, 30.0, sites_per_chrom=1000, on_device=on_device)
        out, st = eng.run()
        assert out == inputs.plain("synth", mkey, chunk_bytes=65536)[0]
        check_rows(inputs, "synth", mkey, eng.depth_hist(), st)
        eng.close()


@pytest.mark.parametrize("mkey", ["local", "lr"])
def test_beside_the_window_rows(sid, inputs, mkey):
    """window=100 as well: both summaries are right and their column sums agree."""
    kw = dict(METHODS[mkey][0])
    sites, codes = WR.site_codes(sid, inputs.oracle, inputs.texts["mix"], kw.pop("method"), **kw)
    for cb in (0, 20_000):
        eng = sid.Engine(depth_hist=True, window=100, chunk_bytes=cb, **METHODS[mkey][0])
        eng.source_text(inputs.texts["mix"])
        out, st = eng.run()
        win, rows = eng.windows(), eng.depth_hist()
        eng.close()
        assert out == inputs.plain("mix", mkey, chunk_bytes=cb)[0]
        check_rows(inputs, "mix", mkey, rows, st)
        assert win == WR.rows(sites, codes, 100) and st.window_rows == len(win)
        assert DH.sums(rows) == DH.sums(win)


def test_state(sid, inputs):
    L = sid.lib()
    eng = sid.Engine(chunk_bytes=20_000)
    assert L.sid_engine_set_depth_hist(eng.h, 2) == 1 and L.sid_engine_set_depth_hist(eng.h, -1) == 1
    eng.set_depth_hist(True)
    with pytest.raises(sid.SidError) as ei:   # before a run
        eng.depth_hist()
    assert ei.value.status == 7
    eng.source_text(inputs.texts["mix"])
    eng.ingest()
    assert L.sid_engine_set_depth_hist(eng.h, 0) == 7 and L.sid_engine_set_depth_hist(eng.h, 1) == 7   # SID_ESTATE
    with pytest.raises(sid.SidError):   # before the emit
        eng.depth_hist()
    eng.estimate()
    out, st = eng.emit()
    assert out == inputs.plain("mix", "local", chunk_bytes=20_000)[0]
    assert eng.depth_hist() == inputs.rows("mix", "local") and st.depth_rows == len(inputs.rows("mix", "local"))
    # two more runs on the engine over other texts: each run's own rows; then off, and on again
    for name in ("cont", "lowcov", "mix"):
        eng.source_text(inputs.texts[name])
        with pytest.raises(sid.SidError):   # a new source: the last run's rows are gone
            eng.depth_hist()
        out, st = eng.run()
        assert out == inputs.plain(name, "local", chunk_bytes=20_000)[0]
        check_rows(inputs, name, "local", eng.depth_hist(), st)
    eng.set_depth_hist(False)
    eng.source_text(inputs.texts["mix"])
    out, st = eng.run()
    assert out == inputs.plain("mix", "local", chunk_bytes=20_000)[0] and st.depth_rows == 0
    with pytest.raises(sid.SidError) as ei:   # the option off
        eng.depth_hist()
    assert ei.value.status == 7
    eng.set_depth_hist(True)
    eng.source_text(inputs.texts["mix"])
    out, st = eng.run()
    check_rows(inputs, "mix", "local", eng.depth_hist(), st)
    eng.close()


def test_failing_run_and_degenerate_inputs(sid, inputs):
    for more in ({}, {"hold_bytes": 1}):
        errs = []
        for on in (False, True):
            eng = sid.Engine(depth_hist=on, chunk_bytes=65536, **more)
            eng.source_text(inputs.texts["bad_late"])
            with pytest.raises(sid.SidError) as ei:
                eng.run()
            errs.append((ei.value.status, ei.value.offset))
            with pytest.raises(sid.SidError) as e2:
                eng.depth_hist()
            assert e2.value.status == 7
            eng.close()
        assert errs[0] == errs[1] and errs[0][0] == 4   # the error as without the option
    for text in (b"", b"\n" * 300):
        for mkey in ("local", "bayes"):
            eng = sid.Engine(depth_hist=True, **METHODS[mkey][0])
            eng.source_text(text)
            out, st = eng.run()
            assert out == sid.HEADER and st.sites == 0 and eng.depth_hist() == [] and st.depth_rows == 0
            eng.close()


def test_dtext_depth_hist(sid, gpu, inputs):
    import torch
    for name in ("mix", "ramp_s"):
        text = inputs.texts[name]
        ds, codes = DH.site_depths_codes(sid, inputs.oracle, text, "local")
        ctx = sid.Context(0, method="local")   # (no switch on the context)
        t = sid.DText(ctx, text)
        n = len(t)
        _, dcode, dhom, dhet = gpu.device_buffers(n)
        ctx.call_local(t.counts_ptr, n, dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr())
        torch.cuda.synchronize()
        assert sid.dtext_depth_hist(ctx, t, dcode.data_ptr()) == DH.rows(ds, codes) == inputs.rows(name, "local")
        for a, b in ((n // 6, n // 2), (0, 1), (n - 1, n), (min(511, n - 2), min(513, n))):
            assert sid.dtext_depth_hist(ctx, t, dcode.data_ptr(), a, b) == DH.rows(ds[a:b], codes[a:b]), (name, a, b)
        assert sid.dtext_depth_hist(ctx, t, dcode.data_ptr(), 5, 5) == []
        assert sid.dtext_depth_hist(ctx, t, None, 0, 0) == []
        with pytest.raises(sid.SidError) as ei:
            sid.dtext_depth_hist(ctx, t, dcode.data_ptr(), 0, n + 1)
        assert ei.value.status == 1
        t.close()
        ctx.close()


def test_cli(sid, inputs, tmp_path):
    out = tmp_path / "d.csv"
    for mkey, name, extra in (("local", "mix", []), ("local", "ramp_s", ["--chunk-bytes", "65536"]),
                              ("lr", "lowcov", ["--chunk-bytes", "20000"]), ("bayes", "mix", []),
                              ("local", "mix", ["--host-parse"]), ("lr", "lowcov", ["--host-parse"]),
                              ("quality", "quality", ["--chunk-bytes", "65536"])):
        b = run(sid.CLI_PATH, extra + METHODS[mkey][1] + [inputs.paths[name]])
        if out.exists():
            out.unlink()
        a = run(sid.CLI_PATH, extra + ["--depth-hist", str(out)] + METHODS[mkey][1] + [inputs.paths[name]])
        assert (a.returncode, a.stdout, a.stderr) == (b.returncode, b.stdout, b.stderr), (mkey, name, extra)
        assert b.returncode == 0 and out.read_bytes() == DH.fmt(inputs.rows(name, mkey)), (mkey, name, extra)
    # with --only het the records are the selected ones, the rows the same; --stats names the rows
    plain = run(sid.CLI_PATH, ["--only", "het", inputs.paths["mix"]])
    a = run(sid.CLI_PATH, ["--stats", "--only", "het", "--depth-hist", "/nonexistent/x", "--depth-hist", str(out),
                           inputs.paths["mix"]])   # (given twice: the last wins)
    assert a.returncode == 0 and a.stdout == plain.stdout
    assert out.read_bytes() == DH.fmt(inputs.rows("mix", "local"))
    assert b'"depth_rows": %d' % len(inputs.rows("mix", "local")) in a.stderr
    # a FILE that cannot be created: exit status 1, nothing on stdout, before any input is read
    nodir = str(tmp_path / "no" / "dir.csv")
    for extra in ([], ["--host-parse"]):
        a = run(sid.CLI_PATH, extra + ["--depth-hist", nodir, "/nonexistent/input.plp"])
        assert (a.returncode, a.stdout, a.stderr) == (1, b"", b"sid: --depth-hist: could not open %s\n" % nodir.encode())
    # a malformed line in the last chunk: the failure as without the option, and no file
    fresh = tmp_path / "none.csv"
    for extra in ([], ["--chunk-bytes", "65536"], ["--host-parse"]):
        b = run(sid.CLI_PATH, extra + [inputs.paths["bad_late"]])
        a = run(sid.CLI_PATH, extra + ["--depth-hist", str(fresh), inputs.paths["bad_late"]])
        assert (a.returncode, a.stdout, a.stderr) == (b.returncode, b"", b.stderr) and b.returncode != 0
        assert not fresh.exists()
    assert b"--depth-hist" not in run(sid.CLI_PATH, ["-h"]).stdout   # -h stays the reference's
