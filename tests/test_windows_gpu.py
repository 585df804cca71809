"""--windows W (sid_opts.window) on the device: through sid_amd.Engine, build/sid
and sid_dtext_windows, every formatter family, the wave, group, tile and chunk
edges of a run, and every record path of the engine.

The expected rows are always the Python model's (tests/windows_ref.py) over
per-site (chrom, pos, code), the codes from the oracle over the host parser's
counts.  Every engine case also asserts that the records are byte-equal to the
same run's without the option, that the rows' sites add up to stats.sites and
their records to the record count of the oracle CLI's unselected stdout."""
import pytest

import bgzf_ref
import windows_ref as WR
from test_select_gpu import BASES, line, run
from test_windows import WS, quirks_text

pytestmark = pytest.mark.gpu

METHODS = {
    "local": (dict(method="local"), []),
    "local_R": (dict(method="local", estimate_prior=True), ["-R", "-m", "local"]),
    "lr": (dict(method="likelihood_ratio", estimate_prior=True), ["-R", "-m", "likelihood_ratio"]),
    "bayes": (dict(method="bayes"), ["-m", "bayes"]),
    "quality": (dict(method="quality"), ["-m", "quality"]),
}


def phase_text(n=6000) -> bytes:
    """Lines of one byte length, positions in a row: with 50 lines a chunk a 37-site window meets every
    offset from a cut."""
    t = b"".join(line(b"chr1", 100000 + i, i % 51 == 0) for i in range(n))
    assert len({len(x) for x in t.splitlines()}) == 1
    return t


def gaps_text() -> bytes:
    """One run (a chrom, positions inside one window of 100) with lines of 60 KB and 300 KB in it: the tiles
    that the long lines cover hold no line start, so whole empty tiles -- and, behind the longer line, whole
    empty 512-slot groups -- lie between two sites of the run."""
    def long_line(pos, k):
        b = b"^I" * k + BASES
        return b"chrG\t%d\tA\t30\t%s\t%s\n" % (pos, b, b"I" * 30)
    head = b"".join(line(b"chrG", 1 + i % 90, i % 9 == 0) for i in range(2000))
    mid = b"".join(line(b"chrG", 1 + i % 90, i % 7 == 0) for i in range(300))
    tail = b"".join(line(b"chrG", 101 + i, False) for i in range(300))
    return head + long_line(50, 30_000) + mid + long_line(60, 150_000) + mid + tail


def low_cov_text() -> bytes:
    """Sites of coverage 2 between 30x sites: the Lynch methods print no record for them."""
    return b"".join(line(b"chr6", i, i % 6 == 1) if i % 3 else line(b"chr6", i, False, b".,") for i in range(1, 2001))


class WInputs:
    def __init__(self, sid, oracle, d):
        self.sid, self.oracle, self.dir = sid, oracle, d
        q = quirks_text()
        self.texts = {
            # chroms change inside waves and tiles; the quirks between two stretches of it
            "mix": sid.synth_text(81, 2100, 30.0, sites_per_chrom=700) + q + sid.synth_text(82, 2000, 30.0, sites_per_chrom=700),
            "phase": phase_text(),
            "gaps": gaps_text(),
            "lowcov": low_cov_text() + sid.synth_text(83, 1500, 30.0, sites_per_chrom=700),
            "tiny": b"".join(b"c\t%d\tA\t0\t*\n" % (i % 10) for i in range(1, 20_000)),
            "deep": sid.synth_text(5, 1500, 200.0, sites_per_chrom=700) +
                    b"".join(line(b"chrD", i, False, b"." * 100 + b"g" * 100 if i % 7 == 0 else b"." * 200)
                             for i in range(1, 701)),
            "quality": sid.synth_text(4, 3000, 30.0, sites_per_chrom=700, mapq=True),
            "empty": b"",
            "newlines": b"\n" * 300,
        }
        good = b"".join(line(b"chr1", i, i % 61 == 0) for i in range(1, 4001))
        self.texts["bad_late"] = good + good + b"chr1\t1\tAC\t3\t...\tIII\n" + good[:3000]
        self.paths = {}
        for k, t in self.texts.items():
            p = d / f"{k}.plp"
            p.write_bytes(t)
            self.paths[k] = str(p)
        self._codes, self._ref, self._plain = {}, {}, {}

    def codes(self, name, mkey):
        """([(chrom, pos)], [code]) once per (input, method)."""
        if (name, mkey) not in self._codes:
            kw = dict(METHODS[mkey][0])
            self._codes[(name, mkey)] = WR.site_codes(self.sid, self.oracle, self.texts[name], kw.pop("method"), **kw)
        return self._codes[(name, mkey)]

    def rows(self, name, mkey, w):
        return WR.rows(*self.codes(name, mkey), w)

    def ref(self, name, mkey, extra=()):
        """The oracle CLI's unselected run."""
        key = (name, mkey, tuple(extra))
        if key not in self._ref:
            self._ref[key] = self.oracle.run_cli(list(extra) + METHODS[mkey][1] + [self.paths[name]])
        return self._ref[key]

    def plain(self, name, mkey, **kw):
        """The engine's records of the same run without the option, once per configuration."""
        key = (name, mkey, tuple(sorted(kw.items())))
        if key not in self._plain:
            eng = self.sid.Engine(**METHODS[mkey][0], **kw)
            eng.source_text(self.texts[name])
            out, st = eng.run()
            with pytest.raises(self.sid.SidError) as ei:   # window == 0: no rows
                eng.windows()
            assert ei.value.status == 7
            eng.close()
            self._plain[key] = (out, st.bytes_out)
        return self._plain[key]


@pytest.fixture(scope="module")
def inputs(sid, oracle, tmp_path_factory):
    return WInputs(sid, oracle, tmp_path_factory.mktemp("windows"))


def check_rows(inputs, name, mkey, w, rows, st):
    want = inputs.rows(name, mkey, w)
    assert rows == want, (name, mkey, w, len(rows), len(want), next(((a, b) for a, b in zip(rows, want) if a != b), None))
    assert sum(r[3] for r in rows) == st.sites
    b = inputs.ref(name, mkey)
    assert b.returncode == 0
    assert sum(r[4] for r in rows) == len(b.stdout.splitlines()) - 1
    assert st.window_rows == len(rows)


def check_engine(sid, inputs, name, w, mkey="local", **kw):
    out0, bytes0 = inputs.plain(name, mkey, **kw)
    eng = sid.Engine(window=w, **METHODS[mkey][0], **kw)
    eng.source_text(inputs.texts[name])
    out, st = eng.run()
    rows = eng.windows()
    eng.close()
    assert out == out0 and st.bytes_out == bytes0, (name, mkey, w, kw)
    check_rows(inputs, name, mkey, w, rows, st)
    return st, rows


@pytest.mark.parametrize("w", WS)
def test_window_sizes_and_chunk_cuts(sid, inputs, w):
    for cb in (4096, 20_000, 0):
        st, rows = check_engine(sid, inputs, "mix", w, chunk_bytes=cb)
        assert st.chunks >= (50 if cb == 4096 else 10 if cb else 1)
    if w == 1:
        assert len(rows) >= 4000   # a row per site, but for the duplicates
    if w == WR.WMAX:
        assert max(r[3] for r in rows) == 700   # a whole chrom: a run over waves, groups and tiles


def test_every_phase_of_a_chunk_cut(sid, gpu, inputs):
    import torch
    L = len(inputs.texts["phase"].splitlines(keepends=True)[0])
    for devices in ([1, 2] if torch.cuda.device_count() >= 2 else [1]):
        for mkey in ("local", "lr"):
            st, rows = check_engine(sid, inputs, "phase", 37, mkey, chunk_bytes=50 * L, devices=devices)
            assert st.chunks >= 100 and len(rows) in (163, 164)
    check_engine(sid, inputs, "phase", 37, chunk_bytes=50 * L, lanes=2)
    check_engine(sid, inputs, "mix", 100, "lr", chunk_bytes=20_000, lanes=2)


def test_runs_across_empty_tiles_and_groups(sid, inputs):
    """A run whose sites lie on both sides of whole empty tiles and whole empty 512-slot groups."""
    for cb in (0, 100_000):
        for mkey in ("local", "lr"):
            st, rows = check_engine(sid, inputs, "gaps", 100, mkey, chunk_bytes=cb)
            assert [r[:3] for r in rows] == [(b"chrG", 0, 100), (b"chrG", 100, 200), (b"chrG", 200, 300), (b"chrG", 300, 400)]
            assert rows[0][3] == 2602
            if mkey == "local" and cb == 0:
                assert st.chunks == 1 and st.chunks_tiled == 1 and st.tile_overflows == 0


@pytest.mark.parametrize("mkey", sorted(METHODS))
def test_methods_and_key_quirks(sid, inputs, mkey):
    """Every formatter family, on the hand-made keys (inside `mix`) and on sites without a record."""
    if mkey == "quality":
        for cb in (0, 20_000):
            check_engine(sid, inputs, "quality", 100, mkey, chunk_bytes=cb)
        return
    for name in ("mix", "lowcov"):
        for w, cb in ((37, 0), (100, 20_000)):
            st, rows = check_engine(sid, inputs, name, w, mkey, chunk_bytes=cb)
        if name == "lowcov" and mkey in ("lr", "bayes"):
            assert sum(r[4] for r in rows) < sum(r[3] for r in rows)   # coverage < 4: sites without a record
    rows = inputs.rows("mix", mkey, 37)
    assert (b"chr1", -74, -37) in [r[:3] for r in rows] and b"chromosomx" in [r[0] for r in rows]


def test_general_option_sets(sid, inputs):
    """No class tables (a negative base): the call kernel and the code / confs formatter."""
    kw = dict(site_error_threshold=-0.5)
    sites, codes = WR.site_codes(sid, inputs.oracle, inputs.texts["mix"], "local", site_error_threshold=-0.5)
    plain = sid.Engine(chunk_bytes=20_000, **kw)
    plain.source_text(inputs.texts["mix"])
    out0, _ = plain.run()
    plain.close()
    eng = sid.Engine(window=37, chunk_bytes=20_000, **kw)
    eng.source_text(inputs.texts["mix"])
    out, st = eng.run()
    assert out == out0 and eng.windows() == WR.rows(sites, codes, 37)
    eng.close()


def test_line_shapes(sid, inputs):
    st, _ = check_engine(sid, inputs, "tiny", 3, chunk_bytes=100_000)   # tile overflow into the two-pass path
    assert st.tile_overflows > 0
    st, _ = check_engine(sid, inputs, "deep", 100, chunk_bytes=300_000)   # 200x lines: the quad shape from chunk 2 on
    assert st.chunks >= 3 and st.chunks_tiled >= 2
    check_engine(sid, inputs, "deep", 100, "lr", chunk_bytes=300_000)


@pytest.mark.parametrize("mkey", ["local", "local_R", "lr"])
def test_budgets_count_every_chunk_once(sid, inputs, mkey):
    """hold_bytes=1: nothing formatted in pass 1; retain_bytes=1: the text read again in pass 2."""
    for more in (dict(hold_bytes=1), dict(retain_bytes=1), dict(hold_bytes=1, retain_bytes=1)):
        st, _ = check_engine(sid, inputs, "mix", 100, mkey, chunk_bytes=20_000, **more)
        assert st.chunks >= 10


@pytest.mark.parametrize("mkey", ["local", "lr", "quality"])
def test_composition_with_the_selections(sid, inputs, mkey):
    """--only, --regions, --context and a BGZF source change the records, not the rows."""
    name = "quality" if mkey == "quality" else "mix"
    bed = b"chr1\t10\t400\nchr2\t0\t50\nchromosome_A\nchr3\t100\t300\n"
    for cb in (0, 20_000):
        for sel in (dict(select="het"), dict(select="hom"), dict(regions=bed), dict(select="het", context=2),
                    dict(select="het", regions=bed), dict(regions=bed, context=2)):
            kw = dict(sel, chunk_bytes=cb)
            outs = []
            for w in (0, 100):
                if "regions" in kw:
                    kw["regions"] = sid.Regions(bed)
                eng = sid.Engine(window=w, **METHODS[mkey][0], **kw)
                eng.source_text(inputs.texts[name])
                out, st = eng.run()
                outs.append((out, st.bytes_out))
                if w:
                    check_rows(inputs, name, mkey, w, eng.windows(), st)
                eng.close()
            assert outs[0] == outs[1], (mkey, sel, cb)
            assert len(outs[0][0]) < len(inputs.plain(name, mkey)[0])   # (the selection selects)
    z = bgzf_ref.write(inputs.texts[name], payload=20000)[0]
    for cb in (0, 65536):
        eng = sid.Engine(window=100, chunk_bytes=cb, **METHODS[mkey][0])
        eng.source_bgzf(z)
        out, st = eng.run()
        assert out == inputs.plain(name, mkey)[0]
        check_rows(inputs, name, mkey, 100, eng.windows(), st)
        eng.close()


@pytest.mark.parametrize("mkey", ["local", "lr"])
def test_sinks_and_reuse(sid, inputs, mkey):
    for sink in (1, 2):
        for more in ({}, {"hold_bytes": 1}):
            eng = sid.Engine(window=100, device_sink=sink, chunk_bytes=20_000, **METHODS[mkey][0], **more)
            eng.source_text(inputs.texts["mix"])
            _, st = eng.run()
            check_rows(inputs, "mix", mkey, 100, eng.windows(), st)
            assert st.bytes_out == inputs.plain("mix", mkey)[1]
            eng.close()
    eng = sid.Engine(window=37, chunk_bytes=20_000, **METHODS[mkey][0])
    with pytest.raises(sid.SidError) as ei:   # before a run
        eng.windows()
    assert ei.value.status == 7
    for name in ("mix", "lowcov", "phase", "mix"):
        eng.source_text(inputs.texts[name])
        with pytest.raises(sid.SidError):   # a new source: the last run's rows are gone
            eng.windows()
        out, st = eng.run()
        assert out == inputs.plain(name, mkey)[0]
        check_rows(inputs, name, mkey, 37, eng.windows(), st)
    eng.close()


def test_degenerate_inputs(sid, inputs):
    for name in ("empty", "newlines"):
        for mkey in ("local", "bayes"):
            eng = sid.Engine(window=100, **METHODS[mkey][0])
            eng.source_text(inputs.texts[name])
            out, st = eng.run()
            assert out == sid.HEADER and st.sites == 0 and eng.windows() == [] and st.window_rows == 0
            eng.close()
    # a malformed line in the last chunk: no rows
    for more in ({}, {"hold_bytes": 1}):
        eng = sid.Engine(window=100, chunk_bytes=65536, **more)
        eng.source_text(inputs.texts["bad_late"])
        with pytest.raises(sid.SidError) as ei:
            eng.run()
        assert ei.value.status == 4
        with pytest.raises(sid.SidError) as ei:
            eng.windows()
        assert ei.value.status == 7
        eng.close()
    with pytest.raises(sid.SidError) as ei:
        sid.Engine(window=-1)
    assert ei.value.status == 1
    with pytest.raises(sid.SidError) as ei:
        sid.Context(0, window=-1)
    assert ei.value.status == 1


def test_dtext_windows(sid, gpu, inputs):
    import torch
    text = inputs.texts["mix"]
    sites, codes = inputs.codes("mix", "local")
    for w in (37, WR.WMAX):
        ctx = sid.Context(0, method="local", window=w)
        t = sid.DText(ctx, text)
        n = len(t)
        _, dcode, dhom, dhet = gpu.device_buffers(n)
        ctx.call_local(t.counts_ptr, n, dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr())
        torch.cuda.synchronize()
        assert sid.dtext_windows(ctx, t, dcode.data_ptr()) == WR.rows(sites, codes, w)
        a, b = 700, 2300   # a range inside: no forced edges, the rows of those sites alone
        assert sid.dtext_windows(ctx, t, dcode.data_ptr(), a, b) == WR.rows(sites[a:b], codes[a:b], w)
        assert sid.dtext_windows(ctx, t, dcode.data_ptr(), 5, 5) == []
        t.close()
        ctx.close()
    ctx = sid.Context(0, method="local")
    t = sid.DText(ctx, text)
    with pytest.raises(sid.SidError) as ei:
        sid.dtext_windows(ctx, t, None, 0, 0)
    assert ei.value.status == 7
    t.close()
    ctx.close()


def test_cli(sid, inputs, tmp_path):
    out = tmp_path / "w.csv"
    for mkey, name, extra in (("local", "mix", []), ("local", "mix", ["--chunk-bytes", "4096"]),
                              ("lr", "lowcov", ["--chunk-bytes", "20000"]), ("bayes", "mix", []),
                              ("local", "mix", ["--host-parse"]), ("lr", "lowcov", ["--host-parse"]),
                              ("quality", "quality", ["--chunk-bytes", "65536"])):
        b = inputs.ref(name, mkey)
        if out.exists():
            out.unlink()
        a = run(sid.CLI_PATH, extra + ["--windows", "100", "--windows-out", str(out)] + METHODS[mkey][1] + [inputs.paths[name]])
        assert (a.returncode, a.stdout, a.stderr) == (b.returncode, b.stdout, b.stderr), (mkey, name, extra)
        assert out.read_bytes() == WR.fmt(inputs.rows(name, mkey, 100)), (mkey, name, extra)
    # with --only het the records are the selected ones, the rows the same; --stats names the rows
    plain = run(sid.CLI_PATH, ["--only", "het", inputs.paths["mix"]])
    a = run(sid.CLI_PATH, ["--stats", "--only", "het", "--windows", "7", "--windows", "100", "--windows-out", "/nonexistent/x",
                           "--windows-out", str(out), inputs.paths["mix"]])   # (given twice: the last wins)
    assert a.returncode == 0 and a.stdout == plain.stdout
    assert out.read_bytes() == WR.fmt(inputs.rows("mix", "local", 100))
    assert b'"window_rows": %d' % len(inputs.rows("mix", "local", 100)) in a.stderr
    # the three messages: exit status 1, nothing on stdout
    p = inputs.paths["mix"]
    for args, msg in ((["--windows", "100"], b"sid: --windows and --windows-out go together\n"),
                      (["--windows-out", str(out)], b"sid: --windows and --windows-out go together\n"),
                      (["--windows", "100", "--windows-out", str(tmp_path / "no" / "dir.csv")],
                       b"sid: --windows-out: could not open %s\n" % str(tmp_path / "no" / "dir.csv").encode())):
        a = run(sid.CLI_PATH, args + [p])
        assert (a.returncode, a.stdout, a.stderr) == (1, b"", msg), args
    for arg in ("0", "-1", "2147483648", "x", "", "1x", "1e3", " 5", "99999999999"):
        for extra in ([], ["--host-parse"]):
            a = run(sid.CLI_PATH, extra + ["--windows", arg, "--windows-out", str(out), p])
            assert (a.returncode, a.stdout) == (1, b"")
            assert a.stderr == b"sid: --windows: expected 1..2147483647, got %s\n" % arg.encode()
    a = run(sid.CLI_PATH, ["--windows", "2147483647", "--windows-out", str(out), p])
    assert a.returncode == 0 and out.read_bytes() == WR.fmt(inputs.rows("mix", "local", WR.WMAX))
    # a malformed line in the last chunk: the oracle's failure, and no file
    b = inputs.oracle.run_cli([inputs.paths["bad_late"]])
    fresh = tmp_path / "none.csv"
    for extra in ([], ["--chunk-bytes", "65536"], ["--host-parse"]):
        a = run(sid.CLI_PATH, extra + ["--windows", "100", "--windows-out", str(fresh), inputs.paths["bad_late"]])
        assert (a.returncode, a.stdout, a.stderr) == (b.returncode, b"", b.stderr)
        assert not fresh.exists()
    # -h stays the reference's
    a, b = run(sid.CLI_PATH, ["-h"]), inputs.oracle.run_cli(["-h"])
    assert a.stdout == b.stdout and b"--windows" not in a.stdout
