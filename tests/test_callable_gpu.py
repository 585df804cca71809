"""--callable FILE on the device: sid_dtext_callable (the stage's flag, link,
scan and fill kernels over a range of a resident shard) and build/sid.

The expected rows are always the Python model's (tests/callable_ref.py) over
per-site (chrom, pos, code, depth): the codes from the oracle over the host
parser's counts (windows_ref.site_codes), the depths from depth_ref.depths.
The texts are built like those of test_windows_gpu.py: chroms changing inside
waves, runs of 36 sites at every offset from a 512-slot group's edge, lines of
60 KB and 300 KB inside a run, sites without a record, 200x lines, and sites
that are callable and not in turn, which make a row per two sites."""
import pytest

import callable_ref as CR
import depth_ref
import windows_ref as WR
from test_callable import quirks_text
from test_select_gpu import BASES, line, run
from test_windows import quirks_text as window_quirks
from test_windows_gpu import METHODS, low_cov_text

pytestmark = pytest.mark.gpu

STARS = b"*" * 30   # as long as a 30x line's bases, and no counted base: depth 0, never callable


def phase_text(n=6000) -> bytes:
    """Positions in a row, every 37th site without a counted base: the runs of 36 sites meet every offset
    from a wave's and a 512-slot group's edge."""
    return b"".join(line(b"chr1", 100000 + i, i % 51 == 0, STARS if i % 37 == 36 else None) for i in range(n))


def gaps_text() -> bytes:
    """One run of positions in a row with lines of 60 KB and 300 KB in it."""
    def long_line(pos, k):
        b = b"^I" * k + BASES
        return b"chrG\t%d\tA\t30\t%s\t%s\n" % (pos, b, b"I" * 30)
    head = b"".join(line(b"chrG", 1 + i, i % 9 == 0) for i in range(2000))
    mid1 = b"".join(line(b"chrG", 2002 + i, i % 7 == 0) for i in range(300))
    mid2 = b"".join(line(b"chrG", 2303 + i, i % 7 == 0) for i in range(300))
    tail = b"".join(line(b"chrG", 2700 + i, False) for i in range(300))   # (a gap in the positions: a second row)
    return head + long_line(2001, 30_000) + mid1 + long_line(2302, 150_000) + mid2 + tail


def alt_text(n=40_000) -> bytes:
    """Callable and non-callable sites in turn: a row per two sites."""
    return b"".join(line(b"chrA", i, i % 10 == 1, STARS if i % 2 == 0 else None) for i in range(1, n + 1))


class CInputs:
    def __init__(self, sid, oracle, d):
        self.sid, self.oracle, self.dir = sid, oracle, d
        self.texts = {
            "mix": sid.synth_text(81, 2100, 30.0, sites_per_chrom=700) + quirks_text() + window_quirks() +
                   sid.synth_text(82, 2000, 30.0, sites_per_chrom=700),
            "phase": phase_text(),
            "gaps": gaps_text(),
            "lowcov": low_cov_text() + b"".join(b"chr7\t%d\tA\t0\t*\t*\n" % i for i in range(1, 301)) +
                      sid.synth_text(83, 1500, 30.0, sites_per_chrom=700),
            "deep": sid.synth_text(5, 1500, 200.0, sites_per_chrom=700) +
                    b"".join(line(b"chrD", i, False, b"." * 100 + b"g" * 100 if i % 7 == 0 else b"." * 200)
                             for i in range(1, 701)),
            "alt": alt_text(),
        }
        good = b"".join(line(b"chr1", i, i % 61 == 0) for i in range(1, 4001))
        self.texts["bad_late"] = good + good + b"chr1\t1\tAC\t3\t...\tIII\n" + good[:3000]
        self.paths = {}
        for k, t in self.texts.items():
            p = d / f"{k}.plp"
            p.write_bytes(t)
            self.paths[k] = str(p)
        self._sites = {}

    def sites(self, name, mkey):
        """([(chrom, pos)], [code], [depth]) once per (input, method)."""
        if (name, mkey) not in self._sites:
            kw = dict(METHODS[mkey][0])
            sites, codes = WR.site_codes(self.sid, self.oracle, self.texts[name], kw.pop("method"), **kw)
            ds = depth_ref.depths(self.texts[name])
            assert len(ds) == len(sites)
            self._sites[(name, mkey)] = (sites, codes, ds)
        return self._sites[(name, mkey)]

    def rows(self, name, mkey, lo=0, hi=0):
        return CR.rows(*self.sites(name, mkey), lo, hi)


@pytest.fixture(scope="module")
def inputs(sid, oracle, tmp_path_factory):
    return CInputs(sid, oracle, tmp_path_factory.mktemp("callable"))


def device_rows(sid, gpu, inputs, name, mkey, lo=0, hi=0, ranges=()):
    """sid_dtext_callable over the whole shard and over `ranges`, the device codes the oracle's (so that
    every method's codes, dropped sites among them, reach the stage)."""
    import numpy as np
    import torch
    sites, codes, ds = inputs.sites(name, mkey)
    ctx = sid.Context(0, method="local")   # (no switch on the context; its depth bounds hold)
    if lo or hi:
        ctx.set_depth(lo, hi)
    t = sid.DText(ctx, inputs.texts[name])
    n = len(t)
    assert n == len(sites)
    dcode = torch.from_numpy(np.array(codes, np.uint8)).cuda()
    torch.cuda.synchronize()
    whole = sid.dtext_callable(ctx, t, dcode.data_ptr())
    for a, b in ranges:
        a, b = min(a, n), min(b, n)
        assert sid.dtext_callable(ctx, t, dcode.data_ptr(), a, b) == CR.rows(sites[a:b], codes[a:b], ds[a:b], lo, hi), \
            (name, mkey, a, b)
    assert sid.dtext_callable(ctx, t, dcode.data_ptr(), 5, 5) == []
    assert sid.dtext_callable(ctx, t, None, 0, 0) == []
    with pytest.raises(sid.SidError) as ei:
        sid.dtext_callable(ctx, t, dcode.data_ptr(), 0, n + 1)
    assert ei.value.status == 1
    t.close()
    ctx.close()
    want = inputs.rows(name, mkey, lo, hi)
    assert whole == want, (name, mkey, lo, hi, len(whole), len(want),
                           next(((x, y) for x, y in zip(whole, want) if x != y), None))
    return whole


RANGES = ((0, 1), (63, 65), (63, 1025), (511, 513), (700, 2900), (4000, 10 ** 9))


@pytest.mark.parametrize("bounds", [(0, 0), (25, 32), (31, 0), (0, 29)])
@pytest.mark.parametrize("mkey", ["local", "lr", "bayes"])
def test_quirks_and_bounds(sid, gpu, inputs, mkey, bounds):
    """Chroms changing inside waves and the hand-made quirks, under bounds that split the depths."""
    lo, hi = bounds
    rows = device_rows(sid, gpu, inputs, "mix", mkey, lo, hi, RANGES)
    sites, codes, ds = inputs.sites("mix", mkey)
    assert 0 < CR.total_sites(rows) < len(sites)
    if bounds == (0, 0):
        assert max(r[2] - r[1] for r in rows) >= 600   # most of a chrom: a run over many waves and groups
        assert (b"chrZ", 2 ** 31 - 2, 2 ** 31 - 1, 0) in rows and (b"c" * 40, 9, 11, 2) in rows
    else:
        assert CR.total_sites(rows) < CR.total_sites(inputs.rows("mix", mkey))


def test_every_phase_of_a_group_edge(sid, gpu, inputs):
    for mkey in ("local", "lr"):
        rows = device_rows(sid, gpu, inputs, "phase", mkey, ranges=[(k, k + 1500) for k in range(0, 40)])
        assert len(rows) == 163 and {r[2] - r[1] for r in rows} == {36, 6}


def test_runs_across_long_lines(sid, gpu, inputs):
    for mkey in ("local", "lr"):
        rows = device_rows(sid, gpu, inputs, "gaps", mkey, ranges=RANGES)
        assert [r[:3] for r in rows] == [(b"chrG", 0, 2602), (b"chrG", 2699, 2999)]


@pytest.mark.parametrize("mkey", ["local", "local_R", "lr", "bayes"])
def test_sites_without_a_record(sid, gpu, inputs, mkey):
    rows = device_rows(sid, gpu, inputs, "lowcov", mkey, ranges=RANGES)
    sites, codes, ds = inputs.sites("lowcov", mkey)
    rec = sum(1 for c in codes if not c & CR.DROPPED)
    if mkey in ("lr", "bayes"):
        assert CR.total_sites(rows) == rec < len(sites)   # coverage < 4: sites without a record
    else:
        assert CR.total_sites(rows) == rec - 300          # -m local's "hom,TT" placeholders at depth 0


def test_deep_lines(sid, gpu, inputs):
    for mkey in ("local", "lr"):
        device_rows(sid, gpu, inputs, "deep", mkey, ranges=RANGES)
        rows = device_rows(sid, gpu, inputs, "deep", mkey, 190, 205)
        assert 0 < CR.total_sites(rows) < 2200 and len(rows) > 100


def test_a_row_per_two_sites(sid, gpu, inputs):
    """40,000 sites, every second one not callable: 20,000 rows, and a head in every second lane."""
    for mkey in ("local", "lr"):
        rows = device_rows(sid, gpu, inputs, "alt", mkey, ranges=RANGES)
        assert len(rows) == 20_000 and all(r[2] - r[1] == 1 for r in rows)


def test_cli(sid, inputs, tmp_path):
    out = tmp_path / "c.bed"
    for mkey, name, lo, hi in (("local", "mix", 0, 0), ("local", "mix", 25, 32), ("lr", "lowcov", 0, 0),
                               ("bayes", "mix", 0, 0), ("local", "alt", 0, 0)):
        dep = (["--min-depth", str(lo)] if lo else []) + (["--max-depth", str(hi)] if hi else [])
        b = run(sid.CLI_PATH, ["--host-parse"] + dep + METHODS[mkey][1] + [inputs.paths[name]])
        if out.exists():
            out.unlink()
        a = run(sid.CLI_PATH, ["--host-parse"] + dep + ["--callable", str(out)] + METHODS[mkey][1] + [inputs.paths[name]])
        assert (a.returncode, a.stdout, a.stderr) == (b.returncode, b.stdout, b.stderr), (mkey, name)
        assert b.returncode == 0 and out.read_bytes() == CR.fmt(inputs.rows(name, mkey, lo, hi)), (mkey, name, lo, hi)
    # with --only het, --variants and --vcf the records are the selected ones, the rows the same; --stats
    # names the rows and sites
    want = inputs.rows("mix", "local")
    for sel in (["--only", "het"], ["--variants", "--vcf"]):
        plain = run(sid.CLI_PATH, ["--host-parse"] + sel + [inputs.paths["mix"]])
        a = run(sid.CLI_PATH, ["--host-parse", "--stats"] + sel + ["--callable", "/nonexistent/x", "--callable", str(out),
                               inputs.paths["mix"]])   # (given twice: the last wins)
        assert a.returncode == 0 and a.stdout == plain.stdout
        assert out.read_bytes() == CR.fmt(want)
        assert b'"callable_rows": %d, "callable_sites": %d' % (len(want), CR.total_sites(want)) in a.stderr
    # a FILE that cannot be created: exit status 1, nothing on stdout, before any input is read
    nodir = str(tmp_path / "no" / "dir.bed")
    a = run(sid.CLI_PATH, ["--host-parse", "--callable", nodir, "/nonexistent/input.plp"])
    assert (a.returncode, a.stdout, a.stderr) == (1, b"", b"sid: --callable: could not open %s\n" % nodir.encode())
    # the streaming path has no rows yet: said before any input is read
    for extra in ([], ["--host-parse", "-m", "quality"]):
        a = run(sid.CLI_PATH, extra + ["--callable", str(out), "/nonexistent/input.plp"])
        assert (a.returncode, a.stdout, a.stderr) == (1, b"", b"sid: --callable: needs --host-parse\n")
    # a malformed line: the failure as without the option, and no file
    fresh = tmp_path / "none.bed"
    b = run(sid.CLI_PATH, ["--host-parse", inputs.paths["bad_late"]])
    a = run(sid.CLI_PATH, ["--host-parse", "--callable", str(fresh), inputs.paths["bad_late"]])
    assert (a.returncode, a.stdout, a.stderr) == (b.returncode, b"", b.stderr) and b.returncode != 0
    assert not fresh.exists()
    assert b"--callable" not in run(sid.CLI_PATH, ["-h"]).stdout   # -h stays the reference's
