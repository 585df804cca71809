"""--region-stats FILE on the host (CPU only): sid_regions_interval,
sid_region_stats_host, sid_region_stats_format, sid_region_stats_merge and
sid_region_stats_valid (sid_amd/csrc/region_stats.cpp, regions.cpp) against the
Python model of tests/region_stats_ref.py, the three sums of the Conventions,
and the layout of sid_region_row."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depth_hist_ref as DH
import region_stats_ref as RS
import windows_ref as WR
from regions_ref import POS_MAX, RefSet, parse_bed, text_sites
from test_select_gpu import special_text
from test_windows import quirks_text

HERE = os.path.dirname(os.path.abspath(__file__))


def pl(chrom: bytes, pos, bases: bytes = b"...,,,..,.") -> bytes:
    pos = pos if isinstance(pos, bytes) else b"%d" % pos
    return b"%s\t%s\tA\t%d\t%s\t%s\n" % (chrom, pos, len(bases), bases, b"I" * len(bases))


def want_intervals(bed: bytes):
    """The merged intervals in row order from the BED text alone: the chroms by the line of their first
    non-empty interval, a chrom's intervals ascending."""
    first = {}
    for no, ln in enumerate(bed.split(b"\n")):
        one = parse_bed(ln + b"\n") if ln else {}
        for c, v in one.items():
            if v and c not in first:
                first[c] = no
    m = RefSet(bed).m
    assert set(m) == set(first)
    return [(c, s, e) for c in sorted(first, key=first.get) for s, e in zip(*m[c])]


QUIRKS_BED = (b"chr2\t0\t2\n" b"chr1\t36\t74\n" b"chromosome_B\n" b"chr1\t0\t1\n" b"chromosom\t2\t3\n" b"chr1\t100\t500\n"
              b"chromosome_A\t1\t2\n" b"chrL\t0\t3\n" b"absent\t5\t9\n" b"chrZ\t2147483640\t2147483647\n" b"ch\t0\t10\n")
SPECIAL_BED = (b"chromosome12\t10\t200\n" b"a,het,b\t0\t300\n" b"a,hom,b\n" b"chr1\t100\t101\n" b"chr1\t7\t90\n" +
               b"N" * 70 + b"\t350\t1000\n" b"chromosome1\t0\t50\n")


@pytest.fixture(scope="module")
def cases(sid, oracle):
    """name -> (Sites, [(chrom, pos)], [depth], {method: codes}, bed)"""
    out = {}
    for name, text, bed in (("quirks", quirks_text(), QUIRKS_BED), ("special", special_text(sid), SPECIAL_BED)):
        s = sid.parse_text(text)
        codes = {}
        for method, kw in (("local", {}), ("likelihood_ratio", {"estimate_prior": True})):
            sites, codes[method] = WR.site_codes(sid, oracle, text, method, **kw)
        ds = DH.depths(s.counts)
        assert len(s) == len(sites) == len(ds)
        out[name] = (s, sites, ds, codes, bed)
    return out


def host(sid, bed, text, codes=None):
    """(rows of the host path, model rows, Regions) for a text whose codes default to 'a hom record each'."""
    r = sid.Regions(bed)
    s = sid.parse_text(text)
    sites = text_sites(text)
    codes = [0] * len(sites) if codes is None else codes
    got = sid.region_stats_host(r, s, np.array(codes, np.uint8))
    return got, RS.rows(RS.intervals(r), sites, codes, DH.depths(s.counts)), r


def test_interval_enumerates_the_merge_in_source_order(sid):
    beds = [QUIRKS_BED, SPECIAL_BED,
            b"b\t5\t9\na\t0\t3\nb\t0\t2\na\t3\t4\nb\t2\t5\n",                 # abutting lines merge; b before a
            b"z\t4\t4\ny\t1\t2\nz\t1\t3\n",                                    # z's first line is empty: y first
            b"c\t10\t20\nc\t15\t30\nc\t12\t13\nc\t40\t50\nc\t0\t1\n",          # overlapping and nested
            b"", b"e\t7\t7\n"]
    for bed in beds:
        r = sid.Regions(bed)
        want = want_intervals(bed)
        assert len(r) == len(want) == RefSet(bed).intervals
        assert RS.intervals(r) == want, bed
        for (c, s, e), (c2, s2, e2) in zip(want, want[1:]):
            assert c != c2 or e < s2   # disjoint, and not abutting: the merge joined those
        with pytest.raises(sid.SidError) as ei:
            r.interval(len(want))
        assert ei.value.status == 1
    assert RS.intervals(sid.Regions(beds[2])) == [(b"b", 0, 9), (b"a", 0, 4)]
    assert RS.intervals(sid.Regions(beds[3])) == [(b"y", 1, 2), (b"z", 1, 3)]
    # array order for sid_regions_from_intervals; the sorted table would put chr1 before chr2
    r = sid.Regions([(b"chr2", 5, 6), (b"chr10", 0, 1), (b"chr1", 3, 4), (b"chr2", 0, 1)])
    assert RS.intervals(r) == [(b"chr2", 0, 1), (b"chr2", 5, 6), (b"chr10", 0, 1), (b"chr1", 3, 4)]
    L = sid.lib()
    assert L.sid_regions_interval(None, 0, None, None, None, None) == 1
    assert L.sid_regions_interval(r.h, 1, None, None, None, None) == 0   # any out pointer may be NULL


def test_host_rows_against_the_model(sid, cases):
    for name, (s, sites, ds, codes, bed) in cases.items():
        r = sid.Regions(bed)
        ivs = RS.intervals(r)
        assert ivs == want_intervals(bed)
        ref = RefSet(bed)
        for method, code in codes.items():
            want = RS.rows(ivs, sites, code, ds)
            got = sid.region_stats_host(r, s, np.array(code, np.uint8))
            assert got == want, (name, method)
            assert len(got) == len(r)
            assert all(x[5] == x[6] + x[7] and x[5] <= x[3] for x in got)
            # the three sums: the sites that sid_regions_contains holds for, the records and the het records
            # of a run whose only selection is the set
            inside = [r.contains(c, p) for c, p in sites]
            assert inside == [ref.contains(c, p) for c, p in sites]
            assert sum(x[3] for x in got) == sum(inside)
            assert sum(x[4] for x in got) == sum(d for d, i in zip(ds, inside) if i)
            marked = sid.regions_mark(s, np.array(code, np.uint8), r)
            assert sum(x[5] for x in got) == int(((marked & 0x40) == 0).sum())
            assert sum(x[6] for x in got) == int((((marked & 0x40) == 0) & ((marked & 0x80) != 0)).sum())
            assert sid.region_stats_format(got) == RS.fmt(want)
            assert sid.region_stats_format(got, header=False) == RS.fmt(want, header=False)
    rows = dict((x[:3], x) for x in sid.region_stats_host(sid.Regions(QUIRKS_BED), cases["quirks"][0],
                                                          np.array(cases["quirks"][3]["likelihood_ratio"], np.uint8)))
    assert rows[(b"absent", 5, 9)][3:] == (0, 0, 0, 0, 0)               # a chrom of the set that is not in the text
    assert rows[(b"chrL", 0, 3)][3] == 3 and rows[(b"chrL", 0, 3)][5] == 1   # coverage 2: sites without a record
    assert rows[(b"chromosom", 2, 3)][3] == 2                           # not chromoso, chromosomx or chromosome_A
    assert rows[(b"chromosome_A", 1, 2)][3] == 1 and rows[(b"chromosome_B", 0, POS_MAX)][3] == 2
    assert rows[(b"chrZ", 2147483640, POS_MAX)][3] == 2                 # 2^31-1 and 2^31-2


def test_interval_edges(sid):
    text = b"".join(pl(b"c", p) for p in (9, 10, 11, 12, 19, 20, 21, 22, 30, 31, 10, 20))
    got, want, r = host(sid, b"c\t10\t20\nc\t21\t30\n", text)
    # start < pos <= end: 11, 12, 19, 20 and the second 20, not 9, 10 or the second 10; 22 and 30, not 21 or 31
    assert got == want == [(b"c", 10, 20, 5, 50, 5, 0, 5), (b"c", 21, 30, 2, 20, 2, 0, 2)]
    # positions 0, negative and 2^31-1 under a whole-chromosome line: only pos >= 1 is inside
    text = b"".join(pl(b"w", p) for p in (0, -1, -2147483648, 1, POS_MAX, b"-0", b"0005", POS_MAX - 1))
    got, want, r = host(sid, b"w\n", text)
    assert got == want == [(b"w", 0, POS_MAX, 4, 40, 4, 0, 4)]
    # a chrom of the text that is not in the set, chroms over 8 bytes that share their first 8, lengths apart
    text = b"".join(pl(c, 5) for c in (b"chromosome_1", b"chromosome_2", b"chromosom", b"chromoso", b"other",
                                       b"chromosome_2", b"chromosome_10"))
    got, want, r = host(sid, b"chromosome_2\t0\t9\nchromosome_1\t4\t5\nchromoso\t5\t6\nchromosome_10\t0\t4\n", text)
    assert got == want and [x[3] for x in got] == [2, 1, 0, 0]
    # the depth column: A + C + G + T as stored, a '*' site depth 0 with a record of its own
    text = pl(b"d", 1, b"*") + pl(b"d", 2, b"A" * 70000) + pl(b"d", 3, b".C^Ig$t+2AC")
    got, want, r = host(sid, b"d\t0\t5\n", text, [0, 0x80, 0x40])
    assert got == want == [(b"d", 0, 5, 3, 0 + (70000 - 65536) + 4, 2, 1, 1)]


def test_empty_inputs(sid):
    for text in (b"", b"\n" * 300):
        got, want, r = host(sid, b"a\t0\t5\nb\n", text)
        assert got == want == [(b"a", 0, 5, 0, 0, 0, 0, 0), (b"b", 0, POS_MAX, 0, 0, 0, 0, 0)]
    got, want, r = host(sid, b"", pl(b"a", 1))
    assert got == want == []
    assert sid.region_stats_format([]) == RS.HEADER and sid.region_stats_format([], header=False) == b""


def test_subranges_and_merge(sid, cases):
    s, sites, ds, codes, bed = cases["special"]
    r = sid.Regions(bed)
    ivs = RS.intervals(r)
    code = np.array(codes["local"], np.uint8)
    n = len(sites)
    for a, b in ((0, 0), (3, 3), (5, 17), (0, 7), (n - 1, n), (100, 1613), (650, 700)):
        assert sid.region_stats_host(r, s, code, a, b) == RS.rows(ivs, sites[a:b], codes["local"][a:b], ds[a:b]), (a, b)
    parts = [sid.region_stats_host(r, s, code, a, b) for a, b in ((0, 100), (100, 101), (101, n))]
    whole = RS.rows(ivs, sites, codes["local"], ds)
    assert sid.region_stats_merge(sid.region_stats_merge(parts[0], parts[1]), parts[2]) == whole
    assert RS.merge(RS.merge(parts[0], parts[1]), parts[2]) == whole
    big = [(b"x", 0, 5, 2 ** 40, 2 ** 50, 2 ** 40, 2 ** 39, 2 ** 39), (b"a_long_chrom_name", 7, POS_MAX, 1, 2, 1, 0, 1)]
    assert sid.region_stats_merge(big, big) == RS.merge(big, big)
    assert sid.region_stats_merge([], []) == []
    for bad in ([(b"y",) + big[0][1:], big[1]], [big[0][:1] + (1,) + big[0][2:], big[1]],
                [big[0], big[1][:2] + (8,) + big[1][3:]], [big[0], (b"a_long_chrom_namf",) + big[1][1:]], big[::-1]):
        for x, y in ((bad, big), (big, bad)):
            with pytest.raises(sid.SidError) as ei:
                sid.region_stats_merge(x, y)
            assert ei.value.status == 1
    with pytest.raises(sid.SidError):
        sid.region_stats_merge(big, big[:1])
    L = sid.lib()
    rows = C.POINTER(sid.RegionRow)()
    assert L.sid_region_stats_merge(None, None, 2, C.byref(rows)) == 1
    assert L.sid_region_stats_merge(None, None, 0, None) == 1


def test_error_returns(sid, cases):
    L = sid.lib()
    s, sites, ds, codes, bed = cases["quirks"]
    r = sid.Regions(bed)
    code = np.array(codes["local"], np.uint8)
    n = len(sites)
    rows, m = C.POINTER(sid.RegionRow)(), C.c_size_t(7)
    p = code.ctypes.data_as(C.c_void_p)
    assert L.sid_region_stats_host(r.h, s.handle, 2, n + 1, p, C.byref(rows), C.byref(m)) == 1 and m.value == 0 and not rows
    assert L.sid_region_stats_host(r.h, s.handle, 5, 4, p, C.byref(rows), C.byref(m)) == 1
    assert L.sid_region_stats_host(None, s.handle, 0, n, p, C.byref(rows), C.byref(m)) == 1
    assert L.sid_region_stats_host(r.h, None, 0, 0, p, C.byref(rows), C.byref(m)) == 1
    assert L.sid_region_stats_host(r.h, s.handle, 0, n, None, C.byref(rows), C.byref(m)) == 1
    assert L.sid_region_stats_host(r.h, s.handle, 0, n, p, None, C.byref(m)) == 1
    assert L.sid_region_stats_host(r.h, s.handle, 0, n, p, C.byref(rows), None) == 1
    assert L.sid_region_stats_host(r.h, s.handle, 3, 3, None, C.byref(rows), C.byref(m)) == 0 and m.value == len(r)
    L.sid_region_stats_free(rows)
    assert L.sid_engine_region_stats(None, C.byref(rows), C.byref(m)) == 1
    assert L.sid_engine_set_region_stats(None, 1) == 1
    assert "region_rows" not in [f for f, _ in sid.RunStats._fields_]   # (sid_run_stats keeps its layout)


def test_format_sizing_convention(sid):
    L = sid.lib()
    rows = [(b"chr1", 0, 5, 3, 90, 2, 1, 1), (b"a,b" + b"N" * 70, 7, POS_MAX, 2 ** 40, 2 ** 60, 2 ** 40, 0, 2 ** 40),
            (b"x", 9, 10, 0, 0, 0, 0, 0)]
    want = RS.fmt(rows)
    assert want == (b"chrom,start,end,sites,depth,records,het,hom\nchr1,0,5,3,90,2,1,1\n" +
                    b"a,b" + b"N" * 70 + b",7,2147483647,%d,%d,%d,0,%d\nx,9,10,0,0,0,0,0\n" % (2 ** 40, 2 ** 60, 2 ** 40, 2 ** 40))
    assert sid.region_stats_format(rows) == want
    arr, m, keep = sid._region_array(rows)
    n = C.c_size_t(0)
    assert L.sid_region_stats_format(arr, 3, 1, None, 0, C.byref(n)) == 3 and n.value == len(want)   # SID_ENOMEM: sizes
    buf = C.create_string_buffer(len(want))
    assert L.sid_region_stats_format(arr, 3, 1, buf, len(want) - 1, C.byref(n)) == 3 and n.value == len(want)
    assert L.sid_region_stats_format(arr, 3, 1, buf, len(want), C.byref(n)) == 0 and buf.raw == want
    assert L.sid_region_stats_format(None, 3, 1, buf, len(want), C.byref(n)) == 1
    assert L.sid_region_stats_format(arr, 3, 1, buf, len(want), None) == 1


def test_the_cap(sid):
    """2^20 merged intervals are the most the option takes: the host-side validity function refuses one more."""
    assert RS.MAX == sid.REGION_STATS_MAX == 1 << 20
    for n, ok in ((RS.MAX, True), (RS.MAX + 1, False)):
        start = np.arange(n, dtype=np.int32) * 2
        names = (C.c_char_p * n)(*([b"c"] * n))
        h = C.c_void_p()
        end = start + 1
        assert sid.lib().sid_regions_from_intervals(names, start.ctypes.data_as(C.c_void_p),
                                                    end.ctypes.data_as(C.c_void_p), n, C.byref(h)) == 0
        assert sid.lib().sid_regions_intervals(h) == n
        assert sid.lib().sid_region_stats_valid(h) == (0 if ok else 1)
        sid.lib().sid_regions_free(h)
    assert sid.lib().sid_region_stats_valid(None) == 1
    assert sid.Regions(b"a\t0\t1\n").region_stats_valid()


def test_region_row_layout(sid, tmp_path):
    """sizeof(sid_region_row) and its offsets from a compiled probe against the ctypes mirror."""
    fields = [f for f, _ in sid.RegionRow._fields_]
    assert fields == ["chrom", "chrom_len", "start", "end", "sites", "depth", "records", "het", "hom"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "sid.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(sid_region_row));']
    lines += [f'  printf("{f} %zu\\n", offsetof(sid_region_row, {f}));' for f in fields]
    lines += ['  printf("stats %zu\\n", sizeof(sid_run_stats));', '  printf("opts %zu\\n", sizeof(sid_opts));',
              '  printf("max %u\\n", (unsigned)SID_REGION_STATS_MAX);', "  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(exe)],
                   check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(sid.RegionRow) == 72
    for f in fields:
        assert int(got[f]) == getattr(sid.RegionRow, f).offset, f
    assert int(got["stats"]) == C.sizeof(sid.RunStats) and int(got["opts"]) == C.sizeof(sid.Opts)
    assert int(got["max"]) == RS.MAX
