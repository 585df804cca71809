"""Region sets on the host (sid_regions_*: the BED parser, the merge, contains,
sid_regions_mark + sid_format_csv -- the --host-parse path of --regions) and in
the binding (sid_amd.Regions, Opts.regions).  CPU.

The expected results come from tests/regions_ref.py, the semantics restated
in Python: a record is inside when its chrom field (the record split from the
right, line.rsplit(b",", 6)) equals a BED chrom byte for byte and start < pos
<= end."""
import ctypes as C
import os

import numpy as np
import pytest

from regions_ref import (POS_MAX, BedError, RefSet, bed_points, bed_runs, bed_whole, filter_csv, parse_bed,
                         text_sites)
from test_select import golden_arrays
from test_select_gpu import special_text

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

GOOD = [
    (b"", 0, 0),
    (b"\n\n", 0, 0),
    (b"chr1\t10\t20\n", 1, 1),
    (b"chr1\t10\t20", 1, 1),                                   # a final line without a newline counts
    (b"chr1 10 20\n", 1, 1),                                   # spaces
    (b"chr1 \t  10\t\t20  \n", 1, 1),                          # runs of separators, trailing ones
    (b"  chr1\t10\t20\n", 1, 1),                               # leading ones
    (b"chr1\t10\t20\tname\t0\t+\n", 1, 1),                     # further fields are ignored
    (b"chr1\t10\t20\t-5\tx y\n", 1, 1),
    (b"# a comment\n#\ntrack name=x\nbrowser position chr1\ntrackless\t1\t2\n", 0, 0),   # "track..." lines are skipped
    (b"chr1\n", 1, 1),                                         # one field: the whole chromosome
    (b"chr1\nchr1\t5\t9\n", 1, 1),
    (b"chr1\t5\t5\n", 0, 0),                                   # an empty interval holds nothing
    (b"chr1\t0\t0\nchr2\t7\t7\n", 0, 0),
    (b"chr1\t0\t99999999999\n", 1, 1),                         # an end above 2^31-1 is clamped
    (b"chr1\t99999999999\t99999999999999999999999999\n", 0, 0),   # ... and so is the start: empty
    (b"chr1\t0005\t0010\n", 1, 1),
    (b"chr1\t2147483646\t2147483647\n", 1, 1),
    # the merge: unsorted, nested, adjacent [a,b) + [b,c), duplicates, empty ones
    (b"c\t30\t40\nc\t10\t20\nc\t20\t30\n", 1, 1),
    (b"c\t10\t20\nc\t21\t30\n", 2, 1),
    (b"c\t10\t100\nc\t20\t30\nc\t40\t50\nc\t10\t100\n", 1, 1),
    (b"c\t10\t20\nc\t15\t25\nc\t15\t25\nd\t1\t2\nc\t22\t22\n", 2, 2),
    (b"b\t1\t2\na\t1\t2\nb\t2\t3\nab\t0\t1\n", 3, 3),
    (b"a,het,b\t1\t5\n", 1, 1),                                # commas belong to the name
]
BAD = [
    (b"chr1\t10\n", 1),                                        # two fields
    (b"ok\t1\t2\nchr1\t10\n", 2),
    (b"# c\n\nok\t1\t2\nchr1\t-1\t5\n", 4),                    # a sign (empty and comment lines count)
    (b"chr1\t+1\t5\n", 1),
    (b"chr1\t1\t-5\n", 1),
    (b"chr1\t1\t5x\n", 1),                                     # a non-digit
    (b"chr1\t1.0\t5\n", 1),
    (b"chr1\t1e3\t5000\n", 1),
    (b"chr1\t0x1\t5\n", 1),
    (b"chr1\t9\t5\n", 1),                                      # start > end
    (b"chr1\t1\t5\r\n", 1),                                    # a carriage return is a non-digit
    (b"chr1\t1\t5\n \t \n", 2),                                # separators alone: no field
    (b"chr1\t99999999999999999999999999\t5\n", 1),             # start > end, far above the range
    (b"a\t1\t2\nb\t1\t2\nc\t1", 3),                            # the last line, without a newline
]


def from_bed(sid, text):
    h, line = C.c_void_p(), C.c_uint64(77)
    rc = sid.lib().sid_regions_from_bed(text, len(text), C.byref(h), C.byref(line))
    return rc, h, line.value


@pytest.mark.parametrize("k", range(len(GOOD)))
def test_bed_accepted(sid, k):
    text, ni, nc = GOOD[k]
    ref = RefSet(text)
    assert (ref.intervals, ref.chroms) == (ni, nc), "the test's own parser"
    rc, h, line = from_bed(sid, text)
    assert rc == 0 and h.value and line == 0
    assert (sid.lib().sid_regions_intervals(h), sid.lib().sid_regions_chroms(h)) == (ni, nc)
    sid.lib().sid_regions_free(h)
    r = sid.Regions(text)
    assert (len(r), r.chroms) == (ni, nc)
    r.close()


@pytest.mark.parametrize("k", range(len(BAD)))
def test_bed_rejected(sid, k):
    text, bad = BAD[k]
    with pytest.raises(BedError) as ei:
        parse_bed(text)
    assert ei.value.line == bad, "the test's own parser"
    rc, h, line = from_bed(sid, text)
    assert rc == 1 and not h.value and line == bad
    with pytest.raises(sid.SidError) as e2:
        sid.Regions(text)
    assert e2.value.status == 1 and f"line {bad}" in str(e2.value)


def test_null_arguments(sid):
    L = sid.lib()
    assert L.sid_regions_from_bed(b"", 0, None, None) == 1
    h = C.c_void_p()
    assert L.sid_regions_from_bed(None, 0, C.byref(h), None) == 0 and h.value   # err_line is optional
    assert L.sid_regions_intervals(h) == 0 and L.sid_regions_contains(h, b"chr1", 4, 1) == 0
    L.sid_regions_free(h)
    assert L.sid_regions_from_bed(None, 5, C.byref(h), None) == 1
    assert L.sid_regions_intervals(None) == 0 and L.sid_regions_chroms(None) == 0
    assert L.sid_regions_contains(None, b"chr1", 4, 1) == 0
    L.sid_regions_free(None)


def test_from_intervals(sid):
    r = sid.Regions([("chr1", 0, 5), (b"chr1", 5, 9), ("chr2", 3, 3), ("chr9", 0, POS_MAX)])
    assert (len(r), r.chroms) == (2, 2)
    assert [r.contains("chr1", p) for p in (0, 1, 9, 10)] == [False, True, True, False]
    assert r.contains(b"chr9", POS_MAX) and not r.contains("chr2", 3)
    r.close()
    with pytest.raises(sid.SidError):
        r.contains("chr1", 1)   # closed
    assert len(sid.Regions([])) == 0
    for bad in ([("chr1", 5, 4)], [("chr1", -1, 4)], [("", 1, 4)], [("a b", 1, 4)], [("a\tb", 1, 4)], [("a\n", 1, 4)],
                [("chr1", 0, 2 ** 31)]):
        with pytest.raises(sid.SidError):
            sid.Regions(bad)


def test_from_a_path(sid, tmp_path):
    p = tmp_path / "x.bed"
    p.write_bytes(b"chr1\t1\t3\n")
    for src in (str(p), p):
        r = sid.Regions(src)
        assert len(r) == 1 and r.contains("chr1", 2) and not r.contains("chr1", 1)
    with pytest.raises(OSError):
        sid.Regions(str(tmp_path / "missing.bed"))


NAMES = [b"1", b"X", b"chr1", b"chr10", b"chr2", b"12345678", b"123456789", b"12345678x", b"1234567", b"N" * 70,
         b"N" * 69 + b"M", b"N" * 71, b"a,het,b", b"abcdefgh_1", b"abcdefgh_2", b"abcdefgh"]


def random_bed(rng, names, n, span=5000):
    out = []
    for _ in range(n):
        c = names[int(rng.integers(len(names)))]
        k = int(rng.integers(10))
        if k == 0:
            out.append(c + b"\n")
            continue
        s = int(rng.integers(0, span))
        e = s + (0 if k == 1 else int(rng.integers(1, 40)))
        if k == 2:
            s, e = 0, int(rng.integers(1, 50))
        if k == 3:
            s, e = POS_MAX - int(rng.integers(1, 50)), POS_MAX + int(rng.integers(0, 3))
        out.append(b"%s%s%d\t%d\n" % (c, b"\t" if k % 2 else b" ", s, e))
    return b"".join(out)


def boundary_queries(ref: RefSet, names, rng, extra=200):
    q = []
    for c, (st, en) in ref.m.items():
        for s, e in zip(st, en):
            q += [(c, p) for p in (s, s + 1, e, e + 1) if p <= POS_MAX]
    for c in names:
        q += [(c, 0), (c, 1), (c, -1), (c, -2 ** 31), (c, POS_MAX), (c, POS_MAX - 1)]
        q += [(c, int(p)) for p in rng.integers(-50, 5200, extra // len(names) + 1)]
    return q


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_contains_against_the_python_filter(sid, seed):
    rng = np.random.default_rng(seed)
    names = NAMES if seed != 3 else NAMES[:4]
    bed = random_bed(rng, names[:-1], 60 * seed * seed)   # (the last name: never in the set)
    ref = RefSet(bed)
    r = sid.Regions(bed)
    assert (len(r), r.chroms) == (ref.intervals, ref.chroms)
    q = boundary_queries(ref, names + [b"chr", b"chr100", b"N" * 8, b""], rng)
    got = [r.contains(c, p) for c, p in q]
    want = [ref.contains(c, p) for c, p in q]
    assert got == want, [x for x, a, b in zip(q, got, want) if a != b][:5]
    assert any(want) and not all(want)
    # the same set from its intervals
    r2 = sid.Regions([(c, s, e) for c, (st, en) in ref.m.items() for s, e in zip(st, en)])
    assert [r2.contains(c, p) for c, p in q] == want


@pytest.fixture(scope="module")
def texts(sid, tmp_path_factory):
    d = tmp_path_factory.mktemp("regions_cpu")
    out = {}
    for name, fn in (("c1", "c1_10k.plp"), ("edge", "edge.plp")):
        out[name] = os.path.join(GOLD, fn)
    p = d / "special.plp"
    p.write_bytes(special_text(sid))
    out["special"] = str(p)
    return out


@pytest.mark.parametrize("flags", [[], ["-m", "bayes"]], ids=["local", "bayes"])
@pytest.mark.parametrize("name", ["c1", "edge", "special"])
def test_regions_mark_and_format_csv_give_the_filtered_oracle_csv(sid, oracle, texts, name, flags):
    with open(texts[name], "rb") as f:
        text = f.read()
    b = oracle.run_cli(flags + [texts[name]])
    assert b.returncode == 0
    csv = b.stdout
    header = csv.splitlines(keepends=True)[0]
    sites = sid.parse_text(text)
    code, hom, het, conf_type = golden_arrays(sites, csv)
    assert header + sid.format_csv(sites, code, hom, het, conf_type) == csv, "the test's own reconstruction"
    s = text_sites(text)
    assert len(s) == len(sites)
    every = 2 if name == "edge" else 61
    beds = {"mix": bed_runs(s, lambda i: (i // 70) % 5 == 2) + bed_points(s, lambda i: i % every == 0),
            "whole": bed_whole(s), "none": b"nochrom\t0\t1000\n"}
    for kind, bed in beds.items():
        ref = RefSet(bed)
        r = sid.Regions(bed)
        for select in ("all", "het", "hom"):
            want, kept, dropped = filter_csv(csv, ref, select)
            if kind == "mix" and (select == "all" or name == "special"):   # (the goldens hold few hets)
                assert kept >= 1 and dropped >= 1, (name, select)
            if kind == "none":
                assert want == header
            if kind == "whole" and select == "all":
                assert want == csv
            marked = sid.regions_mark(sites, sid.select_mark(code, select), r)
            assert header + sid.format_csv(sites, marked, hom, het, conf_type) == want, (kind, select)
            marked2 = sid.select_mark(sid.regions_mark(sites, code, r), select)   # either order
            assert (marked == marked2).all()
            assert ((marked & 0xBF) == (code & 0xBF)).all()   # only the "no record" bit is added
        r.close()
    assert (sid.regions_mark(sites, code, None) == code).all()


def test_regions_mark_ranges(sid):
    text = b"".join(b"c%d\t%d\tA\t4\t....\tIIII\n" % (i // 10, i % 10 + 1) for i in range(40))
    sites = sid.parse_text(text)
    r = sid.Regions(b"c1\t2\t5\nc3\n")
    code = np.zeros(40, np.uint8)
    L = sid.lib()
    p = code.ctypes.data_as(C.c_void_p)
    assert L.sid_regions_mark(r.h, sites.handle, 13, 35, p) == 0   # (begins inside a chrom run)
    want = np.zeros(40, np.uint8)
    want[15:30] = 0x40   # c1:4 and c1:5 (sites 13, 14) are inside, c1:6..10 and c2 outside, c3 (30..) whole
    assert (code == want).all()
    assert L.sid_regions_mark(r.h, sites.handle, 30, 41, p) == 1
    assert L.sid_regions_mark(r.h, sites.handle, 5, 4, p) == 1
    assert L.sid_regions_mark(r.h, None, 0, 1, p) == 1
    assert L.sid_regions_mark(r.h, sites.handle, 0, 4, None) == 1
    assert L.sid_regions_mark(r.h, sites.handle, 7, 7, None) == 0
    with pytest.raises(sid.SidError):
        sid.regions_mark(sites, code, "c1")
    with pytest.raises(sid.SidError):
        sid.regions_mark(sites, code[:5], r)


def test_opts_carry_the_set(sid):
    assert sid.make_opts().regions is None
    r = sid.Regions(b"chr1\n")
    assert sid.make_opts(regions=r).regions == r.h.value
    for bad in ("chr1", b"chr1\t1\t2\n", 5, [("chr1", 1, 2)]):
        with pytest.raises(sid.SidError):
            sid.make_opts(regions=bad)
    r.close()
    with pytest.raises(sid.SidError):
        sid.make_opts(regions=r)   # closed
    o = sid.Opts()
    o.regions = 12345
    sid.lib().sid_opts_default(C.byref(o))
    assert o.regions is None


def test_the_filter_splits_from_the_right():
    csv = (b"chrom,pos,label,gt,hom_conf,het_conf,conf_type\n"
           b"a,het,b,1,hom,AA,1,1,p_value\n"
           b"a,het,b,2,het,AC,0.5,1,p_value\n"
           b"a,7,hom,AA,1,1,p_value\n")
    assert filter_csv(csv, RefSet(b"a,het,b\t1\t2\n"))[0].splitlines()[1:] == [b"a,het,b,2,het,AC,0.5,1,p_value"]
    assert filter_csv(csv, RefSet(b"a\n"))[0].splitlines()[1:] == [b"a,7,hom,AA,1,1,p_value"]
