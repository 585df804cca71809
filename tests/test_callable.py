"""--callable FILE on the host (CPU only): sid_callable_host, sid_callable_format,
sid_callable_join and the stitch of the chunks' row lists
(sid_amd/csrc/callable.cpp) against the Python model of tests/callable_ref.py,
and the layouts that stand."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import callable_ref as CR
import depth_ref
import windows_ref as WR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
BOUNDS = [(0, 0), (30, 30), (0, 29), (31, 0)]
METHODS = (("local", {}), ("likelihood_ratio", {"estimate_prior": True}))
PMAX = 2 ** 31 - 1


def pl(chrom: bytes, pos, bases: bytes = b"." * 30, ref: bytes = b"A") -> bytes:
    pos = pos if isinstance(pos, bytes) else b"%d" % pos
    return b"%s\t%s\t%s\t%d\t%s\t%s\n" % (chrom, pos, ref, len(bases), bases, b"I" * len(bases))


HET = b"." * 15 + b"G" * 15


def quirks_text() -> bytes:
    """The definition's quirks, by hand."""
    t = [pl(b"chr1", p) for p in (1, 2, 3)] + [pl(b"chr1", 4, HET), pl(b"chr1", 5)]
    t += [pl(b"chr1", p) for p in (0, -1, -2, 1, 2)]                        # pos 0 and negative: not callable
    t += [pl(b"chrZ", PMAX - 1), pl(b"chrZ", PMAX), pl(b"chrZ", PMAX)]      # 2^31-1 has no successor
    t += [pl(b"chr1", p) for p in (7, 8, 8, 9, 5, 6)]                       # a duplicate, a position that goes back
    t += [pl(b"chromoso", p) for p in (1, 2)] + [pl(b"chromosom", p) for p in (3, 4)]   # 8 and 9 bytes that share 8
    t += [pl(b"chromosom", 5, HET), pl(b"chromosox", 6)]
    t += [pl(b"c" * 40, p, HET) for p in (10, 11)] + [pl(b"c" * 39 + b"d", 12)]   # 40 bytes
    t += [pl(b"chr2", p) for p in (1, 2)] + [pl(b"chr1", 3)] + [pl(b"chr2", 3)]   # a chrom that returns
    t += [pl(b"chr3", 1), pl(b"chr3", 2, b"*" * 30), pl(b"chr3", 3)]        # depth 0: only '*'
    t += [pl(b"chr3", 4, b"." * 30, b"N"), pl(b"chr3", 5)]                  # an N reference with only '.'
    t += [pl(b"chrL", 1), pl(b"chrL", 2, b".,G"), pl(b"chrL", 3, b".,.G"), pl(b"chrL", 4)]   # coverage 3 and 4
    t += [pl(b"chrD", p, b"." * d) for p, d in ((1, 29), (2, 30), (3, 30), (4, 31), (5, 31), (6, 29), (7, 30))]
    return b"".join(t)


def texts():
    out = {"quirks": quirks_text(), "depth": depth_ref.depth_text(700)}
    with open(os.path.join(GOLD, "edge.plp"), "rb") as f:
        out["edge"] = f.read()
    return out


@pytest.fixture(scope="module")
def cases(sid, oracle):
    """name -> (Sites, [(chrom, pos)], [depth], {method: codes})"""
    out = {}
    for name, text in texts().items():
        s = sid.parse_text(text)
        codes = {}
        for method, kw in METHODS:
            sites, codes[method] = WR.site_codes(sid, oracle, text, method, **kw)
        ds = depth_ref.depths(text)
        assert len(s) == len(sites) == len(ds)
        out[name] = (s, sites, ds, codes)
    return out


@pytest.mark.parametrize("lo,hi", BOUNDS)
def test_host_rows_and_format(sid, cases, lo, hi):
    for name, (s, sites, ds, codes) in cases.items():
        for method, code in codes.items():
            want = CR.rows(sites, code, ds, lo, hi)
            got = sid.callable_host(s, np.array(code, np.uint8), lo, hi)
            assert got == want, (name, method, lo, hi)
            assert CR.total_sites(got) == sum(CR.flags(sites, code, ds, lo, hi))
            assert all(0 <= r[1] < r[2] <= PMAX and r[3] <= r[2] - r[1] for r in got)
            assert sid.callable_format(got) == CR.fmt(want)
    s, sites, ds, codes = cases["depth"]
    assert CR.rows(sites, codes["local"], ds, lo, hi)   # (every bound keeps some site of the depth text)


def test_quirks_make_the_rows_the_contract_names(sid, cases):
    """The rows the definition names, spelled out, from the library and from the model alike."""
    s, sites, ds, codes = cases["quirks"]

    def lib_rows(method, lo=0, hi=0):
        got = sid.callable_host(s, np.array(codes[method], np.uint8), lo, hi)
        assert got == CR.rows(sites, codes[method], ds, lo, hi)
        return got

    r = lib_rows("local")
    assert r[:2] == [(b"chr1", 0, 5, 1), (b"chr1", 0, 2, 0)]                  # 1-5 with a het | 0 -1 -2 | 1 2
    assert [x for x in r if x[0] == b"chrZ"] == [(b"chrZ", PMAX - 2, PMAX, 0), (b"chrZ", PMAX - 1, PMAX, 0)]
    k = r.index((b"chr1", 6, 8, 0))
    assert r[k:k + 3] == [(b"chr1", 6, 8, 0), (b"chr1", 7, 9, 0), (b"chr1", 4, 6, 0)]   # 7 8 | 8 9 | 5 6
    assert [x for x in r if x[0].startswith(b"chromoso")] == [(b"chromoso", 0, 2, 0), (b"chromosom", 2, 5, 1),
                                                              (b"chromosox", 5, 6, 0)]
    assert (b"c" * 40, 9, 11, 2) in r and (b"c" * 39 + b"d", 11, 12, 0) in r
    k = r.index((b"chr2", 0, 2, 0))
    assert r[k:k + 3] == [(b"chr2", 0, 2, 0), (b"chr1", 2, 3, 0), (b"chr2", 2, 3, 0)]   # abutting, never merged
    # depth 0 ('*' only, and '.' on an N reference) splits chr3 into 1 | 3 | 5
    assert [d for (c, p), d in zip(sites, ds) if c == b"chr3"] == [30, 0, 30, 0, 30]
    assert [x for x in r if x[0] == b"chr3"] == [(b"chr3", 0, 1, 0), (b"chr3", 2, 3, 0), (b"chr3", 4, 5, 0)]
    # coverage 3 prints a record under -m local and none under a Lynch method
    assert [x[1:3] for x in r if x[0] == b"chrL"] == [(0, 4)]
    lr = lib_rows("likelihood_ratio")
    assert [x[1:3] for x in lr if x[0] == b"chrL"] == [(0, 1), (2, 4)]
    # the bounds are part of the definition
    assert [x[1:3] for x in lib_rows("local", 30, 30) if x[0] == b"chrD"] == [(1, 3), (6, 7)]
    assert [x[1:3] for x in lib_rows("local", 0, 29) if x[0] == b"chrD"] == [(0, 1), (5, 6)]
    assert [x[1:3] for x in lib_rows("local", 31, 0) if x[0] == b"chrD"] == [(3, 5)]


def test_subrange_and_empty(sid, cases):
    s, sites, ds, codes = cases["quirks"]
    code = np.array(codes["local"], np.uint8)
    n = len(sites)
    for a, b in ((0, 0), (3, 3), (2, 17), (n - 1, n), (4, n - 3)):
        assert sid.callable_host(s, code, 0, 0, a, b) == CR.rows(sites[a:b], codes["local"][a:b], ds[a:b]), (a, b)
    for text in (b"", b"\n" * 300):
        e = sid.parse_text(text)
        assert len(e) == 0 and sid.callable_host(e, np.zeros(0, np.uint8)) == []
    assert sid.callable_format([]) == b""


def test_invalid_bounds_and_error_returns(sid, cases):
    L = sid.lib()
    s, sites, ds, codes = cases["quirks"]
    code = np.array(codes["local"], np.uint8)
    n = len(sites)
    for lo, hi in ((-1, 0), (5, 4), (0, -1), (depth_ref.DEPTH_MAX + 1, 0), (0, depth_ref.DEPTH_MAX + 1)):
        with pytest.raises(sid.SidError) as ei:
            sid.callable_host(s, code, lo, hi)
        assert ei.value.status == 1, (lo, hi)
    assert sid.callable_host(s, code, depth_ref.DEPTH_MAX, depth_ref.DEPTH_MAX) == []
    rows, m = C.POINTER(sid.CallableRow)(), C.c_size_t(7)
    p = code.ctypes.data_as(C.c_void_p)
    assert L.sid_callable_host(s.handle, 2, n + 1, p, 0, 0, C.byref(rows), C.byref(m)) == 1 and m.value == 0 and not rows
    assert L.sid_callable_host(s.handle, 5, 4, p, 0, 0, C.byref(rows), C.byref(m)) == 1
    assert L.sid_callable_host(None, 0, 0, p, 0, 0, C.byref(rows), C.byref(m)) == 1
    assert L.sid_callable_host(s.handle, 0, n, None, 0, 0, C.byref(rows), C.byref(m)) == 1
    assert L.sid_callable_host(s.handle, 0, n, p, 0, 0, None, C.byref(m)) == 1
    assert L.sid_callable_host(s.handle, 0, n, p, 0, 0, C.byref(rows), None) == 1
    assert L.sid_callable_host(s.handle, 3, 3, None, 0, 0, C.byref(rows), C.byref(m)) == 0 and m.value == 0
    L.sid_callable_free(rows)
    assert "callable_rows" not in [f for f, _ in sid.RunStats._fields_]


def test_format_sizing_convention(sid):
    L = sid.lib()
    rows = [(b"a\tb", 0, 5, 1), (b"", PMAX - 1, PMAX, 0), (b"c" * 40, 7, 2 ** 40, 2 ** 40 - 7)]
    want = CR.fmt(rows)
    assert want == b"a\tb\t0\t5\t1\n\t2147483646\t2147483647\t0\n" + b"c" * 40 + b"\t7\t%d\t%d\n" % (2 ** 40, 2 ** 40 - 7)
    assert sid.callable_format(rows) == want
    arr = (sid.CallableRow * 3)()
    keep = [C.create_string_buffer(r[0], max(len(r[0]), 1)) for r in rows]
    for k, r in enumerate(rows):
        arr[k] = sid.CallableRow(C.cast(keep[k], C.c_void_p).value, len(r[0]), 0, *r[1:])
    n = C.c_size_t(0)
    assert L.sid_callable_format(arr, 3, None, 0, C.byref(n)) == 3 and n.value == len(want)   # SID_ENOMEM: sizes
    buf = C.create_string_buffer(len(want))
    assert L.sid_callable_format(arr, 3, buf, len(want) - 1, C.byref(n)) == 3 and n.value == len(want)
    assert L.sid_callable_format(arr, 3, buf, len(want), C.byref(n)) == 0 and buf.raw == want
    assert L.sid_callable_format(None, 3, buf, len(want), C.byref(n)) == 1
    assert L.sid_callable_format(arr, 3, buf, len(want), None) == 1


def stitch_lib(sid, chunks):
    L = sid.lib()
    arr, off, names, noff, edge = CR.device_rows(chunks)
    rows, n = C.POINTER(sid.CallableRow)(), C.c_size_t(0)
    rc = L.sid_callable_stitch_chunks(arr, off, names, noff, edge, len(chunks), C.byref(rows), C.byref(n))
    assert rc == 0
    try:
        return sid._callable_rows(rows, n.value)
    finally:
        L.sid_callable_free(rows)


# a small sequence: a run of five, a site that is not callable, a run that abuts the first one's end, a long
# chrom, a repeated position
SEQ = [(b"chr1", p) for p in (1, 2, 3, 4, 5)] + [(b"chr1", 100)] + [(b"chr1", p) for p in (6, 7)] + \
      [(b"chromosome_long", p) for p in (1, 2, 2)] + [(b"chr1", 3)]
SEQ_CODES = [0, CR.HET, 0, 0, CR.HET, CR.DROPPED, 0, CR.HET, 0, CR.HET, 0, 0]
SEQ_DEPTHS = [30] * 12


def test_stitch_over_every_cut_into_three(sid):
    want = CR.rows(SEQ, SEQ_CODES, SEQ_DEPTHS)
    assert want == [(b"chr1", 0, 5, 2), (b"chr1", 5, 7, 1), (b"chromosome_long", 0, 2, 1),
                    (b"chromosome_long", 1, 2, 0), (b"chr1", 2, 3, 0)]
    n = len(SEQ)
    for k in (0, 1, 2, 3):
        for cut in itertools.combinations_with_replacement(range(n + 1), k):
            cuts = [0] + list(cut) + [n]
            chunks = CR.chunk_model(SEQ, SEQ_CODES, SEQ_DEPTHS, cuts)
            assert CR.stitch(chunks) == want, cuts
            assert stitch_lib(sid, chunks) == want, cuts
    # abutting alone is not enough: ..., 5 | 100 (not callable) | 6, ... is two rows, whichever chunk holds
    # the site between -- also one of its own
    for cuts in ([0, 5, 6, n], [0, 6, n], [0, 5, n], [0, 5, 5, 6, 6, n]):
        chunks = CR.chunk_model(SEQ, SEQ_CODES, SEQ_DEPTHS, cuts)
        got = stitch_lib(sid, chunks)
        assert got == want and got[:2] == [(b"chr1", 0, 5, 2), (b"chr1", 5, 7, 1)]
    assert CR.chunk_model(SEQ, SEQ_CODES, SEQ_DEPTHS, [0, 5, 6, n])[1] == ([], CR.HAS_SITE)
    # a site a chunk, and empty chunks between every two
    chunks = CR.chunk_model(SEQ, SEQ_CODES, SEQ_DEPTHS, list(range(n + 1)))
    assert stitch_lib(sid, chunks) == want
    chunks = CR.chunk_model(SEQ, SEQ_CODES, SEQ_DEPTHS, sorted(list(range(n + 1)) * 2))
    assert stitch_lib(sid, chunks) == want
    assert stitch_lib(sid, []) == [] and stitch_lib(sid, [([], 0), ([], 0)]) == []


def test_stitch_rejects(sid):
    L = sid.lib()
    rows, n = C.POINTER(sid.CallableRow)(), C.c_size_t(0)

    def rc_of(chunks, patch=None):
        arr, off, names, noff, edge = CR.device_rows(chunks)
        if patch:
            patch(arr, edge)
        return L.sid_callable_stitch_chunks(arr, off, names, noff, edge, len(chunks), C.byref(rows), C.byref(n))

    good = [([(b"chromosome_long", 0, 2, 1)], 7)]
    assert rc_of(good) == 0
    L.sid_callable_free(rows)
    assert rc_of([([(b"chr1", 0, 2, 1)], 0)]) == 1           # rows without a site
    assert rc_of([([], CR.HAS_SITE | CR.OPEN_END)]) == 1      # an open edge without a row
    assert rc_of([([], 8)]) == 1                              # an unknown bit
    assert rc_of(good, lambda a, e: setattr(a[0], "name", 5)) == 1     # the name outside the blob
    assert rc_of(good, lambda a, e: setattr(a[0], "pos", 0)) == 1
    assert rc_of(good, lambda a, e: setattr(a[0], "sites", 0)) == 1
    assert L.sid_callable_stitch_chunks(None, None, None, None, None, 1, C.byref(rows), C.byref(n)) == 1
    assert L.sid_callable_stitch_chunks(None, None, None, None, None, 0, None, C.byref(n)) == 1


def test_join(sid, cases):
    a = [(b"chr1", 0, 5, 2), (b"chr1", 9, 12, 0)]
    for b, merged in (([(b"chr1", 12, 14, 1), (b"chr2", 0, 1, 0)], True), ([(b"chr1", 13, 14, 1)], False),
                      ([(b"chr2", 12, 14, 1)], False), ([(b"chr1", 11, 14, 1)], False), ([], False)):
        for fa, fb in itertools.product((False, True), repeat=2):
            want = CR.join(a, fa, b, fb)
            assert sid.callable_join(a, b, fa, fb) == want, (b, fa, fb)
            assert (len(want) < len(a) + len(b)) == (merged and fa and fb)
    assert sid.callable_join([], a, True, True) == a and sid.callable_join([], [], True, True) == []
    long = [(b"c" * 40, 0, 3, 1)]
    assert sid.callable_join(long, [(b"c" * 40, 3, 4, 1)], True, True) == [(b"c" * 40, 0, 4, 2)]
    assert sid.callable_join(long, [(b"c" * 39 + b"d", 3, 4, 1)], True, True) == long + [(b"c" * 39 + b"d", 3, 4, 1)]
    # site ranges, as ranks take them: the host rows of every split join to the whole
    s, sites, ds, codes = cases["quirks"]
    code = codes["local"]
    c = np.array(code, np.uint8)
    want = CR.rows(sites, code, ds)
    f = CR.flags(sites, code, ds)
    for k in range(len(sites) + 1):
        left, right = sid.callable_host(s, c, 0, 0, 0, k), sid.callable_host(s, c, 0, 0, k, len(sites))
        assert sid.callable_join(left, right, k > 0 and f[k - 1], k < len(sites) and f[k]) == want, k
    L = sid.lib()
    rows, n = C.POINTER(sid.CallableRow)(), C.c_size_t(0)
    assert L.sid_callable_join(None, 2, 1, None, 0, 1, C.byref(rows), C.byref(n)) == 1
    assert L.sid_callable_join(None, 0, 1, None, 0, 1, None, C.byref(n)) == 1


def test_layouts_stand(sid, tmp_path):
    """sid_callable_row against its ctypes mirror, and sizeof(sid_opts) and sizeof(sid_run_stats) as they
    were before the option (it is a field of neither)."""
    fields = [f for f, _ in sid.CallableRow._fields_]
    assert fields == ["chrom", "chrom_len", "pad", "start", "end", "het"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "sid.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(sid_callable_row));']
    lines += [f'  printf("{f} %zu\\n", offsetof(sid_callable_row, {f}));' for f in fields]
    lines += ['  printf("stats %zu\\n", sizeof(sid_run_stats));', '  printf("opts %zu\\n", sizeof(sid_opts));',
              "  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(exe)],
                   check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(sid.CallableRow) == 40
    for f in fields:
        assert int(got[f]) == getattr(sid.CallableRow, f).offset, f
    assert int(got["stats"]) == C.sizeof(sid.RunStats) == STATS_SIZE
    assert int(got["opts"]) == C.sizeof(sid.Opts) == OPTS_SIZE
    assert sid.RunStats._fields_[-1][0] == "window_rows" and sid.Opts.WINDOW_OFFSET + 4 == OPTS_SIZE


# sizeof(sid_run_stats) and sizeof(sid_opts) of the header before --callable
STATS_SIZE = 256
OPTS_SIZE = 56
