"""--windows W on the host (CPU only): sid_windows_host and sid_windows_format,
the stitch of the chunks' row lists (sid_amd/csrc/windows.cpp) and the
option's rejects, against the Python model of tests/windows_ref.py."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import windows_ref as WR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
WS = [1, 37, 100, WR.WMAX]


def pl(chrom: bytes, pos, bases: bytes = b"." * 30) -> bytes:
    pos = pos if isinstance(pos, bytes) else b"%d" % pos
    return b"%s\t%s\tA\t%d\t%s\t%s\n" % (chrom, pos, len(bases), bases, b"I" * len(bases))


HET = b"." * 15 + b"G" * 15


def quirks_text() -> bytes:
    """The key's quirks, by hand: the same window on a chrom change, positions that go back, a chrom that
    returns, duplicates, pos 0, negative and zero-padded, chroms of 9+ bytes that share 8, chroms that differ
    in length only, coverage below 4."""
    t = [pl(b"chr1", p) for p in (1, 2, 36, 37, 38, 74, 75, 100, 101)]
    t += [pl(b"chr2", p, HET) for p in (1, 2, 3)]                       # the same wi, another chrom
    t += [pl(b"chr1", p) for p in (5, 6)]                               # chr1 returns
    t += [pl(b"chr1", p) for p in (500, 120, 121, 501, 501, 501)]       # back, and duplicates
    t += [pl(b"chr1", p) for p in (0, -1, -36, -37, b"0005", b"-0")]    # atoi's range
    t += [pl(b"chromosome_A", p) for p in (1, 2)] + [pl(b"chromosome_B", p, HET) for p in (1, 2)]
    t += [pl(b"chromosom", 3), pl(b"chromoso", 3), pl(b"chromosom", 3), pl(b"chromosomx", 3)]
    t += [pl(b"chr", 7), pl(b"chr\0"[:3] + b"1", 7), pl(b"ch", 7)]
    t += [pl(b"chrL", p, b".,") for p in (1, 2)] + [pl(b"chrL", 3, HET)]  # coverage 2: no Lynch record
    t += [pl(b"chrZ", WR.WMAX), pl(b"chrZ", WR.WMAX - 1), pl(b"chrZ", 1)]
    return b"".join(t)


def texts():
    out = {"quirks": quirks_text()}
    for k in ("edge", "c1_10k"):
        with open(os.path.join(GOLD, k + ".plp"), "rb") as f:
            out[k] = f.read()
    return out


@pytest.fixture(scope="module")
def cases(sid, oracle):
    """name -> (Sites, [(chrom, pos)], {method: codes})"""
    out = {}
    for name, text in texts().items():
        s = sid.parse_text(text)
        codes = {}
        for method, kw in (("local", {}), ("likelihood_ratio", {"estimate_prior": True})):
            sites, codes[method] = WR.site_codes(sid, oracle, text, method, **kw)
        assert len(s) == len(sites)
        out[name] = (s, sites, codes)
    return out


@pytest.mark.parametrize("w", WS)
def test_host_rows_and_format(sid, cases, w):
    for name, (s, sites, codes) in cases.items():
        for method, code in codes.items():
            want = WR.rows(sites, code, w)
            got = sid.windows_host(s, np.array(code, np.uint8), w)
            assert got == want, (name, method, w)
            assert sum(r[3] for r in got) == len(sites)
            assert sum(r[4] for r in got) == sum(1 for c in code if not c & WR.DROPPED)
            assert all(r[4] == r[5] + r[6] for r in got)
            assert sid.windows_format(got) == WR.fmt(want)
            assert sid.windows_format(got, header=False) == WR.fmt(want, header=False)
    # the Lynch methods print no record below coverage 4: fewer records than sites
    s, sites, codes = cases["quirks"]
    lr = WR.rows(sites, codes["likelihood_ratio"], w)
    assert sum(r[4] for r in lr) < sum(r[3] for r in lr)


def test_quirks_make_the_rows_the_contract_names(cases):
    s, sites, codes = cases["quirks"]
    r = WR.rows(sites, codes["local"], 37)
    chroms = [x[0] for x in r]
    assert chroms.count(b"chr1") >= 6                              # returns, and goes back
    assert (b"chr1", -37, 0) in [x[:3] for x in r]                 # pos 0, -1, -36
    assert (b"chr1", -74, -37) in [x[:3] for x in r]               # pos -37
    assert [x[0] for x in r if x[0].startswith(b"chromoso")] == [b"chromosome_A", b"chromosome_B", b"chromosom",
                                                                b"chromoso", b"chromosom", b"chromosomx"]
    assert [x[3] for x in r if x[:2] == (b"chr1", 481)] == [1, 3]  # 500 | 120 121 | 501 501 501


def test_subrange_and_empty(sid, cases):
    s, sites, codes = cases["quirks"]
    code = np.array(codes["local"], np.uint8)
    for a, b in ((0, 0), (3, 3), (5, 17), (len(sites) - 1, len(sites))):
        assert sid.windows_host(s, code, 37, a, b) == WR.rows(sites[a:b], codes["local"][a:b], 37)
    assert sid.windows_format([]) == WR.HEADER
    assert sid.windows_format([], header=False) == b""


def test_format_sizing_convention(sid):
    L = sid.lib()
    rows = [(b"a,b", -74, -37, 3, 2, 1, 1), (b"", 0, WR.WMAX, 2 ** 40, 2 ** 40, 0, 2 ** 40)]
    want = WR.fmt(rows)
    assert sid.windows_format(rows) == want
    arr = (sid.Window * 2)()
    keep = [C.create_string_buffer(r[0], len(r[0])) for r in rows]
    for k, r in enumerate(rows):
        arr[k] = sid.Window(C.cast(keep[k], C.c_void_p).value, len(r[0]), *r[1:])
    n = C.c_size_t(0)
    assert L.sid_windows_format(arr, 2, 1, None, 0, C.byref(n)) == 3 and n.value == len(want)   # SID_ENOMEM: sizes
    buf = C.create_string_buffer(len(want))
    assert L.sid_windows_format(arr, 2, 1, buf, len(want) - 1, C.byref(n)) == 3 and n.value == len(want)
    assert L.sid_windows_format(arr, 2, 1, buf, len(want), C.byref(n)) == 0 and buf.raw == want
    assert L.sid_windows_format(None, 2, 1, buf, len(want), C.byref(n)) == 1


def stitch_lib(sid, chunks, w):
    L = sid.lib()
    f = L.sid_win_stitch_chunks
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_int,
                  C.POINTER(C.POINTER(sid.Window)), C.POINTER(C.c_size_t)]
    arr, off, names, noff = WR.device_rows(chunks, w)
    rows, n = C.POINTER(sid.Window)(), C.c_size_t(0)
    rc = f(arr, off, names, noff, len(chunks), w, C.byref(rows), C.byref(n))
    assert rc == 0
    try:
        return [(C.string_at(rows[k].chrom, rows[k].chrom_len) if rows[k].chrom_len else b"", rows[k].start,
                 rows[k].end, rows[k].sites, rows[k].records, rows[k].het, rows[k].hom) for k in range(n.value)]
    finally:
        L.sid_windows_free(rows)


def test_stitch_over_every_cut(sid):
    """A small site sequence cut everywhere into up to four chunks (chunks without sites among them): a run
    spanning three chunks adds up, equal keys that are not neighbours stay apart."""
    w = 10
    seq = [(b"chr1", p) for p in (1, 2, 3, 4, 5, 11)] + [(b"chromosome_long", 1)] * 2 + \
          [(b"chr1", 3), (b"chr2", 3), (b"chr1", 4), (b"chr1", 5)]
    codes = [0, WR.HET, WR.DROPPED, 0, WR.HET, 0, 0, WR.HET, 0, 0, WR.DROPPED, WR.HET]
    want = WR.rows(seq, codes, w)
    assert [r[:2] for r in want].count((b"chr1", 0)) == 3   # 1-5, then 3, then 4 5 behind chr2: never merged
    n = len(seq)
    for k in (0, 1, 2, 3):
        for cut in itertools.combinations_with_replacement(range(n + 1), k):
            cuts = [0] + list(cut) + [n]
            chunks = WR.chunk_rows(seq, codes, w, cuts)
            assert WR.stitch(chunks) == want
            assert stitch_lib(sid, chunks, w) == want, cuts
    # one run over three chunks with an empty one between
    chunks = WR.chunk_rows(seq, codes, w, [0, 2, 2, 3, 5, n])
    assert any(not c for c in chunks) and stitch_lib(sid, chunks, w) == want
    assert stitch_lib(sid, [], w) == [] and stitch_lib(sid, [[], []], w) == []


def test_rejects(sid, cases):
    L = sid.lib()
    s, sites, codes = cases["quirks"]
    code = np.array(codes["local"], np.uint8)
    for w in (0, -1):
        with pytest.raises(sid.SidError) as ei:
            sid.windows_host(s, code, w)
        assert ei.value.status == 1
    with pytest.raises(sid.SidError):
        sid.windows_host(s, code, 37, 2, len(sites) + 1)
    # sid_opts.window: negative is SID_EINVAL from sid_engine_create (before any device is touched)
    o = sid.make_opts(window=-1)
    h = C.c_void_p()
    assert L.sid_engine_create(C.byref(o), None, C.byref(h)) == 1 and not h.value
    assert sid.make_opts().window == 0 and sid.make_opts(window=WR.WMAX).window == WR.WMAX
    assert sid.RunStats._fields_[-1][0] == "window_rows"   # appended
    rows, n = C.POINTER(sid.Window)(), C.c_size_t(0)
    assert L.sid_engine_windows(None, C.byref(rows), C.byref(n)) == 1


def test_window_is_the_last_field_of_sid_opts(sid, tmp_path):
    """The Python mirror keeps `window` in the structure's last four bytes (Opts.WINDOW_OFFSET): the header's
    offset and size, from a compiled probe, and a round trip through sid_opts_default."""
    import subprocess
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sid.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", offsetof(sid_opts, window), offsetof(sid_opts, context), sizeof(sid_opts));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(exe)],
                   check=True)
    off, ctx_off, size = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert (off, ctx_off, size) == (sid.Opts.WINDOW_OFFSET, sid.Opts.context.offset, C.sizeof(sid.Opts))
    assert off + 4 == size   # the last field
    o = sid.make_opts(context=3, window=123456)
    assert (o.context, o.window) == (3, 123456)
    sid.lib().sid_opts_default(C.byref(o))
    assert (o.context, o.window) == (0, 0)
