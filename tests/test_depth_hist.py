"""--depth-hist FILE on the host (CPU only): sid_depth_hist_host,
sid_depth_hist_format and sid_depth_hist_merge (sid_amd/csrc/depth_hist.cpp)
against the Python model of tests/depth_hist_ref.py, the identity with the
window rows' column sums, and the layout of sid_depth_row."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depth_hist_ref as DH
import depth_ref
import windows_ref as WR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def texts():
    with open(os.path.join(GOLD, "edge.plp"), "rb") as f:
        edge = f.read()
    ramp = b"".join(DH.depth_line(b"chrR", i + 1, d, i % 3 == 0)
                    for i, d in enumerate(list(range(0, 40)) + [255, 256, 257, 1023, 1024, 1025, 65535, 65536, 131070]))
    return {"edge": edge, "depth": depth_ref.depth_text(700), "deep": depth_ref.deep_text(300), "ramp": ramp}


@pytest.fixture(scope="module")
def cases(sid, oracle):
    """name -> (Sites, [(chrom, pos)], [depth], {method: codes})"""
    out = {}
    for name, text in texts().items():
        s = sid.parse_text(text)
        codes = {}
        for method, kw in (("local", {}), ("likelihood_ratio", {"estimate_prior": True})):
            sites, codes[method] = WR.site_codes(sid, oracle, text, method, **kw)
        ds = DH.depths(s.counts)
        assert len(s) == len(sites) == len(ds)
        out[name] = (s, sites, ds, codes)
    return out


def test_host_rows_and_format(sid, cases):
    for name, (s, sites, ds, codes) in cases.items():
        for method, code in codes.items():
            want = DH.rows(ds, code)
            got = sid.depth_hist_host(s, np.array(code, np.uint8))
            assert got == want, (name, method)
            assert [r[0] for r in got] == sorted({*ds})
            assert sum(r[1] for r in got) == len(sites)
            assert all(r[2] == r[3] + r[4] for r in got)
            assert sid.depth_hist_format(got) == DH.fmt(want)
            assert sid.depth_hist_format(got, header=False) == DH.fmt(want, header=False)
    # the Lynch methods print no record below coverage 4: sites without a record, and only there
    s, sites, ds, codes = cases["depth"]
    lr = DH.rows(ds, codes["likelihood_ratio"])
    low = [r[2] for r in lr if r[0] < 4]
    assert low and not any(low) and all(r[2] == r[1] for r in lr if r[0] >= 4)
    assert (131070, 1, 1) in [r[:3] for r in DH.rows(cases["ramp"][2], cases["ramp"][3]["local"])]


def test_empty_and_newlines(sid):
    for text in (b"", b"\n" * 300):
        s = sid.parse_text(text)
        assert len(s) == 0
        assert sid.depth_hist_host(s, np.zeros(0, np.uint8)) == []
    assert sid.depth_hist_format([]) == DH.HEADER
    assert sid.depth_hist_format([], header=False) == b""


def test_subranges(sid, cases):
    s, sites, ds, codes = cases["depth"]
    code = np.array(codes["local"], np.uint8)
    n = len(sites)
    for a, b in ((0, 0), (3, 3), (5, 17), (0, 7), (n - 1, n), (100, 613)):
        assert sid.depth_hist_host(s, code, a, b) == DH.rows(ds[a:b], codes["local"][a:b]), (a, b)
    # site ranges add up through the merge, as ranks' do
    parts = [sid.depth_hist_host(s, code, a, b) for a, b in ((0, 100), (100, 101), (101, n))]
    got = sid.depth_hist_merge(sid.depth_hist_merge(parts[0], parts[1]), parts[2])
    assert got == DH.rows(ds, codes["local"])


def test_error_returns(sid, cases):
    L = sid.lib()
    s, sites, ds, codes = cases["depth"]
    code = np.array(codes["local"], np.uint8)
    n = len(sites)
    rows, m = C.POINTER(sid.DepthRow)(), C.c_size_t(7)
    p = code.ctypes.data_as(C.c_void_p)
    assert L.sid_depth_hist_host(s.handle, 2, n + 1, p, C.byref(rows), C.byref(m)) == 1 and m.value == 0 and not rows
    assert L.sid_depth_hist_host(s.handle, 5, 4, p, C.byref(rows), C.byref(m)) == 1
    assert L.sid_depth_hist_host(None, 0, 0, p, C.byref(rows), C.byref(m)) == 1
    assert L.sid_depth_hist_host(s.handle, 0, n, None, C.byref(rows), C.byref(m)) == 1
    assert L.sid_depth_hist_host(s.handle, 0, n, p, None, C.byref(m)) == 1
    assert L.sid_depth_hist_host(s.handle, 0, n, p, C.byref(rows), None) == 1
    assert L.sid_depth_hist_host(s.handle, 3, 3, None, C.byref(rows), C.byref(m)) == 0 and m.value == 0   # no site: no code read
    L.sid_depth_hist_free(rows)
    assert L.sid_engine_depth_hist(None, C.byref(rows), C.byref(m)) == 1
    assert L.sid_engine_set_depth_hist(None, 1) == 1
    assert "depth_rows" not in [f for f, _ in sid.RunStats._fields_] and sid.RunStats().depth_rows == 0   # no field


def test_format_sizing_convention(sid):
    L = sid.lib()
    rows = [(0, 3, 2, 1, 1), (7, 2 ** 40, 2 ** 40, 0, 2 ** 40), (DH.DEPTH_MAX, 1, 0, 0, 0)]
    want = DH.fmt(rows)
    assert want == b"depth,sites,records,het,hom\n0,3,2,1,1\n7,%d,%d,0,%d\n262140,1,0,0,0\n" % ((2 ** 40,) * 3)
    assert sid.depth_hist_format(rows) == want
    arr = (sid.DepthRow * 3)(*[sid.DepthRow(r[1], r[2], r[3], r[4], r[0], 0) for r in rows])
    n = C.c_size_t(0)
    assert L.sid_depth_hist_format(arr, 3, 1, None, 0, C.byref(n)) == 3 and n.value == len(want)   # SID_ENOMEM: sizes
    buf = C.create_string_buffer(len(want))
    assert L.sid_depth_hist_format(arr, 3, 1, buf, len(want) - 1, C.byref(n)) == 3 and n.value == len(want)
    assert L.sid_depth_hist_format(arr, 3, 1, buf, len(want), C.byref(n)) == 0 and buf.raw == want
    assert L.sid_depth_hist_format(None, 3, 1, buf, len(want), C.byref(n)) == 1
    assert L.sid_depth_hist_format(arr, 3, 1, buf, len(want), None) == 1


def test_merge(sid):
    a = [(0, 1, 1, 0, 1), (5, 4, 3, 1, 2), (9, 2, 0, 0, 0)]
    disjoint = [(1, 1, 1, 1, 0), (6, 2, 2, 0, 2), (DH.DEPTH_MAX, 1, 1, 0, 1)]
    overlap = [(5, 10, 10, 5, 5), (9, 1, 1, 1, 0), (10, 1, 0, 0, 0)]
    big = [(5, 2 ** 40, 2 ** 40, 2 ** 39, 2 ** 39)]
    for x, y in ((a, disjoint), (a, overlap), (a, a), (a, []), ([], a), ([], []), (a, big), (overlap, disjoint)):
        assert sid.depth_hist_merge(x, y) == DH.merge(x, y), (x, y)
        assert sid.depth_hist_merge(y, x) == DH.merge(x, y)
    for bad in ([(5, 1, 1, 0, 1), (5, 1, 1, 0, 1)], [(6, 1, 1, 0, 1), (5, 1, 1, 0, 1)], a[::-1]):
        for x, y in ((bad, a), (a, bad)):
            with pytest.raises(sid.SidError) as ei:
                sid.depth_hist_merge(x, y)
            assert ei.value.status == 1
    L = sid.lib()
    rows, m = C.POINTER(sid.DepthRow)(), C.c_size_t(0)
    assert L.sid_depth_hist_merge(None, 2, None, 0, C.byref(rows), C.byref(m)) == 1
    assert L.sid_depth_hist_merge(None, 0, None, 0, None, C.byref(m)) == 1


@pytest.mark.parametrize("w", [1, 37, 2 ** 31 - 1])
def test_column_sums_equal_the_window_rows(sid, cases, w):
    for name, (s, sites, ds, codes) in cases.items():
        for method, code in codes.items():
            c = np.array(code, np.uint8)
            d = sid.depth_hist_host(s, c)
            win = sid.windows_host(s, c, w)
            assert DH.sums(d) == DH.sums(win), (name, method, w)
            assert DH.sums(d) == DH.sums(DH.rows(ds, code)) == DH.sums(WR.rows(sites, code, w))


def test_depth_row_layout(sid, tmp_path):
    """sizeof(sid_depth_row) and its offsets from a compiled probe against the ctypes mirror."""
    fields = [f for f, _ in sid.DepthRow._fields_]
    assert fields == ["sites", "records", "het", "hom", "depth", "pad"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "sid.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(sid_depth_row));']
    lines += [f'  printf("{f} %zu\\n", offsetof(sid_depth_row, {f}));' for f in fields]
    lines += ['  printf("stats %zu\\n", sizeof(sid_run_stats));', "  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(exe)],
                   check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(sid.DepthRow) == 40
    for f in fields:
        assert int(got[f]) == getattr(sid.DepthRow, f).offset, f
    assert int(got["stats"]) == C.sizeof(sid.RunStats)   # (the row count is no field of sid_run_stats)
