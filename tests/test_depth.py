"""The depth bounds on the host (sid_depth_mark + sid_format_csv -- the
--host-parse path) and in the binding (depth_mark).  CPU.

The expected results come from tests/depth_ref.py, the rule restated in Python
from the pileup text: a site's depth is the sum of the counts the oracle's
read_bases gives, and a record stays when min <= depth and (max == 0 or depth
<= max)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depth_ref as D
import variants_ref as V
from context_ref import mark_model as context_model
from regions_ref import bed_runs, text_sites
from test_select import golden_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = [("local", False), ("local", True), ("likelihood_ratio", True), ("bayes", False)]


@pytest.fixture(scope="module")
def texts():
    return {"depth": D.depth_text(), "deep": D.deep_text()}


def test_the_builders_depths(texts):
    """The texts hold the depths the bounds are chosen around (and a few the kinds of site fix: one '*', two
    bases, '.' and ',' on an N reference)."""
    d = D.depths(texts["depth"])
    assert len(d) == 3000 and set(D.DEPTHS) <= set(d) and max(d) == 90 and min(d) == 0
    d = D.depths(texts["deep"])
    assert len(d) == 2500 and set(D.DEEP) <= set(d) and max(d) == 300


@pytest.mark.parametrize("method,prior", METHODS, ids=lambda v: str(v))
@pytest.mark.parametrize("name,bounds", [("depth", D.BOUNDS), ("deep", D.DEEP_BOUNDS)])
def test_depth_mark_equals_the_model(sid, oracle, texts, name, bounds, method, prior):
    sites = sid.parse_text(texts[name])
    n = len(sites)
    rc, code, hom, het, _, _ = oracle.call_method(sites.counts, method, estimate_prior=prior)
    assert rc == 0
    assert [int(c.sum()) for c in sites.counts.astype(np.int64)] == D.depths(texts[name])
    for lo, hi in bounds + ((0, 0), (91, 0) if name == "depth" else (301, 0), (0, D.DEPTH_MAX)):
        want = np.array(D.mark_model(sites.counts, code, lo, hi), np.uint8)
        got = sid.depth_mark(sites, code, lo, hi)
        assert (got == want).all(), (lo, hi)
        assert ((got & 0xBF) == (code & 0xBF)).all()   # only the "no record" bit is added
        rec = (code & 0x40) == 0
        kept, dropped = rec & ((got & 0x40) == 0), rec & ((got & 0x40) != 0)
        het_ = (code & 0x80) != 0
        if (lo, hi) in bounds:   # the four-way cases
            assert (kept & het_).any() and (kept & ~het_).any() and (dropped & het_).any() and (dropped & ~het_).any(), \
                (name, method, lo, hi)
        elif (lo, hi) in ((0, 0), (0, D.DEPTH_MAX)):
            assert (got == code).all()
        else:
            assert not kept.any() and (got & 0x40).all()
        # ranges: [begin, end) alone, the rest untouched
        for b, e in ((0, 0), (0, 1), (17, 2000), (n - 1, n), (n, n)):
            part = sid.depth_mark(sites, code, lo, hi, b, e)
            assert (part == np.array(D.mark_model(sites.counts, code, lo, hi, b, e), np.uint8)).all()
            assert (part[:b] == code[:b]).all() and (part[e:] == code[e:]).all()


def test_the_order_with_the_other_marks(sid, oracle, texts):
    """A site another mark dropped stays dropped, the marks commute, and sid_context_mark behind them sees
    what all of them keep."""
    text = texts["depth"]
    sites = sid.parse_text(text)
    rc, code, _, _, _, _ = oracle.call_method(sites.counts, "local")
    assert rc == 0
    r = sid.Regions(bed_runs(text_sites(text), lambda i: (i // 70) % 3 == 1))
    lo, hi = 8, 31
    d = sid.depth_mark(sites, code, lo, hi)
    for select in ("het", "hom"):
        others = sid.variants_mark(sites, sid.regions_mark(sites, sid.select_mark(code, select), r))
        a = sid.depth_mark(sites, others, lo, hi)
        b = sid.variants_mark(sites, sid.regions_mark(sites, sid.select_mark(d, select), r))
        assert (a == b).all()
        assert ((a & 0x40) >= (others & 0x40)).all() and ((a & 0x40) >= (d & 0x40)).all()   # dropped stays dropped
        assert ((a & 0x40) == ((others | d) & 0x40)).all()                                  # ... and nothing else is
        assert ((a & 0x40) == 0).any() and ((a & 0x40) != (others & 0x40)).any() and ((a & 0x40) != (d & 0x40)).any()
        cx = sid.context_mark(code, a, 2)
        assert (cx == np.array(context_model([int(c) for c in code], [int(c) for c in a], 2), np.uint8)).all()
        assert ((cx & 0x40) == 0).sum() > ((a & 0x40) == 0).sum()
    r.close()


def test_depth_mark_rejects(sid, texts):
    sites = sid.parse_text(texts["depth"])
    n = len(sites)
    code = np.zeros(n, np.uint8)
    L = sid.lib()
    p = code.ctypes.data_as(C.c_void_p)
    assert L.sid_depth_mark(sites.handle, 0, n, 0, 0, p) == 0
    assert L.sid_depth_mark(sites.handle, 0, n, 262140, 262140, p) == 0 and (code == 0x40).all()
    code[:] = 0
    for lo, hi in ((-1, 0), (262141, 0), (0, -1), (0, 262141), (9, 8), (262140, 1), (-5, -5), (1 << 30, 0)):
        assert L.sid_depth_mark(sites.handle, 0, n, lo, hi, p) == 1, (lo, hi)   # SID_EINVAL: bad bounds
    assert not code.any()
    assert L.sid_depth_mark(sites.handle, 0, n + 1, 1, 0, p) == 1     # a range outside the sites
    assert L.sid_depth_mark(sites.handle, n + 1, n + 1, 1, 0, p) == 1
    assert L.sid_depth_mark(sites.handle, 5, 4, 1, 0, p) == 1
    assert L.sid_depth_mark(None, 0, 1, 1, 0, p) == 1                  # NULL pointers
    assert L.sid_depth_mark(sites.handle, 0, 4, 1, 0, None) == 1
    assert not code.any()
    with pytest.raises(sid.SidError):
        sid.depth_mark(sites, code[:5], 1, 0)
    with pytest.raises(sid.SidError) as ei:
        sid.depth_mark(sites, code, 9, 8)
    assert ei.value.status == 1


@pytest.mark.parametrize("bounds", D.BOUNDS + ((91, 0), (0, 0)), ids=str)
def test_depth_mark_and_format_csv_give_the_filtered_oracle_csv(sid, oracle, texts, tmp_path, bounds):
    text = texts["depth"]
    p = tmp_path / "depth.plp"
    p.write_bytes(text)
    b = oracle.run_cli([str(p)])
    assert b.returncode == 0
    csv = b.stdout
    header = csv.splitlines(keepends=True)[0]
    sites = sid.parse_text(text)
    code, hom, het, conf_type = golden_arrays(sites, csv)
    assert header + sid.format_csv(sites, code, hom, het, conf_type) == csv, "the test's own reconstruction"
    want, khom, khet, dhom, dhet = D.filter_csv(csv, text, False, *bounds)
    if bounds in D.BOUNDS:
        assert min(khom, khet, dhom, dhet) >= 1
    elif bounds == (0, 0):
        assert want == csv
    else:
        assert want == header
    marked = sid.depth_mark(sites, code, *bounds)
    assert header + sid.format_csv(sites, marked, hom, het, conf_type) == want


def test_the_abi_did_not_grow(tmp_path):
    """The bounds are set by calls, not by fields: sid_opts and sid_run_stats keep the sizes they had."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "sid.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(sid_opts), sizeof(sid_run_stats)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [56, 256]


def test_the_binding_has_the_setters(sid):
    L = sid.lib()
    for name in ("sid_depth_mark", "sid_set_depth", "sid_engine_set_depth"):
        assert getattr(L, name) is not None
    assert L.sid_set_depth(None, 0, 0) == 1 and L.sid_engine_set_depth(None, 0, 0) == 1   # NULL: SID_EINVAL
    assert C.sizeof(sid.Opts) == 56 and not hasattr(sid.Opts, "min_depth")
