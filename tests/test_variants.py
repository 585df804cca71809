"""--variants on the host (the parser's reference bytes, sid_variants_mark +
sid_format_csv -- the --host-parse path) and in the binding (Sites.refs,
variants_mark, Opts.variants).  CPU.

The expected results come from tests/variants_ref.py, the rule restated in
Python from the pileup text: the third token upper-cased, the counts by the
oracle's read_bases, the gt field of the record."""
import ctypes as C
import os

import numpy as np
import pytest

import variants_ref as V
from regions_ref import bed_runs, text_sites
from test_select import golden_arrays

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
METHODS = [("local", False), ("local", True), ("likelihood_ratio", True), ("likelihood_ratio", False), ("bayes", False)]


def gold(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def texts():
    return {"edge": gold("edge.plp"), "c1": gold("c1_10k.plp"), "base": V.base_text(),
            "second": V.placement_text("second", 700),
            "chroms": V.base_text(900, chrom=lambda i: [b"chrA", b"chrom_12", b"chrom_123", b"chromosome12"][i // 37 % 4]),
            "spaces": b"".join(b"  c \t %d \t%s  5\t....%s\tIIIII\n" % (i, r, r) for i, r in
                               enumerate([b"A", b"c", b"N", b"*", b"t", b"R", b"n", b"G"], 1))}


@pytest.mark.parametrize("name", ["edge", "c1", "base", "second", "chroms", "spaces"])
def test_sites_refs_are_the_third_tokens(sid, texts, name):
    text = texts[name]
    sites = sid.parse_text(text)
    want = [s[2] for s in V.line_sites(text)]
    assert len(want) == len(sites) >= 8
    assert sites.refs.dtype == np.uint8 and sites.refs.tobytes() == b"".join(want)
    # ... and do not depend on how the text is split over the parser's threads
    assert sid.parse_text(text, threads=7).refs.tobytes() == sites.refs.tobytes()
    if name == "base":
        assert set(want) == set(bytes([c]) for c in b"ACGTacgtN")


def test_no_sites_no_refs(sid):
    assert sid.parse_text(b"").refs.size == 0 and sid.parse_text(b"\n\n").refs.size == 0
    assert sid.lib().sid_sites_refs(None) is None


@pytest.mark.parametrize("method,prior", METHODS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", ["base", "c1"])
def test_variants_mark_equals_the_model(sid, oracle, texts, name, method, prior):
    sites = sid.parse_text(texts[name])
    rc, code, hom, het, _, _ = oracle.call_method(sites.counts, method, estimate_prior=prior)
    assert rc == 0
    want = np.array(V.mark_model(sites.refs, sites.counts, [int(c) for c in code]), np.uint8)
    got = sid.variants_mark(sites, code)
    assert (got == want).all()
    assert ((got & 0xBF) == (code & 0xBF)).all()   # only the "no record" bit is added
    rec = (code & 0x40) == 0
    kept, dropped = rec & ((got & 0x40) == 0), rec & ((got & 0x40) != 0)
    if name == "base":   # (the goldens: a synthetic sample on its own reference, few hom-alt sites)
        het_ = (code & 0x80) != 0
        assert (kept & het_).any() and (kept & ~het_).any() and (dropped & het_).any() and (dropped & ~het_).any()
        if method == "local":
            assert (int((kept & ~het_).sum()), int((kept & het_).sum()), int((dropped & ~het_).sum()),
                    int((dropped & het_).sum())) == (175, 176, 5638, 11)
    else:
        assert kept.any() and dropped.any()
    # ranges: [begin, end) alone, the rest untouched
    n = len(sites)
    for b, e in ((0, 0), (0, 1), (17, 4000), (n - 1, n), (n, n)):
        part = sid.variants_mark(sites, code, b, e)
        assert (part[b:e] == want[b:e]).all() and (part[:b] == code[:b]).all() and (part[e:] == code[e:]).all()


@pytest.mark.parametrize("flags", [[], ["-m", "bayes"]], ids=["local", "bayes"])
def test_variants_mark_and_format_csv_give_the_filtered_oracle_csv(sid, oracle, texts, tmp_path, flags):
    text = texts["base"]
    p = tmp_path / "base.plp"
    p.write_bytes(text)
    b = oracle.run_cli(flags + [str(p)])
    assert b.returncode == 0
    csv = b.stdout
    header = csv.splitlines(keepends=True)[0]
    sites = sid.parse_text(text)
    code, hom, het, conf_type = golden_arrays(sites, csv)
    assert header + sid.format_csv(sites, code, hom, het, conf_type) == csv, "the test's own reconstruction"
    want, khom, khet, dhom, dhet = V.filter_csv(csv, text, bool(flags))
    assert min(khom, khet, dhom, dhet) >= 1
    marked = sid.variants_mark(sites, code)
    assert header + sid.format_csv(sites, marked, hom, het, conf_type) == want


def test_the_marks_commute(sid, oracle, texts):
    text = texts["base"]
    sites = sid.parse_text(text)
    rc, code, _, _, _, _ = oracle.call_method(sites.counts, "local")
    assert rc == 0
    r = sid.Regions(bed_runs(text_sites(text), lambda i: (i // 70) % 3 == 1))
    v = sid.variants_mark(sites, code)
    for select in ("het", "hom"):
        a = sid.select_mark(v, select)
        b = sid.variants_mark(sites, sid.select_mark(code, select))
        assert (a == b).all() and ((a & 0x40) == 0).any() and ((a & 0x40) != (v & 0x40)).any()
        c = sid.regions_mark(sites, a, r)
        d = sid.variants_mark(sites, sid.regions_mark(sites, sid.select_mark(code, select), r))
        e = sid.select_mark(sid.regions_mark(sites, v, r), select)
        assert (c == d).all() and (c == e).all() and ((c & 0x40) == 0).any() and ((c & 0x40) != (a & 0x40)).any()
    r.close()


def test_variants_mark_rejects(sid, texts):
    sites = sid.parse_text(texts["second"])
    n = len(sites)
    code = np.zeros(n, np.uint8)
    L = sid.lib()
    p = code.ctypes.data_as(C.c_void_p)
    assert L.sid_variants_mark(sites.handle, 0, n, p) == 0
    assert L.sid_variants_mark(sites.handle, 0, n + 1, p) == 1    # a range outside the sites
    assert L.sid_variants_mark(sites.handle, n + 1, n + 1, p) == 1
    assert L.sid_variants_mark(sites.handle, 5, 4, p) == 1
    assert L.sid_variants_mark(None, 0, 1, p) == 1                # NULL pointers
    assert L.sid_variants_mark(sites.handle, 0, 4, None) == 1
    assert L.sid_variants_mark(sites.handle, 7, 7, None) == 0     # (an empty range reads no code)
    with pytest.raises(sid.SidError):
        sid.variants_mark(sites, code[:5])


def test_opts_default_leaves_variants_off(sid):
    assert sid.make_opts().variants == 0
    assert sid.make_opts(variants=1).variants == 1 and sid.make_opts(variants=True).variants == 1
    o = sid.Opts()
    o.variants = 7
    o.window = 9
    sid.lib().sid_opts_default(C.byref(o))
    assert (o.variants, o.window, o.select, o.context) == (0, 0, 0, 0)
    # the field fills what was padding: the structure's size and its other fields' offsets stand
    assert sid.Opts.variants.offset == sid.Opts.select.offset + 4 and sid.Opts.regions.offset == 40
    assert C.sizeof(sid.Opts) == sid.Opts.WINDOW_OFFSET + 4
