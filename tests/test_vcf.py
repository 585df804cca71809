"""The VCF format on the host (sid_format_vcf, sid_vcf_header -- the
--host-parse path) and in the binding (format_vcf, vcf_header).  CPU.

The expected bytes come from tests/vcf_ref.py: section "VCF" of sid.h's
Conventions restated in Python from the pileup text and the oracle's CSV.  The
golden input's CSVs are the committed ones; edge.plp's and the built text's are
the oracle CLI's."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import variants_ref as V
import vcf_ref as F
from test_select import golden_arrays

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
# flag set -> (the oracle CLI's flags, a Lynch method: no record below coverage 4, the header's conf type)
FLAGSETS = {
    "local": ([], False, b"p_value", dict(method="local")),
    "local_R": (["-R", "-m", "local"], False, b"p_value", dict(method="local", estimate_prior=True)),
    "lr": (["-R", "-m", "likelihood_ratio"], True, b"p_value", dict(method="likelihood_ratio", estimate_prior=True)),
    "bayes": (["-m", "bayes"], True, b"probability", dict(method="bayes")),
}
ENOMEM, EINVAL = 3, 1


def built_text() -> bytes:
    """variants_ref's base input (every reference byte, hom-alt, het with and without the reference, '*' alone,
    two bases) with a second chrom of 70 bytes and positions atoi reads as 0 and below."""
    t = V.base_text(1500) + V.base_text(300, chrom=lambda i: b"L" * 70)
    return t + V.vline(b"chrZ", b"0", b"a", b"G" * 20) + V.vline(b"chrZ", b"-17", b"n", b"." * 9 + b"T" * 9) + \
        V.vline(b"chrZ", b"x9", b"T", b"CCCCCAAAAA")


def covers(vcf: bytes, lynch: bool):
    """Every genotype and a REF N occur (a Lynch method prints nothing below coverage 4, so never "./.")."""
    g, refn = F.kinds(vcf)
    assert (F.ALL_KINDS - ({b"./."} if lynch else set())) <= g and refn, (sorted(g), refn)


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    """{(input, flag set): (text, the oracle's CSV)}."""
    d = tmp_path_factory.mktemp("vcf")
    out = {}
    with open(os.path.join(GOLD, "c1_10k.plp"), "rb") as f:
        gold = f.read()
    with open(os.path.join(GOLD, "edge.plp"), "rb") as f:
        edge = f.read()
    for fs, (flags, _, _, _) in FLAGSETS.items():
        out[("c1_10k", fs)] = (gold, gzip.open(os.path.join(GOLD, f"c1_10k.{fs}.csv.gz")).read())
        for name, text in (("edge", edge), ("built", built_text())):
            p = d / f"{name}.plp"
            p.write_bytes(text)
            b = oracle.run_cli(flags + [str(p)])
            assert b.returncode == 0, b.stderr[-300:]
            out[(name, fs)] = (text, b.stdout)
    return out


@pytest.mark.parametrize("fs", sorted(FLAGSETS))
@pytest.mark.parametrize("name", ["c1_10k", "edge", "built"])
def test_format_vcf_equals_the_restatement(sid, cases, name, fs):
    text, csv = cases[(name, fs)]
    lynch = FLAGSETS[fs][1]
    sites = sid.parse_text(text)
    code, hom, het, conf_type = golden_arrays(sites, csv)
    assert sid.HEADER + sid.format_csv(sites, code, hom, het, conf_type) == csv, "the test's own reconstruction"
    want = F.map_csv(csv, text, lynch)
    assert want.count(b"\n") == csv.count(b"\n") - 1 > 0
    if name == "built":
        covers(want, lynch)
    got = sid.format_vcf(sites, code, hom, het)
    assert got == want
    # ranges: the records of sites [begin, end) alone
    n = len(sites)
    for b, e in ((0, 0), (0, 1), (n // 3, n // 2), (n - 1, n), (n, n)):
        part = code.copy()
        part[:b] |= 0x40
        part[e:] |= 0x40
        assert sid.format_vcf(sites, code, hom, het, b, e) == sid.format_vcf(sites, part, hom, het)
    # a mark drops the line the CSV formatter drops
    het_only = sid.select_mark(code, "het")
    keep = [V.record_fields(ln)[2] == b"het" for ln in csv.splitlines()[1:]]
    assert sid.format_vcf(sites, het_only, hom, het) == F.map_csv(csv, text, lynch, keep)


def test_the_built_text_covers_every_kind(cases):
    text, csv = cases[("built", "local")]
    lines, vcf = F.vcf_lines(csv, text, False)
    F.assert_covers(b"".join(vcf))
    assert vcf[-3].startswith(b"chrZ\t0\t.\tA\tG\t.\t.\tDP=20;") and vcf[-3].endswith(b"\tGT\t1/1\n")
    assert vcf[-2].startswith(b"chrZ\t-17\t.\tN\tT\t.\t.\tDP=9;")   # '.' on an N reference counts nothing
    assert vcf[-1].startswith(b"chrZ\t0\t.\tT\t")                  # atoi("x9") = 0
    assert any(ln.startswith(b"L" * 70 + b"\t") for ln in vcf)


def test_header(sid):
    version = sid.lib().sid_version()
    for fs, (_, _, conf_type, opts) in FLAGSETS.items():
        h = sid.vcf_header(**opts)
        F.check_header(h, version, conf_type)
        assert h == F.header(version, conf_type)
    assert sid.vcf_header(method="quality") == F.header(version, b"p_value")
    # the sizing protocol of sid_format_csv: SID_ENOMEM and a sufficient length
    L = sid.lib()
    o = sid.make_opts(method="bayes")
    need = C.c_size_t(0)
    assert L.sid_vcf_header(C.byref(o), None, 0, C.byref(need)) == ENOMEM and need.value == len(F.header(version, b"probability"))
    buf = C.create_string_buffer(need.value + 8)
    buf.raw = b"\xAA" * (need.value + 8)
    small = C.c_size_t(0)
    assert L.sid_vcf_header(C.byref(o), buf, need.value - 1, C.byref(small)) == ENOMEM and small.value == need.value
    assert buf.raw == b"\xAA" * (need.value + 8)
    ln = C.c_size_t(0)
    assert L.sid_vcf_header(C.byref(o), buf, need.value, C.byref(ln)) == 0 and ln.value == need.value
    assert buf.raw[:need.value] == F.header(version, b"probability") and buf.raw[need.value:] == b"\xAA" * 8
    assert L.sid_vcf_header(None, buf, need.value, C.byref(ln)) == EINVAL
    assert L.sid_vcf_header(C.byref(o), buf, need.value, None) == EINVAL


def test_sizing_and_rejects(sid, cases):
    text, csv = cases[("built", "local")]
    sites = sid.parse_text(text)
    n = len(sites)
    code, hom, het, _ = golden_arrays(sites, csv)
    want = F.map_csv(csv, text, False)
    L = sid.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    need, ln = C.c_size_t(0), C.c_size_t(0)
    assert L.sid_format_vcf(sites.handle, 0, n, p(code), p(hom), p(het), None, 0, C.byref(need)) == ENOMEM
    assert need.value >= len(want)
    buf = C.create_string_buffer(need.value)
    assert L.sid_format_vcf(sites.handle, 0, n, p(code), p(hom), p(het), buf, need.value - 1, C.byref(ln)) == ENOMEM
    assert ln.value == need.value
    assert L.sid_format_vcf(sites.handle, 0, n, p(code), p(hom), p(het), buf, need.value, C.byref(ln)) == 0
    assert buf.raw[:ln.value] == want
    # every site dropped: no byte, whatever the capacity's worth
    none = np.full(n, 0x40, np.uint8)
    assert L.sid_format_vcf(sites.handle, 0, n, p(none), p(hom), p(het), buf, need.value, C.byref(ln)) == 0 and ln.value == 0
    for args in ((None, 0, n, p(code), p(hom), p(het), buf, need.value, C.byref(ln)),
                 (sites.handle, 0, n, None, p(hom), p(het), buf, need.value, C.byref(ln)),
                 (sites.handle, 0, n, p(code), None, p(het), buf, need.value, C.byref(ln)),
                 (sites.handle, 0, n, p(code), p(hom), None, buf, need.value, C.byref(ln)),
                 (sites.handle, 0, n, p(code), p(hom), p(het), buf, need.value, None),
                 (sites.handle, 0, n + 1, p(code), p(hom), p(het), buf, need.value, C.byref(ln)),
                 (sites.handle, n + 1, n + 1, p(code), p(hom), p(het), buf, need.value, C.byref(ln)),
                 (sites.handle, 5, 4, p(code), p(hom), p(het), buf, need.value, C.byref(ln))):
        assert L.sid_format_vcf(*args) == EINVAL


def test_the_worst_case_record(sid):
    """1/2, a 70-byte chrom, an 11-byte position and both confidences 13 bytes: the literal line."""
    chrom = b"W" * 70
    text = V.vline(chrom, b"-2147483648", b"t", b"C" * 15 + b"g" * 15)
    sites = sid.parse_text(text)
    assert len(sites) == 1 and int(sites.positions[0]) == -2**31 and int(sites.counts[0].sum()) == 30
    code = np.array([1 | (2 << 2) | 0x80], np.uint8)             # het,CG
    hom, het = np.array([-4.94066e-324]), np.array([-1.23457e-300])
    assert sid.format_csv(sites, code, hom, het) == chrom + b",-2147483648,het,CG,-4.94066e-324,-1.23457e-300,p_value\n"
    got = sid.format_vcf(sites, code, hom, het)
    assert got == chrom + b"\t-2147483648\t.\tT\tC,G\t.\t.\tDP=30;HOM=-4.94066e-324;HET=-1.23457e-300\tGT\t1/2\n"
    assert len(got) == 70 + 78 - 4   # (the fixed part's 67 + the position's 11, less four of DP's six digits)
    for v, s in ((float("nan"), b"nan"), (-float("nan"), b"-nan"), (float("inf"), b"inf"), (1.0, b"1"), (0.0, b"0")):
        ln = sid.format_vcf(sites, code, np.array([v]), np.array([v]))
        assert b";HOM=%s;HET=%s\tGT" % (s, s) in ln, ln


def test_every_new_symbol_is_exported(sid):
    L = sid.lib()
    for name in ("sid_set_format", "sid_engine_set_format", "sid_format_vcf", "sid_vcf_header"):
        assert getattr(L, name) is not None
    assert L.sid_set_format(None, 1) == EINVAL and L.sid_engine_set_format(None, 1) == EINVAL
    assert sid.FORMATS == {"csv": 0, "vcf": 1}
    assert C.sizeof(sid.Opts) == 56 and not hasattr(sid.Opts, "format")
    with pytest.raises(sid.SidError) as ei:
        sid.Engine(format="bcf")   # (refused in the binding, before anything is created)
    assert "format" in str(ei.value)
