"""A Python restatement of the VCF format (--vcf, sid_set_format), for the
tests, from the pileup text and the oracle's CSV alone (include/sid.h,
Conventions "VCF"): a VCF line for exactly the CSV's records, in their order,
each a pure function of its CSV record, its site's reference byte and its
site's depth.  The sites pair with the records as variants_ref.flags and
depth_ref.record_depths pair them.  Nothing here calls the library under
test."""
import numpy as np

import depth_ref as D
import variants_ref as V

COLUMNS = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"


def header(version: bytes, conf_type: bytes = b"p_value") -> bytes:
    """The header that replaces the CSV's header line; `version` is sid_version()."""
    return (b"##fileformat=VCFv4.2\n"
            b"##source=" + version + b"\n"
            b"##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Counted bases A+C+G+T of the site's profile\">\n"
            b"##INFO=<ID=HOM,Number=1,Type=Float,Description=\"Confidence of the homozygous call (hom_conf)\">\n"
            b"##INFO=<ID=HET,Number=1,Type=Float,Description=\"Confidence of the heterozygous call (het_conf)\">\n"
            b"##sidConfType=" + conf_type + b"\n"
            b"##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" + COLUMNS)


def check_header(h: bytes, version: bytes, conf_type: bytes):
    """What the issue fixes of the header, whatever the descriptions say."""
    lines = h.split(b"\n")
    assert h.endswith(b"\n") and lines[0] == b"##fileformat=VCFv4.2" and lines[1] == b"##source=" + version
    assert lines[-2] + b"\n" == COLUMNS
    meta = lines[2:-2]
    for key, typ in ((b"DP", b"Integer"), (b"HOM", b"Float"), (b"HET", b"Float")):
        assert sum(1 for m in meta if m.startswith(b"##INFO=<ID=" + key + b",") and b"Type=" + typ in m) == 1, key
    assert sum(1 for m in meta if m.startswith(b"##FORMAT=<ID=GT,")) == 1
    assert meta.count(b"##sidConfType=" + conf_type) == 1
    assert not any(m.startswith(b"##contig") for m in meta)
    assert all(m.startswith(b"##") for m in meta)


def ref_base(ref: bytes) -> bytes:
    r = ref.upper()
    return r if r in (b"A", b"C", b"G", b"T") else b"N"


def alleles(ref: bytes, gt: bytes, depth: int):
    """(ALT, <g>) of a record with reference byte REF (upper-cased or N already)."""
    if depth == 0:
        return b".", b"./."
    alt = []
    for b in (gt[0:1], gt[1:2]):
        if b != ref and b not in alt:
            alt.append(b)
    num = [0 if b == ref else 1 + alt.index(b) for b in (gt[0:1], gt[1:2])]
    return (b",".join(alt) if alt else b"."), b"%d/%d" % (min(num), max(num))


def csv_fields(ln: bytes):
    """(chrom, pos bytes, label, gt, hom_conf, het_conf) of a CSV record, from the right: a chrom may hold commas."""
    f = ln.rstrip(b"\n").rsplit(b",", 6)
    return f[0], f[1], f[2], f[3], f[4], f[5]


def vcf_line(csv_line: bytes, ref: bytes, depth: int) -> bytes:
    chrom, pos, _, gt, hom, het = csv_fields(csv_line)
    r = ref_base(ref)
    alt, g = alleles(r, gt, depth)
    return b"\t".join((chrom, pos, b".", r, alt, b".", b".", b"DP=%d;HOM=%s;HET=%s" % (depth, hom, het), b"GT", g)) + b"\n"


def record_sites(lines, text: bytes, lynch: bool):
    """(ref byte, depth) per record line of the unselected CSV (no header): the lines of `text` that print a
    record pair up one to one, in order, with the records by (chrom, pos)."""
    sites = [(s, int(np.asarray(s[3], np.int64).sum())) for s in V.line_sites(text)]
    sites = [(s, d) for s, d in sites if not lynch or d >= 4]
    assert len(sites) == len(lines), (len(sites), len(lines))
    out = []
    for ((chrom, pos, ref, _), d), ln in zip(sites, lines):
        c, p, _, _ = V.record_fields(ln)
        assert (c, p) == (chrom, pos), (chrom, pos, ln)
        out.append((ref, d))
    assert [d for _, d in out] == D.record_depths(lines, text, lynch)
    return out


def vcf_lines(csv: bytes, text: bytes, lynch: bool):
    """The CSV's record lines (header dropped) and their VCF lines, one to one."""
    lines = csv.splitlines(keepends=True)[1:]
    return lines, [vcf_line(ln, ref, d) for ln, (ref, d) in zip(lines, record_sites(lines, text, lynch))]


def map_csv(csv: bytes, text: bytes, lynch: bool, keep=None) -> bytes:
    """The VCF records (no header) of the unselected CSV `csv`; keep: one bool per record (a selection
    restated by another *_ref module), else every record."""
    _, v = vcf_lines(csv, text, lynch)
    return b"".join(ln for k, ln in enumerate(v) if keep is None or keep[k])


def kinds(vcf: bytes):
    """The genotypes and whether a REF N occurs, for the tests' non-vacuity checks."""
    g, refn = set(), False
    for ln in vcf.splitlines():
        if ln.startswith(b"#"):
            continue
        f = ln.split(b"\t")
        g.add(f[-1])
        refn = refn or f[-7] == b"N"
    return g, refn


ALL_KINDS = {b"0/0", b"0/1", b"1/1", b"1/2", b"./."}


def assert_covers(vcf: bytes):
    g, refn = kinds(vcf)
    assert ALL_KINDS <= g and refn, (sorted(g), refn)
