"""A Python restatement of --variants (sid_opts.variants), for the tests, from
the pileup text and the unselected CSV alone: the reference base is the third
token of a site's line, upper-cased (ASCII); the site's counts are the
oracle's read_bases of its fifth token; a record is a variant when the base
is one of A, C, G, T, one of the counts is not 0 and its gt field is not the
base twice.  Which lines print a record: every line for -m local and
-m quality, coverage >= 4 for the Lynch methods.  Nothing here calls the
library under test."""
import re

import numpy as np

import oracle
from regions_ref import atoi

SEP = re.compile(rb"[ \t]+")


def line_sites(text: bytes):
    """(chrom, pos, ref, counts) of every non-empty line (the tokens on runs of ' ' / '\\t')."""
    out = []
    for ln in text.split(b"\n"):
        ln = ln.split(b"\0")[0]   # (a NUL ends the C string the parser sees)
        if not ln:
            continue
        tok = [t for t in SEP.split(ln) if t]
        assert len(tok) >= 5 and len(tok[2]) == 1, ln
        out.append((tok[0], atoi(tok[1]), tok[2], oracle.read_bases(tok[4], tok[2])))
    return out


def is_variant(ref: bytes, counts, gt: bytes) -> bool:
    r = ref.upper()
    return r in (b"A", b"C", b"G", b"T") and int(np.asarray(counts, np.int64).sum()) >= 1 and gt != r + r


def record_fields(ln: bytes):
    """(chrom, pos, label, gt) of a CSV record, from the right: a chrom may hold commas."""
    f = ln.rsplit(b",", 6)
    return f[0], int(f[1]), f[2], f[3]


def flags(lines, text: bytes, lynch: bool):
    """One bool per record line of the unselected CSV: the record is a variant.  The lines of `text` that
    print a record must pair up one to one, in order, with the records by (chrom, pos)."""
    sites = [s for s in line_sites(text) if not lynch or int(np.asarray(s[3], np.int64).sum()) >= 4]
    assert len(sites) == len(lines), (len(sites), len(lines))
    out = []
    for (chrom, pos, ref, counts), ln in zip(sites, lines):
        c, p, _, gt = record_fields(ln)
        assert (c, p) == (chrom, pos), (chrom, pos, ln)
        out.append(is_variant(ref, counts, gt))
    return out


def filter_csv(csv: bytes, text: bytes, lynch: bool):
    """(header + the variants, kept hom, kept het, dropped hom, dropped het)."""
    lines = csv.splitlines(keepends=True)
    if not lines:
        return b"", 0, 0, 0, 0
    var = flags(lines[1:], text, lynch)
    n = {(k, lab): 0 for k in (True, False) for lab in (b"hom", b"het")}
    for ln, k in zip(lines[1:], var):
        n[(k, record_fields(ln)[2])] += 1
    want = lines[0] + b"".join(ln for ln, k in zip(lines[1:], var) if k)
    return want, n[(True, b"hom")], n[(True, b"het")], n[(False, b"hom")], n[(False, b"het")]


def mark_model(refs, counts, code):
    """sid_variants_mark: the codes (a list of ints) after it."""
    out = []
    for r, c, k in zip(refs, counts, code):
        gt = bytes([b"ACGT"[k & 3], b"ACGT"[(k >> 2) & 3]])
        out.append(k if is_variant(bytes([r]), c, gt) else k | 0x40)
    return out


# ------------------------------------------------------------ the builder --
def vline(chrom: bytes, pos, ref: bytes, bases: bytes, mapq: bool = False) -> bytes:
    pos = pos if isinstance(pos, bytes) else b"%d" % pos
    n = sum(1 for b in bases if b in b".,ACGTacgtNn*")
    ln = b"%s\t%s\t%s\t%d\t%s\t%s" % (chrom, pos, ref, n, bases, b"I" * max(n, 1))
    return ln + (b"\t" + b"5" * max(n, 1) if mapq else b"") + b"\n"


def alts(ref: bytes):
    """Two different bases other than the reference's."""
    r = b"ACGT".find(ref.upper())
    return (b"ACGT"[(r + 1) % 4:(r + 1) % 4 + 1], b"ACGT"[(r + 2) % 4:(r + 2) % 4 + 1]) if r >= 0 else (b"G", b"A")


KINDS = ("homalt", "hetref", "hetalt", "star", "cov2", "homref")


def bases_of(kind: str, ref: bytes, depth: int = 30) -> bytes:
    a, b = alts(ref)
    h = depth // 2
    return {"homalt": a * depth, "hetref": b"." * h + a * (depth - h), "hetalt": a * h + b * (depth - h),
            "star": b"*", "cov2": a * 2, "homref": b"." * h + b"," * (depth - h)}[kind]


def base_kind(i: int) -> str:
    return {0: "homalt", 7: "hetref", 13: "hetalt", 20: "star", 21: "cov2"}.get(i % 61, "homref")


def base_ref(i: int) -> bytes:
    return b"ACGTacgtN"[i % 9:i % 9 + 1]


def base_text(n: int = 6000, chrom=lambda i: b"chr1", mapq: bool = False, depth: int = 30) -> bytes:
    """The base input: n lines, pos i, the reference byte b"ACGTacgtN"[i % 9], the read bases by i % 61."""
    return b"".join(vline(chrom(i), i, base_ref(i), bases_of(base_kind(i), base_ref(i), depth), mapq)
                    for i in range(1, n + 1))


def placement_text(kind: str, n: int = 6000) -> bytes:
    """n lines at 30x where the test decides which sites are variants (as test_select_gpu.placement_text
    places hets): the variants hom-alt and, every third, het; the others hom-ref and, but for `every`, now and
    then a het on an N reference (a het record that is dropped).  `none`: no variant at all."""
    var = {
        "none": lambda i: False,
        "every": lambda i: True,
        "second": lambda i: i % 2 == 0,
        "61st": lambda i: i % 61 == 0,
        "runs70": lambda i: (i // 70) % 9 == 3,
        "last100": lambda i: i > n - 100,
    }[kind]
    out, j = [], 0
    for i in range(1, n + 1):
        ref = b"ACGTacgt"[i % 8:i % 8 + 1]
        if var(i):
            j += 1
            out.append(vline(b"chr1", i, ref, bases_of("hetref" if j % 3 == 0 else "homalt", ref)))
        elif i % 97 == 5:
            out.append(vline(b"chr1", i, b"N", bases_of("hetalt", b"N")))
        else:
            out.append(vline(b"chr1", i, ref, bases_of("homref", ref)))
    return b"".join(out)
