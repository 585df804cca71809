"""A Python restatement of the depth bounds (--min-depth / --max-depth,
sid_set_depth), for the tests, from the pileup text and the unselected CSV
alone: a site's depth is the sum of the four counts the oracle's read_bases
gives for its fifth token under its third; a record is kept when min <= depth
and (max == 0 or depth <= max).  Which lines print a record: every line for
-m local and -m quality, coverage >= 4 for the Lynch methods (variants_ref.flags
pairs them the same way).  Nothing here calls the library under test."""
import numpy as np

import variants_ref as V

DEPTH_MAX = 262140   # 4 x 65535


def inside(depth: int, lo: int, hi: int) -> bool:
    return lo <= depth and (hi == 0 or depth <= hi)


def depths(text: bytes):
    """The depth of every non-empty line."""
    return [int(np.asarray(s[3], np.int64).sum()) for s in V.line_sites(text)]


def record_depths(lines, text: bytes, lynch: bool):
    """One depth per record line of the unselected CSV.  The lines of `text` that print a record must pair up
    one to one, in order, with the records by (chrom, pos)."""
    sites = [(s, int(np.asarray(s[3], np.int64).sum())) for s in V.line_sites(text)]
    sites = [(s, d) for s, d in sites if not lynch or d >= 4]
    assert len(sites) == len(lines), (len(sites), len(lines))
    out = []
    for ((chrom, pos, _, _), d), ln in zip(sites, lines):
        c, p, _, _ = V.record_fields(ln)
        assert (c, p) == (chrom, pos), (chrom, pos, ln)
        out.append(d)
    return out


def flags(lines, text: bytes, lynch: bool, lo: int, hi: int):
    """One bool per record line: its site's depth lies within the bounds."""
    return [inside(d, lo, hi) for d in record_depths(lines, text, lynch)]


def tally(lines, keep):
    """{(kept, label): records}."""
    n = {(k, lab): 0 for k in (True, False) for lab in (b"hom", b"het")}
    for ln, k in zip(lines, keep):
        n[(bool(k), V.record_fields(ln)[2])] += 1
    return n


def filter_csv(csv: bytes, text: bytes, lynch: bool, lo: int, hi: int):
    """(header + the records within the bounds, kept hom, kept het, dropped hom, dropped het)."""
    lines = csv.splitlines(keepends=True)
    if not lines:
        return b"", 0, 0, 0, 0
    keep = flags(lines[1:], text, lynch, lo, hi)
    n = tally(lines[1:], keep)
    want = lines[0] + b"".join(ln for ln, k in zip(lines[1:], keep) if k)
    return want, n[(True, b"hom")], n[(True, b"het")], n[(False, b"hom")], n[(False, b"het")]


def mark_model(counts, code, lo: int, hi: int, begin: int = 0, end: int = None):
    """sid_depth_mark: the codes (a list of ints) after it."""
    out = [int(k) for k in code]
    end = len(out) if end is None else end
    for i in range(begin, end):
        if not inside(int(np.asarray(counts[i], np.int64).sum()), lo, hi):
            out[i] |= 0x40
    return out


# ----------------------------------------------------------- the builders --
DEPTHS = (3, 4, 8, 29, 30, 31, 90)
DEEP = (150, 199, 200, 201, 300)
# the bounds whose expected output keeps a hom and a het record and drops one of each, for every flag set
BOUNDS = ((30, 30), (0, 29), (8, 31), (31, 0))
DEEP_BOUNDS = ((200, 200), (0, 199), (151, 201), (201, 0))


def _text(n: int, table, chrom=lambda i: b"chr1", mapq: bool = False) -> bytes:
    return b"".join(V.vline(chrom(i), i, V.base_ref(i), V.bases_of(V.base_kind(i), V.base_ref(i),
                                                                  table[i % len(table)]), mapq)
                    for i in range(1, n + 1))


def depth_text(n: int = 3000, chrom=lambda i: b"chr1", mapq: bool = False) -> bytes:
    """n lines, pos i from 1, the reference byte and the kind of site as variants_ref.base_text's, the number
    of read bases by i % 7: below the Lynch methods' coverage 4, at it, around 30 and at 90."""
    return _text(n, DEPTHS, chrom, mapq)


def deep_text(n: int = 2500, chrom=lambda i: b"chr1", mapq: bool = False) -> bytes:
    """The same at 150 .. 300 read bases: the tile parse's quad shape, a major count of 256 and more (the
    second class table) and sites no table covers (the fix-up)."""
    return _text(n, DEEP, chrom, mapq)
