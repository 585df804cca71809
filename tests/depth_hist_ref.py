"""A Python restatement of the depth histogram (--depth-hist FILE,
sid_engine_set_depth_hist), for the tests: the rows from per-site counts and
codes, their CSV and the merge of two row sets.  Nothing here calls the code
under test; site_rows takes the per-site counts from the host parser and the
codes from the oracle, the way windows_ref.site_codes gets them."""
import numpy as np

import windows_ref as WR

DROPPED, HET = 0x40, 0x80
HEADER = b"depth,sites,records,het,hom\n"
DEPTH_MAX = 262140   # 4 x 65535


def depths(counts):
    """A + C + G + T of every site's profile_t as the parser stores it."""
    return [int(d) for d in np.asarray(counts, np.int64).reshape(-1, 4).sum(axis=1)]


def rows(ds, codes):
    """[(depth, sites, records, het, hom)] in ascending depth order: a row per depth that a site has."""
    assert len(ds) == len(codes)
    bins = {}
    for d, c in zip(ds, codes):
        r = bins.setdefault(d, [d, 0, 0, 0, 0])
        rec = not c & DROPPED
        het = bool(rec and c & HET)
        r[1] += 1
        r[2] += rec
        r[3] += het
        r[4] += rec and not het
    return [tuple(bins[d]) for d in sorted(bins)]


def merge(a, b):
    bins = {}
    for r in list(a) + list(b):
        t = bins.setdefault(r[0], [r[0], 0, 0, 0, 0])
        for k in range(1, 5):
            t[k] += r[k]
    return [tuple(bins[d]) for d in sorted(bins)]


def fmt(rs, header=True) -> bytes:
    return (HEADER if header else b"") + b"".join(b"%d,%d,%d,%d,%d\n" % r for r in rs)


def sums(rs):
    """(sites, records, het, hom) summed over the rows (depth rows or, from column 3 on, window rows)."""
    return tuple(sum(r[k] for r in rs) for k in range(-4, 0))


def site_depths_codes(sid, oracle, text: bytes, method="local", estimate_prior=False, **kw):
    """([depth], [code]) of the text's sites: the host parser's counts, the oracle's call over them."""
    _, codes = WR.site_codes(sid, oracle, text, method, estimate_prior=estimate_prior, **kw)
    ds = depths(sid.parse_text(text).counts) if text.strip(b"\n") else []
    assert len(ds) == len(codes)
    return ds, codes


def site_rows(sid, oracle, text: bytes, method="local", estimate_prior=False, **kw):
    return rows(*site_depths_codes(sid, oracle, text, method, estimate_prior=estimate_prior, **kw))


def depth_line(chrom: bytes, pos: int, depth: int, het: bool = False, mapq: bool = False) -> bytes:
    """A line of exactly `depth` counted bases (0 .. DEPTH_MAX) on reference A: '.' for the major base up to
    65535, then C, G, T; het: half of the first 65535 as G instead.  mapq: the seventh column of -m quality."""
    assert 0 <= depth <= DEPTH_MAX
    if mapq:
        ln = depth_line(chrom, pos, depth, het)
        return ln[:-1] + b"\t" + b"5" * max(depth, 1) + b"\n"
    if depth == 0:
        return b"%s\t%d\tA\t0\t*\t*\n" % (chrom, pos)
    n = [0, 0, 0, 0]
    left = depth
    for k in range(4):
        n[k] = min(left, 65535)
        left -= n[k]
    bases = b"." * n[0] + b"C" * n[1] + b"G" * n[2] + b"T" * n[3]
    if het and n[2] == 0:
        bases = b"." * (n[0] - n[0] // 2) + b"G" * (n[0] // 2) + b"C" * n[1]
    return b"%s\t%d\tA\t%d\t%s\t%s\n" % (chrom, pos, len(bases), bases, b"I" * len(bases))
