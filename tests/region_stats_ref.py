"""A Python restatement of the region rows (--region-stats FILE,
sid_engine_set_region_stats), for the tests: the rows from per-site (chrom,
pos, code, depth) and the set's intervals as Regions.interval enumerates them,
their CSV and the merge of two row lists.  Nothing here calls the stage under
test; site_rows takes the per-site counts from the host parser and the codes
from the oracle, the way depth_hist_ref.site_depths_codes gets them."""
import bisect

import depth_hist_ref as DH
import windows_ref as WR

DROPPED, HET = 0x40, 0x80
HEADER = b"chrom,start,end,sites,depth,records,het,hom\n"
MAX = 1 << 20


def intervals(regions):
    """[(chrom, start, end)] of the set's merged intervals in row order."""
    return [regions.interval(j) for j in range(len(regions))]


def rows(ivs, sites, codes, ds):
    """[(chrom, start, end, sites, depth, records, het, hom)], one per interval in the order given: a site
    belongs to the interval of its chrom (byte-equal) with start < pos <= end."""
    assert len(sites) == len(codes) == len(ds)
    out = [[c, s, e, 0, 0, 0, 0, 0] for c, s, e in ivs]
    by = {}
    for j, (c, s, e) in enumerate(ivs):
        by.setdefault(c, []).append((s, e, j))
    for v in by.values():
        v.sort()
        assert all(a[1] <= b[0] for a, b in zip(v, v[1:])), "the merged intervals are disjoint"
    starts = {c: [x[0] for x in v] for c, v in by.items()}
    for (chrom, pos), code, d in zip(sites, codes, ds):
        v = by.get(chrom)
        if not v:
            continue
        k = bisect.bisect_left(starts[chrom], pos) - 1   # the last start < pos
        if k < 0 or pos > v[k][1]:
            continue
        r = out[v[k][2]]
        rec = not code & DROPPED
        het = bool(rec and code & HET)
        r[3] += 1
        r[4] += d
        r[5] += rec
        r[6] += het
        r[7] += rec and not het
    return [tuple(r) for r in out]


def merge(a, b):
    assert [r[:3] for r in a] == [r[:3] for r in b]
    return [x[:3] + tuple(p + q for p, q in zip(x[3:], y[3:])) for x, y in zip(a, b)]


def fmt(rs, header=True) -> bytes:
    return (HEADER if header else b"") + b"".join(b"%s,%d,%d,%d,%d,%d,%d,%d\n" % r for r in rs)


def site_rows(sid, oracle, regions, text: bytes, method="local", estimate_prior=False, **kw):
    """The model's rows of a text for a Regions object: the host parser's counts, the oracle's call."""
    sites, codes = WR.site_codes(sid, oracle, text, method, estimate_prior=estimate_prior, **kw)
    ds = DH.depths(sid.parse_text(text).counts) if text.strip(b"\n") else []
    return rows(intervals(regions), sites, codes, ds)
