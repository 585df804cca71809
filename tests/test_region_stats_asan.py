"""region_stats.cpp -- sid_region_stats_host, the check and the sum of the
chunks' row lists, sid_region_stats_merge and sid_region_stats_format --
regions.cpp (the merge, the source order, sid_regions_interval) and parse.cpp
compiled with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone
program (tests/asan, mode region_stats: its own main, nothing preloaded) and run over
the cases of tests/test_region_stats.py plus random BED sets and site
sequences.  Every array it touches is an exact-size heap block.  A sanitizer
report fails the test, and every result must equal the Python model's.  CPU
only."""
import numpy as np

import depth_ref
import region_stats_ref as RS
from regions_ref import POS_MAX, BedError, parse_bed, text_sites
from sanitized import asan, run   # noqa: F401 (asan: the fixture)
from test_region_stats import QUIRKS_BED, pl, want_intervals
from test_windows import quirks_text

DROPPED, HET = 0x40, 0x80


def bed_ok(bed: bytes) -> bool:
    try:
        parse_bed(bed)
        return True
    except BedError:
        return False


def bed_head(bed: bytes) -> bytes:
    return b"B %d\n" % len(bed) + bed + b"\n"


def interval_case(bed):
    if not bed_ok(bed):
        return bed_head(bed) + b"I\n", b"1 0\n1\n"
    ivs = want_intervals(bed)
    return bed_head(bed) + b"I\n", b"0 %d\n" % len(ivs) + b"".join(b"%s %d %d\n" % iv for iv in ivs) + b"0\n"


def model(bed, text, codes, a, b):
    sites, ds = text_sites(text), depth_ref.depths(text)
    assert len(sites) == len(codes) == len(ds)
    return RS.rows(want_intervals(bed), sites[a:b], codes[a:b], ds[a:b])


def text_case(bed, text, codes, a=0, b=None):
    n = len(codes)
    b = n if b is None else b
    case = bed_head(bed) + b"T %d %d %d %d\n" % (len(text), n, a, b) + text + b"\n" + b" ".join(b"%d" % c for c in codes) + b"\n"
    if not bed_ok(bed) or not a <= b <= n:
        return case, b"1 0\n"
    want = model(bed, text, codes, a, b)
    return case, b"0 %d\n" % len(want) + RS.fmt(want, header=False)


def merge_case(bed, text, codes, cut, spoil):
    n = len(codes)
    case = bed_head(bed) + b"M %d %d %d %d\n" % (len(text), n, cut, spoil) + text + b"\n" + b" ".join(b"%d" % c for c in codes) + b"\n"
    want = RS.merge(model(bed, text, codes, 0, cut), model(bed, text, codes, cut, n))
    if spoil and want:
        return case, b"1 0\n"
    return case, b"0 %d\n" % len(want) + RS.fmt(want, header=False)


def chunk_case(bed, chunks):
    """chunks: [[(row index, sites, het, hom, depth)]] by the model's row order; the device's index is the flat
    table's, the chroms sorted by (first 8 bytes little-endian, length, bytes)."""
    ivs = want_intervals(bed)
    chroms = sorted({c for c, _, _ in ivs}, key=lambda c: (int.from_bytes(c[:8].ljust(8, b"\0"), "little"), len(c), c))
    table = [iv for c in chroms for iv in ivs if iv[0] == c]
    case = bed_head(bed) + b"C %d\n" % len(chunks)
    tot = [[0, 0, 0, 0, 0] for _ in ivs]
    ok = True
    for ch in chunks:
        case += b"R %d\n" % len(ch)
        seen = set()
        for j, s, h, m, d in ch:
            idx = table.index(ivs[j]) if j < len(ivs) else j
            case += b"%d %d %d %d %d\n" % (idx, s, h, m, d)
            ok = ok and j < len(ivs) and j not in seen and s > 0 and h + m <= s
            seen.add(j)
            if ok:
                t = tot[j]
                t[0] += s
                t[1] += d
                t[2] += h + m
                t[3] += h
                t[4] += m
    if not ok:
        return case, b"7 0\n"
    want = [iv + tuple(t) for iv, t in zip(ivs, tot)]
    return case, b"0 %d\n" % len(want) + RS.fmt(want, header=False)


def random_bed(rng, names, n):
    out = []
    for _ in range(n):
        c = names[int(rng.integers(len(names)))]
        u = rng.random()
        if u < 0.05:
            out.append(c + b"\n")
        elif u < 0.1:
            s = int(rng.integers(0, 300))
            out.append(b"%s\t%d\t%d\n" % (c, s, s))   # an empty interval
        else:
            s = int(rng.integers(0, 300))
            out.append(b"%s\t%d\t%d\textra\n" % (c, s, s + int(rng.integers(1, 40))))
    return b"".join(out)


def corpus():
    rng = np.random.default_rng(23)
    names = [b"chr1", b"chr2", b"chromosome_A", b"chromosome_B", b"c", b"chromoso", b"c" * 40, b"chr10"]
    out = []
    q = quirks_text()
    nq = len(text_sites(q))
    beds = [QUIRKS_BED, b"", b"chr1\n", b"# none\n\n", b"chr1\t5\t5\n", b"chr1\t0\t2147483647\nchr1\t3\t9\n",
            b"chrZ\t0\t99999999999\n", b"chr1 7\n", b"chr1\t9\t3\n"]
    beds += [random_bed(rng, names, int(k)) for k in (1, 3, 10, 40, 120, 400)]
    for bed in beds:
        out.append(interval_case(bed))
        out.append(text_case(bed, q, [0] * nq))
        codes = [int(c) for c in rng.choice([0, HET, DROPPED, HET | 3, 5], nq)]
        out.append(text_case(bed, q, codes))
        out.append(text_case(bed, q, codes, nq // 3, 2 * nq // 3))
        out.append(text_case(bed, q, codes, 5, 5))
        out.append(text_case(bed, q, codes, 0, nq + 1))
        out.append(text_case(bed, b"", []))
        if bed_ok(bed):
            for cut in (0, 1, nq // 2, nq):
                out.append(merge_case(bed, q, codes, cut, 0))
            out.append(merge_case(bed, q, codes, nq // 2, 1))
    # random walks over the random sets' chroms and positions, sites on every edge
    for k in range(6):
        bed = random_bed(rng, names, 60)
        lines, chrom, pos = [], names[0], 1
        for _ in range(400):
            u = rng.random()
            if u < 0.05:
                chrom = names[int(rng.integers(len(names)))]
            if u > 0.97:
                pos = int(rng.choice([-3, 0, 1, POS_MAX]))
            elif u > 0.8:
                pos = int(rng.integers(0, 345))
            elif pos < POS_MAX:
                pos += 1
            lines.append(pl(chrom, pos, rng.choice([b"*", b"..", b"...,,,..,.", b"A" * 70])))
        text = b"".join(lines)
        codes = [int(c) for c in rng.choice([0, 0, HET, DROPPED], len(lines))]
        out.append(text_case(bed, text, codes))
        out.append(text_case(bed, text, codes, 17, 333))
        out.append(merge_case(bed, text, codes, 123, 0))
        ni = len(want_intervals(bed))
        # the chunks' rows as the device hands them back: any order, each interval at most once a chunk
        chunks = []
        for _ in range(int(rng.integers(0, 5))):
            js = rng.permutation(ni)[:int(rng.integers(0, ni + 1))]
            chunks.append([(int(j), int(s), int(s) // 3, int(s) // 2, int(rng.integers(0, 2 ** 40))) for j in js
                           for s in [rng.integers(1, 2 ** 32)]])
        out.append(chunk_case(bed, chunks))
        if ni >= 2:
            out.append(chunk_case(bed, [[(0, 1, 0, 1, 3)], [(1, 2, 1, 1, 5), (1, 1, 0, 0, 0)]]))   # an interval twice
            out.append(chunk_case(bed, [[(ni, 1, 0, 0, 0)]]))                                     # outside the set
            out.append(chunk_case(bed, [[(0, 0, 0, 0, 0)]]))                                      # a row without a site
            out.append(chunk_case(bed, [[(0, 2, 2, 1, 0)]]))                                      # more records than sites
            out.append(chunk_case(bed, [[(j, 1, 0, 0, 0) for j in range(ni)] + [(0, 1, 0, 0, 0)]]))   # more rows than intervals
    out.append(chunk_case(b"", []))
    out.append(chunk_case(b"a\t0\t1\n", []))
    return out


def test_corpus_sanitized(asan, tmp_path):
    cases = corpus()
    p = tmp_path / "corpus.bin"
    p.write_bytes(b"".join(c for c, _ in cases))
    got = run(asan, "region_stats", p)
    want = b"".join(w for _, w in cases)
    if got != want:   # (name the first case that differs)
        at = 0
        for k, (c, w) in enumerate(cases):
            assert got[at:at + len(w)] == w, (k, c[:300], got[at:at + 300], w[:300])
            at += len(w)
    assert got == want
    assert len(cases) >= 150
