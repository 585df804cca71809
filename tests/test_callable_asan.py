"""callable.cpp -- sid_callable_host, the stitch of the chunks' row lists,
sid_callable_join and sid_callable_format -- and parse.cpp compiled with
AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program
(tests/asan, mode callable: its own main, nothing preloaded) and run over the cases
of tests/test_callable.py plus random site sequences under random cuts and the
"a site a chunk" cut.  Every array it touches is an exact-size heap block.  A
sanitizer report fails the test, and every result must equal the Python
model's.  CPU only."""
import itertools

import numpy as np

import callable_ref as CR
import depth_ref
from regions_ref import text_sites
from sanitized import asan, run   # noqa: F401 (asan: the fixture)
from test_callable import BOUNDS, SEQ, SEQ_CODES, SEQ_DEPTHS, quirks_text


def sequences():
    """[(sites, depths)]: the hand-made quirks, then random walks with runs, repeats, steps back, chrom
    changes and returns, positions around 0 and at the top, depths around the bounds."""
    rng = np.random.default_rng(17)
    q = quirks_text()
    out = [(text_sites(q), depth_ref.depths(q))]
    names = [b"chr1", b"chr2", b"chromosome_A", b"chromosome_B", b"c", b"chromoso", b"c" * 40]
    for _ in range(6):
        seq, ds, chrom, pos = [], [], names[0], 1
        for _ in range(300):
            u = rng.random()
            if u < 0.04:
                chrom = names[int(rng.integers(len(names)))]
            if u > 0.97:
                pos = int(rng.choice([-3, 0, 1, 2 ** 31 - 3]))
            elif u > 0.9:
                pos = min(pos + int(rng.integers(-2, 4)), 2 ** 31 - 1)   # (what atoi's int holds)
            elif pos < 2 ** 31 - 1:
                pos += 1
            seq.append((chrom, pos))
            ds.append(int(rng.choice([0, 1, 29, 30, 30, 30, 31, 31, 90, 70000, depth_ref.DEPTH_MAX])))
        out.append((seq, ds))
    return out


def host_case(seq, codes, ds, lo, hi, b, e):
    head = b"H %d %d %d %d %d\n" % (lo, hi, len(seq), b, e)
    body = b"".join(b"%s %d %d %d\n" % (c, p, k, d) for (c, p), k, d in zip(seq, codes, ds))
    ok = 0 <= lo <= depth_ref.DEPTH_MAX and (hi == 0 or lo <= hi <= depth_ref.DEPTH_MAX) and b <= e <= len(seq)
    want = CR.rows(seq[b:e], codes[b:e], ds[b:e], lo, hi) if ok else []
    return head + body, b"%d %d\n" % (0 if ok else 1, len(want)) + CR.fmt(want)


def text_case(text, codes, lo, hi):
    sites, ds = text_sites(text), depth_ref.depths(text)
    assert len(sites) == len(codes)
    want = CR.rows(sites, codes, ds, lo, hi)
    case = b"T %d %d %d %d\n" % (lo, hi, len(text), len(codes)) + text + b"\n" + b" ".join(b"%d" % c for c in codes) + b"\n"
    return case, b"0 %d\n" % len(want) + CR.fmt(want)


def stitch_case(seq, codes, ds, lo, hi, cuts):
    chunks = CR.chunk_model(seq, codes, ds, cuts, lo, hi)
    case = [b"S %d\n" % len(chunks)]
    for rs, edge in chunks:
        case.append(b"C %d %d\n" % (len(rs), edge))
        case += [b"%s %d %d %d\n" % (r[0], r[1] + 1, r[2] - r[1], r[3]) for r in rs]
    want = CR.rows(seq, codes, ds, lo, hi)
    return b"".join(case), b"0 %d\n" % len(want) + CR.fmt(want)


def join_case(a, fa, b, fb):
    want = CR.join(a, fa, b, fb)
    case = b"J %d %d %d %d\n" % (len(a), fa, len(b), fb) + b"".join(b"%s %d %d %d\n" % tuple(r) for r in a + b)
    return case, b"0 %d\n" % len(want) + CR.fmt(want)


def corpus():
    rng = np.random.default_rng(5)
    out = []
    for seq, ds in sequences():
        keep = [k for k, (c, _) in enumerate(seq) if c and b"\0" not in c]
        seq, ds = [seq[k] for k in keep], [ds[k] for k in keep]
        n = len(seq)
        codes = [int(c) for c in rng.choice([0, 0, 0, CR.HET, CR.DROPPED, CR.HET | 3, 5], n)]
        for lo, hi in BOUNDS + [(-1, 0), (5, 4), (0, depth_ref.DEPTH_MAX + 1), (depth_ref.DEPTH_MAX, 0)]:
            out.append(host_case(seq, codes, ds, lo, hi, 0, n))
        out.append(host_case(seq, codes, ds, 0, 0, n // 3, 2 * n // 3))
        out.append(host_case(seq, codes, ds, 0, 0, 5, 5))
        out.append(host_case(seq, codes, ds, 0, 0, 0, n + 1))
        for lo, hi in BOUNDS:
            for k in (0, 1, 5, 40):
                cuts = [0] + sorted(int(x) for x in rng.integers(0, n + 1, k)) + [n]
                out.append(stitch_case(seq, codes, ds, lo, hi, cuts))
            out.append(stitch_case(seq, codes, ds, lo, hi, list(range(n + 1))))   # a site a chunk
        f = CR.flags(seq, codes, ds)
        for k in sorted({0, n} | {int(x) for x in rng.integers(0, n + 1, 12)}):   # site ranges, as ranks take them
            a, b = CR.rows(seq[:k], codes[:k], ds[:k]), CR.rows(seq[k:], codes[k:], ds[k:])
            case, want = join_case(a, int(k > 0 and f[k - 1]), b, int(k < n and f[k]))
            assert want == b"0 %d\n" % len(CR.rows(seq, codes, ds)) + CR.fmt(CR.rows(seq, codes, ds))
            out.append((case, want))
    # the small sequence of test_callable.py under every cut into three chunks
    for cut in itertools.combinations_with_replacement(range(len(SEQ) + 1), 2):
        out.append(stitch_case(SEQ, SEQ_CODES, SEQ_DEPTHS, 0, 0, [0] + list(cut) + [len(SEQ)]))
    a = [(b"chr1", 0, 5, 2), (b"c" * 40, 9, 12, 0)]
    for b in ([(b"c" * 40, 12, 14, 1), (b"chr2", 0, 1, 0)], [(b"c" * 39 + b"d", 12, 14, 1)], [(b"c" * 40, 11, 14, 1)], []):
        for fa, fb in itertools.product((0, 1), repeat=2):
            out.append(join_case(a, fa, b, fb))
    # the parser's own sites: the quirks' text, all codes 0 and a mix
    q = quirks_text()
    nq = len(text_sites(q))
    for lo, hi in BOUNDS:
        out.append(text_case(q, [0] * nq, lo, hi))
        out.append(text_case(q, [int(c) for c in rng.choice([0, CR.HET, CR.DROPPED], nq)], lo, hi))
    out.append(text_case(b"", [], 0, 0))
    out.append(text_case(b"\n" * 50, [], 0, 0))
    out.append((b"S 0\n", b"0 0\n"))
    out.append((b"H 0 0 0 0 0\n", b"0 0\n"))
    out.append((b"J 0 1 0 1\n", b"0 0\n"))
    return out


def test_corpus_sanitized(asan, tmp_path):
    cases = corpus()
    p = tmp_path / "corpus.bin"
    p.write_bytes(b"".join(c for c, _ in cases))
    assert run(asan, "callable", p) == b"".join(w for _, w in cases)
    assert len(cases) >= 300
