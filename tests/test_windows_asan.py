"""windows.cpp -- the stitch of the chunks' row lists, sid_windows_host and
sid_windows_format -- compiled with AddressSanitizer +
UndefinedBehaviorSanitizer into a stand-alone program (tests/asan, mode
windows: its own main, nothing preloaded) and run over the cases of
tests/test_windows.py and random site sequences under every cut.  Every array
it touches is an exact-size heap block.  A sanitizer report fails the test, and
every result must equal the Python model's.  CPU only."""
import itertools

import numpy as np

import windows_ref as WR
from regions_ref import text_sites
from sanitized import asan, run   # noqa: F401 (asan: the fixture)
from test_windows import WS, quirks_text


def sequences():
    rng = np.random.default_rng(11)
    out = [[(c, p) for c, p in text_sites(quirks_text()) if b"\0" not in c]]
    names = [b"chr1", b"chr2", b"chromosome_A", b"chromosome_B", b"c", b"a,b"]
    for _ in range(6):
        seq, chrom, pos = [], names[0], 1
        for _ in range(300):
            u = rng.random()
            if u < 0.04:
                chrom = names[int(rng.integers(len(names)))]
            pos = int(rng.integers(-80, 400)) if u > 0.93 else pos + int(rng.integers(0, 9))
            seq.append((chrom, pos))
        out.append(seq)
    return out


def host_case(seq, codes, w, b, e):
    head = b"H %d %d %d %d\n" % (w, len(seq), b, e)
    body = b"".join(b"%s %d %d\n" % (c, p, k) for (c, p), k in zip(seq, codes))
    ok = 1 <= w and b <= e <= len(seq)
    want = WR.rows(seq[b:e], codes[b:e], w) if ok else []
    return head + body, b"%d %d\n" % (0 if ok else 1, len(want)) + WR.fmt(want, header=False)


def stitch_case(seq, codes, w, cuts):
    chunks = WR.chunk_rows(seq, codes, w, cuts)
    case = [b"S %d %d\n" % (w, len(chunks))]
    for ch in chunks:
        case.append(b"C %d\n" % len(ch))
        case += [b"%s %d %d %d %d\n" % (r[0], r[1] // w, r[3], r[4], r[5]) for r in ch]
    want = WR.rows(seq, codes, w)
    return b"".join(case), b"0 %d\n" % len(want) + WR.fmt(want, header=False)


def corpus():
    rng = np.random.default_rng(3)
    out = []
    for seq in sequences():
        n = len(seq)
        codes = [int(c) for c in rng.choice([0, WR.HET, WR.DROPPED, WR.HET | 3, 5], n)]
        for w in WS + [0, -5]:
            out.append(host_case(seq, codes, w, 0, n))
        out.append(host_case(seq, codes, 37, n // 3, 2 * n // 3))
        out.append(host_case(seq, codes, 37, 5, 5))
        out.append(host_case(seq, codes, 37, 0, n + 1))
        for w in WS:
            for k in (0, 1, 5, 40):
                cuts = [0] + sorted(int(x) for x in rng.integers(0, n + 1, k)) + [n]
                out.append(stitch_case(seq, codes, w, cuts))
            out.append(stitch_case(seq, codes, w, list(range(n + 1))))   # a site a chunk
    small = [(b"chr1", p) for p in (1, 2, 3, 11)] + [(b"chromosome_long", 1)] * 2 + [(b"chr1", 3), (b"chr2", 3)]
    for cut in itertools.combinations_with_replacement(range(len(small) + 1), 3):
        out.append(stitch_case(small, [0, WR.HET] * 4, 10, [0] + list(cut) + [len(small)]))
    out.append((b"S 10 0\n", b"0 0\n"))
    out.append((b"H 10 0 0 0\n", b"0 0\n"))
    return out


def test_corpus_sanitized(asan, tmp_path):
    cases = corpus()
    p = tmp_path / "corpus.bin"
    p.write_bytes(b"".join(c for c, _ in cases))
    assert run(asan, "windows", p) == b"".join(w for _, w in cases)
    assert len(cases) >= 300
