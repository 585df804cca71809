"""depth_hist.cpp and parse.cpp -- the depth histogram's host code and the host
parser -- compiled with AddressSanitizer + UndefinedBehaviorSanitizer into a
stand-alone program (tests/asan, mode depth_hist: its own main, nothing preloaded)
and run over a corpus of valid and damaged pileup texts generated here with a
fixed seed.  A sanitizer report fails the test, and every result must equal the
unsanitized build/libsid.so's; the rows of the valid texts also equal the
Python restatement's.  CPU only."""
import os

import numpy as np

import depth_hist_ref as DH
import depth_ref as D
import variants_ref as V
from sanitized import asan, check_parse, mangle, random_text, run, write_cases   # noqa: F401 (asan: the fixture)

HERE = os.path.dirname(os.path.abspath(__file__))


def corpus(seed=47):
    rng = np.random.default_rng(seed)
    with open(os.path.join(HERE, "golden", "edge.plp"), "rb") as f:
        edge = f.read()
    wrap = b"c\t1\tG\t9\t" + b"A" * 65536 + b"CCC\t*\nc\t2\tG\t9\t" + b"A" * 65536 + b"\t*\n"
    ramp = b"".join(DH.depth_line(b"r", i + 1, d, i % 2 == 0) for i, d in enumerate([0, 1, 2, 1023, 1024, 65535, 65536]))
    cases = [(b"", 1), (b"\n\n\n", 2), (edge, 1), (edge, 3), (D.depth_text(700), 1), (D.depth_text(3000), 5),
             (D.deep_text(300), 2), (wrap, 1), (ramp, 2), (b"c\t1\tA\t1\t.\tI", 1), (b"c\t1\tAC\t1\t.\tI\n", 1),
             (b"c\t1\n", 1), (b"c\t1\tA\n", 1), (b" \t \n", 1)]
    for k in range(150):
        t = random_text(rng, int(rng.integers(1, 120)))
        cases.append((t, int(rng.integers(1, 4))))
        cases.append((mangle(rng, t), int(rng.integers(1, 4))))
        if k % 10 == 0:
            cases.append((t[:-1], 1))   # no final newline
    return cases


def take(blob: bytes, at: int, tag: bytes):
    """One "<tag> <bytes>\\n<bytes of text>" item of the driver's output: (text, the offset behind it)."""
    nl = blob.index(b"\n", at)
    t, n = blob[at:nl].split()
    assert t == tag
    return blob[nl + 1:nl + 1 + int(n)], nl + 1 + int(n)


def test_corpus_sanitized(sid, asan, tmp_path):
    cases = corpus()
    p = tmp_path / "corpus.bin"
    write_cases(p, cases)
    blob = run(asan, "depth_hist", p)
    L = sid.lib()
    at = nbad = ngood = nmodel = 0
    for text, threads in cases:
        nl = blob.index(b"\n", at)
        rc, h, n = check_parse(L, text, threads, blob[at:nl])
        at = nl + 1
        if rc != 0:
            nbad += 1
            continue
        ngood += 1
        s = sid.parse_text(text, threads)
        code = np.array([((i * 37 + (i >> 3)) & 0x8F) | (0x40 if i % 5 == 0 else 0) for i in range(n)], np.uint8)
        rows = sid.depth_hist_host(s, code)
        got_h, at = take(blob, at, b"H")
        got_m, at = take(blob, at, b"M")
        assert got_h == sid.depth_hist_format(rows), text[:200]
        half = n // 2
        merged = sid.depth_hist_merge(sid.depth_hist_host(s, code, 0, half), sid.depth_hist_host(s, code, half, n))
        assert merged == rows and got_m == sid.depth_hist_format(merged, header=False), text[:200]
        if b"\0" not in text and b"\r" not in text:   # (the model's tokens: the plain separators)
            ds = [int((np.asarray(x[3], np.int64) & 0xFFFF).sum()) for x in V.line_sites(text)]   # (u16 counts wrap)
            assert got_h == DH.fmt(DH.rows(ds, [int(c) for c in code])), text[:200]
            nmodel += 1
        nl = blob.index(b"\n", at)
        e = [int(x) for x in blob[at:nl].split()[1:]]
        assert blob[at:at + 2] == b"E " and e == [1, 1, 1, 1, 1, 1], (e, text[:200])
        at = nl + 1
        L.sid_sites_free(h)
    assert at == len(blob)
    assert nbad >= 30 and ngood >= 150 and nmodel >= 150
