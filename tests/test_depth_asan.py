"""parse.cpp -- the host parser and sid_depth_mark -- compiled with
AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program
(tests/asan, mode depth: its own main, nothing preloaded) and run over a corpus
of valid and damaged pileup texts generated here with a fixed seed.  A
sanitizer report fails the test, and every result must equal the unsanitized
build/libsid.so's; the marks of the valid texts also equal the Python
restatement's.  CPU only."""
import ctypes as C
import os

import numpy as np

import depth_ref as D
import variants_ref as V
from sanitized import asan, check_parse, mangle, random_text, run, write_cases   # noqa: F401 (asan: the fixture)

HERE = os.path.dirname(os.path.abspath(__file__))


def corpus(seed=43):
    rng = np.random.default_rng(seed)
    with open(os.path.join(HERE, "golden", "edge.plp"), "rb") as f:
        edge = f.read()
    cases = [(b"", 1, 1, 0), (b"\n\n\n", 2, 0, 5), (edge, 1, 4, 0), (edge, 3, 0, 3), (D.depth_text(700), 1, 8, 31),
             (D.depth_text(3000), 5, 30, 30), (D.deep_text(300), 2, 151, 201), (D.depth_text(50), 1, 0, 0),
             (D.depth_text(50), 1, D.DEPTH_MAX, D.DEPTH_MAX), (b"c\t1\tA\t1\t.\tI", 1, 1, 1),
             (b"c\t1\tAC\t1\t.\tI\n", 1, 1, 0), (b"c\t1\n", 1, 1, 0), (b"c\t1\tA\n", 1, 1, 0), (b" \t \n", 1, 1, 0)]
    for k in range(150):
        t = random_text(rng, int(rng.integers(1, 120)))
        lo = int(rng.integers(0, 40))
        hi = 0 if rng.random() < 0.3 else lo + int(rng.integers(0, 30))
        cases.append((t, int(rng.integers(1, 4)), lo, hi))
        cases.append((mangle(rng, t), int(rng.integers(1, 4)), lo, hi))
        if k % 10 == 0:
            cases.append((t[:-1], 1, lo, hi))   # no final newline
    return cases


def test_corpus_sanitized(sid, asan, tmp_path):
    cases = corpus()
    p = tmp_path / "corpus.bin"
    write_cases(p, cases)
    lines = run(asan, "depth", p).split(b"\n")
    L = sid.lib()
    k = nbad = ngood = nmodel = 0
    for text, threads, lo, hi in cases:
        rc, h, n = check_parse(L, text, threads, lines[k])
        k += 1
        if rc != 0:
            nbad += 1
            continue
        ngood += 1
        code0 = np.array([((i * 37 + (i >> 3)) & 0x8F) | (0x40 if i % 11 == 0 else 0) for i in range(n)], np.uint8)
        code = code0.copy()
        cp = code.ctypes.data_as(C.c_void_p)
        assert L.sid_depth_mark(h, 0, n, lo, hi, cp) == 0
        assert lines[k] == b"M" + b"".join(b"1" if c & 0x40 else b"0" for c in code), text[:200]
        if b"\0" not in text and b"\r" not in text:   # (the model's tokens: the plain separators)
            counts = [s[3] for s in V.line_sites(text)]
            assert [int(c) for c in code] == D.mark_model(counts, code0, lo, hi), text[:200]
            nmodel += 1
        e = (L.sid_depth_mark(h, 0, n + 1, lo, hi, cp), L.sid_depth_mark(h, n + 1, n + 1, lo, hi, cp),
             L.sid_depth_mark(None, 0, 0, lo, hi, cp), L.sid_depth_mark(h, 0, n, lo, hi, None),
             L.sid_depth_mark(h, 0, n, -1, 0, cp), L.sid_depth_mark(h, 0, n, 9, 8, cp),
             L.sid_depth_mark(h, 0, n, 0, D.DEPTH_MAX + 1, cp))
        assert lines[k + 1] == b"E %d %d %d %d %d %d %d" % e and e[:3] == (1, 1, 1) and e[4:] == (1, 1, 1)
        k += 2
        L.sid_sites_free(h)
    assert nbad >= 30 and ngood >= 150 and nmodel >= 150
