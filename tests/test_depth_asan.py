"""parse.cpp -- the host parser and sid_depth_mark -- compiled with
AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program
(tests/asan_depth: its own main, nothing preloaded) and run over a corpus of
valid and damaged pileup texts generated here with a fixed seed.  A sanitizer
report fails the test, and every result must equal the unsanitized
build/libsid.so's; the marks of the valid texts also equal the Python
restatement's.  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depth_ref as D
import variants_ref as V
from test_variants_asan import mangle

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "asan_depth")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def asan():
    # (hipcc's clang, which the project's own build needs, links the sanitizer
    # runtime into the program: no skip, a missing tool fails the test)
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    return os.path.join(DIR, "_build", "depth_asan")


def random_text(rng, n: int) -> bytes:
    refs = [b"A", b"C", b"G", b"T", b"a", b"c", b"g", b"t", b"N", b"n", b"R", b"*"]
    out = []
    for i in range(1, n + 1):
        ref = refs[int(rng.integers(len(refs)))]
        bases = V.bases_of(V.KINDS[int(rng.integers(len(V.KINDS)))], ref, int(rng.integers(1, 60)))
        if rng.random() < 0.1:
            bases += b"+2AC^].*N"
        sep = [b"\t", b" ", b" \t "][int(rng.integers(3))]
        out.append(V.vline(b"chr%d" % (i // 50), i, ref, bases).replace(b"\t", sep))
    return b"".join(out)


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
    with open(p, "wb") as f:
        for text, threads, lo, hi in cases:
            f.write(b"T %d %d %d %d\n" % (len(text), threads, lo, hi) + text + b"\n")
    r = subprocess.run([asan, str(p)], capture_output=True, env=ENV, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert "AddressSanitizer" not in err and "runtime error" not in err and "LeakSanitizer" not in err, err[-3000:]
    assert r.returncode == 0, (r.returncode, err[-3000:])
    lines = r.stdout.split(b"\n")
    L = sid.lib()
    k = nbad = ngood = nmodel = 0
    for text, threads, lo, hi in cases:
        h, bad = C.c_void_p(), C.c_uint64(0)
        rc = L.sid_parse_text(text, len(text), threads, C.byref(h), C.byref(bad))
        n = L.sid_sites_count(h)
        assert lines[k] == b"%d %d %d" % (rc, bad.value if rc else 0, n), text[:200]
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
