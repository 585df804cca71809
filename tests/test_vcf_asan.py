"""emit.cpp's sid_format_vcf over parse.cpp's sites, compiled with
AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program
(tests/asan, mode vcf: its own main, nothing preloaded) and run over a corpus of
valid and damaged pileup texts generated here with a fixed seed.  A sanitizer
report fails the test, and every result must equal the unsanitized
build/libsid.so's; the lines of the valid texts also equal the Python
restatement's (tests/vcf_ref.py over the host CSV of the same arrays).  CPU
only."""
import ctypes as C
import os

import numpy as np

import depth_ref as D
import variants_ref as V
import vcf_ref as F
from sanitized import asan, check_parse, mangle, random_text, run, write_cases   # noqa: F401 (asan: the fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
CONF = [1.0, 0.0, 1e-300, -4.94066e-324, float("nan"), float("inf"), 0.05, 123456.0, 1e22]


def corpus(seed=47):
    rng = np.random.default_rng(seed)
    with open(os.path.join(HERE, "golden", "edge.plp"), "rb") as f:
        edge = f.read()
    long_chrom = V.base_text(200, chrom=lambda i: b"Q" * 70)
    cases = [(b"", 1), (b"\n\n\n", 2), (edge, 1), (edge, 3), (D.depth_text(700), 1), (D.deep_text(300), 2),
             (V.base_text(900), 4), (long_chrom, 1), (V.vline(b"c", b"-2147483648", b"n", b"ACGT" * 9), 1),
             (b"c\t1\tA\t1\t.\tI", 1), (b"c\t1\tAC\t1\t.\tI\n", 1), (b"c\t1\n", 1), (b"c\t1\tA\n", 1), (b" \t \n", 1)]
    for k in range(150):
        t = random_text(rng, int(rng.integers(1, 120)))
        cases.append((t, int(rng.integers(1, 4))))
        cases.append((mangle(rng, t), int(rng.integers(1, 4))))
        if k % 10 == 0:
            cases.append((t[:-1], 1))   # no final newline
    return cases


def arrays(n: int):
    code = np.array([((i * 37 + (i >> 3)) & 0x8F) | (0x40 if i % 11 == 0 else 0) for i in range(n)], np.uint8)
    hom = np.array([CONF[i % 9] for i in range(n)], np.float64)
    het = np.array([CONF[(i * 7 + 3) % 9] for i in range(n)], np.float64)
    return code, hom, het


def test_corpus_sanitized(sid, asan, tmp_path):
    cases = corpus()
    p = tmp_path / "corpus.bin"
    write_cases(p, cases)
    out = run(asan, "vcf", p)
    L = sid.lib()
    at = nbad = ngood = nmodel = nrec = 0

    def line():
        nonlocal at
        e = out.index(b"\n", at)
        ln, at = out[at:e], e + 1
        return ln

    for text, threads in cases:
        rc, h, n = check_parse(L, text, threads, line())
        if rc != 0:
            nbad += 1
            continue
        ngood += 1
        head = line()
        assert head.startswith(b"V ")
        k = int(head[2:])
        got, at = out[at:at + k], at + k + 1
        assert out[at - 1:at] == b"\n"
        sites = sid.Sites(None, np.zeros(n, np.int32), [], h)   # (the handle alone: freed with the object)
        code, hom, het = arrays(n)
        want = sid.format_vcf(sites, code, hom, het)
        assert got == want, text[:200]
        nrec += want.count(b"\n")
        if b"\0" not in text and b"\r" not in text:   # (the model's tokens: the plain separators)
            csv = sid.format_csv(sites, code, hom, het)
            ls = [s for s, c in zip(V.line_sites(text), code) if not c & 0x40]
            model = b"".join(F.vcf_line(ln, s[2], int(np.asarray(s[3], np.int64).sum()))
                             for ln, s in zip(csv.splitlines(keepends=True), ls))
            assert len(ls) == csv.count(b"\n") and got == model, text[:200]
            nmodel += 1
        cp = lambda a: a.ctypes.data_as(C.c_void_p)
        tiny, ln = C.create_string_buffer(8), C.c_size_t(0)
        e = (L.sid_format_vcf(h, 0, n + 1, cp(code), cp(hom), cp(het), tiny, 8, C.byref(ln)),
             L.sid_format_vcf(h, n + 1, n + 1, cp(code), cp(hom), cp(het), tiny, 8, C.byref(ln)),
             L.sid_format_vcf(None, 0, 0, cp(code), cp(hom), cp(het), tiny, 8, C.byref(ln)),
             L.sid_format_vcf(h, 0, n, None, cp(hom), cp(het), tiny, 8, C.byref(ln)),
             L.sid_format_vcf(h, 0, n, cp(code), cp(hom), cp(het), tiny, 8, None),
             L.sid_format_vcf(h, 0, n, cp(code), cp(hom), cp(het), tiny, 8, C.byref(ln)) if n else 3)
        assert line() == b"E %d %d %d %d %d %d" % e and e == (1, 1, 1, 1, 1, 3)
        del sites
    assert at == len(out)
    assert nbad >= 30 and ngood >= 150 and nmodel >= 150 and nrec >= 5000
