"""parse.cpp -- the host parser's reference bytes and sid_variants_mark --
compiled with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone
program (tests/asan, mode variants: its own main, nothing preloaded) and run
over a corpus of valid and damaged pileup texts generated here with a fixed
seed.  A sanitizer report fails the test, and every result must equal the
unsanitized build/libsid.so's; the reference bytes of the valid texts also
equal the Python restatement's.  CPU only."""
import ctypes as C
import os

import numpy as np

import variants_ref as V
from sanitized import asan, check_parse, mangle, run, write_cases   # noqa: F401 (asan: the fixture)

HERE = os.path.dirname(os.path.abspath(__file__))


def random_text(rng, n: int) -> bytes:
    """(this module's own: reference bytes of every kind, the parser's metacharacters among them)"""
    refs = [b"A", b"C", b"G", b"T", b"a", b"c", b"g", b"t", b"N", b"n", b"R", b"*", b"^", b"+", b"."]
    out = []
    for i in range(1, n + 1):
        ref = refs[int(rng.integers(len(refs)))]
        kind = V.KINDS[int(rng.integers(len(V.KINDS)))]
        bases = V.bases_of(kind, ref, int(rng.integers(1, 40)))
        if rng.random() < 0.1:
            bases += b"+2AC^]."
        sep = [b"\t", b" ", b" \t "][int(rng.integers(3))]
        out.append(V.vline(b"chr%d" % (i // 50), i, ref, bases).replace(b"\t", sep))
    return b"".join(out)


def corpus(seed=41):
    rng = np.random.default_rng(seed)
    with open(os.path.join(HERE, "golden", "edge.plp"), "rb") as f:
        edge = f.read()
    cases = [(b"", 1), (b"\n\n\n", 2), (edge, 1), (edge, 3), (V.base_text(700), 1), (V.base_text(4000), 5),
             (V.placement_text("second", 300), 2), (b"c\t1\tA\t1\t.\tI", 1), (b"c\t1\tAC\t1\t.\tI\n", 1),
             (b"c\t1\n", 1), (b"c\t1\tA\n", 1), (b" \t \n", 1)]
    for k in range(150):
        t = random_text(rng, int(rng.integers(1, 120)))
        cases.append((t, int(rng.integers(1, 4))))
        cases.append((mangle(rng, t), int(rng.integers(1, 4))))
        if k % 10 == 0:
            cases.append((t[:-1], 1))   # no final newline
    return cases


def test_corpus_sanitized(sid, asan, tmp_path):
    cases = corpus()
    p = tmp_path / "corpus.bin"
    write_cases(p, cases)
    lines = run(asan, "variants", p).split(b"\n")
    L = sid.lib()
    k = nbad = ngood = 0
    for text, threads in cases:
        rc, h, n = check_parse(L, text, threads, lines[k])
        k += 1
        if rc != 0:
            nbad += 1
            continue
        ngood += 1
        refs = C.string_at(L.sid_sites_refs(h), n) if n else b""
        assert lines[k] == refs.hex().encode(), text[:200]
        if b"\0" not in text and b"\r" not in text:   # (the model's tokens: the plain separators)
            assert refs == b"".join(s[2] for s in V.line_sites(text)), text[:200]
        code = np.array([((i * 37 + (i >> 3)) & 0x8F) | (0x40 if i % 11 == 0 else 0) for i in range(n)], np.uint8)
        cp = code.ctypes.data_as(C.c_void_p)
        assert L.sid_variants_mark(h, 0, n, cp) == 0
        assert lines[k + 1] == b"M" + b"".join(b"1" if c & 0x40 else b"0" for c in code), text[:200]
        e = (L.sid_variants_mark(h, 0, n + 1, cp), L.sid_variants_mark(h, n + 1, n + 1, cp),
             L.sid_variants_mark(None, 0, 0, cp), L.sid_variants_mark(h, 0, n, None))
        assert lines[k + 2] == b"E %d %d %d %d" % e and e[:3] == (1, 1, 1)
        k += 3
        L.sid_sites_free(h)
    assert nbad >= 30 and ngood >= 150
