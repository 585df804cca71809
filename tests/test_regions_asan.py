"""regions.cpp -- the BED parser, the merge, contains, the flat table and
sid_regions_mark -- compiled with AddressSanitizer + UndefinedBehaviorSanitizer
into a stand-alone program (tests/asan, mode regions: its own main, nothing
preloaded) and run over a corpus of valid and malformed BED texts generated
here with a fixed seed, with contains queries against every set.  A sanitizer
report fails the test, and every result must equal the unsanitized
build/libsid.so's and the Python restatement's.  CPU only."""
import ctypes as C

import numpy as np

from regions_ref import BedError, RefSet
from sanitized import asan, run   # noqa: F401 (asan: the fixture)
from test_regions import BAD, GOOD, NAMES, boundary_queries, random_bed


def mangle(rng, bed: bytes) -> bytes:
    """A BED text damaged at random: bytes replaced, dropped or inserted, lines cut."""
    b = bytearray(bed)
    for _ in range(int(rng.integers(1, 6))):
        if not b:
            break
        k = int(rng.integers(len(b)))
        op = int(rng.integers(5))
        if op == 0:
            b[k] = int(rng.integers(1, 256))
        elif op == 1:
            del b[k]
        elif op == 2:
            b[k:k] = bytes(rng.integers(1, 256, int(rng.integers(1, 4)), dtype=np.uint8))
        elif op == 3:
            b[k:k] = [b"-", b"+", b"\t", b" ", b"\n", b"\r", b"#", b"99999999999999999999"][int(rng.integers(8))]
        else:
            del b[k:]
    return bytes(b)


def corpus(seed=20):
    rng = np.random.default_rng(seed)
    cases = [t for t, _, _ in GOOD] + [t for t, _ in BAD]
    for k in range(120):
        bed = random_bed(rng, NAMES[:-1], int(rng.integers(0, 80)))
        cases.append(bed)
        cases.append(mangle(rng, bed))
        if k % 10 == 0:
            cases.append(bed[:-1])   # no final newline
    out = []
    for bed in cases:
        try:
            ref = RefSet(bed)
        except (BedError, ValueError):
            ref = None
        names = NAMES + [b"chr", b"N" * 8]
        q = boundary_queries(ref, names, rng, extra=60) if ref else [(b"chr1", 1), (b"x", 0)]
        q = [(c, p) for c, p in q if c and b" " not in c and b"\n" not in c and b"\t" not in c]
        q.sort(key=lambda x: x[0])   # runs by chrom, as a sid_sites holds them
        out.append((bed, ref, q))
    return out


def test_corpus_sanitized(sid, asan, tmp_path):
    cases = corpus()
    p = tmp_path / "corpus.bin"
    with open(p, "wb") as f:
        for bed, _, q in cases:
            f.write(b"B %d %d\n" % (len(bed), len(q)) + bed + b"\n")
            f.write(b"".join(b"%s %d\n" % (c, pos) for c, pos in q))
    lines = run(asan, "regions", p).split(b"\n")
    L = sid.lib()
    k = nbad = ngood = 0
    for bed, ref, q in cases:
        h, bad = C.c_void_p(), C.c_uint64(0)
        rc = L.sid_regions_from_bed(bed, len(bed), C.byref(h), C.byref(bad))
        ni, nc = L.sid_regions_intervals(h), L.sid_regions_chroms(h)
        assert lines[k] == b"%d %d %d %d" % (rc, bad.value, ni, nc), bed
        assert (rc == 0) == (ref is not None), bed
        if rc != 0:
            assert lines[k + 1] == b""
            k += 2
            nbad += 1
            continue
        ngood += 1
        assert (ni, nc) == (ref.intervals, ref.chroms), bed
        lib = b"".join(b"1" if L.sid_regions_contains(h, c, len(c), pos) else b"0" for c, pos in q)
        want = b"".join(b"1" if ref.contains(c, pos) else b"0" for c, pos in q)
        assert lines[k + 1] == lib == want, bed
        assert lines[k + 2] == b"R %d %d" % (ni, nc)
        assert lines[k + 3] == b"M" + b"".join(b"0" if ref.contains(c, pos) else b"1" for c, pos in q), bed
        k += 4
        L.sid_regions_free(h)
    assert nbad >= 30 and ngood >= 100
