"""What the sanitizer test modules (test_sanitized.py, test_*_asan.py) share:
the product's host code compiled with AddressSanitizer +
UndefinedBehaviorSanitizer into one stand-alone program (tests/asan: its own
main, a mode per module, nothing preloaded), the run that fails on any report,
and the corpus pieces more than one module uses.  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import variants_ref as V

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def asan():
    # (hipcc's clang, which the project's own build needs, links the sanitizer
    # runtime into the program: no skip, a missing tool fails the test; make
    # does nothing after the first module's build)
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    return os.path.join(DIR, "_build", "sid_asan")


def run(asan, mode, path, *args):
    """sid_asan MODE PATH [ARGS]: no sanitizer report, exit status 0; its stdout."""
    r = subprocess.run([asan, mode, str(path)] + [str(a) for a in args], capture_output=True, env=ENV, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert "AddressSanitizer" not in err and "runtime error" not in err and "LeakSanitizer" not in err, err[-3000:]
    assert r.returncode == 0, (r.returncode, err[-3000:])
    return r.stdout


def write_cases(path, cases):
    """The text cases of tests/asan/harness.h: (text, threads, further integers...) each."""
    with open(path, "wb") as f:
        for text, *ints in cases:
            f.write(b"T %d " % len(text) + b" ".join(b"%d" % i for i in ints) + b"\n" + text + b"\n")


def check_parse(L, text, threads, line):
    """The program's "rc err_line sites" line of one text case against
    build/libsid.so's sid_parse_text: (rc, the sites' handle, their count)."""
    h, bad = C.c_void_p(), C.c_uint64(0)
    rc = L.sid_parse_text(text, len(text), threads, C.byref(h), C.byref(bad))
    n = L.sid_sites_count(h)
    assert line == b"%d %d %d" % (rc, bad.value if rc else 0, n), text[:200]
    return rc, h, n


def mangle(rng, text: bytes) -> bytes:
    """A pileup text damaged at random: bytes replaced, dropped or inserted, the text cut."""
    b = bytearray(text)
    for _ in range(int(rng.integers(1, 6))):
        if not b:
            break
        k = int(rng.integers(len(b)))
        op = int(rng.integers(5))
        if op == 0:
            b[k] = int(rng.integers(0, 256))
        elif op == 1:
            del b[k]
        elif op == 2:
            b[k:k] = bytes(rng.integers(0, 256, int(rng.integers(1, 4)), dtype=np.uint8))
        elif op == 3:
            b[k:k] = [b"\t", b" ", b"\n", b"\r", b"\0", b"^", b"+99999999999999999999", b"-3"][int(rng.integers(8))]
        else:
            del b[k:]
    return bytes(b)


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

