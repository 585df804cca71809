"""bgzf.cpp and the decoder core bgzf.h -- the member header parse, the
inflate and the CRC32 that the device kernel runs, in their host build --
compiled with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone
program (tests/asan_bgzf: its own main, nothing preloaded) and run over the
shape list plus damaged inputs generated here with a fixed seed, each in
exact-size heap blocks.  A sanitizer report fails the test; every status,
offset and inflated byte must equal the unsanitized build/libsid.so's and
zlib's verdict (a range whose every member zlib inflates to the right size and
CRC is good, anything else is SID_EBGZF).  CPU only."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "asan_bgzf")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def asan():
    # (hipcc's clang, which the project's own build needs, links the sanitizer
    # runtime into the program: no skip, a missing tool fails the test)
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    return os.path.join(DIR, "_build", "bgzf_asan")


def corpus(seed=31, mangled=260):
    """[(bytes, blocks or None)]: the shape list, then damaged copies of its
    smaller members (every kind of block, several members each)."""
    shapes = R.shapes()
    cases = [(z, b) for _, _, z, b in shapes]
    rng = np.random.default_rng(seed)
    small = [(z, b) for _, _, z, b in shapes if 0 < len(z) < 260_000]
    for k in range(mangled):
        z, b = small[k % len(small)]
        cases.append((R.mangle(rng, z, b), None))
    return cases


def test_corpus_sanitized(sid, asan, tmp_path):
    cases = corpus()
    p = tmp_path / "corpus.bin"
    with open(p, "wb") as f:
        for z, _ in cases:
            f.write(b"Z %d\n" % len(z) + z + b"\n")
    r = subprocess.run([asan, str(p)], capture_output=True, env=ENV, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert "AddressSanitizer" not in err and "runtime error" not in err and "LeakSanitizer" not in err, err[-3000:]
    assert r.returncode == 0, err[-3000:]
    out = r.stdout
    q = ngood = nbad = nmangled_good = 0
    for z, blocks in cases:
        nl = out.index(b"\n", q)
        rc, off, nblocks, tlen, crc = (int(x) for x in out[q:nl].split())
        want_rc, want_text, want_off = R.verdict(z)
        assert rc == want_rc, (len(z), rc, off)
        if rc == 0:
            text = out[nl + 1:nl + 1 + tlen]
            assert out[nl + 1 + tlen:nl + 2 + tlen] == b"\n"
            q = nl + 2 + tlen
            assert text == want_text and crc == zlib.crc32(text)
            assert sid.bgzf_inflate_host(z) == text and len(sid.bgzf_index(z)) == nblocks
            ngood += 1
            nmangled_good += blocks is None
        else:
            assert out[nl + 1:nl + 2] == b"\n"
            q = nl + 2
            assert off == want_off, (len(z), off, want_off)
            with pytest.raises(sid.SidError) as e:
                sid.bgzf_inflate_host(z)
            assert (e.value.status, e.value.offset) == (rc, off)
            nbad += 1
        if blocks is not None:
            assert rc == 0 and nblocks == len(blocks)
    assert q == len(out)
    # (a lie in a field nothing reads, or a cut at a member boundary, leaves a valid range)
    assert nbad >= 200 and ngood >= 30, (nbad, ngood, nmangled_good)
