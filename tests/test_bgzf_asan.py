"""bgzf.cpp and the decoder core bgzf.h -- the member header parse, the
inflate and the CRC32 that the device kernel runs, in their host build --
compiled with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone
program (tests/asan, mode bgzf: its own main, nothing preloaded) and run over
the shape list plus damaged inputs generated with a fixed seed (bgzf_ref.corpus),
each in exact-size heap blocks.  A sanitizer report fails the test; every status,
offset and inflated byte must equal the unsanitized build/libsid.so's and
zlib's verdict (a range whose every member zlib inflates to the right size and
CRC is good, anything else is SID_EBGZF).  CPU only."""
import zlib

import pytest

import bgzf_ref as R
from sanitized import asan, run   # noqa: F401 (asan: the fixture)


def test_corpus_sanitized(sid, asan, tmp_path):
    cases = R.corpus()
    p = tmp_path / "corpus.bin"
    with open(p, "wb") as f:
        for z, _ in cases:
            f.write(b"Z %d\n" % len(z) + z + b"\n")
    out = run(asan, "bgzf", p)
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
