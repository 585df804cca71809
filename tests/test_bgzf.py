"""BGZF input on the host: the block index, the host inflate (the decoder core
the device runs, host build) and sid_crc32, against Python's zlib / gzip over
the shape list of bgzf_ref.py and over malformed inputs.  CPU only."""
import ctypes as C
import gzip
import struct
import zlib

import numpy as np
import pytest

import bgzf_ref as R

SHAPES = R.shapes()


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=[s[0] for s in SHAPES])
def test_index_and_host_inflate(sid, k):
    _, text, z, blocks = SHAPES[k]
    assert sid.bgzf_index(z) == blocks
    idx = sid.BgzfIndex(z)
    assert len(idx) == len(blocks) and idx.text_len == len(text)
    assert sid.bgzf_inflate_host(z) == text == gzip.decompress(z) if z else text == b""


def test_shape_list_covers_the_decoder():
    """The writer's members really hold what their names say (read off the
    deflate bits: block types, a second deflate block, the longest match)."""
    by = {s[0]: s for s in SHAPES}

    def btype(name, member=0):
        _, _, z, blocks = by[name]
        coff = blocks[member][0]
        hdr = R.parse_member(z, coff)[0]
        return (z[coff + hdr] >> 1) & 3, z[coff + hdr] & 1
    assert btype("stored")[0] == 0 and btype("stored_65280")[0] == 0
    assert btype("fixed")[0] == 1 and btype("dynamic_pileup")[0] == 2
    assert btype("full_flush")[1] == 0   # BFINAL == 0: more deflate blocks follow
    assert by["stored_65280"][3][0][3] == 65280 and by["run_65536"][3][0][3] == 65536
    assert by["one_byte"][3][0][3] == 1 and by["empty_members"][3][0][3] == 0
    assert len(by["random_sizes_300"][3]) == 301 and len(SHAPES) >= 30
    assert len(by["no_eof"][3]) == 2 and by["no_eof"][3][-1][3] != 0


def test_sizing_and_small_cap(sid):
    _, text, z, _ = SHAPES[3]
    L = sid.lib()
    n, off = C.c_size_t(0), C.c_uint64(0)
    assert L.sid_bgzf_inflate_host(z, len(z), None, 0, C.byref(n), C.byref(off)) == 0 and n.value == len(text)
    buf = C.create_string_buffer(len(text))
    n.value = 0
    assert L.sid_bgzf_inflate_host(z, len(z), buf, len(text) - 1, C.byref(n), C.byref(off)) == 3   # SID_ENOMEM
    assert n.value == len(text)
    assert L.sid_bgzf_inflate_host(z, len(z), buf, len(text), C.byref(n), C.byref(off)) == 0
    assert buf.raw == text
    h = C.c_void_p()
    assert L.sid_bgzf_index(None, 0, C.byref(h), C.byref(off)) == 0 and L.sid_bgzf_blocks(h) == 0
    assert L.sid_bgzf_text_len(h) == 0
    assert L.sid_bgzf_block(h, 0, None, None, None, None) == 1
    L.sid_bgzf_free(h)
    assert sid.bgzf_inflate_host(b"") == b""
    assert L.sid_strerror(14) == b"not a BGZF file, or a truncated or corrupt BGZF block"


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 65536])
def test_crc32(sid, n):
    data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    assert sid.crc32(data) == zlib.crc32(data)
    assert sid.crc32(data, 0xdeadbeef) == zlib.crc32(data, 0xdeadbeef)
    assert sid.crc32(data[n // 3:], sid.crc32(data[:n // 3])) == zlib.crc32(data)


def named_bad():
    """[(name, bytes, expected err_offset)]"""
    plp = R.pileup()[:200_000]
    z, blocks = R.write(plp)
    c1, s1 = blocks[1][0], blocks[1][1]
    out = [("plain_gzip", gzip.compress(plp[:1000]), 0),
           ("plain_text", plp[:1000], 0),
           ("one_byte", b"\x1f", 0),
           ("plain_gzip_after_a_member", z[:c1] + gzip.compress(b"abc"), c1)]
    b = bytearray(z)
    b[c1 + 14:c1 + 16] = struct.pack("<H", 0)   # BC with SLEN 0
    out.append(("empty_bc", bytes(b), c1))
    b = bytearray(z)
    b[c1 + 12:c1 + 14] = b"BD"
    out.append(("no_bc", bytes(b), c1))
    last = blocks[-2]
    out.append(("bsize_past_end", z[:last[0] + last[1] - 100], last[0]))
    out.append(("truncated_trailer", z[:c1 + s1 - 3], c1))
    out.append(("truncated_header", z[:c1 + 7], c1))
    out.append(("trailing_garbage", z + b"garbage", len(z)))
    out.append(("trailing_nul", z + b"\0", len(z)))
    b = bytearray(z)
    b[c1 + s1 - 8] ^= 0x10
    out.append(("crc_lie", bytes(b), c1))
    for name, v in (("isize_short", blocks[1][3] - 1), ("isize_long", blocks[1][3] + 1), ("isize_zero", 0),
                    ("isize_over_64k", 65537)):
        b = bytearray(z)
        b[c1 + s1 - 4:c1 + s1] = struct.pack("<I", v)
        out.append((name, bytes(b), c1))
    b = bytearray(z)
    b[c1 + 16:c1 + 18] = struct.pack("<H", 20)   # BSIZE + 1 < header + 8
    out.append(("bsize_too_small", bytes(b), c1))
    rng = np.random.default_rng(11)
    for k in range(24):   # CRC32 catches every single-bit error
        b = bytearray(z)
        j = 1 + k % 2
        pos = blocks[j][0] + 18 + int(rng.integers(blocks[j][1] - 26))
        b[pos] ^= 1 << int(rng.integers(8))
        out.append((f"bit_flip_{k}", bytes(b), blocks[j][0]))
    sz, sblocks = R.write(plp[:100_000], level=0)
    b = bytearray(sz)
    b[sblocks[1][0] + 18 + 3] ^= 1   # a stored block's NLEN
    out.append(("stored_nlen", bytes(b), sblocks[1][0]))
    return out


BAD = named_bad()


@pytest.mark.parametrize("k", range(len(BAD)), ids=[b[0] for b in BAD])
def test_malformed(sid, k):
    _, z, want = BAD[k]
    assert R.verdict(z) == (R.SID_EBGZF, None, want)   # zlib's verdict agrees that it is bad, and where
    with pytest.raises(sid.SidError) as e:
        sid.bgzf_inflate_host(z)
    assert (e.value.status, e.value.offset) == (R.SID_EBGZF, want)


def test_counts():
    assert len(BAD) >= 30 and len(SHAPES) >= 30


def test_index_fails_only_on_the_container(sid):
    """The index hops over headers and trailers: a payload error is not its
    business, a container error is, with the member's offset."""
    for name, z, want in BAD:
        hops_ok = name.startswith(("bit_flip", "crc_lie", "stored_nlen")) or name in ("isize_short", "isize_long",
                                                                                      "isize_zero")
        if hops_ok:
            assert len(sid.bgzf_index(z)) > 0, name
        else:
            with pytest.raises(sid.SidError) as e:
                sid.bgzf_index(z)
            assert (e.value.status, e.value.offset) == (R.SID_EBGZF, want), name
