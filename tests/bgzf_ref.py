"""BGZF test helper (no tests): a writer over Python's zlib, the shape list the
decoder is checked on, zlib's verdict on a byte range, and a mangler.  All
expected bytes come from zlib / gzip, none from the code under test."""
import gzip
import os
import struct
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SID_EBGZF = 14


def member(payload: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, extra=b"", flush_at=None) -> bytes:
    """One BGZF member.  extra: subfields in front of BC; flush_at: a
    Z_FULL_FLUSH after that many payload bytes (several deflate blocks)."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        body = c.compress(payload) + c.flush()
    else:
        body = c.compress(payload[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(payload[flush_at:]) + c.flush()
    xlen = len(extra) + 6
    bsize = 12 + xlen + len(body) + 8
    assert bsize <= 65536, bsize
    return (b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\x00\xff" + struct.pack("<H", xlen) + extra
            + b"BC" + struct.pack("<HH", 2, bsize - 1) + body
            + struct.pack("<II", zlib.crc32(payload), len(payload)))


def write(data: bytes, payload=0xff00, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, extra=b"", flush_at=None,
          eof=True, sizes=None):
    """(bgzf bytes, blocks): blocks = [(coff, csize, toff, isize)].  sizes: the
    payload size of each member in turn (0 = an empty member), else `payload`
    bytes each."""
    out, blocks, t = [], [], 0
    coff = 0
    it = iter(sizes) if sizes is not None else None
    while True:
        if it is not None:
            try:
                n = next(it)
            except StopIteration:
                assert t == len(data)
                break
        else:
            if t >= len(data):
                break
            n = payload
        chunk = data[t:t + n]
        m = member(chunk, level, strategy, extra, flush_at if flush_at is not None and flush_at < len(chunk) else None)
        out.append(m)
        blocks.append((coff, len(m), t, len(chunk)))
        coff += len(m)
        t += len(chunk)
    if eof:
        out.append(EOF_MARKER)
        blocks.append((coff, len(EOF_MARKER), t, 0))
    z = b"".join(out)
    assert gzip.decompress(z) == data if z else data == b""   # an independent reader of the container
    return z, blocks


def handmade_dist_32768(rnd: bytes):
    """A member zlib's compressor cannot make (its matches reach back 32506 at
    most): 32768 stored bytes, then a fixed-Huffman block of 100 matches of
    length 258 at distance 32768.  (text, bgzf bytes, blocks)"""
    assert len(rnd) == 32768
    bits = []

    def put(v, n, msb=False):   # Huffman codes go in from their first bit, everything else from bit 0
        bits.extend((v >> (n - 1 - i if msb else i)) & 1 for i in range(n))
    put(1, 1), put(1, 2)                       # BFINAL, fixed
    for _ in range(100):
        put(0b11000000 + 285 - 280, 8, True)   # length symbol 285: 258
        put(29, 5, True), put(32768 - 24577, 13)
    put(0, 7, True)                            # end of block
    bits += [0] * (-len(bits) % 8)
    fixed = bytes(sum(b << i for i, b in enumerate(bits[k:k + 8])) for k in range(0, len(bits), 8))
    body = b"\x00" + struct.pack("<HH", 32768, 32768 ^ 0xffff) + rnd + fixed
    text = rnd + rnd[:25800]
    bsize = 18 + len(body) + 8
    m = (b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\x00\xff" + struct.pack("<H", 6) + b"BC"
         + struct.pack("<HH", 2, bsize - 1) + body + struct.pack("<II", zlib.crc32(text), len(text)))
    assert gzip.decompress(m) == text
    return text, m + EOF_MARKER, [(0, len(m), 0, len(text)), (len(m), len(EOF_MARKER), len(text), 0)]


def pileup() -> bytes:
    with open(os.path.join(HERE, "golden", "c1_10k.plp"), "rb") as f:
        return f.read()


def shapes():
    """[(name, text, bgzf bytes, blocks)]: the smallest inputs at which each
    branch of the decoder can go wrong."""
    rng = np.random.default_rng(7)
    plp = pileup()
    rnd = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    geo = np.minimum(rng.geometric(0.05, 200_000) - 1, 255).astype(np.uint8).tobytes()
    big = rng.integers(0, 256, 3_000_000, dtype=np.uint8).tobytes()
    S = []

    def add(name, data, **kw):
        z, b = write(data, **kw)
        S.append((name, data, z, b))
    add("stored", plp[:200_000], level=0, payload=0xff00)
    add("stored_65280", plp[:65280], level=0, payload=65280)
    add("fixed", plp[:150_000], strategy=zlib.Z_FIXED)
    add("dynamic_pileup", plp)
    add("dynamic_pileup_l1", plp[:300_000], level=1)
    add("dynamic_pileup_l9", plp[:300_000], level=9)
    add("run_65280", b"A" * 65280, payload=65280)
    add("run_65536", b"\0" * 65536, payload=65536)
    add("period3", b"abc" * 30_000)
    add("dist_30000", rnd[:30000] + rnd[:30000], payload=60000)   # (zlib's own matches stop at 32768 - 262)
    S.append(("dist_32768",) + handmade_dist_32768(rnd))
    add("geometric", geo)
    add("incompressible", rng.integers(0, 256, 200_000, dtype=np.uint8).tobytes(), payload=0xff00 - 64)
    add("one_byte", b"x", payload=1)
    add("empty_members", plp[:5000], sizes=[0, 2000, 0, 0, 3000, 0])
    add("no_eof", plp[:100_000], eof=False)
    add("no_eof_one", b"hello\n", eof=False)
    add("only_eof", b"")
    add("extra_subfield", plp[:100_000], extra=b"XY" + struct.pack("<H", 5) + b"12345")
    add("two_extra_subfields", plp[:70_000], extra=b"AB\x00\x00" + b"BD\x02\x00zz")
    add("full_flush", plp[:200_000], flush_at=20_000)
    add("full_flush_fixed", plp[:100_000], flush_at=1, strategy=zlib.Z_FIXED)
    add("payload_777", plp[:120_000], payload=777)
    add("huffman_only", geo[:100_000], strategy=zlib.Z_HUFFMAN_ONLY)
    add("rle", (b"a" * 300 + b"b" * 7) * 300, strategy=zlib.Z_RLE)
    sizes = [int(x) for x in rng.integers(1, 65281, 300)]
    data = (plp * (sum(sizes) // len(plp) + 1))[:sum(sizes)]
    # (every third member random bytes: payload sizes and content both vary)
    mix = bytearray(data)
    t = 0
    for k, n in enumerate(sizes):
        if k % 3 == 0:
            mix[t:t + min(n, 40_000)] = big[t % 1_000_000:t % 1_000_000 + min(n, 40_000)]
        t += n
    add("random_sizes_300", bytes(mix), sizes=sizes)
    for lvl in (1, 2, 3, 4, 5, 7, 8):
        add(f"pileup_level{lvl}", plp[lvl * 1000:lvl * 1000 + 90_000], level=lvl, payload=30_000 + lvl)
    return S


def parse_member(z: bytes, off: int):
    """The issue's container rules restated: (header bytes, member bytes,
    crc, isize) or None when no whole BGZF member starts at off."""
    p = z[off:]
    if len(p) < 12 or p[0] != 0x1f or p[1] != 0x8b or p[2] != 8 or not p[3] & 4:
        return None
    xlen = struct.unpack_from("<H", p, 10)[0]
    if len(p) < 12 + xlen:
        return None
    q, end, bsize = 12, 12 + xlen, None
    while q + 4 <= end:
        slen = struct.unpack_from("<H", p, q + 2)[0]
        if q + 4 + slen > end:
            break
        if p[q:q + 2] == b"BC" and slen == 2:
            bsize = struct.unpack_from("<H", p, q + 4)[0] + 1
            break
        q += 4 + slen
    if bsize is None or bsize < end + 8 or len(p) < bsize:
        return None
    crc, isize = struct.unpack_from("<II", p, bsize - 8)
    if isize > 65536:
        return None
    return end, bsize, crc, isize


def verdict(z: bytes):
    """zlib's verdict on a byte range: (0, text, None) when every member
    parses, zlib inflates its payload to exactly ISIZE bytes with nothing left
    over and the right CRC; else (SID_EBGZF, None, the first bad member's
    offset).  As the library's, the walk over the headers comes first: a range
    that does not index fails at the member that does not parse."""
    off, members = 0, []
    while off < len(z):
        m = parse_member(z, off)
        if m is None:
            return SID_EBGZF, None, off
        members.append((off,) + m)
        off += m[1]
    out = []
    for off, hdr, bsize, crc, isize in members:
        d = zlib.decompressobj(-15)
        try:
            text = d.decompress(z[off + hdr:off + bsize - 8])
        except zlib.error:
            return SID_EBGZF, None, off
        if not d.eof or len(text) != isize or zlib.crc32(text) != crc:
            return SID_EBGZF, None, off
        out.append(text)
    return 0, b"".join(out), None


def mangle(rng, z: bytes, blocks) -> bytes:
    """A BGZF range damaged at random: payload bits flipped, the range cut, or
    a lie in BSIZE / ISIZE / CRC of one member."""
    b = bytearray(z)
    real = [x for x in blocks if x[1] > 28] or list(blocks)
    coff, csize, _, _ = real[int(rng.integers(len(real)))]
    op = int(rng.integers(7))
    if op == 0:      # one payload bit
        k = coff + 18 + int(rng.integers(max(csize - 26, 1)))
        b[k] ^= 1 << int(rng.integers(8))
    elif op == 1:    # a few payload bytes
        for _ in range(int(rng.integers(1, 5))):
            k = coff + 18 + int(rng.integers(max(csize - 26, 1)))
            b[k] = int(rng.integers(256))
    elif op == 2:    # cut
        del b[int(rng.integers(1, len(b))):]
    elif op == 3:    # BSIZE
        v = int(rng.integers(0, 65536))
        b[coff + 16:coff + 18] = struct.pack("<H", v)
    elif op == 4:    # ISIZE
        v = [0, 1, 65536, 65537, 0xffffffff, int(rng.integers(0, 70000))][int(rng.integers(6))]
        b[coff + csize - 4:coff + csize] = struct.pack("<I", v)
    elif op == 5:    # CRC
        b[coff + csize - 8 + int(rng.integers(4))] ^= 1 << int(rng.integers(8))
    else:            # the first deflate bytes: block type and code lengths
        k = coff + 18 + int(rng.integers(min(max(csize - 26, 1), 40)))
        b[k] = int(rng.integers(256))
    return bytes(b)


def corpus(seed=31, mangled=260):
    """[(bytes, blocks or None)]: the shape list, then damaged copies of its
    smaller members (every kind of block, several members each): what the
    sanitized host build (tests/test_bgzf_asan.py) and the device inflate's
    status test (tests/test_bgzf_gpu.py) both run."""
    all_shapes = shapes()
    cases = [(z, b) for _, _, z, b in all_shapes]
    rng = np.random.default_rng(seed)
    small = [(z, b) for _, _, z, b in all_shapes if 0 < len(z) < 260_000]
    for k in range(mangled):
        z, b = small[k % len(small)]
        cases.append((mangle(rng, z, b), None))
    return cases
