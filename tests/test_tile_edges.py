"""Texts that put lines at chosen offsets of the tile parse's geometry
(sid_tile_parse_kernel, textpath.hip), and the CPU proof that they do.

A builder returns an EdgeText: the bytes and a list of claims about them,
(kind, byte_offset, ...).  The tests here check every claim from the bytes
alone, the constants the texts aim at against the sources, the conditions
under which the engine picks the lane or the quad shape for a text, the
vacuity guards of the counter texts, and sid.parse_text (parse.cpp) against
the oracle's counts and positions on every text.  tests/test_tile_edges_gpu.py
runs the same texts through the engine.

A host source's chunk has c0 = 0, so with one chunk tile k starts at text byte
k * T; a line that starts in tile k - 1 is read from LDS up to byte
k * T + H (the halo's end) and from HBM after it."""
import functools
import os
import re

import numpy as np
import pytest

T_LANE, T_QUAD = 20480, 24576     # tile bytes per shape (TP_ROWS / TP_ROWS_QUAD rows of TILE bytes)
HALO = 1024                       # tp_halo
ROW = 4096                        # TILE: an LDS-DMA row, and the index kernels' tile
CAP0 = 288                        # Dev::tile_cap of a fresh engine
CAP_QUAD = 256                    # the quad shape's largest line list
LUTN = 1024                       # SID_LUTN: -m local's table covers coverage < 1024
SHAPES = ("lane", "quad")
TILE_OF = {"lane": T_LANE, "quad": T_QUAD}
DEPTH_OF = {"lane": 30, "quad": 200}
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sid_amd", "csrc")


class EdgeText:
    """A pileup text under construction and the claims about its bytes."""

    def __init__(self, shape):
        self.shape, self.T, self.depth = shape, TILE_OF[shape], DEPTH_OF[shape]
        self.b = bytearray()
        self.site = 0
        self.claims = []

    @property
    def text(self):
        return bytes(self.b)

    def __len__(self):
        return len(self.b)

    def bases(self, n, k=None):
        """n read-base symbols, by the site's number: hom, het, a line with
        '^' and '$', one with two errors (refs in turn)."""
        k = self.site if k is None else k
        ref = b"ACGT"[k % 4:k % 4 + 1]
        alt = b"GTAC"[k % 4:k % 4 + 1]
        kind = (k // 4) % 4
        if kind == 0:
            s = (b".," * n)[:n]
        elif kind == 1:
            s = b"." * (n // 2) + alt * (n - n // 2)
        elif kind == 2 and n >= 12:
            s = b"^I." + (b",." * n)[:n - 7] + b"$" + alt.lower() * 3
        else:
            s = (b",.." * n)[:max(n - 2, 0)] + (alt + alt.lower())[:min(n, 2)]
        assert len(s) == n
        return ref, s

    def head(self, chrom=b"chr1"):
        self.site += 1
        return b"%s\t%d\t" % (chrom, self.site)

    def line(self, nb=None, bases=None, quals=None, chrom=b"chr1", nl=True):
        """Append one line; returns (start, offset of token 5, offset of token 6)."""
        nb = self.depth if nb is None else nb
        hd = self.head(chrom)
        ref, s = self.bases(nb) if bases is None else (b"ACGT"[self.site % 4:self.site % 4 + 1], bases)
        q = b"I" * len(s) if quals is None else quals
        pre = hd + b"%s\t%d\t" % (ref, len(s))
        start = len(self.b)
        self.b += pre + s + b"\t" + q + (b"\n" if nl else b"")
        return start, start + len(pre), start + len(pre) + len(s) + 1

    def exact_line(self, size, nl=True, chrom=b"chr1"):
        """A line of exactly `size` bytes (its newline included when nl): at
        most `depth` real read bases behind a run of '*' (which no count
        takes, so the site's record stays sensitive to every count), the
        qualities stretched to fit."""
        hd = self.head(chrom)
        ref = b"ACGT"[self.site % 4:self.site % 4 + 1]
        for digits in range(1, 7):
            room = size - len(hd) - 2 - digits - 1 - 1 - (1 if nl else 0)   # bases + qualities
            nb = room // 2
            if nb >= 1 and len(b"%d" % nb) == digits:
                break
        else:
            raise AssertionError(("no line of this size", size))
        real = min(nb, self.depth)
        s = b"*" * (nb - real) + self.bases(real)[1]
        start = len(self.b)
        self.b += hd + b"%s\t%d\t%s\t%s" % (ref, nb, s, b"I" * (room - nb)) + (b"\n" if nl else b"")
        assert len(self.b) - start == size
        return start

    def nominal(self):
        return 21 + 2 * self.depth   # about a filler line's bytes

    def pad_to(self, target):
        """Filler lines, the last one's read bases and qualities stretched,
        so that the next line starts exactly at byte `target`."""
        nom = self.nominal()
        assert target - len(self.b) >= nom, (len(self.b), target)
        while target - len(self.b) > 2 * nom + 40:
            self.line()
        self.exact_line(target - len(self.b))
        assert len(self.b) == target
        self.claims.append(("line_start", target))

    def finish(self, tail=3):
        for _ in range(tail):
            self.line()
        return self


def claim_errors(text, claims):
    """The claims that the bytes do not bear out."""
    bad = []
    for c in claims:
        kind, off = c[0], c[1]
        if kind == "line_start":      # a non-empty line starts at off
            ok = (off == 0 or text[off - 1:off] == b"\n") and text[off:off + 1] not in (b"\n", b"")
        elif kind == "newline":       # text[off] is a newline
            ok = text[off:off + 1] == b"\n"
        elif kind == "line_len":      # the line at off has c[2] bytes, its newline included
            ok = (off == 0 or text[off - 1:off] == b"\n") and text.find(b"\n", off) == off + c[2] - 1
        elif kind == "token":         # token c[2] (from 1) of the line at off covers [c[3], c[4])
            end = text.find(b"\n", off)
            toks, at = [], off
            for t in text[off:end if end >= 0 else len(text)].split(b"\t"):
                toks.append((at, at + len(t)))
                at += len(t) + 1
            ok = (off == 0 or text[off - 1:off] == b"\n") and len(toks) >= c[2] and toks[c[2] - 1] == (c[3], c[4])
        elif kind == "bytes":         # text[off:] starts with c[2]
            ok = text[off:off + len(c[2])] == c[2]
        elif kind == "length":        # the text has `off` bytes; c[2]: whether it ends in a newline
            ok = len(text) == off and text.endswith(b"\n") == c[2]
        else:
            ok = False
        if not ok:
            bad.append(c)
    return bad


# ---------------------------------------------------------------- families --
A_OFFSETS = list(range(-49, 18))


@functools.lru_cache(maxsize=None)
def text_a(shape):
    """A: at boundary k a line starts at k*T + d, one boundary per d in
    [-49, 17]; d = 0: the newline before it is the tile's last byte; negative
    d: the header's three 16-B windows lie across the edge."""
    e = EdgeText(shape)
    for k, d in enumerate(A_OFFSETS, 1):
        e.pad_to(k * e.T + d)
        start, t5, t6 = e.line()
        e.claims.append(("newline", start - 1))
        e.claims.append(("token", start, 5, t5, t6 - 1))
        assert start == k * e.T + d
    return e.finish()


TINY = [b"c\t7\tA\t0\t*\t*\n", b"cc\t7\tA\t0\t*\t*\n", b"cc\t17\tA\t0\t*\t*\n", b"ccc\t17\tA\t0\t*\t*\n",
        b"c\t7\tA\t0\t*\n", b"cc\t7\tA\t0\t*\n"]   # 12, 13, 14, 15, 10 and 11 bytes, depth 0


@functools.lru_cache(maxsize=None)
def text_b(shape):
    """B: at boundary k = 1..16 a run of 12 depth-0 lines of 10-15 bytes
    starts at k*T - 70 - (k - 1): the edge at each byte phase of the run."""
    e = EdgeText(shape)
    for k in range(1, 17):
        at = k * e.T - 70 - (k - 1)
        e.pad_to(at)
        for i in range(12):
            ln = TINY[(i + k) % len(TINY)]
            e.claims.append(("line_len", len(e.b), len(ln)))
            e.b += ln
        assert at < k * e.T < len(e.b)
        e.claims.append(("line_start", len(e.b)))
    return e.finish()


C_ENDS = list(range(-20, 21))
C_STARTS = (1, 40)
C_PAIRS = (b"^I", b"+2AC", b"$.", b"\tI")   # the constructs whose first byte is the last byte read from LDS


@functools.lru_cache(maxsize=None)
def text_c(shape, variant):
    """C: a line starts at k*T - s (s in 1, 40), so in tile k - 1, and its
    newline is at k*T + H + e, e in [-20, 20], across the end of that tile's
    halo.  Variant 1: token 5 runs to the line's end (one quality byte after
    it); variant 2: token 5 has 30 bases and token 6 runs across.  Then four
    lines with a two-byte construct at k*T + H - 1, the last byte read from
    LDS: '^I', '+2AC' (the general routine), '$' and the separator of tokens
    5 and 6."""
    e = EdgeText(shape)
    k = 0
    for s in C_STARTS:
        for end in C_ENDS:
            k += 1
            start, nl = k * e.T - s, k * e.T + HALO + end
            e.pad_to(start)
            hd = e.head()
            pre = hd + b"A\t30\t"
            room = nl - start - len(pre) - 1       # bases + qualities
            real = e.bases(30, k)[1]
            if variant == 1:
                s5, q = b"*" * (room - 31) + real, b"I"
            else:
                s5, q = real, b"I" * (room - 30)
            e.b += pre + s5 + b"\t" + q + b"\n"
            t5 = start + len(pre)
            e.claims += [("line_len", start, nl + 1 - start), ("newline", nl), ("token", start, 5, t5, t5 + len(s5)),
                         ("token", start, 6, t5 + len(s5) + 1, nl)]
            assert start < k * e.T and len(e.b) == nl + 1
    for pair in C_PAIRS:
        k += 1
        start, at = k * e.T - 40, k * e.T + HALO - 1
        e.pad_to(start)
        pre = e.head() + b"A\t30\t"
        t5 = start + len(pre)
        real = e.bases(30, k)[1]
        if pair == b"\tI":   # token 5 ends at `at`, token 6 starts behind it
            s5 = b"*" * (at - t5 - 30) + real
            e.b += pre + s5 + b"\t" + b"I" * 30 + b"\n"
            e.claims.append(("token", start, 5, t5, at))
        else:
            s5 = b"*" * (at - t5 - 15) + real[:15] + pair + real[15:]
            e.b += pre + s5 + b"\t" + b"I" * 30 + b"\n"
            e.claims.append(("token", start, 5, t5, t5 + len(s5)))
        e.claims.append(("bytes", at, pair))
        assert at == (k - 1) * e.T + e.T + HALO - 1
    return e.finish()


def d_ends(shape, form="short"):
    """D: the chunk's end c1 (the text's length): T + e and T + H + e for
    every second e in [-17, 17] and the window-aligned 0 and +-16 (all 35
    would take the file past its budget of oracle processes), one byte around
    every 4 KiB row, and 2T +- 1.  The long last line starts before T, so it
    takes the ends from T - 17 on."""
    T = TILE_OF[shape]
    es = sorted(set(range(-17, 18, 2)) | {-16, 0, 16})
    ends = {T + x for x in es} | {T + HALO + x for x in es}
    ends |= {ROW * r + x for r in range(1, 6) for x in (-1, 0, 1)} | {2 * T - 1, 2 * T + 1}
    return sorted((c for c in ends if form == "short" or c >= T - 17), reverse=True)   # longest first


@functools.lru_cache(maxsize=None)
def text_d(shape, c1, form, nl):
    """The text of c1 bytes, with or without a final newline, whose last
    line is short (about a filler line) or long (from before T to c1)."""
    e = EdgeText(shape)
    last = c1 - (e.nominal() + 3) if form == "short" else e.T - 100
    e.pad_to(last)
    e.exact_line(c1 - last, nl=nl)
    e.claims += [("length", c1, nl), ("line_start", last)]
    if nl:
        e.claims.append(("line_len", last, c1 - last))
    return e


E_FIRST = {"tiny": b"c\t7\tA\t0\t*\n", "plain": None}   # 9 bytes and a newline, depth 0; or an ordinary line


@functools.lru_cache(maxsize=None)
def text_e(shape, first):
    """E: a first line and text A up to the first line end past three tiles."""
    a = text_a(shape).text
    body = a[:a.index(b"\n", 3 * TILE_OF[shape]) + 1]
    head = E_FIRST[first]
    if head is None:
        x = EdgeText(shape)
        x.line(chrom=b"chr0")
        head = x.text
    e = EdgeText(shape)
    e.b += head + body
    e.claims += [("line_len", 0, len(head)), ("line_start", len(head))]
    return e


def surround(before, after=256):
    """Valid-looking pileup lines to put around a device text: exactly
    `before` bytes whose last 10 are a whole line (a line start in the first
    window, before c0, for s >= 10), and `after` bytes that begin with one (a
    line start at c1 itself)."""
    x = EdgeText("lane")
    for _ in range(8):
        x.line(chrom=b"chrS")
    t = x.text
    return (t + TINY[4])[-before:], (TINY[4] + t)[:after]


GEOMETRY = [("A", text_a, ()), ("B", text_b, ()), ("C1", text_c, (1,)), ("C2", text_c, (2,))]


def geometry_texts(shape):
    return [(name, f(shape, *args)) for name, f, args in GEOMETRY]


# ------------------------------------------------- counter texts (section 3) --
RUNS = [1007, 1008, 1009, 1023, 1024, 1025, 2015, 2016, 2017, 4095, 4096, 4097, 65535, 65536, 65537]
ALIGN = (0, 1, 15)
SYMBOLS = [(bytes([c]), b"A") for c in b"ACGTacgt"] + [(s, bytes([r])) for s in (b".", b",") for r in b"ACGT"]


def second_base(sym, ref):
    first = (ref if sym in b".," else sym).upper()
    return b"GTAC"[b"ACGT".index(first):][:1]


def second_run(n):
    """The second run's length: a fifth of the first up to 4097 -- there both
    of -m local's p-values move with every count (the CPU guard below proves
    it per line); past it the first run's count wraps or the p-values
    underflow to 0 whatever the second run is, and the Lynch table's exact
    counts alone stand."""
    return n // 5 if n <= 4097 else 40


def counter_lines(align, indel=False):
    """(line, read bases, ref, n) per probe: a run of n copies of one symbol
    starting at window offset `align`, then the second run ('+2AC' appended:
    the general routine)."""
    out = []
    site = 0
    for sym, ref in SYMBOLS:
        for n in RUNS:
            site += 1
            s5 = sym * n + second_base(sym, ref) * second_run(n) + (b"+2AC" if indel else b"")
            depth = b"%d" % (n + second_run(n))
            pos = b"%d" % site
            # the chrom's length puts token 5 at the wanted offset of its window
            fixed = 1 + len(pos) + 1 + 1 + 1 + len(depth) + 1
            chrom = b"k" * ((align - fixed) % 16 or 16)
            pre = b"%s\t%s\t%s\t%s\t" % (chrom, pos, ref, depth)
            assert len(pre) % 16 == align
            quals = b"I" * min(len(s5), 100 if n > 4097 else len(s5))
            out.append((pre + s5 + b"\t" + quals + b"\n", s5, ref, n))
    return out


@functools.lru_cache(maxsize=None)
def counter_text(align, indel=False):
    """Every line starts a 16-B window (the lines before it padded by their
    qualities), so token 5 starts at window offset `align`."""
    b = bytearray()
    claims = []
    for ln, s5, ref, n in counter_lines(align, indel):
        if len(b) % 16:   # stretch the previous line's qualities
            b[-1:] = b"I" * (16 - len(b) % 16) + b"\n"
        t5 = len(b) + ln.index(s5)
        claims += [("line_start", len(b)), ("token", len(b), 5, t5, t5 + len(s5))]
        assert t5 % 16 == align
        b += ln
    return bytes(b), claims


def counter_counts(oracle, align, indel=False):
    return np.array([oracle.read_bases(s5, ref) for _, s5, ref, _ in counter_lines(align, indel)], np.uint16)


# ------------------------------------------------------------------- tests --
def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_match_the_sources():
    msg = "the tile parse's geometry changed: retarget the edge texts"
    tp, run, math = source("textpath.hip"), source("run.cpp"), source("sid_math.h")

    def const(src, pattern):
        m = re.search(pattern, src)
        assert m, (msg, pattern)
        return int(m.group(1))
    tb = const(tp, r"constexpr int TB = (\d+);")
    assert re.search(r"constexpr int TILE = TB \* 16;", tp), msg
    tile = tb * 16
    assert tile == ROW, msg
    assert const(tp, r"constexpr uint32_t TP_ROWS = (\d+);") * tile == T_LANE, msg
    assert const(tp, r"constexpr uint32_t TP_ROWS_QUAD = (\d+);") * tile == T_QUAD, msg
    assert const(tp, r"tp_halo\(bool\) \{ return (\d+); \}") == HALO, msg
    assert const(run, r"uint32_t tile_cap = (\d+);") == CAP0, msg
    assert len(re.findall(r"tile_cap = 288;", run)) == 2, msg   # the member's default and tile_reset
    assert const(math, r"#define SID_LUTN (\d+)") == LUTN, msg


def shape_facts(text, T):
    """(mean line length, the most line starts in a tile of T bytes)."""
    a = np.frombuffer(text, np.uint8)
    nl = np.flatnonzero(a == 10)
    starts = np.concatenate([[0], nl + 1])
    starts = starts[starts < len(a)]
    starts = starts[a[starts] != 10]
    return len(a) / len(starts), int(np.bincount(starts // T).max())


def all_edge_texts():
    for shape in SHAPES:
        for name, e in geometry_texts(shape):
            yield f"{name}-{shape}", shape, e
        for first in E_FIRST:
            yield f"E-{first}-{shape}", shape, text_e(shape, first)
        for form in ("short", "long"):
            for c1 in d_ends(shape, form):
                for nl in (True, False):
                    yield f"D-{c1}-{form}-{nl}-{shape}", shape, text_d(shape, c1, form, nl)


@pytest.mark.parametrize("shape", SHAPES)
def test_every_claim_holds(shape):
    n = 0
    for name, sh, e in all_edge_texts():
        if sh != shape:
            continue
        assert e.claims, name
        assert claim_errors(e.text, e.claims) == [], name
        n += len(e.claims)
    assert n > 1000
    for align in ALIGN:
        for indel in (False, True):
            text, claims = counter_text(align, indel)
            assert claim_errors(text, claims) == [], (align, indel)


def test_a_wrong_claim_is_caught():
    e = text_a("lane")
    for c in (("line_start", T_LANE + 3), ("newline", T_LANE), ("line_len", A_OFFSETS[0] + T_LANE, 5),
              ("token", A_OFFSETS[0] + T_LANE, 5, 1, 2), ("bytes", 0, b"x"), ("length", 5, True)):
        assert claim_errors(e.text, [c]) == [c]


@pytest.mark.parametrize("shape", SHAPES)
def test_shape_conditions(shape):
    """What makes the engine parse a text with the intended shape: the lane
    shape on a fresh engine's first chunk if no 20 KiB tile has more than 288
    line starts (and a mean of at most 256 B keeps it for the runs after);
    the quad shape after a 200x text while the mean stays above 256 B and no
    24 KiB tile has more than 256 line starts."""
    T = TILE_OF[shape]
    for name, sh, e in all_edge_texts():
        if sh != shape:
            continue
        mean, most = shape_facts(e.text, T)
        if shape == "lane":
            assert mean <= 256 and most <= CAP0, (name, mean, most)
        else:
            assert mean > 256 and most <= CAP_QUAD, (name, mean, most)
    # the counter texts: long lines, few a tile, in either shape
    text, _ = counter_text(0)
    mean, most = shape_facts(text, T)
    assert mean > 256 and most <= CAP_QUAD


def test_geometry_reaches_the_edges():
    """The texts hit what they aim at (from the claims just proven)."""
    for shape in SHAPES:
        T = TILE_OF[shape]
        a = text_a(shape)
        assert sorted(c[1] - (c[1] + 100) // T * T for c in a.claims if c[0] == "token") == A_OFFSETS
        nls = sorted(c[1] % T - HALO for c in text_c(shape, 1).claims if c[0] == "newline")
        assert nls == sorted(C_ENDS * len(C_STARTS))
        assert {c[1] % T for c in text_c(shape, 2).claims if c[0] == "bytes"} == {HALO - 1}
        ends = d_ends(shape)
        assert {T, T + 1, T + HALO, ROW + 1, 2 * T - 1} <= set(ends) and len(ends) >= 56


def printed(oracle, counts):
    """What -m local prints of a site but its name: the code and both
    confidences as the CSV's %g shows them."""
    code, h, t = oracle.call_local(np.asarray(counts, np.uint16))
    return [(int(c), "%g" % x, "%g" % y) for c, x, y in zip(code, h, t)]


def test_counter_lines_are_sensitive(oracle):
    """Vacuity guard of the CSV comparison: the record of every probe line up
    to 4097 differs from the record of the same site with one count less in
    either base, and with 1024 less in one base and one more in any other --
    a counter's field spilt into its neighbour.  The lines past 4097 wrap a
    u16 count (65536, 65537) or have p-values of 0 and 1 whatever the second
    run (65535): for them the exact counts of the Lynch table alone stand
    (test_tile_edges_gpu.test_counter_profiles); no probe line has a coverage
    below 4."""
    counts = counter_counts(oracle, 0)
    lines = counter_lines(0)
    assert len(counts) == len(SYMBOLS) * len(RUNS)
    checked = 0
    for (ln, s5, ref, n), c in zip(lines, counts.astype(np.int64)):
        if n > 4097:
            assert sorted(c.tolist())[2:] == sorted([second_run(n), n % 65536]), (s5[:1], ref, n)
            continue
        i, j = [k for k in range(4) if c[k]]
        hi, lo = (i, j) if c[i] == n else (j, i)
        assert c[hi] == n and c[lo] == second_run(n) and c.sum() == n + second_run(n) >= 4
        variants = []
        for k in (hi, lo):
            v = c.copy()
            v[k] -= 1
            variants.append(v)
        if n >= 1024:
            for k in range(4):
                if k != hi:
                    v = c.copy()
                    v[hi] -= 1024
                    v[k] += 1
                    variants.append(v)
        recs = printed(oracle, np.array([c] + variants))
        assert all(r != recs[0] for r in recs[1:]), (s5[:1], ref, n, recs)
        checked += 1
    assert checked == len(SYMBOLS) * 12


def oracle_parse(oracle, text):
    """Counts and positions of a text's sites by the oracle's read_bases."""
    counts, pos = [], []
    for ln in text.split(b"\n"):
        if not ln:
            continue
        tok = ln.split(b"\t")
        pos.append(int(tok[1]))
        counts.append(oracle.read_bases(tok[4], tok[2]))
    return np.array(counts, np.uint16).reshape(-1, 4), np.array(pos, np.int32)


def assert_host_parse(sid, oracle, text, what):
    s = sid.parse_text(text)
    counts, pos = oracle_parse(oracle, text)
    assert np.array_equal(s.positions, pos), what
    assert np.array_equal(s.counts, counts), what


@pytest.mark.parametrize("shape", SHAPES)
def test_host_parser_on_the_geometry_texts(sid, oracle, shape):
    for name, e in geometry_texts(shape):
        assert_host_parse(sid, oracle, e.text, name)
    for first in E_FIRST:
        assert_host_parse(sid, oracle, text_e(shape, first).text, first)
    for form in ("short", "long"):
        for c1 in d_ends(shape, form):
            for nl in (True, False):
                assert_host_parse(sid, oracle, text_d(shape, c1, form, nl).text, (c1, form, nl))


@pytest.mark.parametrize("indel", [False, True], ids=["plain", "indel"])
@pytest.mark.parametrize("align", ALIGN)
def test_host_parser_on_the_counter_texts(sid, oracle, align, indel):
    text, _ = counter_text(align, indel)
    s = sid.parse_text(text)
    assert np.array_equal(s.counts, counter_counts(oracle, align, indel))
    assert s.positions.tolist() == list(range(1, len(SYMBOLS) * len(RUNS) + 1))
