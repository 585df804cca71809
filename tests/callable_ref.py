"""A Python restatement of --callable FILE (sid_callable_host, sid_dtext_callable), for the
tests: the rows from per-site (chrom, pos, code, depth), the model of the
per-chunk row lists with their edge bits that the stitch is fed, the stitch and
the BED format.  Nothing here calls the library; the codes come from
windows_ref.site_codes (the oracle over the host parser's counts), the depths
from depth_ref.depths."""
import ctypes as C

DROPPED, HET = 0x40, 0x80
HAS_SITE, OPEN_START, OPEN_END = 1, 2, 4


def is_callable(pos: int, code: int, depth: int, lo: int, hi: int) -> bool:
    """A record in the unselected output, a depth >= 1 within the bounds, a pos that BED can hold."""
    return (not code & DROPPED) and depth >= 1 and lo <= depth and (hi == 0 or depth <= hi) and pos >= 1


def flags(sites, codes, depths, lo=0, hi=0):
    return [is_callable(p, c, d, lo, hi) for (_, p), c, d in zip(sites, codes, depths)]


def rows(sites, codes, depths, lo=0, hi=0):
    """[(chrom, start, end, het)]: a row per maximal run of consecutive sites that are all callable, with
    equal chrom and each pos the previous pos + 1 (Python's integers: 2^31-1 has no successor among the
    positions atoi gives)."""
    out, prev = [], None   # prev: the previous site, if it was callable
    for (chrom, pos), c, d in zip(sites, codes, depths):
        if not is_callable(pos, c, d, lo, hi):
            prev = None
            continue
        if prev is not None and prev == (chrom, pos - 1):
            out[-1][2] = pos
        else:
            out.append([chrom, pos - 1, pos, 0])
        out[-1][3] += bool(c & HET)
        prev = (chrom, pos)
    return [tuple(r) for r in out]


def chunk_model(sites, codes, depths, cuts, lo=0, hi=0):
    """Every chunk alone: chunk j holds the sites [cuts[j], cuts[j + 1]).  Per chunk (rows, edge): whether it
    has a site, whether its first site lies in its first row, whether its last site lies in its last row."""
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        f = flags(sites[a:b], codes[a:b], depths[a:b], lo, hi)
        edge = (HAS_SITE if f else 0) | (OPEN_START if f and f[0] else 0) | (OPEN_END if f and f[-1] else 0)
        out.append((rows(sites[a:b], codes[a:b], depths[a:b], lo, hi), edge))
    return out


def join(a, a_open_end, b, b_open_start):
    """Two row lists that are neighbours in file order: the boundary rows merge only when both flags are set,
    the chroms are equal and b's start is a's end."""
    a, b = [tuple(r) for r in a], [tuple(r) for r in b]
    if a and b and a_open_end and b_open_start and a[-1][0] == b[0][0] and b[0][1] == a[-1][2]:
        return a[:-1] + [(a[-1][0], a[-1][1], b[0][2], a[-1][3] + b[0][3])] + b[1:]
    return a + b


def stitch(chunks):
    """The chunks' (rows, edge) in file order into the run's rows: chunks without a site are transparent."""
    out, open_end = [], False
    for rs, edge in chunks:
        if not edge & HAS_SITE:
            assert not rs and not edge
            continue
        out = join(out, open_end, rs, bool(edge & OPEN_START))
        open_end = bool(rs) and bool(edge & OPEN_END)
    return out


def fmt(rs) -> bytes:
    return b"".join(b"%s\t%d\t%d\t%d\n" % tuple(r) for r in rs)


def total_sites(rs) -> int:
    return sum(r[2] - r[1] for r in rs)


class Row(C.Structure):
    """sid_call_row (sid_amd/csrc/callable.h): a chunk's row as the device writes it."""
    _fields_ = [("c8", C.c_uint64), ("pos", C.c_int32), ("clen", C.c_uint32), ("name", C.c_uint32),
                ("sites", C.c_uint32), ("het", C.c_uint32), ("pad", C.c_uint32)]


def device_rows(chunks):
    """The chunks' (rows, edge) in the device's layout: (Row array, off, names, noff, edge) for
    sid_callable_stitch_chunks."""
    flat, off, names, noff, edges = [], [0], b"", [0], []
    for rs, edge in chunks:
        blob = b""
        for chrom, start, end, het in rs:
            r = Row(int.from_bytes(chrom[:8], "little"), start + 1, len(chrom), 0, end - start, het, 0)
            if len(chrom) > 8:
                r.name = len(blob)
                blob += chrom
            flat.append(r)
        names += blob
        off.append(len(flat))
        noff.append(len(names))
        edges.append(edge)
    arr = (Row * max(len(flat), 1))(*flat)
    return (arr, (C.c_uint64 * len(off))(*off), names, (C.c_uint64 * len(noff))(*noff),
            (C.c_uint32 * max(len(edges), 1))(*edges))
