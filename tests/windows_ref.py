"""A Python restatement of --windows W (sid_opts.window), for the tests: the
rows from per-site (chrom, pos, code), their CSV, and the model of the
per-chunk row lists that the stitch is fed.  Nothing here calls the library;
site_codes gets the per-site codes from the oracle over the host parser's
counts, as the other GPU tests get theirs."""
import ctypes as C

from regions_ref import text_sites

DROPPED, HET = 0x40, 0x80
HEADER = b"chrom,start,end,sites,records,het,hom\n"
WMAX = 2 ** 31 - 1


def win_index(pos: int, w: int) -> int:
    return (pos - 1) // w   # (Python's // is the floor, for negative numbers too)


def rows(sites, codes, w):
    """[(chrom, start, end, sites, records, het, hom)]: a row per maximal run of
    consecutive sites with equal chrom and equal window index."""
    out, key = [], None
    for (chrom, pos), c in zip(sites, codes):
        k = (chrom, win_index(pos, w))
        if k != key:
            out.append([chrom, k[1] * w, k[1] * w + w, 0, 0, 0, 0])
            key = k
        r = out[-1]
        rec = not c & DROPPED
        het = bool(rec and c & HET)
        r[3] += 1
        r[4] += rec
        r[5] += het
        r[6] += rec and not het
    return [tuple(r) for r in out]


def chunk_rows(sites, codes, w, cuts):
    """The rows of every chunk alone: chunk j holds the sites [cuts[j], cuts[j + 1])."""
    return [rows(sites[a:b], codes[a:b], w) for a, b in zip(cuts[:-1], cuts[1:])]


def stitch(chunks):
    """The chunks' row lists into the run's rows: a row merges into the one in
    front of it when chrom and start are equal -- across chunks only, since a
    chunk's own neighbours differ."""
    out = []
    for ch in chunks:
        for r in ch:
            if out and out[-1][:2] == list(r[:2]):
                for k in range(3, 7):
                    out[-1][k] += r[k]
            else:
                out.append(list(r))
    return [tuple(r) for r in out]


def fmt(rs, header=True) -> bytes:
    return (HEADER if header else b"") + b"".join(b"%s,%d,%d,%d,%d,%d,%d\n" % r for r in rs)


def site_codes(sid, oracle, text: bytes, method="local", estimate_prior=False, **kw):
    """([(chrom, pos)], [code]) of the text's sites: the oracle's call over the host parser's counts."""
    sites = text_sites(text)
    if method == "quality":
        rc, code, _, _ = oracle.call_quality(text, estimate_prior=estimate_prior, **kw)
        assert rc == 0
    elif method == "local" and not estimate_prior:
        code = oracle.call_local(sid.parse_text(text).counts, **kw)[0]
    else:
        rc, code, _, _, _, _ = oracle.call_method(sid.parse_text(text).counts, method, estimate_prior=estimate_prior, **kw)
        assert rc == 0
    assert len(code) == len(sites)
    return sites, [int(c) for c in code]


class Row(C.Structure):
    """sid_win_row (sid_amd/csrc/windows.h): a chunk's row as the device writes it."""
    _fields_ = [("wi", C.c_int64), ("c8", C.c_uint64), ("clen", C.c_uint32), ("name", C.c_uint32),
                ("sites", C.c_uint32), ("records", C.c_uint32), ("het", C.c_uint32), ("pad", C.c_uint32)]


def device_rows(chunks, w):
    """The chunks' row lists in the device's layout: (Row array, off, names, noff) for sid_win_stitch_chunks."""
    flat, off, names, noff = [], [0], b"", [0]
    for ch in chunks:
        blob = b""
        for chrom, start, _, ns, nr, nh, _ in ch:
            r = Row(start // w, int.from_bytes(chrom[:8], "little"), len(chrom), 0, ns, nr, nh, 0)
            if len(chrom) > 8:
                r.name = len(blob)
                blob += chrom
            flat.append(r)
        names += blob
        off.append(len(flat))
        noff.append(len(names))
    arr = (Row * max(len(flat), 1))(*flat)
    return arr, (C.c_uint64 * len(off))(*off), names, (C.c_uint64 * len(noff))(*noff)
