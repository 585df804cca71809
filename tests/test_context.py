"""--context N on the host (CPU only): sid_context_mark, the host path's mark,
and the stitch of the chunks' forced edge records (sid_amd/csrc/context.cpp),
both against the Python model of tests/context_ref.py."""
import ctypes as C

import numpy as np
import pytest

from context_ref import MAXN, chunk_desc, dilate, mark_model

DROPPED, HET = 0x40, 0x80
NS = [0, 1, 2, 64]


class Desc(C.Structure):
    """sid_cx_desc (sid_amd/csrc/context.h)."""
    _fields_ = [("records", C.c_uint32), ("has_sel", C.c_uint32), ("lead", C.c_uint32), ("trail", C.c_uint32),
                ("head_keep", C.c_uint64), ("tail_keep", C.c_uint64),
                ("head_len", C.c_uint32 * MAXN), ("tail_len", C.c_uint32 * MAXN)]


def make_desc(m) -> Desc:
    d = Desc(m["records"], m["has_sel"], m["lead"], m["trail"], m["head_keep"], m["tail_keep"])
    for k, v in enumerate(m["head_len"]):
        d.head_len[k] = v
    for k, v in enumerate(m["tail_len"]):
        d.tail_len[k] = v
    return d


def mark_cases(n):
    """(code_all, selected sites): the placements the contract names, for context n."""
    m = max(6 * n + 9, 12)
    plain = [0] * m
    out = [(plain, []), (plain, list(range(m))), (plain, [0]), (plain, [m - 1]), (plain, [0, m - 1]),
           (plain, [3, 4]), (plain, [1, 1 + 2 * n]), (plain, [1, 2 + 2 * n]), (plain, [2, 3 + 2 * n, 4 + 4 * n])]
    # dropped sites between a selected site and its neighbours: the distance is in records
    gaps = [0] * m
    for i in range(2, m, 3):
        gaps[i] = DROPPED
    out += [(gaps, [0]), (gaps, [m // 2 if gaps[m // 2] == 0 else m // 2 + 1]), (gaps, [i for i in range(m) if i % 7 == 0 and not gaps[i]])]
    run = [0] * 3 + [DROPPED] * (2 * n + 5) + [0] * 4
    out += [(run, [2]), (run, [len(run) - 4]), (run, [0, len(run) - 1])]
    out += [([DROPPED] * 9, []), ([], [])]
    return out


@pytest.mark.parametrize("n", NS)
def test_mark_against_the_model(sid, n):
    for code_all, sel in mark_cases(n):
        rng = np.random.default_rng(len(code_all) + 31 * len(sel))
        base = [c | (HET if rng.integers(2) else 0) | int(rng.integers(16)) for c in code_all]
        code = [c if i in sel else c | DROPPED for i, c in enumerate(base)]
        got = sid.context_mark(np.array(base, dtype=np.uint8), np.array(code, dtype=np.uint8), n)
        assert got.tolist() == mark_model(base, code, n), (n, code_all, sel)
        assert (np.array(code, dtype=np.uint8) & ~np.uint8(DROPPED) == got & ~np.uint8(DROPPED)).all()   # only bit 6 moves
        if n == 0:
            assert got.tolist() == code


def test_mark_counts_records_not_sites(sid):
    a = np.array([0, 0, HET, 0, DROPPED, 0, 0, 0, 0], dtype=np.uint8)
    c = sid.select_mark(a, "het")
    assert sid.context_mark(a, c, 2).tolist() == [0, 0, HET, 0, DROPPED, 0, DROPPED, DROPPED, DROPPED]
    assert sid.context_mark(a, c, 1).tolist() == [DROPPED, 0, HET, 0, DROPPED, DROPPED, DROPPED, DROPPED, DROPPED]


def test_mark_rejects(sid):
    L = sid.lib()
    a = np.zeros(4, dtype=np.uint8)
    p = a.ctypes.data_as(C.c_void_p)
    for n in (-1, 65, 1 << 20):
        assert L.sid_context_mark(p, p, 4, n) == 1
        with pytest.raises(sid.SidError) as ei:
            sid.context_mark(a, a, n)
        assert ei.value.status == 1
    assert L.sid_context_mark(None, p, 4, 2) == 1
    assert L.sid_context_mark(p, None, 4, 2) == 1
    assert L.sid_context_mark(None, None, 0, 2) == 0
    with pytest.raises(sid.SidError):
        sid.context_mark(np.zeros(3, dtype=np.uint8), np.zeros(4, dtype=np.uint8), 1)


def test_opts_field_and_builder(sid):
    o = sid.make_opts()
    assert o.context == 0 and sid.Opts._fields_[-1][0] == "context"
    assert sid.make_opts(select="het", context=7).context == 7


def records(rng, m):
    """m record lines of varied length."""
    return [b"c%d,%d,hom,AA,1,0,p_value\n" % (int(rng.integers(1, 10 ** int(rng.integers(1, 6)))), i) for i in range(m)]


def stitch(sid, recs, sel, sizes, n):
    """The records cut into chunks of `sizes`, each forced and described as a chunk alone would be, through
    sid_cx_stitch_chunks -> the bytes that stay."""
    descs, blobs, at = [], [], 0
    for sz in sizes:
        rs, ss = recs[at:at + sz], sel[at:at + sz]
        at += sz
        m = chunk_desc(ss, [len(r) for r in rs], n)
        keep = dilate(ss, n)
        z = min(n, sz)
        forced = [k or i < z or i >= sz - z for i, k in enumerate(keep)]   # what the chunk's writer emits
        m["head_len"] = [len(r) for r in rs[:z]]
        m["tail_len"] = [len(r) for r in rs[sz - z:]] if z else []
        descs.append(make_desc(m))
        blobs.append(b"".join(r for r, f in zip(rs, forced) if f))
    assert at == len(recs)
    arr = (Desc * max(len(descs), 1))(*descs)
    buf = C.create_string_buffer(b"".join(blobs), max(sum(map(len, blobs)), 1))
    off = np.cumsum([0] + [len(b) for b in blobs[:-1]]).astype(np.uint64) if blobs else np.zeros(1, dtype=np.uint64)
    ln = np.array([len(b) for b in blobs] or [0], dtype=np.uint64)
    rc = sid.lib().sid_cx_stitch_chunks(arr, len(descs), n, buf, off.ctypes.data_as(C.c_void_p),
                                        ln.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return b"".join(buf.raw[int(o):int(o) + int(k)] for o, k in zip(off[:len(descs)], ln[:len(descs)]))


def cuts(rng, total, n):
    """Chunk sizes that sum to `total`: 1, n - 1, n, n + 1, 2n, 2n + 1 and 500, empty chunks among them."""
    pool = sorted({1, max(n - 1, 0), n, n + 1, 2 * n, 2 * n + 1, 500, 0})
    out = []
    while total:
        s = min(int(pool[int(rng.integers(len(pool)))]), total)
        out.append(s)
        total -= s
    return out + [0]


@pytest.mark.parametrize("n", [1, 2, 3, 29, 64])
def test_stitch_against_the_model(sid, n):
    L = sid.lib()
    L.sid_cx_stitch_chunks.restype = C.c_int
    rng = np.random.default_rng(100 + n)
    m = 2500
    recs = records(rng, m)
    placements = {
        "none": [False] * m,
        "every": [True] * m,
        "sparse": [i % 211 == 0 for i in range(m)],
        "ends": [i in (0, m - 1) for i in range(m)],
        "2n": [i % (2 * n) == 0 for i in range(m)],
        "2n+1": [i % (2 * n + 1) == 0 for i in range(m)],
        "2n+2": [i % (2 * n + 2) == 0 for i in range(m)],
        "runs": [(i // 300) % 3 == 1 and i % 5 == 0 for i in range(m)],   # long runs of chunks without a selected record
        "random": list(rng.random(m) < 0.02),
    }
    for name, sel in placements.items():
        want = b"".join(r for r, k in zip(recs, dilate(sel, n)) if k)
        shapes = [[m], [1] * 40 + [m - 40], [n] * 7 + [m - 7 * n], [m - 3, 0, 0, 1, 1, 1]]
        shapes += [cuts(rng, m, n) for _ in range(6)]
        for k in (1, max(n - 1, 1), n, n + 1, 2 * n, 2 * n + 1, 500):
            shapes.append([k] * (m // k) + ([m % k] if m % k else []))
        for sizes in shapes:
            assert stitch(sid, recs, sel, sizes, n) == want, (n, name, sizes[:12])


def test_stitch_rejects(sid):
    L = sid.lib()
    assert L.sid_cx_stitch_chunks(None, 0, 65, None, None, None) == 1
    assert L.sid_cx_stitch_chunks(None, 0, -1, None, None, None) == 1
    assert L.sid_cx_stitch_chunks(None, 2, 2, None, None, None) == 1
    assert L.sid_cx_stitch_chunks(None, 0, 2, None, None, None) == 0
