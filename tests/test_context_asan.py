"""context.cpp -- sid_context_mark and the stitch of the chunks' forced edge
records -- compiled with AddressSanitizer + UndefinedBehaviorSanitizer into a
stand-alone program (tests/asan, mode context: its own main, nothing preloaded)
and run over the cases of tests/test_context.py, plus chunks whose last record
lacks its newline.  Every array it touches is an exact-size heap block.  A
sanitizer report fails the test, and every result must equal the Python
model's.  CPU only."""
import numpy as np

from context_ref import chunk_desc, dilate
from sanitized import asan, run   # noqa: F401 (asan: the fixture)
from test_context import NS, cuts, mark_cases, records


def mark_corpus():
    out = []
    for n in NS + [65, -1]:
        for code_all, sel in mark_cases(max(n, 0) if n <= 64 else 3):
            rec = "".join("x" if c else "." for c in code_all)
            s = "".join("1" if i in sel and not code_all[i] else "0" for i in range(len(code_all)))
            if 0 <= n <= 64:
                keep = dilate([ch == "1" for ch, r in zip(s, rec) if r == "."], n)
                it = iter(keep)
                want = "0 " + "".join(("1" if next(it) else "0") if r == "." else "0" for r in rec)
            else:
                want = "1 " + s   # SID_EINVAL: nothing changes
            out.append((b"M %d %d\n%s\n%s\n" % (len(rec), n, rec.encode(), s.encode()), want.encode()))
    return out


def stitch_corpus(seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for n in (1, 2, 3, 29, 64):
        m = 1200
        recs = records(rng, m)
        for sel in ([False] * m, [True] * m, [i % 211 == 0 for i in range(m)], [i in (0, m - 1) for i in range(m)],
                    [i % (2 * n + 1) == 0 for i in range(m)], list(rng.random(m) < 0.03)):
            want = b"".join(r for r, k in zip(recs, dilate(sel, n)) if k)
            for sizes in ([m], [1] * 30 + [m - 30], cuts(rng, m, n), cuts(rng, m, n),
                          [n + 1] * (m // (n + 1)) + [m % (n + 1)], [2 * n] * (m // (2 * n)) + [m % (2 * n)]):
                for newline in (True, False):
                    case, at = [b"S %d %d\n" % (n, len(sizes))], 0
                    for k, sz in enumerate(sizes):
                        rs, ss = recs[at:at + sz], sel[at:at + sz]
                        at += sz
                        d = chunk_desc(ss, [len(r) for r in rs], n)
                        z = min(n, sz)
                        keep = dilate(ss, n)
                        blob = b"".join(r for i, r in enumerate(rs) if keep[i] or i < z or i >= sz - z)
                        if not newline and at == m and blob:
                            blob = blob[:-1]   # the input's last record without its newline
                        case.append(b"C %d %d %d %d %d %d %d\n" % (len(blob), d["records"], d["has_sel"], d["lead"],
                                                                  d["trail"], d["head_keep"], d["tail_keep"]) + blob + b"\n")
                    w = want if newline or not dilate(sel, n)[-1] else want[:-1]
                    out.append((b"".join(case), b"S %d\n" % len(w) + w))
    return out


def test_corpus_sanitized(asan, tmp_path):
    cases = mark_corpus() + stitch_corpus()
    p = tmp_path / "corpus.bin"
    p.write_bytes(b"".join(c for c, _ in cases))
    assert run(asan, "context", p) == b"".join(w + b"\n" for _, w in cases)
    assert len(cases) >= 400
