"""The line stripper (sid_strip_lines, sid_amd/csrc/strip.cpp): the copy of a
pileup text without its quality columns that the engine's strip crews upload.
Its properties, the vector variants against the scalar one byte for byte, the
hand-made lines, and -- what makes it safe -- the oracle CLI giving the same
stdout, stderr and return code on the stripped text as on the original, for
every method that reads no quality column.  CPU only."""
import gzip
import os

import numpy as np
import pytest

from test_parser import blank, fuzz_lines

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANTS = {"scalar": 1, "avx2": 2, "avx512": 3}
L6 = b"chr1\t100\tA\t3\t.,.\tIII\n"           # 6 tokens: the usual line
S6 = b"chr1\t100\tA\t3\t.,.\n"                # ... stripped


def model(text: bytes) -> bytes:
    """The stripper restated: the semantics of strip.h, line by line."""
    out = []
    for line in text.split(b"\n")[:-1]:
        toks, i, n = [], 0, len(line)
        while len(toks) < 5:
            while i < n and line[i] in b" \t":
                i += 1
            if i == n:
                break
            a = i
            while i < n and line[i] not in b" \t":
                i += 1
            toks.append((a, i))
        if len(toks) == 5 and not any(c < 0x20 and c != 9 for c in line[:toks[4][1]]):
            out.append(line[:toks[4][1]])
        else:
            out.append(line)
    tail = text.split(b"\n")[-1]
    return b"".join(l + b"\n" for l in out) + tail


def variants(sid):
    return {k: v for k, v in VARIANTS.items() if sid.strip_lines(b"", v) is not None}


@pytest.fixture(scope="module")
def fuzz_text():
    """2,000 seeded lines: synthetic sites, damaged ones, odd separators."""
    rng = np.random.default_rng(20261)
    import sid_amd
    good = sid_amd.synth_text(5, 1200, 30.0, sites_per_chrom=500).split(b"\n")[:-1]
    good += sid_amd.synth_text(6, 300, 200.0).split(b"\n")[:-1]
    out = []
    for i in range(2000):
        l = bytearray(good[int(rng.integers(len(good)))])
        r = rng.random()
        if r < 0.25:
            for _ in range(int(rng.integers(1, 4))):
                k = int(rng.integers(len(l)))
                l[k:k + 1] = [b"\t", b" ", b"\t\t ", b"\r", b"\0", b"", b"\x01", b"\x7f", b"\xff", b"\n"][int(rng.integers(10))]
        elif r < 0.35:
            l = l[:int(rng.integers(len(l) + 1))]
        elif r < 0.40:
            l = b" \t" + l
        elif r < 0.45:
            l = l.replace(b"\t", b" ")
        out.append(bytes(l))
    return b"\n".join(out) + b"\n"


def test_hand_made_lines(sid):
    cases = [
        (L6, S6),
        (b"chr1 \t 100\t\tA  3 \t.,.\t \tIII\n", b"chr1 \t 100\t\tA  3 \t.,.\n"),     # runs of separators
        (b"chr1 100 A 3 .,. III\n", b"chr1 100 A 3 .,.\n"),                           # spaces
        (b" \t chr1\t100\tA\t3\t.,.\tIII\n", b" \t chr1\t100\tA\t3\t.,.\n"),          # leading separators
        (b"chr1\t100\tA\t3\n", b"chr1\t100\tA\t3\n"),                                 # 4 tokens: whole
        (b"chr1\t100\tA\t3\t\n", b"chr1\t100\tA\t3\t\n"),
        (S6, S6),                                                                     # 5 tokens
        (b"chr1\t100\tA\t3\t.,.\t\n", S6),                                            # ... and a separator
        (L6[:-1] + b"\t]]]\n", S6),                                                   # 7 tokens
        (b"\n", b"\n"),                                                               # an empty line
        (b"\n\n" + L6 + b"\n", b"\n\n" + S6 + b"\n"),
        (L6 + L6[:-1], S6 + L6[:-1]),                                                 # no final newline: whole
        (L6[:-1], L6[:-1]),
        (L6[:-1] + b"\r\n", S6),                                                      # CR behind the cut goes
        (b"chr1\t100\tA\t3\t.,.\r\n", b"chr1\t100\tA\t3\t.,.\r\n"),                   # CR in the 5th token: whole
        (b"chr1\t1\r00\tA\t3\t.,.\tIII\n", b"chr1\t1\r00\tA\t3\t.,.\tIII\n"),
        (b"chr1\t100\tA\t3\t.\0.\tIII\n", b"chr1\t100\tA\t3\t.\0.\tIII\n"),           # NUL before the cut: whole
        (b"chr1\t100\tA\t3\t.,.\tI\0I\n", S6),                                        # ... behind it: dropped
        (b"", b""),
    ]
    for impl in variants(sid).values():
        for text, want in cases:
            assert model(text) == want, text
            got, lines = sid.strip_lines(text, impl)
            assert got == want, (impl, text)
            assert lines == text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)
        whole = b"".join(t for t, _ in cases if t.endswith(b"\n"))
        assert sid.strip_lines(whole, impl)[0] == b"".join(w for t, w in cases if t.endswith(b"\n"))


def test_long_line_and_cut_at_a_64_byte_boundary(sid):
    long_line = b"chr2\t7\tC\t150000\t" + b".," * 75_000 + b"\t" + b"I" * 150_000 + b"\n"
    assert len(long_line) > 300_000
    for impl in variants(sid).values():
        got, lines = sid.strip_lines(L6 + long_line + L6, impl)
        assert got == S6 + long_line[:long_line.index(b"\tI")] + b"\n" + S6 and lines == 3
        # the cut (the end of the 5th token) at byte 64 of an aligned buffer, and around it
        for at in range(60, 70):
            head = b"chr1\t100\tA\t3\t"
            line = head + b"." * (at - len(head)) + b"\tIIII\n"
            for pre in (b"", L6):
                for align in (0, 64 - len(pre) % 64 if pre else 0):
                    got, _ = sid.strip_lines(pre + line + L6, impl, align=align)
                    assert got == model(pre) + line[:at] + b"\n" + S6, (impl, at, align)


def test_properties(sid, fuzz_text):
    text = fuzz_text
    got, lines = sid.strip_lines(text)
    assert got == model(text)
    assert len(got) <= len(text) and len(got) < 0.8 * len(text)
    assert lines == text.count(b"\n") == got.count(b"\n")
    for a, b in zip(text.split(b"\n"), got.split(b"\n")):
        assert a.startswith(b)
    assert sid.strip_lines(got)[0] == got   # idempotent
    # split at any line boundaries: the parts' output is the whole's
    rng = np.random.default_rng(7)
    nls = np.flatnonzero(np.frombuffer(text, np.uint8) == 10) + 1
    for _ in range(8):
        cuts = [0] + sorted(int(c) for c in rng.choice(nls, int(rng.integers(1, 12)), replace=False)) + [len(text)]
        assert b"".join(sid.strip_lines(text[a:b])[0] for a, b in zip(cuts, cuts[1:])) == got


def test_map_back(sid, fuzz_text):
    """sid_strip_map: every line start of the stripped text maps to its input
    line's start, and an offset inside a line to the same offset in it."""
    text = fuzz_text[:40_000]
    text = text[:text.rindex(b"\n") + 1]
    got, _ = sid.strip_lines(text)
    i = o = 0
    for a, b in zip(text.split(b"\n")[:-1], got.split(b"\n")[:-1]):
        assert sid.strip_map(text, o) == i
        if len(b) > 1:
            assert sid.strip_map(text, o + len(b) - 1) == i + len(b) - 1
        assert sid.strip_map(text, o + len(b)) == i + len(a)   # the newline
        i += len(a) + 1
        o += len(b) + 1
    assert sid.strip_map(text, len(got)) == len(text)


def test_variants_agree_at_every_alignment(sid, fuzz_text):
    vs = variants(sid)
    assert "scalar" in vs
    if len(vs) == 1:
        pytest.skip("this CPU runs no vector variant")
    want = sid.strip_lines(fuzz_text, vs["scalar"])
    assert sid.strip_impl() == max(vs.values())
    for name, impl in vs.items():
        assert sid.strip_lines(fuzz_text, impl) == want, name
        piece = fuzz_text[:9_000]
        for align in range(64):
            for skip in (0, 1 + align % 7):   # (the text's start at another byte of its first line, too)
                assert sid.strip_lines(piece[skip:], impl, align=align) == sid.strip_lines(piece[skip:], vs["scalar"]), \
                    (name, align, skip)


METHODS = [[], ["-R"], ["-m", "likelihood_ratio"], ["-m", "bayes"]]


def same_runs(sid, oracle, tmp_path, text, what):
    a, b = tmp_path / "raw.plp", tmp_path / "stripped.plp"
    a.write_bytes(text)
    b.write_bytes(sid.strip_lines(text)[0])
    for flags in METHODS:
        ra, rb = oracle.run_cli(flags + [str(a)]), oracle.run_cli(flags + [str(b)])
        assert (ra.returncode, ra.stdout, ra.stderr) == (rb.returncode, rb.stdout, rb.stderr), (what, flags)
    return ra


@pytest.mark.parametrize("name", ["edge.plp", "c1_10k.plp"])
def test_oracle_cli_on_stripped_golden(sid, oracle, tmp_path, name):
    text = open(os.path.join(HERE, "golden", name), "rb").read()
    assert len(sid.strip_lines(text)[0]) < len(text)
    same_runs(sid, oracle, tmp_path, text, name)


def test_oracle_cli_on_stripped_fuzz_lines(sid, oracle, tmp_path):
    """The fuzzed line corpus of tests/golden/ref_pileup_fuzz.tsv.gz (its
    lines from test_parser.fuzz_lines, the reference's verdicts from the
    file): the lines the reference parses, in one text; and every line it
    refuses, each between a few good ones -- the same error, nothing
    written."""
    path = os.path.join(HERE, "golden", "ref_pileup_fuzz.tsv.gz")
    verdicts = [o.split(b"\t")[0] for o in gzip.open(path).read().split(b"\n")[:-1]]
    lines = [l for s in (1, 2, 3) for l in fuzz_lines(s, 1500) if l and not blank(l)]
    assert len(lines) == len(verdicts)
    ok = [l for l, v in zip(lines, verdicts) if v == b"OK" and b"\n" not in l]
    bad = [l for l, v in zip(lines, verdicts) if v != b"OK" and b"\n" not in l]
    assert len(ok) > 1000 and len(bad) > 20
    r = same_runs(sid, oracle, tmp_path, b"".join(l + b"\n" for l in ok), "parsed lines")
    assert r.returncode == 0
    head = b"".join(l + b"\n" for l in ok[:5])
    assert len(bad) > 1500
    for l in bad:
        r = same_runs(sid, oracle, tmp_path, head + l + b"\n" + head, l)
        assert r.returncode != 0 and r.stdout == b""
