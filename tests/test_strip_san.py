"""strip.cpp -- sid_strip_lines in every variant the CPU runs, the engine's
streaming form and sid_strip_map -- compiled with AddressSanitizer +
UndefinedBehaviorSanitizer into a stand-alone program (tests/strip_san: its own
main, nothing preloaded) and run over the cases of tests/test_strip.py: the
hand-made lines, a 300 KB line, cuts around a 64-B boundary, and the seeded
fuzz at every input alignment.  Every input is a heap block that ends with the
text's last byte and every output a block of exactly the input's size, so a
read or write past either is a report.  A report fails the test, and every
output must equal the Python model's.  CPU only."""
import os
import subprocess

import pytest

from sanitized import ENV
from test_strip import L6, fuzz_text, model   # noqa: F401 (fuzz_text: the fixture)

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "strip_san")


@pytest.fixture(scope="module")
def strip_san():
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    return os.path.join(DIR, "_build", "strip_san")


def run_cases(prog, path, cases):
    with open(path, "wb") as f:
        for text, align in cases:
            f.write(b"%d %d\n" % (len(text), align) + text + b"\n")
    r = subprocess.run([prog, str(path)], capture_output=True, env=ENV, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert "AddressSanitizer" not in err and "runtime error" not in err and "LeakSanitizer" not in err, err[-3000:]
    assert r.returncode == 0, (r.returncode, err[-3000:])
    out, at = r.stdout, 0
    for text, align in cases:
        nl = out.index(b"\n", at)
        m, lines = (int(x) for x in out[at:nl].split())
        got = out[nl + 1:nl + 1 + m]
        assert got == model(text), (text[:200], align)
        assert lines == text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)
        at = nl + 1 + m + 1
    assert at == len(out)


def test_hand_made_lines_sanitized(strip_san, tmp_path):
    texts = [b"", b"\n", L6, L6[:-1], L6 + L6[:-1], b" \t chr1 \t100  A\t3 .,.\t \tIII\t]]]\n", b"chr1\t100\tA\t3\n",
             b"chr1\t100\tA\t3\t.,.\n", L6[:-1] + b"\r\n", b"chr1\t100\tA\t3\t.\0.\tIII\n", b"chr1\t100\tA\t3\t.,.\tI\0I\n",
             b"\n\n" + L6 + b"\n", b"\t", b" ", b"a", b"a b c d e", b"a b c d e\n", b"a b c d e f\n"]
    long_line = b"chr2\t7\tC\t150000\t" + b".," * 75_000 + b"\t" + b"I" * 150_000 + b"\n"
    texts += [L6 + long_line + L6, long_line[:-1], long_line[:200_000]]
    head = b"chr1\t100\tA\t3\t"
    texts += [pre + head + b"." * (at - len(head)) + b"\tIIII\n" + L6 for at in range(60, 70) for pre in (b"", L6)]
    run_cases(strip_san, tmp_path / "hand.cases", [(t, a) for t in texts for a in (0, 1, 63)])


def test_fuzz_sanitized_at_every_alignment(strip_san, tmp_path, fuzz_text):
    piece = fuzz_text[:9_000]
    cases = [(fuzz_text, 0), (fuzz_text[3:], 5)]
    cases += [(piece[skip:len(piece) - drop], align) for align in range(64) for skip, drop in ((0, 0), (1 + align % 7, align % 5))]
    run_cases(strip_san, tmp_path / "fuzz.cases", cases)
