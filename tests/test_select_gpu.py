"""--only het|hom (sid_opts.select) on the device: through build/sid and through
sid_amd.Engine, every formatter (the tile parse and its writers, the sparse
writers, the Lynch pass 2, the generic kernels, --host-parse).

The expected stdout is always the oracle CLI's unselected stdout for the same
flags and input, filtered in Python by the label field -- the fifth
comma-separated field from the right, line.rsplit(",", 5)[1] -- and the
expected stderr and exit status are the oracle's own.  Every case asserts that
its expected output holds at least one selected and one unselected record
(a filter that passes everything or nothing cannot pass), but for the two
header-only cases, which assert exactly that."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
SELECTS = ["het", "hom"]
BASES = b"." * 15 + b"G" * 15   # on reference A: a het site at 30x
HOMS = b"." * 30


def run(exe, args, **kw):
    return subprocess.run([exe] + list(args), capture_output=True, timeout=600, **kw)


def select_lines(csv: bytes, select: str):
    """(header + the records whose label field is `select`, selected, unselected)."""
    lines = csv.splitlines(keepends=True)
    if not lines:
        return b"", 0, 0
    keep = [ln for ln in lines[1:] if select == "all" or ln.rsplit(b",", 5)[1] == select.encode()]
    return lines[0] + b"".join(keep), len(keep), len(lines) - 1 - len(keep)


def line(chrom: bytes, pos, het: bool, bases: bytes = None) -> bytes:
    b = bases if bases is not None else (BASES if het else HOMS)
    pos = pos if isinstance(pos, bytes) else b"%d" % pos
    return b"%s\t%s\tA\t%d\t%s\t%s\n" % (chrom, pos, len(b), b, b"I" * len(b))


def placement_text(kind: str, n: int = 6000) -> bytes:
    """n lines at 30x where the test decides which sites are het."""
    het = {
        "none": lambda i: False,
        "every": lambda i: True,
        "second": lambda i: i % 2 == 0,
        "61st": lambda i: i % 61 == 0,
        "runs70": lambda i: (i // 70) % 9 == 3,
        "last100": lambda i: i > n - 100,
    }[kind]
    return b"".join(line(b"chr1", i, het(i)) for i in range(1, n + 1))


def special_text(sid) -> bytes:
    """Lines of every kind the formatters tell apart, hets among them."""
    rng = np.random.default_rng(64)

    def fixups(chrom, n, depth, indel_every):   # four alleles in numbers: no class table covers them
        out = []
        for i in range(1, n + 1):
            k = rng.integers(0, 4, 4) * (depth // 8) + rng.integers(0, 3, 4)
            bases = bytearray(b"A" * int(k[0]) + b"c" * int(k[1]) + b"G" * int(k[2]) + b"t" * int(k[3]) +
                              b"." * int(rng.integers(0, depth // 2)))
            rng.shuffle(bases)
            if indel_every and i % indel_every == 0:
                bases[len(bases) // 2:len(bases) // 2] = b"+2AC"   # the general routine
            out.append(line(chrom, i, False, bytes(bases) or b"*"))
        return b"".join(out)

    parts = [
        # a chromosome name with the other label in it: its sites are hom
        b"".join(line(b"a,het,b", i, False) for i in range(1, 601)),
        b"".join(line(b"a,hom,b", i, True) for i in range(1, 41)),
        fixups(b"chr1", 500, 40, 5),
        # names longer than the header pair's 8 bytes, and of 70 bytes (a
        # 512-site group's records pass the writers' LDS buffer)
        b"".join(line(b"chromosome12", i, i % 3 == 0) for i in range(1, 301)),
        b"".join(line(b"N" * 70, i, i % 2 == 0) for i in range(1, 701)),
        # zero-padded positions: the formatter's tokeniser
        b"".join(line(b"chrZ", b"%04d" % i, i % 4 == 0) for i in range(1, 61)),
        # depth 0
        b"".join(b"chr2\t%d\tA\t0\t*\t*\n" % i for i in range(1, 301)),
        # coverage < 4 between hets (LR / bayes print no record for them)
        b"".join(line(b"chr6", i, True) if i % 2 else line(b"chr6", i, False, b".,") for i in range(1, 201)),
        # '+2AC' indels on otherwise plain het and hom lines
        b"".join(line(b"chr7", i, False, (BASES if i % 5 == 0 else HOMS) + b"+2AC") for i in range(1, 201)),
        sid.synth_text(65, 3000, 30.0, sites_per_chrom=10 ** 6),
        fixups(b"chr3", 200, 40, 0),
    ]
    return b"".join(parts)


class Inputs:
    """The test inputs as files, and the oracle's run of each (flags, input), computed once."""

    def __init__(self, sid, oracle, d):
        self.oracle = oracle
        self.paths = {"c1": os.path.join(GOLD, "c1_10k.plp"), "edge": os.path.join(GOLD, "edge.plp")}
        texts = {
            # 200x: the quad shape (the generator's hets are too few at this size: some by hand)
            "deep": (sid.synth_text(5, 1500, 200.0, sites_per_chrom=1000) +
                     b"".join(line(b"chrD", i, False, b"." * 100 + b"g" * 100 if i % 7 == 0 else b"." * 200)
                              for i in range(1, 701)) +
                     sid.synth_text(6, 800, 200.0, sites_per_chrom=1000)),
            "quality": sid.synth_text(4, 5000, 30.0, sites_per_chrom=2000, mapq=True),
            "special": special_text(sid),
            "synth": sid.synth_text(71, 12_000, 30.0, sites_per_chrom=5000),
            "synth2": sid.synth_text(72, 9_000, 30.0, sites_per_chrom=4000),
        }
        for k in ("none", "every", "second", "61st", "runs70", "last100"):
            texts[k] = placement_text(k)
        good = placement_text("61st", 4000)
        texts["bad_late"] = good + good + b"chr1\t1\tAC\t3\t...\tIII\n" + placement_text("second", 50)
        self.texts = texts
        for k, t in texts.items():
            p = d / f"{k}.plp"
            p.write_bytes(t)
            self.paths[k] = str(p)
        self._ref = {}

    def text(self, name):
        if name not in self.texts:
            with open(self.paths[name], "rb") as f:
                self.texts[name] = f.read()
        return self.texts[name]

    def ref(self, flags, name):
        key = (tuple(flags), name)
        if key not in self._ref:
            self._ref[key] = self.oracle.run_cli(list(flags) + [self.paths[name]])
        return self._ref[key]


@pytest.fixture(scope="module")
def inputs(sid, oracle, tmp_path_factory):
    return Inputs(sid, oracle, tmp_path_factory.mktemp("select"))


def expect(inputs, flags, name, select, header_only=False):
    """The oracle's run and its stdout filtered; asserts the case is not vacuous."""
    b = inputs.ref(flags, name)
    assert b.returncode == 0, b.stderr[-300:]
    want, nsel, nother = select_lines(b.stdout, select)
    if header_only:
        assert nsel == 0 and nother > 0 and want == b.stdout.splitlines(keepends=True)[0]
    else:
        assert nsel >= 1 and nother >= 1, (flags, name, select, nsel, nother)
    return b, want


def check_cli(sid, inputs, flags, name, select, extra=(), header_only=False):
    b, want = expect(inputs, flags, name, select, header_only)
    a = run(sid.CLI_PATH, list(extra) + ["--only", select] + list(flags) + [inputs.paths[name]])
    assert a.returncode == 0, (a.returncode, a.stderr[-400:])
    assert a.stdout == want, (flags, name, select, extra)
    assert a.stderr == b.stderr


FLAGS = [[], ["-R", "-m", "likelihood_ratio"], ["-m", "bayes"], ["-R", "-m", "local"],
         ["-E", "0.05", "-p", "0.01", "-r", "0.001"],
         ["-E", "-0.5"]]   # (a negative base: no class tables, the call kernel and the generic formatter)


@pytest.mark.parametrize("select", SELECTS)
@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: " ".join(f) or "default")
def test_cli_flag_sets(sid, inputs, flags, select):
    for name in ("c1", "edge", "special"):
        check_cli(sid, inputs, flags, name, select)
    check_cli(sid, inputs, flags, "deep", select, extra=["--chunk-bytes", "300000"])


@pytest.mark.parametrize("select", SELECTS)
@pytest.mark.parametrize("flags", [["-m", "quality"], ["-R", "-m", "quality"]], ids=lambda f: " ".join(f))
def test_cli_quality(sid, inputs, flags, select):
    """-m quality (text with a mapping-quality column): the generic formatter kernels."""
    check_cli(sid, inputs, flags, "quality", select)
    check_cli(sid, inputs, flags, "quality", select, extra=["--chunk-bytes", "65536"])


SHAPES = {
    "chunk-4096": ["--chunk-bytes", "4096"],                 # smaller than a tile
    "chunk-65536": ["--chunk-bytes", "65536"],
    "devices-2": ["--chunk-bytes", "200000", "--devices", "2"],
    "pass-2-kept": ["--chunk-bytes", "200000", "--hold-bytes", "1"],
    "pass-2-reloaded": ["--chunk-bytes", "200000", "--hold-bytes", "1", "--retain-bytes", "1"],
    "host-hold-small": ["--chunk-bytes", "65536", "--host-hold", "3000"],
    "host-hold": ["--chunk-bytes", "65536", "--host-hold", "4000000"],
    "host-parse": ["--host-parse"],
    "host-parse-2": ["--host-parse", "--devices", "2"],
}


@pytest.mark.parametrize("select", SELECTS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_cli_engine_shapes(sid, inputs, shape, select):
    """(the default shape: test_cli_flag_sets)"""
    for flags in ([], ["-R", "-m", "likelihood_ratio"]):
        check_cli(sid, inputs, flags, "special", select, extra=SHAPES[shape])


@pytest.mark.parametrize("select", SELECTS)
@pytest.mark.parametrize("kind", ["second", "61st", "runs70", "last100"])
def test_cli_het_placements(sid, inputs, kind, select):
    """Chunks and 512-slot groups without a selected record, and with only selected ones."""
    for flags, extra in (([], ["--chunk-bytes", "65536"]), ([], []), (["-m", "bayes"], ["--chunk-bytes", "65536"]),
                         (["-R", "-m", "local"], ["--chunk-bytes", "100000", "--hold-bytes", "1"])):
        check_cli(sid, inputs, flags, kind, select, extra=extra)


def engine_run(sid, text, method="local", **kw):
    eng = sid.Engine(method=method, **kw)
    eng.source_text(text)
    out, st = eng.run()
    eng.close()
    return out, st


@pytest.mark.parametrize("name,select", [("none", "het"), ("every", "hom")])
def test_nothing_selected_gives_the_header_only(sid, inputs, name, select):
    for extra in ([], ["--chunk-bytes", "65536"], ["--chunk-bytes", "65536", "--hold-bytes", "1"],
                  ["--chunk-bytes", "65536", "--host-hold", "100000"], ["--host-parse"]):
        check_cli(sid, inputs, [], name, select, extra=extra, header_only=True)
    for kw in ({}, {"chunk_bytes": 65536}, {"chunk_bytes": 65536, "hold_bytes": 1},
               {"chunk_bytes": 65536, "host_hold_bytes": 1 << 20}):
        out, st = engine_run(sid, inputs.text(name), select=select, **kw)
        assert out == sid.HEADER and st.bytes_out == 0 and st.sites == 6000, kw
    # the PCIe path without a writer: every chunk's records, none, in the host arena
    eng = sid.Engine(select=select, device_sink=2, chunk_bytes=65536, host_hold_bytes=1 << 20)
    eng.source_text(inputs.text(name))
    st = eng.ingest()
    eng.estimate()
    _, st2 = eng.emit()
    assert st.chunks >= 4 and st2.bytes_out == 0
    assert eng.records_bytes(st.chunks) == b""
    eng.close()


@pytest.mark.parametrize("select", SELECTS)
@pytest.mark.parametrize("method", ["local", "likelihood_ratio"])
def test_engine_host_arena_records(sid, inputs, method, select):
    """Engine(device_sink=2) + records_bytes: the selected records in the pinned host arena."""
    flags = [] if method == "local" else ["-R", "-m", method]
    for name in ("special", "61st"):
        b, want = expect(inputs, flags, name, select)
        text = inputs.text(name)
        eng = sid.Engine(method=method, estimate_prior=method != "local", select=select, device_sink=2,
                         chunk_bytes=100_000, host_hold_bytes=len(text))
        eng.source_text(text)
        st = eng.ingest()
        eng.estimate()
        _, st2 = eng.emit()
        got = eng.records_bytes(st.chunks)
        assert st.chunks >= 4 and st2.bytes_out == len(got)
        assert sid.HEADER + got == want
        eng.close()


def test_engine_reuse_and_contexts_do_not_share_tables(sid, inputs):
    """One Engine(select="het") run twice on different texts; a second engine
    with select="all" afterwards gives the whole output."""
    for method, flags in (("local", []), ("likelihood_ratio", ["-R", "-m", "likelihood_ratio"])):
        kw = dict(method=method, estimate_prior=method != "local", chunk_bytes=200_000)
        eng = sid.Engine(select="het", **kw)
        for name in ("synth", "synth2", "synth"):
            b, want = expect(inputs, flags, name, "het")
            eng.source_text(inputs.text(name))
            out, st = eng.run()
            assert out == want, (method, name)
            assert st.bytes_out == len(want) - len(sid.HEADER)
            if method == "local":   # the tile parse and the sparse writer took the chunks
                assert st.chunks >= 3 and st.chunks_tiled == st.chunks
        full = sid.Engine(select="all", **kw)
        full.source_text(inputs.text("synth"))
        assert full.run()[0] == inputs.ref(flags, "synth").stdout
        hom = sid.Engine(select=2, **kw)   # the integer
        hom.source_text(inputs.text("synth"))
        assert hom.run()[0] == expect(inputs, flags, "synth", "hom")[1]
        # ... and the first engine still selects
        eng.source_text(inputs.text("synth2"))
        assert eng.run()[0] == expect(inputs, flags, "synth2", "het")[1]
        for e in (eng, full, hom):
            e.close()


def test_dtext_format_honours_the_context(sid, gpu, oracle, inputs):
    """sid_dtext_format of a context with a selection (the generic length / write kernels)."""
    import torch
    text = inputs.text("synth")
    ref = inputs.ref([], "synth")
    for select in ("all", "het", "hom"):
        ctx = sid.Context(0, method="local", select=select)
        t = sid.DText(ctx, text)
        n = len(t)
        _, dcode, dhom, dhet = gpu.device_buffers(n)
        ctx.call_local(t.counts_ptr, n, dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr())
        torch.cuda.synchronize()
        want, nsel, nother = select_lines(ref.stdout, select)
        assert nsel >= 1 and (select == "all" or nother >= 1)
        assert sid.HEADER + t.format(dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr(), "p_value") == want
        t.close()
        ctx.close()


def test_malformed_line_in_the_last_chunk(sid, inputs):
    b = inputs.ref([], "bad_late")
    assert b.returncode != 0 and b.stdout == b""
    for extra in ([], ["--chunk-bytes", "65536"], ["--chunk-bytes", "65536", "--hold-bytes", "1"], ["--host-parse"]):
        a = run(sid.CLI_PATH, extra + ["--only", "het", inputs.paths["bad_late"]])
        assert a.returncode == b.returncode, (extra, a.returncode, b.returncode)
        assert a.stdout == b""
        assert a.stderr == b.stderr


def test_only_rejects_other_values(sid, inputs):
    for args in (["--only", "bogus", inputs.paths["c1"]], ["--only", "HET", inputs.paths["c1"]],
                 ["-m", "bayes", "--only", "", inputs.paths["c1"]], ["--host-parse", "--only=x", inputs.paths["c1"]]):
        a = run(sid.CLI_PATH, args)
        assert a.returncode == 1
        assert a.stdout == b""
        assert a.stderr == b"sid: --only: expected het, hom or all\n"
    with pytest.raises(sid.SidError) as ei:
        sid.Engine(select=3)
    assert ei.value.status == 1   # SID_EINVAL
    with pytest.raises(sid.SidError) as ei:
        sid.Context(0, select=-1)
    assert ei.value.status == 1


def test_only_all_equals_no_option(sid, inputs):
    for flags in ([], ["-R", "-m", "likelihood_ratio"]):
        b = inputs.ref(flags, "special")
        for extra in ([], ["--host-parse"]):
            a = run(sid.CLI_PATH, extra + ["--only", "all"] + flags + [inputs.paths["special"]])
            assert a.returncode == b.returncode == 0
            assert a.stdout == b.stdout and a.stderr == b.stderr


def test_help_text_is_the_reference_s(sid, oracle):
    a, b = run(sid.CLI_PATH, ["-h"]), oracle.run_cli(["-h"])
    assert a.stdout == b.stdout and b"--only" not in a.stdout
