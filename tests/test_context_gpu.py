"""--context N (sid_opts.context) on the device: through build/sid and through
sid_amd.Engine, every formatter family, the chunk edges and every record path
of the engine.

The expected stdout is always the oracle CLI's unselected stdout for the same
flags and input, filtered in Python (tests/context_ref.py, not the library):
the label by line.rsplit(b",", 5)[1], the region by tests/regions_ref.py, then
the dilation over record indices.  stderr and the exit status are the
oracle's own.  Every case asserts that its expected output holds at least one
context record (kept, not selected) and drops at least one record -- but for
the keep-everything and header-only cases, which assert exactly that."""
import pytest

import bgzf_ref
from context_ref import filter_csv
from regions_ref import RefSet, bed_points, text_sites
from test_regions_gpu import ENGINE_KW, dense_text
from test_select_gpu import FLAGS, SHAPES, Inputs, line, placement_text, run

pytestmark = pytest.mark.gpu


def phase_text(n=6000) -> bytes:
    """Lines of one byte length, a het every 51st: with 50 lines a chunk the hets meet every offset from a cut."""
    t = b"".join(line(b"chr1", 100000 + i, i % 51 == 0) for i in range(n))
    assert len({len(x) for x in t.splitlines()}) == 1
    return t


class CInputs(Inputs):
    def __init__(self, sid, oracle, d):
        super().__init__(sid, oracle, d)
        self.dir = d
        for k, t in {"dense": dense_text(), "phase": phase_text()}.items():
            self.texts[k] = t
            p = d / f"{k}.plp"
            p.write_bytes(t)
            self.paths[k] = str(p)
        self._beds = {}

    def bed(self, key, text: bytes):
        if key not in self._beds:
            p = self.dir / f"{key}.bed"
            p.write_bytes(text)
            self._beds[key] = (str(p), RefSet(text), text)
        return self._beds[key]


@pytest.fixture(scope="module")
def inputs(sid, oracle, tmp_path_factory):
    return CInputs(sid, oracle, tmp_path_factory.mktemp("context"))


def expect(inputs, flags, name, n, select="het", ref=None, mode="some"):
    b = inputs.ref(flags, name)
    assert b.returncode == 0, b.stderr[-300:]
    want, nsel, nctx, ndrop = filter_csv(b.stdout, n, select, ref)
    if mode == "header":
        assert nsel == 0 and ndrop > 0 and want == b.stdout.splitlines(keepends=True)[0]
    elif mode == "all":
        assert ndrop == 0 and nctx > 0 and want == b.stdout
    elif mode == "few":
        assert nsel >= 1 and nctx >= 1
    elif mode == "tiled":   # every window touches the next: all but the records in front of the first window
        lines = b.stdout.splitlines(keepends=True)
        assert ndrop == 60 - n and want == lines[0] + b"".join(lines[1 + ndrop:])
    else:
        assert nsel >= 1 and nctx >= 1 and ndrop >= 1, (flags, name, n, select, nsel, nctx, ndrop)
    return b, want


def check_cli(sid, inputs, flags, name, n, extra=(), select="het", bed=None, mode="some"):
    b, want = expect(inputs, flags, name, n, select, bed[1] if bed else None, mode)
    sel = ([] if select == "all" else ["--only", select]) + (["--regions", bed[0]] if bed else [])
    a = run(sid.CLI_PATH, list(extra) + ["--context", str(n)] + sel + list(flags) + [inputs.paths[name]])
    assert a.returncode == 0, (a.returncode, a.stderr[-400:])
    assert a.stdout == want, (flags, name, n, select, extra)
    assert a.stderr == b.stderr
    return a


def check_engine(sid, inputs, flags, name, n, select="het", bed=None, mode="some", **kw):
    b, want = expect(inputs, flags, name, n, select, bed[1] if bed else None, mode)
    rg = sid.Regions(bed[2]) if bed else None
    eng = sid.Engine(regions=rg, select=select, context=n, **ENGINE_KW[tuple(flags)], **kw)
    if rg:
        rg.close()
    eng.source_text(inputs.text(name))
    out, st = eng.run()
    eng.close()
    assert out == want, (flags, name, n, select, kw)
    assert st.bytes_out == len(want) - len(sid.HEADER)
    return st


PLACE_FLAGS = [[], ["-R", "-m", "likelihood_ratio"], ["-m", "bayes"]]
CHUNKS = {"one": [], "4096": ["--chunk-bytes", "4096"]}


@pytest.mark.parametrize("chunks", sorted(CHUNKS))
@pytest.mark.parametrize("flags", PLACE_FLAGS, ids=lambda f: " ".join(f) or "local")
def test_placements(sid, inputs, flags, chunks):
    extra = CHUNKS[chunks]
    for n in (1, 2, 29):   # (29: exactly one record in 61 goes)
        check_cli(sid, inputs, flags, "61st", n, extra=extra)
    # 30: the windows tile the file from the first het on (record 60; the 30 records in front of its window
    # are the only ones that go); 60: they reach the file's first record too, and the output is the oracle's
    check_cli(sid, inputs, flags, "61st", 30, extra=extra, mode="tiled")
    check_cli(sid, inputs, flags, "61st", 60, extra=extra, mode="all")
    for name in ("runs70", "last100"):
        check_cli(sid, inputs, flags, name, 2, extra=extra)
    check_cli(sid, inputs, flags, "second", 2, extra=extra, mode="all")   # (a het every second record: nothing goes)
    check_cli(sid, inputs, flags, "none", 2, extra=extra, mode="header")
    kw = {"chunk_bytes": 4096} if extra else {}
    check_engine(sid, inputs, flags, "61st", 2, **kw)
    check_engine(sid, inputs, flags, "runs70", 2, **kw)


@pytest.mark.parametrize("flags", PLACE_FLAGS, ids=lambda f: " ".join(f) or "local")
def test_context_wider_than_a_chunk(sid, inputs, flags):
    """N = 64 at ~50 records a chunk: the context crosses whole chunks."""
    check_cli(sid, inputs, flags, "61st", 64, extra=["--chunk-bytes", "4096"], mode="all")
    check_cli(sid, inputs, flags, "runs70", 64, extra=["--chunk-bytes", "4096"])
    check_engine(sid, inputs, flags, "last100", 64, chunk_bytes=4096)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_every_phase_of_a_chunk_cut(sid, gpu, inputs, n):
    import torch
    L = len(inputs.text("phase").splitlines(keepends=True)[0])
    for devices in ([1, 2] if torch.cuda.device_count() >= 2 else [1]):
        for flags in ([], ["-m", "bayes"]):
            check_cli(sid, inputs, flags, "phase", n, extra=["--chunk-bytes", str(50 * L), "--devices", str(devices)])
        # (the engine's stats: the chunks that ran)
        st = check_engine(sid, inputs, [], "phase", n, chunk_bytes=50 * L, devices=devices)
        assert st.chunks >= 100
        st = check_engine(sid, inputs, ["-R", "-m", "likelihood_ratio"], "phase", n, chunk_bytes=50 * L, devices=devices)
        assert st.chunks >= 100


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: " ".join(f) or "default")
def test_rank_not_slot(sid, inputs, flags):
    """Sites without a record between hets, depth 0, fix-up sites, general-routine lines, long chroms."""
    for name in ("special", "c1"):
        check_cli(sid, inputs, flags, name, 2)
    # (`edge` has ten records under the Lynch methods, all within two of a het: nothing to drop there)
    check_cli(sid, inputs, flags, "edge", 2, mode="few")
    check_cli(sid, inputs, flags, "deep", 2, extra=["--chunk-bytes", "300000"])
    if tuple(flags) in ENGINE_KW:
        check_engine(sid, inputs, flags, "special", 2, chunk_bytes=200_000)


MORE = {"hold-1": ["--hold-bytes", "1"], "host-hold-100000": ["--host-hold", "100000"]}


@pytest.mark.parametrize("shape", sorted(SHAPES) + sorted(MORE))
def test_shapes_and_budgets(sid, inputs, shape):
    extra = SHAPES.get(shape) or MORE[shape]
    for flags in ([], ["-R", "-m", "likelihood_ratio"]):
        check_cli(sid, inputs, flags, "special", 2, extra=extra)


def test_pass_two_of_local_with_a_prior(sid, inputs):
    check_cli(sid, inputs, ["-R", "-m", "local"], "special", 2, extra=["--chunk-bytes", "100000", "--hold-bytes", "1"])
    check_cli(sid, inputs, ["-R", "-m", "local"], "61st", 2, extra=["--chunk-bytes", "100000", "--hold-bytes", "1"])


def edge_bed(inputs):
    s = text_sites(inputs.text("dense"))
    marks = sorted(set([40, 64, 128, 253, 254, 255, 256, 507, 512, 1024, 5999] + list(range(49, 6000, 101))))
    return inputs.bed("dense.edges", bed_points(s, lambda i: i in marks) + b"chr1\t3000\t3009\n")


@pytest.mark.parametrize("extra", [[], ["--chunk-bytes", "4096"], ["--chunk-bytes", "65536"]], ids=lambda e: "-".join(e) or "one")
def test_with_regions(sid, inputs, extra):
    """--regions alone: the context is by record, not by position; and with --only het as well."""
    bed = edge_bed(inputs)
    for flags in ([], ["-R", "-m", "likelihood_ratio"], ["-E", "-0.5"]):
        check_cli(sid, inputs, flags, "dense", 2, extra=extra, select="all", bed=bed)
    kw = {"chunk_bytes": int(extra[1])} if extra else {}
    check_engine(sid, inputs, [], "dense", 2, select="all", bed=bed, **kw)
    # both selections: the hets of `dense` (every 97th site) inside a set of runs
    s = text_sites(inputs.text("dense"))
    both = inputs.bed("dense.halves", b"".join(b"chr1\t%d\t%d\n" % (a, a + 700) for a in range(0, 6000, 1400)))
    for flags in ([], ["-m", "bayes"]):
        check_cli(sid, inputs, flags, "dense", 2, extra=extra, select="het", bed=both)
    check_engine(sid, inputs, [], "dense", 2, select="het", bed=both, **kw)
    check_cli(sid, inputs, [], "dense", 2, extra=["--host-parse"], select="het", bed=both)
    assert len(s) == 6000


@pytest.mark.parametrize("flags", [["-m", "quality"], ["-R", "-m", "quality"]], ids=lambda f: " ".join(f))
def test_quality(sid, inputs, flags):
    check_cli(sid, inputs, flags, "quality", 2)
    check_cli(sid, inputs, flags, "quality", 2, extra=["--chunk-bytes", "65536"])


def test_bgzf_input(sid, inputs):
    p = inputs.dir / "special.plp.gz"
    p.write_bytes(bgzf_ref.write(inputs.text("special"), payload=20000)[0])
    for flags, extra in (([], []), ([], ["--chunk-bytes", "65536"]), (["-m", "bayes"], ["--chunk-bytes", "65536"])):
        b, want = expect(inputs, flags, "special", 2)
        a = run(sid.CLI_PATH, ["--bgzf", "--context", "2", "--only", "het"] + extra + flags + [str(p)])
        assert (a.returncode, a.stdout, a.stderr) == (0, want, b.stderr), (flags, extra)


def test_dtext_format_honours_the_context(sid, gpu, inputs):
    import torch
    text = inputs.text("synth")
    ref = inputs.ref([], "synth")
    ctx = sid.Context(0, method="local", select="het", context=2)
    t = sid.DText(ctx, text)
    n = len(t)
    _, dcode, dhom, dhet = gpu.device_buffers(n)
    ctx.call_local(t.counts_ptr, n, dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr())
    torch.cuda.synchronize()
    before = dcode[:n].cpu().numpy().copy()
    want, nsel, nctx, ndrop = filter_csv(ref.stdout, 2, "het")
    assert nsel >= 1 and nctx >= 1 and ndrop >= 1
    assert sid.HEADER + t.format(dcode.data_ptr(), dhom.data_ptr(), dhet.data_ptr(), "p_value") == want
    assert (dcode[:n].cpu().numpy() == before).all()
    t.close()
    ctx.close()


@pytest.mark.parametrize("method", ["local", "likelihood_ratio"])
def test_engine_sinks_and_records(sid, inputs, method):
    flags = [] if method == "local" else ["-R", "-m", method]
    kw = dict(method=method, estimate_prior=method != "local", select="het", context=2)
    for name in ("special", "61st"):
        _, want = expect(inputs, flags, name, 2)
        text = inputs.text(name)
        for sink in (1, 2):
            for more in ({}, {"hold_bytes": 1}):
                eng = sid.Engine(device_sink=sink, chunk_bytes=20_000, **kw, **more)
                eng.source_text(text)
                _, st = eng.run()
                assert st.chunks >= 10 and st.bytes_out == len(want) - len(sid.HEADER), (name, sink, more)
                eng.close()
        eng = sid.Engine(device_sink=2, chunk_bytes=20_000, host_hold_bytes=len(text), **kw)
        eng.source_text(text)
        st = eng.ingest()
        eng.estimate()
        _, st2 = eng.emit()
        got = eng.records_bytes(st.chunks)
        assert st2.bytes_out == len(got) and sid.HEADER + got == want
        eng.close()


def test_engine_reuse_and_context_zero(sid, inputs):
    for method, flags in (("local", []), ("likelihood_ratio", ["-R", "-m", "likelihood_ratio"])):
        kw = dict(method=method, estimate_prior=method != "local", chunk_bytes=100_000)
        eng = sid.Engine(select="het", context=2, **kw)
        for name in ("synth", "special", "synth2"):
            _, want = expect(inputs, flags, name, 2)
            eng.source_text(inputs.text(name))
            out, st = eng.run()
            assert out == want and st.bytes_out == len(want) - len(sid.HEADER), (method, name)
        eng.close()
        zero = sid.Engine(select="het", context=0, **kw)   # today's selected output
        zero.source_text(inputs.text("synth"))
        assert zero.run()[0] == filter_csv(inputs.ref(flags, "synth").stdout, 0, "het")[0]
        zero.close()
        plain = sid.Engine(context=5, **kw)   # no selection: the whole output
        plain.source_text(inputs.text("synth"))
        assert plain.run()[0] == inputs.ref(flags, "synth").stdout
        plain.close()


def test_rejects(sid, inputs):
    for v in (65, -1):
        with pytest.raises(sid.SidError) as ei:
            sid.Engine(select="het", context=v)
        assert ei.value.status == 1
        with pytest.raises(sid.SidError) as ei:
            sid.Context(0, context=v)
        assert ei.value.status == 1
    for arg in ("65", "-1", "x", "", "2x", "1e1", " 2"):
        for extra in ([], ["--host-parse"], ["-m", "bayes"]):
            a = run(sid.CLI_PATH, extra + ["--only", "het", "--context", arg, inputs.paths["c1"]])
            assert (a.returncode, a.stdout) == (1, b"")
            assert a.stderr == b"sid: --context: expected 0..64, got %s\n" % arg.encode()
    # given twice: the last wins; and 0 is today's output
    _, want = expect(inputs, [], "61st", 2)
    a = run(sid.CLI_PATH, ["--context", "9", "--only", "het", "--context", "2", inputs.paths["61st"]])
    assert a.returncode == 0 and a.stdout == want
    a = run(sid.CLI_PATH, ["--context", "0", "--only", "het", inputs.paths["61st"]])
    assert a.stdout == filter_csv(inputs.ref([], "61st").stdout, 0, "het")[0]


def test_malformed_line_in_the_last_chunk(sid, inputs):
    b = inputs.ref([], "bad_late")
    assert b.returncode != 0 and b.stdout == b""
    for extra in ([], ["--chunk-bytes", "65536"], ["--chunk-bytes", "65536", "--hold-bytes", "1"], ["--host-parse"]):
        a = run(sid.CLI_PATH, extra + ["--only", "het", "--context", "2", inputs.paths["bad_late"]])
        assert a.returncode == b.returncode, (extra, a.returncode, b.returncode)
        assert a.stdout == b""
        assert a.stderr == b.stderr


def test_help_text_is_the_reference_s(sid, oracle):
    a, b = run(sid.CLI_PATH, ["-h"]), oracle.run_cli(["-h"])
    assert a.stdout == b.stdout and b"--context" not in a.stdout
