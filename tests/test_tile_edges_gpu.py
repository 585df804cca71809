"""The tile parse (sid_tile_parse_kernel, textpath.hip) at its tile, halo,
chunk-end and counter edges: the texts of tests/test_tile_edges.py (whose
geometry the CPU tests there prove) through sid_amd.Engine, against the oracle
CLI's stdout on the same bytes, byte for byte; --only het against that stdout
filtered as test_select_gpu.select_lines does.

The shape is controlled by construction, as run_stats does not report it: a
fresh engine parses its first chunk with the lane shape (20 KiB tiles); an
engine that has just run a 200x text parses the next chunk with the quad shape
(24 KiB tiles) and keeps it while the lines average over 256 B.  Every
geometry case is one chunk, so tile k starts at text byte k * T.  An intended
case asserts chunks == 1, chunks_tiled == chunks and tile_overflows == 0 (the
quad shape on the second of two passes: the first may raise the slot cap);
each text also runs on the other engine state with its output checked only."""
import numpy as np
import pytest

import test_tile_edges as E
from test_parse_stress_gpu import first_diff
from test_select_gpu import select_lines

pytestmark = pytest.mark.gpu

CHUNK = 8 << 20   # over every geometry text
FLAGSETS = {
    "local": ([], dict(method="local")),
    # the counts instantiation, sid_tile_compact_kernel
    "lynch": (["-R", "-m", "likelihood_ratio"], dict(method="likelihood_ratio", estimate_prior=True)),
    "het": ([], dict(method="local", select="het")),                         # the SEL instantiation
    "twopass": (["-E", "-0.5"], dict(method="local", site_error_threshold=-0.5)),   # no class tables: index + parse
}


class Refs:
    """The oracle CLI's run of a (text, flags), one process each, kept."""

    def __init__(self, oracle, d):
        self.oracle, self.d, self.kept, self.runs = oracle, d, {}, 0

    def want(self, key, text, flagset):
        flags = FLAGSETS[flagset][0]
        k = (key, tuple(flags))
        if k not in self.kept:
            p = self.d / "edge.plp"
            p.write_bytes(text)
            r = self.oracle.run_cli(flags + [str(p)])
            self.runs += 1
            assert r.returncode == 0, (key, r.returncode, r.stderr[-300:])
            self.kept[k] = r.stdout
        out = self.kept[k]
        if flagset == "het":
            out, nsel, nother = select_lines(out, "het")
            assert nsel >= 1 and nother >= 1, (key, nsel, nother)
        return out


@pytest.fixture(scope="module")
def refs(oracle, tmp_path_factory):
    return Refs(oracle, tmp_path_factory.mktemp("tile_edges"))


@pytest.fixture(scope="module")
def prime(sid):
    """The 200x text after which an engine parses with the quad shape."""
    return sid.synth_text(5, 1500, 200.0, sites_per_chrom=1000)


def engine(sid, flagset, prime_text=None, **kw):
    """A fresh engine (lane shape next), or one that has run the 200x text
    (quad shape next)."""
    eng = sid.Engine(chunk_bytes=kw.pop("chunk_bytes", CHUNK), **FLAGSETS[flagset][1], **kw)
    if prime_text is not None:
        eng.source_text(prime_text)
        _, st = eng.run()
        assert st.chunks == 1 and st.chunks_tiled == (flagset != "twopass")
    return eng


def run_text(eng, text, want, what, intended=False):
    eng.source_text(text)
    out, st = eng.run()
    same = out == want
    assert same, (what, first_diff(out, want))
    if intended:
        assert (st.chunks, st.chunks_tiled, st.tile_overflows) == (1, 1, 0), what
    return st


def run_intended(eng, shape, text, want, what):
    """Lane: the engine's first chunk.  Quad: twice, the stats of the second pass."""
    if shape == "quad":
        run_text(eng, text, want, what)
    run_text(eng, text, want, what, intended=True)


def both_states(sid, prime, shape, flagset, text, want, what):
    """The text on the engine state it was built for, stats asserted, and on
    the other one."""
    for state in E.SHAPES:
        eng = engine(sid, flagset, prime if state == "quad" else None)
        try:
            if state == shape:
                run_intended(eng, shape, text, want, (what, state))
            else:
                run_text(eng, text, want, (what, state))
        finally:
            eng.close()


GEOMETRY = [g[0] for g in E.GEOMETRY]


@pytest.mark.parametrize("flagset", ["local", "lynch", "het"])
@pytest.mark.parametrize("name", GEOMETRY)
@pytest.mark.parametrize("shape", E.SHAPES)
def test_geometry(sid, refs, prime, shape, name, flagset):
    """Families A (line starts across the tile edge), B (lines under 16 B
    across it) and C (lines across the halo's end; variant 2's long token 6 is
    accepted by the oracle, so it stays)."""
    e = dict(E.geometry_texts(shape))[name]
    both_states(sid, prime, shape, flagset, e.text, refs.want((name, shape), e.text, flagset), (name, shape, flagset))


@pytest.mark.parametrize("name", GEOMETRY)
@pytest.mark.parametrize("shape", E.SHAPES)
def test_geometry_two_pass(sid, refs, shape, name):
    """The same edges under the index kernels' 4 KiB tiles: -E -0.5 has no
    class tables, so the chunk goes through the index and the per-line parse."""
    e = dict(E.geometry_texts(shape))[name]
    eng = engine(sid, "twopass")
    st = run_text(eng, e.text, refs.want((name, shape), e.text, "twopass"), (name, shape))
    eng.close()
    assert st.chunks == 1 and st.chunks_tiled == 0


@pytest.mark.parametrize("form", ["short", "long"])
@pytest.mark.parametrize("shape", E.SHAPES)
def test_chunk_ends(sid, refs, prime, shape, form):
    """Family D: one text per chunk end c1, with and without a final newline,
    longest first on one engine with one ring slot, so that the previous
    run's valid-looking lines lie directly behind c1.  -m local for every
    end; Lynch, --only het and the other engine state for every fourth, the
    two-pass path for every eighth."""
    ends = E.d_ends(shape, form)
    other = "lane" if shape == "quad" else "quad"
    for flagset, state, step in (("local", shape, 1), ("lynch", shape, 4), ("het", shape, 4), ("twopass", None, 8),
                                 ("local", other, 4)):
        eng = engine(sid, flagset, prime if state == "quad" else None, slots=1, chunk_bytes=1 << 20)
        try:
            first = True
            for c1 in ends[::step]:
                for nl in (True, False):
                    text = E.text_d(shape, c1, form, nl).text
                    want = refs.want(("D", shape, c1, form, nl), text, flagset)
                    what = (shape, form, c1, nl, flagset, state)
                    if first and state == shape == "quad":
                        run_text(eng, text, want, what)   # (the pass that may raise the cap)
                    first = False
                    run_text(eng, text, want, what, intended=state == shape)
        finally:
            eng.close()


@pytest.mark.parametrize("first", sorted(E.E_FIRST))
@pytest.mark.parametrize("shape", E.SHAPES)
def test_c0_sweep(sid, gpu, refs, prime, shape, first):
    """Family E: the text in device memory at every offset s of a 16-B
    window (source_device_text: c0 = s, the base rounded down), valid-looking
    lines before and behind it."""
    import torch
    text = E.text_e(shape, first).text
    for fs, offsets in (("local", range(16)), ("lynch", (1, 15)), ("het", (1, 15))):
        want = refs.want(("E", shape, first), text, fs)
        eng = engine(sid, fs, prime if shape == "quad" else None)
        try:
            for i, s in enumerate(offsets):
                before, after = E.surround(64 + s)
                buf = torch.frombuffer(bytearray(before + text + after), dtype=torch.uint8).cuda()
                torch.cuda.synchronize()
                assert buf.data_ptr() % 16 == 0
                for rep in range(2 if shape == "quad" and i == 0 else 1):   # (the pass that may raise the cap)
                    eng.source_device_text(buf.data_ptr() + 64 + s, len(text), keep=buf)
                    out, st = eng.run()
                    same = out == want
                    assert same, (shape, first, s, fs, first_diff(out, want))
                assert (st.chunks, st.chunks_tiled, st.tile_overflows) == (1, 1, 0), (shape, first, s, fs)
        finally:
            eng.close()


# ------------------------------------------------------------ counter edges --
PATHS = {"lane": (False, "lane"), "quad": (False, "quad"), "general": (True, "lane")}   # (indel, engine state)


@pytest.mark.parametrize("align", E.ALIGN)
@pytest.mark.parametrize("path", sorted(PATHS))
def test_counter_profiles(sid, oracle, refs, prime, path, align):
    """Runs of one symbol around the 63-window flush (1008), the 10-bit field
    (1024), the accumulator (4096) and the u16 wrap: the Lynch pass's unique
    profiles, keys and multiplicities, against oracle.unique_profiles of the
    counts oracle.read_bases gives for each line; then the records."""
    indel, state = PATHS[path]
    text, _ = E.counter_text(align, indel)
    rows, _, u = oracle.unique_profiles(E.counter_counts(oracle, align, indel))
    want = {int(sid.profile_key(np.array([p], np.uint16))[0]): c for p, c, _ in rows}
    eng = engine(sid, "lynch", prime if state == "quad" else None, chunk_bytes=2 * len(text))
    try:
        for rep in range(2 if state == "quad" else 1):
            eng.source_text(text)
            st = eng.ingest()
            keys, cnts = eng.profile_table()
            got = dict(zip(keys.tolist(), cnts.tolist()))
            assert len(keys) == len(got) == u
            diff = {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
            assert not diff, (path, align, [(hex(k), v) for k, v in sorted(diff.items())[:6]])
            eng.estimate()
            out, _ = eng.emit()
            ref = refs.want(("counter", align, indel), text, "lynch")
            same = out == ref
            assert same, (path, align, first_diff(out, ref))
        assert (st.chunks, st.chunks_tiled, st.tile_overflows) == (1, 1, 0)
    finally:
        eng.close()


@pytest.mark.parametrize("align", E.ALIGN)
@pytest.mark.parametrize("path", sorted(PATHS) + ["twopass"])
def test_counter_csv(sid, refs, prime, path, align):
    """-m local's records of the same lines (coverage across the table's
    limit of 1024: the fix-up kernel above it); test_tile_edges proves on the
    CPU that a count one off, or a field spilt into its neighbour, changes
    the record of every line up to 4097."""
    indel, state = PATHS.get(path, (False, "lane"))
    text, _ = E.counter_text(align, indel)
    flagset = "twopass" if path == "twopass" else "local"
    eng = engine(sid, flagset, prime if state == "quad" else None, chunk_bytes=2 * len(text))
    try:
        want = refs.want(("counter", align, indel), text, flagset)
        if path == "twopass":
            assert run_text(eng, text, want, (path, align)).chunks_tiled == 0
        else:
            run_intended(eng, state, text, want, (path, align))
    finally:
        eng.close()
