"""The engine's strip crews (sid_engine_cfg.strip): pinned host
text whose quality columns host threads drop ahead of the upload.  Whatever the
crew strips, the records, the rows, the first error and its offset are those
of the run that uploads the text as it is.  370,000 synthetic 30x sites (the
size tests/test_engine_gpu.py uses) in 3 MiB chunks, the engine bench.py's
PCIe leg builds (device_sink 2, a host arena)."""
import pytest

pytestmark = pytest.mark.gpu

N, SEED, SPC = 370_000, 31, 100_000
CHUNK = 3 << 20
METHODS = {"local": (dict(method="local"), []),
           "bayes": (dict(method="bayes"), ["-m", "bayes"]),
           "R-lr": (dict(method="likelihood_ratio", estimate_prior=True), ["-R", "-m", "likelihood_ratio"])}


def pin(text: bytes):
    import torch
    return torch.frombuffer(bytearray(text), dtype=torch.uint8).pin_memory()


class Inputs:
    def __init__(self, sid, oracle, tmp):
        self.sid, self.oracle, self.tmp = sid, oracle, tmp
        self.text = sid.synth_text(SEED, N, 30.0, sites_per_chrom=SPC)
        self.host = pin(self.text)
        self._ref = {}

    def ref(self, text: bytes, flags, key):
        """The oracle CLI's records (its stdout behind the header) for text, computed once per key."""
        if key not in self._ref:
            p = self.tmp / f"{key}.plp"
            p.write_bytes(text)
            r = self.oracle.run_cli(list(flags) + [str(p)])
            assert r.returncode == 0, r.stderr[-500:]
            assert r.stdout.startswith(self.sid.HEADER)
            self._ref[key] = r.stdout[len(self.sid.HEADER):]
            p.unlink()
        return self._ref[key]


@pytest.fixture(scope="module")
def inputs(sid, oracle, gpu, tmp_path_factory):
    return Inputs(sid, oracle, tmp_path_factory.mktemp("strip"))


def engine(sid, n_bytes, strip, **kw):
    return sid.Engine(device_sink=2, chunk_bytes=CHUNK, host_hold_bytes=n_bytes, strip=strip, **kw)


def run(sid, host, n_bytes, strip, rows=None, **kw):
    """One run over pinned text: (ingest stats, records, rows)."""
    eng = engine(sid, n_bytes, strip, **kw)
    try:
        eng.source_host_ptr(host.data_ptr(), n_bytes, keep=host)
        st = eng.ingest()
        eng.estimate()
        _, st2 = eng.emit()
        got = eng.records_bytes(st.chunks)
        assert st2.bytes_out == len(got)
        return st, got, (getattr(eng, rows)() if rows else None)
    finally:
        eng.close()


@pytest.mark.parametrize("strip", [-1, 1, 2])
@pytest.mark.parametrize("mkey", sorted(METHODS))
def test_records_equal_the_oracles(sid, inputs, mkey, strip):
    kw, flags = METHODS[mkey]
    st, got, _ = run(sid, inputs.host, len(inputs.text), strip, **kw)
    assert st.sites == N and st.chunks >= 8 and st.bytes_in == len(inputs.text)
    assert got == inputs.ref(inputs.text, flags, mkey)
    print(f"strip={strip} {mkey}: chunks {st.chunks} stripped {st.chunks_stripped} strip_bytes {st.strip_bytes} "
          f"h2d_bytes {st.h2d_bytes} tiled {st.chunks_tiled} overflows {st.tile_overflows}")
    assert st.h2d_bytes == st.bytes_in - st.strip_bytes
    if strip == 1:
        assert st.chunks_stripped == st.chunks
        # (a 30x line of ~81 B loses its ~31 B of qualities: every region of every chunk was stripped)
        assert st.strip_bytes > 0.3 * st.bytes_in
    elif strip == 2:
        assert st.chunks_stripped == (st.chunks + 1) // 2
        assert st.tile_overflows == 0
    else:
        assert st.chunks_stripped == 0 and st.strip_bytes == 0
    if mkey == "local":
        assert st.tile_overflows == 0 and st.chunks_tiled == st.chunks


@pytest.mark.parametrize("mkey", ["local", "R-lr"])
def test_default_takes_what_is_ready(sid, inputs, mkey):
    """strip 0, the default: the upload never waits for the crew, so how much
    of a chunk goes up stripped depends on the timing -- any mix of stripped
    and untouched regions gives the same records, and the stats add up."""
    kw, flags = METHODS[mkey]
    for _ in range(2):
        st, got, _ = run(sid, inputs.host, len(inputs.text), 0, **kw)
        print(f"strip=0 {mkey}: chunks {st.chunks} stripped {st.chunks_stripped} strip_bytes {st.strip_bytes} "
              f"overflows {st.tile_overflows}")
        assert got == inputs.ref(inputs.text, flags, mkey)
        assert st.h2d_bytes == st.bytes_in - st.strip_bytes and st.chunks_stripped <= st.chunks
        assert (st.strip_bytes > 0) == (st.chunks_stripped > 0)
        assert st.tile_overflows == 0


@pytest.mark.parametrize("what", ["vcf", "regions", "windows"])
def test_options_see_the_same_sites(sid, inputs, what):
    rg = None
    if what == "vcf":
        kw, rows = dict(format="vcf"), None
    elif what == "regions":
        rg = sid.Regions(b"chr1\t1000\t60000\nchr2\t5\t777\nchr3\t99000\t100000\nchr4\t0\t70000\n")
        kw, rows = dict(regions=rg), None
    else:
        kw, rows = dict(window=1000), "windows"
    try:
        st0, got0, rows0 = run(sid, inputs.host, len(inputs.text), -1, rows=rows, **kw)
        st1, got1, rows1 = run(sid, inputs.host, len(inputs.text), 1, rows=rows, **kw)
    finally:
        if rg:
            rg.close()
    assert st1.chunks_stripped == st1.chunks == st0.chunks and st0.chunks_stripped == 0
    assert len(got0) > 100_000 and got1 == got0
    assert rows1 == rows0 and (rows is None or len(rows0) >= N // 1000)


def test_quality_is_not_stripped(sid, inputs):
    text = sid.synth_text(SEED, 120_000, 30.0, sites_per_chrom=SPC, mapq=True)
    host = pin(text)
    st0, got0, _ = run(sid, host, len(text), -1, method="quality")
    st1, got1, _ = run(sid, host, len(text), 1, method="quality")
    assert st1.chunks_stripped == 0 and st1.strip_bytes == 0 and st1.h2d_bytes == len(text)
    assert st1.sites == 120_000 and got1 == got0 and len(got0) > 100_000


def test_error_kind_and_offset(sid, inputs):
    """A line with a two-byte reference token in chunk 3: the same status and
    input byte offset as the run that strips nothing."""
    at = inputs.text.index(b"\n", 3 * CHUNK + CHUNK // 2) + 1
    f = inputs.text[at:inputs.text.index(b"\n", at)].split(b"\t")
    f[2] += b"C"
    text = inputs.text[:at] + b"\t".join(f) + inputs.text[inputs.text.index(b"\n", at):]
    host = pin(text)
    seen = []
    for strip in (-1, 1, 2):
        eng = engine(sid, len(text), strip)
        eng.source_host_ptr(host.data_ptr(), len(text), keep=host)
        with pytest.raises(sid.SidError) as ei:
            eng.ingest()
        seen.append((ei.value.status, ei.value.stats.status_kind, ei.value.offset))
        eng.close()
    print(seen, at)
    assert seen[0][0] != 0 and seen[0][2] // CHUNK == 3
    assert seen[1] == seen[0] and seen[2] == seen[0]


def test_missing_quality_column(sid, inputs):
    """Lines without their quality column (five tokens) are no error for the
    methods that do not read it, stripped or not."""
    lines = inputs.text[:inputs.text.index(b"\n", 8 * CHUNK) + 1].split(b"\n")[:-1]
    text = b"".join((l[:l.rindex(b"\t")] if i % 7 == 3 else l) + b"\n" for i, l in enumerate(lines))
    host = pin(text)
    st0, got0, _ = run(sid, host, len(text), -1)
    st1, got1, _ = run(sid, host, len(text), 1)
    assert st0.sites == st1.sites == len(lines) and st1.chunks_stripped == st1.chunks
    assert got1 == got0 == inputs.ref(text, [], "noquals")


def test_two_runs_on_one_engine(sid, inputs):
    eng = engine(sid, len(inputs.text), 1)
    eng.source_host_ptr(inputs.host.data_ptr(), len(inputs.text), keep=inputs.host)
    for _ in range(2):
        st = eng.ingest()
        eng.estimate()
        eng.emit()
        assert st.chunks_stripped == st.chunks and st.tile_overflows == 0
        assert eng.records_bytes(st.chunks) == inputs.ref(inputs.text, [], "local")
    eng.close()


def test_deep_text_quad_shape(sid, inputs):
    """200x lines (over 256 B: the quad shape) whose stripped form is under
    256 B a line (the lane shape)."""
    n = 60_000
    text = sid.synth_text(77, n, 200.0, sites_per_chrom=SPC)
    assert len(text) / n > 256
    host = pin(text)
    st, got, _ = run(sid, host, len(text), 1)
    print(f"200x: chunks {st.chunks} stripped {st.chunks_stripped} strip_bytes {st.strip_bytes} of {st.bytes_in} "
          f"tiled {st.chunks_tiled} overflows {st.tile_overflows}")
    assert st.sites == n and st.chunks >= 8 and st.chunks_stripped == st.chunks
    # (the slots and the shape follow the stripped lines ahead of every chunk: none goes the two-pass way)
    assert st.tile_overflows == 0 and st.chunks_tiled == st.chunks
    assert got == inputs.ref(text, [], "deep")


@pytest.mark.parametrize("strip", [1, 2, 0])
def test_pass_two_reads_stripped_chunks_again(sid, inputs, strip):
    """-R -m likelihood_ratio with a retain budget that holds a chunk's kept
    parse (28 B a site) but none of the text: pass 2 uploads the chunks again,
    and the kept parse's line offsets must meet the bytes they were made on.
    Chrom names longer than 8 bytes are read from the text by the writer."""
    n = 150_000
    text = sid.synth_text(41, n, 30.0, sites_per_chrom=40_000).replace(b"chr", b"chromosome_")
    host = pin(text)
    eng = engine(sid, len(text), strip, method="likelihood_ratio", estimate_prior=True, retain_bytes=5 << 19)
    try:
        eng.source_host_ptr(host.data_ptr(), len(text), keep=host)
        st = eng.ingest()
        eng.estimate()
        _, st2 = eng.emit()
        got = eng.records_bytes(st.chunks)
    finally:
        eng.close()
    print(f"reload strip={strip}: chunks {st.chunks} stripped {st.chunks_stripped} retained {st.chunks_retained} "
          f"reloaded {st2.chunks_reloaded}")
    assert st.sites == n and st.chunks >= 4 and st.chunks_retained == 0 and st2.chunks_reloaded == st.chunks
    if strip:
        assert st.chunks_stripped == (st.chunks if strip == 1 else (st.chunks + 1) // 2)
    assert got == inputs.ref(text, ["-R", "-m", "likelihood_ratio"], "reload")
