"""BGZF input on the device: sid_bgzf_inflate_device against zlib over the
shape list of bgzf_ref.py, and compressed input through build/sid --bgzf and
sid_amd.Engine.source_bgzf against the oracle CLI's run on the plain file
(stdout, stderr, exit status).  Every compressed input is written here by
Python's zlib (bgzf_ref.write, which also reads it back through gzip)."""
import json
import os

import numpy as np
import pytest

import bgzf_ref as R
from test_select_gpu import FLAGS, Inputs, line, run

pytestmark = pytest.mark.gpu

PAYLOADS = [0xff00, 777]


@pytest.fixture(scope="module")
def shapes():
    return R.shapes()


@pytest.fixture(scope="module")
def ctx(sid, gpu):
    c = sid.Context(0)
    yield c
    c.close()


def device_inflate(sid, ctx, z, first=0, n=None, slack=0):
    """Members [first, first + n) of z inflated on the device -> bytes."""
    import torch
    idx = sid.BgzfIndex(z)
    blocks = idx.blocks()
    n = len(blocks) - first if n is None else n
    size = sum(b[3] for b in blocks[first:first + n])
    d_in = torch.frombuffer(bytearray(z) or bytearray(1), dtype=torch.uint8).cuda()
    d_out = torch.full((size + slack + 1,), 0xAA, dtype=torch.uint8, device="cuda")
    sid.bgzf_inflate_device(ctx, d_in, idx, d_out, cap=size, first_block=first, nblocks=n)
    out = d_out.cpu().numpy().tobytes()
    assert out[size:] == b"\xaa" * (slack + 1)   # nothing past the text
    idx.close()
    return out[:size]


def test_device_inflate_shapes(sid, ctx, shapes):
    """Every shape byte-exact (all of them run, the failing ones are listed)."""
    bad = []
    for name, text, z, blocks in shapes:
        try:
            if device_inflate(sid, ctx, z, slack=64) != text:
                bad.append((name, "bytes differ"))
        except sid.SidError as e:
            bad.append((name, f"status {e.status} block {e.block}"))
    assert not bad, bad


def test_device_inflate_sub_range(sid, ctx, shapes):
    by = {s[0]: s for s in shapes}
    for name, first, n in (("random_sizes_300", 7, 100), ("random_sizes_300", 299, 2), ("dynamic_pileup", 3, 1),
                           ("empty_members", 1, 4), ("payload_777", 100, 50), ("stored", 1, 0)):
        _, text, z, blocks = by[name]
        a = blocks[first][2]
        size = sum(b[3] for b in blocks[first:first + n])
        assert device_inflate(sid, ctx, z, first, n, slack=64) == text[a:a + size], (name, first, n)


def test_device_inflate_cap_too_small(sid, ctx, shapes):
    import torch
    _, text, z, _ = shapes[3]
    idx = sid.BgzfIndex(z)
    d_in = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    d_out = torch.full((len(text),), 0xAA, dtype=torch.uint8, device="cuda")
    with pytest.raises(sid.SidError) as e:
        sid.bgzf_inflate_device(ctx, d_in, idx, d_out, cap=len(text) - 1)
    assert e.value.status == 3   # SID_ENOMEM, before anything is launched
    torch.cuda.synchronize()
    assert bool((d_out == 0xAA).all())


def test_device_inflate_reports_the_lowest_bad_block(sid, ctx, shapes):
    """Damaged ranges that still index (the sanitized host build ran the same
    corpus clean, tests/test_bgzf_asan.py): SID_EBGZF and the lowest bad member,
    zlib's verdict member by member.  Status reporting only."""
    import torch
    done = 0
    for z, blocks in R.corpus():
        if blocks is not None or done >= 24:
            continue
        try:
            idx = sid.BgzfIndex(z)
        except sid.SidError:
            continue   # (a container error: the index's business, checked on the CPU)
        bad = [k for k, (coff, csize, _, _) in enumerate(idx.blocks()) if R.verdict(z[coff:coff + csize])[0] != 0]
        if not bad:
            continue
        size = idx.text_len
        d_in = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
        d_out = torch.zeros((size + 1,), dtype=torch.uint8, device="cuda")
        with pytest.raises(sid.SidError) as e:
            sid.bgzf_inflate_device(ctx, d_in, idx, d_out, cap=size)
        assert (e.value.status, e.value.block) == (R.SID_EBGZF, bad[0])
        idx.close()
        done += 1
    assert done >= 20


# ------------------------------------------------------------- the engine --
class ZInputs(Inputs):
    def __init__(self, sid, oracle, d):
        super().__init__(sid, oracle, d)
        self.dir = d
        good = [line(b"chr1", i, i % 5 == 0) for i in range(1, 1201)]
        head, tail = b"".join(good[:500]), b"".join(good[500:])
        extra = {
            # a 2,000-byte line: at payload 777 it spans three members
            "long_line": head + line(b"chr2", 1, True, b"." * 500 + b"G" * 480) + tail,
            # a line longer than the chunk: a chunk is dropped
            "huge_line": head + line(b"chr3", 7, True, b"." * 20_000 + b"T" * 20_000) + tail,
            # a malformed line in the middle
            "bad_mid": head + b"chr1\t1\tAC\t3\t...\tIII\n" + tail + head,
        }
        for k, t in extra.items():
            self.texts[k] = t
            p = d / f"{k}.plp"
            p.write_bytes(t)
            self.paths[k] = str(p)
        self._z = {}

    def bgzf(self, name, payload, **kw):
        """(path of the BGZF file, its bytes, the writer's blocks)"""
        key = (name, payload, tuple(sorted(kw.items())))
        if key not in self._z:
            z, blocks = R.write(self.text(name), payload=payload, **kw)
            p = self.dir / f"{name}.{payload}.{len(self._z)}.plp.gz"
            p.write_bytes(z)
            self._z[key] = (str(p), z, blocks)
        return self._z[key]


@pytest.fixture(scope="module")
def inputs(sid, oracle, tmp_path_factory):
    return ZInputs(sid, oracle, tmp_path_factory.mktemp("bgzf"))


def split_stats(stderr: bytes):
    """(stderr without the --stats line, the stats)"""
    lines = stderr.splitlines(keepends=True)
    js = [ln for ln in lines if ln.startswith(b'{"sites"')]
    assert len(js) == 1, stderr[-400:]
    return b"".join(ln for ln in lines if ln is not js[0]), json.loads(js[0])


def check(sid, inputs, flags, name, payload, extra=(), chunks=6, min_chunks=None, engine=True, **kw):
    """build/sid --bgzf and Engine.source_bgzf on the compressed input against
    the oracle on the plain file; chunk_bytes = a `chunks`-th of the text."""
    b = inputs.ref(flags, name)
    path, z, blocks = inputs.bgzf(name, payload, **kw)
    text = inputs.text(name)
    cb = max(len(text) // chunks, 1)
    real = [x for x in blocks if x[3]]
    a = run(sid.CLI_PATH, ["--bgzf", "--stats", "--chunk-bytes", str(cb)] + list(extra) + list(flags) + [path])
    assert a.returncode == b.returncode, (a.returncode, b.returncode, a.stderr[-400:])
    assert a.stdout == b.stdout, (flags, name, payload, extra)
    if b.returncode != 0:
        assert a.stderr == b.stderr
        return None
    err, st = split_stats(a.stderr)
    assert err == b.stderr
    if "--host-parse" in extra:
        return st
    if min_chunks is None:
        min_chunks = 5 if len(real) >= 2 * chunks else 1
    assert st["chunks"] >= min_chunks, (st["chunks"], len(real))
    assert st["bytes_in"] == len(text)
    assert (st["bgzf_bytes"], st["bgzf_blocks"]) == (sum(x[1] for x in real), len(real))
    if engine:
        method = flags[flags.index("-m") + 1] if "-m" in flags else "local"
        kwargs = {"estimate_prior": "-R" in flags}
        for f, k in (("-E", "site_error_threshold"), ("-p", "significance_level"), ("-r", "snp_prior")):
            if f in flags:
                kwargs[k] = float(flags[flags.index(f) + 1])
        if method == "bayes":
            kwargs["estimate_prior"] = False
        eng = sid.Engine(method=method, chunk_bytes=cb, **kwargs)
        eng.source_bgzf(z)
        out, est = eng.run()
        eng.close()
        assert out == b.stdout, (flags, name, payload)
        assert est.chunks == st["chunks"] and est.bgzf_blocks == len(real) and est.bytes_in == len(text)
    return st


@pytest.mark.parametrize("payload", PAYLOADS)
@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: " ".join(f) or "default")
def test_flag_sets(sid, inputs, flags, payload):
    for name in ("c1", "edge", "special", "deep"):
        check(sid, inputs, flags, name, payload)


def test_long_lines(sid, inputs):
    for flags in ([], ["-m", "bayes"]):
        check(sid, inputs, flags, "long_line", 777)
        # the 80 KB line is longer than seven chunks, whose cuts coincide
        full = check(sid, inputs, flags, "huge_line", 777, chunks=16, min_chunks=5)
        assert full["chunks"] < 16


def test_lynch_reload(sid, inputs):
    st = check(sid, inputs, ["-R", "-m", "likelihood_ratio"], "c1", 777, extra=["--hold-bytes", "1", "--retain-bytes", "1"],
               engine=False)
    assert st["chunks_reloaded"] > 0
    st = check(sid, inputs, ["-m", "bayes"], "special", 0xff00, engine=False)   # (kept in HBM for the second pass)
    assert st["chunks_retained"] > 0 and st["chunks_reloaded"] == 0


def test_lanes_2(sid, inputs):
    name, flags = "c1", ["-R", "-m", "likelihood_ratio"]
    b = inputs.ref(flags, name)
    _, z, blocks = inputs.bgzf(name, 777)
    for method, kw, ref in (("likelihood_ratio", {"estimate_prior": True}, b), ("local", {}, inputs.ref([], name))):
        eng = sid.Engine(method=method, chunk_bytes=len(inputs.text(name)) // 9, lanes=2, **kw)
        eng.source_bgzf(z)
        out, st = eng.run()
        eng.close()
        assert out == ref.stdout and st.chunks >= 5 and st.devices == 2


def test_file_source_and_engine_reuse(sid, inputs):
    """Engine.source_bgzf_file (a mapping, at an offset), then the same engine on plain text."""
    name = "special"
    b = inputs.ref([], name)
    _, z, _ = inputs.bgzf(name, 0xff00)
    p = inputs.dir / "offset.bin"
    p.write_bytes(b"x" * 5000 + z)
    eng = sid.Engine(chunk_bytes=len(inputs.text(name)) // 6)
    fd = os.open(str(p), os.O_RDONLY)
    try:
        eng.source_bgzf_file(fd, 5000)
        out, st = eng.run()
        assert out == b.stdout and st.chunks >= 5
        with pytest.raises(sid.SidError) as e:
            eng.source_bgzf_file(fd, 0)
        assert (e.value.status, e.value.offset) == (R.SID_EBGZF, 0)
        with pytest.raises(sid.SidError):   # the engine keeps no source
            eng.run()
        eng.source_text(inputs.text(name))
        out, st = eng.run()
        assert out == b.stdout and st.bgzf_blocks == 0
    finally:
        os.close(fd)
        eng.close()


def test_only_and_regions_together(sid, inputs, tmp_path):
    name = "c1"
    b = inputs.ref([], name)
    path, _, _ = inputs.bgzf(name, 777)
    recs = b.stdout.splitlines(keepends=True)
    pos = sorted({int(r.split(b",")[1]) for r in recs[1:]})
    lo, hi = pos[len(pos) // 4], pos[3 * len(pos) // 4]
    chrom = recs[1].split(b",")[0]
    bed = tmp_path / "r.bed"
    bed.write_bytes(b"%s\t%d\t%d\n" % (chrom, lo, hi))
    want = [r for r in recs[1:] if r.split(b",")[0] == chrom and lo < int(r.split(b",")[1]) <= hi
            and r.rsplit(b",", 5)[1] == b"het"]
    assert 0 < len(want) < len(recs) - 1
    cb = str(len(inputs.text(name)) // 6)
    a = run(sid.CLI_PATH, ["--bgzf", "--only", "het", "--regions", str(bed), "--chunk-bytes", cb, path])
    assert (a.returncode, a.stdout, a.stderr) == (0, recs[0] + b"".join(want), b.stderr)


def test_host_parse(sid, inputs):
    for flags in ([], ["-R", "-m", "likelihood_ratio"]):
        check(sid, inputs, flags, "special", 777, extra=["--host-parse"])
        check(sid, inputs, flags, "c1", 0xff00, extra=["--host-parse"])


def test_pipe_input(sid, inputs):
    b = inputs.ref([], "special")
    path, _, _ = inputs.bgzf("special", 777)
    with open(path, "rb") as f:
        a = run(sid.CLI_PATH, ["--bgzf", "--chunk-bytes", "50000", "/dev/stdin"], input=f.read())
    assert (a.returncode, a.stdout, a.stderr) == (b.returncode, b.stdout, b.stderr)


def test_malformed_line_late(sid, inputs):
    b = inputs.ref([], "bad_late")
    assert b.returncode != 0 and b.stdout == b""
    for payload in PAYLOADS:
        for extra in ([], ["--hold-bytes", "1"], ["--host-parse"]):
            check(sid, inputs, [], "bad_late", payload, extra=extra)
    _, z, _ = inputs.bgzf("bad_late", 777)
    text = inputs.text("bad_late")
    eng = sid.Engine(chunk_bytes=len(text) // 6)
    eng.source_bgzf(z)
    with pytest.raises(sid.SidError) as e:
        eng.run()
    eng.close()
    # the parse error's offset is the line's offset in the inflated text
    assert (e.value.status, e.value.offset) == (4, text.index(b"chr1\t1\tAC\t"))


def test_corrupt_block_and_not_bgzf(sid, inputs):
    name = "c1"
    path, z, blocks = inputs.bgzf(name, 777)
    text = inputs.text(name)
    cb = len(text) // 6
    # a member of the third chunk (text offset 2.5 chunks in), one payload bit flipped
    k = next(i for i, x in enumerate(blocks) if x[2] >= 2 * cb + cb // 2)
    coff, csize = blocks[k][0], blocks[k][1]
    bad = bytearray(z)
    bad[coff + 18 + (csize - 26) // 2] ^= 4
    # ... and a malformed line in a later chunk must not win over it, one in an earlier chunk must
    p = inputs.dir / "corrupt.plp.gz"
    p.write_bytes(bytes(bad))
    for extra in ([], ["--host-parse"], ["-m", "bayes"]):
        a = run(sid.CLI_PATH, ["--bgzf", "--chunk-bytes", str(cb)] + extra + [str(p)])
        assert (a.returncode, a.stdout) == (1, b"")
        assert a.stderr == b"sid: %s: corrupt BGZF block at byte %d\n" % (str(p).encode(), coff)
    eng = sid.Engine(chunk_bytes=cb)
    eng.source_bgzf(bytes(bad))
    with pytest.raises(sid.SidError) as e:
        eng.run()
    assert (e.value.status, e.value.offset) == (R.SID_EBGZF, coff)
    eng.source_bgzf(z)   # the engine is reusable after it
    out, _ = eng.run()
    eng.close()
    assert out == inputs.ref([], name).stdout
    # truncated in the middle of a member: found by the index
    t = inputs.dir / "cut.plp.gz"
    t.write_bytes(z[:coff + 40])
    a = run(sid.CLI_PATH, ["--bgzf", str(t)])
    assert (a.returncode, a.stdout) == (1, b"")
    assert a.stderr == b"sid: %s: corrupt BGZF block at byte %d\n" % (str(t).encode(), coff)
    # plain text and plain gzip under --bgzf
    import gzip
    g = inputs.dir / "plain.gz"
    g.write_bytes(gzip.compress(text[:5000]))
    for q in (inputs.paths[name], str(g)):
        for extra in ([], ["--host-parse"]):
            a = run(sid.CLI_PATH, ["--bgzf"] + extra + [q])
            assert (a.returncode, a.stdout, a.stderr) == (1, b"", b"sid: %s: not a BGZF file\n" % q.encode())


def test_error_order_across_chunks(sid, inputs):
    """The earliest chunk in file order with any error is the one reported."""
    text = inputs.text("bad_mid")
    at = text.index(b"chr1\t1\tAC\t")
    z, blocks = R.write(text, payload=777)
    cb = len(text) // 10
    b = inputs.ref([], "bad_mid")
    assert b.returncode != 0 and b.stdout == b""

    def flipped(k):
        bad = bytearray(z)
        bad[blocks[k][0] + 18 + (blocks[k][1] - 26) // 2] ^= 1
        return bytes(bad)
    early = next(i for i, x in enumerate(blocks) if x[2] >= at // 3)
    late = next(i for i, x in enumerate(blocks) if x[2] >= at + 2 * cb)
    for k, want_bgzf in ((early, True), (late, False)):
        p = inputs.dir / f"order{k}.plp.gz"
        p.write_bytes(flipped(k))
        a = run(sid.CLI_PATH, ["--bgzf", "--chunk-bytes", str(cb), str(p)])
        assert a.stdout == b""
        if want_bgzf:
            assert (a.returncode, a.stderr) == (1, b"sid: %s: corrupt BGZF block at byte %d\n"
                                                % (str(p).encode(), blocks[k][0]))
        else:
            assert (a.returncode, a.stderr) == (b.returncode, b.stderr)
