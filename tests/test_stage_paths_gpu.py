"""The stages between a chunk's parse and its writer -- window, depth histogram,
region mark, variant / depth mark, context mark, VCF length -- all switched on
in one engine, through every chunk formatter that runs them: the tile path's
lane and quad shapes, the two-pass path behind a tile overflow, pass 2 of
-m local -R on the kept parse (no class words: the first storing stage writes
them), the Lynch formatter and the code formatter (-m quality).  Once with the
separate marks and once with context=2, whose route does their tests itself;
each as CSV and as VCF.

The expected records are the oracle CLI's unselected records filtered by the
Python models, as test_depth_gpu.expect (CSV) and test_vcf_gpu.expect (VCF)
build them; the expected window and depth rows are windows_ref's and
depth_hist_ref's over the oracle's codes.  Both kinds of rows count every
site whatever is selected -- their stages run in front of the marks -- so they
also equal the rows of a run without any selection."""
import pytest

import depth_hist_ref as DH
import test_depth_gpu as TD
import test_vcf_gpu as TV
import windows_ref as WR
from test_depth_gpu import FLAGSETS
from test_vcf_gpu import VcfInputs

pytestmark = pytest.mark.gpu

W = 100
# path -> (flag set, input, the engine's settings, the depth bounds, what shows that the path was taken)
PATHS = {
    "tile_lane": ("local", "depth", dict(chunk_bytes=20_000), (8, 31), lambda st: st.chunks_tiled > 0),
    "tile_quad": ("local", "deep", dict(chunk_bytes=20_000), (151, 201), lambda st: st.chunks_tiled > 0),
    "two_pass": ("local", "tiny", dict(chunk_bytes=100_000), (8, 31), lambda st: st.tile_overflows > 0),
    "kept_parse": ("local_R", "depth", dict(chunk_bytes=20_000, hold_bytes=1), (8, 31),
                   lambda st: st.chunks_reloaded == 0),
    "lr": ("lr", "depth", dict(chunk_bytes=20_000), (8, 31), lambda st: True),
    "quality": ("quality", "depthq", dict(chunk_bytes=20_000), (8, 31), lambda st: True),
}


class StageInputs(VcfInputs):
    def __init__(self, sid, oracle, d):
        super().__init__(sid, oracle, d)
        self._side, self._plain = {}, {}

    def side(self, fs, name):
        """The models' (window rows, depth rows) of an input under a flag set, once each."""
        if (fs, name) not in self._side:
            kw = dict(FLAGSETS[fs][2])
            text = self.texts[name]
            sites, codes = WR.site_codes(self.sid, self.oracle, text, kw.pop("method"), **kw)
            self._side[(fs, name)] = (WR.rows(sites, codes, W), DH.rows(DH.depths(self.sid.parse_text(text).counts), codes))
        return self._side[(fs, name)]

    def plain(self, path):
        """The rows of the path's run without any selection, once each."""
        if path not in self._plain:
            self._plain[path] = run_engine(self.sid, self, path, "csv")[2:]
        return self._plain[path]


@pytest.fixture(scope="module")
def inputs(sid, oracle, tmp_path_factory):
    return StageInputs(sid, oracle, tmp_path_factory.mktemp("stages"))


def run_engine(sid, inputs, path, fmt, select="all", bed=None, variants=False, bounds=(0, 0), context=0, text=None,
               fs=None):
    """(records, stats, window rows, depth rows) of the path's engine with the window and the histogram on."""
    name, kw = PATHS[path][1:3]
    fs = fs or PATHS[path][0]
    rg = sid.Regions(bed[2]) if bed else None
    eng = sid.Engine(format=fmt, window=W, depth_hist=True, select=select, regions=rg, variants=int(variants),
                     min_depth=bounds[0], max_depth=bounds[1], context=context, **FLAGSETS[fs][2], **kw)
    if rg:
        rg.close()
    eng.source_text(inputs.texts[name] if text is None else text)
    out, st = eng.run(header=inputs.header(fs) if fmt == "vcf" else sid.HEADER)
    rows = eng.windows(), eng.depth_hist()
    eng.close()
    assert st.window_rows == len(rows[0]) and st.depth_rows == len(rows[1])
    return (out, st) + rows


@pytest.mark.parametrize("context", [0, 2], ids=["marks", "context"])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_every_stage_on(sid, inputs, path, context):
    fs, name, kw, bounds, taken = PATHS[path]
    sel = dict(select="het", bed=inputs.bed(name), variants=True, bounds=bounds, context=context)
    want = {"csv": TD.expect(inputs, fs, name, bounds, select="het", bed=sel["bed"], context=context, variants=True)[1],
            "vcf": TV.expect(inputs, fs, name, **sel)[1]}
    win, dep = inputs.side(fs, name)
    assert len(win) >= 15 and len(dep) >= 5 and DH.sums(win) == DH.sums(dep)
    for fmt in ("csv", "vcf"):
        out, st, w, d = run_engine(sid, inputs, path, fmt, **sel)
        assert st.chunks >= 3 and taken(st), (path, fmt, st.chunks, st.chunks_tiled, st.tile_overflows, st.chunks_reloaded)
        assert out == want[fmt], (path, fmt, context)
        assert w == win, (path, fmt, context, len(w), len(win))
        assert d == dep, (path, fmt, context, len(d), len(dep))
    assert inputs.plain(path) == (win, dep), path


@pytest.mark.parametrize("text", [b"", b"\n" * 300], ids=["no_line", "blank_lines"])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_empty_source(sid, inputs, path, text):
    fs, name, kw, bounds, _ = PATHS[path]
    # (likelihood_ratio has no estimate without a profile of coverage 4, SID_EEMPTY as the reference's exit:
    # the Lynch formatter's empty chunk through bayes)
    fs = "bayes" if fs == "lr" else fs
    for context in (0, 2):
        for fmt in ("csv", "vcf"):
            out, st, w, d = run_engine(sid, inputs, path, fmt, select="het", bed=inputs.bed(name), variants=True,
                                       bounds=bounds, context=context, text=text, fs=fs)
            assert out == (inputs.header(fs) if fmt == "vcf" else sid.HEADER), (path, fmt, context)
            assert st.sites == 0 and st.bytes_out == 0 and w == [] and d == []
