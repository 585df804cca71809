"""The selection by label on the host (sid_select_mark + sid_format_csv, the
--host-parse path of --only) and in the binding (Opts.select).  CPU.

The expected output is always the unselected output filtered in Python by the
label field, the fifth comma-separated field from the right
(line.rsplit(",", 5)[1]) -- not "the line contains ,het,"."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
TAGS = ["local", "local_R", "lr", "lr_R", "bayes"]


def select_lines(csv: bytes, select: str) -> bytes:
    """Header + the records of `csv` whose label field is `select` ("all": every one)."""
    lines = csv.splitlines(keepends=True)
    keep = [ln for ln in lines[1:] if select == "all" or ln.rsplit(b",", 5)[1] == select.encode()]
    return lines[0] + b"".join(keep)


@pytest.fixture(scope="module")
def sites(sid):
    with open(os.path.join(GOLD, "c1_10k.plp"), "rb") as f:
        return sid.parse_text(f.read())


def golden_arrays(sites, csv: bytes):
    """code / hom_conf / het_conf per site of the input from a golden CSV: its
    records are in site order, a site without one was dropped (bit 6)."""
    n = len(sites)
    names = np.empty(n, object)
    bounds = [st for st, _ in sites.chroms] + [n]
    for k, (st, nm) in enumerate(sites.chroms):
        names[st:bounds[k + 1]] = nm
    code = np.full(n, 0x40, np.uint8)
    hom, het = np.zeros(n), np.zeros(n)
    recs = csv.splitlines()[1:]
    i = 0
    for r in recs:
        chrom, pos, label, gt, a, b, conf_type = r.rsplit(b",", 6)
        while not (names[i] == chrom and sites.positions[i] == int(pos)):
            i += 1
        code[i] = b"ACGT".index(gt[0:1]) | (b"ACGT".index(gt[1:2]) << 2) | (0x80 if label == b"het" else 0)
        hom[i], het[i] = float(a), float(b)
        i += 1
    return code, hom, het, conf_type.decode()


@pytest.mark.parametrize("select", ["all", "het", "hom"])
@pytest.mark.parametrize("tag", TAGS)
def test_select_mark_and_format_csv_give_the_filtered_golden(sid, sites, tag, select):
    csv = gzip.open(os.path.join(GOLD, f"c1_10k.{tag}.csv.gz")).read()
    code, hom, het, conf_type = golden_arrays(sites, csv)
    header = csv.splitlines(keepends=True)[0]
    # the arrays reproduce the golden itself (the test's own reconstruction)
    assert header + sid.format_csv(sites, code, hom, het, conf_type) == csv
    want = select_lines(csv, select)
    nhet = len(select_lines(csv, "het").splitlines()) - 1
    assert nhet >= 10, "the golden holds too few het records for the case to mean anything"
    assert 0 < nhet < len(csv.splitlines()) - 1
    marked = sid.select_mark(code, select)
    assert header + sid.format_csv(sites, marked, hom, het, conf_type) == want
    if select == "all":
        assert (marked == code).all()
    else:   # only the "no record" bit is added, and only on the other label's sites
        other = ((code & 0x80) != 0) != (select == "het")
        assert (marked == np.where(other, code | 0x40, code)).all()


def test_select_mark_rejects_a_bad_value(sid):
    code = np.array([0x00, 0x80, 0x40], np.uint8)
    before = code.copy()
    for bad in (3, -1, 99):
        rc = sid.lib().sid_select_mark(code.ctypes.data_as(C.c_void_p), code.size, bad)
        assert rc == 1   # SID_EINVAL
        assert (code == before).all()
    assert sid.lib().sid_select_mark(None, 3, 1) == 1
    assert sid.lib().sid_select_mark(None, 0, 1) == 0
    with pytest.raises(sid.SidError):
        sid.select_mark(code, "bogus")


def test_opts_carry_the_selection(sid):
    assert sid.make_opts().select == 0
    assert sid.make_opts(select="all").select == 0
    assert sid.make_opts(select="het").select == 1
    assert sid.make_opts(select="hom").select == 2
    assert sid.make_opts(select=2).select == 2
    with pytest.raises(sid.SidError):
        sid.make_opts(select="bogus")
    o = sid.Opts()
    o.select = 7
    sid.lib().sid_opts_default(C.byref(o))
    assert o.select == 0


def test_label_field_is_not_a_substring_match():
    csv = (b"chrom,pos,label,gt,hom_conf,het_conf,conf_type\n"
           b"a,het,b,1,hom,AA,1,1,p_value\n"
           b"a,het,b,2,het,AC,0.5,1,p_value\n")
    assert select_lines(csv, "het").splitlines()[1:] == [b"a,het,b,2,het,AC,0.5,1,p_value"]
    assert select_lines(csv, "hom").splitlines()[1:] == [b"a,het,b,1,hom,AA,1,1,p_value"]
