"""The region selection's semantics restated in Python for the tests -- not the
library: a BED parser, the membership test and the filter of a CSV, plus the
builders that make a BED from an input's own (chrom, pos) list.

A site is inside when its record's chrom field equals a BED chrom byte for
byte and start < pos <= end (BED: 0-based, half-open), pos being the integer
the record prints."""
import bisect

POS_MAX = 2 ** 31 - 1


class BedError(ValueError):
    def __init__(self, line):
        super().__init__(f"line {line}")
        self.line = line


def parse_bed(text: bytes):
    """{chrom: [(start, end), ...]} as written (unmerged, empty ones dropped); BedError(line) for a bad line."""
    out = {}
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for no, ln in enumerate(lines, 1):
        if ln == b"" or ln.startswith((b"#", b"track", b"browser")):
            continue
        f = [x for x in ln.replace(b"\t", b" ").split(b" ") if x]
        if len(f) == 1:
            s, e = 0, POS_MAX
        elif len(f) >= 3:
            if not (f[1].isdigit() and f[2].isdigit() and f[1].isascii() and f[2].isascii()):
                raise BedError(no)
            s, e = int(f[1]), int(f[2])
            if s > e:
                raise BedError(no)
            s, e = min(s, POS_MAX), min(e, POS_MAX)
        else:
            raise BedError(no)
        if s < e:
            out.setdefault(f[0], []).append((s, e))
        else:
            out.setdefault(f[0], [])
    return out


class RefSet:
    """The union of the intervals, per chrom; `in` by bisection over the merged list."""

    def __init__(self, bed):
        iv = parse_bed(bed) if isinstance(bed, (bytes, bytearray)) else bed
        self.m = {}
        for c, v in iv.items():
            merged = []
            for s, e in sorted(x for x in v if x[0] < x[1]):
                if merged and s <= merged[-1][1]:
                    merged[-1][1] = max(merged[-1][1], e)
                else:
                    merged.append([s, e])
            if merged:
                self.m[c] = ([a for a, _ in merged], [b for _, b in merged])

    @property
    def intervals(self):
        return sum(len(s) for s, _ in self.m.values())

    @property
    def chroms(self):
        return len(self.m)

    def contains(self, chrom: bytes, pos: int) -> bool:
        v = self.m.get(chrom)
        if v is None:
            return False
        k = bisect.bisect_left(v[0], pos) - 1   # the last start < pos
        return k >= 0 and pos <= v[1][k]


def filter_csv(csv: bytes, ref: RefSet, select: str = "all"):
    """(header + the records inside (and of the label), kept, dropped)."""
    lines = csv.splitlines(keepends=True)
    if not lines:
        return b"", 0, 0
    keep = []
    for ln in lines[1:]:
        f = ln.rsplit(b",", 6)   # from the right: a chrom may hold commas
        if ref.contains(f[0], int(f[1])) and (select == "all" or f[2] == select.encode()):
            keep.append(ln)
    return lines[0] + b"".join(keep), len(keep), len(lines) - 1 - len(keep)


def atoi(tok: bytes) -> int:
    """C atoi on a token: optional sign, leading digits, wrapped to int32."""
    i, sign = 0, 1
    if tok[:1] in (b"+", b"-"):
        sign = -1 if tok[:1] == b"-" else 1
        i = 1
    j = i
    while j < len(tok) and tok[j:j + 1].isdigit():
        j += 1
    v = sign * int(tok[i:j] or b"0")
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


def text_sites(text: bytes):
    """[(chrom, pos)] of a pileup text's non-empty lines."""
    out = []
    for ln in text.split(b"\n"):
        f = ln.replace(b"\t", b" ").split()
        if len(f) >= 2:
            out.append((f[0], atoi(f[1])))
    return out


def bed_points(sites, keep) -> bytes:
    """One-position intervals (pos - 1, pos) of the sites i with keep(i) (positive positions only)."""
    return b"".join(b"%s\t%d\t%d\n" % (c, p - 1, p) for i, (c, p) in enumerate(sites) if keep(i) and p > 0)


def bed_runs(sites, keep) -> bytes:
    """An interval over every maximal run of kept sites that share a chrom and ascend by position."""
    out, run = [], None
    for i, (c, p) in enumerate(sites + [(None, 0)]):
        k = c is not None and keep(i) and p > 0
        if run and k and c == run[0] and p > run[2]:
            run[2] = p
            continue
        if run:
            out.append(b"%s\t%d\t%d\n" % (run[0], run[1] - 1, run[2]))
        run = [c, p, p] if k else None
    return b"".join(out)


def bed_whole(sites) -> bytes:
    seen = []
    for c, _ in sites:
        if c not in seen:
            seen.append(c)
    return b"".join(c + b"\n" for c in seen)
