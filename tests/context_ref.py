"""A Python restatement of --context N (sid_opts.context), for the tests: the
dilation over record indices, the filter of a CSV by label, region and
context, and the model of the chunks' descriptors that the stitch is fed.
Nothing here calls the library."""

MAXN = 64


def dilate(sel, n):
    """keep[i] = some selected j with |i - j| <= n (sel: one bool per record)."""
    m = len(sel)
    keep = [False] * m
    d = n + 1
    for i in range(m):
        d = 0 if sel[i] else min(d + 1, n + 1)
        keep[i] = d <= n
    d = n + 1
    for i in range(m - 1, -1, -1):
        d = 0 if sel[i] else min(d + 1, n + 1)
        keep[i] = keep[i] or d <= n
    return keep


def selected(lines, select="all", ref=None):
    """One bool per record line: its label is `select` (the fifth field from the right) and it lies in `ref`."""
    out = []
    for ln in lines:
        ok = select == "all" or ln.rsplit(b",", 5)[1] == select.encode()
        if ok and ref is not None:
            f = ln.rsplit(b",", 6)   # from the right: a chrom may hold commas
            ok = ref.contains(f[0], int(f[1]))
        out.append(ok)
    return out


def filter_csv(csv: bytes, n: int, select="all", ref=None):
    """(header + the records within n records of a selected one, selected, context records, dropped)."""
    lines = csv.splitlines(keepends=True)
    if not lines:
        return b"", 0, 0, 0
    sel = selected(lines[1:], select, ref)
    keep = dilate(sel, n)
    out = [ln for ln, k in zip(lines[1:], keep) if k]
    return lines[0] + b"".join(out), sum(sel), len(out) - sum(sel), len(lines) - 1 - len(out)


def mark_model(code_all, code, n):
    """sid_context_mark: the codes (lists of ints) after it."""
    idx = [i for i, c in enumerate(code_all) if not c & 0x40]
    keep = dilate([not code[i] & 0x40 for i in idx], n)
    out = list(code)
    for i, k in zip(idx, keep):
        if k:
            out[i] &= ~0x40 & 0xFF
    return out


def chunk_desc(sel, lens, n):
    """The descriptor of a chunk alone: sel / lens = its records' selected flags and byte lengths.  A dict of
    records, has_sel, lead, trail (saturated at n + 1), head_keep / tail_keep (the in-chunk verdicts of the
    first / last min(n, records) records, as bit masks), head_len / tail_len."""
    r = len(sel)
    z = min(n, r)
    keep = dilate(sel, n)
    first = next((i for i, s in enumerate(sel) if s), None)
    last = next((i for i in range(r - 1, -1, -1) if sel[i]), None)
    return dict(records=r, has_sel=int(first is not None),
                lead=min(first if first is not None else r, n + 1),
                trail=min(r - 1 - last if last is not None else r, n + 1),
                head_keep=sum(1 << k for k in range(z) if keep[k]),
                tail_keep=sum(1 << k for k in range(z) if keep[r - z + k]),
                head_len=list(lens[:z]), tail_len=list(lens[r - z:]) if z else [])
