"""The judge of the grep tests: the semantics of include/plakar_cdc.h, "grep",
restated over bytes.find.  It calls nothing of the library.  No test lives in
this file.

A hit is the tuple (text, line, off, len, col, mask, nocc), the fields of
cdc_grep_hit in order."""

NOCC_MAX = 2 ** 32 - 1


def fold(b):
    """ASCII-only case folding: A-Z to a-z, every other byte as it is."""
    return bytes(c | 0x20 if 0x41 <= c <= 0x5A else c for c in b)


def check_patterns(patterns):
    if not 1 <= len(patterns) <= 32:
        raise ValueError("1 to 32 patterns")
    for p in patterns:
        if not 1 <= len(p) <= 256 or b"\n" in p:
            raise ValueError("a pattern has 1 to 256 bytes and no newline")


def split_lines(text):
    """grep's lines as (offset, bytes): k newlines make k lines when the text
    ends in one or is empty, else k + 1."""
    out, lo = [], 0
    while lo < len(text):
        hi = text.find(b"\n", lo)
        if hi < 0:
            hi = len(text)
        out.append((lo, text[lo:hi]))
        lo = hi + 1
    return out


def occurrences(line, pat):
    """Every column at which pat occurs in line, overlapping ones included."""
    cols, i = [], line.find(pat)
    while i >= 0:
        cols.append(i)
        i = line.find(pat, i + 1)
    return cols


def grep_text(text, patterns, ignore_case=False, index=0, base=0):
    """(hits, lines, binary) of one text: all matching lines, `off` counted from base."""
    check_patterns(patterns)
    pats = [fold(p) for p in patterns] if ignore_case else [bytes(p) for p in patterns]
    lines = split_lines(bytes(text))
    hits = []
    for no, (off, raw) in enumerate(lines, 1):
        line = fold(raw) if ignore_case else raw
        mask, nocc, col, seen = 0, 0, None, {}
        for k, p in enumerate(pats):
            cols = seen[p] if p in seen else seen.setdefault(p, occurrences(line, p))  # a duplicate counts again
            if cols:
                mask |= 1 << k
                nocc += len(cols)
                col = cols[0] if col is None else min(col, cols[0])
        if mask:
            hits.append((index, no, base + off, len(raw), col, mask, min(nocc, NOCC_MAX)))
    return hits, len(lines), b"\0" in bytes(text)


def grep_buffer(buf, texts, patterns, ignore_case=False, limit=0):
    """cdc_grep_device's answer for the texts (offset, length) of buf:
    (hits, lines, matched, binary), the hits cut to `limit` per text."""
    hits, lines, matched, binary = [], [], [], []
    for i, (off, ln) in enumerate(texts):
        h, nl, b = grep_text(bytes(buf[off:off + ln]), patterns, ignore_case, i, off)
        lines.append(nl)
        matched.append(len(h))
        binary.append(b)
        hits += h[:limit] if limit else h
    return hits, lines, matched, binary


def text_of(data, hits, max_line_bytes, base=0):
    """The matched-line text: per hit the line's first max_line_bytes bytes and a newline."""
    return b"".join(bytes(data[h[2] - base:h[2] - base + min(h[3], max_line_bytes)]) + b"\n" for h in hits)
