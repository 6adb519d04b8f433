"""The yardstick of the diff tests: the Go split rule, Python's difflib over
the lines it gives, a Python executor of emit records, and the id cases the
matcher is held to."""
import difflib
import random

import numpy as np

from plakar_amd import diff

PREFIX, LITERAL, NEWLINE = 0x100, 0x200, 0x400


def split_lines(text):
    """difflib.SplitLines of go-difflib: strings.SplitAfter(s, "\\n"), then
    "\\n" appended to the last element: k newlines give k + 1 lines, each
    ending in a newline."""
    parts = bytes(text).split(b"\n")
    return [p + b"\n" for p in parts]


def line_records(text, base=0):
    """(off, len) of every line of a text that starts at `base`."""
    out, off = [], base
    for p in bytes(text).split(b"\n"):
        out.append((off, len(p)))
        off += len(p) + 1
    return out


def expected_diff(a, b, from_name=b"a", to_name=b"b", n=3):
    return b"".join(difflib.diff_bytes(difflib.unified_diff, split_lines(a), split_lines(b), from_name, to_name, n=n,
                                       lineterm=b"\n"))


def first_ids(lines):
    """ids[i] = the smallest j <= i with the same line."""
    seen = {}
    return [seen.setdefault(ln, i) for i, ln in enumerate(lines)]


def execute(records, plain, literal, size, fill=0xEE):
    """What cdc_diff_emit_device writes, on the host: returns a bytearray of
    `size` bytes, untouched bytes left as `fill`."""
    out = bytearray([fill]) * size
    for r in records:
        src = literal if int(r["flags"]) & LITERAL else plain
        o, ln, f, d = int(r["src_off"]), int(r["len"]), int(r["flags"]), int(r["dst_off"])
        if f & PREFIX:
            out[d] = f & 0xFF
            d += 1
        out[d:d + ln] = bytes(src[o:o + ln])
        if f & NEWLINE:
            out[d + ln] = 0x0A
    return out


def plan_text(a, b, n, from_name=b"a", to_name=b"b"):
    """The unified diff of two texts through cdc_diff_script and
    cdc_diff_emit_plan, executed on the host: ids from a Python dict, the
    plaintext a + b."""
    la, lb = split_lines(a), split_lines(b)
    ids = first_ids(la + lb)
    plain = bytes(a) + bytes(b)
    ra = np.zeros(len(la), dtype=diff.LINE_DTYPE)
    rb = np.zeros(len(lb), dtype=diff.LINE_DTYPE)
    for r, recs in ((ra, line_records(a)), (rb, line_records(b, len(a)))):
        for k, (off, ln) in enumerate(recs):
            r[k]["off"], r[k]["len"] = off, ln
    ops = diff.diff_ops(ids[:len(la)], ids[len(la):], n)
    recs, lit, size = diff.diff_emit_plan(ops, ra, rb, from_name, to_name)
    return bytes(execute(recs, plain, lit, size)), recs, lit


def id_cases():
    """(name, a, b) sequences of ids for the matcher."""
    cases = [("both empty", [], []), ("a empty", [], [1, 2, 3]), ("b empty", [1, 2, 3], []),
             ("equal", list(range(40)), list(range(40))), ("one each, equal", [7], [7]), ("one each, different", [7], [8])]
    base = list(range(100, 140))
    for where, at in (("start", 0), ("middle", 20), ("end", 39)):
        r = list(base)
        r[at] = 999
        cases.append((f"replace at the {where}", base, r))
        cases.append((f"insert at the {where}", base, base[:at + (where == "end")] + [999] + base[at + (where == "end"):]))
        cases.append((f"delete at the {where}", base, base[:at] + base[at + 1:]))
    long = list(range(1000, 1100))
    for n in (0, 1, 3):
        for gap in (2 * n, 2 * n + 1):
            r = list(long)
            r[30] = 5
            r[30 + gap + 1] = 6  # `gap` equal lines between the two changes
            cases.append((f"two changes {gap} apart (n={n})", long, r))
    for nb in (199, 200, 201):
        # id 1 occurs 4 times: past the popular threshold of nb // 100 + 1 = 2 or 3 once nb >= 200
        b = list(range(10, 10 + nb))
        for at in (5, 60, 120, 180):
            b[at] = 1
        a = [1, 11, 12, 1, 13] + b[40:90] + [1, 1] + b[130:170]
        cases.append((f"popular id, len(b)={nb}", a, b))
    # every third line is "}" (id 0): 1,000 occurrences in 3,000 lines, far past the threshold
    a = [0 if i % 3 == 2 else 10 + i for i in range(3000)]
    b = list(a)
    del b[1500:1506]
    b[700] = 5
    b[2222:2222] = [6, 0, 7]
    cases.append(("every third line is }", a, b))
    rng = random.Random(20240611)
    for t in range(200):
        k = rng.randint(2, 50)
        cases.append((f"random {t}", [rng.randrange(k) for _ in range(rng.randint(0, 400))],
                      [rng.randrange(k) for _ in range(rng.randint(0, 400))]))
    return cases


def ids_to_text(ids):
    """A text whose Go split is one line per id, plus the phantom last line."""
    return b"".join(b"line %d\n" % i for i in ids)
