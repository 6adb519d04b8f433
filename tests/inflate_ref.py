"""Test infrastructure for the device GZIP Decode: a strict pure-Python reader
of one gzip member (RFC 1952) over DEFLATE (RFC 1951) with the reject list of
plakar_amd/csrc/inflate_walk.h, restated independently (codes are assigned as
the RFC's section 3.2.2 does and looked up in a dictionary, sets are judged by
their Kraft sum); a bit writer for hand-made blocks; and the fixtures, the
corruptions and the mutations that the CPU and GPU tests share."""
import functools
import struct
import zlib

import numpy as np

OK, CORRUPT, UNSUPPORTED = 0, -13, -2   # CDC_OK, CDC_E_CORRUPT, CDC_E_UNSUPPORTED
MAX_RATIO = 1032
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class Corrupt(ValueError):
    status = CORRUPT


class Unsupported(ValueError):
    status = UNSUPPORTED


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def text(n, seed=0):
    words = [b"plakar", b"snapshot", b"chunk", b"the", b"of", b"packfile", b"restore", b"a", b"device", b"blob",
             b"and", b"index", b"state", b"to", b"repository", b"checksum"]
    rng = np.random.default_rng(1000 + seed)
    out = bytearray()
    while len(out) < n:
        out += b" ".join(words[i] for i in rng.integers(0, len(words), size=64)) + b".\n"
    return bytes(out[:n])


# ---- codes ---------------------------------------------------------------------------
def assign_codes(lengths):
    """RFC 1951 3.2.2: {symbol: (code, length)}, the code's first bit highest."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s, n in enumerate(lengths):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def kraft(lengths):
    """Sum of 2^(15 - length) over the codes: 2^15 for a complete set."""
    return sum(1 << (15 - n) for n in lengths if n)


def set_ok(lengths, dist=False):
    k = kraft(lengths)
    if k == 1 << 15:
        return True
    if k > 1 << 15:
        return False
    used = [n for n in lengths if n]
    return dist and (not used or used == [1])


class _Bits:
    def __init__(self, data, pos):
        self.d, self.pos, self.buf, self.cnt = data, pos, 0, 0

    def bit(self):
        if self.cnt == 0:
            if self.pos >= len(self.d):
                raise Corrupt("the input ended")
            self.buf, self.cnt = self.d[self.pos], 8
            self.pos += 1
        b = self.buf & 1
        self.buf >>= 1
        self.cnt -= 1
        return b

    def bits(self, n):
        v = 0
        for i in range(n):
            v |= self.bit() << i
        return v

    def sym(self, table):
        code = 0
        for n in range(1, 16):
            code = code << 1 | self.bit()
            s = table.get((code, n))
            if s is not None:
                return s, n
        raise Corrupt("no such code")

    def align(self):
        self.buf = self.cnt = 0
        return self.pos


def _table(lengths):
    return {v: s for s, v in assign_codes(lengths).items()}


_FIXED = None


def inflate(data, start=0, omax=None):
    """The DEFLATE stream at data[start:]: (output, index after the last block,
    walk).  walk: per block a dict(btype, first (output index), matches [(pos,
    length, distance)], maxbits, cl (the code-length symbols read), nlit,
    ndist, litlens, distlens, and bit0 / bit1: the bit of data (counted from
    its byte 0) at which the block's BFINAL stands, and the one after the
    block's last bit, a stored block's last byte included).  Raises Corrupt."""
    global _FIXED
    if _FIXED is None:
        _FIXED = (_table(FIXED_LIT), _table(FIXED_DIST))
    B = _Bits(data, start)
    out = bytearray()
    walk = []
    while True:
        bit0 = 8 * B.pos - B.cnt
        final, btype = B.bit(), B.bits(2)
        blk = dict(btype=btype, first=len(out), matches=[], maxbits=0, cl=[], stored=None, bit0=bit0, bit1=None)
        walk.append(blk)
        if btype == 3:
            raise Corrupt("BTYPE 3")
        if btype == 0:
            at = B.align()
            if len(data) - at < 4:
                raise Corrupt("stored header")
            ln, nln = struct.unpack_from("<HH", data, at)
            if ln ^ nln != 0xFFFF:
                raise Corrupt("LEN / NLEN")
            if ln > len(data) - at - 4:
                raise Corrupt("stored block past the input")
            if omax is not None and len(out) + ln > omax:
                raise Corrupt("output past the claim")
            out += data[at + 4:at + 4 + ln]
            blk["stored"] = ln
            B.pos = at + 4 + ln
        else:
            if btype == 1:
                lit, dist = _FIXED
            else:
                nlit, ndist, ncl = B.bits(5) + 257, B.bits(5) + 1, B.bits(4) + 4
                if nlit > 286 or ndist > 30:
                    raise Corrupt("too many symbols")
                cl = [0] * 19
                for i in range(ncl):
                    cl[CL_ORDER[i]] = B.bits(3)
                if not set_ok(cl):
                    raise Corrupt("code-length set")
                clt = _table(cl)
                lens = []
                while len(lens) < nlit + ndist:
                    s, _ = B.sym(clt)
                    if s < 16:
                        lens.append(s)
                        blk["cl"].append((s, 1, len(lens) - 1))
                        continue
                    if s == 16:
                        if not lens:
                            raise Corrupt("repeat with nothing before it")
                        rep, fill = 3 + B.bits(2), lens[-1]
                    elif s == 17:
                        rep, fill = 3 + B.bits(3), 0
                    else:
                        rep, fill = 11 + B.bits(7), 0
                    if len(lens) + rep > nlit + ndist:
                        raise Corrupt("a run past HLIT + HDIST")
                    blk["cl"].append((s, rep, len(lens)))
                    lens += [fill] * rep
                if lens[256] == 0:
                    raise Corrupt("no end-of-block code")
                ll, dl = lens[:nlit], lens[nlit:]
                if not set_ok(ll) or not set_ok(dl, dist=True):
                    raise Corrupt("code set")
                blk.update(nlit=nlit, ndist=ndist, litlens=ll, distlens=dl)
                lit, dist = _table(ll), _table(dl)
            while True:
                s, n = B.sym(lit)
                blk["maxbits"] = max(blk["maxbits"], n)
                if s < 256:
                    if omax is not None and len(out) >= omax:
                        raise Corrupt("output past the claim")
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise Corrupt("literal/length symbol 286 or 287")
                ln = LEN_BASE[s - 257] + B.bits(LEN_EXTRA[s - 257])
                d, n = B.sym(dist)
                if d > 29:
                    raise Corrupt("distance symbol 30 or 31")
                ds = DIST_BASE[d] + B.bits(DIST_EXTRA[d])
                if ds > len(out):
                    raise Corrupt("a distance before the first byte")
                if omax is not None and len(out) + ln > omax:
                    raise Corrupt("output past the claim")
                blk["matches"].append((len(out), ln, ds))
                if ds >= ln:
                    out += out[len(out) - ds:len(out) - ds + ln]
                else:
                    for _ in range(ln):
                        out.append(out[-ds])
        blk["bit1"] = 8 * B.pos - B.cnt
        if final:
            break
    return bytes(out), B.align(), walk


def member_header(data):
    """The index of the body's first byte.  Raises Corrupt."""
    n = len(data)
    if n < 10 or data[0] != 0x1F or data[1] != 0x8B or data[2] != 8:
        raise Corrupt("magic / CM")
    flg = data[3]
    if flg & 0xE0:
        raise Corrupt("reserved FLG bit")
    p = 10
    if flg & 4:
        if n - p < 2:
            raise Corrupt("FEXTRA")
        p += 2 + struct.unpack_from("<H", data, p)[0]
        if p > n:
            raise Corrupt("FEXTRA")
    for f in (8, 16):
        if flg & f:
            z = data.find(b"\0", p)
            if z < 0:
                raise Corrupt("FNAME / FCOMMENT")
            p = z + 1
    if flg & 2:
        if n - p < 2 or struct.unpack_from("<H", data, p)[0] != zlib.crc32(data[:p]) & 0xFFFF:
            raise Corrupt("FHCRC")
        p += 2
    return p


def claim(data):
    """What sizing decides: (status, claimed size)."""
    if not data:
        return OK, 0
    if len(data) > 0x7FFFFFFF:
        return UNSUPPORTED, 0
    try:
        h = member_header(data)
    except Corrupt:
        return CORRUPT, 0
    if len(data) - h < 8:
        return CORRUPT, 0
    c = struct.unpack_from("<I", data, len(data) - 4)[0]
    if c > MAX_RATIO * (len(data) - h - 8):
        return CORRUPT, 0
    return OK, c


def gunzip(data):
    """The member's content.  Raises Corrupt or Unsupported."""
    data = bytes(data)
    st, c = claim(data)
    if st == UNSUPPORTED:
        raise Unsupported("too long")
    if st:
        raise Corrupt("header or claim")
    if not data:
        return b""
    out, end, _ = inflate(data, member_header(data), c)
    if len(data) - end < 8:
        raise Corrupt("trailer")
    crc, isize = struct.unpack_from("<II", data, end)
    if crc != zlib.crc32(out) or isize != len(out) & 0xFFFFFFFF:
        raise Corrupt("CRC-32 / ISIZE")
    rest = data[end + 8:]
    if rest:
        if rest[:2] == b"\x1f\x8b":
            raise Unsupported("a second member")
        raise Corrupt("bytes after the trailer")
    if len(out) != c:
        raise Corrupt("less than the claim")
    return out


def status_of(data):
    """(status, content or None) as the device reports a blob."""
    try:
        return OK, gunzip(data)
    except (Corrupt, Unsupported) as e:
        return e.status, None


# ---- writing -------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.out, self.buf, self.cnt = bytearray(), 0, 0

    def bits(self, v, n):
        self.buf |= (v & ((1 << n) - 1)) << self.cnt
        self.cnt += n
        while self.cnt >= 8:
            self.out.append(self.buf & 0xFF)
            self.buf >>= 8
            self.cnt -= 8

    def code(self, cv):
        code, n = cv
        self.bits(int(format(code, f"0{n}b")[::-1], 2), n)  # codes go first bit first

    def align(self):
        if self.cnt:
            self.bits(0, 8 - self.cnt)

    def bytes_(self, b):
        self.align()
        self.out += b

    def done(self):
        self.align()
        return bytes(self.out)


def len_sym(ln):
    if ln == 258:
        return 285, 0, 0
    i = max(k for k in range(28) if LEN_BASE[k] <= ln)
    return 257 + i, LEN_EXTRA[i], ln - LEN_BASE[i]


def dist_sym(d):
    i = max(k for k in range(30) if DIST_BASE[k] <= d)
    return i, DIST_EXTRA[i], d - DIST_BASE[i]


def put_ops(w, ops, lit, dist):
    """ops: ints (literals), (length, distance) pairs, or ("sym", literal/length
    symbol) / ("dsym", length, distance symbol) for what no encoder writes;
    then the end-of-block code unless the last op is "noeob"."""
    for op in ops:
        if isinstance(op, int):
            w.code(lit[op])
        elif op[0] == "sym":
            w.code(lit[op[1]])
        elif op[0] == "dsym":
            s, e, x = len_sym(op[1])
            w.code(lit[s])
            w.bits(x, e)
            w.code(dist[op[2]])
        elif op[0] == "noeob":
            return
        else:
            s, e, x = len_sym(op[0])
            w.code(lit[s])
            w.bits(x, e)
            d, e, x = dist_sym(op[1])
            w.code(dist[d])
            w.bits(x, e)
    w.code(lit[256])


def stored_block(w, data, final=False, nlen=None):
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.out += struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen) + data


def fixed_block(w, ops, final=False):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    put_ops(w, ops, assign_codes(FIXED_LIT), assign_codes(FIXED_DIST))


def flat_lengths(k):
    """k >= 2 code lengths of a complete set, as even as can be."""
    m = k.bit_length() - 1
    deep = 2 * (k - (1 << m))
    return [m] * (k - deep) + [m + 1] * deep


def plain_cl(lens):
    return [(n, None) for n in lens]


def dynamic_header(w, litlens, distlens, cl_seq=None, final=False, hlit=None, hdist=None):
    """BFINAL, BTYPE 2, the counts, the code-length code and the lengths.
    cl_seq: [(symbol, extra value or None)] spelling litlens + distlens
    (default: every length by itself).  Nothing is validated."""
    seq = cl_seq if cl_seq is not None else plain_cl(list(litlens) + list(distlens))
    used = sorted({s for s, _ in seq})
    if len(used) < 2:
        used = sorted(set(used) | {0, 18})
    fl = flat_lengths(len(used))
    cl = [0] * 19
    for s, n in zip(used, fl):
        cl[s] = n
    ncl = max(i for i in range(19) if cl[CL_ORDER[i]]) + 1
    ncl = max(ncl, 4)
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits((len(litlens) if hlit is None else hlit) - 257, 5)
    w.bits((len(distlens) if hdist is None else hdist) - 1, 5)
    w.bits(ncl - 4, 4)
    for i in range(ncl):
        w.bits(cl[CL_ORDER[i]], 3)
    codes = assign_codes(cl)
    for s, x in seq:
        w.code(codes[s])
        if s == 16:
            w.bits(x - 3, 2)
        elif s == 17:
            w.bits(x - 3, 3)
        elif s == 18:
            w.bits(x - 11, 7)


def dynamic_block(w, litlens, distlens, ops, cl_seq=None, final=False):
    dynamic_header(w, litlens, distlens, cl_seq, final)
    put_ops(w, ops, assign_codes(litlens), assign_codes(distlens))


def lengths_for(symbols, shape, size):
    """A lengths array of `size` with the given code lengths on `symbols`."""
    out = [0] * size
    for s, n in zip(sorted(symbols), shape):
        out[s] = n
    return out


def expand(ops, before=b""):
    """What a list of ops decodes to after `before`."""
    out = bytearray(before)
    for op in ops:
        if isinstance(op, int):
            out.append(op)
        elif isinstance(op[0], int):
            for _ in range(op[0]):
                out.append(out[-op[1]])
    return bytes(out[len(before):])


def member(body, content, flg=0, extra=b"", name=b"", comment=b"", cm=8, crc=None, isize=None, fhcrc=None):
    """A gzip member around a raw DEFLATE body."""
    h = bytearray(struct.pack("<BBBBIBB", 0x1F, 0x8B, cm, flg, 0, 0, 255))
    if flg & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flg & 8:
        h += name + b"\0"
    if flg & 16:
        h += comment + b"\0"
    if flg & 2:
        h += struct.pack("<H", (zlib.crc32(bytes(h)) & 0xFFFF) if fhcrc is None else fhcrc)
    return bytes(h) + body + struct.pack("<II", zlib.crc32(content) if crc is None else crc,
                                         (len(content) & 0xFFFFFFFF) if isize is None else isize)


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = b"", 0
    for f in flush_at:
        out += c.compress(data[at:f]) + c.flush(flush)
        at = f
    return out + c.compress(data[at:]) + c.flush()


def gz(data, **kw):
    return member(raw_deflate(data, **kw), data)


# ---- fixtures ------------------------------------------------------------------------
@functools.lru_cache(None)
def zlib_streams():
    """{name: (member, content)} of what zlib writes: the levels, strategies and
    flushes, the small lengths, two stored blocks, and mixes."""
    out = {}
    mix = rnd(3000, 1) + text(5000, 1) + bytes(4000) + rnd(500, 2) + text(3000, 2) + b"\xff" * 700
    for lv in (0, 1, 6, 9):
        out[f"mix-level{lv}"] = (gz(mix, level=lv), mix)
        out[f"text-level{lv}"] = (gz(text(20000), level=lv), text(20000))
    for nm, stg in (("fixed", zlib.Z_FIXED), ("huffman", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
        out[f"mix-{nm}"] = (gz(mix, strategy=stg), mix)
    out["mix-sync-flush"] = (gz(mix, flush_at=(1000, 1001, 9000)), mix)
    out["mix-full-flush"] = (gz(mix, flush_at=(4000, 12000), flush=zlib.Z_FULL_FLUSH), mix)
    small = rnd(300, 4) + text(700, 4) + bytes(300) + text(300, 4)[::-1]
    for nm, kw in (("level6", {}), ("fixed", dict(strategy=zlib.Z_FIXED)), ("level0", dict(level=0))):
        out[f"small-mix-{nm}"] = (gz(small, **kw), small)
    out["empty"] = (gz(b""), b"")
    r = rnd(70000, 3)
    out["random-70000"] = (gz(r), r)  # does not shrink: two stored blocks
    for n in range(0, 301):
        out[f"zeros-{n}"] = (gz(bytes(n)), bytes(n))
        out[f"text-{n}"] = (gz(text(n, n)), text(n, n))
    return out


def _lit_set(ops, extra=()):
    s = {256} | set(extra)
    for op in ops:
        if isinstance(op, int):
            s.add(op)
        elif isinstance(op[0], int):
            s.add(len_sym(op[0])[0])
    return s


def _dist_set(ops):
    return {dist_sym(op[1])[0] for op in ops if not isinstance(op, int) and isinstance(op[0], int)}


@functools.lru_cache(None)
def handmade():
    """{name: (member, content)}: each named for the structure it holds."""
    out = {}

    def add(name, w, content, **kw):
        out[name] = (member(w.done(), content, **kw), content)

    # every length 3-258, every distance code with extra bits that vary
    base = rnd(32768, 10)
    ops, k = [], 0
    for ln in range(3, 259):
        d = k % 30
        x = (0x1555 * (k + 1)) & ((1 << DIST_EXTRA[d]) - 1)
        ops.append((ln, DIST_BASE[d] + x))
        k += 1
    for d in range(30):  # each code once more at its largest distance
        ops.append((3 + d, DIST_BASE[d] + (1 << DIST_EXTRA[d]) - 1))
    w = BitWriter()
    stored_block(w, base)
    fixed_block(w, ops, final=True)
    add("all-lengths-all-distances", w, base + expand(ops, base))

    ops = [ord("x"), (258, 1)]
    w = BitWriter()
    fixed_block(w, ops, final=True)
    add("258-at-distance-1-from-byte-1", w, expand(ops))

    ops = [(10, 32768), 7, (258, 32768)]
    w = BitWriter()
    stored_block(w, base)
    fixed_block(w, ops, final=True)
    add("distance-32768", w, base + expand(ops, base))

    head = b"stored bytes, then a match into them"
    ops = [ord("!"), (12, len(head) + 1), (5, 3)]
    w = BitWriter()
    stored_block(w, head)
    fixed_block(w, ops, final=True)
    add("fixed-match-into-stored", w, head + expand(ops, head))

    a = rnd(30000, 11)
    ops_b = [(258, 30000)] * 12 + [1, 2, 3, (200, 2)]
    mid = expand(ops_b, a)
    ops_c = [(100, 32768), ord("z"), (258, 1), (40, 20000)]
    syms = _lit_set(ops_c)
    ll = lengths_for(syms, flat_lengths(len(syms)), max(syms) + 1)
    ds = _dist_set(ops_c)
    dl = lengths_for(ds, flat_lengths(len(ds)), max(ds) + 1)
    w = BitWriter()
    stored_block(w, a)
    fixed_block(w, ops_b)
    dynamic_block(w, ll, dl, ops_c, final=True)
    add("three-blocks-beyond-32k", w, a + mid + expand(ops_c, a + mid))

    # lengths 1, 2, ..., 14, 15, 15 on 16 symbols: the last two codes have 15 bits
    syms = list(range(ord("a"), ord("a") + 15)) + [256]
    ll = lengths_for(syms, list(range(1, 16)) + [15], 257)
    ops = [ord("a") + i for i in (14, 0, 13, 14, 1, 12)]   # 'o' and 256 are the 15-bit codes
    w = BitWriter()
    dynamic_block(w, ll, [0], ops, final=True)
    add("15-bit-code", w, expand(ops))

    # 16, 17 and 18, and an 18 run from literal/length 258 into distance 1
    syms = list(range(ord("a"), ord("a") + 14)) + [256, 257]      # 16 symbols of 4 bits
    ll = lengths_for(syms, [4] * 16, 286)
    dl = [0, 0, 1, 1]
    seq = [(18, 97), (4, None), (16, 6), (16, 6), (4, None), (18, 138), (17, 7), (4, None), (4, None),
           (18, 30), (1, None), (1, None)]
    total = []
    for s, x in seq:
        total += [s] if s < 16 else [total[-1]] * x if s == 16 else [0] * x
    assert total == ll + dl
    ops = [ord("a"), ord("b"), ord("c"), (3, 3), ord("n"), (3, 4)]
    w = BitWriter()
    dynamic_block(w, ll, dl, ops, cl_seq=seq, final=True)
    add("repeat-codes-across-the-boundary", w, expand(ops))

    ops = [ord("q"), (7, 1), ord("r"), (3, 1)]
    syms = _lit_set(ops)
    ll = lengths_for(syms, flat_lengths(len(syms)), max(syms) + 1)
    w = BitWriter()
    dynamic_block(w, ll, [1], ops, final=True)
    add("single-distance-code", w, expand(ops))

    ops = list(b"only literals here")
    syms = _lit_set(ops)
    ll = lengths_for(syms, flat_lengths(len(syms)), 257)
    w = BitWriter()
    dynamic_block(w, ll, [0], ops, final=True)
    add("literal-only-hdist-1-length-0", w, expand(ops))

    w = BitWriter()
    stored_block(w, b"")
    fixed_block(w, [ord("e")])
    stored_block(w, b"", final=True)
    add("empty-stored-blocks", w, b"e")

    body = raw_deflate(text(3000, 5))
    for name, kw in {
        "fextra": dict(flg=4, extra=b"AP\x04\x00abcd"),
        "fextra-empty": dict(flg=4),
        "fname": dict(flg=8, name=b"file.txt"),
        "fcomment": dict(flg=16, comment=b"a comment"),
        "fhcrc": dict(flg=2),
        "ftext": dict(flg=1),
        "all-fields": dict(flg=31, extra=b"xy\x01\x00z", name=b"n", comment=b""),
    }.items():
        out["member-" + name] = (member(body, text(3000, 5), **kw), text(3000, 5))
    return out


@functools.lru_cache(None)
def corruptions():
    """{name: (stream, status)}: one named fault each."""
    content = text(2000, 7)
    good = gz(content)
    small = gz(b"thirty bytes or so")
    assert len(small) <= 40
    out = {
        "truncated-in-header": good[:6],
        "truncated-in-block": good[:10 + (len(good) - 18) // 2],
        "truncated-in-trailer": good[:-3],
        "crc-bit": good[:-8] + bytes([good[-8] ^ 4]) + good[-7:],
        "isize-plus-1": member(good[10:-8], content, isize=len(content) + 1),
        "isize-minus-1": member(good[10:-8], content, isize=len(content) - 1),
        "isize-1GiB-in-30-bytes": small[:-4] + struct.pack("<I", 1 << 30),
        "reserved-flg-bit": member(good[10:-8], content, flg=0x20),
        "cm-7": member(good[10:-8], content, cm=7),
        "wrong-fhcrc": member(good[10:-8], content, flg=2, fhcrc=(zlib.crc32(good[:10]) ^ 1) & 0xFFFF),
        "trailing-byte": good + b"\0",
    }
    out = {k: (v, CORRUPT) for k, v in out.items()}
    out["second-member"] = (good + good, UNSUPPORTED)

    def bad(name, w, content=b""):
        out[name] = (member(w.done(), content), CORRUPT)

    w = BitWriter()
    w.bits(1, 1)
    w.bits(3, 2)
    bad("btype-3", w)

    w = BitWriter()
    stored_block(w, b"abcdef", final=True, nlen=0xFFF8)
    bad("len-nlen", w, b"abcdef")

    w = BitWriter()
    fixed_block(w, [ord("a"), (3, 2)], final=True)
    bad("distance-before-start", w, b"aaaa")

    lits = list(b"abcd")
    w = BitWriter()   # three codes of one bit
    dynamic_header(w, lengths_for([97, 98, 256], [1, 1, 1], 257), [0], final=True)
    w.bits(0, 16)
    bad("over-subscribed", w)

    w = BitWriter()   # two codes of two bits
    dynamic_header(w, lengths_for([97, 256], [2, 2], 257), [0], final=True)
    w.bits(0, 16)
    bad("incomplete-literal-length-set", w)

    ll = lengths_for(lits + [256, 257, 258, 259], [3] * 8, 260)
    w = BitWriter()
    dynamic_header(w, ll, [0], cl_seq=[(16, 3)] + plain_cl(ll[3:] + [0]), final=True)
    w.bits(0, 16)
    bad("code-16-first", w)

    w = BitWriter()   # the last run goes 9 past the 261 lengths
    dynamic_header(w, ll, [0], cl_seq=plain_cl(ll[:250]) + [(18, 20)], final=True)
    w.bits(0, 16)
    bad("run-past-hlit-hdist", w)

    w = BitWriter()
    fixed_block(w, [ord("a"), ("sym", 286)], final=True)
    bad("symbol-286", w, b"a")

    w = BitWriter()
    fixed_block(w, [ord("a"), ord("b"), ord("c"), ("dsym", 3, 30)], final=True)
    bad("distance-code-30", w, b"abcabc")

    w = BitWriter()   # a complete set in which 256 has no code
    dynamic_header(w, lengths_for(lits + [257, 258, 259, 260], [3] * 8, 261), [0], final=True)
    w.bits(0, 16)
    bad("no-end-of-block-code", w)
    return out


def recompute_trailer(stream):
    """The stream with the CRC-32 and ISIZE of what its body decodes to under
    zlib's lenient reader (unchanged when that fails)."""
    try:
        h = member_header(stream)
        d = zlib.decompressobj(-15)
        out = d.decompress(stream[h:-8])
        if not d.eof or d.unused_data:
            return stream
    except (Corrupt, zlib.error):
        return stream
    return stream[:-8] + struct.pack("<II", zlib.crc32(out), len(out) & 0xFFFFFFFF)


@functools.lru_cache(None)
def mutations(n=512, seed=21):
    """n single-bit mutations of valid streams; every second one gets the
    trailer of what it now decodes to, so the DEFLATE layer is reached."""
    pool = [zlib_streams()[k][0] for k in ("small-mix-level6", "small-mix-fixed", "small-mix-level0", "text-300",
                                           "text-200", "zeros-300")]
    pool += [handmade()[k][0] for k in ("repeat-codes-across-the-boundary", "15-bit-code", "single-distance-code",
                                        "member-all-fields", "fixed-match-into-stored")]
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = bytearray(pool[i % len(pool)])
        # half of the flips land in the first 96 bytes, where the headers and the code lengths are
        at = int(rng.integers(0, min(len(s), 96))) if rng.integers(0, 2) else int(rng.integers(0, len(s)))
        s[at] ^= 1 << int(rng.integers(0, 8))
        s = bytes(s)
        out.append(recompute_trailer(s) if i % 2 else s)
    return out


@functools.lru_cache(None)
def mutation_refs():
    """status_of every mutation, computed once."""
    return tuple(status_of(m) for m in mutations())


def crc_boundary_contents():
    sizes = list(range(0, 301)) + [65536 + d for d in (-5, -4, -3, -1, 0, 1, 3, 4, 5)] + [(1 << 20) + 1]
    return [rnd(n, 3000 + i) for i, n in enumerate(sizes)]


def stored_member(content):
    w = BitWriter()
    if not content:
        stored_block(w, b"", final=True)
    for p in range(0, len(content), 65535):
        stored_block(w, content[p:p + 65535], final=p + 65535 >= len(content))
    return member(w.done(), content)


def all_streams():
    """Every stream the GPU tests decode (the CPU test runs them through the
    walker under the sanitizers first)."""
    out = [v[0] for v in zlib_streams().values()] + [v[0] for v in handmade().values()]
    out += [v[0] for v in corruptions().values()] + list(mutations())
    out += [stored_member(c) for c in crc_boundary_contents() if len(c) <= 70000]
    return out
