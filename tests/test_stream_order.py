"""Every device entry point on a busy non-blocking stream (stream_busy.py).

The rest of the suite pins what each entry point computes, on torch's current
stream, with inputs that were complete long before the call and a device-wide
synchronise after it.  Here the caller's stream is a non-blocking stream that
is still running a delay when the call is made, and the call's real input is
written behind that delay: at the time of the call the input buffers hold a
decoy of zeros.  A kernel or copy issued on another stream, a missing fork or
join event, or a "synchronous" call that drains only a side stream then gives
the decoy's answer, or none.

  A  the answer is the reference's for the real input (every entry point);
  B  a synchronous call has finished when it returns: its outputs are read on
     another stream without synchronising the caller's, its host results are
     final, and the caller's stream is drained;
  C  an asynchronous call returns while the delay still runs, and a consumer
     enqueued on the same stream sees its output;
  D  the assemble ring, the digest descriptor ring and the emit scratch under
     a backlog that is really pending, on one stream and across two;
  E  a call waits only for its own stream;
  F  negative controls: the same harness fails when the call is made on a
     stream other than the one that holds the delayed input write.

Zeros are valid input for Encode, the digests, assemble, the line table, the
zip and gzip pieces and the chunker, and a malformed stream that Decode, the
check and Transcode report and contain.  References: liblz4, libcrypto, zlib,
hashlib, numpy, diff_ref and the C oracle; never another entry point."""
import ctypes
import hashlib
import os
import struct
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import crypto_ref  # noqa: E402
import decode_ref as dr  # noqa: E402
import diff_ref  # noqa: E402
import inflate_ref as ir  # noqa: E402
import stream_busy as sb  # noqa: E402
from datagen import random_bytes  # noqa: E402
from plakar_amd import _lib, archive, chunkers, decode, device, diff, encode, hashing, restore, sync  # noqa: E402
from plakar_amd._lib import CDC_E_MISMATCH  # noqa: E402

pytestmark = pytest.mark.gpu

KEY_A = bytes(range(64, 96))
KEY_B = bytes(range(160, 192))
SENT = 0xA5
SLACK = 4096
SIZES = [0, 1, 1000, 65537, 200000]  # one byte past a 64-KiB GCM piece; several 8-KiB segments and DEFLATE spans
_MASKL_ENV = os.environ.get("CDC_MASKL_INDEX", "1")[:1]
_MASKL_MODE = int(_MASKL_ENV) if _MASKL_ENV in ("0", "1", "2", "3") else 1
V = ctypes.c_void_p
_p64 = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module", autouse=True)
def _init():
    _lib.ensure_init(gear=_lib.default_gear())  # ends with a device-wide synchronise
    sb.calibrate()
    yield
    torch.cuda.synchronize()
    device.set_maskl_index_mode(_MASKL_MODE)


@pytest.fixture(scope="module")
def streams():
    """Non-blocking streams none of which waits for another: with few hardware
    queues two streams may share one, and then run one after the other."""
    ss = sb.independent_streams(4)
    assert len(ss) >= 2, f"no two independent streams among torch's pool ({sb.calibration()})"
    return ss


# ---- the harness ----------------------------------------------------------------------------------------
def _dev(b):
    a = np.frombuffer(bytes(b), dtype=np.uint8).copy() if not isinstance(b, np.ndarray) else np.ascontiguousarray(b)
    if a.size == 0:
        return torch.zeros(1, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a).cuda()


def _outbuf(cap):
    """(the whole sentinel-filled buffer, the capacity's view in its middle)"""
    buf = torch.full((SLACK + cap + SLACK,), SENT, dtype=torch.uint8, device="cuda")
    return buf, buf[SLACK:SLACK + cap]


def _whole(host, body, what=""):
    """The margins, the expected bytes, and nothing after them."""
    assert (host[:SLACK] == SENT).all(), f"{what}: bytes before the output were written"
    got = host[SLACK:SLACK + len(body)].tobytes()
    assert got == bytes(body), f"{what}: the output differs from the reference"
    assert (host[SLACK + len(body):] == SENT).all(), f"{what}: bytes past the output were written"


class Case:
    """One entry point with its real input (`staged`), the decoy it is called
    over (`inp`), sentinel-filled outputs, and the reference's verdict.
    call(inp, stream) -> host results; verify(host outputs, host results)."""

    def __init__(self, staged, outs, call, verify, fill=SENT):
        self.staged = staged
        self.inp = [torch.zeros_like(t) for t in staged]
        self.outs = outs
        self.fill = fill
        self.snap = [torch.empty_like(o) for o in outs]
        self.pinned = [torch.empty(o.shape, dtype=o.dtype, pin_memory=True) for o in outs]
        self._call = call
        self.verify = verify

    def call(self, stream):
        return self._call(self.inp, stream)

    def reset(self):
        for o in self.outs:
            o.view(torch.uint8).fill_(self.fill)
        for t in self.inp:
            t.zero_()
        torch.cuda.synchronize()

    def warm(self, stream):
        """One identical call on the idle stream over the real input: caches grow now."""
        for t, s in zip(self.inp, self.staged):
            t.copy_(s)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            r = self.call(stream)
        torch.cuda.synchronize()
        return r

    def hosts(self):
        return [o.cpu().numpy() for o in self.outs]


def _contents():
    return [ir.rnd(n, 40 + i) if n == 65537 else ir.text(n, 40 + i) for i, n in enumerate(SIZES)]


def _gzip(data):
    if not data:
        return b""  # DeflateStream of empty input is an empty stream
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def _stored(content, compression, key, seed):
    """A blob as a repository with this codec stores it, made by liblz4 / zlib / libcrypto."""
    body = content if compression is None else _gzip(content) if compression == "GZIP" else \
        (dr.lz4f_compress(content) if content else b"")
    return dr.seal_stream(key, body, seed) if key is not None else body


def _read_back(blob, compression, key):
    body = crypto_ref.decrypt_stream(key, blob)[0] if key is not None else blob
    if compression is None or not body:
        return body
    return zlib.decompress(body, 31) if compression == "GZIP" else crypto_ref.lz4f_decompress(body)


def _pack(blobs):
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return _dev(b"".join(blobs) + b"\0"), offs[:-1], lens


def _rnd_rows(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=56 * n, dtype=np.uint8).tobytes()


# ---- synchronous entry points ---------------------------------------------------------------------------
def encode_case(compression, keyed, level):
    contents = _contents()
    base, offs, lens = _pack(contents)
    key = KEY_A if keyed else None
    sel = False if compression is None else True if compression == "LZ4" else "GZIP"
    rnd = _rnd_rows(len(contents), 7)
    cap = sum(encode.encode_bound(len(c), sel, keyed) for c in contents)
    buf, out = _outbuf(cap)

    def call(inp, s):
        return encode.encode_device(inp[0], offs, lens, out, key=key, compress=sel, random=rnd if keyed else None,
                                    stream=s, level=level)

    def verify(hosts, oo):
        (host,) = hosts
        assert oo[0] == 0 and (np.diff(oo) >= 0).all() and oo[-1] <= cap, oo
        body = host[SLACK:SLACK + int(oo[-1])].tobytes()
        for i, c in enumerate(contents):
            enc = body[oo[i]:oo[i + 1]]
            try:  # liblz4 verifies the frame's content checksum, zlib the CRC-32, libcrypto every tag
                got = _read_back(enc, compression, key)
            except (ValueError, zlib.error) as e:
                raise AssertionError(f"blob {i} ({len(c)} bytes) does not read back: {e}") from None
            assert got == c, f"blob {i} ({len(c)} bytes) reads back as other bytes"
        _whole(host, body, "encode")

    return Case([base], [buf], call, verify)


def gzip_piece_case(writer, content, last):
    src = _dev(content)
    cap = archive.gzip_stream_bound(len(content))
    buf, out = _outbuf(cap)

    def call(inp, s):
        return writer.piece_device(inp[0], len(content), out, last=last, stream=s)

    def verify(hosts, n):
        (host,) = hosts
        assert 0 < n <= cap
        _whole(host, host[SLACK:SLACK + n].tobytes(), "gzip piece")

    return Case([src], [buf], call, verify)


def zip_case(level):
    lens = [0, 1, 1000, 65537, 200000]
    shapes = [1, 2, 2]  # pieces per entry
    content, pieces, headers, k = bytearray(), [], bytearray(), 0
    for e, n in enumerate(shapes):
        before = b""
        for j in range(n):
            body = ir.text(lens[k], 60 + k) if k % 2 == 0 else ir.rnd(lens[k], 60 + k)
            p = dict(off=len(content), len=len(body), first=j == 0, last=j == n - 1,
                     crc_reg=zlib.crc32(before) ^ 0xFFFFFFFF, csize_before=1000 * j, usize_before=len(before), body=body)
            if j == 0:
                h = bytes((7 * e + i) & 255 for i in range(31 + e))
                p.update(hdr_off=len(headers), hdr_len=len(h), hdr=h)
                headers += h
            content += body + b"\xEE" * (k % 3)
            before += body
            pieces.append(p)
            k += 1
    src = _dev(bytes(content))
    cap = sum(archive.zip_piece_bound(p["len"], p.get("hdr_len", 0)) for p in pieces)
    buf, out = _outbuf(cap)
    headers = bytes(headers)

    def call(inp, s):
        return archive.zip_pieces_device(inp[0], pieces, headers, out, stream=s, level=level)

    def verify(hosts, res):
        total, outs = res
        (host,) = hosts
        data = host[SLACK:SLACK + total].tobytes()
        at, raw, body = 0, b"", b""
        for p, o in zip(pieces, outs):
            assert o["out_off"] == at
            q = at
            if p["first"]:
                assert data[q:q + p["hdr_len"]] == p["hdr"], "the local header"
                q += p["hdr_len"]
                raw, body = b"", b""
            raw += data[q:q + o["deflate_len"]]
            body += p["body"]
            assert o["crc_reg"] == zlib.crc32(p["body"]) ^ zlib.crc32(bytes(p["len"])), "the piece's CRC register"
            if p["last"]:
                desc = data[q + o["deflate_len"]:q + o["deflate_len"] + 16]
                assert desc == struct.pack("<IIII", 0x08074B50, zlib.crc32(body), p["csize_before"] + o["deflate_len"],
                                           len(body)), "the data descriptor"
                z = zlib.decompressobj(-15)
                assert z.decompress(raw) == body and z.eof and z.unused_data == b"", "the entry does not inflate"
            at += o["out_len"]
        assert at == total
        _whole(host, data, "zip pieces")

    return Case([src], [buf], call, verify)


def decode_case(kind, compression, sealed):
    contents = _contents()
    key = KEY_A if sealed else None
    blobs = [_stored(c, compression, key, 300 + i) for i, c in enumerate(contents)]
    base, offs, lens = _pack(blobs)
    sel = True if compression == "LZ4" else "GZIP"
    n = len(blobs)
    if kind == "decode":
        want = contents
    elif kind == "prefix":
        upto = [0, 1, 500, 65537, 100000]
        want = [c[:u] for c, u in zip(contents, upto)]
    total = sum(len(c) for c in contents) if kind == "check" else sum(len(w) for w in want)
    buf, out = _outbuf(total)
    sums = [hashlib.sha256(c).digest() for c in contents]
    sums[2] = hashlib.sha256(b"another blob").digest()

    def call(inp, s):
        if kind == "decode":
            return decode.decode_device(inp[0], offs, lens, out, key=key, compressed=sel, stream=s)
        if kind == "prefix":
            return decode.decode_prefix_device(inp[0], offs, lens, upto, out, key=key, compressed=sel, stream=s)
        st = np.full(n, 99, dtype=np.int32)
        needed = ctypes.c_uint64(0)
        rc = _lib.lib().cdc_check_device(0, V(inp[0].data_ptr()), offs.ctypes.data_as(_p64), lens.ctypes.data_as(_p64), n,
                                         decode._sel(sel), key, b"".join(sums), V(out.data_ptr()), total,
                                         ctypes.byref(needed), st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                         V(s.cuda_stream))
        return rc, st

    def verify(hosts, res):
        (host,) = hosts
        if kind == "check":
            rc, st = res
            assert rc == 0, rc
            assert st.tolist() == [0, 0, CDC_E_MISMATCH, 0, 0], st
            assert (host[:SLACK] == SENT).all() and (host[SLACK + total:] == SENT).all(), "bytes outside the scratch"
            return
        oo, st = res
        assert st.tolist() == [0] * n, st
        assert oo.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist(), "out_offsets"
        _whole(host, b"".join(want), kind)

    return Case([base], [buf], call, verify)


def transcode_case(kind):
    contents = _contents()
    if kind == "rekey":
        src, dst, level = (KEY_A, "LZ4"), (KEY_B, "LZ4"), 0
        cap = None
    else:
        src, dst, level = (None, "LZ4"), (KEY_B, "GZIP"), 1
        cap = sum(encode.encode_bound(len(c), "GZIP", True) for c in contents)
    blobs = [_stored(c, src[1], src[0], 500 + i) for i, c in enumerate(contents)]
    base, offs, lens = _pack(blobs)
    cap = cap or int(lens.sum()) + 333
    buf, out = _outbuf(cap)
    rnd = _rnd_rows(len(blobs), 11)
    sums = [hashlib.sha256(c).digest() for c in contents]

    def call(inp, s):
        return sync.transcode_device(inp[0], offs, lens, out, src=src, dst=dst, checksums=None if kind == "rekey" else sums,
                                     random=rnd, stream=s, level=level)

    def verify(hosts, res):
        oo, st = res
        (host,) = hosts
        assert st.tolist() == [0] * len(blobs), st
        body = host[SLACK:SLACK + int(oo[-1])].tobytes()
        for i, c in enumerate(contents):
            g = body[oo[i]:oo[i + 1]]
            if kind == "rekey":
                assert len(g) == len(blobs[i])
            try:
                got = _read_back(g, dst[1], dst[0])
            except (ValueError, zlib.error) as e:
                raise AssertionError(f"blob {i} does not read back: {e}") from None
            assert got == c, f"blob {i} reads back as other bytes"
        _whole(host, body, "transcode")

    return Case([base], [buf], call, verify)


def object_digests_case():
    data = ir.rnd(200000, 70)
    objects = [[(0, 0)], [(5, 1)], [(100, 1000), (7, 64), (7, 64)], [(1000, 65537)], [(0, 200000)], [], [(199999, 1), (0, 63)]]
    seg0 = np.zeros(len(objects) + 1, dtype=np.uint64)
    flat = []
    for i, segs in enumerate(objects):
        flat.extend(segs)
        seg0[i + 1] = len(flat)
    seg = np.asarray(flat, dtype=np.uint64).reshape(-1, 2)
    off, ln = np.ascontiguousarray(seg[:, 0]), np.ascontiguousarray(seg[:, 1])
    buf, out = _outbuf(32 * len(objects))
    src = _dev(data)
    want = b"".join(hashlib.sha256(b"".join(data[o:o + n] for o, n in segs)).digest() for segs in objects)

    def call(inp, s):
        return _lib.lib().cdc_object_digests_device(0, V(inp[0].data_ptr()), len(data), off.ctypes.data_as(_p64),
                                                    ln.ctypes.data_as(_p64), len(off), seg0.ctypes.data_as(_p64),
                                                    len(objects), V(out.data_ptr()), V(s.cuda_stream))

    def verify(hosts, rc):
        assert rc == 0, rc
        _whole(hosts[0], want, "object digests")

    return Case([src], [buf], call, verify)


def _texts():
    """Two texts of a few KiB in one buffer: repeated lines, empty lines, one line past the 4,096-byte threshold."""
    rng = np.random.default_rng(81)
    long_line = bytes(rng.integers(11, 256, 5000, dtype=np.uint8))
    lines = [b"line %d of the text" % (i % 23) for i in range(120)] + [b"", long_line, b"", long_line[:-1] + b"\x0b"]
    a = b"\n".join(lines)
    b = b"\n".join(lines[40:] + [b"a new line", long_line] + lines[:30])
    buf = b"\xEE" * 3 + a + b"\xEE" * 5 + b
    return buf, [(3, len(a)), (3 + len(a) + 5, len(b))]


def line_table_case():
    data, texts = _texts()
    want, counts = [], []
    for o, n in texts:
        r = diff_ref.line_records(data[o:o + n], o)
        want.extend(r)
        counts.append(len(r))
    cap = len(want)
    buf, out = _outbuf(32 * cap)
    src = _dev(data)
    t = np.asarray(texts, dtype=np.uint64)
    toff, tlen = np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1])

    def call(inp, s):
        cnt = np.full(len(texts), 99, dtype=np.uint64)
        total = ctypes.c_uint64(99)
        rc = _lib.lib().cdc_line_table_device(0, V(inp[0].data_ptr()), len(data), toff.ctypes.data_as(_p64),
                                              tlen.ctypes.data_as(_p64), len(texts), V(out.data_ptr()), cap,
                                              cnt.ctypes.data_as(_p64), ctypes.byref(total), V(s.cuda_stream))
        return rc, cnt, int(total.value)

    def verify(hosts, res):
        rc, cnt, total = res
        (host,) = hosts
        assert rc == 0 and cnt.tolist() == counts and total == cap, (rc, cnt, total)
        assert (host[:SLACK] == SENT).all() and (host[SLACK + 32 * cap:] == SENT).all(), "bytes outside the records"
        r = host[SLACK:SLACK + 32 * cap].view(diff.LINE_DTYPE).reshape(-1)
        assert r["off"].tolist() == [o for o, _ in want] and r["len"].tolist() == [n for _, n in want]
        assert not r["reserved"].any()
        by_line = {}
        for (o, n), h in zip(want, r["hash"].tolist()):
            assert by_line.setdefault(data[o:o + n], h) == h, "equal lines with different hashes"

    return Case([src], [buf], call, verify)


def line_ids_case(stream):
    """hash_bits = 4: nearly every line meets a candidate with other bytes, so
    the ids depend on the comparison of the bytes on the device."""
    table = line_table_case()
    table.warm(stream)
    cap = table.outs[0].numel() // 32 - 2 * SLACK // 32
    recs = table.outs[0].cpu().numpy()[SLACK:SLACK + 32 * cap].view(diff.LINE_DTYPE).reshape(-1).copy()
    data, texts = _texts()
    lines = [data[int(r["off"]):int(r["off"]) + int(r["len"])] for r in recs]
    na = len(diff_ref.line_records(data[texts[0][0]:texts[0][0] + texts[0][1]]))
    groups = [0, len(lines)]
    want = diff_ref.first_ids(lines)
    assert want[na:] != list(range(na, len(lines))), "the second text repeats lines of the first"
    src = _dev(data)

    def call(inp, s):
        return diff.line_ids_device(inp[0], recs, groups, hash_bits=4, stream=s)

    def verify(hosts, res):
        ids, rounds = res
        assert ids.tolist() == want
        assert rounds >= 1

    return Case([src], [], call, verify)


def _cut_lists():
    """(data, cut list) of three buffers: empty and one-byte chunks, one past 64 KiB, gaps and an overlap."""
    out = []
    for k, n in enumerate((200000, 65537, 1000)):
        b = random_bytes(n, 900 + k)
        cuts, o = [(0, 0), (0, 1)], 1
        while o < n:
            m = min(n - o, 70000 if o == 1 and n > 100000 else 100 + (o * 2654435761 + k) % 9000)
            cuts.append((o, m))
            o += m + (k == 1)
        cuts.append((n // 2, min(64, n - n // 2)))
        out.append((b, cuts))
    return out


def _digest_check(hosts, lists):
    dig, hist = hosts
    want_d, want_h = bytearray(), []
    for b, cuts in lists:
        for o, n in cuts:
            piece = b[o:o + n]
            want_d += hashlib.sha256(piece.tobytes()).digest()
            want_h.append(np.bincount(piece, minlength=256).astype("<u4"))
    _whole(dig, want_d, "digests")
    _whole(hist, np.concatenate(want_h).tobytes(), "histograms")


def digests_case(form, nbufs=3, host_threads=4, host_min_len=1):
    """form: "one" (cdc_chunk_digests_device_async), "batch" or "hybrid"."""
    lists = _cut_lists()[:1 if form == "one" else nbufs]
    datas = [_dev(b) for b, _ in lists]
    cls = [torch.tensor(np.asarray(c, np.int64).reshape(-1, 2), device="cuda") for _, c in lists]
    counts = [len(c) for _, c in lists]
    total = sum(counts)
    dbuf, dig = _outbuf(32 * total)
    hbuf, hist = _outbuf(1024 * total)
    base = np.concatenate([[0], np.cumsum(counts)])
    n = len(lists)
    lens = (ctypes.c_uint64 * n)(*[len(b) for b, _ in lists])
    caps = (ctypes.c_uint64 * n)(*counts)
    cutp = (V * n)(*[c.data_ptr() for c in cls])
    digp = (V * n)(*[dig.data_ptr() + 32 * int(base[i]) for i in range(n)])
    histp = (V * n)(*[hist.data_ptr() + 1024 * int(base[i]) for i in range(n)])
    L = _lib.lib()

    def call(inp, s):
        datap = (V * n)(*[t.data_ptr() for t in inp])
        if form == "one":
            return L.cdc_chunk_digests_device_async(0, datap[0], lens[0], cutp[0], counts[0], None, digp[0], histp[0],
                                                    V(s.cuda_stream))
        if form == "batch":
            return L.cdc_chunk_digests_device_batch_async(0, datap, lens, n, cutp, caps, None, digp, histp, V(s.cuda_stream))
        hc = ctypes.c_uint64(0)
        rc = L.cdc_chunk_digests_hybrid(0, datap, lens, n, cutp, caps, None, digp, histp, host_threads, host_min_len,
                                        V(s.cuda_stream), ctypes.byref(hc), None)
        return rc, int(hc.value)

    def verify(hosts, res):
        if form == "hybrid":
            rc, hc = res
            assert rc == 0 and hc == (sum(1 for _, c in lists for _, m in c if m) if host_threads else 0), res
        else:
            assert res == 0, res
        _digest_check(hosts, lists)

    return Case(datas, [dbuf, hbuf], call, verify)


# ---- asynchronous entry points --------------------------------------------------------------------------
def assemble_case(nseg=300, seed=7, inp=None):
    rng = np.random.default_rng(seed)
    src_np = random_bytes(1 << 16, 78)
    lens = rng.integers(1, 65, nseg)
    so = rng.integers(0, src_np.size - 64, nseg)
    do = np.cumsum(lens + rng.integers(0, 3, nseg)) - lens
    size = int(do[-1] + lens[-1]) + 16
    segs = [(int(s), int(n), int(d)) for s, n, d in zip(so, lens, do)]
    want = np.full(size, SENT, np.uint8)
    for s, n, d in segs:
        want[d:d + n] = src_np[s:s + n]
    buf, dst = _outbuf(size)

    def call(inp_, s):
        return restore.assemble_device(inp_[0], segs, dst, stream=s)

    def verify(hosts, _):
        _whole(hosts[0], want.tobytes(), "assemble")

    c = Case([_dev(src_np)], [buf], call, verify)
    if inp is not None:  # a sequence shares one gated source
        c.inp = inp
    return c


PLAIN_LEN, LIT_LEN = 65536 + 77, 3000
P_, L_, N_ = diff_ref.PREFIX, diff_ref.LITERAL, diff_ref.NEWLINE


def _emit_sources():
    rng = np.random.default_rng(21)
    return rng.integers(0, 256, PLAIN_LEN, dtype=np.uint8).tobytes(), rng.integers(0, 256, LIT_LEN, dtype=np.uint8).tobytes()


def emit_case(nrec, seed, lit_dev, inp=None):
    """nrec records: short prefixed lines, a literal every tenth, a record of
    2 KiB or more (16-KiB pieces of 16-byte stores) every 97th."""
    plain, lit = _emit_sources()
    rng = np.random.default_rng(seed)
    i = np.arange(nrec)
    long, lits = i % 97 == 50, (i % 10 == 9) & (i % 97 != 50)
    ln = np.where(long, rng.integers(2048, 5000, nrec), np.where(lits, rng.integers(0, 40, nrec), rng.integers(0, 121, nrec)))
    flags = np.where(long, N_, np.where(lits, L_, P_ | N_ | rng.choice([32, 43, 45], nrec)))
    room = np.where(lits, LIT_LEN, PLAIN_LEN) - ln + 1
    step = ln + ((flags & P_) != 0) + ((flags & N_) != 0) + rng.integers(0, 3, nrec)  # a gap of 0-2 bytes after each
    recs = np.zeros(nrec, dtype=diff.EMIT_DTYPE)
    recs["src_off"] = (rng.random(nrec) * room).astype(np.uint64)
    recs["dst_off"] = int(rng.integers(0, 16)) + np.cumsum(step) - step
    recs["len"], recs["flags"] = ln, flags
    size = int(recs["dst_off"][-1] + step[-1]) + 64
    want = bytes(diff_ref.execute(recs, plain, lit, size, SENT))
    buf, dst = _outbuf(size)

    def call(inp_, s):
        return diff.diff_emit_device(inp_[0], lit_dev, recs, dst, stream=s)

    def verify(hosts, _):
        _whole(hosts[0], want, f"emit of {nrec} records")

    c = Case([_dev(plain)], [buf], call, verify)
    if inp is not None:
        c.inp = inp
    return c


def chunker_case(mode, oracle):
    device.set_maskl_index_mode(mode)
    data = random_bytes(65536, 55)
    data[20000:30000] = 0  # a run the MaskL stage cuts at max_size
    src = _dev(data)
    want = oracle.chunk(data, _lib.default_gear(), min_size=64, normal_size=256, max_size=1024)
    holder = {}

    def make(inp):
        holder["b"] = device.DeviceBatch([inp[0]], chunkers.ChunkerOpts(MinSize=64, NormalSize=256, MaxSize=1024))
        return holder["b"]

    c = Case([src], [], lambda inp, s: holder["b"].launch(s), None, fill=0)
    b = make(c.inp)
    c.outs = [b.cuts[0], b.res]
    c.snap = [torch.empty_like(o) for o in c.outs]
    c.pinned = [torch.empty(o.shape, dtype=o.dtype, pin_memory=True) for o in c.outs]

    def verify(hosts, _):
        cuts, res = hosts
        ncuts, _consumed, status, _needed = (int(x) for x in res[0])
        assert status == 0, res
        assert ncuts == want.shape[0], f"{ncuts} chunks, the oracle has {want.shape[0]}"
        got = cuts[:ncuts].astype(np.uint64)
        got[:, 1] &= 0xFFFFFFFF
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, f"first mismatch at chunk {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"

    c.verify = verify
    return c


def entropy_case():
    rows = []
    for n in (1, 255, 4096, 65537, 200000):
        rows.append(np.bincount(random_bytes(n, n).astype(np.int64), minlength=256))
        rows.append(np.bincount(np.frombuffer(ir.text(n, n), dtype=np.uint8).astype(np.int64), minlength=256))
    rows.append(np.zeros(256, np.int64))
    rows = np.stack(rows)
    want = hashing.entropy_rows(rows, rows.sum(1))
    assert (want[:-1] > 0).sum() >= 8
    hist = torch.from_numpy(rows.astype(np.int32)).cuda()
    buf, out = _outbuf(8 * len(rows))

    def call(inp, s):
        return _lib.lib().cdc_chunk_entropy_device_async(0, V(inp[0].data_ptr()), len(rows), V(out.data_ptr()),
                                                         V(s.cuda_stream))

    def verify(hosts, rc):
        assert rc == 0
        (host,) = hosts
        assert (host[:SLACK] == SENT).all() and (host[SLACK + 8 * len(rows):] == SENT).all(), "bytes outside the rows"
        got = host[SLACK:SLACK + 8 * len(rows)].view("<f8")
        bad = np.nonzero(got != want)[0]  # equal floats, as test_entropy.py holds them (a zero of either sign)
        assert bad.size == 0, f"{bad.size} rows differ, first {bad[:5]}: {got[bad[:5]]} vs {want[bad[:5]]}"

    return Case([hist], [buf], call, verify)


# ---- A and B: synchronous entry points ------------------------------------------------------------------
def _sync_run(case, streams, lane=0):
    """A and B for one synchronous call: the caller's stream is never
    synchronised by the test before the outputs are read on another stream."""
    s, other = streams[lane % len(streams)], streams[(lane + 1) % len(streams)]
    try:
        case.warm(s)
        case.reset()
        res, gate = sb.run_busy(lambda st: case.call(st), s, case.staged, case.inp)
        early = [h.copy() for h in sb.fetch_via(case.outs, case.pinned, other)]
        drained = not gate.pending()
        case.verify(early, res)  # B: outputs and host results are final at the return
        assert drained, f"the call returned before its stream reached the call's work ({sb.calibration()})"
        torch.cuda.synchronize()
        case.verify(case.hosts(), res)  # A: and nothing changed them afterwards
    finally:
        torch.cuda.synchronize()


@pytest.mark.parametrize("keyed", [False, True], ids=["plain", "sealed"])
@pytest.mark.parametrize("compression,level", [(None, 0), (None, 1), ("LZ4", 0), ("LZ4", 1), ("GZIP", 0), ("GZIP", 1)])
def test_encode_device(streams, compression, level, keyed):
    _sync_run(encode_case(compression, keyed, level), streams)


@pytest.mark.parametrize("lane", [1, 2, 3])
def test_encode_lz4_checksum_fork_on_every_stream(streams, lane):
    """The LZ4 frames' content checksums (k_xxh32) run on a side stream of the
    library's between a fork and a join event.  A side stream that shares the
    caller's hardware queue runs behind the caller's work with or without the
    fork, so the LZ4 case runs on each of the independent streams (lane 0 is
    test_encode_device's): the side stream shares a queue with one at most."""
    _sync_run(encode_case("LZ4", lane % 2 == 0, 0), streams, lane)


def test_gzip_stream_two_pieces(streams):
    first, second = ir.text(200000, 91), ir.rnd(65537, 92)
    s, other = streams[0], streams[1]
    try:
        with archive.GzipStream(level=0) as w:  # another writer warms what the writers share
            for c, last in ((first, False), (second, True)):
                gzip_piece_case(w, c, last).warm(s)
        member = b""
        with archive.GzipStream(level=0) as w:
            for c, last in ((first, False), (second, True)):
                case = gzip_piece_case(w, c, last)
                torch.cuda.synchronize()
                n, gate = sb.run_busy(lambda st: case.call(st), s, case.staged, case.inp)
                (early,) = sb.fetch_via(case.outs, case.pinned, other)
                early = early.copy()
                assert not gate.pending(), f"the piece returned before its stream was drained ({sb.calibration()})"
                case.verify([early], n)
                member += early[SLACK:SLACK + n].tobytes()
                torch.cuda.synchronize()
                case.verify(case.hosts(), n)
        z = zlib.decompressobj(31)
        got = z.decompress(member)
        assert z.eof and z.unused_data == b"" and got == first + second, "the member does not inflate to the pieces"
    finally:
        torch.cuda.synchronize()


@pytest.mark.parametrize("level", [0, 1])
def test_zip_pieces_device(streams, level):
    _sync_run(zip_case(level), streams)


@pytest.mark.parametrize("sealed", [False, True], ids=["plain", "sealed"])
@pytest.mark.parametrize("compression", ["LZ4", "GZIP"])
@pytest.mark.parametrize("kind", ["decode", "prefix", "check"])
def test_decode_prefix_and_check(streams, kind, compression, sealed):
    _sync_run(decode_case(kind, compression, sealed), streams)


@pytest.mark.parametrize("kind", ["rekey", "recompress"])
def test_transcode_device(streams, kind):
    _sync_run(transcode_case(kind), streams)


def test_object_digests_device(streams):
    _sync_run(object_digests_case(), streams)


def test_line_table_device(streams):
    _sync_run(line_table_case(), streams)


def test_line_ids_device(streams):
    try:
        case = line_ids_case(streams[0])
    finally:
        torch.cuda.synchronize()
    _sync_run(case, streams)


@pytest.mark.parametrize("host_threads", [4, 0], ids=["host-share", "all-on-device"])
def test_chunk_digests_hybrid(streams, host_threads):
    _sync_run(digests_case("hybrid", host_threads=host_threads), streams)


# ---- A and C: asynchronous entry points -----------------------------------------------------------------
def _async_run(case, streams):
    s = streams[0]
    try:
        case.warm(s)
        case.reset()
        res, gate = sb.run_busy(lambda st: case.call(st), s, case.staged, case.inp)
        still = gate.pending()
        with torch.cuda.stream(s):  # a consumer on the same stream, nothing in between
            for snap, o in zip(case.snap, case.outs):
                snap.copy_(o, non_blocking=True)
        s.synchronize()
        assert still, f"the call did not return while its stream was busy: it is not asynchronous ({sb.calibration()})"
        case.verify([t.cpu().numpy() for t in case.snap], res)
    finally:
        torch.cuda.synchronize()


def test_assemble_device(streams):
    _async_run(assemble_case(), streams)


def test_diff_emit_device(streams):
    _async_run(emit_case(400, 5, _dev(_emit_sources()[1])), streams)


@pytest.mark.parametrize("mode", [0, 2, 3], ids=["k_scan", "maskl-fused", "maskl-own-pass"])
def test_device_batch_launch(streams, oracle, mode):
    try:
        _async_run(chunker_case(mode, oracle), streams)
    finally:
        device.set_maskl_index_mode(_MASKL_MODE)


@pytest.mark.parametrize("form", ["one", "batch"])
def test_chunk_digests(streams, form):
    _async_run(digests_case(form), streams)


def test_chunk_entropy_device(streams):
    _async_run(entropy_case(), streams)


# ---- D: the rings and the emit scratch under a backlog --------------------------------------------------
def _sequence(make_cases, streams, nstreams):
    """The cases' calls one after the other behind one delay per stream,
    call i on stream i % nstreams; each stream has its own gated source."""
    ss = streams[:nstreams]
    try:
        cases, staged, inps = make_cases(nstreams)
        torch.cuda.synchronize()
        gates = []
        for s, inp in zip(ss, inps):  # the delay and the input write on every stream, then the calls
            sb.busy(s)
            with torch.cuda.stream(s):
                inp.copy_(staged, non_blocking=True)
            gates.append(sb.Gate(s))
        assert all(g.pending() for g in gates), f"premise: the input writes are pending ({sb.calibration()})"
        for i, c in enumerate(cases):
            with torch.cuda.stream(ss[i % nstreams]):
                c.call(ss[i % nstreams])
        for s in ss:
            s.synchronize()
        for i, c in enumerate(cases):
            try:
                c.verify(c.hosts(), None)
            except AssertionError as e:
                raise AssertionError(f"call {i}: {e}") from None
    finally:
        torch.cuda.synchronize()


def _assemble_cases(nstreams, sizes=(10, 3000, 10, 3000, 10, 10)):
    staged = _dev(random_bytes(1 << 16, 78))
    inps = [torch.zeros_like(staged) for _ in range(nstreams)]
    return [assemble_case(n, 100 + i, [inps[i % nstreams]]) for i, n in enumerate(sizes)], staged, inps


def _emit_cases(sizes):
    def make(nstreams):
        staged = _dev(_emit_sources()[0])
        lit = _dev(_emit_sources()[1])
        inps = [torch.zeros_like(staged) for _ in range(nstreams)]
        return [emit_case(n, 200 + i, lit, [inps[i % nstreams]]) for i, n in enumerate(sizes)], staged, inps
    return make


@pytest.mark.parametrize("nstreams", [1, 2], ids=["one-stream", "two-streams"])
def test_assemble_ring_under_backlog(streams, nstreams):
    """Six calls over the four-slot ring: the fifth and sixth wait for slots
    whose launches are still behind the delay (on two streams, the other's)."""
    _sequence(_assemble_cases, streams, nstreams)


@pytest.mark.parametrize("nstreams", [1, 2], ids=["one-stream", "two-streams"])
@pytest.mark.parametrize("larger", [True, False], ids=["larger-second", "equal"])
def test_emit_scratch_under_backlog(streams, larger, nstreams):
    """Three calls over the single emit scratch.  A larger second plan makes the
    grow-only scratch grow while the first launch, which reads it, is still
    pending: 40,000 records (about 1 MB of tables), four times the largest plan
    the suite executes before this file, and twice that on two streams, which
    runs second."""
    _sequence(_emit_cases((300, 40000 * nstreams if larger else 300, 300)), streams, nstreams)


def test_digest_descriptor_ring_under_backlog(streams):
    """Twenty calls of 40 buffers each (past 32 buffers the descriptors are read
    from device memory) over the 16-slot descriptor ring, behind one delay."""
    s = streams[0]
    nb, ncalls = 40, 20
    try:
        rng = np.random.default_rng(12)
        data = random_bytes(nb * 2048, 13)
        staged = _dev(data)
        inp = torch.zeros_like(staged)
        calls = []
        L = _lib.lib()
        for k in range(ncalls):
            cuts = []
            for b in range(nb):
                n0 = int(rng.integers(0, 1024))
                cuts.append([(0, n0), (n0, 2048 - n0 - int(rng.integers(0, 3)))])
            cl = torch.tensor(np.asarray(cuts, np.int64).reshape(-1, 2), device="cuda")
            dbuf, dig = _outbuf(32 * 2 * nb)
            hbuf, hist = _outbuf(1024 * 2 * nb)
            args = ((V * nb)(*[inp.data_ptr() + 2048 * b for b in range(nb)]), (ctypes.c_uint64 * nb)(*[2048] * nb), nb,
                    (V * nb)(*[cl.data_ptr() + 32 * b for b in range(nb)]), (ctypes.c_uint64 * nb)(*[2] * nb), None,
                    (V * nb)(*[dig.data_ptr() + 64 * b for b in range(nb)]),
                    (V * nb)(*[hist.data_ptr() + 2048 * b for b in range(nb)]))
            calls.append((cuts, cl, dbuf, hbuf, args))
        torch.cuda.synchronize()
        sb.busy(s)
        with torch.cuda.stream(s):
            inp.copy_(staged, non_blocking=True)
        gate = sb.Gate(s)
        assert gate.pending(), f"premise: the input write is pending ({sb.calibration()})"
        for _, _, _, _, args in calls:
            assert L.cdc_chunk_digests_device_batch_async(0, *args, V(s.cuda_stream)) == 0
        s.synchronize()
        for k, (cuts, _, dbuf, hbuf, _) in enumerate(calls):
            lists = [(data[2048 * b:2048 * (b + 1)], cuts[b]) for b in range(nb)]
            try:
                _digest_check([dbuf.cpu().numpy(), hbuf.cpu().numpy()], lists)
            except AssertionError as e:
                raise AssertionError(f"call {k}: {e}") from None
    finally:
        torch.cuda.synchronize()


# ---- E: a call waits only for its own stream ------------------------------------------------------------
E_CASES = {
    "encode_device": lambda oracle: encode_case("LZ4", True, 0),
    "decode_device": lambda oracle: decode_case("decode", "LZ4", True),
    "transcode_device": lambda oracle: transcode_case("recompress"),
    "assemble_device": lambda oracle: assemble_case(),
    "chunk_digests_batch": lambda oracle: digests_case("batch"),
    "DeviceBatch.launch": lambda oracle: chunker_case(_MASKL_MODE, oracle),
}


@pytest.mark.parametrize("name", sorted(E_CASES))
def test_call_waits_only_for_its_own_stream(streams, oracle, name):
    """The delay (four times the default) runs on another stream u; the call
    and a synchronise of its own idle stream s must leave u's event pending: a
    device-wide synchronise, a free or a wait for every stream inside the call
    would have drained it.  Streams that share a hardware queue (there are 4 by
    default) wait for each other whatever the library does, the library's own
    side streams included, so u is taken in turn from the independent streams:
    a call that drains the device leaves none of them pending."""
    s, us = streams[0], streams[1:]
    try:
        case = E_CASES[name](oracle)
        case.warm(s)
        pending = False
        for u in us:
            case.reset()
            for t, st in zip(case.inp, case.staged):
                t.copy_(st)
            torch.cuda.synchronize()
            sb.busy(u, 4 * sb.DEFAULT_MS)
            ev = sb.Gate(u)
            assert ev.pending(), f"premise: the delay on the other stream runs ({sb.calibration()})"
            with torch.cuda.stream(s):
                res = case.call(s)
            s.synchronize()
            pending = ev.pending()
            torch.cuda.synchronize()
            case.verify(case.hosts(), res)
            if pending:
                break
        assert pending, (f"{name} and a synchronise of its stream outlasted a {4 * sb.DEFAULT_MS:.0f}-ms delay on each "
                         f"of {len(us)} other streams ({sb.calibration()})")
    finally:
        torch.cuda.synchronize()
        device.set_maskl_index_mode(_MASKL_MODE)


# ---- F: the harness can fail ----------------------------------------------------------------------------
F_CASES = {
    "encode_device": lambda: encode_case("LZ4", False, 0),
    "assemble_device": lambda: assemble_case(),
    "decode_device": lambda: decode_case("decode", "LZ4", False),
}


@pytest.mark.parametrize("name", sorted(F_CASES))
def test_negative_control_call_on_another_stream(streams, name):
    """The same run_busy, the call made on an idle stream other than the one
    that holds the delayed input write: it sees the decoy (zeros; for Decode a
    stream the library reports as corrupt), and the comparison must raise."""
    s, t = streams[0], streams[1]
    try:
        case = F_CASES[name]()
        case.warm(t)
        case.reset()
        res, _ = sb.run_busy(lambda st: case.call(st), s, case.staged, case.inp, call_stream=t)
        # (no premise on the gate here: a side stream of the library's that shares a hardware
        # queue with s makes the call outlast the delay, and it still reads the decoy on t)
        t.synchronize()
        s.synchronize()
        with pytest.raises(AssertionError):
            case.verify(case.hosts(), res)
    finally:
        torch.cuda.synchronize()
