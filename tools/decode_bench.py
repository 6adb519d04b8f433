"""Device Decode throughput beside Encode's, on the chunks of the C1 / C2 / C3
buffers of bench.py: each set is chunked, encoded and decoded in one process,
hipEvents around each call, then decoded again on the host (libcrypto open +
liblz4 inflate on --host-threads threads) as the baseline.  One JSON line per
set and setting:

    python tools/decode_bench.py [--sets c1,c2,c3] [--size-mib 1024] [--reps 3] [--labels lz4+gcm]

With --gzip the sets are the chunks of C1 and C3 and of a text-like buffer,
deflated on the host with zlib at level 6 (the algorithm class of Go's
compress/gzip at its default level), wrapped as gzip members and sealed with
AES-256-GCM; Decode (compressed = "GZIP") is timed the same way, beside
zlib.decompress of the unsealed members on --host-threads threads (it releases
the GIL), and tools/inflate_count.cpp counts the symbols for the cost of one:

    python tools/decode_bench.py --gzip [--sets c1,c3,text] [--size-mib 128] [--reps 3]

k_gz_emit's own time comes from a kernel trace of the same command
(rocprofv3 --kernel-trace --stats -- python tools/decode_bench.py --gzip ...).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def text_like(np, n, seed=7):
    """n bytes of words drawn from a 20,000-word vocabulary with probability 1 / rank."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"etaoinshrdlucmfwypvbgkqjxz", dtype=np.uint8)
    pl = 1.0 / np.arange(4, 30)
    pl /= pl.sum()
    vocab = np.array([letters[rng.choice(26, size=int(k), p=pl)].tobytes() for k in rng.integers(2, 11, size=20000)],
                     dtype=object)
    pw = 1.0 / np.arange(1, 20001)
    pw /= pw.sum()
    out, have = [], 0
    while have < n:
        part = b" ".join(vocab[rng.choice(20000, size=1 << 18, p=pw)]) + b".\n"
        out.append(part)
        have += len(part)
    return b"".join(out)[:n]


def inflate_count(streams):
    """tools/inflate_count.cpp over the members: its JSON line as a dict."""
    import struct
    import subprocess
    import tempfile
    exe = os.path.join(ROOT, "tools", "_bin", "inflate_count")
    src = os.path.join(ROOT, "tools", "inflate_count.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], check=True)
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        for s in streams:
            f.write(struct.pack("<I", len(s)) + s)
        f.flush()
        return json.loads(subprocess.run([exe, f.name], check=True, capture_output=True, text=True).stdout)


def gzip_sets(a):
    import zlib
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np
    import torch

    import bench
    import decode_ref
    import inflate_ref
    from plakar_amd import _lib, chunkers, decode, device
    _lib.ensure_init()
    dev = torch.device("cuda", 0)
    key = os.urandom(32)
    opts = chunkers.ChunkerOpts(65536, 1 << 20, 4 << 20)
    size = a.size_mib << 20
    for name in a.sets.split(","):
        if name == "text":
            buf = torch.from_numpy(np.frombuffer(text_like(np, size), dtype=np.uint8).copy()).to(dev)
        else:
            buf = bench.make_buffers(torch, bench.WORKLOADS[name], 0, dev, size)[0]
        b = device.DeviceBatch([buf], opts)
        b.launch()
        cuts, _ = b.results()
        c = cuts[0].cpu().numpy().astype(np.int64)
        offs, lens = c[:, 0], c[:, 1]
        host = buf.cpu().numpy()
        del b
        plains = [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)]
        with ThreadPoolExecutor(a.host_threads) as pool:
            t0 = time.perf_counter()
            members = list(pool.map(lambda p: inflate_ref.member(inflate_ref.raw_deflate(p, level=6), p), plains))
            deflate_s = time.perf_counter() - t0
            sealed = list(pool.map(lambda im: decode_ref.seal_stream(key, im[1], im[0]), enumerate(members)))
        n = int(lens.sum())
        elens = np.array([len(x) for x in sealed], dtype=np.uint64)
        eoffs = np.concatenate([[0], np.cumsum(elens)[:-1]]).astype(np.uint64)
        enc = torch.from_numpy(np.frombuffer(b"".join(sealed), dtype=np.uint8).copy()).to(dev)
        out = torch.empty(n, dtype=torch.uint8, device=dev)

        def timed(fn):
            fn()  # warm: workspace growth, tables
            best = None
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = fn()
                e1.record()
                e1.synchronize()
                best = e0.elapsed_time(e1) if best is None else min(best, e0.elapsed_time(e1))
            return r, best / 1e3

        (doo, st), dec_s = timed(lambda: decode.decode_device(enc, eoffs, elens, out, key=key, compressed="GZIP"))
        ok = bool((st == 0).all()) and int(doo[-1]) == n and torch.equal(out, buf[:n] if n < buf.numel() else buf)
        counts = inflate_count(members)
        line = dict(set=name, setting="gzip+gcm", deflate="zlib level 6", blobs=len(lens), bytes=n,
                    deflated_bytes=int(sum(len(m) for m in members)), encoded_bytes=int(elens.sum()), reps=a.reps,
                    round_trip_ok=ok, decode_s=dec_s, decode_gibs=n / dec_s / 2**30, host_deflate_s=deflate_s,
                    symbols=counts["literals"] + counts["matches"], **counts)
        if not a.no_host:
            with ThreadPoolExecutor(a.host_threads) as pool:
                t0 = time.perf_counter()
                total = sum(pool.map(lambda m: len(zlib.decompress(m, 31)), members))
                host_s = time.perf_counter() - t0
            assert total == n
            line.update(host_threads=a.host_threads, host_inflate_s=host_s, host_inflate_gibs=n / host_s / 2**30,
                        device_over_host=host_s / dec_s, host_leg="zlib.decompress only (no GCM open)")
        print(json.dumps(line), flush=True)
        del enc, out, buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gzip", action="store_true", help="the GZIP sets (see the module's docstring)")
    ap.add_argument("--sets", default=None)
    ap.add_argument("--size-mib", type=int, default=None,
                    help="bytes per set (C2: split over its 32 buffers); default 1024, with --gzip 128")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--labels", default="lz4+gcm")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    a.sets = a.sets or ("c1,c3,text" if a.gzip else "c1,c2,c3")
    a.size_mib = a.size_mib or (128 if a.gzip else 1024)
    if a.gzip:
        return gzip_sets(a)
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np
    import torch

    import bench
    import crypto_ref
    from plakar_amd import _lib, chunkers, decode, device, encode
    _lib.ensure_init()
    dev = torch.device("cuda", 0)
    key = os.urandom(32)
    opts = chunkers.ChunkerOpts(65536, 1 << 20, 4 << 20)

    def timed(fn):
        fn()  # warm: workspace growth, tables
        best = None
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        return r, best / 1e3

    for name in a.sets.split(","):
        wl = bench.WORKLOADS[name]
        size = (a.size_mib << 20) // wl["nbuf"]
        bufs = bench.make_buffers(torch, wl, 0, dev, size)
        b = device.DeviceBatch(bufs, opts)
        b.launch()
        cuts, _ = b.results()
        base = torch.cat(bufs) if len(bufs) > 1 else bufs[0]
        offs = np.concatenate([c.cpu().numpy().astype(np.int64)[:, 0] + i * size for i, c in enumerate(cuts)])
        lens = np.concatenate([c.cpu().numpy().astype(np.int64)[:, 1] for c in cuts])
        del bufs, b
        n = int(lens.sum())
        for label, k, comp in (("lz4+gcm", key, True), ("lz4", None, True), ("gcm", key, False)):
            if label not in a.labels.split(","):
                continue
            cap = sum(encode.encode_bound(int(x), comp, k is not None) for x in lens)
            enc = torch.empty(cap, dtype=torch.uint8, device=dev)
            oo, enc_s = timed(lambda: encode.encode_device(base, offs, lens, enc, key=k, compress=comp))
            eoffs, elens = oo[:-1], np.diff(oo)
            out = torch.empty(n, dtype=torch.uint8, device=dev)
            (doo, st), dec_s = timed(lambda: decode.decode_device(enc, eoffs, elens, out, key=k, compressed=comp))
            ok = bool((st == 0).all()) and int(doo[-1]) == n and all(
                torch.equal(out[int(doo[i]):int(doo[i + 1])], base[int(offs[i]):int(offs[i]) + int(lens[i])])
                for i in range(0, len(lens), max(1, len(lens) // 16)))
            line = dict(set=name, setting=label, blobs=len(lens), bytes=n, encoded_bytes=int(oo[-1]), reps=a.reps,
                        round_trip_ok=ok, encode_s=enc_s, decode_s=dec_s, encode_gibs=n / enc_s / 2**30,
                        decode_gibs=n / dec_s / 2**30, decode_over_encode=enc_s / dec_s)
            if not a.no_host:
                host = enc[:int(oo[-1])].cpu().numpy()
                blobs = [host[int(eoffs[i]):int(eoffs[i]) + int(elens[i])].tobytes() for i in range(len(lens))]
                with ThreadPoolExecutor(a.host_threads) as pool:
                    t0 = time.perf_counter()
                    total = sum(pool.map(lambda x: len(crypto_ref.decode(x, k, comp)), blobs))
                    host_s = time.perf_counter() - t0
                assert total == n
                line.update(host_threads=a.host_threads, host_decode_s=host_s, host_decode_gibs=n / host_s / 2**30,
                            device_over_host=host_s / dec_s)
            print(json.dumps(line), flush=True)
            del enc, out
        del base


if __name__ == "__main__":
    main()
