"""Device Encode throughput (LZ4 frame + AES-256-GCM stream) on chunked
buffers: python tools/encode_bench.py [--size-mib 1024] [--reps 5]

With --gzip the sets are the chunks of C1 and C3 of bench.py and of the
text-like buffer of tools/decode_bench.py --gzip: GZIP Encode (gzip member,
with and without the GCM stream) and LZ4 Encode of the same chunks in one
process, hipEvents around each call, the device members decoded again on the
device (the round trip), and zlib.compress at level 6 of the same chunks on
--host-threads threads (it releases the GIL) for the host's speed and size.
One JSON line per set:

    python tools/encode_bench.py --gzip [--sets c1,c3,text] [--size-mib 128] [--reps 3]

With --level 1 every label runs at both levels in the same process (level 1:
the match search with a 32-KiB window, k_lz_seq_wide): the level-1 figures
carry the suffix _l1, the round trip is checked at both levels, and liblz4's
block size of the same chunks stands beside zlib's.  With --level 9 all
three levels run (level 9: four candidates per bucket and a lazy parse,
k_lz_seq_deep), its figures with the suffix _l9.

Per-kernel times come from a kernel trace of the same command
(rocprofv3 --kernel-trace --stats -- python tools/encode_bench.py --gzip ...).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def gzip_sets(a):
    import zlib
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np
    import torch

    import bench
    import decode_bench
    from plakar_amd import _lib, chunkers, decode, device, encode
    _lib.ensure_init()
    dev = torch.device("cuda", 0)
    key = os.urandom(32)
    opts = chunkers.ChunkerOpts(65536, 1 << 20, 4 << 20)
    size = (a.size_mib or 128) << 20

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

    levels = {0: (0,), 1: (0, 1), 9: (0, 1, 9)}[a.level]
    for name in a.sets.split(","):
        if name == "text":
            buf = torch.from_numpy(np.frombuffer(decode_bench.text_like(np, size), dtype=np.uint8).copy()).to(dev)
        else:
            buf = bench.make_buffers(torch, bench.WORKLOADS[name], 0, dev, size)[0]
        b = device.DeviceBatch([buf], opts)
        b.launch()
        cuts, _ = b.results()
        c = cuts[0].cpu().numpy().astype(np.int64)
        offs, lens = c[:, 0].copy(), c[:, 1].copy()
        del b
        n = int(lens.sum())
        line = dict(set=name, blobs=len(lens), bytes=n, reps=a.reps)
        for label, k, comp in (("gzip+gcm", key, "GZIP"), ("gzip", None, "GZIP"), ("lz4+gcm", key, True),
                               ("lz4", None, True)):
            if a.labels and label not in a.labels.split(","):
                continue
            cap = sum(encode.encode_bound(int(x), comp, k is not None) for x in lens)
            enc = torch.empty(cap, dtype=torch.uint8, device=dev)
            for lv in levels:
                oo, enc_s = timed(lambda: encode.encode_device(buf, offs, lens, enc, key=k, compress=comp, level=lv))
                tag = label.replace("+", "_") + (f"_l{lv}" if lv else "")
                line.update({f"{tag}_s": enc_s, f"{tag}_gibs": n / enc_s / 2**30, f"{tag}_bytes": int(oo[-1])})
                if label in ("gzip+gcm", "lz4+gcm") and (lv or label == "gzip+gcm"):  # the round trip, on the device
                    out = torch.empty(n, dtype=torch.uint8, device=dev)
                    doo, st = decode.decode_device(enc, oo[:-1], np.diff(oo), out, key=k, compressed=comp)
                    ok = bool((st == 0).all()) and int(doo[-1]) == n and all(
                        torch.equal(out[int(doo[i]):int(doo[i + 1])], buf[int(offs[i]):int(offs[i]) + int(lens[i])])
                        for i in range(len(lens)))
                    line["round_trip_ok" if label == "gzip+gcm" and not lv else f"{tag}_round_trip_ok"] = ok
                    del out
            del enc
        if not a.no_host:
            host = buf.cpu().numpy()
            plains = [host[int(o):int(o) + int(x)].tobytes() for o, x in zip(offs, lens)]
            with ThreadPoolExecutor(a.host_threads) as pool:
                t0 = time.perf_counter()
                zbytes = sum(pool.map(lambda p: len(zlib.compress(p, 6)), plains))
                host_s = time.perf_counter() - t0
            # zlib's wrapper is 6 bytes, a gzip member's 18
            line.update(host_threads=a.host_threads, host_zlib6_s=host_s, host_zlib6_gibs=n / host_s / 2**30,
                        host_zlib6_bytes=zbytes + 12 * len(lens))
            if "gzip_s" in line:
                line["device_over_host"] = host_s / line["gzip_s"]
            if a.level:
                import lz4_ref
                with ThreadPoolExecutor(a.host_threads) as pool:
                    # a chunk is at most one 4-MiB block: the block, and the frame's 19 bytes around it
                    line["host_liblz4_bytes"] = sum(pool.map(lz4_ref.lz4_block_size, plains)) + 19 * len(lens)
                for lv in levels[1:]:
                    if f"gzip_gcm_l{lv}_s" in line:
                        line[f"level{lv}_gzip_gcm_over_host"] = host_s / line[f"gzip_gcm_l{lv}_s"]
        print(json.dumps(line), flush=True)
        del buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mib", type=int, default=None, help="default 1024, with --gzip 128")
    ap.add_argument("--reps", type=int, default=None, help="default 5, with --gzip 3")
    ap.add_argument("--kinds", default="random,low_entropy,text")
    ap.add_argument("--labels", default=None, help="default lz4+gcm,lz4,gcm; with --gzip gzip+gcm,gzip,lz4+gcm,lz4")
    ap.add_argument("--gzip", action="store_true", help="the GZIP sets (see the module's docstring)")
    ap.add_argument("--sets", default="c1,c3,text")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--level", type=int, default=0, choices=(0, 1, 9),
                    help="1: every label at levels 0 and 1 (*_l1); 9: at 0, 1 and 9 (*_l9)")
    a = ap.parse_args()
    if a.gzip:
        a.reps = a.reps or 3
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        return gzip_sets(a)
    a.size_mib = a.size_mib or 1024
    a.reps = a.reps or 5
    a.labels = a.labels or "lz4+gcm,lz4,gcm"
    import numpy as np
    import torch

    from datagen import low_entropy, random_bytes
    from plakar_amd import _lib, chunkers, device, encode
    _lib.ensure_init()
    n = a.size_mib << 20
    kinds = {
        "random": lambda: random_bytes(n, 1),
        "low_entropy": lambda: low_entropy(n, 3),
        "text": lambda: np.frombuffer((b"backup snapshot chunk packfile plakar " * (n // 38 + 1))[:n], np.uint8).copy(),
    }
    key = os.urandom(32)
    opts = chunkers.ChunkerOpts(65536, 1 << 20, 4 << 20)
    kinds = {k: v for k, v in kinds.items() if k in a.kinds.split(",")}
    for kind, make in kinds.items():
        t = torch.from_numpy(make()).cuda()
        b = device.DeviceBatch([t], opts)
        b.launch()
        (cuts,), _ = b.results()
        c = cuts.cpu().numpy().astype(np.int64)
        offs, lens = c[:, 0].copy(), c[:, 1].copy()
        for label, k, comp in (("lz4+gcm", key, True), ("lz4", None, True), ("gcm", key, False)):
            if label not in a.labels.split(","):
                continue
            cap = sum(encode.encode_bound(x, comp, k is not None) for x in lens)
            out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            for lv in ({1: (0, 1), 9: (0, 1, 9)}[a.level] if a.level and comp else (0,)):
                encode.encode_device(t, offs, lens, out, key=k, compress=comp, level=lv)  # warm
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    oo = encode.encode_device(t, offs, lens, out, key=k, compress=comp, level=lv)
                torch.cuda.synchronize()
                el = (time.perf_counter() - t0) / a.reps
                print(f"{kind:12s} {label:8s} level {lv} {len(lens):6d} blobs  {n / el / 2**30:8.1f} GiB/s  "
                      f"ratio {oo[-1] / n:.3f}", flush=True)


if __name__ == "__main__":
    main()
