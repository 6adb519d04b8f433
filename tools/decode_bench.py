"""Device Decode throughput beside Encode's, on the chunks of the C1 / C2 / C3
buffers of bench.py: each set is chunked, encoded and decoded in one process,
hipEvents around each call, then decoded again on the host (libcrypto open +
liblz4 inflate on --host-threads threads) as the baseline.  One JSON line per
set and setting:

    python tools/decode_bench.py [--sets c1,c2,c3] [--size-mib 1024] [--reps 3] [--labels lz4+gcm]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="c1,c2,c3")
    ap.add_argument("--size-mib", type=int, default=1024, help="bytes per set (C2: split over its 32 buffers)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--labels", default="lz4+gcm")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
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
