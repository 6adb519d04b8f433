"""Transcode throughput beside the chain a caller had before it: decode_device
under the source codec into a plaintext buffer, then encode_device under the
destination's.  The sets are the chunks of bench.py's C1 and C3 buffers and of
tools/decode_bench.py's text-like buffer, encoded under key A; per set four
settings are timed with hipEvents, both routes in the same process, alternated:

    rekey-lz4, rekey-gzip       A -> B, the compression kept (k_rekey)
    lz4-to-gzip, gzip-to-lz4    A -> B, decoded and encoded again on the device

    python tools/sync_bench.py [--sets c1,c3,text] [--size-mib 128] [--reps 5] [--settings ...]

One JSON line per set and setting: every repetition's seconds for both routes,
their medians and spreads ((max - min) / median), GiB/s of stored bytes and of
plaintext, and chain over transcode (above 1: the transcode is faster).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SETTINGS = {"rekey-lz4": ("LZ4", "LZ4"), "rekey-gzip": ("GZIP", "GZIP"), "lz4-to-gzip": ("LZ4", "GZIP"),
            "gzip-to-lz4": ("GZIP", "LZ4")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="c1,c3,text")
    ap.add_argument("--size-mib", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--settings", default=",".join(SETTINGS))
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("at least 3 repetitions: the spread is part of the result")

    import numpy as np
    import torch

    import bench
    from decode_bench import text_like
    from plakar_amd import _lib, chunkers, decode, device, encode, sync
    _lib.ensure_init()
    dev = torch.device("cuda", 0)
    key_a, key_b = os.urandom(32), os.urandom(32)
    opts = chunkers.ChunkerOpts(65536, 1 << 20, 4 << 20)
    size = a.size_mib << 20

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return r, e0.elapsed_time(e1) / 1e3

    def sel(name):
        return "GZIP" if name == "GZIP" else True

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
        del b
        n = int(lens.sum())
        stored = {}  # compression -> (tensor, offsets, lens) under key A
        for setting in a.settings.split(","):
            sc, dc = SETTINGS[setting]
            if sc not in stored:
                cap = sum(encode.encode_bound(int(x), sel(sc), True) for x in lens)
                enc = torch.empty(cap, dtype=torch.uint8, device=dev)
                oo = encode.encode_device(buf, offs, lens, enc, key=key_a, compress=sel(sc))
                stored[sc] = (enc[:int(oo[-1])].clone(), oo[:-1].copy(), np.diff(oo))
                del enc
            src, soffs, slens = stored[sc]
            nb = len(slens)
            rnd = os.urandom(56 * nb)
            cap = sum(encode.encode_bound(int(x), sel(dc), True) for x in lens)
            out_t = torch.empty(cap, dtype=torch.uint8, device=dev)
            out_c = torch.empty(cap, dtype=torch.uint8, device=dev)
            plain = torch.empty(n, dtype=torch.uint8, device=dev)

            def transcode():
                return sync.transcode_device(src, soffs, slens, out_t, src=(key_a, sc), dst=(key_b, dc), random=rnd)

            def chain():
                doo, st = decode.decode_device(src, soffs, slens, plain, key=key_a, compressed=sel(sc))
                eoo = encode.encode_device(plain, doo[:-1], np.diff(doo), out_c, key=key_b, compress=sel(dc), random=rnd)
                return eoo, st

            transcode(), chain()  # warm: workspace growth, tables
            ts, cs = [], []
            for _ in range(a.reps):  # alternated, so both routes see the same neighbours
                (too, tst), t = once(transcode)
                (coo, cst), s = once(chain)
                ts.append(t)
                cs.append(s)
            same = bool((tst == 0).all() and (cst == 0).all() and np.array_equal(too, coo) and
                        torch.equal(out_t[:int(too[-1])], out_c[:int(coo[-1])]))
            # what the transcode wrote reads back to the chunks under key B
            doo, dst = decode.decode_device(out_t, too[:-1], np.diff(too), plain, key=key_b, compressed=sel(dc))
            ok = bool((dst == 0).all()) and int(doo[-1]) == n and all(
                torch.equal(plain[int(doo[i]):int(doo[i + 1])], buf[int(offs[i]):int(offs[i]) + int(lens[i])])
                for i in range(0, nb, max(1, nb // 16)))
            tm, cm = statistics.median(ts), statistics.median(cs)
            sbytes = int(slens.sum())
            print(json.dumps(dict(
                set=name, setting=setting, path=sync.path_of((key_a, sc), (key_b, dc)), blobs=nb, plain_bytes=n,
                stored_bytes=sbytes, out_bytes=int(too[-1]), reps=a.reps, round_trip_ok=ok, same_bytes_as_chain=same,
                transcode_s=ts, chain_s=cs, transcode_median_s=tm, chain_median_s=cm,
                transcode_spread=(max(ts) - min(ts)) / tm, chain_spread=(max(cs) - min(cs)) / cm,
                transcode_stored_gibs=sbytes / tm / 2**30, transcode_plain_gibs=n / tm / 2**30,
                chain_stored_gibs=sbytes / cm / 2**30, chain_plain_gibs=n / cm / 2**30,
                chain_over_transcode=cm / tm)), flush=True)
            del out_t, out_c, plain
        del stored, buf


if __name__ == "__main__":
    main()
