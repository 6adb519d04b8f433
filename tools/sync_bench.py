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

    python tools/sync_bench.py --pipeline [--sets c1,c3,text] [--size-mib 128] [--reps 5] [--batch-mib 16]

times whole syncs of packfiles instead: each set's chunks are stored once under
key A / LZ4 in packfiles, and per leg (A -> B re-key with and without the
check, LZ4 -> GZIP re-encode) sync.SyncSession.run() and the native
sync.SyncPipeline.run() are alternated in one process on the same packfiles
and the same batch size.  One JSON line per set and leg, and all of them in
profiles/sync_bench_pipeline.json: both walls with medians and spreads, the
native run's stage seconds, the overlap it achieved (the sum of the stage
walls over wall_s) and device_wait_s.

    python tools/sync_bench.py --pipeline --stored [--out profiles/...json]

times the native pipeline alone, in the form a repository keeps
(snapshot.PutPackfile: stored packfiles in, stored packfiles out) beside the
plain form (plain in, plain out), alternated in one process on the same blobs:
what the destination's tail Encode per packfile adds to the wall, beside the
spread of either.  The packers' busy time (pack_s) includes the tail's Encode.
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


# --pipeline: leg -> (destination compression, verify)
LEGS = {"rekey-verify": ("LZ4", True), "rekey": ("LZ4", False), "lz4-to-gzip": ("GZIP", True)}
STAGES = ("read_s", "h2d_s", "transcode_s", "d2h_s", "pack_s", "callback_s")
SESSION_STAGES = ("gather_s", "h2d_s", "transcode_s", "d2h_s", "pack_s")


def stored_leg(a, name, leg, kw, packs, stored_packs, nblobs, torch, sync):
    """One leg of --pipeline --stored: plain -> plain beside stored -> stored, alternated."""
    import time
    runs = {"plain": sync.SyncPipeline(packers=a.packers, **kw),
            "stored": sync.SyncPipeline(packers=a.packers, dst_packfile_form="stored", **kw)}
    for p in packs:
        runs["plain"].add_packfile(p)
    t0 = time.perf_counter()
    assert not any(runs["stored"].add_packfiles(stored_packs, form="stored"))
    register_s = time.perf_counter() - t0
    for r in runs.values():
        r.run()  # warm: workspace growth, tables, the slots' buffers, the codec's
    walls, stats = {k: [] for k in runs}, {k: [] for k in runs}
    out = {}
    for _ in range(a.reps):
        for k, r in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[k], fail, st = r.run()
            walls[k].append(time.perf_counter() - t0)
            stats[k].append(st)
            assert not fail
    for r in runs.values():
        r.close()
    med = {k: statistics.median(v) for k, v in walls.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in walls.items()}
    stage = {k: {s: statistics.mean(st[s] for st in stats[k]) for s in STAGES + ("device_wait_s", "wall_s")} for k in runs}
    added = med["stored"] - med["plain"]
    noise = max(spread["plain"] * med["plain"], spread["stored"] * med["stored"])
    return dict(set=name, leg=leg, blobs=nblobs, source_packfiles=len(packs), packfiles=len(out["stored"]),
                packers=a.packers, size_mib=a.size_mib, reps=a.reps, batch_bytes=kw["batch_bytes"],
                stored_register_s=register_s, plain_wall_s=walls["plain"], stored_wall_s=walls["stored"],
                plain_median_s=med["plain"], stored_median_s=med["stored"], plain_spread=spread["plain"],
                stored_spread=spread["stored"], stored_minus_plain_s=added, larger_spread_s=noise,
                within_spread=bool(added <= noise), stage_s=stage,
                stage_with_largest_increase=max(STAGES, key=lambda s: stage["stored"][s] - stage["plain"][s]),
                plain_out_bytes=sum(len(p) for p in out["plain"]), stored_out_bytes=sum(len(p) for p in out["stored"]))


def pipeline(a):
    """Whole syncs of packfiles: SyncSession.run() against SyncPipeline.run()."""
    import hashlib
    import time

    import numpy as np
    import torch

    import bench
    from decode_bench import text_like
    from plakar_amd import _lib, chunkers, device, encode, packer, restore, sync
    _lib.ensure_init()
    dev = torch.device("cuda", 0)
    key_a, key_b = os.urandom(32), os.urandom(32)
    opts = chunkers.ChunkerOpts(65536, 1 << 20, 4 << 20)
    size = a.size_mib << 20
    batch = a.batch_mib << 20
    records = []
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
        # the source repository: every distinct chunk once, under key A / LZ4, in packfiles of the default size
        cap = sum(encode.encode_bound(int(x), True, True) for x in lens)
        enc = torch.empty(cap, dtype=torch.uint8, device=dev)
        oo = encode.encode_device(buf, offs, lens, enc, key=key_a, compress=True)
        stored = enc[:int(oo[-1])].cpu().numpy()
        plain = buf.cpu().numpy()
        del enc, buf
        packs, stored_packs, seen = [], [], set()
        pk = packer.Packer(timestamp=1)

        def flush():
            packs.append(pk.Serialize())
            if a.stored:
                stored_packs.append(pk.PutPackfileBytes(device=0, key=key_a, compression="LZ4"))
            pk.Reset()

        for i in range(len(lens)):
            digest = hashlib.sha256(plain[int(offs[i]):int(offs[i]) + int(lens[i])]).digest()
            if digest in seen:
                continue
            seen.add(digest)
            if pk.AddBlob(1, digest, stored[int(oo[i]):int(oo[i + 1])]):
                flush()
        if pk.Count():
            flush()
        pk.close()
        nblobs, sbytes, pbytes = len(seen), sum(len(p) for p in packs), int(lens.sum())
        del stored, plain
        for leg in a.legs.split(","):
            dc, verify = LEGS[leg]
            kw = dict(src_key=key_a, src_compression="LZ4", dst_key=key_b, dst_compression=dc, verify=verify,
                      batch_bytes=batch, timestamp=2)
            if a.stored:
                records.append(stored_leg(a, name, leg, kw, packs, stored_packs, nblobs, torch, sync))
                print(json.dumps(records[-1]), flush=True)
                continue
            session = sync.SyncSession(**kw)
            native = sync.SyncPipeline(packers=a.packers, **kw)
            for p in packs:
                session.add_packfile(p)
                native.add_packfile(p)

            def timed(run):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = run()
                return out, time.perf_counter() - t0

            session.run(), native.run()  # warm: workspace growth, tables, the slots' buffers
            ss, ns, nstats, sstats = [], [], [], []
            for _ in range(a.reps):  # alternated, so both routes see the same neighbours
                (spacks, sfail, sst), s = timed(session.run)
                (npacks, nfail, nst), n = timed(native.run)
                ss.append(s)
                ns.append(n)
                sstats.append(sst)
                nstats.append(nst)
            rows = lambda ps: sorted((t, c, ln) for p in ps for t, c, _, ln in restore.packfile_index(p)[1])  # noqa: E731
            same = sfail == nfail == {} and rows(spacks) == rows(npacks)
            native.close()
            sm, nm = statistics.median(ss), statistics.median(ns)
            s_spread, n_spread = (max(ss) - min(ss)) / sm, (max(ns) - min(ns)) / nm
            stage = {k: statistics.mean(st[k] for st in nstats) for k in STAGES + ("device_wait_s", "wall_s")}
            sstage = {k: statistics.mean(st[k] for st in sstats) for k in SESSION_STAGES}
            rec = dict(
                set=name, leg=leg, path=nst["path"], verify=verify, blobs=nblobs, batches=int(nst["batches"]),
                source_packfiles=len(packs), packfiles=int(nst["packfiles"]), plain_bytes=pbytes, stored_bytes=sbytes,
                bytes_in=int(nst["bytes_in"]), bytes_out=int(nst["bytes_out"]), batch_bytes=batch, packers=a.packers,
                size_mib=a.size_mib, reps=a.reps, same_rows_as_session=bool(same),
                session_wall_s=ss, native_wall_s=ns, session_median_s=sm, native_median_s=nm,
                session_spread=s_spread, native_spread=n_spread, session_over_native=sm / nm,
                session_gibs=nst["bytes_in"] / sm / 2**30, native_gibs=nst["bytes_in"] / nm / 2**30,
                # the expectation: native no longer than the session by more than the larger of the two spreads
                expectation_met=bool(nm - sm <= max(s_spread * sm, n_spread * nm)),
                native_stage_s=stage, session_stage_s=sstage,
                bounding_stage=max(STAGES, key=lambda k: stage[k]),
                overlap=sum(stage[k] for k in STAGES) / stage["wall_s"], device_wait_s=stage["device_wait_s"])
            records.append(rec)
            print(json.dumps(rec), flush=True)
        del packs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/sync_bench.py --pipeline" + (" --stored" if a.stored else ""), records=records), f,
                      indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="c1,c3,text")
    ap.add_argument("--size-mib", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--settings", default=",".join(SETTINGS))
    ap.add_argument("--pipeline", action="store_true", help="whole syncs: SyncSession against the native pipeline")
    ap.add_argument("--stored", action="store_true",
                    help="--pipeline: the native pipeline stored -> stored beside plain -> plain")
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--batch-mib", type=int, default=16, help="--pipeline: stored bytes per batch, both routes")
    ap.add_argument("--packers", type=int, default=0, help="--pipeline: the native run's packer threads (0: 8)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sync_bench_pipeline.json"),
                    help="--pipeline: where the records go ('' for nowhere)")
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("at least 3 repetitions: the spread is part of the result")
    if a.stored and not a.pipeline:
        ap.error("--stored goes with --pipeline")
    if a.stored and a.out == ap.get_default("out"):
        a.out = ""  # the default file holds the SyncSession comparison
    if a.pipeline:
        if a.reps < 5:
            ap.error("--pipeline: at least 5 repetitions of each route")
        return pipeline(a)

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
