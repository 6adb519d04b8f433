"""Restore throughput: backup, then restore, of the C1 and C3 buffers of bench.py
cut into files, and of a duplicate-heavy set (every C1 file present twice);
and the assemble kernel alone against a device-to-device copy.

    python tools/restore_bench.py [--sets c1,c3,dup,assemble] [--size-mib 1024] [--file-mib 16] [--reps 3]

One JSON line per set: GiB/s of restored output (bytes / the pipeline's wall
time, files written to --tmp) with cdc_restore_stats, and beside it the host
path the reference takes: tests/crypto_ref.decode per chunk occurrence on
--host-threads threads.  The `assemble` line times cdc_assemble_device over
1 GiB of 64-KiB..4-MiB segments at odd source and destination alignments with
hipEvents, under each cache policy, against a same-device tensor copy (torch
issues it as hipMemcpyAsync device-to-device) of the same bytes in the same
process.

    python tools/restore_bench.py --stored [--size-mib 1024] [--reps 3] [--out profiles/stored_form.json]

measures what registering packfiles costs in the form a repository keeps
(snapshot.PutPackfile) beside the plain form: one chunk set (--size-mib of C1
bytes in 16-KiB chunks, 65,536 of them at 1 GiB, under a key and LZ4) is laid
out once as packfiles of 64 rows (1,024 at 1 GiB) and once as packfiles of the
default MaxSize, each written to disk in both forms.  Per layout, in one
process and alternated, --reps times after a warm-up: add_packfile(path) per
plain packfile (the yardstick), one add_packfiles(form="stored") call, and one
add_packfiles call per stored packfile; then a restore of every file from a
session of each kind.  One JSON line per layout with every repetition's
seconds, medians and spreads ((max - min) / median)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def bench_assemble(a, torch, np):
    from plakar_amd import _lib, restore
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    total, lens, d = a.size_mib << 20, [], 0
    while d < total:
        n = min(int(rng.integers(64 << 10, (4 << 20) + 1)) | 1, total - d)  # odd lengths: every alignment follows
        lens.append(n)
        d += n
    # Every source byte is read once, as in a restore without duplicates (a
    # source that repeats is served by the caches and would flatter the kernel
    # beside a copy that reads 1 GiB from HBM): the segments' sources lie back
    # to back in a shuffled order, from offset 1.
    src = torch.randint(0, 256, (total + 16,), dtype=torch.uint8, device=dev)
    src_of, s = {}, 1
    for i in rng.permutation(len(lens)):
        src_of[int(i)] = s
        s += lens[int(i)]
    segs, d = [], 0
    for i, n in enumerate(lens):
        segs.append((src_of[i], n, d))
        d += n
    dst = torch.empty(total + 64, dtype=torch.uint8, device=dev)[3:3 + total]
    flat_src = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev)
    flat_dst = torch.empty(total, dtype=torch.uint8, device=dev)

    def timed(fn):
        fn()
        best = None
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            best = e0.elapsed_time(e1) if best is None else min(best, e0.elapsed_time(e1))
        return best / 1e3

    copy_s = timed(lambda: flat_dst.copy_(flat_src))
    line = dict(set="assemble", bytes=total, segments=len(segs), reps=a.reps, d2d_copy_s=copy_s,
                d2d_copy_gibs=total / copy_s / 2**30)
    for policy, name in ((2, "nt_stores"), (0, "plain"), (1, "nt_loads"), (3, "nt_both")):
        _lib.lib().cdc_debug_set_assemble_policy(policy)
        s = timed(lambda: restore.assemble_device(src, segs, dst))
        line[f"{name}_s"], line[f"{name}_gibs"], line[f"{name}_over_copy"] = s, total / s / 2**30, copy_s / s
    _lib.lib().cdc_debug_set_assemble_policy(2)
    k = len(segs) // 2
    so, n, do = segs[k]
    line["spot_check_ok"] = bool(torch.equal(dst[do:do + n], src[so:so + n]))
    print(json.dumps(line), flush=True)


def bench_stored(a):
    import hashlib
    import statistics
    import types

    import numpy as np
    import torch

    import bench
    from plakar_amd import _lib, encode, packer, restore
    _lib.ensure_init()
    dev = torch.device("cuda", 0)
    key = os.urandom(32)
    chunk, per_file = 16 << 10, 1024
    size = (a.size_mib << 20) // (chunk * per_file) * (chunk * per_file)
    buf = bench.make_buffers(torch, bench.WORKLOADS["c1"], 0, dev, size)[0]
    n = size // chunk
    offs, lens = np.arange(n, dtype=np.int64) * chunk, np.full(n, chunk, dtype=np.int64)
    enc = torch.empty(encode.encode_bound(chunk, True, True) * n, dtype=torch.uint8, device=dev)
    oo = encode.encode_device(buf, offs, lens, enc, key=key, compress=True)
    blobs = enc[:int(oo[-1])].cpu().numpy()
    plain = buf.cpu().numpy()
    del enc, buf
    sums = [hashlib.sha256(plain[i * chunk:(i + 1) * chunk]).digest() for i in range(n)]
    objs = [types.SimpleNamespace(Chunks=[types.SimpleNamespace(Checksum=sums[i], Length=chunk)
                                          for i in range(f * per_file, (f + 1) * per_file)]) for f in range(n // per_file)]
    work = tempfile.mkdtemp(prefix="stored_bench_", dir=a.tmp)
    records = []
    try:
        for layout, rows_per in (("64-row packfiles", 64), ("default packfiles", None)):
            pk = packer.Packer(timestamp=1)
            paths = {"plain": [], "stored": []}

            def flush():
                k = len(paths["plain"])
                for form, data in (("plain", pk.Serialize()),
                                   ("stored", pk.PutPackfileBytes(device=0, key=key, compression="LZ4"))):
                    path = os.path.join(work, f"{rows_per}_{form}_{k:05d}")
                    with open(path, "wb") as f:
                        f.write(data)
                    paths[form].append(path)
                pk.Reset()

            for i in range(n):
                full = pk.AddBlob(1, sums[i], blobs[int(oo[i]):int(oo[i + 1])])
                if (pk.Count() == rows_per) if rows_per else full:
                    flush()
            if pk.Count():
                flush()
            pk.close()
            npacks = len(paths["plain"])

            def register(kind):
                s = restore.RestoreSession(key=key)
                t0 = time.perf_counter()
                if kind == "plain":
                    for path in paths["plain"]:
                        s.add_packfile(path)
                elif kind == "stored_one_call":
                    assert not any(s.add_packfiles(paths["stored"], form="stored"))
                else:
                    for path in paths["stored"]:
                        assert s.add_packfiles([path], form="stored") == [0]
                return s, time.perf_counter() - t0

            kinds = ("plain", "stored_one_call", "stored_call_each")
            for kind in kinds:  # warm: the codec's buffers, Decode's workspace, the page cache
                register(kind)[0].close()
            reg = {k: [] for k in kinds}
            rst = {k: [] for k in kinds}
            dests = [os.path.join(work, f"out{i:05d}") for i in range(len(objs))]
            ok = True
            for r in range(a.reps + 1):  # alternated; the first round grows the restore buffers and is dropped
                for kind in kinds:
                    s, t = register(kind)
                    _, statuses, st = s.run(objs, dests)
                    s.close()
                    ok = ok and not any(statuses)
                    if r:
                        reg[kind].append(t)
                        rst[kind].append(st["wall_s"])
            k = len(dests) // 2
            ok = ok and open(dests[k], "rb").read() == plain[k * per_file * chunk:(k + 1) * per_file * chunk].tobytes()
            med = lambda v: statistics.median(v)  # noqa: E731
            spread = lambda v: (max(v) - min(v)) / med(v)  # noqa: E731
            rec = dict(layout=layout, packfiles=npacks, rows=n, rows_per_packfile=rows_per or n / npacks, bytes=size,
                       reps=a.reps, round_trip_ok=bool(ok),
                       stored_bytes=sum(os.path.getsize(x) for x in paths["stored"]),
                       plain_bytes=sum(os.path.getsize(x) for x in paths["plain"]))
            for kind in kinds:
                rec[kind] = dict(register_s=reg[kind], register_median_s=med(reg[kind]), register_spread=spread(reg[kind]),
                                 register_us_per_packfile=med(reg[kind]) / npacks * 1e6,
                                 restore_wall_s=rst[kind], restore_median_s=med(rst[kind]), restore_spread=spread(rst[kind]))
            rec["one_call_over_plain"] = rec["stored_one_call"]["register_median_s"] / rec["plain"]["register_median_s"]
            rec["call_each_over_one_call"] = rec["stored_call_each"]["register_median_s"] / \
                rec["stored_one_call"]["register_median_s"]
            records.append(rec)
            print(json.dumps(rec), flush=True)
            for form in paths:
                for path in paths[form]:
                    os.remove(path)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="c1,c3,dup,assemble")
    ap.add_argument("--size-mib", type=int, default=1024)
    ap.add_argument("--file-mib", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--tmp", default=None, help="directory for the files (default: a temporary one)")
    ap.add_argument("--stored", action="store_true", help="registration and restore: the stored form beside the plain")
    ap.add_argument("--out", default=None, help="--stored: also write the records to this JSON file")
    a = ap.parse_args()
    if a.stored:
        records = bench_stored(a)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(dict(tool="tools/restore_bench.py --stored", records=records), f, indent=1)
                f.write("\n")
        return
    import hashlib
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np
    import torch

    import bench
    import crypto_ref
    from plakar_amd import _lib, restore, snapshot
    _lib.ensure_init()
    dev = torch.device("cuda", 0)
    key = os.urandom(32)
    for name in a.sets.split(","):
        if name == "assemble":
            bench_assemble(a, torch, np)
            continue
        wl = bench.WORKLOADS["c1" if name == "dup" else name]
        data = bench.make_buffers(torch, wl, 0, dev, a.size_mib << 20)[0].cpu().numpy()
        work = tempfile.mkdtemp(prefix="restore_bench_", dir=a.tmp)
        try:
            step = a.file_mib << 20
            paths = []
            for i in range(0, data.size, step):
                for copy in range(2 if name == "dup" else 1):
                    p = os.path.join(work, f"in{i // step:04d}_{copy}")
                    data[i:i + step].tofile(p)
                    paths.append(p)
            objs, packs, bst = snapshot.backup_files(paths, key=key)
            dests = [os.path.join(work, f"out{i:05d}") for i in range(len(paths))]
            best = None
            with restore.RestoreSession(key=key) as s:
                for p in packs:
                    s.add_packfile(p)
                for _ in range(a.reps + 1):  # the first run grows the buffers
                    _, statuses, st = s.run(objs, dests)
                    assert not any(statuses)
                    if best is None or st["wall_s"] < best["wall_s"]:
                        best = st
            ok = all(hashlib.sha256(open(d, "rb").read()).digest() == hashlib.sha256(open(p, "rb").read()).digest()
                     for p, d in list(zip(paths, dests))[::max(1, len(paths) // 8)])
            line = dict(set=name, reps=a.reps, round_trip_ok=ok, backup_wall_s=bst["wall_s"],
                        restore_gibs=best["bytes"] / best["wall_s"] / 2**30, **best)
            if not a.no_host:
                blobs = {}
                for p in packs:
                    for _, c, o, n in restore.packfile_index(p)[1]:
                        blobs[c] = p[o:o + n]
                occ = [blobs[bytes(c.Checksum)] for o in objs for c in o.Chunks]
                with ThreadPoolExecutor(a.host_threads) as pool:
                    t0 = time.perf_counter()
                    total = sum(pool.map(lambda x: len(crypto_ref.decode(x, key, True)), occ))
                    host_s = time.perf_counter() - t0
                assert total == best["bytes"]
                line.update(host_threads=a.host_threads, host_decode_s=host_s,
                            host_decode_gibs=total / host_s / 2**30, restore_over_host=host_s / best["wall_s"])
            print(json.dumps(line), flush=True)
        finally:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
