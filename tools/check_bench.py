"""Check throughput: backup, then check, of the C1 and C3 buffers of bench.py cut
into 64 files each and of text-like bytes as files of 16 KiB (archive_bench's
small-file set), all LZ4 + AES-256-GCM.

    python tools/check_bench.py [--sets c1,c3,small] [--size-mib 256] [--reps 3] [--out profiles/check_bench.json]

One JSON line per set, every measurement in one process, --reps runs each
after one that grows the buffers (every run's GiB/s of file bytes is kept: the
spread between them is the margin for every comparison):

  * the check with the default split, forced all-host (host_min_len = 1) and
    forced all-device for single-batch files (host_min_len = 2^64 - 1), with
    the best run's stage seconds and device/host shares;
  * the baseline a caller had before cdc_check_files: restore_files(dests=None),
    then SHA-256 of every returned file on --host-threads threads;
  * k_object_digest against k_chunk_digest over the same bytes, one segment
    per object = the same chunks (the set's own chunk lengths laid back to
    back over the buffer), as microseconds per 64-byte block of the longest
    chunk: a launch lasts as long as its longest chain."""
import argparse
import ctypes
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

U64_MAX = 2 ** 64 - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="c1,c3,small")
    ap.add_argument("--size-mib", type=int, default=256)
    ap.add_argument("--files", type=int, default=64, help="files of the c1 and c3 sets")
    ap.add_argument("--small-kib", type=int, default=16, help="the file size of the `small` set")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--tmp", default=None, help="directory for the files (default: a temporary one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_bench.json"))
    a = ap.parse_args()
    import hashlib
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np
    import torch

    import bench
    import decode_bench
    from plakar_amd import _lib, check, hashing, restore, snapshot
    _lib.ensure_init()
    dev = torch.device("cuda", 0)
    key = os.urandom(32)
    size = a.size_mib << 20
    lines = []
    for name in a.sets.split(","):
        if name == "small":
            data = np.frombuffer(decode_bench.text_like(np, size), dtype=np.uint8)
            step = a.small_kib << 10
        else:
            data = bench.make_buffers(torch, bench.WORKLOADS[name], 0, dev, size)[0].cpu().numpy()
            step = -(-data.size // a.files)
        work = tempfile.mkdtemp(prefix="check_bench_", dir=a.tmp)
        try:
            paths = []
            for i in range(0, data.size, step):
                p = os.path.join(work, f"in{i // step:06d}")
                data[i:i + step].tofile(p)
                paths.append(p)
            objs, packs, _ = snapshot.backup_files(paths, key=key)
            want = [bytes(o.Checksum) for o in objs]
            line = dict(set=name, reps=a.reps, files=len(paths), file_bytes=int(data.size),
                        chunks=sum(len(o.Chunks) for o in objs))
            for label, hml in (("default", 0), ("all_host", 1), ("all_device", U64_MAX)):
                runs, best = [], None
                with check.CheckSession(key=key, host_min_len=hml, threads=a.host_threads) as s:
                    for p in packs:
                        s.add_packfile(p)
                    for r in range(a.reps + 1):  # the first run grows the buffers
                        res, st = s.run(objs)
                        assert [x["status"] for x in res] == [0] * len(objs)
                        assert [x["checksum"] for x in res] == want
                        if r:
                            runs.append(data.size / st["wall_s"] / 2**30)
                            if best is None or st["wall_s"] < best["wall_s"]:
                                best = st
                line[f"{label}_gibs_runs"] = runs
                line[f"{label}_gibs"] = max(runs)
                line.update({f"{label}_{k}": v for k, v in best.items()})
            # what a caller had before: the files copied back, then hashed on the host
            runs = []
            with restore.RestoreSession(key=key) as s, ThreadPoolExecutor(a.host_threads) as pool:
                for p in packs:
                    s.add_packfile(p)
                for r in range(a.reps + 1):
                    t0 = time.perf_counter()
                    contents, statuses, _ = s.run(objs)
                    got = list(pool.map(lambda b: hashlib.sha256(b).digest(), contents))
                    dt = time.perf_counter() - t0
                    assert not any(statuses) and got == want
                    if r:
                        runs.append(data.size / dt / 2**30)
                del contents
            line["restore_then_hash_gibs_runs"] = runs
            line["restore_then_hash_gibs"] = max(runs)
            line["default_over_restore_then_hash"] = line["default_gibs"] / line["restore_then_hash_gibs"]
            # the two digest kernels over the same chunks of the same buffer
            lens = [int(c.Length) for o in objs for c in o.Chunks if c.Length]
            offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
            src = torch.from_numpy(data.copy()).to(dev)
            cuts = torch.from_numpy(np.stack([offs, np.asarray(lens, np.int64)], axis=1).copy()).to(dev)
            # both through the C ABI with their arguments made beforehand: the object call plans its runs
            # on the host and is synchronous, the chunk call only launches
            seg_off, seg_len = offs.astype(np.uint64), np.asarray(lens, np.uint64)
            seg0 = np.arange(len(lens) + 1, dtype=np.uint64)
            dobj = torch.empty((len(lens), 32), dtype=torch.uint8, device=dev)
            p64 = ctypes.POINTER(ctypes.c_uint64)
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            blocks = max(lens) // 64 + 1

            def object_call():
                _lib.check(_lib.lib().cdc_object_digests_device(
                    0, ctypes.c_void_p(src.data_ptr()), src.numel(), seg_off.ctypes.data_as(p64),
                    seg_len.ctypes.data_as(p64), len(lens), seg0.ctypes.data_as(p64), len(lens),
                    ctypes.c_void_p(dobj.data_ptr()), stream), "cdc_object_digests_device")
                return dobj

            def timed(fn):
                out = []
                for r in range(a.reps + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    d = fn()
                    torch.cuda.synchronize()
                    if r:
                        out.append((time.perf_counter() - t0) * 1e6 / blocks)
                return out, d

            c_us, dc = timed(lambda: hashing.chunk_digests(src, cuts, hist=False)[0])
            o_us, do = timed(object_call)
            assert torch.equal(dc, do)
            line.update(kernel_chunks=len(lens), kernel_longest_blocks=blocks, chunk_digest_us_per_block_runs=c_us,
                        object_digest_us_per_block_runs=o_us, chunk_digest_us_per_block=min(c_us),
                        object_digest_us_per_block=min(o_us))
            del src, cuts
            text = json.dumps(line)
            print(text, flush=True)
            lines.append(line)
        finally:
            shutil.rmtree(work, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(size_mib=a.size_mib, host_threads=a.host_threads, sets=lines), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
