"""State throughput: cdc_state_merge of a repository's state files, the queries
against the aggregate, and a single-threaded host merge over the same bytes.

    python tools/state_bench.py [--rows 1000000,16000000] [--states 1,64,1024] [--reps 3]
                                [--queries 1000000] [--out profiles/state_bench.json]

For each total of TYPE_CHUNK rows, split over 1, 64 and 1,024 states (a
packfile per 1,000 rows, IdToChecksum and location records in shuffled order,
as a Go map writes them), in two configurations, LZ4 + AES-256-GCM and no
compression with no key:

  * cdc_state_merge of all stored states in one call into a fresh aggregate:
    wall seconds of the C call (sources prepared beforehand), and the
    library's own decode / index / insert seconds (cdc_state_info);
  * the host merge: the states' plaintexts through state_plan.h's reader into
    an unordered_map keyed as cdc_locator.h's Locator is (checksum -> blob
    number, first location wins), one thread, compiled here with g++ -O2;
    timed alone, and with the host's own Decode before it (libcrypto open +
    liblz4 inflate, tests/crypto_ref.py, one thread).

Then, on the aggregate of the first total in 64 states (LZ4 + key): --queries
blob_exists queries, half present, and packfile_rows of everything.

Medians of --reps runs after one warm-up, each with its smallest and largest
run; a merge whose warm-up run takes more than --slow-s seconds is not run
again, and that one run is what is reported (reps = 1).  One JSON line per measurement; all of them in --out."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HOST_MERGE_SRC = r"""
// The host's merge: DeserializeStream's ranges (state_plan.h), then
// SetPackfileForBlob's rule over an unordered_map keyed as Locator's is.
#include <chrono>
#include <unordered_map>
#include <vector>
#include "state_plan.h"
namespace {
struct Loc { uint32_t pack, offset, length; };
}
extern "C" double host_merge(const uint8_t *base, const uint64_t *off, const uint64_t *len, uint32_t n, uint64_t *entries)
{
    const auto t0 = std::chrono::steady_clock::now();
    std::unordered_map<splan::Sum, uint32_t, splan::SumHash> index[splan::kTypes];
    std::unordered_map<splan::Sum, uint32_t, splan::SumHash> packs;
    std::vector<Loc> locs;
    std::vector<const uint8_t *> sum_of;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t *s = base + off[i];
        splan::Layout L;
        if (splan::read(s, len[i], &L) != CDC_OK) return -1;
        const splan::Section &I = L.sec[splan::kSecIds];
        sum_of.assign(I.count, nullptr);
        for (uint64_t k = 0; k < I.count; ++k) {
            const uint8_t *r = s + I.off + splan::kIdBytes * k;
            const uint64_t id = splan::rd64(r);
            if (id >= I.count || sum_of[id]) return -1;
            sum_of[id] = r + 8;
        }
        for (uint32_t sec = splan::kSecFirstType; sec < splan::kSections; ++sec) {
            auto &M = index[splan::type_of_section(sec)];
            const splan::Section &C = L.sec[sec];
            for (uint64_t k = 0; k < C.count; ++k) {
                const uint8_t *r = s + C.off + splan::kLocBytes * k;
                const uint64_t id = splan::rd64(r), pk = splan::rd64(r + 8);
                if (id >= I.count || pk >= I.count) return -1;
                splan::Sum key, pkey;
                memcpy(key.b, sum_of[id], 32);
                if (M.emplace(key, uint32_t(locs.size())).second) {
                    memcpy(pkey.b, sum_of[pk], 32);
                    const uint32_t p = packs.emplace(pkey, uint32_t(packs.size())).first->second;
                    locs.push_back(Loc{p, splan::rd32(r + 16), splan::rd32(r + 20)});
                }
            }
        }
    }
    for (auto &M : index) total += M.size();
    *entries = total;
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
"""


def med(runs):
    return dict(median=statistics.median(runs), min=min(runs), max=max(runs), runs=runs)


def make_state(np, rng, rows, per_pack=1000):
    """One state's plaintext with `rows` chunk rows, and its blob checksums (rows, 32)."""
    packs = -(-rows // per_pack)
    nids = packs + rows
    sums = np.frombuffer(rng.bytes(32 * nids), dtype=np.uint8).reshape(nids, 32)
    ids = np.zeros(nids, dtype=[("id", "<u8"), ("sum", "u1", 32)])
    perm = rng.permutation(nids)
    ids["id"], ids["sum"] = perm, sums[perm]
    locs = np.zeros(rows, dtype=[("id", "<u8"), ("pack", "<u8"), ("off", "<u4"), ("len", "<u4")])
    order = rng.permutation(rows)
    locs["id"], locs["pack"] = packs + order, order // per_pack
    locs["off"], locs["len"] = (order % per_pack) * 16384, 16384
    u64 = lambda v: np.uint64(v).tobytes()  # noqa: E731
    head = np.uint32(100).tobytes() + u64(1_700_000_000_000_000_000) + b"\0" + u64(0) + u64(0)
    plain = b"".join([head, u64(nids), ids.tobytes(), u64(rows), locs.tobytes(), u64(0) * 8])
    assert len(plain) == 109 + 40 * nids + 24 * rows
    return plain, sums[packs:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,16000000")
    ap.add_argument("--states", default="1,64,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--slow-s", type=float, default=10.0,
                    help="a merge whose warm-up run takes longer is not repeated: that run is the measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401 - its HIP runtime comes up before the library's

    import crypto_ref
    from plakar_amd import _lib, encode, state
    L = _lib.lib()
    work = tempfile.mkdtemp(prefix="state_bench_")
    host = None
    if not a.no_host:
        src, so = os.path.join(work, "host_merge.cpp"), os.path.join(work, "host_merge.so")
        with open(src, "w") as f:
            f.write(HOST_MERGE_SRC)
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "plakar_amd", "csrc"), "-o", so, src], check=True)
        host = ctypes.CDLL(so).host_merge
        host.restype = ctypes.c_double
        host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
    key = bytes(range(32))
    configs = [("lz4+gcm", "LZ4", key), ("none", None, None)]
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)
        if a.out:  # rewritten after every measurement: a run that is cut short keeps what it had
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(dict(reps=a.reps, slow_s=a.slow_s, measurements=lines), f, indent=1)
                f.write("\n")

    def note(text):
        print(f"[state_bench] {text}", file=sys.stderr, flush=True)

    query_case = None
    for total in [int(x) for x in a.rows.split(",")]:
        for nstates in [int(x) for x in a.states.split(",")]:
            note(f"{total} rows in {nstates} states: generating")
            rng = np.random.default_rng(total + nstates)
            per = total // nstates
            plains, blob_sums = [], []
            for _ in range(nstates):
                p, s = make_state(np, rng, per)
                plains.append(p)
                blob_sums.append(s)
            rows = per * nstates
            plain_bytes = sum(len(p) for p in plains)
            base = np.frombuffer(b"".join(plains), dtype=np.uint8)
            lens = np.array([len(p) for p in plains], dtype=np.uint64)
            offs = (np.cumsum(lens) - lens).astype(np.uint64)
            host_s = None
            if host is not None:
                note("host merge")
                runs, n = [], ctypes.c_uint64()
                for r in range(a.reps + 1):
                    dt = host(base.ctypes.data, offs.ctypes.data, lens.ctypes.data, nstates, ctypes.byref(n))
                    assert dt >= 0 and n.value == rows
                    if r:
                        runs.append(dt)
                host_s = med(runs)
            for label, comp, k in configs:
                note(f"{label}: encode, then merge")
                enc = encode.DeviceEncoder(key=k, compression=comp)
                stored = []
                for i in range(0, nstates, 64):  # 64 states per Encode call
                    stored += enc.encode_many(plains[i:i + 64])
                arr = (_lib.cdc_state_src * nstates)()
                keep = []
                for i, b in enumerate(stored):
                    buf = ctypes.create_string_buffer(b, len(b))
                    keep.append(buf)
                    arr[i].bytes, arr[i].len, arr[i].form = ctypes.cast(buf, ctypes.c_void_p), len(b), _lib.STATE_STORED
                status = (ctypes.c_int32 * nstates)()
                wall, stages, info = [], dict(decode_s=[], index_s=[], insert_s=[]), None
                for r in range(a.reps + 1):
                    S = state.State(key=k, compression=comp)
                    t0 = time.perf_counter()
                    rc = L.cdc_state_merge(S._h, arr, nstates, status)
                    dt = time.perf_counter() - t0
                    assert rc == 0 and not any(status), (rc, list(status)[:8])
                    info = S.info()
                    assert info["rows"][1] == rows and info["states"] == nstates
                    slow = r == 0 and dt > a.slow_s
                    if r or slow:
                        wall.append(dt)
                        for name in stages:
                            stages[name].append(info[name])
                    last = slow or r == a.reps
                    if not last or query_case is not None or label != "lz4+gcm" or nstates != 64:
                        S.close()
                    else:
                        query_case = (S, np.concatenate(blob_sums), rows)
                    if last:
                        break
                line = dict(what="merge", config=label, rows=rows, states=nstates, plain_bytes=plain_bytes,
                            stored_bytes=sum(len(b) for b in stored), reps=len(wall), merge_s=med(wall),
                            rows_per_s=rows / statistics.median(wall), capacity=info["capacity"],
                            device_bytes=info["device_bytes"], **{n: med(v) for n, v in stages.items()})
                if host_s is not None:
                    note("host decode")
                    line["host_merge_s"] = host_s
                    runs = []
                    for r in range(2 if rows > 4_000_000 else a.reps + 1):  # the large decode once after its warm-up
                        t0 = time.perf_counter()
                        parts = [crypto_ref.decode(b, k, bool(comp)) for b in stored]
                        dt = time.perf_counter() - t0
                        assert sum(len(p) for p in parts) == plain_bytes
                        if r:
                            runs.append(dt)
                    line["host_decode_s"] = med(runs)
                    line["host_decode_and_merge_s"] = statistics.median(runs) + host_s["median"]
                    line["device_over_host_merge"] = host_s["median"] / statistics.median(wall)
                    line["device_over_host_decode_and_merge"] = line["host_decode_and_merge_s"] / statistics.median(wall)
                emit(line)
                del keep, arr, stored
    if query_case is not None:
        S, sums, rows = query_case
        rng = np.random.default_rng(7)
        nq = a.queries
        q = np.frombuffer(rng.bytes(32 * nq), dtype=np.uint8).reshape(nq, 32).copy()
        q[::2] = sums[rng.integers(0, len(sums), size=(nq + 1) // 2)]
        runs = []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            found = S.blob_exists(state.TYPE_CHUNK, q)
            dt = time.perf_counter() - t0
            assert found[::2].all() and not found[1::2].any()
            if r:
                runs.append(dt)
        emit(dict(what="blob_exists", rows=rows, queries=nq, present=(nq + 1) // 2, seconds=med(runs),
                  queries_per_s=nq / statistics.median(runs)))
        runs, runs_rows = [], []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            got = S.rows(state.TYPE_CHUNK)
            t1 = time.perf_counter()
            by_pack = S.packfile_rows(state.TYPE_CHUNK)
            dt = time.perf_counter() - t1
            assert len(got) == rows and sum(len(v) for v in by_pack.values()) == rows
            if r:
                runs.append(dt)
                runs_rows.append(t1 - t0)
        emit(dict(what="packfile_rows", rows=rows, packfiles=len(by_pack), seconds=med(runs),
                  cdc_state_rows_seconds=med(runs_rows)))
        S.close()


if __name__ == "__main__":
    main()
