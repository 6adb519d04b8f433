"""Maintenance throughput: cdc_state_mark and cdc_state_sweep on an aggregate of
chunk rows, and a single-threaded host restatement of the same rule.

    python tools/maintenance_bench.py [--rows 1000000,16000000] [--states 64] [--live 50,95] [--reps 3]
                                      [--out profiles/maintenance_bench.json]

For each total of TYPE_CHUNK rows (a packfile per 1,000 rows, in --states
states made as tools/state_bench.py makes them, merged in the plain form) and
each live share: that share of the rows is referenced, every reference given
twice (snapshots share chunks), in shuffled order.  Timed:

  * cdc_state_mark of all references in one call (upload, k_state_mark, the
    miss count), after cdc_state_clear_marks;
  * cdc_state_sweep: the wall seconds of the C call, and the library's own
    seconds per stage (cdc_sweep_info: packs, sweep, verdict, compaction, the
    plan's download);
  * the plan's copy out of the cdc_sweep (cdc_sweep_packs, _kept_rows,
    _repack_rows into numpy arrays);
  * the host leg, one thread, compiled here with g++ -O2: state_plan.h's reader
    into an unordered_map (the index, built once and not part of the timings:
    tools/state_bench.py measures it), then the marks (one lookup per
    reference into a bit vector) and the sweep (the live rule per record, the
    per-packfile sums in a second unordered_map, sweep_plan.h's verdict, the
    kept rows and the grouped repack rows as 80-byte rows).

The two legs' plans are compared (counts, live bytes, verdict counts) before a
figure is reported.  Medians of --reps runs after one warm-up, each with its
smallest and largest run.  One JSON line per measurement; all of them in --out."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOST_SRC = r"""
// The host's maintenance: the index as tools/state_bench.py's host merge builds
// it (with the records kept in order), then mark and sweep by the same rule.
#include <algorithm>
#include <chrono>
#include <unordered_map>
#include <vector>
#include "state_plan.h"
#include "sweep_plan.h"
namespace {
struct Rec { const uint8_t *sum; uint32_t pack, offset, length, type; };
struct Pack { const uint8_t *sum; uint64_t extent, live_bytes, live_rows, first; int32_t verdict; };
struct Host {
    std::unordered_map<splan::Sum, uint64_t, splan::SumHash> index[splan::kTypes];  // key -> winner's record number
    std::unordered_map<splan::Sum, uint32_t, splan::SumHash> pack_of;
    std::vector<const uint8_t *> pack_sum;
    std::vector<Rec> recs;
    std::vector<uint8_t> marks;
};
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}
extern "C" void *host_build(const uint8_t *base, const uint64_t *off, const uint64_t *len, uint32_t n)
{
    Host *H = new Host();
    std::vector<const uint8_t *> sum_of;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t *s = base + off[i];
        splan::Layout L;
        if (splan::read(s, len[i], &L) != CDC_OK) return nullptr;
        const splan::Section &I = L.sec[splan::kSecIds];
        sum_of.assign(I.count, nullptr);
        for (uint64_t k = 0; k < I.count; ++k) {
            const uint8_t *r = s + I.off + splan::kIdBytes * k;
            const uint64_t id = splan::rd64(r);
            if (id >= I.count || sum_of[id]) return nullptr;
            sum_of[id] = r + 8;
        }
        for (uint32_t sec = splan::kSecFirstType; sec < splan::kSections; ++sec) {
            const uint32_t type = splan::type_of_section(sec);
            const splan::Section &C = L.sec[sec];
            for (uint64_t k = 0; k < C.count; ++k) {
                const uint8_t *r = s + C.off + splan::kLocBytes * k;
                const uint64_t id = splan::rd64(r), pk = splan::rd64(r + 8);
                if (id >= I.count || pk >= I.count) return nullptr;
                splan::Sum key, pkey;
                memcpy(key.b, sum_of[id], 32);
                memcpy(pkey.b, sum_of[pk], 32);
                const auto p = H->pack_of.emplace(pkey, uint32_t(H->pack_sum.size()));
                if (p.second) H->pack_sum.push_back(sum_of[pk]);
                H->index[type].emplace(key, uint64_t(H->recs.size()));
                H->recs.push_back(Rec{sum_of[id], p.first->second, splan::rd32(r + 16), splan::rd32(r + 20), type});
            }
        }
    }
    return H;
}
extern "C" void host_free(void *h) { delete static_cast<Host *>(h); }
// out: records, live, packs, keep, drop, repack, kept_rows, repack_rows, live_bytes, reclaimable, missing
extern "C" int host_mark_sweep(void *h, const uint8_t *refs, uint64_t nrefs, uint32_t keep_types, uint32_t permille,
                               uint64_t *out, double *seconds)
{
    Host *H = static_cast<Host *>(h);
    const double t0 = now();
    H->marks.assign(H->recs.size(), 0);
    uint64_t missing = 0;
    for (uint64_t i = 0; i < nrefs; ++i) {
        const uint8_t *r = refs + 33 * i;
        if (r[0] >= splan::kTypes) return -1;
        splan::Sum key;
        memcpy(key.b, r + 1, 32);
        const auto it = H->index[r[0]].find(key);
        if (it == H->index[r[0]].end()) ++missing;
        else H->marks[it->second] = 1;
    }
    const double t1 = now();
    std::vector<Pack> packs(H->pack_sum.size(), Pack{nullptr, 0, 0, 0, ~0ull, 0});
    std::vector<uint8_t> live(H->recs.size(), 0);
    uint64_t nlive = 0;
    for (uint64_t r = 0; r < H->recs.size(); ++r) {
        const Rec &R = H->recs[r];
        Pack &P = packs[R.pack];
        if (P.first == ~0ull) P.first = r, P.sum = H->pack_sum[R.pack];
        P.extent = std::max<uint64_t>(P.extent, uint64_t(R.offset) + R.length);
        splan::Sum key;
        memcpy(key.b, R.sum, 32);
        const bool winner = H->index[R.type].find(key)->second == r;
        if (winner && (H->marks[r] || (keep_types >> R.type & 1))) {
            live[r] = 1, ++nlive;
            ++P.live_rows, P.live_bytes += R.length;
        }
    }
    uint64_t nv[3] = {0, 0, 0}, live_bytes = 0, reclaim = 0;
    std::vector<cdc_sweep_pack> list(packs.size(), cdc_sweep_pack{});
    for (size_t p = 0; p < packs.size(); ++p) {  // packs are numbered in first-record order already
        Pack &P = packs[p];
        P.verdict = swplan::verdict(P.live_rows, P.live_bytes, P.extent, permille);
        ++nv[P.verdict], live_bytes += P.live_bytes;
        if (P.verdict != CDC_SWEEP_KEEP) reclaim += P.extent - P.live_bytes;
        memcpy(list[p].packfile, P.sum, 32);
        list[p].extent = P.extent, list[p].live_bytes = P.live_bytes, list[p].live_rows = P.live_rows;
        list[p].first_record = P.first, list[p].verdict = P.verdict;
    }
    std::vector<cdc_state_row> kept, repack;
    for (uint64_t r = 0; r < H->recs.size(); ++r) {
        if (!live[r]) continue;
        const Rec &R = H->recs[r];
        cdc_state_row row{};
        memcpy(row.checksum, R.sum, 32), memcpy(row.packfile, H->pack_sum[R.pack], 32);
        row.offset = R.offset, row.length = R.length, row.type = uint8_t(R.type), row.found = 1;
        (packs[R.pack].verdict == CDC_SWEEP_KEEP ? kept : repack).push_back(row);
    }
    if (swplan::group_repack(repack.data(), repack.size(), list.data(), list.size()) != CDC_OK) return -1;
    const double t2 = now();
    out[0] = H->recs.size(), out[1] = nlive, out[2] = packs.size(), out[3] = nv[0], out[4] = nv[1], out[5] = nv[2];
    out[6] = kept.size(), out[7] = repack.size(), out[8] = live_bytes, out[9] = reclaim, out[10] = missing;
    seconds[0] = t1 - t0, seconds[1] = t2 - t1;
    return 0;
}
"""

COMPARED = ("records", "live", "packs", "keep", "drop", "repack", "kept_rows", "repack_rows", "live_bytes",
            "reclaimable_bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,16000000")
    ap.add_argument("--states", type=int, default=64)
    ap.add_argument("--live", default="50,95", help="percent of the rows that are referenced")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--permille", type=int, default=500)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maintenance_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401 - its HIP runtime comes up before the library's

    from state_bench import make_state, med
    from plakar_amd import _lib, state
    L = _lib.lib()
    host = None
    if not a.no_host:
        work = tempfile.mkdtemp(prefix="maintenance_bench_")
        src, so = os.path.join(work, "host_maint.cpp"), os.path.join(work, "host_maint.so")
        with open(src, "w") as f:
            f.write(HOST_SRC)
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "plakar_amd", "csrc"), "-o", so, src], check=True)
        host = ctypes.CDLL(so)
        host.host_build.restype = ctypes.c_void_p
        host.host_build.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        host.host_free.argtypes = [ctypes.c_void_p]
        host.host_mark_sweep.restype = ctypes.c_int
        host.host_mark_sweep.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                         ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)
        if a.out:  # rewritten after every measurement: a run that is cut short keeps what it had
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(dict(reps=a.reps, states=a.states, permille=a.permille, measurements=lines), f, indent=1)
                f.write("\n")

    def note(text):
        print(f"[maintenance_bench] {text}", file=sys.stderr, flush=True)

    for total in [int(x) for x in a.rows.split(",")]:
        note(f"{total} rows in {a.states} states: generating")
        rng = np.random.default_rng(total + a.states)
        per = total // a.states
        plains, blob_sums = [], []
        for _ in range(a.states):
            p, s = make_state(np, rng, per)
            plains.append(p)
            blob_sums.append(s)
        rows = per * a.states
        sums = np.concatenate(blob_sums)
        base = np.frombuffer(b"".join(plains), dtype=np.uint8)
        lens = np.array([len(p) for p in plains], dtype=np.uint64)
        offs = (np.cumsum(lens) - lens).astype(np.uint64)
        note("merge")
        S = state.State(key=None, compression=None)
        t0 = time.perf_counter()
        assert S.merge(plains, ids=[bytes([i % 256, i // 256]) + bytes(30) for i in range(a.states)], form="plain") == [0] * a.states
        merge_s = time.perf_counter() - t0
        del plains
        H = None
        if host is not None:
            note("host index")
            t0 = time.perf_counter()
            H = host.host_build(base.ctypes.data, offs.ctypes.data, lens.ctypes.data, a.states)
            host_build_s = time.perf_counter() - t0
            assert H
        for pct in [int(x) for x in a.live.split(",")]:
            pick = rng.permutation(rows)[:rows * pct // 100]
            twice = np.concatenate([pick, pick])
            rng.shuffle(twice)
            refs = np.empty((len(twice), 33), dtype=np.uint8)
            refs[:, 0] = state.TYPE_CHUNK
            refs[:, 1:] = sums[twice]
            nrefs = len(refs)
            note(f"{pct}% live: {nrefs} references")
            mark, sweep, fetch = [], [], []
            stages = dict(packs_s=[], sweep_s=[], verdict_s=[], compact_s=[], download_s=[])
            info = None
            for r in range(a.reps + 1):
                S.clear_marks()
                missing = ctypes.c_uint64()
                t0 = time.perf_counter()
                rc = L.cdc_state_mark(S._h, refs.ctypes.data, nrefs, None, ctypes.byref(missing))
                t1 = time.perf_counter()
                assert rc == 0 and missing.value == 0
                o = _lib.cdc_sweep_opts()
                L.cdc_sweep_default_opts(ctypes.byref(o))
                o.repack_permille = a.permille
                h = ctypes.c_void_p()
                t2 = time.perf_counter()
                rc = L.cdc_state_sweep(S._h, ctypes.byref(o), ctypes.byref(h))
                t3 = time.perf_counter()
                assert rc == 0
                plan = state.SweepPlan._from_handle(h)
                t4 = time.perf_counter()
                L.cdc_sweep_free(h)
                info = plan.info
                assert info["live"] == len(pick) and info["kept_rows"] + info["repack_rows"] == len(pick)
                if r:
                    mark.append(t1 - t0)
                    sweep.append(t3 - t2)
                    fetch.append(t4 - t3)
                    for name in stages:
                        stages[name].append(info[name])
                del plan
            line = dict(what="maintenance", rows=rows, states=a.states, live_percent=pct, references=nrefs, permille=a.permille,
                        merge_s=merge_s, mark_s=med(mark), references_per_s=nrefs / statistics.median(mark),
                        sweep_call_s=med(sweep), records_per_s=rows / statistics.median(sweep), plan_copy_s=med(fetch),
                        plan={k: info[k] for k in COMPARED}, **{n: med(v) for n, v in stages.items()})
            line["sweep_kernels_s"] = sum(statistics.median(stages[n]) for n in ("packs_s", "sweep_s", "verdict_s", "compact_s"))
            if H is not None:
                hm, hs = [], []
                out, secs = (ctypes.c_uint64 * 11)(), (ctypes.c_double * 2)()
                for r in range(a.reps + 1):
                    assert host.host_mark_sweep(H, refs.ctypes.data, nrefs, 1, a.permille, out, secs) == 0
                    if r:
                        hm.append(secs[0])
                        hs.append(secs[1])
                assert dict(zip(COMPARED, list(out)[:10])) == line["plan"] and out[10] == 0, (list(out), line["plan"])
                line.update(host_index_s=host_build_s, host_mark_s=med(hm), host_sweep_s=med(hs),
                            device_over_host_mark=statistics.median(hm) / statistics.median(mark),
                            device_over_host_sweep=statistics.median(hs) / statistics.median(sweep),
                            device_over_host_both=(statistics.median(hm) + statistics.median(hs)) /
                            (statistics.median(mark) + statistics.median(sweep)))
            emit(line)
        if H is not None:
            host.host_free(H)
        S.close()


if __name__ == "__main__":
    main()
