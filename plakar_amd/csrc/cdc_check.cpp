// cdc_object_digests_device and cdc_check_*: a snapshot's chunks and object
// checksums verified on the device (include/plakar_cdc.h, "check").
//
// The reference checks one chunk at a time: snapshot/check.go:56-113 reads
// every chunk of a file (one GetBlob: a ranged packfile read and one Decode),
// hashes it, compares it with Chunk.Checksum and feeds it into a second
// hasher whose sum must be Object.Checksum.  Here a run is restore's pipeline
// over batches of file bytes (restore_plan.h) without an output image:
//
//   reader   gathers the batch's distinct encoded blobs and uploads them
//            (cdc_reader.h: gather, on `threads` threads);
//   device   (the calling thread) the shared decode step over the distinct
//            blobs (cdc_reader.h: decode_batch); the
//            objects the device takes are hashed by k_object_digest where
//            their blobs lie (check_plan.h: runs and seam copies), the bytes
//            of the others are gathered by cdc_assemble_device into a staging
//            image;
//   hasher   downloads the staging image, hashes the host's objects and
//            pieces on `threads` threads, compares and makes the callbacks.
//
// Two input slots and two staging slots rotate: batch k + 1 is read and
// uploaded while batch k is on the device and batch k - 1's host-bound
// objects are hashed.  A file that spans batches keeps one incremental
// cdc::Sha256 on the host; the device keeps no midstate between batches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "cdc_reader.h"
#include "check_plan.h"
#include "restore_plan.h"

namespace {

using cdc::Clock;
using cdc::parallel_for;
using cdc::since;

constexpr uint64_t kMaxBatch = 1ull << 30;

// cdc_object_digests_device's per-device scratch: the records and runs (pinned
// and device) and the seam area, kept across calls and grown on demand.
struct ObjScratch {
    std::mutex mu;
    cdc::PinBuf h;
    cdc::DevBuf d, seam;
};
ObjScratch &obj_scratch(int device)
{
    static ObjScratch *s = new ObjScratch[cdc::kMaxDevices];  // never destroyed (DevBuf)
    return s[unsigned(device) % cdc::kMaxDevices];
}

}  // namespace

int cdc::object_digests(int device, const void *d_data, uint64_t len, const uint64_t *seg_off, const uint64_t *seg_len,
                        uint64_t nsegs, const uint64_t *obj_seg0, uint32_t n, uint8_t *d_digests, void *stream,
                        uint64_t *seam_bytes)
{
    if (seam_bytes) *seam_bytes = 0;
    if (n == 0) return CDC_OK;
    (void)nsegs;
    cplan::Runs P;
    cplan::plan_runs(seg_off, seg_len, obj_seg0, n, P);
    if (seam_bytes) *seam_bytes = P.seam_bytes;
    if (hipSetDevice(device) != hipSuccess) return CDC_E_DEVICE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ObjScratch &S = obj_scratch(device);
    std::lock_guard<std::mutex> lk(S.mu);
    static_assert(sizeof(cdc::ObjRun) == sizeof(cplan::Run), "the planner's runs are the kernel's");
    const size_t rec_bytes = size_t(n) * sizeof(cdc::ObjRec), run_bytes = P.runs.size() * sizeof(cdc::ObjRun);
    const uint64_t seam_cap = P.seam_bytes + 64;
    if (!S.h.reserve(rec_bytes + run_bytes) || !S.d.reserve(rec_bytes + run_bytes) || !S.seam.reserve(seam_cap))
        return CDC_E_NOMEM;
    cdc::ObjRec *rec = S.h.as<cdc::ObjRec>();
    for (uint32_t i = 0; i < n; ++i)
        rec[i] = cdc::ObjRec{P.total[i], P.run0[i], P.run0[size_t(i) + 1] - P.run0[i], 0};
    std::memcpy(S.h.as<uint8_t>() + rec_bytes, P.runs.data(), run_bytes);
    // from the first enqueue on, every return drains the stream: the scratch is the next call's
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{st};
    if (hipMemcpyAsync(S.d.data(), S.h.data(), rec_bytes + run_bytes, hipMemcpyHostToDevice, st) != hipSuccess)
        return CDC_E_DEVICE;
    if (!P.copies.empty()) {
        std::vector<uint64_t> so(P.copies.size()), sl(P.copies.size()), sd(P.copies.size());
        for (size_t c = 0; c < P.copies.size(); ++c) {
            so[c] = P.copies[c].src_off;
            sl[c] = P.copies[c].len;
            sd[c] = P.copies[c].dst_off;
        }
        const int s2 = cdc_assemble_device(device, d_data, len, so.data(), sl.data(), sd.data(), so.size(), S.seam.data(),
                                           seam_cap, stream);
        if (s2 != CDC_OK) return s2;
    }
    cdc::ObjBatch B{};
    B.data = static_cast<const uint8_t *>(d_data);
    B.len = len;
    B.seam = S.seam.as<uint8_t>();
    B.seam_len = P.seam_bytes;
    B.objs = S.d.as<cdc::ObjRec>();
    B.n = n;
    B.runs = reinterpret_cast<const cdc::ObjRun *>(S.d.as<uint8_t>() + rec_bytes);
    B.nruns = P.runs.size();
    B.digests = d_digests;
    const int s3 = cdc::launch_object_digests(B, stream);
    if (s3 != CDC_OK) return s3;
    return hipStreamSynchronize(st) == hipSuccess ? CDC_OK : CDC_E_DEVICE;
}

namespace {

using InSlot = cdc::Arena;  // reader -> device stage
struct OutSlot {  // device stage -> hasher: the staging image of the host's objects and pieces
    cdc::DevBuf d;
    cdc::PinBuf h;
    std::vector<uint32_t> piece;       // index into the batch's pieces
    std::vector<uint64_t> off;         // where that piece's bytes start in the image
    uint64_t bytes = 0;
};

}  // namespace

struct cdc_check {
    cdc::PackSource src;  // device, codec, locator, run lock
    cdc_check_opts o{};
    hipStream_t stream[3] = {nullptr, nullptr, nullptr};  // upload, device stages, download
    InSlot in[2];
    OutSlot out[2];
    cdc::DevBuf plain, dig;
    cdc::PinBuf hdig;
};

namespace {

struct Run {
    cdc_check *R;
    const cdc_check_file *files;
    int n;
    cdc_check_file_fn on_file;
    void *ctx;
    std::vector<rplan::Batch> batches;
    std::vector<std::vector<uint32_t>> fblob;  // planned file -> its chunks' blob ids
    std::vector<rplan::File> pf;
    std::vector<int> pidx;                     // planned file -> index in files
    std::unique_ptr<std::atomic<int>[]> fstatus;
    std::vector<int64_t> fbad;
    std::vector<uint8_t> reported, fhashed;
    std::vector<uint64_t> fsize;
    std::vector<std::array<uint8_t, 32>> fsum;
    std::vector<cdc::Sha256> fsha;             // the host's incremental hasher of a file
    cdc::Handoff hand;  // the stages' hand-offs: counts of batches past each point
    int uploaded = 0, consumed = 0, staged = 0, hashed = 0;
    cdc_check_stats st{};
    double gather_s = 0;  // the device stage's share of d2h_s

    // the first failure of a file stays (the device stage meets chunks in file order)
    void fail_file(int fi, int status, int64_t chunk)
    {
        int ok = CDC_OK;
        if (fstatus[fi].compare_exchange_strong(ok, status)) fbad[size_t(fi)] = chunk;
    }
    void report(int fi)
    {
        reported[size_t(fi)] = 1;
        const int s = fstatus[fi].load();
        st.failed_files += s != CDC_OK;
        if (!on_file) return;
        cdc_check_result r{};
        r.index = fi;
        r.status = s;
        r.bad_chunk = s != CDC_OK ? fbad[size_t(fi)] : -1;
        r.hashed = fhashed[size_t(fi)];
        if (r.hashed) std::memcpy(r.checksum, fsum[size_t(fi)].data(), 32);
        r.size = fsize[size_t(fi)];
        on_file(ctx, &r);
    }
};

// ---- reader stage ----------------------------------------------------------------------
static void reader_stage(Run &X)
{
    cdc_check *R = X.R;
    if (hipSetDevice(R->src.device) != hipSuccess) return X.hand.abort_run(CDC_E_DEVICE);
    for (int k = 0; k < int(X.batches.size()); ++k) {
        if (!X.hand.wait_for(X.consumed, k - 1)) return;  // batch k - 2 has left this input slot
        InSlot &S = R->in[k & 1];
        S.set_blobs(R->src.loc, X.batches[k].blobs.data(), X.batches[k].blobs.size());
        const int st = cdc::gather(R->src.loc, S, R->o.threads, R->stream[0], &X.st.read_s, &X.st.h2d_s, &X.st.encoded_bytes);
        if (st != CDC_OK) return X.hand.abort_run(st);
        X.hand.advance(X.uploaded);
    }
}

// ---- device stage (the calling thread) ---------------------------------------------
static void device_stage(Run &X)
{
    cdc_check *R = X.R;
    std::vector<uint64_t> so, sl, sd, lens, obj_seg0;
    std::vector<uint8_t> to_host;
    cdc::Decoded D;
    const std::vector<int32_t> &bst = D.bst;
    const std::vector<uint64_t> &pos = D.pos;
    const cdc::DecodeCtx C{R->src.device, R->src.compress, R->src.key_ptr(), true, R->stream[1]};
    const cdc::DecodeTally T{&X.st.decoded_bytes, &X.st.decode_s, &X.st.verify_s};
    std::vector<uint32_t> single, dev_piece;
    const double rate = R->o.host_min_len ? 0.0 : cdc::host_sha256_rate();
    for (int k = 0; k < int(X.batches.size()); ++k) {
        if (!X.hand.wait_for(X.uploaded, k + 1) || !X.hand.wait_for(X.hashed, k - 1)) return;
        const rplan::Batch &B = X.batches[k];
        InSlot &I = R->in[k & 1];
        OutSlot &O = R->out[k & 1];
        const uint32_t nb = uint32_t(B.blobs.size());
        if (!R->plain.reserve(B.plain_bytes)) return X.hand.abort_run(CDC_E_NOMEM);
        uint8_t *const plain = R->plain.as<uint8_t>();
        D.set_blobs(true, R->src.loc, B.blobs.data(), nb);
        int st = cdc::decode_batch(C, I, plain, B.plain_bytes, D, T);
        if (st != CDC_OK) return X.hand.abort_run(st);
        const uint64_t plain_used = D.plain_used;
        X.hand.advance(X.consumed);
        // objects with a failed blob are settled, not hashed
        for (const rplan::Piece &P : B.pieces)
            for (uint64_t s = P.seg0; s < P.seg0 + P.nchunks; ++s)
                if (bst[B.segs[s].blob] != CDC_OK) {
                    X.fail_file(X.pidx[P.file], bst[B.segs[s].blob], int64_t(P.chunk0 + (s - P.seg0)));
                    break;
                }
        // the split: whole files of this batch by the model or host_min_len, pieces of longer files to the host
        single.clear();
        lens.clear();
        O.piece.clear();
        O.off.clear();
        O.bytes = 0;
        for (uint32_t p = 0; p < B.pieces.size(); ++p) {
            const rplan::Piece &P = B.pieces[p];
            if (X.fstatus[X.pidx[P.file]].load() != CDC_OK) continue;
            if (P.first && P.last) {
                single.push_back(p);
                lens.push_back(P.len);
            } else {
                O.piece.push_back(p);
            }
        }
        cplan::split(lens.data(), lens.size(), R->o.threads, R->o.host_min_len, rate, to_host);
        dev_piece.clear();
        for (size_t j = 0; j < single.size(); ++j) (to_host[j] ? O.piece : dev_piece).push_back(single[j]);
        std::sort(O.piece.begin(), O.piece.end());
        if (!dev_piece.empty()) {  // hashed where the blobs lie
            const auto t0 = Clock::now();
            so.clear();
            sl.clear();
            obj_seg0.assign(1, 0);
            for (uint32_t p : dev_piece) {
                const rplan::Piece &P = B.pieces[p];
                for (uint64_t s = P.seg0; s < P.seg0 + P.nchunks; ++s) {
                    so.push_back(pos[B.segs[s].blob]);
                    sl.push_back(B.segs[s].len);
                }
                obj_seg0.push_back(so.size());
            }
            const size_t nd = dev_piece.size(), dig_bytes = nd * 32;
            if (!R->dig.reserve(dig_bytes) || !R->hdig.reserve(dig_bytes)) return X.hand.abort_run(CDC_E_NOMEM);
            uint64_t seam = 0;
            if (!cplan::segments_valid(so.data(), sl.data(), so.size(), obj_seg0.data(), nd, plain_used))
                return X.hand.abort_run(CDC_E_DEVICE);  // the planner's places are inside what Decode wrote
            st = cdc::object_digests(R->src.device, plain, plain_used, so.data(), sl.data(), so.size(), obj_seg0.data(),
                                     uint32_t(nd), R->dig.as<uint8_t>(), R->stream[1], &seam);
            if (st != CDC_OK) return X.hand.abort_run(st);
            if (hipMemcpyAsync(R->hdig.data(), R->dig.data(), dig_bytes, hipMemcpyDeviceToHost, R->stream[1]) != hipSuccess ||
                hipStreamSynchronize(R->stream[1]) != hipSuccess)
                return X.hand.abort_run(CDC_E_DEVICE);
            for (size_t j = 0; j < nd; ++j) {
                const int fi = X.pidx[B.pieces[dev_piece[j]].file];
                std::memcpy(X.fsum[size_t(fi)].data(), R->hdig.as<uint8_t>() + 32 * j, 32);
                X.fhashed[size_t(fi)] = 1;
            }
            X.st.seam_bytes += seam;
            X.st.digest_s += since(t0);
        }
        if (!O.piece.empty()) {  // the host's bytes, gathered for one copy back
            const auto t0 = Clock::now();
            so.clear();
            sl.clear();
            sd.clear();
            for (uint32_t p : O.piece) {
                const rplan::Piece &P = B.pieces[p];
                O.off.push_back(O.bytes);
                for (uint64_t s = P.seg0; s < P.seg0 + P.nchunks; ++s) {
                    so.push_back(pos[B.segs[s].blob]);
                    sl.push_back(B.segs[s].len);
                    sd.push_back(O.bytes);
                    O.bytes += B.segs[s].len;
                }
            }
            if (!O.d.reserve(O.bytes) || !O.h.reserve(O.bytes)) return X.hand.abort_run(CDC_E_NOMEM);
            if (O.bytes) {
                st = cdc_assemble_device(R->src.device, plain, plain_used, so.data(), sl.data(), sd.data(), so.size(),
                                         O.d.data(), O.bytes, R->stream[1]);
                if (st != CDC_OK) return X.hand.abort_run(st);
                if (hipStreamSynchronize(R->stream[1]) != hipSuccess) return X.hand.abort_run(CDC_E_DEVICE);
            }
            X.gather_s += since(t0);
        }
        X.hand.advance(X.staged);
    }
}

// ---- hasher stage -------------------------------------------------------------------
static void hasher_stage(Run &X)
{
    cdc_check *R = X.R;
    if (hipSetDevice(R->src.device) != hipSuccess) return X.hand.abort_run(CDC_E_DEVICE);
    for (int k = 0; k < int(X.batches.size()); ++k) {
        if (!X.hand.wait_for(X.staged, k + 1)) return;
        const rplan::Batch &B = X.batches[k];
        OutSlot &O = R->out[k & 1];
        const uint8_t *const image = O.h.as<uint8_t>();
        auto t0 = Clock::now();
        if (O.bytes && (hipMemcpyAsync(O.h.data(), O.d.data(), O.bytes, hipMemcpyDeviceToHost, R->stream[2]) != hipSuccess ||
                        hipStreamSynchronize(R->stream[2]) != hipSuccess))
            return X.hand.abort_run(CDC_E_DEVICE);
        X.st.d2h_s += since(t0);
        t0 = Clock::now();
        // a file has one piece per batch at most: the pieces hash side by side
        parallel_for(R->o.threads, O.piece.size(), [&](size_t j) {
            const rplan::Piece &P = B.pieces[O.piece[j]];
            const int fi = X.pidx[P.file];
            if (X.fstatus[fi].load() != CDC_OK) return;  // a later batch's blob has failed it meanwhile
            X.fsha[size_t(fi)].update(image + O.off[j], size_t(P.len));
            if (P.last) {
                X.fsha[size_t(fi)].final(X.fsum[size_t(fi)].data());
                X.fhashed[size_t(fi)] = 2;
            }
        });
        X.st.hash_s += since(t0);
        for (const rplan::Piece &P : B.pieces) {
            if (!P.last) continue;
            const int fi = X.pidx[P.file];
            const uint8_t *rec = X.files[fi].object_checksum;
            if (X.fstatus[fi].load() != CDC_OK) {
                X.fhashed[size_t(fi)] = 0;
            } else if (X.fhashed[size_t(fi)]) {
                const bool dev = X.fhashed[size_t(fi)] == 1;
                ++(dev ? X.st.device_objects : X.st.host_objects);
                (dev ? X.st.device_bytes : X.st.host_bytes) += X.fsize[size_t(fi)];
                if (rec && std::memcmp(rec, X.fsum[size_t(fi)].data(), 32) != 0) X.fail_file(fi, CDC_E_MISMATCH, -1);
            } else {
                X.fail_file(fi, CDC_E_DEVICE, -1);  // never reached: every fine file was hashed somewhere
            }
            X.report(fi);
        }
        X.hand.advance(X.hashed);
    }
}

static void write_stats(cdc_check_stats *stats, cdc_check_stats &st)
{
    if (!stats) return;
    st.struct_size = uint32_t(std::min<size_t>(stats->struct_size, sizeof(st)));
    std::memcpy(stats, &st, st.struct_size);
}

static int run_files(cdc_check *R, const cdc_check_file *files, int n, cdc_check_file_fn on_file, void *ctx,
                     cdc_check_stats *stats)
{
    const auto w0 = Clock::now();
    Run X{};
    X.R = R;
    X.files = files;
    X.n = n;
    X.on_file = on_file;
    X.ctx = ctx;
    X.fstatus.reset(new std::atomic<int>[size_t(std::max(n, 1))]);
    X.fbad.assign(size_t(n), -1);
    X.reported.assign(size_t(n), 0);
    X.fhashed.assign(size_t(n), 0);
    X.fsize.assign(size_t(n), 0);
    X.fsum.resize(size_t(n));
    X.st.files = uint64_t(n);
    // the locator: every chunk's blob id, or CDC_E_NOTFOUND with the first missing index
    for (int i = 0; i < n; ++i) {
        X.fstatus[i].store(CDC_OK);
        const cdc_check_file &F = files[i];
        std::vector<uint32_t> ids(size_t(F.nchunks));  // a fast run only asks whether they are there
        const int64_t miss = cdc::resolve(R->src.loc, F.checksums, F.nchunks, ids.data());
        if (miss >= 0) X.fail_file(i, CDC_E_NOTFOUND, miss);
        for (uint64_t c = 0; c < F.nchunks; ++c) X.fsize[size_t(i)] += F.lengths[c];
        if (R->o.fast || X.fstatus[i].load() != CDC_OK) {
            X.report(i);
            continue;
        }
        X.fblob.push_back(std::move(ids));
        X.pidx.push_back(i);
    }
    if (!R->o.fast) {
        for (size_t p = 0; p < X.pidx.size(); ++p)
            X.pf.push_back(rplan::File{files[X.pidx[p]].nchunks, X.fblob[p].data(), files[X.pidx[p]].lengths});
        rplan::plan(X.pf.data(), X.pf.size(), R->o.batch_bytes, X.batches);
        std::vector<bool> used(R->src.loc.locs.size(), false);
        for (const rplan::Batch &B : X.batches) {
            X.st.bytes += B.out_bytes;
            X.st.segments += B.segs.size();
            X.st.decoded_blobs += B.blobs.size();
            for (const rplan::Blob &b : B.blobs)
                if (!used[b.id]) {
                    used[b.id] = true;
                    ++X.st.distinct_blobs;
                }
            X.st.pieces += B.pieces.size();
        }
        X.st.batches = X.batches.size();
        X.fsha.resize(size_t(n));
    }
    if (!X.batches.empty()) {
        if (hipSetDevice(R->src.device) != hipSuccess) return CDC_E_DEVICE;
        auto guarded = [&X](void (*stage)(Run &)) {
            try {
                stage(X);
            } catch (...) {
                X.hand.abort_run(CDC_E_NOMEM);
            }
        };
        std::thread reader(guarded, reader_stage);
        std::thread hasher(guarded, hasher_stage);
        guarded(device_stage);
        reader.join();
        hasher.join();
    }
    // a run that broke off: the files it did not finish fail with its status
    for (int i = 0; i < n; ++i)
        if (!X.reported[size_t(i)]) {
            X.fhashed[size_t(i)] = 0;
            X.fstatus[i].store(X.hand.fail != CDC_OK ? X.hand.fail : CDC_E_DEVICE);
            X.report(i);
        }
    X.st.d2h_s += X.gather_s;
    X.st.wall_s = since(w0);
    write_stats(stats, X.st);
    return X.hand.fail;
}

}  // namespace

extern "C" {

int cdc_object_digests_device(int device, const void *d_data, uint64_t len, const uint64_t *seg_off,
                              const uint64_t *seg_len, uint64_t nsegs, const uint64_t *obj_seg0, uint32_t n,
                              uint8_t *d_digests, void *stream)
{
    if (device < 0 || device >= cdc::kMaxDevices || !obj_seg0 || (nsegs && (!seg_off || !seg_len)) || (len && !d_data) ||
        (n && !d_digests) || (reinterpret_cast<uintptr_t>(d_digests) & 15u))
        return CDC_E_INVALID;
    if (!cplan::segments_valid(seg_off, seg_len, nsegs, obj_seg0, n, len)) return CDC_E_INVALID;
    if (!cdc::device_count_initialised()) return CDC_E_NOT_INIT;
    try {
        return cdc::object_digests(device, d_data, len, seg_off, seg_len, nsegs, obj_seg0, n, d_digests, stream, nullptr);
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

void cdc_check_default_opts(cdc_check_opts *out)
{
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
}

int cdc_check_new(int device, const cdc_check_opts *opts, cdc_check **out)
{
    if (!opts || !out) return CDC_E_INVALID;
    *out = nullptr;
    if (opts->struct_size != sizeof(*opts) || device < 0 || device >= cdc::kMaxDevices || opts->threads < 0 ||
        opts->threads > 256 || opts->batch_bytes > kMaxBatch ||
        (opts->compress != CDC_COMPRESS_NONE && opts->compress != CDC_COMPRESS_LZ4 && opts->compress != CDC_COMPRESS_GZIP))
        return CDC_E_INVALID;
    if (!cdc::device_count_initialised()) return CDC_E_NOT_INIT;
    auto *c = new (std::nothrow) cdc_check();
    if (!c) return CDC_E_NOMEM;
    try {
        c->src.open(device, opts->compress, opts->key);
        c->o = *opts;
        c->o.key = nullptr;
        if (!c->o.threads) c->o.threads = 8;
        if (!c->o.batch_bytes) c->o.batch_bytes = 256ull << 20;
    } catch (...) {
        delete c;
        return CDC_E_NOMEM;
    }
    if (!c->o.fast) {  // a fast context never touches the device
        bool ok = hipSetDevice(device) == hipSuccess;
        for (int i = 0; i < 3; ++i) ok = ok && hipStreamCreateWithFlags(&c->stream[i], hipStreamNonBlocking) == hipSuccess;
        if (!ok) {
            cdc_check_free(c);
            return CDC_E_DEVICE;
        }
    }
    *out = c;
    return CDC_OK;
}

int cdc_check_add_packfile(cdc_check *c, const uint8_t *bytes, uint64_t len)
{
    return c && (bytes || !len) ? c->src.add_memory(bytes, len) : CDC_E_INVALID;
}

int cdc_check_add_packfile_path(cdc_check *c, const char *path)
{
    return c && path ? c->src.add_path(path) : CDC_E_INVALID;
}

int cdc_check_add_packfiles(cdc_check *c, const cdc_packfile_src *srcs, uint32_t n, int32_t *status)
{
    return c ? c->src.add_many(srcs, n, status) : CDC_E_INVALID;
}

int cdc_check_files(cdc_check *c, const cdc_check_file *files, int n, cdc_check_file_fn on_file, void *ctx,
                    cdc_check_stats *stats)
{
    if (!c || n < 0 || (n && !files) || (stats && stats->struct_size < 8)) return CDC_E_INVALID;
    for (int i = 0; i < n; ++i)
        if (files[i].nchunks && (!files[i].checksums || !files[i].lengths)) return CDC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->src.run_mu);
    try {
        return run_files(c, files, n, on_file, ctx, stats);
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

void cdc_check_free(cdc_check *c)
{
    if (!c) return;
    c->src.release(c->stream, 3);
    delete c;  // the slots' buffers go with it, the streams drained above
}

}  // extern "C"
