// cdc_restore_*: packfiles in, files out (include/plakar_cdc.h, "restore").
//
// The reference restores one chunk at a time: snapshot/restore.go:103-110 opens
// a reader per file, snapshot/vfs/vfilep.go:58-122 serves Read by one
// repo.GetBlob per chunk, repository/repository.go:449-466 looks the checksum
// up (GetSubpartForBlob) and repository.go:407-429 does one ranged packfile
// read and one Decode; a chunk that occurs twice is decoded twice and nothing
// is verified.  Here a run is a pipeline over batches of output bytes planned
// up front (restore_plan.h), three stages on three threads and three streams:
//
//   reader   gathers the batch's distinct encoded blobs and uploads them
//            (cdc_reader.h: gather, on `writers` threads);
//   device   (the calling thread) the shared decode step over the distinct
//            blobs (cdc_reader.h: decode_together, decode_one_by_one), then
//            cdc_assemble_device into the batch's output image, or nothing
//            when the plaintext buffer already is that image;
//   writer   downloads the image into a pinned slot, pwrites every piece
//            (`writers` threads) and makes the callbacks.
//
// Two input slots and two output slots rotate: batch k + 1 is read and
// uploaded while batch k is on the device and batch k - 1 is downloaded and
// written.  Decode is synchronous and holds the per-device workspace, so the
// device stages of two batches never overlap.
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "cdc_reader.h"
#include "read_plan.h"
#include "restore_plan.h"

namespace {

using cdc::Clock;
using cdc::parallel_for;
using cdc::pwrite_all;
using cdc::since;
using InSlot = cdc::Arena;  // reader -> device stage

struct OutSlot {  // device stage -> writer
    cdc::DevBuf d;
    cdc::PinBuf h;
};

}  // namespace

struct cdc_restore {
    cdc::PackSource src;  // device, codec, locator, run lock
    cdc_restore_opts o{};
    hipStream_t stream[3] = {nullptr, nullptr, nullptr};  // upload, device stages, download
    InSlot in[2];
    OutSlot out[2];
    cdc::DevBuf plain;
};

namespace {

struct Run {
    cdc_restore *R;
    const cdc_restore_file *files;
    int n;
    cdc_restore_file_fn on_file;
    void *ctx;
    std::vector<rplan::Batch> batches;
    std::vector<std::vector<uint32_t>> fblob;  // planned file -> its chunks' blob ids
    std::vector<rplan::File> pf;
    std::vector<int> pidx;                     // planned file -> index in files
    std::unique_ptr<std::atomic<int>[]> fstatus;
    std::vector<uint8_t> created, reported;
    std::vector<uint64_t> fsize;
    std::vector<uint32_t> fpieces, fseen;
    // the stages' hand-offs: counts of batches past each point
    cdc::Handoff hand;
    int uploaded = 0, consumed = 0, assembled = 0, written = 0;
    cdc_restore_stats st{};
    double read_s = 0, h2d_s = 0, decode_s = 0, verify_s = 0, assemble_s = 0, d2h_s = 0, write_s = 0;

    void fail_file(int fi, int status)
    {
        int ok = CDC_OK;
        fstatus[fi].compare_exchange_strong(ok, status);
    }
    void report(int fi, int status, uint32_t piece, uint32_t pieces, const uint8_t *data, uint64_t off, uint64_t len)
    {
        if (!on_file) return;
        cdc_restore_result r{};
        r.index = fi;
        r.status = status;
        r.size = fsize[fi];
        r.piece = piece;
        r.pieces = pieces;
        r.data = data;
        r.data_offset = off;
        r.data_len = len;
        on_file(ctx, &r);
    }
};

// ---- reader stage ---------------------------------------------------------------
static void reader_stage(Run &X)
{
    cdc_restore *R = X.R;
    if (hipSetDevice(R->src.device) != hipSuccess) return X.hand.abort_run(CDC_E_DEVICE);
    for (int k = 0; k < int(X.batches.size()); ++k) {
        if (!X.hand.wait_for(X.consumed, k - 1)) return;  // batch k - 2 has left this input slot
        InSlot &S = R->in[k & 1];
        S.set_blobs(R->src.loc, X.batches[k].blobs.data(), X.batches[k].blobs.size());
        const int st = cdc::gather(R->src.loc, S, R->o.writers, R->stream[0], &X.read_s, &X.h2d_s, &X.st.encoded_bytes);
        if (st != CDC_OK) return X.hand.abort_run(st);
        X.hand.advance(X.uploaded);
    }
}

// ---- device stage (the calling thread) --------------------------------------------
static void device_stage(Run &X)
{
    cdc_restore *R = X.R;
    std::vector<uint64_t> so, sl, sd;
    cdc::Decoded D;
    const std::vector<int32_t> &bst = D.bst;
    const cdc::DecodeCtx C{R->src.device, R->src.compress, R->src.key_ptr(), R->o.verify != 0, R->stream[1]};
    const cdc::DecodeTally T{&X.st.decoded_bytes, &X.decode_s, &X.verify_s};
    for (int k = 0; k < int(X.batches.size()); ++k) {
        if (!X.hand.wait_for(X.uploaded, k + 1) || !X.hand.wait_for(X.written, k - 1)) return;
        const rplan::Batch &B = X.batches[k];
        InSlot &I = R->in[k & 1];
        OutSlot &O = R->out[k & 1];
        const uint32_t nb = uint32_t(B.blobs.size());
        bool direct = B.identity;  // decode straight into the output image
        if (!O.d.reserve(B.out_bytes) || !O.h.reserve(B.out_bytes) || (!direct && !R->plain.reserve(B.plain_bytes)))
            return X.hand.abort_run(CDC_E_NOMEM);
        uint8_t *const out = O.d.as<uint8_t>();
        D.set_blobs(C.verify, R->src.loc, B.blobs.data(), nb);
        int st = cdc::decode_together(C, I, direct ? out : R->plain.as<uint8_t>(), B.plain_bytes, D, T);
        if (st == CDC_E_NOSPACE) {  // the slow path: never into the output image
            direct = false;
            st = R->plain.reserve(B.plain_bytes) ? cdc::decode_one_by_one(C, I, R->plain.as<uint8_t>(), B.plain_bytes, D, T)
                                                 : CDC_E_NOMEM;
        }
        if (st != CDC_OK) return X.hand.abort_run(st);
        const bool bad = std::any_of(bst.begin(), bst.begin() + nb, [](int32_t s) { return s != CDC_OK; });
        X.hand.advance(X.consumed);
        if (bad)
            for (const rplan::Piece &P : B.pieces)
                for (uint64_t s = P.seg0; s < P.seg0 + P.nchunks; ++s)
                    if (bst[B.segs[s].blob] != CDC_OK) {
                        X.fail_file(X.pidx[P.file], bst[B.segs[s].blob]);
                        break;
                    }
        if (direct && !bad) {
            ++X.st.batches_identity;
        } else {
            const auto t0 = Clock::now();
            bool ok = true;
            if (direct) {  // the plaintext sits compacted in the image: move it out of the way first
                if (!R->plain.reserve(D.plain_used)) return X.hand.abort_run(CDC_E_NOMEM);
                ok = !D.plain_used ||
                     hipMemcpyAsync(R->plain.data(), out, D.plain_used, hipMemcpyDeviceToDevice, R->stream[1]) == hipSuccess;
            }
            so.clear();
            sl.clear();
            sd.clear();
            for (const rplan::Segment &S : B.segs) {
                if (bst[S.blob] != CDC_OK) continue;  // its files have failed; their bytes are not delivered
                so.push_back(D.pos[S.blob]);
                sl.push_back(S.len);
                sd.push_back(S.dst_off);
            }
            if (ok && !so.empty())
                st = cdc_assemble_device(R->src.device, R->plain.data(), D.plain_used, so.data(), sl.data(), sd.data(), so.size(), out,
                                         B.out_bytes, R->stream[1]);
            if (st != CDC_OK) return X.hand.abort_run(st);
            if (!ok || hipStreamSynchronize(R->stream[1]) != hipSuccess) return X.hand.abort_run(CDC_E_DEVICE);
            X.assemble_s += since(t0);
        }
        X.hand.advance(X.assembled);
    }
}

// ---- writer stage -------------------------------------------------------------------
static void write_piece(Run &X, const rplan::Piece &P, const uint8_t *image)
{
    const int fi = X.pidx[P.file];
    const char *path = X.files[fi].path;
    if (!path || X.fstatus[fi].load() != CDC_OK) return;
    const int fd = open(path, P.first ? O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC : O_WRONLY | O_CLOEXEC, 0644);
    if (fd < 0) return X.fail_file(fi, CDC_E_IO);
    if (P.first) X.created[fi] = 1;
    const bool ok = pwrite_all(fd, image + P.dst_off, P.len, P.file_off);
    if (close(fd) != 0 || !ok) X.fail_file(fi, CDC_E_IO);
}

static void writer_stage(Run &X)
{
    cdc_restore *R = X.R;
    if (hipSetDevice(R->src.device) != hipSuccess) return X.hand.abort_run(CDC_E_DEVICE);
    for (int k = 0; k < int(X.batches.size()); ++k) {
        if (!X.hand.wait_for(X.assembled, k + 1)) return;
        const rplan::Batch &B = X.batches[k];
        OutSlot &O = R->out[k & 1];
        uint8_t *const image = O.h.as<uint8_t>();
        auto t0 = Clock::now();
        if (B.out_bytes && (hipMemcpyAsync(image, O.d.data(), B.out_bytes, hipMemcpyDeviceToHost, R->stream[2]) != hipSuccess ||
                            hipStreamSynchronize(R->stream[2]) != hipSuccess))
            return X.hand.abort_run(CDC_E_DEVICE);
        X.d2h_s += since(t0);
        t0 = Clock::now();
        parallel_for(R->o.writers, B.pieces.size(), [&](size_t i) { write_piece(X, B.pieces[i], image); });
        X.write_s += since(t0);
        for (const rplan::Piece &P : B.pieces) {
            const int fi = X.pidx[P.file];
            const int s = X.fstatus[fi].load();
            const char *path = X.files[fi].path;
            if (path) {
                if (s != CDC_OK && X.created[fi]) {  // what earlier pieces wrote goes with the failure
                    unlink(path);
                    X.created[fi] = 0;
                }
                if (P.last) {
                    X.reported[fi] = 1;
                    X.report(fi, s, 0, 1, nullptr, 0, 0);
                }
            } else {
                if (P.last) X.reported[fi] = 1;
                X.report(fi, s, X.fseen[fi]++, X.fpieces[fi], s == CDC_OK ? image + P.dst_off : nullptr, P.file_off,
                         s == CDC_OK ? P.len : 0);
            }
        }
        X.hand.advance(X.written);
    }
}

static int run_files(cdc_restore *R, const cdc_restore_file *files, int n, cdc_restore_file_fn on_file, void *ctx,
                     cdc_restore_stats *stats)
{
    const auto w0 = Clock::now();
    Run X{};
    X.R = R;
    X.files = files;
    X.n = n;
    X.on_file = on_file;
    X.ctx = ctx;
    X.fstatus.reset(new std::atomic<int>[size_t(std::max(n, 1))]);
    X.created.assign(size_t(n), 0);
    X.reported.assign(size_t(n), 0);
    X.fsize.assign(size_t(n), 0);
    X.fpieces.assign(size_t(n), 0);
    X.fseen.assign(size_t(n), 0);
    // the locator: every chunk's blob id, or CDC_E_NOTFOUND for the file
    for (int i = 0; i < n; ++i) {
        X.fstatus[i].store(CDC_OK);
        const cdc_restore_file &F = files[i];
        std::vector<uint32_t> ids(size_t(F.nchunks));
        const int64_t miss = cdc::resolve(R->src.loc, F.checksums, F.nchunks, ids.data());
        for (uint64_t c = 0; c < (miss < 0 ? F.nchunks : uint64_t(miss)); ++c) X.fsize[i] += F.lengths[c];
        if (miss >= 0) {
            X.fstatus[i].store(CDC_E_NOTFOUND);
            continue;
        }
        if (X.fstatus[i].load() != CDC_OK) continue;
        X.fblob.push_back(std::move(ids));
        X.pidx.push_back(i);
    }
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
        for (const rplan::Piece &P : B.pieces) ++X.fpieces[X.pidx[P.file]];
    }
    X.st.batches = X.batches.size();
    X.st.files = uint64_t(n);
    for (int i = 0; i < n; ++i)
        if (X.fstatus[i].load() != CDC_OK) {
            X.reported[i] = 1;
            X.report(i, X.fstatus[i].load(), 0, 1, nullptr, 0, 0);
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
        std::thread writer(guarded, writer_stage);
        guarded(device_stage);
        reader.join();
        writer.join();
    }
    // a run that broke off: the files it did not finish fail with its status
    for (int i = 0; i < n; ++i) {
        if (!X.reported[i]) {
            if (files[i].path && X.created[i]) unlink(files[i].path);
            X.fstatus[i].store(X.hand.fail != CDC_OK ? X.hand.fail : CDC_E_DEVICE);
            X.report(i, X.fstatus[i].load(), 0, 1, nullptr, 0, 0);
        }
        X.st.failed_files += X.fstatus[i].load() != CDC_OK;
    }
    X.st.read_s = X.read_s;
    X.st.h2d_s = X.h2d_s;
    X.st.decode_s = X.decode_s;
    X.st.verify_s = X.verify_s;
    X.st.assemble_s = X.assemble_s;
    X.st.d2h_s = X.d2h_s;
    X.st.write_s = X.write_s;
    X.st.wall_s = since(w0);
    if (stats) *stats = X.st;
    return X.hand.fail;
}

// ---- ranged reads -------------------------------------------------------------------
// cdc_restore_ranges: the batches of read_plan.h one after the other on the
// calling thread (gather, upload, prefix Decode + check, assemble, download,
// callbacks), in the context's first input and output slot.
constexpr uint64_t kGcmHeader = 60, kGcmRecord = 65536 + 28;

static int run_ranges(cdc_restore *R, const cdc_restore_file *files, int nfiles, const cdc_read_range *ranges, int nranges,
                      cdc_read_range_fn on_range, void *ctx, cdc_read_stats *stats)
{
    const auto w0 = Clock::now();
    cdc_read_stats st{};
    // the locator: every chunk's blob id, or kMissing (its ranges are CDC_E_NOTFOUND)
    std::vector<std::vector<uint32_t>> fblob((size_t(nfiles)));
    std::vector<rplan::File> pf;
    for (int i = 0; i < nfiles; ++i) {
        const cdc_restore_file &F = files[i];
        fblob[size_t(i)].resize(size_t(F.nchunks));
        uint32_t *const ids = fblob[size_t(i)].data();
        for (uint64_t c = 0; c < F.nchunks; ++c) {  // past every miss
            const int64_t miss = cdc::resolve(R->src.loc, F.checksums + 32 * c, F.nchunks - c, ids + c);
            if (miss < 0) break;
            c += uint64_t(miss);
            ids[c] = rplan::kMissing;
        }
        pf.push_back(rplan::File{F.nchunks, ids, F.lengths});
    }
    std::vector<rplan::Range> rr;
    for (int i = 0; i < nranges; ++i) rr.push_back(rplan::Range{ranges[i].file, ranges[i].offset, ranges[i].length});
    std::vector<rplan::RBatch> batches;
    std::vector<rplan::RangeInfo> info;
    rplan::plan_ranges(pf.data(), pf.size(), rr.data(), rr.size(), R->o.batch_bytes, R->o.batch_bytes, batches, info);
    std::vector<int> rstatus(size_t(nranges), CDC_OK);
    auto report = [&](int i, uint32_t piece, const uint8_t *data, uint64_t off, uint64_t len) {
        if (!on_range) return;
        cdc_read_result r{};
        r.index = i;
        r.status = rstatus[size_t(i)];
        r.piece = piece;
        r.pieces = std::max<uint32_t>(info[size_t(i)].pieces, 1);
        r.data = r.status == CDC_OK ? data : nullptr;
        r.data_offset = off;
        r.data_len = r.status == CDC_OK ? len : 0;
        r.length = info[size_t(i)].length;
        on_range(ctx, &r);
    };
    st.ranges = uint64_t(nranges);
    for (int i = 0; i < nranges; ++i) {
        rstatus[size_t(i)] = info[size_t(i)].status;
        if (rstatus[size_t(i)] != CDC_OK) report(i, 0, nullptr, 0, 0);
    }
    std::vector<bool> used(R->src.loc.locs.size(), false);
    for (const rplan::RBatch &B : batches) {
        st.bytes += B.out_bytes;
        st.segments += B.segs.size();
        st.decoded_bytes += B.scratch_bytes;
        for (const rplan::RBlob &b : B.blobs) {
            ++(b.upto == b.len ? st.whole_blobs : st.prefix_blobs);
            st.skipped_bytes += b.len - b.upto;
            if (!used[b.id]) {
                used[b.id] = true;
                ++st.distinct_blobs;
            }
        }
    }
    st.batches = batches.size();
    int fail = CDC_OK;
    if (!batches.empty() && hipSetDevice(R->src.device) != hipSuccess) fail = CDC_E_DEVICE;
    const uint8_t *key = R->src.key_ptr();
    InSlot &I = R->in[0];
    OutSlot &O = R->out[0];
    std::vector<uint64_t> upto, oo, so, sl, sd;
    std::vector<int32_t> bst;
    std::vector<uint8_t> want, whole;
    size_t done = 0;  // batches whose callbacks were made
    for (; done < batches.size() && fail == CDC_OK; ++done) {
        const rplan::RBatch &B = batches[done];
        const size_t nb = B.blobs.size();
        // gather: whole blobs, or without compression the header and the records that hold the prefix
        I.set_blobs(R->src.loc, B.blobs.data(), nb);
        if (R->src.compress == CDC_COMPRESS_NONE)
            for (size_t b = 0; b < nb; ++b)
                I.spans[b].length = std::min<uint64_t>(
                    I.spans[b].length, key ? kGcmHeader + (B.blobs[b].upto + 65535) / 65536 * kGcmRecord : B.blobs[b].upto);
        fail = cdc::gather(R->src.loc, I, R->o.writers, R->stream[0], &st.read_s, &st.h2d_s, &st.encoded_bytes);
        if (fail != CDC_OK) break;
        // prefix Decode into the scratch buffer, the check of the blobs decoded whole
        if (!R->plain.reserve(B.scratch_bytes) || !O.d.reserve(B.out_bytes) || !O.h.reserve(B.out_bytes)) {
            fail = CDC_E_NOMEM;
            break;
        }
        upto.assign(nb, 0);
        whole.assign(nb + 1, 0);
        oo.assign(nb + 1, 0);
        bst.assign(std::max<size_t>(nb, 1), CDC_OK);
        want.resize(nb * 32 + 1);
        for (size_t b = 0; b < nb; ++b) {
            upto[b] = B.blobs[b].upto;
            whole[b] = B.blobs[b].upto == B.blobs[b].len;
            std::memcpy(&want[b * 32], R->src.loc.sums[B.blobs[b].id].b, 32);
            if (I.pre[b] != CDC_OK) I.elen[b] = 0;  // never read: nothing of it goes through Decode
        }
        int rc = cdc::decode_prefix_checked(R->src.device, I.d.data(), I.eoff.data(), I.elen.data(), upto.data(), uint32_t(nb),
                                            R->src.compress, key, R->o.verify ? want.data() : nullptr, whole.data(),
                                            R->plain.as<uint8_t>(), B.scratch_bytes, oo.data(), bst.data(), R->stream[1],
                                            &st.decode_s, &st.verify_s);
        if (rc != CDC_OK) {
            fail = rc;
            break;
        }
        for (size_t b = 0; b < nb; ++b) {
            if (I.pre[b] != CDC_OK) bst[b] = I.pre[b];
            if (R->o.verify && whole[b] && bst[b] == CDC_OK) ++st.verified_blobs;
        }
        // a blob's failure fails every range of the batch that touches it
        for (const rplan::RPiece &P : B.pieces)
            for (uint64_t s = P.seg0; s < P.seg0 + P.nsegs; ++s) {
                const int32_t e = bst[B.segs[size_t(s)].blob];
                if (e != CDC_OK && rstatus[P.range] == CDC_OK) rstatus[P.range] = e;
            }
        auto t0 = Clock::now();
        so.clear();
        sl.clear();
        sd.clear();
        for (const rplan::Segment &S : B.segs) {
            if (bst[S.blob] != CDC_OK) continue;  // its ranges have failed; their bytes are not delivered
            so.push_back(S.src_off);
            sl.push_back(S.len);
            sd.push_back(S.dst_off);
        }
        if (!so.empty())
            rc = cdc_assemble_device(R->src.device, R->plain.data(), B.scratch_bytes, so.data(), sl.data(), sd.data(), so.size(),
                                     O.d.data(), B.out_bytes, R->stream[1]);
        if (rc == CDC_OK && hipStreamSynchronize(R->stream[1]) != hipSuccess) rc = CDC_E_DEVICE;
        if (rc != CDC_OK) {
            fail = rc;
            break;
        }
        st.assemble_s += since(t0);
        t0 = Clock::now();
        uint8_t *const image = O.h.as<uint8_t>();
        if (B.out_bytes && (hipMemcpyAsync(image, O.d.data(), B.out_bytes, hipMemcpyDeviceToHost, R->stream[2]) != hipSuccess ||
                            hipStreamSynchronize(R->stream[2]) != hipSuccess)) {
            fail = CDC_E_DEVICE;
            break;
        }
        st.d2h_s += since(t0);
        for (const rplan::RPiece &P : B.pieces) report(int(P.range), P.piece, image + P.dst_off, P.range_off, P.len);
    }
    // a run that broke off: the pieces it did not deliver fail with its status
    for (; done < batches.size(); ++done)
        for (const rplan::RPiece &P : batches[done].pieces) {
            rstatus[P.range] = fail;
            report(int(P.range), P.piece, nullptr, P.range_off, 0);
        }
    for (int i = 0; i < nranges; ++i) st.failed_ranges += rstatus[size_t(i)] != CDC_OK;
    st.wall_s = since(w0);
    if (stats) {
        st.struct_size = uint32_t(std::min<size_t>(stats->struct_size, sizeof(st)));
        std::memcpy(stats, &st, st.struct_size);
    }
    return fail;
}

}  // namespace

extern "C" {

int cdc_packfile_index(const uint8_t *bytes, uint64_t len, cdc_packfile_footer *footer, cdc_packfile_row *rows,
                       uint64_t cap, uint64_t *needed)
{
    if (!footer || (!bytes && len) || (!rows && cap)) return CDC_E_INVALID;
    if (needed) *needed = 0;
    const int st = rplan::parse_packfile(bytes, len, cdc::Locator::sha, footer, rows, cap);
    if (st != CDC_OK) return st;
    if (needed) *needed = footer->count;
    return footer->count > cap ? CDC_E_NOSPACE : CDC_OK;
}

void cdc_restore_default_opts(cdc_restore_opts *out)
{
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->verify = 1;
}

int cdc_restore_new(int device, const cdc_restore_opts *opts, cdc_restore **out)
{
    if (!opts || !out) return CDC_E_INVALID;
    *out = nullptr;
    if (device < 0 || device >= cdc::kMaxDevices || opts->writers < 0 || opts->writers > 256) return CDC_E_INVALID;
    if (!cdc::device_count_initialised()) return CDC_E_NOT_INIT;
    auto *r = new (std::nothrow) cdc_restore();
    if (!r) return CDC_E_NOMEM;
    try {
        r->src.open(device, opts->compress, opts->key);
        r->o = *opts;
        r->o.key = nullptr;
        if (!r->o.writers) r->o.writers = 8;
        if (!r->o.batch_bytes) r->o.batch_bytes = 256ull << 20;
    } catch (...) {
        delete r;
        return CDC_E_NOMEM;
    }
    bool ok = hipSetDevice(device) == hipSuccess;
    for (int i = 0; i < 3; ++i) ok = ok && hipStreamCreateWithFlags(&r->stream[i], hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
        cdc_restore_free(r);
        return CDC_E_DEVICE;
    }
    *out = r;
    return CDC_OK;
}

int cdc_restore_add_packfile(cdc_restore *r, const uint8_t *bytes, uint64_t len)
{
    return r && (bytes || !len) ? r->src.add_memory(bytes, len) : CDC_E_INVALID;
}

int cdc_restore_add_packfile_path(cdc_restore *r, const char *path)
{
    return r && path ? r->src.add_path(path) : CDC_E_INVALID;
}

int cdc_restore_add_packfiles(cdc_restore *r, const cdc_packfile_src *srcs, uint32_t n, int32_t *status)
{
    return r ? r->src.add_many(srcs, n, status) : CDC_E_INVALID;
}

int cdc_restore_files(cdc_restore *r, const cdc_restore_file *files, int n, cdc_restore_file_fn on_file, void *ctx,
                      cdc_restore_stats *stats)
{
    if (!r || n < 0 || (n && !files)) return CDC_E_INVALID;
    for (int i = 0; i < n; ++i)
        if (files[i].nchunks && (!files[i].checksums || !files[i].lengths)) return CDC_E_INVALID;
    std::lock_guard<std::mutex> lk(r->src.run_mu);
    try {
        return run_files(r, files, n, on_file, ctx, stats);
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

int cdc_restore_ranges(cdc_restore *r, const cdc_restore_file *files, int nfiles, const cdc_read_range *ranges,
                       int nranges, cdc_read_range_fn on_range, void *ctx, cdc_read_stats *stats)
{
    if (!r || nfiles < 0 || nranges < 0 || (nfiles && !files) || (nranges && !ranges) || (stats && stats->struct_size < 8))
        return CDC_E_INVALID;
    for (int i = 0; i < nfiles; ++i)
        if (files[i].nchunks && (!files[i].checksums || !files[i].lengths)) return CDC_E_INVALID;
    std::lock_guard<std::mutex> lk(r->src.run_mu);
    try {
        return run_ranges(r, files, nfiles, ranges, nranges, on_range, ctx, stats);
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

void cdc_restore_free(cdc_restore *r)
{
    if (!r) return;
    r->src.release(r->stream, 3);
    delete r;  // the slots' buffers and `plain` go with it, the streams drained above
}

}  // extern "C"
