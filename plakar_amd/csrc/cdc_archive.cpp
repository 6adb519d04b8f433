// cdc_archive_*: a snapshot's entries as one tar or tar.gz stream, or as a zip
// (include/plakar_cdc.h, "archive").
//
// The reference (cmd/plakar/subcommands/archive/archive.go:125-190) reads each
// file chunk by chunk (one GetBlob and one Decode per chunk, a chunk that
// occurs twice decoded twice), copies the bytes into an archive/tar writer and,
// for its default format, pushes the whole tar stream through one
// gzip.NewWriter.  Here the tar stream is planned up front (archive_plan.h) in
// batches of stream bytes, and a batch goes through
//
//   read      its distinct encoded blobs gathered (cdc_reader.h: gather_read,
//             on `writers` threads) with the batch's header blocks and a zero
//             block behind them;
//   H2D       one copy of each;
//   Decode    the shared decode step (+ verify) over the distinct blobs
//             (cdc_reader.h: decode_batch);
//   assemble  cdc_assemble_device: chunk occurrences, header blocks and
//             padding into the batch's image of the tar stream;
//   deflate   tar.gz: cdc_gzip_stream_piece over the image, one member for
//             the whole run;
//   D2H       the image, or for tar.gz only the compressed bytes;
//   write     to the path or to on_data, in stream order.
//
// A context from cdc_archive_new_zip writes the zip format instead
// (archive.go:194-245; zip_plan.h has the container and its planner): a batch's
// image holds only file bytes, and in the place of the deflate stage
//
//   deflate   cdc_zip_pieces_device: every entry of the batch (or the part of
//             one that the batch holds) as its own raw DEFLATE stream, its
//             local header before it and its data descriptor behind it;
//
// only the compressed bytes come back, and after the last batch the host
// writes the central directory and the end records from what it kept per
// entry (CRC-32, sizes, the local header's offset).
//
// The stages of one batch run one after the other on the calling thread and
// batches do not overlap yet (restore's three-thread rotation is the model for
// that step); every stage's seconds are in the stats.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "archive_plan.h"
#include "cdc_reader.h"
#include "deflate_enc.h"
#include "inflate_walk.h"
#include "zip_plan.h"

namespace {

using cdc::Clock;
using cdc::since;

constexpr uint64_t kMaxBatch = 1ull << 30;  // a batch's image is one gzip piece: under 2 GiB with its largest chunk

}  // namespace

struct cdc_archive {
    cdc::PackSource src;  // device, codec, locator, run lock
    cdc_archive_opts o{};
    bool zip = false;  // cdc_archive_new_zip: o.format is not read
    int level = CDC_LEVEL_FAST;  // cdc_archive_set_level: the match search of tar.gz and zip
    hipStream_t stream = nullptr;
    cdc::Arena in;  // the batch's encoded blobs, its header blocks behind them in the pinned half
    cdc::PinBuf h_out;
    cdc::DevBuf d_plain, d_img, d_gz;
};

namespace {

struct Run {
    cdc_archive *A;
    cdc_archive_data_fn on_data;
    void *ctx;
    int fd = -1;
    std::vector<int> pidx;  // planned entry -> index in entries
    cdc_archive_stats st{};
    int failed = -1;        // the entry a failure names

    int emit(const uint8_t *p, uint64_t len)
    {
        if (!len) return CDC_OK;
        st.output_bytes += len;
        if (fd >= 0) return cdc::write_all(fd, p, len) ? CDC_OK : CDC_E_IO;
        return on_data && on_data(ctx, p, len) == 0 ? CDC_OK : CDC_E_IO;
    }
};

// read, H2D, Decode (+ verify) and assemble: the batch's image in A->d_img.
// CDC_OK or the run's failure (X.failed set when a blob is to blame).
static int stage_image(Run &X, const aplan::Batch &B)
{
    cdc_archive *A = X.A;
    const cdc::Locator &L = A->src.loc;
    const uint32_t nb = uint32_t(B.blobs.size());
    hipStream_t s = A->stream;
    // read
    const uint64_t arena_base = cdc::align_up(B.plain_bytes, 16), plain_cap = arena_base + B.arena.size();
    if (!A->d_plain.reserve(plain_cap) || !A->d_img.reserve(B.out_bytes)) return CDC_E_NOMEM;
    cdc::Arena &I = A->in;
    I.set_blobs(L, B.blobs.data(), nb);
    int st = cdc::gather_read(L, I, A->o.writers, B.arena.size(), &X.st.read_s, &X.st.encoded_bytes);
    if (st != CDC_OK) return st;
    auto t0 = Clock::now();
    uint8_t *const h_arena = I.h.as<uint8_t>() + cdc::align_up(I.total, 16);
    if (!B.arena.empty()) std::memcpy(h_arena, B.arena.data(), B.arena.size());
    X.st.read_s += since(t0);
    // which entry a blob belongs to (its first use in the batch), for a failure's name
    auto blame = [&](uint32_t b, int status) {
        for (const aplan::Segment &S : B.segs)
            if (!S.arena && S.blob == b) {
                X.failed = X.pidx[S.entry];
                break;
            }
        return status;
    };
    for (uint32_t b = 0; b < nb; ++b)
        if (I.pre[b] != CDC_OK) return blame(b, I.pre[b]);
    // H2D
    t0 = Clock::now();
    uint8_t *const plain = A->d_plain.as<uint8_t>();
    if ((I.total && hipMemcpyAsync(I.d.data(), I.h.data(), I.total, hipMemcpyHostToDevice, s) != hipSuccess) ||
        (!B.arena.empty() && hipMemcpyAsync(plain + arena_base, h_arena, B.arena.size(), hipMemcpyHostToDevice, s) != hipSuccess) ||
        hipStreamSynchronize(s) != hipSuccess)
        return CDC_E_DEVICE;
    X.st.h2d_s += since(t0);
    // Decode (+ verify): the first blob in batch order that is not right names the entry
    cdc::Decoded D;
    uint64_t decoded = 0;
    D.set_blobs(A->o.verify != 0, L, B.blobs.data(), nb);
    if (nb) {
        st = cdc::decode_batch(cdc::DecodeCtx{A->src.device, A->src.compress, A->src.key_ptr(), A->o.verify != 0, s}, I, plain,
                               B.plain_bytes, D, cdc::DecodeTally{&decoded, &X.st.decode_s, &X.st.verify_s});
        if (st != CDC_OK) return st;
        for (uint32_t b = 0; b < nb; ++b)
            if (D.bst[b] != CDC_OK) return blame(b, D.bst[b]);
        X.st.decoded_bytes += decoded;
    }
    // assemble
    t0 = Clock::now();
    if (!B.segs.empty()) {
        const size_t ns = B.segs.size();
        std::vector<uint64_t> so(ns), sl(ns), sd(ns);
        for (size_t i = 0; i < ns; ++i) {
            const aplan::Segment &S = B.segs[i];
            so[i] = S.arena ? arena_base + S.src_off : D.pos[S.blob];
            sl[i] = S.len;
            sd[i] = S.dst_off;
        }
        st = cdc_assemble_device(A->src.device, plain, plain_cap, so.data(), sl.data(), sd.data(), ns, A->d_img.data(),
                                 B.out_bytes, s);
        if (st != CDC_OK) return st;
        if (hipStreamSynchronize(s) != hipSuccess) return CDC_E_DEVICE;
    }
    X.st.assemble_s += since(t0);
    return CDC_OK;
}

// One batch through every stage; CDC_OK or the run's failure.
static int run_batch(Run &X, const aplan::Batch &B, cdc_gzip_stream *gz, bool last)
{
    cdc_archive *A = X.A;
    hipStream_t s = A->stream;
    int st = stage_image(X, B);
    if (st != CDC_OK) return st;
    auto t0 = Clock::now();
    // deflate
    const uint8_t *d_src = A->d_img.as<uint8_t>();
    uint64_t out_len = B.out_bytes;
    if (gz) {
        t0 = Clock::now();
        const uint64_t cap = cdc_gzip_stream_bound(B.out_bytes);
        if (!A->d_gz.reserve(cap)) return CDC_E_NOMEM;
        st = cdc_gzip_stream_piece(gz, d_src, B.out_bytes, last ? 1 : 0, A->d_gz.as<uint8_t>(), cap, &out_len, s);
        if (st != CDC_OK) return st;
        d_src = A->d_gz.as<uint8_t>();
        X.st.deflate_s += since(t0);
    }
    // D2H
    t0 = Clock::now();
    if (!A->h_out.reserve(out_len)) return CDC_E_NOMEM;
    if (out_len && (hipMemcpyAsync(A->h_out.data(), d_src, out_len, hipMemcpyDeviceToHost, s) != hipSuccess ||
                    hipStreamSynchronize(s) != hipSuccess))
        return CDC_E_DEVICE;
    X.st.d2h_s += since(t0);
    // write
    t0 = Clock::now();
    st = X.emit(A->h_out.as<uint8_t>(), out_len);
    X.st.write_s += since(t0);
    return st;
}

static int run(cdc_archive *A, const cdc_archive_entry *entries, int n, const char *path, cdc_archive_data_fn on_data,
               cdc_archive_entry_fn on_entry, void *ctx, cdc_archive_stats *stats)
{
    const auto w0 = Clock::now();
    Run X{};
    X.A = A;
    X.on_data = on_data;
    X.ctx = ctx;
    auto finish = [&](int st) {
        X.st.failed_entry = st == CDC_OK ? -1 : X.failed;
        X.st.wall_s = since(w0);
        if (stats) {
            X.st.struct_size = uint32_t(std::min<size_t>(stats->struct_size, sizeof(X.st)));
            std::memcpy(stats, &X.st, X.st.struct_size);
        }
        return st;
    };
    // the locator: every chunk's blob id; an entry with a checksum in no
    // packfile is left out whole, header included, and the run goes on
    std::vector<std::vector<uint32_t>> fblob;
    std::vector<std::vector<uint8_t>> hdrs;
    for (int i = 0; i < n; ++i) {
        const cdc_archive_entry &E = entries[i];
        const bool dir = E.type == CDC_ARCHIVE_DIR;
        std::vector<uint32_t> ids(dir ? 0 : size_t(E.nchunks));
        uint64_t size = 0;
        for (uint64_t c = 0; c < ids.size(); ++c) size += E.lengths[c];
        if (cdc::resolve(A->src.loc, E.checksums, ids.size(), ids.data()) >= 0) {
            ++X.st.skipped_entries;
            if (on_entry) on_entry(ctx, i, CDC_E_NOTFOUND);
            continue;
        }
        std::vector<uint8_t> h;
        const aplan::Entry pe{E.name, std::strlen(E.name), E.type, E.mode, E.mtime, size};
        const int st = aplan::build_header(pe, h);
        if (st != CDC_OK) {  // a name or mode no header can carry: nothing is written
            X.failed = i;
            if (on_entry) on_entry(ctx, i, st);
            return finish(st);
        }
        fblob.push_back(std::move(ids));
        hdrs.push_back(std::move(h));
        X.pidx.push_back(i);
    }
    std::vector<aplan::File> pf;
    for (size_t p = 0; p < X.pidx.size(); ++p)
        pf.push_back(aplan::File{hdrs[p].data(), hdrs[p].size(), fblob[p].size(), fblob[p].data(), entries[X.pidx[p]].lengths});
    std::vector<aplan::Batch> batches;
    aplan::plan(pf.data(), pf.size(), A->o.batch_bytes, batches);
    for (const aplan::Batch &B : batches) {
        X.st.stream_bytes += B.out_bytes;
        X.st.segments += B.segs.size();
        X.st.decoded_blobs += B.blobs.size();
    }
    X.st.batches = batches.size();
    X.st.entries = X.pidx.size();
    if (hipSetDevice(A->src.device) != hipSuccess) return finish(CDC_E_DEVICE);
    if (path) {
        X.fd = open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
        if (X.fd < 0) return finish(CDC_E_IO);
    }
    cdc_gzip_stream *gz = nullptr;
    int st = A->o.format == CDC_ARCHIVE_TARGZ ? cdc_gzip_stream_new(A->src.device, &gz) : CDC_OK;
    if (st == CDC_OK && gz) st = cdc_gzip_stream_set_level(gz, A->level);
    for (size_t k = 0; k < batches.size() && st == CDC_OK; ++k) st = run_batch(X, batches[k], gz, k + 1 == batches.size());
    cdc_gzip_stream_free(gz);
    if (X.fd >= 0) {
        if (close(X.fd) != 0 && st == CDC_OK) st = CDC_E_IO;
        if (st != CDC_OK) unlink(path);  // nothing is left behind: the reference's log.Fatal before its rename
    }
    if (on_entry) {
        if (st == CDC_OK)
            for (int i : X.pidx) on_entry(ctx, i, CDC_OK);
        else if (X.failed >= 0)
            on_entry(ctx, X.failed, st);
    }
    return finish(st);
}

// ---- zip ---------------------------------------------------------------------
struct OpenEntry {   // an entry whose stream is not closed yet
    uint32_t reg = 0xFFFFFFFFu;  // CRC-32 register over its bytes so far
    uint64_t csize = 0, usize = 0;
};

// The most a batch's pieces write: header, len and 5 bytes per span, the joiner's 6 (a last
// piece's end is shorter), the 24-byte descriptor.
static uint64_t zip_bound(const zplan::Batch &B)
{
    uint64_t cap = 0;
    for (const zplan::Piece &P : B.pieces)
        cap += P.hdr_len + P.len + 5 * ((P.len + dfl::kSpan - 1) / dfl::kSpan) + 6 + 24;
    return cap;
}

// One zip batch: the image (file bytes only), every piece deflated in one call,
// D2H of the compressed bytes, write; then the host's share: running CRC-32 and
// sizes of the open entry, a directory record per entry that ends here.
static int run_zip_batch(Run &X, const zplan::Batch &B, std::vector<zplan::Record> &recs, OpenEntry &open, uint64_t &stream_off)
{
    cdc_archive *A = X.A;
    hipStream_t s = A->stream;
    int st = stage_image(X, B.a);
    if (st != CDC_OK) return st;
    // deflate
    auto t0 = Clock::now();
    const size_t np = B.pieces.size();
    std::vector<cdc_zip_piece> pc(np);
    std::vector<cdc_zip_piece_out> po(np);
    for (size_t i = 0; i < np; ++i) {
        const zplan::Piece &P = B.pieces[i];
        cdc_zip_piece &p = pc[i];
        p = cdc_zip_piece{};
        p.src_off = P.img_off;
        p.len = P.len;
        p.first = P.first;
        p.last = P.last;
        p.hdr_off = P.hdr_off;
        p.hdr_len = P.hdr_len;
        // only a batch's first piece can continue an entry: every other one starts its own
        p.crc_reg = P.first ? 0xFFFFFFFFu : open.reg;
        p.csize_before = P.first ? 0 : open.csize;
        p.usize_before = P.first ? 0 : open.usize;
    }
    const uint64_t cap = zip_bound(B);
    uint64_t total = 0;
    if (!A->d_gz.reserve(cap)) return CDC_E_NOMEM;
    st = cdc_zip_pieces_device_level(A->src.device, A->d_img.data(), B.a.out_bytes, pc.data(), uint32_t(np), B.hdrs.data(),
                                     B.hdrs.size(), A->d_gz.as<uint8_t>(), cap, po.data(), &total, A->level, s);
    if (st != CDC_OK) {
        // a piece the pass cannot take (2 GiB or more): the entry is to blame
        if (st == CDC_E_UNSUPPORTED)
            for (const zplan::Piece &P : B.pieces)
                if (P.len > dfl::kMaxBlob) {
                    X.failed = X.pidx[P.entry];
                    break;
                }
        return st;
    }
    X.st.deflate_s += since(t0);
    for (size_t i = 0; i < np; ++i) {
        const zplan::Piece &P = B.pieces[i];
        if (P.first) {
            open = OpenEntry();
            recs[P.entry].offset = stream_off + po[i].out_off;
        }
        open.reg = infw::crc_mul(open.reg, infw::crc_shift(P.len)) ^ po[i].crc_reg;
        open.csize += po[i].deflate_len;
        open.usize += P.len;
        if (P.last) {
            zplan::Record &R = recs[P.entry];
            R.crc = ~open.reg;
            R.csize = open.csize;
            R.usize = open.usize;
        }
    }
    stream_off += total;
    // D2H
    t0 = Clock::now();
    if (!A->h_out.reserve(total)) return CDC_E_NOMEM;
    if (total && (hipMemcpyAsync(A->h_out.data(), A->d_gz.data(), total, hipMemcpyDeviceToHost, s) != hipSuccess ||
                  hipStreamSynchronize(s) != hipSuccess))
        return CDC_E_DEVICE;
    X.st.d2h_s += since(t0);
    // write
    t0 = Clock::now();
    st = X.emit(A->h_out.as<uint8_t>(), total);
    X.st.write_s += since(t0);
    return st;
}

static int run_zip(cdc_archive *A, const cdc_archive_entry *entries, int n, const char *path, cdc_archive_data_fn on_data,
                   cdc_archive_entry_fn on_entry, void *ctx, cdc_archive_stats *stats)
{
    const auto w0 = Clock::now();
    Run X{};
    X.A = A;
    X.on_data = on_data;
    X.ctx = ctx;
    auto finish = [&](int st) {
        X.st.failed_entry = st == CDC_OK ? -1 : X.failed;
        X.st.wall_s = since(w0);
        if (stats) {
            X.st.struct_size = uint32_t(std::min<size_t>(stats->struct_size, sizeof(X.st)));
            std::memcpy(stats, &X.st, X.st.struct_size);
        }
        return st;
    };
    // the locator, as for tar; a directory is accepted and not written (archive.go:211-213)
    std::vector<std::vector<uint32_t>> fblob;
    std::vector<std::vector<uint8_t>> hdrs;
    std::vector<zplan::Record> recs;
    std::vector<int> dirs;
    for (int i = 0; i < n; ++i) {
        const cdc_archive_entry &E = entries[i];
        if (E.type == CDC_ARCHIVE_DIR) {
            dirs.push_back(i);
            continue;
        }
        std::vector<uint32_t> ids(size_t(E.nchunks));
        if (cdc::resolve(A->src.loc, E.checksums, ids.size(), ids.data()) >= 0) {
            ++X.st.skipped_entries;
            if (on_entry) on_entry(ctx, i, CDC_E_NOTFOUND);
            continue;
        }
        std::vector<uint8_t> h;
        zplan::Record R;
        const int st = zplan::build_local(zplan::Entry{E.name, std::strlen(E.name), E.mode, E.mtime}, h, R);
        if (st != CDC_OK) {  // a name or mode no header can carry: nothing is written
            X.failed = i;
            if (on_entry) on_entry(ctx, i, st);
            return finish(st);
        }
        fblob.push_back(std::move(ids));
        hdrs.push_back(std::move(h));
        recs.push_back(std::move(R));
        X.pidx.push_back(i);
    }
    std::vector<aplan::File> pf;
    for (size_t p = 0; p < X.pidx.size(); ++p)
        pf.push_back(aplan::File{hdrs[p].data(), hdrs[p].size(), fblob[p].size(), fblob[p].data(), entries[X.pidx[p]].lengths});
    std::vector<zplan::Batch> batches;
    zplan::plan(pf.data(), pf.size(), A->o.batch_bytes, batches);
    for (const zplan::Batch &B : batches) {
        X.st.stream_bytes += B.used;
        X.st.segments += B.a.segs.size();
        X.st.decoded_blobs += B.a.blobs.size();
    }
    X.st.batches = batches.size();
    X.st.entries = X.pidx.size();
    if (hipSetDevice(A->src.device) != hipSuccess) return finish(CDC_E_DEVICE);
    if (path) {
        X.fd = open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
        if (X.fd < 0) return finish(CDC_E_IO);
    }
    int st = CDC_OK;
    OpenEntry open_entry;
    uint64_t stream_off = 0;
    for (size_t k = 0; k < batches.size() && st == CDC_OK; ++k) st = run_zip_batch(X, batches[k], recs, open_entry, stream_off);
    if (st == CDC_OK) {
        // the central directory and the end records, on the host
        const auto t0 = Clock::now();
        std::vector<uint8_t> tail;
        zplan::build_tail(recs.data(), recs.size(), stream_off, tail);
        st = X.emit(tail.data(), tail.size());
        X.st.write_s += since(t0);
    }
    if (X.fd >= 0) {
        if (close(X.fd) != 0 && st == CDC_OK) st = CDC_E_IO;
        if (st != CDC_OK) unlink(path);
    }
    if (on_entry) {
        if (st == CDC_OK) {
            for (int i : X.pidx) on_entry(ctx, i, CDC_OK);
            for (int i : dirs) on_entry(ctx, i, CDC_OK);
        } else if (X.failed >= 0) {
            on_entry(ctx, X.failed, st);
        }
    }
    return finish(st);
}

}  // namespace

extern "C" {

void cdc_archive_default_opts(cdc_archive_opts *out)
{
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
    out->verify = 1;
    out->format = CDC_ARCHIVE_TARGZ;  // the reference's default, "tarball"
}

int cdc_archive_new(int device, const cdc_archive_opts *opts, cdc_archive **out)
{
    if (!opts || !out) return CDC_E_INVALID;
    *out = nullptr;
    if (opts->struct_size != sizeof(*opts) || device < 0 || device >= cdc::kMaxDevices || opts->writers < 0 ||
        opts->writers > 256 || (opts->format != CDC_ARCHIVE_TAR && opts->format != CDC_ARCHIVE_TARGZ))
        return CDC_E_INVALID;
    if (!cdc::device_count_initialised()) return CDC_E_NOT_INIT;
    auto *a = new (std::nothrow) cdc_archive();
    if (!a) return CDC_E_NOMEM;
    try {
        a->src.open(device, opts->compress, opts->key);
        a->o = *opts;
        a->o.key = nullptr;
        if (!a->o.writers) a->o.writers = 8;
        if (!a->o.batch_bytes) a->o.batch_bytes = 256ull << 20;
        a->o.batch_bytes = std::min<uint64_t>(a->o.batch_bytes, kMaxBatch);
    } catch (...) {
        delete a;
        return CDC_E_NOMEM;
    }
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking) != hipSuccess) {
        cdc_archive_free(a);
        return CDC_E_DEVICE;
    }
    *out = a;
    return CDC_OK;
}

int cdc_archive_new_zip(int device, const cdc_archive_opts *opts, cdc_archive **out)
{
    if (!opts || !out) return CDC_E_INVALID;
    *out = nullptr;
    if (opts->struct_size != sizeof(*opts)) return CDC_E_INVALID;
    cdc_archive_opts o = *opts;
    o.format = CDC_ARCHIVE_TAR;  // the caller's is not read: zip is no value of it
    const int st = cdc_archive_new(device, &o, out);
    if (st == CDC_OK) (*out)->zip = true;
    return st;
}

int cdc_archive_set_level(cdc_archive *a, int level)
{
    if (!a || (!cdc::level_ok(level))) return CDC_E_INVALID;
    std::lock_guard<std::mutex> lk(a->src.run_mu);
    a->level = level;
    return CDC_OK;
}

int cdc_archive_add_packfile(cdc_archive *a, const uint8_t *bytes, uint64_t len)
{
    return a && (bytes || !len) ? a->src.add_memory(bytes, len) : CDC_E_INVALID;
}

int cdc_archive_add_packfile_path(cdc_archive *a, const char *path)
{
    return a && path ? a->src.add_path(path) : CDC_E_INVALID;
}

int cdc_archive_add_packfiles(cdc_archive *a, const cdc_packfile_src *srcs, uint32_t n, int32_t *status)
{
    return a ? a->src.add_many(srcs, n, status) : CDC_E_INVALID;
}

int cdc_archive_run(cdc_archive *a, const cdc_archive_entry *entries, int n, const char *path, cdc_archive_data_fn on_data,
                    cdc_archive_entry_fn on_entry, void *ctx, cdc_archive_stats *stats)
{
    if (!a || n < 0 || (n && !entries) || (!path && !on_data)) return CDC_E_INVALID;
    if (stats && stats->struct_size < 8) return CDC_E_INVALID;
    for (int i = 0; i < n; ++i) {
        const cdc_archive_entry &E = entries[i];
        if (!E.name || (E.type != CDC_ARCHIVE_FILE && E.type != CDC_ARCHIVE_DIR)) return CDC_E_INVALID;
        if (E.type == CDC_ARCHIVE_FILE && E.nchunks && (!E.checksums || !E.lengths)) return CDC_E_INVALID;
    }
    std::lock_guard<std::mutex> lk(a->src.run_mu);
    try {
        return (a->zip ? run_zip : run)(a, entries, n, path, on_data, on_entry, ctx, stats);
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

void cdc_archive_free(cdc_archive *a)
{
    if (!a) return;
    a->src.release(&a->stream, 1);
    delete a;
}

}  // extern "C"
