// The stored packfile form (snapshot.PutPackfile, snapshot/snapshot.go:232-267):
//
//   data || Encode(index) || Encode(footer) || u32le version || u8 len(Encode(footer))
//
// where Encode is the repository's compression and AES-256-GCM stream, the one
// the blobs go through.  No kernel of its own: the two small blobs of every
// packfile go through cdc_decode_device and cdc_encode_device_level.  What this
// file adds is the batching: registering n packfiles is two Decode calls, one
// over the n encoded footers and one over the n encoded indexes, whatever n is
// (DESIGN.md 5.22).  The layout arithmetic is stored_plan.h (host only).
#include "cdc_stored.h"

#include <sys/random.h>

#include <algorithm>
#include <new>

#include "stored_plan.h"

namespace cdc {

namespace {

constexpr uint64_t kTailRead = stplan::kTrailerBytes + stplan::kMaxFooterCode;  // the most a footer range and trailer take

// Decode's and the planner's statuses as cdc_*_add_packfiles reports them.
int32_t source_status(int32_t st)
{
    return st == CDC_OK || st == CDC_E_AUTH || st == CDC_E_IO ? st : CDC_E_CORRUPT;
}

struct Fd {
    int fd = -1;
    explicit Fd(const char *path) : fd(open(path, O_RDONLY | O_CLOEXEC)) {}
    ~Fd()
    {
        if (fd >= 0) close(fd);
    }
    // the length of a regular file, or false
    bool length(uint64_t *len) const
    {
        struct stat sb;
        if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) return false;
        *len = uint64_t(sb.st_size);
        return true;
    }
};

// CDC_OK or CDC_E_IO: bytes [off, off + n) of the source into dst.
int read_source(const cdc_packfile_src &s, uint64_t off, uint64_t n, uint8_t *dst)
{
    if (n == 0) return CDC_OK;
    if (s.bytes) {
        std::memcpy(dst, s.bytes + off, size_t(n));
        return CDC_OK;
    }
    Fd f(s.path);
    return f.fd >= 0 && pread_all(f.fd, dst, n, off) ? CDC_OK : CDC_E_IO;
}

}  // namespace

int random_fill(uint8_t *p, size_t n)
{
    while (n) {
        const ssize_t k = getrandom(p, n, 0);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) return CDC_E_IO;
        p += k;
        n -= size_t(k);
    }
    return CDC_OK;
}

StoredCodec::~StoredCodec()
{
    if (stream) {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
        (void)hipStreamDestroy(stream);
    }
    if (!key.empty()) std::memset(key.data(), 0, key.size());
}

int StoredCodec::open(int dev, int comp, const uint8_t *k)
{
    device = dev;
    compress = comp;
    if (k) key.assign(k, k + 32);
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) {
        stream = nullptr;
        return CDC_E_DEVICE;
    }
    return CDC_OK;
}

// One upload of h[0, in_bytes), one cdc_decode_device over the blobs at
// off/len in it, one download: *plain then points at the plaintext in pinned
// memory, blob j at oo[j].  `expect` sizes the output; when a malformed blob
// decodes to more than its source announced, the call is made once more with
// what Decode asked for (bounded by Decode's own expansion bounds over bytes
// that were really read).
int StoredCodec::decode_batch(uint64_t in_bytes, const std::vector<uint64_t> &off, const std::vector<uint64_t> &len,
                              uint64_t expect, std::vector<uint64_t> &oo, std::vector<int32_t> &st,
                              const uint8_t **plain)
{
    const uint32_t m = uint32_t(off.size());
    oo.assign(size_t(m) + 1, 0);
    st.assign(m, CDC_OK);
    *plain = h.as<uint8_t>();
    if (m == 0) return CDC_OK;
    if (hipSetDevice(device) != hipSuccess) return CDC_E_DEVICE;
    const uint64_t in_room = align_up(size_t(in_bytes), 256);
    uint64_t cap = align_up(size_t(expect), 256) + 256;
    for (int attempt = 0;; ++attempt) {
        if (!d.reserve(size_t(in_room + cap))) return CDC_E_NOMEM;
        uint8_t *const d_in = d.as<uint8_t>(), *const d_out = d_in + in_room;
        if (in_bytes && (hipMemcpyAsync(d_in, h.data(), size_t(in_bytes), hipMemcpyHostToDevice, stream) != hipSuccess ||
                         hipStreamSynchronize(stream) != hipSuccess))
            return CDC_E_DEVICE;
        const int r = cdc_decode_device(device, d_in, off.data(), len.data(), m, compress, key_ptr(), d_out, cap,
                                        oo.data(), st.data(), stream);
        if (r == CDC_E_NOSPACE && attempt == 0) {
            cap = align_up(size_t(oo[m]), 256) + 256;
            continue;
        }
        if (r != CDC_OK) return r == CDC_E_NOSPACE ? CDC_E_DEVICE : r;
        // the encoded bytes are not needed on the host any more
        if (!h.reserve(size_t(oo[m]))) return CDC_E_NOMEM;
        if (oo[m] && (hipMemcpyAsync(h.data(), d_out, size_t(oo[m]), hipMemcpyDeviceToHost, stream) != hipSuccess ||
                      hipStreamSynchronize(stream) != hipSuccess))
            return CDC_E_DEVICE;
        *plain = h.as<uint8_t>();
        return CDC_OK;
    }
}

int StoredCodec::read_many(const cdc_packfile_src *srcs, uint32_t n, int32_t *status, cdc_packfile_footer *footer,
                           std::vector<cdc_packfile_row> *rows, uint64_t *len)
{
    const bool encrypted = !key.empty(), coded = encrypted || compress != CDC_COMPRESS_NONE;
    std::vector<stplan::Tail> tail(n);
    std::vector<uint32_t> who;  // the sources of the current Decode call
    std::vector<uint64_t> off, blen, oo;
    std::vector<int32_t> st;
    const uint8_t *plain = nullptr;

    // 1. the trailers and the encoded footers: one read of at most 260 bytes per source
    if (!h.reserve(size_t(n) * 256)) return CDC_E_NOMEM;
    uint64_t in_bytes = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const cdc_packfile_src &s = srcs[i];
        uint8_t buf[kTailRead];
        uint64_t L = s.len, got = 0;
        status[i] = CDC_OK;
        if (s.bytes) {
            got = std::min<uint64_t>(L, kTailRead);
            std::memcpy(buf + (kTailRead - got), s.bytes + (L - got), size_t(got));
        } else {
            Fd f(s.path);
            if (!f.length(&L)) {
                status[i] = CDC_E_IO;
            } else {
                got = std::min<uint64_t>(L, kTailRead);
                if (got && !pread_all(f.fd, buf + (kTailRead - got), got, L - got)) status[i] = CDC_E_IO;
            }
        }
        len[i] = L;
        if (status[i] != CDC_OK) continue;
        // the planner reads the last five bytes only when there are that many
        status[i] = stplan::split_tail(buf + kTailRead - stplan::kTrailerBytes, L, coded, &tail[i]);
        if (status[i] != CDC_OK) continue;
        const stplan::Tail &t = tail[i];
        std::memcpy(h.as<uint8_t>() + in_bytes, buf + kTailRead - stplan::kTrailerBytes - t.L, t.L);
        who.push_back(i);
        off.push_back(in_bytes);
        blen.push_back(t.L);
        in_bytes += t.L;  // at most 255 each: within the 256 per source reserved
    }

    // 2. Decode of the footers
    int r = decode_batch(in_bytes, off, blen, uint64_t(who.size()) * rplan::kFooterBytes, oo, st, &plain);
    if (r != CDC_OK) return r;

    // 3. the index ranges, and the encoded indexes gathered
    std::vector<stplan::IndexRange> range(n);
    std::vector<uint32_t> who2;
    uint64_t idx_bytes = 0, idx_plain = 0;
    for (size_t j = 0; j < who.size(); ++j) {
        const uint32_t i = who[j];
        status[i] = source_status(st[j]);
        if (status[i] != CDC_OK) continue;
        status[i] = stplan::index_range(plain + oo[j], oo[j + 1] - oo[j], tail[i], compress, encrypted, &footer[i],
                                        &range[i]);
        if (status[i] != CDC_OK) continue;
        who2.push_back(i);
        idx_bytes += range[i].len;
    }
    if (!h.reserve(size_t(idx_bytes))) return CDC_E_NOMEM;  // the decoded footers have been parsed: the buffer may go
    off.clear();
    blen.clear();
    who.clear();
    in_bytes = 0;
    for (uint32_t i : who2) {
        status[i] = read_source(srcs[i], range[i].off, range[i].len, h.as<uint8_t>() + in_bytes);
        if (status[i] != CDC_OK) continue;
        who.push_back(i);
        off.push_back(in_bytes);
        blen.push_back(range[i].len);
        in_bytes += range[i].len;
        idx_plain += range[i].plain;
    }

    // 4. Decode of the indexes
    r = decode_batch(in_bytes, off, blen, idx_plain, oo, st, &plain);
    if (r != CDC_OK) return r;

    // 5. hash and parse on the host
    for (size_t j = 0; j < who.size(); ++j) {
        const uint32_t i = who[j];
        status[i] = source_status(st[j]);
        if (status[i] != CDC_OK) continue;
        if (oo[j + 1] - oo[j] != range[i].plain) {
            status[i] = CDC_E_CORRUPT;
            continue;
        }
        rows[i].resize(footer[i].count);  // 41 * count bytes were decoded: count is real
        status[i] = rplan::parse_index(plain + oo[j], footer[i], Locator::sha, rows[i].data(), rows[i].size());
        if (status[i] != CDC_OK) rows[i].clear();
    }
    return CDC_OK;
}

int StoredCodec::write_tail(const uint8_t *index, uint64_t index_len, const uint8_t *footer52, const uint8_t *random,
                            std::vector<uint8_t> &tail)
{
    uint8_t drawn[112];
    if (!key.empty() && !random) {
        const int st = random_fill(drawn, sizeof(drawn));
        if (st != CDC_OK) return st;
        random = drawn;
    }
    if (hipSetDevice(device) != hipSuccess) return CDC_E_DEVICE;
    const uint64_t foff = align_up(size_t(index_len), 16), in_bytes = foff + rplan::kFooterBytes;
    const uint64_t in_room = align_up(size_t(in_bytes), 256);
    const int enc = key.empty() ? 0 : 1;
    const uint64_t cap = cdc_encode_bound(index_len, compress, enc) + cdc_encode_bound(rplan::kFooterBytes, compress, enc) + 64;
    if (!h.reserve(size_t(std::max(in_bytes, cap))) || !d.reserve(size_t(in_room + cap))) return CDC_E_NOMEM;
    uint8_t *const hp = h.as<uint8_t>(), *const d_in = d.as<uint8_t>(), *const d_out = d_in + in_room;
    if (index_len) std::memcpy(hp, index, size_t(index_len));
    std::memset(hp + index_len, 0, size_t(foff - index_len));
    std::memcpy(hp + foff, footer52, rplan::kFooterBytes);
    if (hipMemcpyAsync(d_in, hp, size_t(in_bytes), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return CDC_E_DEVICE;
    const uint64_t off[2] = {0, foff}, len[2] = {index_len, rplan::kFooterBytes};
    uint64_t oo[3] = {0, 0, 0};
    int st = cdc_encode_device_level(device, d_in, off, len, 2, compress, key_ptr(), key.empty() ? nullptr : random,
                                     d_out, cap, oo, CDC_LEVEL_FAST, stream);
    if (st != CDC_OK) return st;
    uint8_t trailer[stplan::kTrailerBytes];
    uint64_t total = 0;
    st = stplan::make_trailer(0, oo[1] - oo[0], oo[2] - oo[1], trailer, &total);
    if (st != CDC_OK) return st;
    if (oo[2] && (hipMemcpyAsync(hp, d_out, size_t(oo[2]), hipMemcpyDeviceToHost, stream) != hipSuccess ||
                  hipStreamSynchronize(stream) != hipSuccess))
        return CDC_E_DEVICE;
    tail.assign(hp, hp + oo[2]);
    tail.insert(tail.end(), trailer, trailer + sizeof(trailer));
    return CDC_OK;
}

bool add_packfiles_invalid(const cdc_packfile_src *srcs, uint32_t n, const int32_t *status)
{
    if (n && (!srcs || !status)) return true;
    for (uint32_t i = 0; i < n; ++i) {
        const cdc_packfile_src &s = srcs[i];
        if (s.form != CDC_PACKFILE_PLAIN && s.form != CDC_PACKFILE_STORED && s.form != CDC_PACKFILE_ROWS) return true;
        if (!s.bytes && !s.path) return true;
        if (s.form == CDC_PACKFILE_ROWS && !s.rows) return true;
    }
    return false;
}

int add_packfiles(Locator &loc, std::unique_ptr<StoredCodec> &codec, int device, int compress, const uint8_t *key,
                  const cdc_packfile_src *srcs, uint32_t n, int32_t *status)
{
    // the stored sources, together, through the codec
    std::vector<uint32_t> at;
    std::vector<cdc_packfile_src> stored;
    for (uint32_t i = 0; i < n; ++i)
        if (srcs[i].form == CDC_PACKFILE_STORED) {
            at.push_back(i);
            stored.push_back(srcs[i]);
        }
    const uint32_t m = uint32_t(stored.size());
    std::vector<int32_t> sst(m);
    std::vector<cdc_packfile_footer> footer(m);
    std::vector<std::vector<cdc_packfile_row>> rows(m);
    std::vector<uint64_t> len(m);
    if (m) {
        if (!codec) {
            std::unique_ptr<StoredCodec> c(new StoredCodec());
            const int st = c->open(device, compress, key);
            if (st != CDC_OK) return st;
            codec = std::move(c);
        }
        const int st = codec->read_many(stored.data(), m, sst.data(), footer.data(), rows.data(), len.data());
        if (st != CDC_OK) return st;
    }
    // every source into the locator, in source order
    uint32_t k = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const cdc_packfile_src &s = srcs[i];
        if (s.form == CDC_PACKFILE_PLAIN) {
            status[i] = s.bytes ? loc.add_memory(s.bytes, s.len) : loc.add_path(s.path);
        } else if (s.form == CDC_PACKFILE_STORED) {
            status[i] = sst[k];
            if (status[i] == CDC_OK) loc.add_rows(Locator::Pack{s.bytes, s.bytes ? std::string() : std::string(s.path), len[k]}, rows[k]);
            ++k;
        } else {  // the caller's rows: nothing of the file but its length is read
            uint64_t L = s.len;
            status[i] = CDC_OK;
            if (!s.bytes && !Fd(s.path).length(&L)) status[i] = CDC_E_IO;
            for (uint64_t q = 0; q < s.nrows && status[i] == CDC_OK; ++q)
                if (uint64_t(s.rows[q].offset) + s.rows[q].length > L) status[i] = CDC_E_CORRUPT;
            if (status[i] == CDC_OK)
                loc.add_rows(Locator::Pack{s.bytes, s.bytes ? std::string() : std::string(s.path), L},
                             std::vector<cdc_packfile_row>(s.rows, s.rows + s.nrows));
        }
    }
    return CDC_OK;
}

int seal_stored(StoredCodec &codec, cdc_packer *p, int64_t timestamp, std::vector<uint8_t> &tail, const uint8_t **data,
                uint64_t *len)
{
    const uint8_t *index = nullptr;
    uint64_t index_len = 0;
    uint8_t footer[rplan::kFooterBytes];
    packer_tail_parts(p, timestamp, &index, &index_len, footer);
    const int st = codec.write_tail(index, index_len, footer, nullptr, tail);
    if (st != CDC_OK) return st;
    return packer_seal_tail(p, tail.data(), tail.size(), data, len);
}

}  // namespace cdc

extern "C" {

int cdc_packfile_index_stored(int device, const uint8_t *bytes, uint64_t len, int compress, const uint8_t *key,
                              cdc_packfile_footer *footer, cdc_packfile_row *rows, uint64_t cap, uint64_t *needed)
{
    if (!footer || (!bytes && len) || (!rows && cap) || device < 0 || device >= cdc::kMaxDevices) return CDC_E_INVALID;
    if (needed) *needed = 0;
    if (!bytes) return CDC_E_CORRUPT;
    try {
        cdc::StoredCodec codec;
        int st = codec.open(device, compress, key);
        if (st != CDC_OK) return st;
        cdc_packfile_src src{};
        src.bytes = bytes;
        src.len = len;
        src.form = CDC_PACKFILE_STORED;
        int32_t status = CDC_OK;
        std::vector<cdc_packfile_row> got;
        uint64_t flen = 0;
        st = codec.read_many(&src, 1, &status, footer, &got, &flen);
        if (st != CDC_OK) return st;
        if (status != CDC_OK) return status;
        std::copy(got.begin(), got.begin() + std::min<uint64_t>(cap, got.size()), rows);
        if (needed) *needed = footer->count;
        return footer->count > cap ? CDC_E_NOSPACE : CDC_OK;
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

uint64_t cdc_packer_stored_bound(const cdc_packer *p, int compress, int encrypt)
{
    if (!p) return 0;
    return cdc_packer_size(p) + cdc_encode_bound(rplan::kRowBytes * uint64_t(cdc_packer_count(p)), compress, encrypt) +
           cdc_encode_bound(rplan::kFooterBytes, compress, encrypt) + stplan::kTrailerBytes;
}

int cdc_packer_serialize_stored(const cdc_packer *p, int64_t timestamp, int device, int compress, const uint8_t *key,
                                const uint8_t *random, uint8_t *out, uint64_t cap, uint64_t *len)
{
    if (!p || !len || device < 0 || device >= cdc::kMaxDevices) return CDC_E_INVALID;
    try {
        const uint8_t *index = nullptr;
        uint64_t index_len = 0;
        uint8_t footer[rplan::kFooterBytes];
        cdc::packer_tail_parts(p, timestamp, &index, &index_len, footer);
        cdc::StoredCodec codec;
        int st = codec.open(device, compress, key);
        if (st != CDC_OK) return st;
        std::vector<uint8_t> tail;
        st = codec.write_tail(index, index_len, footer, random, tail);
        if (st != CDC_OK) return st;
        uint64_t data_len = 0;
        (void)cdc_packer_serialize_part(p, 0, timestamp, nullptr, 0, &data_len);
        *len = data_len + tail.size();
        if (*len > cap || !out) return CDC_E_NOSPACE;
        uint64_t got = 0;
        st = cdc_packer_serialize_part(p, 0, timestamp, out, data_len, &got);
        if (st != CDC_OK) return st;
        std::memcpy(out + data_len, tail.data(), tail.size());
        return CDC_OK;
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

}  // extern "C"
