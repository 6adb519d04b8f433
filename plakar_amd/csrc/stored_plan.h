// Host-only pieces of the stored packfile form, shared by the library
// (cdc_stored.cpp) and the stand-alone sanitizer program
// tests/c/stored_plan_check.cpp.
//
// A repository keeps a packfile as snapshot.PutPackfile writes it
// (snapshot/snapshot.go:249-267; read back in cmd/plakar/subcommands/info/
// info.go:387-426):
//
//   data || Encode(index) || Encode(footer) || u32le version || u8 len(Encode(footer))
//
// The planner turns a file's length and last bytes into the encoded footer's
// range (split_tail), the decoded footer into the encoded index's range
// (index_range), and two encoded lengths into the writer's trailer
// (make_trailer).  The index rows themselves go through rplan::parse_index.
//
// No HIP, no library state: everything is a function of its arguments.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "plakar_cdc.h"
#include "restore_plan.h"

namespace stplan {

constexpr uint64_t kTrailerBytes = 5;     // u32le version, u8 len(Encode(footer))
constexpr uint64_t kMaxFooterCode = 255;  // the length field is one byte

struct Tail {
    uint32_t version;
    uint32_t L;            // len(Encode(footer))
    uint64_t footer_off;   // the encoded footer: bytes [footer_off, footer_off + L)
};

// `last5` are the file's last five bytes (not read when len < 5); `coded`: the
// repository has a key or a compression, so no Encode output is empty.
static inline int split_tail(const uint8_t *last5, uint64_t len, bool coded, Tail *t)
{
    memset(t, 0, sizeof(*t));
    if (len < kTrailerBytes) return CDC_E_CORRUPT;
    t->version = rplan::rd32(last5);
    t->L = last5[4];
    if (t->L == 0 && coded) return CDC_E_CORRUPT;
    if (uint64_t(t->L) + kTrailerBytes > len) return CDC_E_CORRUPT;
    if (t->version != rplan::kPackVersion) return CDC_E_CORRUPT;
    t->footer_off = len - kTrailerBytes - t->L;
    return CDC_OK;
}

// The most plaintext `enc_len` encoded bytes can decode to: Decode's own
// bounds.  The GCM envelope (60 bytes, then 28 per record of at most 65,564)
// comes off first, and a length Decode refuses (under 60, or a last record
// under 28) holds nothing; a GZIP member inflates to at most 1032 bytes per
// byte (include/plakar_cdc.h, Decode), an LZ4 block to at most 255.
static inline uint64_t inflate_bound(uint64_t enc_len, int compress, bool encrypted)
{
    uint64_t frame = enc_len;
    if (encrypted) {
        if (enc_len < 60) return 0;
        const uint64_t rem = enc_len - 60, nr = (rem + 65563) / 65564;
        if (nr && rem - (nr - 1) * 65564 < 28) return 0;
        frame = rem - 28 * nr;
    }
    const uint64_t per = compress == CDC_COMPRESS_GZIP ? 1032 : compress != CDC_COMPRESS_NONE ? 255 : 1;
    return frame > UINT64_MAX / per ? UINT64_MAX : frame * per;
}

struct IndexRange {
    uint64_t off, len;     // the encoded index: bytes [off, off + len)
    uint64_t plain;        // what it must decode to: 41 * count
};

// `footer` is Decode of the encoded footer (footer_len bytes of it), `t` what
// split_tail gave.  Fills *f and *r.  The row count is held against what the
// encoded index can inflate to before anything is sized from it.
static inline int index_range(const uint8_t *footer, uint64_t footer_len, const Tail &t, int compress, bool encrypted,
                              cdc_packfile_footer *f, IndexRange *r)
{
    memset(f, 0, sizeof(*f));
    memset(r, 0, sizeof(*r));
    if (footer_len != rplan::kFooterBytes) return CDC_E_CORRUPT;
    f->version = rplan::rd32(footer);
    f->timestamp = int64_t(rplan::rd64(footer + 4));
    f->count = rplan::rd32(footer + 12);
    f->index_offset = rplan::rd32(footer + 16);
    memcpy(f->index_checksum, footer + 20, 32);
    if (f->version != t.version) return CDC_E_CORRUPT;
    if (f->index_offset > t.footer_off) return CDC_E_CORRUPT;
    r->off = f->index_offset;
    r->len = t.footer_off - f->index_offset;
    r->plain = rplan::kRowBytes * uint64_t(f->count);
    if (r->plain > inflate_bound(r->len, compress, encrypted)) return CDC_E_CORRUPT;
    return CDC_OK;
}

// The writer's side: after `data_len` bytes of blobs come enc_index and
// enc_footer bytes of the two encodings, then trailer[5].
static inline int make_trailer(uint64_t data_len, uint64_t enc_index, uint64_t enc_footer, uint8_t trailer[5],
                               uint64_t *total)
{
    if (enc_footer > kMaxFooterCode) return CDC_E_UNSUPPORTED;
    const uint32_t v = rplan::kPackVersion;
    trailer[0] = uint8_t(v), trailer[1] = uint8_t(v >> 8), trailer[2] = uint8_t(v >> 16), trailer[3] = uint8_t(v >> 24);
    trailer[4] = uint8_t(enc_footer);
    *total = data_len + enc_index + enc_footer + kTrailerBytes;
    return CDC_OK;
}

}  // namespace stplan
