// The stored-form codec (cdc_stored.cpp): Decode of the encoded footers and
// indexes of many stored packfiles in two device calls, and Encode of one
// packfile's index and footer in one.  DESIGN.md 5.22.  Internal.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "cdc_hostmem.h"
#include "cdc_internal.h"
#include "cdc_locator.h"

namespace cdc {

struct StoredCodec {
    int device = 0;
    int compress = CDC_COMPRESS_NONE;
    std::vector<uint8_t> key;  // 32 bytes, or empty
    hipStream_t stream = nullptr;
    PinBuf h;
    DevBuf d;

    StoredCodec() = default;
    StoredCodec(const StoredCodec &) = delete;
    StoredCodec &operator=(const StoredCodec &) = delete;
    ~StoredCodec();

    // CDC_OK, CDC_E_DEVICE.
    int open(int device, int compress, const uint8_t *key);
    const uint8_t *key_ptr() const { return key.empty() ? nullptr : key.data(); }

    // n stored packfiles (srcs[i].form is not looked at): status[i], and for
    // CDC_OK footer[i], rows[i] and len[i], the file's length.  Two
    // cdc_decode_device calls whatever n is (one more after a malformed source
    // made the first of either too small).  Returns the call's own failure
    // (CDC_E_DEVICE, CDC_E_NOMEM), else CDC_OK.
    int read_many(const cdc_packfile_src *srcs, uint32_t n, int32_t *status, cdc_packfile_footer *footer,
                  std::vector<cdc_packfile_row> *rows, uint64_t *len);

    // Encode(index) || Encode(footer) || trailer into `tail`, for a packfile
    // whose data section is data_len bytes.  random: 112 bytes (the index's 56,
    // then the footer's), or NULL: drawn here.  One cdc_encode_device_level.
    int write_tail(const uint8_t *index, uint64_t index_len, const uint8_t *footer52, const uint8_t *random,
                   std::vector<uint8_t> &tail);

private:
    int decode_batch(uint64_t in_bytes, const std::vector<uint64_t> &off, const std::vector<uint64_t> &len,
                     uint64_t expect, std::vector<uint64_t> &oo, std::vector<int32_t> &st, const uint8_t **plain);
};

// The body of every cdc_*_add_packfiles: `codec` is the context's own, made at
// its first stored source.  The caller has checked the arguments
// (add_packfiles_invalid) and holds the context's lock.
bool add_packfiles_invalid(const cdc_packfile_src *srcs, uint32_t n, const int32_t *status);
int add_packfiles(Locator &loc, std::unique_ptr<StoredCodec> &codec, int device, int compress, const uint8_t *key,
                  const cdc_packfile_src *srcs, uint32_t n, int32_t *status);

// packer_seal for the stored form: the packer's index and footer through the
// codec (`tail` is the caller's scratch), then appended to its data section;
// *data / *len hold the stored packfile until cdc_packer_reset.
int seal_stored(StoredCodec &codec, cdc_packer *p, int64_t timestamp, std::vector<uint8_t> &tail, const uint8_t **data,
                uint64_t *len);

int random_fill(uint8_t *p, size_t n);

}  // namespace cdc
