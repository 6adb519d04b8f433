/*
 * plakar_cdc.h — C ABI of the MI355X content-defined chunker (libplakar_cdc.so).
 *
 * Drop-in boundary for plakar's chunking path.  Every entry point below names
 * the reference interface it replaces.  Reference paths are relative to the
 * plakar tree; "ext" marks the third-party Go module
 * github.com/PlakarKorp/go-cdc-chunkers v0.0.8 (go.mod:37), whose source is not
 * vendored in the reference.
 *
 * Plain C types only: no HIP or torch types appear in any signature.  Device
 * pointers are `void *`, and HIP streams are passed as `void *` (a hipStream_t,
 * or NULL for the null stream).  No call throws.  Every call returns an int
 * status: CDC_OK / CDC_EOF / CDC_NEED_DATA (>= 0) or a negative CDC_E_* code.
 * cdc_strerror() turns a status into text.
 *
 * Streams.  Every device entry point takes the caller's stream and states one
 * of two contracts.  "Synchronous on `stream`": all device work is ordered
 * after what `stream` already holds, and the call returns once that work has
 * finished and `stream` is drained, so device outputs may be read from any
 * stream and host outputs are final.  "Asynchronous on `stream`": the call
 * enqueues its work in stream order and returns without waiting for what the
 * stream holds (it may wait for an earlier call of its own whose table slot it
 * takes again); the outputs are ready for work enqueued on `stream` after it.
 * Either way the call waits for no other stream of the caller, and the host
 * arrays passed in (offsets, lengths, segment and record tables, keys, random
 * bytes) may be reused as soon as it returns: they are copied into pinned
 * staging, or passed as kernel arguments, before that.  Side streams and
 * events of the library's own are forked from and joined back to `stream`
 * inside the call.
 *
 * The product never falls back to the CPU.  If no GPU is present, or the HIP
 * runtime fails, calls return CDC_E_DEVICE / CDC_E_NO_DEVICE.
 */
#ifndef PLAKAR_CDC_H
#define PLAKAR_CDC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CDC_ABI_VERSION 1

/* ---- status codes --------------------------------------------------------- */
#define CDC_OK 0
#define CDC_EOF 1           /* io.EOF: the stream is drained (Next() returned its last chunk) */
#define CDC_NEED_DATA 2     /* streaming: append more bytes (or mark EOF) before the next chunk */
#define CDC_E_INVALID (-1)  /* bad argument (NULL pointer, bad length, misaligned, ...) */
#define CDC_E_UNSUPPORTED (-2) /* algorithm not implemented here (e.g. "ultracdc") */
#define CDC_E_NOSPACE (-3)  /* output array too small; the needed count is reported */
#define CDC_E_DEVICE (-4)   /* HIP runtime / kernel failure */
#define CDC_E_NOMEM (-5)    /* host or device allocation failed */
#define CDC_E_NORMAL_SIZE (-6) /* ext fastcdc ErrNormalSize */
#define CDC_E_MIN_SIZE (-7)    /* ext fastcdc ErrMinSize */
#define CDC_E_MAX_SIZE (-8)    /* ext fastcdc ErrMaxSize */
#define CDC_E_IO (-9)       /* a reader callback reported an error */
#define CDC_E_NOT_INIT (-10) /* cdc_init() has not been called */
#define CDC_E_NO_DEVICE (-11) /* no HIP device visible */

/* ---- data types -------------------------------------------------------------- */

/* chunkers.ChunkerOpts (ext chunker.go; used at repository/repository.go:288-292,
 * chunking/chunking_test.go:19-23).  Sizes in bytes. */
typedef struct cdc_opts {
    uint32_t min_size;
    uint32_t normal_size;
    uint32_t max_size;
    uint32_t reserved; /* must be 0 */
} cdc_opts;

/* One chunk: [offset, offset + length) of its buffer.  plakar stores only the
 * length (objects.Chunk.Length, objects/objects.go:73-79); the offsets are the
 * prefix sums the VFS walks (snapshot/vfs/vfilep.go:30-49). */
typedef struct cdc_cut {
    uint64_t offset;
    uint32_t length;
    uint32_t reserved;
} cdc_cut;

/* An independent input buffer (one file, or a window of one). */
typedef struct cdc_buf {
    const void *data;
    uint64_t len;
} cdc_buf;

/* Device-side result block, written by the device path.  Read it after the
 * stream has been synchronised. */
typedef struct cdc_result {
    uint64_t ncuts;    /* chunks written (final chunk included when final != 0) */
    uint64_t consumed; /* bytes covered by the written chunks (== len when final) */
    int64_t status;    /* CDC_OK, or CDC_E_NOSPACE */
    uint64_t needed;   /* chunks needed when status == CDC_E_NOSPACE */
} cdc_result;

/* ---- library setup ------------------------------------------------------------ */

/* Initialise the library on the devices in dev_mask (bit i = HIP device i;
 * 0 = every visible device).  gear = 256-entry Gear table of
 * ext chunkers/fastcdc (the package-level G), or NULL for the built-in
 * placeholder table (see cdc_default_gear).  mask_s / mask_l = the FastCDC
 * small/large masks (0 selects the defaults 0x0003590703530000 /
 * 0x0000d90003530000).  cut_convention: 0 = Algorithm returns i (the chunk
 * excludes the byte whose fingerprint matched), 1 = returns i + 1.
 * May be called again to change the parameters: it waits for the devices to
 * go idle first, and must not race with other calls.  A different device set
 * returns CDC_E_INVALID (call cdc_shutdown() first).  A failure leaves the
 * library uninitialised with nothing allocated. */
int cdc_init(uint32_t dev_mask, const uint64_t gear[256], uint64_t mask_s, uint64_t mask_l,
             int cut_convention);
/* 1 while the table in use is the built-in placeholder (cdc_init with gear ==
 * NULL): cut points then differ from plakar's; pass the real fastcdc.G. */
int cdc_gear_is_placeholder(void);
void cdc_shutdown(void);
const char *cdc_strerror(int status);
int cdc_abi_version(void);
int cdc_device_count(void);

/* The built-in Gear table: a PLACEHOLDER (splitmix64 from a fixed seed).  The
 * v0.0.8 table of ext chunkers/fastcdc is not available in this build (see
 * DESIGN.md, "Oracle").  Pass the real table to cdc_init() once it is. */
void cdc_default_gear(uint64_t out[256]);
uint64_t cdc_default_mask_s(void);
uint64_t cdc_default_mask_l(void);

/* ext fastcdc (*FastCDC).Validate + chunkers.NewChunker's registry lookup
 * (algorithm names are matched after lower-casing, as
 * repository/repository.go:288 does).  Returns CDC_OK, CDC_E_UNSUPPORTED or
 * CDC_E_{NORMAL,MIN,MAX}_SIZE. */
int cdc_validate(const char *algorithm, const cdc_opts *opts);

/* chunking.DefaultConfiguration() (chunking/chunking.go:10-17). */
void cdc_default_opts(cdc_opts *out);

/* ---- batch path: host buffers in, host cut lists out ---------------------------
 * Replaces the per-file loop `chk := repo.Chunker(rd); for { chk.Next() }`
 * (snapshot/backup.go:647-665) for a batch of whole files already in host
 * memory.  Each buffer is chunked independently, as one complete stream.
 * out receives the cuts of buffer 0, then buffer 1, ...; out_counts[i] = the
 * number of cuts of buffer i.  If out_cap is too small, returns CDC_E_NOSPACE
 * with *out_needed set (out_needed may be NULL).  Synchronous. */
int cdc_chunk(const cdc_buf *bufs, int nbufs, const cdc_opts *opts, cdc_cut *out,
              uint64_t out_cap, uint64_t *out_counts, uint64_t *out_needed);

/* ---- collector: concurrent per-file callers -> device batches -------------------
 * plakar chunks each file in its own goroutine (snapshot/backup.go:216-225,
 * each running the Next() loop of backup.go:647-665).  A collector takes such
 * per-file calls from any number of threads and submits them to the devices
 * as batches: a batch closes at batch_bytes (0: 256 MiB), at 32 files, or
 * max_wait_us after its first file arrived; each device runs its batches
 * through a two-slot pipeline (batch k + 1 staged while batch k is chunked).
 * cdc_collector_chunk blocks until the caller's own cut list is back and has
 * cdc_chunk's contract for one buffer (CDC_E_NOSPACE with *count set when cap
 * is too small).  cdc_collector_free drains pending calls, then stops. */
typedef struct cdc_collector cdc_collector;
int cdc_collector_new(const cdc_opts *opts, uint64_t batch_bytes, uint32_t max_wait_us, cdc_collector **out);
int cdc_collector_chunk(cdc_collector *c, const void *data, uint64_t len, cdc_cut *out, uint64_t cap,
                        uint64_t *count);
int cdc_collector_stats(cdc_collector *c, uint64_t *requests, uint64_t *batches);
void cdc_collector_free(cdc_collector *c);

/* ---- Encode: LZ4 frame or gzip member, then the AES-256-GCM stream --------------
 * (*Repository).Encode (repository/repository.go:212-236) of n blobs that sit
 * in device memory at d_base + offsets[i], lens[i] bytes each:
 *   compress: Decode's selector (CDC_COMPRESS_NONE, _LZ4, _GZIP below; every
 *     other non-zero value means LZ4).
 *   compress == CDC_COMPRESS_LZ4: the LZ4 frame of compression.DeflateLZ4Stream
 *     (compression/compression.go:94-106; pierrec/lz4/v4 writer defaults:
 *     4-MiB independent blocks, content checksum; a block that does not
 *     shrink is stored);
 *   compress == CDC_COMPRESS_GZIP: the gzip member of
 *     compression.DeflateGzipStream (compression.go:78-92): the ten header
 *     bytes Go's gzip.NewWriter writes (1f 8b 08, no flags, MTIME 0, XFL 0,
 *     OS 255), one DEFLATE stream, CRC-32 and ISIZE, nothing after them.  The
 *     DEFLATE bytes are not Go's (compress/flate level 6): each 32-KiB span
 *     is one block, stored, fixed or dynamic Huffman, whichever is smallest,
 *     with matches inside 8-KiB segments; any inflater reads them.  An empty
 *     blob is an empty stream (compression.go:58-62) under either name.  A
 *     blob of 2 GiB or more is CDC_E_UNSUPPORTED (ISIZE is 32 bits and Decode
 *     refuses such a stream), reported before the device is touched;
 *   key != NULL (32 bytes, host memory): then encryption.EncryptStream
 *     (encryption/symmetric.go:72-163): subkey nonce (12) || Seal(key,
 *     subkey nonce, subkey) (48) || per 64-KiB piece k of the stream: nonce
 *     (12) || Seal(subkey, nonce, piece).  random (host, 56 bytes per blob:
 *     subkey 32, subkey nonce 12, data nonce 12) supplies what crypto/rand
 *     supplies in the reference; piece k's nonce is the data nonce with its
 *     last four bytes XOR k (big-endian).
 * Blob i's encoding lands at d_out + out_offsets[i] (device memory; host
 * array of n + 1 offsets, out_offsets[n] = total).  Returns CDC_E_NOSPACE
 * when out_cap is smaller than out_offsets[n], CDC_E_INVALID for a NULL
 * argument or a device outside 0..63.  Synchronous on `stream`. */
int cdc_encode_device(int device, const void *d_base, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                      int compress, const uint8_t *key, const uint8_t *random, uint8_t *d_out, uint64_t out_cap,
                      uint64_t *out_offsets, void *stream);

/* The compression level: compression.Configuration carries a Level beside the
 * algorithm (compression/compression.go:12-51), and the reference's GZIP is
 * flate level 6, a 32-KiB window.  Here the level chooses the match search:
 *   CDC_LEVEL_FAST (0): matches inside their 8-KiB segment (what
 *     cdc_encode_device writes);
 *   CDC_LEVEL_WIDE (1): a match may also copy from up to 32,768 bytes before
 *     its segment, never from before its 4-MiB block (LZ4's blocks stay
 *     independent; DEFLATE uses the same floor) nor from before its blob, piece
 *     or zip entry.  Smaller output, a slower search; the formats, the bounds
 *     and every reader are the same;
 *   CDC_LEVEL_BEST (9, gzip.BestCompression): the smallest the device writes.
 *     CDC_LEVEL_WIDE's window and floors, with four earlier occurrences kept
 *     per hash bucket, the longest of them taken, and a lazy look: a match
 *     gives way to a strictly longer one that starts one byte later.  Slower
 *     again; the formats, the bounds and every reader are the same.
 * Every other value (2, 3, 6, -1, ...) is CDC_E_INVALID; with CDC_COMPRESS_NONE
 * the level changes nothing.  cdc_transcode_device and cdc_backup_run are
 * their _level forms at CDC_LEVEL_FAST. */
#define CDC_LEVEL_FAST 0
#define CDC_LEVEL_WIDE 1
#define CDC_LEVEL_BEST 9

/* cdc_encode_device at `level` (compression/compression.go:12-51): the level
 * changes which matches the LZ4 frame's sequences or the gzip member's blocks
 * hold, so the bytes and their count, nothing else.  cdc_encode_device is this
 * call with CDC_LEVEL_FAST.  Synchronous on `stream`. */
int cdc_encode_device_level(int device, const void *d_base, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                            int compress, const uint8_t *key, const uint8_t *random, uint8_t *d_out, uint64_t out_cap,
                            uint64_t *out_offsets, int level, void *stream);

/* Upper bound of one blob's encoding (for out_cap); `compress` is the selector.
 * It holds at either level.
 * GZIP: len + 18 + 5 * (ceil(len / 32768) + 1) before encryption (a span is
 * coded only when that is no larger than storing it). */
uint64_t cdc_encode_bound(uint64_t len, int compress, int encrypt);

/* ---- A gzip member written piece by piece ----------------------------------------
 * The output pieces of one writer, concatenated, are one RFC 1952 member of
 * the concatenated inputs, as gzip.NewWriter(out) ... Close() gives (the
 * DEFLATE bytes are cdc_encode_device's kind, not Go's):
 *   - the first piece starts with cdc_encode_device's ten header bytes;
 *   - a piece is DEFLATE blocks with BFINAL clear, one per 32-KiB span, stored,
 *     fixed or dynamic, whichever is smallest at the bit where it starts;
 *   - an empty stored block (000, zeros to the byte boundary, 00 00 ff ff)
 *     ends every piece on a byte boundary;
 *   - the piece given with last != 0 then adds the final empty block
 *     (01 00 00 ff ff), the CRC-32 of the whole stream and ISIZE, the
 *     stream's length mod 2^32: a stream may be 4 GiB or longer.
 * A stream with no bytes at all is still a whole member (header, final block,
 * trailer).  len == 0 with last == 0 writes nothing.  A piece of 2 GiB or
 * more is CDC_E_UNSUPPORTED.  d_in and d_out are device memory; the call is
 * synchronous on `stream`, and calls on one writer are serialised.
 * *out_len: the bytes written at d_out.  CDC_E_NOSPACE when out_cap is
 * smaller, with *out_len the bytes needed, nothing written and the writer
 * unchanged (the piece may be given again).  After the last piece every
 * further piece is CDC_E_INVALID.  cdc_gzip_stream_bound(len): the most one
 * call with len input bytes writes, header, joiner and trailer included. */
typedef struct cdc_gzip_stream cdc_gzip_stream;
int cdc_gzip_stream_new(int device, cdc_gzip_stream **out);
uint64_t cdc_gzip_stream_bound(uint64_t len);
int cdc_gzip_stream_piece(cdc_gzip_stream *s, const void *d_in, uint64_t len, int last, uint8_t *d_out,
                          uint64_t out_cap, uint64_t *out_len, void *stream);
void cdc_gzip_stream_free(cdc_gzip_stream *s);
/* The level of the member's match search (compression/compression.go:12-51;
 * CDC_LEVEL_* above): with CDC_LEVEL_WIDE a match reaches up to 32,768 bytes
 * back inside its piece, never into the piece before.  A member is written at
 * one level: CDC_E_INVALID once a piece has been written.  The bound holds. */
int cdc_gzip_stream_set_level(cdc_gzip_stream *s, int level);

/* ---- Many raw DEFLATE streams in one call (zip entries) --------------------------
 * What compress/flate does under archive/zip's fileWriter
 * (cmd/plakar/subcommands/archive/archive.go:194-245 through zip.Writer's
 * CreateHeader, one flate.NewWriter per entry), for n pieces that lie in one
 * device buffer, into one device output, back to back in piece order.  A piece
 * is an entry of the zip or, for an entry that spans calls, one part of it:
 *   - a piece starts at bit 0 and is DEFLATE blocks, one per 32-KiB span, as
 *     cdc_encode_device's GZIP members hold them (no ten-byte header);
 *   - `first`: the entry's local file header (hdr_len > 0 bytes at
 *     hdr_arena + hdr_off, host memory) goes before the deflate bytes;
 *   - `last`: the piece's last block carries BFINAL and the stream ends at the
 *     next byte boundary; an entry with no bytes at all (first and last,
 *     len 0) is 01 00 00 ff ff.  Then comes the data descriptor: 50 4b 07 08,
 *     the entry's CRC-32 (crc_reg: the register over the entry before this
 *     piece, from 0xFFFFFFFF), its compressed and uncompressed size
 *     (csize_before, usize_before plus this piece), 4 bytes each, or 8 bytes
 *     each when either is 0xFFFFFFFF or more (archive/zip's isZip64);
 *   - a piece that is not last ends with an empty stored block (000, zeros to
 *     the byte boundary, 00 00 ff ff), so the entry's next piece, in a later
 *     call, continues the stream; an empty one writes no deflate bytes.
 * Per piece the call reports where it lies in d_out (out_off, out_len, the
 * header and descriptor included), its deflate bytes, its CRC-32 register from
 * 0 (the caller's running register r becomes crc_mul(r, x^(8 len)) ^ crc_reg,
 * as cdc_gzip_stream_piece keeps it) and whether the descriptor is the 64-bit
 * one; *total is the sum of out_len.  CDC_E_NOSPACE when out_cap is smaller
 * than *total: *total is still set, nothing is written.  A piece of 2 GiB or
 * more is CDC_E_UNSUPPORTED; a first piece without a header, a header outside
 * the arena or a piece outside [0, src_cap) is CDC_E_INVALID.  The call keeps a
 * workspace of its own per device, is synchronous on `stream`, and calls on
 * one device are serialised. */
typedef struct cdc_zip_piece {
    uint64_t src_off, len;     /* in d_src */
    uint32_t first, last;
    uint32_t hdr_off, hdr_len; /* in hdr_arena (first pieces) */
    uint32_t crc_reg;          /* the entry's CRC-32 register before this piece (0xFFFFFFFF at its start) */
    uint32_t reserved;         /* 0 */
    uint64_t csize_before, usize_before;
} cdc_zip_piece;
typedef struct cdc_zip_piece_out {
    uint64_t out_off, out_len; /* in d_out: header, deflate bytes, descriptor */
    uint64_t deflate_len;
    uint32_t crc_reg;          /* over this piece's bytes, from 0, no final inversion */
    uint32_t zip64;            /* last pieces: the descriptor holds 8-byte sizes */
} cdc_zip_piece_out;
int cdc_zip_pieces_device(int device, const void *d_src, uint64_t src_cap, const cdc_zip_piece *pieces, uint32_t n,
                          const uint8_t *hdr_arena, uint64_t hdr_arena_len, uint8_t *d_out, uint64_t out_cap,
                          cdc_zip_piece_out *outs, uint64_t *total, void *stream);
/* cdc_zip_pieces_device at `level` (compression/compression.go:12-51; CDC_LEVEL_*
 * above): with CDC_LEVEL_WIDE a match reaches up to 32,768 bytes back inside
 * its piece, never into another piece.  cdc_zip_pieces_device is this call
 * with CDC_LEVEL_FAST.  Synchronous on `stream`. */
int cdc_zip_pieces_device_level(int device, const void *d_src, uint64_t src_cap, const cdc_zip_piece *pieces, uint32_t n,
                                const uint8_t *hdr_arena, uint64_t hdr_arena_len, uint8_t *d_out, uint64_t out_cap,
                                cdc_zip_piece_out *outs, uint64_t *total, int level, void *stream);

/* ---- Decode: open the AES-256-GCM stream, then inflate (LZ4 or GZIP) -------------
 * (*Repository).Decode (repository/repository.go:186-210) of n encoded blobs
 * that sit in device memory at d_in + offsets[i], lens[i] bytes each:
 *   key != NULL (32 bytes, host memory): encryption.DecryptStream
 *     (encryption/symmetric.go:165-243): the subkey is opened from the first
 *     60 bytes, then every record nonce (12) || ciphertext (<= 65536) || tag
 *     (16) with the nonce it carries; record boundaries follow from the
 *     length, min(remaining, 65580) bytes each.  A blob under 60 bytes or a
 *     trailing record under 28 is CDC_E_CORRUPT (the reference takes exactly
 *     12 trailing bytes for a clean end; no writer produces them and they are
 *     rejected here), a tag that does not verify CDC_E_AUTH.
 *   compressed == CDC_COMPRESS_LZ4 (1; or any value but 0 and 2):
 *     compression.InflateLZ4Stream (compression/compression.go:148-160;
 *     empty input is an empty blob, compression.go:108-116): one LZ4 frame
 *     of independent blocks, any block maximum, with or without block
 *     checksums, content size and content checksum, all verified
 *     (CDC_E_CORRUPT).  Linked blocks, a dictionary ID, skippable and legacy
 *     frames are CDC_E_UNSUPPORTED (pierrec/lz4 v4's writer makes none).
 *   compressed == CDC_COMPRESS_GZIP (2): compression.InflateGzipStream
 *     (compression/compression.go:32-55, 108-146, over Go's compress/gzip;
 *     the other algorithm a repository's configuration may name): one gzip
 *     member (RFC 1952) whose
 *     body is DEFLATE (RFC 1951: stored, fixed and dynamic blocks), the
 *     optional header fields skipped (FHCRC verified), CRC-32 and ISIZE
 *     verified.  A malformed header, block, code set, distance or trailer is
 *     CDC_E_CORRUPT (plakar_amd/csrc/inflate_walk.h has the list); so is an
 *     ISIZE of more than 1032 bytes per body byte, which DEFLATE cannot
 *     reach, so a few bytes cannot make the call ask for gigabytes.  A second
 *     member after the first and a stream of 2 GiB or more are
 *     CDC_E_UNSUPPORTED (Go's writer makes neither).  Empty input is an empty
 *     blob.  There is no preset dictionary.
 *   The selector: CDC_COMPRESS_NONE (0), CDC_COMPRESS_LZ4 (1), CDC_COMPRESS_GZIP
 *     (2).  Any other non-zero value means LZ4, as it did before GZIP existed.
 *     cdc_decode_device, cdc_check_device, cdc_restore_opts.compress,
 *     cdc_encode_device, cdc_encode_bound and cdc_backup_opts.compress take it.
 *   compressed == 0 and key == NULL: a plain copy.
 * Blob i's plaintext lands at d_out + out_offsets[i] (host array of n + 1,
 * out_offsets[n] = total), blobs packed without padding, so (out_offsets[i],
 * out_offsets[i + 1] - out_offsets[i]) is a cdc_cut for the digest entry
 * points.  Returns CDC_OK whenever the batch ran: status[i] (host, n) is
 * CDC_OK or blob i's error, and a failed blob contributes 0 bytes.  Decoded
 * sizes are not stored in the blobs, so the call sizes them on the device
 * first: when they exceed out_cap it returns CDC_E_NOSPACE with
 * out_offsets[n] the capacity needed and nothing written (d_out may be NULL
 * when out_cap is 0).  d_out[out_offsets[n], out_cap) is scratch for the
 * call: an LZ4 frame whose content checksum fails, and a gzip member with any
 * fault in its body or trailer, is found out only after it was (partly)
 * written into its planned range, the blobs after it are then moved down
 * over it, and the bytes between the final out_offsets[n] and the total
 * planned before that failure are left overwritten.  Keep nothing of your own behind out_offsets[n] in
 * the same buffer.  Synchronous on `stream`. */
#define CDC_COMPRESS_NONE 0
#define CDC_COMPRESS_LZ4  1
#define CDC_COMPRESS_GZIP 2
#define CDC_E_AUTH     (-12) /* a GCM tag did not verify (sealed subkey or a data record) */
#define CDC_E_CORRUPT  (-13) /* malformed stream: short record, bad LZ4 frame/block or gzip member, checksum or size mismatch */
#define CDC_E_MISMATCH (-14) /* cdc_check_device: decoded fine, SHA-256 differs from the expected checksum */
int cdc_decode_device(int device, const void *d_in, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                      int compressed, const uint8_t *key, uint8_t *d_out, uint64_t out_cap, uint64_t *out_offsets,
                      int32_t *status, void *stream);

/* cdc_decode_device for the first upto[i] plaintext bytes of blob i: what a
 * reader of a byte range needs (VFilep.Read, snapshot/vfs/vfilep.go:58-122,
 * decodes the whole chunk for every call).  The decode chains are serial, so a
 * walk that stops at upto[i] costs in proportion to upto[i].
 *   The caller knows every blob's recorded length, so there is no sizing pass:
 *   out_offsets (host, n + 1) is the exclusive sum of upto, computed before
 *   anything is launched; out_cap < out_offsets[n] is CDC_E_NOSPACE with
 *   nothing launched.  Blob i's prefix lands at d_out + out_offsets[i].
 *   Nothing at or beyond d_out + out_offsets[n] is written: no scratch tail,
 *   no compaction.  A failed blob leaves its own range undefined and no other.
 *   The sequence (literal run, stored block, match) that crosses upto[i] is
 *   cut to the byte and the walk ends there, CDC_OK.  What the stream holds
 *   after it is not validated and need not be well formed: the rest of the
 *   block, later blocks, the end mark, the LZ4 content checksum, the gzip
 *   CRC-32 and ISIZE.  When the stream produces exactly upto[i] bytes and the
 *   walk reaches its end, everything cdc_decode_device verifies is verified,
 *   with its status codes.  (An LZ4 frame is at its end when the end mark
 *   follows the block that produced byte upto[i] - 1; a gzip member when the
 *   final block closes without another output byte.)
 *   A stream that ends before upto[i] bytes is CDC_E_MISMATCH.  upto[i] == 0
 *   is CDC_OK with nothing of the blob read.  upto[i] >= 2^32 is
 *   CDC_E_UNSUPPORTED for that blob.
 *   key != NULL with a compression: every record of the blob is opened (the
 *   compressed length of a prefix is not known before the walk), so a bad tag
 *   anywhere is CDC_E_AUTH for any upto[i] > 0.  With CDC_COMPRESS_NONE only
 *   records 0 .. ceil(upto[i] / 65536) - 1 are opened; a bad tag in a later
 *   record does not fail the prefix, and the blob may be passed without its
 *   later records (lens[i] = 60 + 65564 per record kept).
 * Synchronous on `stream`.  CDC_E_INVALID for a NULL array or device out of
 * range, before the device is touched. */
int cdc_decode_prefix_device(int device, const void *d_in, const uint64_t *offsets, const uint64_t *lens,
                             const uint64_t *upto, uint32_t n, int compressed, const uint8_t *key, uint8_t *d_out,
                             uint64_t out_cap, uint64_t *out_offsets, int32_t *status, void *stream);

/* The blob check of snapshot/check.go:83-98 (decode, hash, compare with the
 * index checksum) without the plaintext leaving the device: decodes into
 * d_scratch as cdc_decode_device does (CDC_E_NOSPACE and *needed, when given,
 * the capacity to retry with), hashes every blob that decoded with the
 * SHA-256 kernels of cdc_chunk_digests_device_async (so cdc_init must have
 * run) and compares with checksums (host, 32 bytes per blob) on the device.
 * status[i]: CDC_OK, CDC_E_MISMATCH, or blob i's decode error.  Synchronous on
 * `stream`. */
int cdc_check_device(int device, const void *d_in, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                     int compressed, const uint8_t *key, const uint8_t *checksums, uint8_t *d_scratch,
                     uint64_t scratch_cap, uint64_t *needed, int32_t *status, void *stream);

/* ---- Transcode: a blob of one repository as a blob of another ---------------------
 * What `plakar sync` does to every blob the destination lacks (synchronize,
 * cmd/plakar/subcommands/sync/sync.go:182-266): GetBlob decodes it with the
 * source repository's compression and key (repository/repository.go:186-210,
 * 407-429), PutBlob encodes it with the destination's (repository.go:212-236,
 * snapshot/blobs.go:9-24).  A codec is one side's configuration: the
 * compression selector above and the 32-byte repository key (host memory), or
 * NULL when that side is not encrypted. */
typedef struct cdc_codec {
    int compress;        /* CDC_COMPRESS_NONE, _LZ4 or _GZIP */
    const uint8_t *key;  /* 32 bytes, or NULL */
} cdc_codec;

/* The exact stored length after a transcode that keeps the compression (the
 * same selector on both sides) of a blob of `len` stored bytes: the GCM
 * envelope of encryption.EncryptStream (encryption/symmetric.go:72-163) taken
 * off, put on, or exchanged (then the length stays).  CDC_E_CORRUPT for a
 * length no writer produces (an encrypted source under 60 bytes, or with a
 * trailing record under 28, as cdc_decode_device).  Host only; needs no
 * cdc_init. */
int64_t cdc_transcode_size(uint64_t len, int src_encrypted, int dst_encrypted);

/* synchronize's GetBlob + PutBlob (sync.go:182-266) for n stored blobs that sit
 * in device memory at d_in + offsets[i], lens[i] bytes each.  The host decides
 * the path from the two codecs:
 *   same compression, both keys: the re-key.  Only the envelope changes (the
 *     sealed subkey, the nonces, the ciphertext and the tags); the compressed
 *     bytes inside it are carried over, and the plaintext never exists in
 *     device memory: one kernel authenticates each record under the source
 *     subkey (every tag compared in full: CDC_E_AUTH), exchanges the two
 *     keystreams in registers and seals it under the destination's.  Output
 *     length = input length; record k of a blob carries the blob's data nonce
 *     with its last four bytes XOR k, as cdc_encode_device writes it.
 *   same compression, only the source key: cdc_decode_device with compressed = 0.
 *   same compression, only the destination key: cdc_encode_device with
 *     compress = 0 over the stored bytes.
 *   same compression, no key: a copy.
 *   different compression: cdc_decode_device into a workspace the library keeps
 *     per device, then cdc_encode_device from there, over the blobs that
 *     decoded only (a failed blob is never encoded as an empty one).  The
 *     plaintext stays on the device.
 * checksums (host, 32 bytes per blob, or NULL): when given, every blob is
 * first checked as cdc_check_device does (decoded into the workspace, SHA-256,
 * compared); one that fails gets its decode error or CDC_E_MISMATCH and is
 * left out of the path that follows.  Without checksums the same-compression
 * paths trust the envelope and do not inflate: an encrypted source is
 * authenticated by its tags, an unencrypted one is copied unvalidated.  The
 * reference always inflates in GetBlob, so a caller who wants to be at least
 * as strict passes the index checksums.
 * random (host, 56 bytes per blob of the batch, as cdc_encode_device: subkey
 * 32, subkey nonce 12, data nonce 12) is needed when dst->key is set; row i
 * belongs to blob i whether or not other blobs fail.
 * Blob i's new encoding lands at d_out + out_offsets[i] (host array of n + 1,
 * out_offsets[n] = total), packed without padding.  Returns CDC_OK whenever
 * the batch ran: status[i] (host, n) is CDC_OK or blob i's error, and a failed
 * blob contributes 0 bytes.  CDC_E_NOSPACE comes with out_offsets[n] = the
 * capacity needed and nothing written (d_out may be NULL when out_cap is 0);
 * on the re-key path that is the sum of the well-formed blobs' lengths.
 * d_out[out_offsets[n], out_cap) is scratch for the call, as for
 * cdc_decode_device: a blob whose tag fails is found out after its planned
 * range was (partly) written, the blobs after it are then moved down over it,
 * and the bytes between the final out_offsets[n] and the total planned before
 * are left overwritten.  [d_in, ...) and [d_out, + out_cap) must not overlap.
 * CDC_E_INVALID: a NULL argument, a device outside 0..63, dst->key without
 * random, or a batch of more than 2^31 - 1 GCM records; CDC_E_NOT_INIT before
 * cdc_init.  Every read stays inside its blob and every write inside
 * d_out[0, out_cap).  Synchronous on `stream`. */
int cdc_transcode_device(int device, const void *d_in, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                         const cdc_codec *src, const cdc_codec *dst, const uint8_t *checksums, const uint8_t *random,
                         uint8_t *d_out, uint64_t out_cap, uint64_t *out_offsets, int32_t *status, void *stream);

/* cdc_transcode_device with the re-encode path's Encode at `level`
 * (compression/compression.go:12-51; CDC_LEVEL_* above).  The re-key path, the
 * paths that only open, seal or copy, and a destination without compression
 * ignore it; a level that does not exist is CDC_E_INVALID on every path.
 * cdc_transcode_device is this call with CDC_LEVEL_FAST.  Synchronous on
 * `stream`. */
int cdc_transcode_device_level(int device, const void *d_in, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                               const cdc_codec *src, const cdc_codec *dst, const uint8_t *checksums,
                               const uint8_t *random, uint8_t *d_out, uint64_t out_cap, uint64_t *out_offsets,
                               int32_t *status, int level, void *stream);

/* ---- packfile builder: the consumer of the cut lists ---------------------------
 * snapshot/packer.go + packfile/packfile.go: blobs are appended to a
 * packfile whose bytes are those of (*PackFile).Serialize (packfile.go:241-294):
 * Blobs, then per blob {u8 type, 32-B checksum, u32 offset, u32 length}, then
 * the footer {u32 version 100, i64 timestamp, u32 count, u32 index offset,
 * 32-B SHA-256 of the index}, all little-endian.
 *   cdc_packer_add_blob    Packer.AddBlob; returns 1 once Size() > MaxSize
 *                          (packerJob's flush rule, snapshot/snapshot.go:71)
 *   cdc_packer_add_chunks  TYPE_CHUNK blobs base[cuts[i]] with digests[32 i]
 *                          (k_chunk_digest's output), rows with skip[i] != 0
 *                          skipped (BlobExists); stops after the blob that
 *                          fills the packfile; returns rows consumed
 *   cdc_packer_serialize   the whole packfile; _part: 0 data, 1 index,
 *                          2 footer (PutPackfile Encode's index and footer) */
typedef struct cdc_packer cdc_packer;
int cdc_packer_new(uint32_t max_size, cdc_packer **out);
int cdc_packer_add_blob(cdc_packer *p, uint8_t type, const uint8_t checksum[32], const uint8_t *data, uint64_t len);
int64_t cdc_packer_add_chunks(cdc_packer *p, const uint8_t *base, const cdc_cut *cuts, uint64_t n,
                              const uint8_t *digests, const uint8_t *skip);
uint64_t cdc_packer_size(const cdc_packer *p);
uint32_t cdc_packer_count(const cdc_packer *p);
int cdc_packer_serialize(const cdc_packer *p, int64_t timestamp, uint8_t *out, uint64_t cap, uint64_t *len);
int cdc_packer_serialize_part(const cdc_packer *p, int part, int64_t timestamp, uint8_t *out, uint64_t cap,
                              uint64_t *len);
void cdc_packer_reset(cdc_packer *p);
void cdc_packer_free(cdc_packer *p);

/* ---- end-to-end backup: files in, packfiles out ---------------------------------
 * chunkify (snapshot/backup.go:571-687) + PutBlob (snapshot/blobs.go:9-24) +
 * packerJob (snapshot/snapshot.go:51-92) for a list of files, as a pipeline
 * over batches of whole files (at most batch_bytes each, 0: 256 MiB): reader
 * threads read each file into a pinned arena and SHA-256 it there (the
 * object checksum); the device cuts, digests (SHA-256 + byte histogram per
 * chunk) and Encodes the new chunks (LZ4 or GZIP as compress says, then AES-256-GCM
 * when key != NULL; a chunk whose digest is in `known` (sorted, 32 B each:
 * BlobExists) or was already seen in this run is not stored again); packer
 * threads append the blobs to their own packfiles and hand each one, at
 * Size() > packfile_max (0: 20 MiB) and at the end, to on_pack (PutPackfile;
 * calls are serialised, from packer threads).  on_file is called once per
 * file (per piece, below) in the order the pipeline processes them: every
 * file's first piece, largest file first (a large file's object hash is a
 * long serial chain), then the later pieces of large files round by round,
 * so pieces of different files interleave; from one library thread (the
 * calling thread meanwhile
 * drives the next batches through the device), with pointers valid during the
 * call only; chunk entropies come from the device (cdc_chunk_entropy_device_async).
 * An empty file is one empty chunk (backup.go:631-635); a file shorter than
 * MinSize is one chunk.  A file larger than the batch size is processed in
 * pieces of about batch_bytes, in order, each chunked from the previous
 * piece's carried chunk start (the cut points are those of the whole file),
 * so the pinned and device buffers stay bounded by batch_bytes + Max per slot
 * whatever the file sizes; on_file is then called once per piece (piece /
 * pieces; cut offsets are file-relative; checksum and object_entropy are set
 * in the last piece's call).  A file that cannot be read (missing, not a
 * regular file, shorter than when it was listed) is reported through on_file
 * with status CDC_E_IO and no chunks, and the backup goes on with the others
 * (backupCtx.recordError, snapshot/backup.go:264-267); stats.failed_files
 * counts them.  A file in pieces that fails in a later piece (it shrank
 * mid-run) has had its earlier pieces reported with status CDC_OK and their
 * chunks (and blobs packed); that piece and every later one then come with
 * status CDC_E_IO and no chunks, and the last piece's call carries no
 * checksum: the caller drops the partial object (snapshot.BackupSession does).  Returns CDC_OK, or the first failure of the run itself (a
 * device error, a negative status from on_pack). */
typedef struct cdc_backup_opts {
    cdc_opts chunking;
    uint32_t packfile_max;
    int compress;             /* CDC_COMPRESS_NONE, _LZ4 or _GZIP, as cdc_encode_device's `compress` */
    const uint8_t *key;       /* 32-byte repository key, or NULL: no encryption */
    int packers;              /* packer threads (0: 8, NumCPU in the reference) */
    int readers;              /* reader threads (0: 8) */
    uint64_t batch_bytes;
    const uint8_t *known;     /* sorted digests already in the repository, or NULL */
    uint64_t nknown;
    int64_t timestamp;        /* packfile footer timestamp */
} cdc_backup_opts;
typedef struct cdc_backup_file {
    int index;                /* position in paths */
    int status;
    uint8_t checksum[32];     /* SHA-256 of the whole file (Object.Checksum) */
    uint64_t size;
    uint64_t nchunks;
    const cdc_cut *cuts;      /* (offset, length) in the file */
    const uint8_t *digests;   /* 32 B per chunk (Chunk.Checksum) */
    const uint32_t *hists;    /* 256 per chunk (entropy / Distribution) */
    const uint8_t *is_new;    /* 1: stored by this run (PutBlob), 0: deduplicated */
    const double *entropy;    /* per chunk (Chunk.Entropy: entropy() with Go's math.Log2) */
    double object_entropy;    /* Object.Entropy: sum of entropy * length in chunk order / size */
    uint32_t piece, pieces;   /* this call's piece of the file (pieces == 1: the whole file) */
    /* This piece's bytes as read (file offsets [data_offset, data_offset +
     * data_len)), valid during the callback; NULL when the file failed.  The
     * piece's chunks cover [data_offset, data_offset + the sum of their
     * lengths); a piece before the last carries its tail into the next.  For
     * the Object fields the caller computes from the bytes: ContentType
     * (mime.TypeByExtension, else mimetype.Detect of the first chunk,
     * snapshot/backup.go:580, 598-601) and the classifier feed
     * (cprocessor.Write per chunk, backup.go:577, 605). */
    const uint8_t *data;
    uint64_t data_offset, data_len;
} cdc_backup_file;
typedef struct cdc_backup_stats {
    uint64_t files, bytes, chunks, new_blobs, new_bytes, encoded_bytes, packfiles, packed_bytes, batches;
    double read_s;            /* file reads, summed over reader threads */
    double objhash_s;         /* object SHA-256, summed over reader threads */
    double h2d_s, chunk_s, digest_s, d2h_s, encode_s;  /* device stages (events; Encode: host wall) */
    double device_s;          /* the calling thread's time in the device stages (callbacks excluded) */
    double callback_s;        /* in on_file (the callback thread) */
    double read_wait_s;       /* the calling thread waiting for a batch's reads (device idle) */
    double pack_s;            /* packer threads' busy time, summed */
    double wall_s;
    uint64_t failed_files;    /* files reported with status CDC_E_IO */
    uint64_t pieces;          /* units through the pipeline (files + extra pieces of large files) */
    uint64_t slot_arena_bytes;  /* pinned arena bytes per slot this run needed (<= batch_bytes + Max) */
    /* GPU_MAX_HW_QUEUES in the process environment at cdc_backup_new (0: unset,
     * HIP's default of 4).  The pipeline's eight streams (scans, H2D, two
     * digest streams, two encoder streams and one side stream per Encode
     * workspace) run independently only with >= 8 hardware queues; with fewer,
     * HIP maps several streams onto one queue and the stages serialise
     * (INTEGRATION.md).  Other streams of the process (torch's, the collector's)
     * share queues with them even at 8. */
    int32_t hw_queues;
    int32_t streams_serialised;  /* 1 when hw_queues < 8 (or unset) */
    /* What sets the wall (round 6): fill_s, the call's start until batch 0's
     * reads have landed (the device's first work); drain_s, the last batch's
     * device stages done until the call returns (Encode, packers, callbacks
     * of the tail); chain_s / chain_bytes, the longest serial object SHA-256
     * chain of one file (a file's pieces hash one after another). */
    double fill_s, drain_s, chain_s;
    uint64_t chain_bytes;
} cdc_backup_stats;
typedef void (*cdc_backup_file_fn)(void *ctx, const cdc_backup_file *f);
typedef int (*cdc_backup_pack_fn)(void *ctx, const uint8_t *packfile, uint64_t len);
/* A backup context: its options (key and known digests copied), streams and
 * pinned / device buffers kept across calls (grown on demand).  Each
 * cdc_backup_files call is one backup of the given files: its dedup set
 * starts empty (plus `known`).  One call at a time per context. */
typedef struct cdc_backup cdc_backup;
int cdc_backup_new(int device, const cdc_backup_opts *opts, cdc_backup **out);
int cdc_backup_files(cdc_backup *b, const char *const *paths, int n, cdc_backup_file_fn on_file,
                     cdc_backup_pack_fn on_pack, void *ctx, cdc_backup_stats *stats);
void cdc_backup_free(cdc_backup *b);
/* The level Encode runs at in later cdc_backup_files calls of this session
 * (compression/compression.go:12-51; CDC_LEVEL_* above): CDC_LEVEL_WIDE stores
 * smaller LZ4 or GZIP blobs.  A run in progress keeps the level it began with.
 * cdc_backup_run has no session: cdc_backup_run_level takes the level. */
int cdc_backup_set_level(cdc_backup *b, int level);
/* The form of the packfiles on_pack receives in later cdc_backup_files calls:
 * CDC_PACKFILE_PLAIN (0, the default) or CDC_PACKFILE_STORED (1), the bytes
 * repository.PutPackfile stores (the stored form, below): a packer seals its
 * packfile as before, then its index and footer go through one Encode call at
 * CDC_LEVEL_FAST with the session's compress and key, under the lock that
 * serialises on_pack.  That Encode uses the workspace of the pipeline's first
 * encoder thread and waits for a batch's Encode there.  Any
 * other form is CDC_E_INVALID.  A run in progress keeps its form. */
int cdc_backup_set_packfile_form(cdc_backup *b, int form);
/* new + files + free in one call. */
int cdc_backup_run(int device, const char *const *paths, int n, const cdc_backup_opts *opts,
                   cdc_backup_file_fn on_file, cdc_backup_pack_fn on_pack, void *ctx, cdc_backup_stats *stats);
/* cdc_backup_run with Encode at `level` (compression/compression.go:12-51;
 * CDC_LEVEL_* above); a level that does not exist is CDC_E_INVALID before
 * anything is opened.  cdc_backup_run is this call with CDC_LEVEL_FAST. */
int cdc_backup_run_level(int device, const char *const *paths, int n, const cdc_backup_opts *opts,
                         cdc_backup_file_fn on_file, cdc_backup_pack_fn on_pack, void *ctx, cdc_backup_stats *stats,
                         int level);

/* ---- restore: packfiles in, files out --------------------------------------------
 * The read path of snapshot/restore.go:103-110 (a reader per file handed to
 * the exporter), snapshot/vfs/vfilep.go:58-122 (Read walks the chunk lengths,
 * one GetBlob per chunk) and repository/repository.go:407-429, 449-466
 * (GetSubpartForBlob, one ranged packfile read and one Decode per chunk), as
 * a pipeline over batches that decodes every distinct blob of a batch once. */
#define CDC_E_NOTFOUND (-15) /* a chunk's checksum is in no registered packfile (repository.ErrPackfileNotFound) */

/* packfile.NewFromBytes (packfile/packfile.go:152-239) for the plain
 * Serialize form (packfile.go:241-294; the form cdc_packer_serialize and
 * cdc_backup_files' on_pack produce): the footer, and the index rows into
 * rows[0, cap) (rows may be NULL when cap is 0).  With cap < count it returns
 * CDC_E_NOSPACE, *needed (may be NULL) = count, and the footer and the first
 * cap rows are set.  CDC_E_CORRUPT: fewer than 52 bytes, a version other than
 * 100, an index that is not 41 * count bytes, an entry whose offset + length
 * passes the index offset, or an index whose SHA-256 (cdc_sha256) is not the
 * footer's.  Host only; needs no cdc_init.  The PutPackfile form, whose index
 * and footer went through Encode (snapshot/snapshot.go:249-267), is
 * CDC_E_CORRUPT here: cdc_packfile_index_stored reads it. */
typedef struct cdc_packfile_footer {
    uint32_t version;       /* 100 */
    uint32_t count;
    int64_t timestamp;
    uint32_t index_offset;  /* = the length of the blob data */
    uint32_t reserved;
    uint8_t index_checksum[32];
} cdc_packfile_footer;
typedef struct cdc_packfile_row {
    uint8_t checksum[32];
    uint32_t offset, length;  /* of the encoded blob in the packfile */
    uint8_t type;             /* 1: TYPE_CHUNK */
    uint8_t reserved[3];
} cdc_packfile_row;
int cdc_packfile_index(const uint8_t *bytes, uint64_t len, cdc_packfile_footer *footer, cdc_packfile_row *rows,
                       uint64_t cap, uint64_t *needed);

/* ---- the stored form: what a repository keeps -------------------------------------
 * snapshot.PutPackfile (snapshot/snapshot.go:232-267) stores, and the fs
 * backend writes unchanged (storage/backends/fs/fs.go:270-292),
 *     data || Encode(index) || Encode(footer) || u32le version || u8 len(Encode(footer))
 * with Encode the repository's compression, then its AES-256-GCM stream
 * (repository/repository.go:212-262), as for every blob.  Read back
 * (cmd/plakar/subcommands/info/info.go:387-426) for a file of len bytes:
 * L = bytes[len - 1], version = u32le(bytes[len - 5 .. len - 1)), the encoded
 * footer is bytes[len - 5 - L .. len - 5) and decodes to the 52-byte footer,
 * the encoded index is bytes[footer.index_offset .. len - 5 - L) and decodes to
 * 41 * footer.count bytes whose SHA-256 is footer.index_checksum.  The blobs
 * sit at the offsets the rows give, as in the plain form.
 * A source of a cdc_*_add_packfiles call names its form: */
#define CDC_PACKFILE_PLAIN  0   /* (*PackFile).Serialize: cdc_packer_serialize's form, the default everywhere */
#define CDC_PACKFILE_STORED 1   /* snapshot.PutPackfile: what a repository keeps */
#define CDC_PACKFILE_ROWS   2   /* the caller supplies the index (the repository state's rows,
                                 * state.GetSubpartForBlob): nothing of the file's tail is read or decoded */
typedef struct cdc_packfile_src {
    const uint8_t *bytes;         /* memory form (lifetime as cdc_restore_add_packfile), or NULL */
    uint64_t len;
    const char *path;             /* path form, when bytes == NULL */
    int form;                     /* CDC_PACKFILE_* */
    const cdc_packfile_row *rows; /* CDC_PACKFILE_ROWS only; copied */
    uint64_t nrows;
} cdc_packfile_src;

/* cdc_packfile_index for one stored packfile in host memory: the two tails go
 * through cdc_decode_device on `device` (compress, key: as there), the rows
 * are checked and hashed on the host.  footer, rows, cap, *needed and
 * CDC_E_NOSPACE as cdc_packfile_index.  CDC_E_CORRUPT: fewer than 5 bytes, a
 * last byte of 0 in a repository with a key or a compression, a last byte
 * that passes the file, a trailer or footer version other than 100, a footer
 * that does not decode to 52 bytes, an index offset past the encoded footer, a
 * count the encoded index cannot inflate to (checked before anything is sized
 * from it), an index that does not decode to 41 * count bytes, a row past the
 * index offset, an index checksum mismatch, and any Decode failure but
 * CDC_E_AUTH, which is a GCM tag of the footer or the index.  A plain-form
 * packfile is CDC_E_CORRUPT or CDC_E_AUTH. */
int cdc_packfile_index_stored(int device, const uint8_t *bytes, uint64_t len, int compress, const uint8_t *key,
                              cdc_packfile_footer *footer, cdc_packfile_row *rows, uint64_t cap, uint64_t *needed);

/* The packer's packfile in the stored form: its data section, then its index
 * and its footer through one cdc_encode_device_level at CDC_LEVEL_FAST
 * (compress, key: as there; random: 112 bytes, the index's 56 then the
 * footer's 56, or NULL: drawn with getrandom(2)), then the trailer.
 * CDC_E_NOSPACE with *len set when cap is too small; cdc_packer_stored_bound
 * is enough.  CDC_E_UNSUPPORTED when the encoded footer takes 256 bytes or
 * more (its length field is one byte; no configuration here reaches 200). */
uint64_t cdc_packer_stored_bound(const cdc_packer *p, int compress, int encrypt);
int cdc_packer_serialize_stored(const cdc_packer *p, int64_t timestamp, int device, int compress, const uint8_t *key,
                                const uint8_t *random, uint8_t *out, uint64_t cap, uint64_t *len);

/* The copy loop of vfilep.go:58-122 (`copy(p, data[...])` per chunk) for a
 * batch, on the device: for each of n segments (host arrays), d_dst[dst_off[i],
 * + len[i]) = d_src[src_off[i], + len[i]).  Any byte alignment on either
 * side; sources may repeat and overlap each other (a deduplicated chunk);
 * destinations are sorted by dst_off and disjoint, and [d_src, + src_cap) and
 * [d_dst, + dst_cap) do not overlap.  Exactly the bytes asked for are written.
 * Checked on the host before anything is launched (CDC_E_INVALID): NULL
 * arrays, src_off + len > src_cap, dst_off + len > dst_cap, destinations
 * unsorted or overlapping.  The segment arrays are copied before the call
 * returns.  Asynchronous on `stream`. */
int cdc_assemble_device(int device, const void *d_src, uint64_t src_cap, const uint64_t *src_off,
                        const uint64_t *len, const uint64_t *dst_off, uint64_t n, void *d_dst, uint64_t dst_cap,
                        void *stream);
/* Cache policy of the assemble kernel: bit 0 nontemporal loads, bit 1
 * nontemporal stores (default 2).  The bytes written never
 * depend on it.  Diagnostic, not a reference interface.  CDC_OK or CDC_E_INVALID. */
int cdc_debug_set_assemble_policy(int policy);

/* A restore context: Decode's configuration (compress, key: as
 * cdc_decode_device; the key is copied), the registered packfiles with their
 * locator (checksum -> packfile, offset, length: state.GetSubpartForBlob,
 * repository.go:449-466), three streams and its pinned / device buffers kept
 * across runs (grown on demand).  One cdc_restore_files at a time per context. */
typedef struct cdc_restore_opts {
    int compress;          /* CDC_COMPRESS_NONE, _LZ4 or _GZIP, as cdc_decode_device's `compressed` */
    const uint8_t *key;    /* 32-byte repository key, or NULL: not encrypted */
    int verify;            /* 0: off; otherwise every decoded blob's SHA-256 is compared with its checksum */
    int writers;          /* reader and writer threads (0: 8) */
    uint64_t batch_bytes;  /* output bytes per batch (0: 256 MiB) */
} cdc_restore_opts;
/* verify = 1, everything else 0. */
void cdc_restore_default_opts(cdc_restore_opts *out);
typedef struct cdc_restore_file {
    const char *path;          /* destination, or NULL: on_file receives the bytes */
    uint64_t nchunks;
    const uint8_t *checksums;  /* 32 B per chunk (Chunk.Checksum) */
    const uint32_t *lengths;   /* Chunk.Length */
} cdc_restore_file;
typedef struct cdc_restore_result {
    int index;                 /* position in files */
    int status;                /* CDC_OK, CDC_E_NOTFOUND, CDC_E_IO, CDC_E_MISMATCH or the blob's Decode error */
    uint64_t size;             /* the file's size (sum of its chunk lengths) */
    uint32_t piece, pieces;    /* path == NULL: this call's piece of the file (pieces == 1: all of it) */
    const uint8_t *data;       /* path == NULL and status == CDC_OK: file bytes [data_offset, + data_len) */
    uint64_t data_offset, data_len;
} cdc_restore_result;
typedef struct cdc_restore_stats {
    uint64_t files, failed_files, bytes, segments;  /* bytes: output bytes of the batches */
    uint64_t distinct_blobs;   /* distinct checksums among the chunks of the files that were found */
    uint64_t decoded_blobs, encoded_bytes, decoded_bytes;  /* through Decode: each batch's distinct blobs, summed */
    uint64_t batches, batches_identity;  /* identity: decoded straight into the output image, no assemble launch */
    uint64_t pieces;
    double read_s, h2d_s, decode_s, verify_s, assemble_s, d2h_s, write_s;  /* wall time of each stage, summed */
    double wall_s;
} cdc_restore_stats;
typedef void (*cdc_restore_file_fn)(void *ctx, const cdc_restore_result *r);
typedef struct cdc_restore cdc_restore;
int cdc_restore_new(int device, const cdc_restore_opts *opts, cdc_restore **out);
/* Parse the index (cdc_packfile_index) and enter every TYPE_CHUNK row into the
 * locator; a checksum already there keeps its first location.  The memory
 * form reads the blobs from `bytes` during later runs: the buffer must stay
 * valid and unchanged until cdc_restore_free (from cgo: C or pinned memory,
 * never a Go pointer).  The path form reads the footer and the index now and
 * pread(2)s blob ranges during a run (the fs backend's GetPackfileBlob).
 * CDC_E_CORRUPT, CDC_E_IO (the path form), CDC_E_NOMEM. */
int cdc_restore_add_packfile(cdc_restore *r, const uint8_t *bytes, uint64_t len);
int cdc_restore_add_packfile_path(cdc_restore *r, const char *path);
/* n packfiles in one call, each in the form it names (cdc_packfile_src above;
 * one call may mix forms).  The stored ones cost two cdc_decode_device calls
 * together, one over their encoded footers and one over their encoded indexes,
 * whatever their number (a repository holds one packfile per 20 MiB); the
 * context's own compress and key decode them (for cdc_sync: the source's).
 * Plain sources go through cdc_restore_add_packfile[_path].  A
 * CDC_PACKFILE_ROWS source enters the caller's rows for a file whose length is
 * `len` or fstat(2)'s; nothing else of the file is read now.
 * Returns CDC_OK whenever the call ran; status[i] (n) is CDC_OK, CDC_E_IO,
 * CDC_E_AUTH (a GCM tag of the footer or the index) or CDC_E_CORRUPT (as
 * cdc_packfile_index_stored; a row of a rows source past the file's length).
 * Only sources with CDC_OK are entered, in source order: a checksum already
 * there keeps its first location.  CDC_E_INVALID before the device is
 * touched: NULL arguments, an unknown form, CDC_PACKFILE_ROWS without rows,
 * neither bytes nor path, a call during a run of the context.  One each for
 * restore (and cdc_restore_ranges), check, diff, archive and sync. */
int cdc_restore_add_packfiles(cdc_restore *r, const cdc_packfile_src *srcs, uint32_t n, int32_t *status);
/* Restore n files from their chunk lists (what cdc_backup_files' on_file
 * delivered: Object.Chunks).  Per batch of at most batch_bytes of output (a
 * larger file goes in pieces cut on chunk boundaries): reader threads gather
 * the batch's distinct encoded blobs into a pinned arena, one host-to-device
 * copy, one Decode over the distinct blobs (with verify: plus SHA-256 and
 * compare, as cdc_check_device), cdc_assemble_device into the batch's output
 * image (skipped when the plaintext buffer already is that image), one
 * device-to-host copy, then writer threads pwrite(2) each file's bytes.
 * Batch k + 1's reads and upload overlap batch k's device stages and batch
 * k - 1's download and writes.
 * Failures are per file and the run goes on (FileErrorEvent, restore.go:
 * 103-116): CDC_E_NOTFOUND for a checksum in no packfile; a blob that fails
 * Decode, whose decoded length is not the recorded Length (CDC_E_MISMATCH) or
 * whose SHA-256 differs (CDC_E_MISMATCH) fails every file that uses it; a
 * destination that cannot be created or written is CDC_E_IO.  A failed file
 * is not written, and what earlier pieces of it wrote is removed.  A file
 * with a path is created with O_CREAT|O_TRUNC (an empty file empty) and
 * on_file is called once for it, after its last byte was written or with
 * its failure.  With path == NULL on_file is called once per piece with that
 * piece's bytes (valid during the call only); a file's last call carries its
 * final status, and a caller that was handed earlier pieces of a file that
 * then fails drops them.  on_file (may be NULL) is called from one library
 * thread at a time.  Returns CDC_OK, or the run's own first failure (a device
 * error); *stats may be NULL. */
int cdc_restore_files(cdc_restore *r, const cdc_restore_file *files, int n, cdc_restore_file_fn on_file, void *ctx,
                      cdc_restore_stats *stats);
void cdc_restore_free(cdc_restore *r);

/* Byte ranges of files: the reader behind `plakar cat`, `plakar mount`,
 * `plakar exec` and the HTTP API's file download (VFilep.Read and Seek,
 * snapshot/vfs/vfilep.go:58-122, 168-197), which fetches and decodes a whole
 * chunk again for every Read.  Here a batch of ranges decodes each blob it
 * touches once, and only as far as its last byte asked for
 * (cdc_decode_prefix_device), so a 4-KiB page costs about 4 KiB of decode
 * chain, not its chunk and not its file.
 * A range is (files[file], offset, length) and means the file's bytes
 * [offset, min(offset + length, size)).  offset == size or length == 0 is an
 * empty range that succeeds; offset > size is CDC_E_INVALID for that range
 * alone (Seek's rule), and so is a file index out of bounds.  Overlapping
 * ranges, the same range twice and ranges in any file order are legal. */
typedef struct cdc_read_range {
    uint32_t file;      /* index into files */
    uint32_t reserved;  /* 0 */
    uint64_t offset, length;
} cdc_read_range;
typedef struct cdc_read_result {
    int index;                 /* position in ranges */
    int status;                /* CDC_OK, CDC_E_INVALID, CDC_E_NOTFOUND, CDC_E_IO, CDC_E_MISMATCH or a blob's Decode error */
    uint32_t piece, pieces;    /* this call's piece of the range (pieces == 1: all of it) */
    const uint8_t *data;       /* status == CDC_OK: range bytes [data_offset, + data_len), valid during the call only */
    uint64_t data_offset, data_len;
    uint64_t length;           /* the bytes the whole range delivers: min(length, size - offset) */
} cdc_read_result;
/* A new struct with its size in front (set struct_size = sizeof before the
 * call; the library fills that many bytes): cdc_restore_stats has no such
 * field and cannot grow. */
typedef struct cdc_read_stats {
    uint32_t struct_size, reserved;
    uint64_t ranges, failed_ranges;
    uint64_t bytes;            /* output bytes: the ranges' lengths, summed */
    uint64_t segments;         /* (range, chunk) overlaps */
    uint64_t batches;
    uint64_t distinct_blobs;   /* distinct blobs touched by the run */
    uint64_t whole_blobs;      /* per batch, the blobs decoded to their recorded length ... */
    uint64_t prefix_blobs;     /* ... and those decoded only so far */
    uint64_t verified_blobs;   /* whole blobs whose SHA-256 was compared (verify) */
    uint64_t encoded_bytes;    /* gathered and uploaded */
    uint64_t decoded_bytes;    /* the sum of upto: what the decode chains produced */
    uint64_t skipped_bytes;    /* the sum of recorded length - upto: what they did not have to */
    double read_s, h2d_s, decode_s, verify_s, assemble_s, d2h_s;  /* wall time of each stage, summed */
    double wall_s;
} cdc_read_stats;
typedef void (*cdc_read_range_fn)(void *ctx, const cdc_read_result *r);
/* Runs on a restore context: its packfiles, locator, key, compression,
 * streams and buffers (files[i].path is ignored; one run of either kind at a
 * time per context).  The ranges are laid into batches in the caller's order
 * (batch_bytes bounds both a batch's output and the bytes it decodes; a larger
 * range goes in pieces cut on chunk boundaries).  Per batch: reader threads
 * gather the distinct encoded blobs (whole, except that without compression
 * only the header and the records that hold the prefix are read), one
 * host-to-device copy, one cdc_decode_prefix_device with upto = the largest
 * end offset any range of the batch has inside the blob, with verify SHA-256
 * and compare for exactly the blobs decoded to their recorded length (a
 * prefix cannot be hashed: its integrity is what GCM gives), one
 * cdc_assemble_device into the output image, one device-to-host copy, then
 * on_range once per range piece, in the caller's order, from one library
 * thread at a time.
 * Failures are per range and the run goes on: a checksum in no packfile
 * (CDC_E_NOTFOUND), a blob that cannot be read (CDC_E_IO), fails Decode, ends
 * before the bytes asked for or differs from its checksum (CDC_E_MISMATCH)
 * fails every range that touches that blob and no other range, not even of
 * the same file.  A range's last call carries its final status; a caller that
 * was handed earlier pieces of a range that then fails drops them.
 * CDC_E_INVALID before the device is touched: NULL r, nfiles < 0 or nranges <
 * 0, NULL arrays, a file without its chunk arrays, stats->struct_size < 8.
 * Returns CDC_OK, or the run's own first failure (a device error). */
int cdc_restore_ranges(cdc_restore *r, const cdc_restore_file *files, int nfiles, const cdc_read_range *ranges,
                       int nranges, cdc_read_range_fn on_range, void *ctx, cdc_read_stats *stats);

/* ---- check: a snapshot's chunks and object checksums -------------------------------
 * `plakar check` (snapshot/check.go:56-113) and `plakar checksum`
 * (cmd/plakar/subcommands/checksum/checksum.go:108-119) for the objects the
 * caller supplies (it walks the snapshot, as for restore).
 *
 * digests[i] = SHA-256 of the concatenation of object i's segments
 * seg[obj_seg0[i] .. obj_seg0[i+1]) of d_data.  Host arrays; d_digests device,
 * 32 B per object, 16-byte aligned.  A segment is any (offset, length) in the
 * buffer: any alignment, any length including 0; segments may repeat and
 * overlap.  An object without segments, or with empty ones only, hashes to
 * SHA-256("").  The bytes are hashed where they lie: only the 64-byte blocks
 * that a segment boundary cuts are copied (cdc_assemble_device, into a seam
 * area the library keeps).  Synchronous on `stream`.
 * CDC_E_INVALID: a segment outside [0, len), a list that does not ascend to
 * nsegs, an object of 2^61 bytes or more, a NULL argument (d_data may be NULL
 * when len is 0) or a d_digests that is not 16-byte aligned; CDC_E_NOT_INIT
 * before cdc_init; CDC_OK when n == 0.  Nothing is launched and d_digests is
 * untouched unless CDC_OK or CDC_E_DEVICE comes back. */
int cdc_object_digests_device(int device, const void *d_data, uint64_t len,
                              const uint64_t *seg_off, const uint64_t *seg_len, uint64_t nsegs,
                              const uint64_t *obj_seg0, uint32_t n, uint8_t *d_digests, void *stream);

/* A check context, shaped like a restore context: Decode's configuration, the
 * registered packfiles and their locator, streams and buffers kept across
 * runs.  One cdc_check_files at a time per context. */
typedef struct cdc_check_opts {
    uint32_t struct_size;   /* sizeof(cdc_check_opts) */
    int compress;           /* CDC_COMPRESS_NONE, _LZ4 or _GZIP */
    const uint8_t *key;     /* 32-byte repository key, or NULL */
    int fast;               /* check -fast: presence only, no device work */
    int threads;            /* reader and host-hash threads (0: 8) */
    uint64_t batch_bytes;   /* of file bytes per batch (0: 256 MiB; at most 1 GiB) */
    uint64_t host_min_len;  /* 0: the model; else objects at least this long hash on the host */
} cdc_check_opts;
/* struct_size set, everything else 0. */
void cdc_check_default_opts(cdc_check_opts *out);
typedef struct cdc_check_file {
    uint64_t nchunks;
    const uint8_t *checksums;        /* 32 B per chunk (Chunk.Checksum) */
    const uint32_t *lengths;         /* Chunk.Length */
    const uint8_t *object_checksum;  /* 32 B, or NULL: compute only (plakar checksum) */
} cdc_check_file;
typedef struct cdc_check_result {
    int index;              /* position in files */
    int status;
    int64_t bad_chunk;      /* the chunk `status` names, or -1 (none, or the object itself) */
    int hashed;             /* 0 not hashed, 1 on the device, 2 on the host */
    uint8_t checksum[32];   /* the computed object SHA-256 when hashed != 0 */
    uint64_t size;          /* the sum of the chunk lengths */
} cdc_check_result;
typedef struct cdc_check_stats {
    uint32_t struct_size;   /* set by the caller; at most that many bytes are written */
    uint32_t reserved;
    uint64_t files, failed_files, bytes, segments;  /* bytes: file bytes of the batches */
    uint64_t distinct_blobs, decoded_blobs, encoded_bytes, decoded_bytes, batches, pieces;  /* as cdc_restore_stats */
    uint64_t device_objects, device_bytes;  /* objects hashed by k_object_digest where their blobs lie */
    uint64_t host_objects, host_bytes;      /* objects gathered, copied back and hashed on host threads */
    uint64_t seam_bytes;                    /* copied for the device's objects (blocks a chunk boundary cuts) */
    /* wall time of each stage, summed.  digest_s: the device's objects (runs planned, seam copies,
     * k_object_digest, the digests back); d2h_s: the host's bytes gathered and copied back; hash_s: hashed */
    double read_s, h2d_s, decode_s, verify_s, digest_s, d2h_s, hash_s;
    double wall_s;
} cdc_check_stats;
typedef void (*cdc_check_file_fn)(void *ctx, const cdc_check_result *r);
typedef struct cdc_check cdc_check;
/* CDC_E_INVALID: NULL, a struct_size that is not this header's, a device
 * outside 0..63, an unknown compress, threads outside 0..256, batch_bytes
 * over 1 GiB; CDC_E_NOT_INIT before cdc_init (fast contexts too). */
int cdc_check_new(int device, const cdc_check_opts *opts, cdc_check **out);
int cdc_check_add_packfile(cdc_check *c, const uint8_t *bytes, uint64_t len);  /* as cdc_restore_add_packfile */
int cdc_check_add_packfile_path(cdc_check *c, const char *path);
int cdc_check_add_packfiles(cdc_check *c, const cdc_packfile_src *srcs, uint32_t n, int32_t *status);  /* as cdc_restore_add_packfiles */
/* Check n files from their chunk lists and object checksums.  Per batch of at
 * most batch_bytes of file bytes (restore's plan): reader threads gather the
 * batch's distinct encoded blobs, one upload, one Decode with SHA-256 and
 * compare over the distinct blobs (restore's, with its slow path for a blob
 * that decodes to more than its Length).  Then the objects are hashed: those
 * the device takes by k_object_digest over the places of their chunks in the
 * plaintext buffer (no image is assembled; 32 bytes per object come back),
 * those the host takes are gathered by cdc_assemble_device into a staging
 * image, copied back once and hashed on `threads` threads.  The split is
 * cdc_chunk_digests_hybrid's model over the objects' lengths, or host_min_len.
 * A file that spans batches is always hashed on the host, piece by piece as
 * the pieces come back: the device keeps no midstate between batches.  Batch
 * k + 1 is read and uploaded while batch k is on the device and batch k - 1's
 * host-bound objects are hashed.
 * on_file (may be NULL) is called once per file, from one library thread at a
 * time, with (check.go:66-111):
 *   CDC_OK          every chunk is found, decodes to its recorded Length with
 *                   its SHA-256, and the object's SHA-256 equals
 *                   object_checksum when one is given;
 *   CDC_E_NOTFOUND  a chunk in no registered packfile: bad_chunk its index,
 *                   hashed = 0, the file is not decoded (as restore does not).
 *                   When a file has a missing chunk and an earlier damaged one
 *                   the reference names the earlier one, this the missing one;
 *   a blob's status a blob that cannot be read (CDC_E_IO), fails Decode, has
 *                   the wrong Length or SHA-256 (CDC_E_MISMATCH): bad_chunk is
 *                   the lowest index in the file with a failed blob, hashed =
 *                   0; every file that uses the blob fails, and no other;
 *   CDC_E_MISMATCH  with bad_chunk = -1 and hashed != 0: all chunks fine, the
 *                   object's SHA-256 (in `checksum`) is not object_checksum.
 * With opts.fast only the locator is asked (check.go:68-75): CDC_E_NOTFOUND
 * with the first missing index, or CDC_OK; hashed = 0, nothing is read,
 * uploaded or launched and stats.decoded_blobs is 0.  The reference compares
 * the empty hasher's sum with the recorded checksum in that mode too
 * (check.go:107), which fails every file with bytes; that is not reproduced.
 * Returns CDC_OK, or the run's own first failure; CDC_E_INVALID (NULL context
 * or files, a file with chunks and no arrays) before the device is touched. */
int cdc_check_files(cdc_check *c, const cdc_check_file *files, int n, cdc_check_file_fn on_file, void *ctx,
                    cdc_check_stats *stats);
void cdc_check_free(cdc_check *c);

/* ---- diff: unified diffs of snapshot files ------------------------------------------
 * `plakar diff` for two files (cmd/plakar/subcommands/diff/diff.go:152-196):
 * both files read whole, split with difflib.SplitLines, go-difflib's
 * UnifiedDiff with Context 3, and "identical" without a read when the two
 * Object.Checksums are equal.  go-difflib is a port of Python's difflib; the
 * text here is difflib.unified_diff's (DESIGN.md 5.21 on what is pinned).
 *
 * Lines (SplitLines): a text with k newline bytes has k + 1 lines; line j is
 * the bytes after the j-th newline up to and excluding the next one, or up to
 * the end of the text; every line is compared and printed as if it ended in
 * "\n".  An empty text is one empty line.  Every other byte is ordinary. */
typedef struct cdc_line_rec {
    uint64_t off;       /* of the line's first byte in the buffer */
    uint32_t len;       /* without the newline */
    uint32_t reserved;  /* 0 */
    uint64_t hash[2];   /* of (len, bytes): equal for equal lines; the values are not part of the interface */
} cdc_line_rec;

/* The line table of n texts (text_off[i], text_len[i]: host arrays) of one
 * device buffer: any alignment, texts may overlap, a text is shorter than
 * 4 GiB.  counts[i] (host, may be NULL) = the lines of text i; d_recs (device,
 * 16-byte aligned, room for cap records) receives the records of text 0, then
 * text 1, ...; a line never passes the end of its text.  *total (may be NULL)
 * = the lines of all texts.  When cap is smaller, CDC_E_NOSPACE with *total
 * and counts set and nothing written to d_recs.  Three passes: a newline count
 * per 16-KiB tile, a scan of the tile counts, and the records with their
 * hashes (a line of cdc_debug_set_line_threshold bytes or more is hashed by a
 * whole wave).  Synchronous on `stream`.
 * CDC_E_INVALID before any HIP call: device outside 0..63, NULL arrays with
 * n > 0, a text outside [0, len) or of 4 GiB or more, d_data NULL with len > 0,
 * d_recs NULL or misaligned with cap > 0, more than 2^32 - 2 lines possible
 * (the sum of the text lengths plus n); CDC_E_NOT_INIT before cdc_init; CDC_OK
 * and nothing launched for n == 0. */
int cdc_line_table_device(int device, const void *d_data, uint64_t len, const uint64_t *text_off,
                          const uint64_t *text_len, uint32_t n, cdc_line_rec *d_recs, uint64_t cap, uint64_t *counts,
                          uint64_t *total, void *stream);

/* Exact line ids.  recs: a host copy of nlines records over d_data; group[g]
 * .. group[g + 1] (ngroups + 1 ascending entries from 0 to nlines) are the
 * lines of one pair, A's then B's.  ids[i] = the smallest j in i's group, not
 * after i, whose line has the same bytes, counted from the group's start.
 * The first hash_bits bits of the hashes propose (0: all 128); k_line_verify
 * compares each line's bytes with its candidate's, and flagged lines move on
 * until none is flagged: *rounds (may be NULL) = the comparison launches.
 * The hash maps are built on up to 8 host threads, a group per task.
 * Synchronous on `stream`.  CDC_E_INVALID: NULL arguments, hash_bits outside
 * 0..128, a group list that does not ascend from 0 to nlines, a record outside
 * [0, len), nlines of 2^32 - 1 or more. */
int cdc_line_ids_device(int device, const void *d_data, uint64_t len, const cdc_line_rec *recs, uint64_t nlines,
                        const uint64_t *group, uint32_t ngroups, int hash_bits, uint32_t *ids, uint32_t *rounds,
                        void *stream);
/* Lines of at least this many bytes take the wave-cooperative hash and compare
 * kernels (0: the default, 4096).  The hashes and ids never depend on it.
 * Diagnostic.  CDC_OK. */
int cdc_debug_set_line_threshold(uint32_t bytes);

/* difflib.SequenceMatcher(None, a, b).get_grouped_opcodes(context) over line
 * ids (autojunk on: with 200 ids or more in b, those that occur more than
 * len(b) / 100 + 1 times do not start matches).  ops[0, cap) receives the
 * opcodes of all groups, `group` counting the groups from 0; *nops their
 * number.  CDC_E_NOSPACE with *nops set when cap is smaller.  Host only; needs
 * no cdc_init.  CDC_E_INVALID: NULL arrays with a nonzero count, context < 0,
 * 2^32 - 1 ids or more.  The worst case is quadratic, as the reference's. */
#define CDC_DIFF_EQUAL 0
#define CDC_DIFF_REPLACE 1
#define CDC_DIFF_DELETE 2
#define CDC_DIFF_INSERT 3
typedef struct cdc_diff_op {
    uint32_t tag, group;
    uint32_t i1, i2, j1, j2;  /* a[i1:i2] and b[j1:j2] */
} cdc_diff_op;
int cdc_diff_script(const uint32_t *a_ids, uint64_t na, const uint32_t *b_ids, uint64_t nb, int context,
                    cdc_diff_op *ops, uint64_t cap, uint64_t *nops);

/* An emit record: at dst_off the prefix byte (CDC_EMIT_PREFIX: flags & 0xff),
 * then len bytes from src_off of the plaintext or (CDC_EMIT_LITERAL) the
 * literal area, then "\n" (CDC_EMIT_NEWLINE). */
#define CDC_EMIT_PREFIX 0x100u
#define CDC_EMIT_LITERAL 0x200u
#define CDC_EMIT_NEWLINE 0x400u
typedef struct cdc_emit_rec {
    uint64_t src_off, dst_off;
    uint32_t len, flags;
} cdc_emit_rec;
/* The unified diff of one pair as an emit plan: "--- from\n+++ to\n" before
 * the first hunk, per group "@@ -r1 +r2 @@\n" (difflib's range format) and the
 * lines with ' ', '-', '+', all '-' of a replace before its '+'; no group, no
 * output.  The header and @@ lines are literals, written to lit[0, lit_cap)
 * and addressed from lit_base; destinations ascend from dst_base.  *nrecs,
 * *lit_bytes, *out_bytes (each may be NULL) are always set; CDC_E_NOSPACE when
 * rec_cap or lit_cap is smaller (then nothing is written).  Host only. */
int cdc_diff_emit_plan(const cdc_diff_op *ops, uint64_t nops, const cdc_line_rec *a_lines, uint64_t na,
                       const cdc_line_rec *b_lines, uint64_t nb, const char *from_name, const char *to_name,
                       uint64_t dst_base, uint64_t lit_base, cdc_emit_rec *recs, uint64_t rec_cap, uint8_t *lit,
                       uint64_t lit_cap, uint64_t *nrecs, uint64_t *lit_bytes, uint64_t *out_bytes);
/* Execute an emit plan: n records (host array; copied before the call
 * returns) over the plaintext [d_plain, + plain_cap) and the literal area
 * [d_lit, + lit_cap), into [d_dst, + dst_cap).  Records are short and many:
 * a wave takes up to 64 of them with its lanes over their output bytes; a
 * record of 2 KiB or more goes in 16-KiB pieces of 16-byte stores.  Exactly
 * the bytes of the records are written.  Asynchronous on `stream`.
 * CDC_E_INVALID before any HIP call: NULL arguments, a source range outside
 * its area, a destination outside [0, dst_cap), destinations that do not
 * ascend or that overlap, unknown flag bits, more than 2^32 - 1 records, or a
 * destination that overlaps a source area.  CDC_OK and nothing launched for
 * n == 0. */
int cdc_diff_emit_device(int device, const void *d_plain, uint64_t plain_cap, const void *d_lit, uint64_t lit_cap,
                         const cdc_emit_rec *recs, uint64_t n, void *d_dst, uint64_t dst_cap, void *stream);

/* A diff context, shaped like a check context. */
typedef struct cdc_diff_opts {
    uint32_t struct_size;   /* sizeof(cdc_diff_opts) */
    int compress;           /* CDC_COMPRESS_NONE, _LZ4 or _GZIP */
    const uint8_t *key;     /* 32-byte repository key, or NULL */
    int context;            /* lines of context (0: 3) */
    int threads;            /* reader and matcher threads (0: 8) */
    uint64_t batch_bytes;   /* of file bytes per batch (0: 256 MiB; at most 1 GiB) */
    uint64_t max_lines;     /* per batch (0: 16 Mi) */
    int hash_bits;          /* diagnostic: only so many bits of the line hashes propose (0: all 128) */
} cdc_diff_opts;
/* struct_size set, everything else 0. */
void cdc_diff_default_opts(cdc_diff_opts *out);
typedef struct cdc_diff_pair {
    cdc_check_file a, b;    /* the two versions; object_checksum may be NULL */
    const char *from_name, *to_name;
} cdc_diff_pair;
typedef struct cdc_diff_result {
    int index;              /* position in pairs */
    int status;             /* CDC_OK, CDC_E_NOTFOUND, CDC_E_NOSPACE, CDC_E_IO, CDC_E_MISMATCH or a blob's Decode error */
    int bad_side;           /* 0: a, 1: b, -1: none */
    int identical;          /* no hunk: equal checksums or chunk lists, or equal lines */
    int64_t bad_chunk;      /* the chunk `status` names on bad_side, or -1 */
    uint64_t a_lines, b_lines;  /* 0 for a pair that was not read */
    uint64_t hunks;
    const uint8_t *text;    /* the unified diff, valid during the call */
    uint64_t text_len;
} cdc_diff_result;
typedef struct cdc_diff_stats {
    uint32_t struct_size;   /* set by the caller; at most that many bytes are written */
    uint32_t reserved;
    uint64_t pairs, failed_pairs, identical_pairs, skipped_pairs;  /* skipped: identical without device work */
    uint64_t bytes, segments;  /* file bytes and chunk occurrences of the batches */
    uint64_t distinct_blobs, decoded_blobs, encoded_bytes, decoded_bytes, batches;  /* as cdc_check_stats */
    uint64_t lines, distinct_lines, verify_rounds, hunks, out_bytes;
    double read_s, h2d_s, decode_s, verify_s, assemble_s, table_s, ids_s, match_s, emit_s, d2h_s;
    double wall_s;
} cdc_diff_stats;
typedef void (*cdc_diff_pair_fn)(void *ctx, const cdc_diff_result *r);
typedef struct cdc_diff cdc_diff;
/* CDC_E_INVALID: NULL, a struct_size that is not this header's, a device
 * outside 0..63, an unknown compress, context < 0, threads outside 0..256,
 * batch_bytes over 1 GiB, max_lines over 2^31, hash_bits outside 0..128;
 * CDC_E_NOT_INIT before cdc_init. */
int cdc_diff_new(int device, const cdc_diff_opts *opts, cdc_diff **out);
int cdc_diff_add_packfile(cdc_diff *d, const uint8_t *bytes, uint64_t len);  /* as cdc_restore_add_packfile */
int cdc_diff_add_packfile_path(cdc_diff *d, const char *path);
int cdc_diff_add_packfiles(cdc_diff *d, const cdc_packfile_src *srcs, uint32_t n, int32_t *status);  /* as cdc_restore_add_packfiles */
/* The unified diffs of n pairs.  A pair whose two object checksums are given
 * and equal, or whose chunk lists are equal, is identical with no device work
 * (diff.go:156).  The others go in batches of whole pairs of at most
 * batch_bytes of file bytes: reader threads gather the distinct encoded blobs
 * of both sides, one upload, one Decode with SHA-256 and compare over the
 * distinct blobs (restore's plan, Check's calls), both images laid out by
 * cdc_assemble_device, the line table, exact ids, the matcher on `threads`
 * host threads (one pair per task), the emit plan, cdc_diff_emit_device and
 * one copy back of the batch's diff text.  The stages of a batch run in
 * sequence.  on_pair (may be NULL) is called once per pair from the calling
 * thread.  Failures are per pair and the run goes on: CDC_E_NOTFOUND with
 * bad_side and bad_chunk for a chunk in no packfile; a blob that cannot be
 * read, fails Decode or has the wrong Length or SHA-256 fails every pair that
 * uses it (bad_side, bad_chunk: the first such chunk, a's before b's), and no
 * other; a pair whose two sizes exceed batch_bytes or whose lines exceed
 * max_lines fails alone with CDC_E_NOSPACE.  Returns CDC_OK, or the run's own
 * first failure; CDC_E_INVALID (NULL context or pairs, a file with chunks and
 * no arrays, stats->struct_size < 8) before the device is touched. */
int cdc_diff_files(cdc_diff *d, const cdc_diff_pair *pairs, int n, cdc_diff_pair_fn on_pair, void *ctx,
                   cdc_diff_stats *stats);
void cdc_diff_free(cdc_diff *d);

/* ---- grep: fixed strings in snapshot files -------------------------------------------
 * `grep -F -e p0 -e p1 ... [-i] [-n] [-b] [-c] [-l] [-m]` over texts that lie in
 * device memory.  The reference has no such command: its Snapshot.Search
 * matches names, sizes and content types, never a file's bytes.
 *
 * Patterns: 1 to 32 fixed strings of 1 to 256 bytes; a pattern with the byte
 * 0x0A is CDC_E_INVALID, every other byte (0x00 too) is ordinary; duplicates
 * are allowed, each with its own bit and count.  CDC_GREP_IGNORE_CASE folds
 * ASCII only: 'A'..'Z' equal 'a'..'z' and nothing else folds.
 * Lines (grep's count): a text with k newline bytes has k lines when it ends in
 * a newline or is empty, else k + 1; a line is the bytes between newlines (a
 * '\r' before the newline belongs to it); numbers start at 1.
 * Pattern k of m bytes occurs at column i of a line of len bytes when
 * i + m <= len and the m bytes there equal the pattern after folding: an
 * occurrence lies inside one line of one text, and no byte of a neighbouring
 * text, of a gap between texts or outside them ever completes one.  A line
 * with an occurrence yields one record: */
#define CDC_GREP_IGNORE_CASE 1u
typedef struct cdc_grep_hit {
    uint32_t text;   /* index of the text (device entry point) or of the file in `files` (session) */
    uint32_t line;   /* 1-based */
    uint64_t off;    /* of the line's first byte: in the buffer (device entry point), in the file (session) */
    uint32_t len;    /* without the newline */
    uint32_t col;    /* the smallest column of any occurrence */
    uint32_t mask;   /* bit k set: pattern k occurs in the line */
    uint32_t nocc;   /* occurrences of all patterns, overlapping ones included; saturates at 2^32 - 1 */
} cdc_grep_hit;

/* Search n texts (text_off[i], text_len[i]: host arrays) of one device buffer.
 * The texts ascend and do not overlap, at any alignment; a text is shorter
 * than 4 GiB.  d_hits (device, 16-byte aligned, room for cap records) receives
 * the records in text order, then line order, whatever the scheduling (every
 * accumulator is an integer OR, add or min, and the compaction is stable by
 * rank).  limit > 0: only the first `limit` matching lines of each text are
 * written.  lines[i], matched[i], binary[i] (host, n each, may be NULL): the
 * lines of text i, all its matching lines (limit or not), and 1 when it holds
 * a 0x00 byte (grep's heuristic, for -I).  *total (may be NULL) = the records,
 * the sum of min(matched, limit).  When cap is smaller: CDC_E_NOSPACE with
 * lines, matched, binary and *total set and nothing written to d_hits.
 * The line table is cdc_line_table_device's without the hashes; k_grep_scan
 * then reads every byte of the texts once (and 255 bytes past each 16-KiB tile
 * once more) and nothing else of the buffer: the work follows the texts, not
 * len.  The worst case is bounded: a text of one byte value against 32
 * patterns of 256 such bytes compares 8 KiB per position.
 * Synchronous on `stream` (work ordered after the stream, which is drained at
 * return; no other stream is waited for).
 * CDC_E_INVALID before any HIP call: device outside 0..63, NULL arrays with a
 * nonzero count, a text outside [0, len) or of 4 GiB or more, texts that do
 * not ascend or that overlap, more than 2^32 - 2 lines possible, no pattern or
 * more than 32, a pattern length outside 1..256, a newline in a pattern,
 * unknown flag bits, d_hits NULL or misaligned with cap > 0; CDC_E_NOT_INIT
 * before cdc_init; CDC_OK and nothing launched for n == 0. */
int cdc_grep_device(int device, const void *d_data, uint64_t len, const uint64_t *text_off, const uint64_t *text_len,
                    uint32_t n, const uint8_t *const *patterns, const uint32_t *pattern_len, uint32_t npatterns,
                    uint32_t flags, uint64_t limit, cdc_grep_hit *d_hits, uint64_t cap, uint64_t *lines,
                    uint64_t *matched, uint8_t *binary, uint64_t *total, void *stream);

/* A grep context, shaped like a check context. */
typedef struct cdc_grep_opts {
    uint32_t struct_size;   /* sizeof(cdc_grep_opts) */
    int compress;           /* CDC_COMPRESS_NONE, _LZ4 or _GZIP */
    const uint8_t *key;     /* 32-byte repository key, or NULL */
    int threads;            /* reader threads (0: 8) */
    uint64_t batch_bytes;   /* of file bytes per batch (0: 256 MiB; at most 1 GiB) */
    uint64_t max_lines;     /* per batch (0: 16 Mi) */
} cdc_grep_opts;
/* struct_size set, everything else 0. */
void cdc_grep_default_opts(cdc_grep_opts *out);
typedef struct cdc_grep_query {
    uint32_t struct_size;   /* sizeof(cdc_grep_query) */
    uint32_t flags;         /* CDC_GREP_IGNORE_CASE */
    const uint8_t *const *patterns;
    const uint32_t *pattern_len;
    uint32_t npatterns;
    uint64_t limit;         /* matching lines reported per file (0: 65,536) */
    int want_text;          /* also return the matching lines' bytes */
    uint32_t max_line_bytes;  /* of each line in the text (0: 4,096) */
} cdc_grep_query;
typedef struct cdc_grep_result {
    int index;              /* position in files */
    int status;             /* CDC_OK, CDC_E_NOTFOUND, CDC_E_NOSPACE, CDC_E_IO, CDC_E_MISMATCH or a blob's Decode error */
    int64_t bad_chunk;      /* the chunk `status` names, or -1 */
    int binary;             /* the file holds a 0x00 byte */
    uint64_t size, lines, matched;  /* matched: all matching lines, limit or not; 0 for a file that failed */
    const cdc_grep_hit *hits;       /* the first min(matched, limit), valid during the call */
    uint64_t nhits;
    const uint8_t *text;    /* want_text: per hit the line's first max_line_bytes bytes and "\n"; valid during the call */
    uint64_t text_len;
} cdc_grep_result;
typedef struct cdc_grep_stats {
    uint32_t struct_size;   /* set by the caller; at most that many bytes are written */
    uint32_t reserved;
    uint64_t files, failed_files, bytes, segments;  /* as cdc_check_stats */
    uint64_t distinct_blobs, decoded_blobs, encoded_bytes, decoded_bytes, batches;
    uint64_t lines, matched_lines, hits, occurrences, out_bytes;  /* occurrences: of the reported hits */
    double read_s, h2d_s, decode_s, verify_s, assemble_s, table_s, scan_s, compact_s, emit_s, d2h_s;
    double wall_s;
} cdc_grep_stats;
typedef void (*cdc_grep_file_fn)(void *ctx, const cdc_grep_result *r);
typedef struct cdc_grep cdc_grep;
/* CDC_E_INVALID: NULL, a struct_size that is not this header's, a device
 * outside 0..63, an unknown compress, threads outside 0..256, batch_bytes over
 * 1 GiB, max_lines over 2^31; CDC_E_NOT_INIT before cdc_init. */
int cdc_grep_new(int device, const cdc_grep_opts *opts, cdc_grep **out);
int cdc_grep_add_packfile(cdc_grep *g, const uint8_t *bytes, uint64_t len);  /* as cdc_restore_add_packfile */
int cdc_grep_add_packfile_path(cdc_grep *g, const char *path);
int cdc_grep_add_packfiles(cdc_grep *g, const cdc_packfile_src *srcs, uint32_t n, int32_t *status);  /* as cdc_restore_add_packfiles */
/* Search n files from their chunk lists (object_checksum is not used).  The
 * files go in batches of whole files of at most batch_bytes: reader threads
 * gather the batch's distinct encoded blobs, one upload, one Decode with
 * SHA-256 and compare over the distinct blobs (a blob many files share decodes
 * once), the images laid out by cdc_assemble_device, then cdc_grep_device's
 * stages over the images (groups of files of at most max_lines lines) and one
 * copy back of the hit records, whose `text` is the file's index and `off` the
 * line's offset in the file.  With want_text the lines are gathered by
 * cdc_diff_emit_device and copied back once.  The stages of a batch run in
 * sequence.  on_file (may be NULL) is called once per file from the calling
 * thread, in file order.  Failures are per file and the run goes on:
 * CDC_E_NOTFOUND with bad_chunk for a chunk in no packfile; a blob that cannot
 * be read, fails Decode or has the wrong Length or SHA-256 fails every file
 * that uses it (bad_chunk: the first such chunk) and no other; a file larger
 * than batch_bytes or whose lines exceed max_lines fails alone with
 * CDC_E_NOSPACE.  A file of 0 bytes has 0 lines and no hit and takes no device
 * work.  Returns CDC_OK, or the run's own first failure; CDC_E_INVALID (NULL
 * context, files or query, a query cdc_grep_device would refuse, a file with
 * chunks and no arrays, stats->struct_size < 8) before the device is touched. */
int cdc_grep_files(cdc_grep *g, const cdc_grep_query *q, const cdc_check_file *files, int n, cdc_grep_file_fn on_file,
                   void *ctx, cdc_grep_stats *stats);
void cdc_grep_free(cdc_grep *g);

/* ---- sync: packfiles of one repository in, packfiles of another out ----------------
 * The loop of synchronize (cmd/plakar/subcommands/sync/sync.go:182-266): for
 * every blob the destination lacks, GetBlob from the source, PutBlob
 * (snapshot/blobs.go:9-24) into the destination, whose packerJob
 * (snapshot/snapshot.go:51-92) writes packfiles.  Here it is a pipeline over
 * batches of stored blobs whose device work is cdc_transcode_device_level.
 *
 * Which rows a run takes: every index row of the registered packfiles, in
 * registration and index order, of every blob type.  A row is skipped when its
 * (type, checksum) is in `known` or was already taken in this run, and, when
 * `wanted` is given, unless it is in `wanted`.  One checksum under two types is
 * two blobs.  known and wanted are 33-byte records, the type byte then the
 * checksum, sorted ascending by memcmp (equal neighbours are accepted).
 * A batch is rows up to batch_bytes of stored bytes; a larger blob goes alone;
 * a stored length of 0 is a legal row and is carried (an empty chunk of a
 * repository with no key and no compression is stored that way). */
#define CDC_SYNC_PATH_COPY 0      /* the path cdc_transcode_device takes between the two codecs */
#define CDC_SYNC_PATH_REKEY 1
#define CDC_SYNC_PATH_OPEN 2
#define CDC_SYNC_PATH_SEAL 3
#define CDC_SYNC_PATH_REENCODE 4
typedef struct cdc_sync_opts {
    uint32_t struct_size;      /* sizeof(cdc_sync_opts) */
    cdc_codec src, dst;        /* the two repositories; the keys are copied */
    int verify;                /* not 0: the index checksums are checked first (cdc_transcode_device's `checksums`) */
    int level;                 /* CDC_LEVEL_*; the re-encode path only */
    uint32_t packfile_max;     /* 0: 20 MiB */
    uint64_t batch_bytes;      /* stored bytes per batch (0: 64 MiB) */
    int readers, packers;      /* threads (0: 8 each) */
    int64_t timestamp;         /* packfile footer timestamp */
    const uint8_t *known;      /* the destination's BlobExists: sorted 33-byte records, copied; or NULL */
    uint64_t nknown;
} cdc_sync_opts;
/* struct_size set, verify = 1, everything else 0 (both codecs CDC_COMPRESS_NONE without a key). */
void cdc_sync_default_opts(cdc_sync_opts *out);
typedef struct cdc_sync_stats {
    uint32_t struct_size;      /* set by the caller; at most that many bytes are written */
    int32_t path;              /* CDC_SYNC_PATH_* */
    uint64_t blobs, skipped, failed;  /* rows taken; rows known or already taken; taken rows that failed */
    uint64_t bytes_in, bytes_out;     /* stored bytes of the rows taken; of the blobs written */
    uint64_t batches, packfiles, packed_bytes;
    /* wall time of each stage, summed over the batches: read (the gather),
     * h2d, transcode (the check included), d2h, pack (the packers' step and the
     * last flush, callbacks excluded), callback (inside on_pack and on_fail) */
    double read_s, h2d_s, transcode_s, d2h_s, pack_s, callback_s;
    double device_wait_s;      /* the calling thread waiting for a batch's reads and upload (device idle) */
    double wall_s;
} cdc_sync_stats;
/* A blob of the run that failed: CDC_E_IO (it could not be read), or its
 * status from cdc_transcode_device (CDC_E_AUTH, CDC_E_CORRUPT, CDC_E_UNSUPPORTED,
 * CDC_E_MISMATCH). */
typedef void (*cdc_sync_blob_fn)(void *ctx, uint8_t type, const uint8_t checksum[32], int status);
/* A sync context: the two codecs, `known`, the registered packfiles, three
 * streams, two input and two output slots and its packers, kept across runs.
 * CDC_E_INVALID before the device is touched: NULL, a struct_size that is not
 * this header's, a device outside 0..63, an unknown compress or level, readers
 * or packers outside 0..256, known NULL with nknown > 0 or unsorted;
 * CDC_E_NOT_INIT before cdc_init. */
typedef struct cdc_sync cdc_sync;
int cdc_sync_new(int device, const cdc_sync_opts *opts, cdc_sync **out);
int cdc_sync_add_packfile(cdc_sync *s, const uint8_t *bytes, uint64_t len);  /* as cdc_restore_add_packfile */
int cdc_sync_add_packfile_path(cdc_sync *s, const char *path);
int cdc_sync_add_packfiles(cdc_sync *s, const cdc_packfile_src *srcs, uint32_t n, int32_t *status);  /* as cdc_restore_add_packfiles */
/* One sync of the registered packfiles.  Three stages, batch k + 1 read and
 * uploaded while batch k is on the device and batch k - 1 is downloaded and
 * packed:
 *   reader   gathers the batch's stored blobs into a pinned arena (memcpy, or
 *            pread for a packfile registered by path, on `readers` threads)
 *            and uploads it; a blob that cannot be read fails alone, CDC_E_IO;
 *   device   (the calling thread) one cdc_transcode_device_level call over the
 *            batch's blobs, with their index checksums when verify is set and
 *            fresh OS random bytes (getrandom) when dst has a key; the output
 *            buffer grows and the call is repeated on CDC_E_NOSPACE;
 *   packers  one download into pinned memory, then `packers` threads append the
 *            surviving blobs with their type and checksum (cdc_packer_add_blob),
 *            each to its own packfile; a batch's blobs are split among them in
 *            contiguous ranges, so every packfile holds its rows in source
 *            order.  A packer hands its packfile to on_pack (PutPackfile) when
 *            cdc_packer_add_blob returns 1, and the rest at the end of the run,
 *            packer by packer.  With packers = 1 the packfiles are those of the
 *            loop above run blob by blob; without dst.key their bytes depend
 *            on nothing else.
 * on_pack calls are serialised; the bytes are valid during the call.  A
 * negative status from on_pack stops the run: that status is returned and
 * on_pack is not called again.  on_fail (may be NULL) is called once per failed
 * blob, from one library thread; a failed blob contributes no bytes and the
 * run goes on.  The reference aborts the snapshot at the first failed GetBlob:
 * a caller must not commit the destination snapshot after a failure.
 * wanted: nwanted sorted 33-byte records, or NULL: every row.  stats may be
 * NULL.  One run at a time per context; a context can run again, and each
 * run's taken-set starts empty.  Returns CDC_OK, or the run's own first
 * failure (a device error, on_pack's status); CDC_E_INVALID before the device
 * is touched: NULL s or on_pack, wanted unsorted, stats->struct_size < 8.
 * Out of scope: the snapshot, state and header records, more than one device. */
int cdc_sync_run(cdc_sync *s, const uint8_t *wanted, uint64_t nwanted, cdc_backup_pack_fn on_pack,
                 cdc_sync_blob_fn on_fail, void *ctx, cdc_sync_stats *stats);
/* The destination's packfile form in later runs (CDC_PACKFILE_PLAIN, the
 * default, or CDC_PACKFILE_STORED; as cdc_backup_set_packfile_form, with the
 * destination's codec).  The source's form comes with each source. */
int cdc_sync_set_packfile_form(cdc_sync *s, int form);
void cdc_sync_free(cdc_sync *s);

/* ---- archive: a snapshot's entries as one tar or tar.gz stream -------------------
 * `plakar archive` (cmd/plakar/subcommands/archive/archive.go) for its tar and
 * tarball formats.  The caller supplies the entries (it walks the snapshot, as
 * it supplies objects to restore): files with their chunk lists, and
 * directories.  The tar stream is entries in caller order: a POSIX ustar
 * header block (magic "ustar\0", version "00", uid/gid 0, no uname/gname,
 * typeflag 0 or 5, mtime in whole seconds; a name over 100 bytes split at a
 * "/" into prefix and name), the file's bytes, zeros to the next 512; 1,024
 * zeros at the end and no blocking-factor padding (archive/tar's Close).  An
 * entry that does not fit the block gets a PAX extended header first with the
 * records archive/tar would choose: path (no valid split, over 255 bytes, or a
 * byte >= 0x80), size (8 GiB or more), mtime (negative or over eleven octal
 * digits).  `mode` is the permission bits, 0..07777 (the reference passes Go's
 * FileMode with its type bits; that is not reproduced).
 * CDC_ARCHIVE_TARGZ puts the stream through one cdc_gzip_stream: one member.
 *   compress, key, verify, writers, batch_bytes: as cdc_restore_opts, the
 *     batch counted in bytes of tar stream (0: 256 MiB; at most 1 GiB).
 * Output goes to `path` (created, truncated) or, with path == NULL, to
 * on_data in stream order (a nonzero return ends the run with CDC_E_IO).
 * Failures: an entry with a checksum in no registered packfile is left out
 * whole, header included; on_entry gets CDC_E_NOTFOUND for it and the run goes
 * on.  A blob that cannot be read or fails Decode, whose decoded length is not
 * its recorded Length or whose SHA-256 differs ends the run with that status;
 * on_entry and stats->failed_entry name the first entry that uses it, nothing
 * more is written and a `path` output is removed.  After a run that succeeds
 * on_entry gets CDC_OK for every entry in the archive.  on_entry may be NULL.
 * stats (may be NULL): the caller sets struct_size; at most that many bytes
 * are written. */
#define CDC_ARCHIVE_TAR   0
#define CDC_ARCHIVE_TARGZ 1
#define CDC_ARCHIVE_FILE  0
#define CDC_ARCHIVE_DIR   1
typedef struct cdc_archive_opts {
    uint32_t struct_size;  /* sizeof(cdc_archive_opts) */
    int compress;          /* the repository's: CDC_COMPRESS_NONE, _LZ4 or _GZIP */
    const uint8_t *key;    /* 32-byte repository key, or NULL */
    int verify;
    int writers;           /* reader threads (0: 8) */
    uint64_t batch_bytes;
    int format;            /* CDC_ARCHIVE_TAR or CDC_ARCHIVE_TARGZ */
} cdc_archive_opts;
/* struct_size set, verify = 1, format = CDC_ARCHIVE_TARGZ (the reference's default), everything else 0. */
void cdc_archive_default_opts(cdc_archive_opts *out);
typedef struct cdc_archive_entry {
    const char *name;
    int type;                  /* CDC_ARCHIVE_FILE or CDC_ARCHIVE_DIR */
    uint32_t mode;
    int64_t mtime;
    uint64_t nchunks;          /* files: Object.Chunks */
    const uint8_t *checksums;  /* 32 B per chunk */
    const uint32_t *lengths;
} cdc_archive_entry;
typedef struct cdc_archive_stats {
    uint32_t struct_size;
    int32_t failed_entry;      /* the entry a failed run names, or -1 */
    uint64_t entries, skipped_entries;   /* in the archive; left out (CDC_E_NOTFOUND) */
    uint64_t stream_bytes, output_bytes; /* tar stream; what was written (tar.gz: compressed) */
    uint64_t segments, decoded_blobs, encoded_bytes, decoded_bytes, batches;
    double read_s, h2d_s, decode_s, verify_s, assemble_s, deflate_s, d2h_s, write_s;  /* each stage, summed */
    double wall_s;
} cdc_archive_stats;
typedef int (*cdc_archive_data_fn)(void *ctx, const uint8_t *data, uint64_t len);
typedef void (*cdc_archive_entry_fn)(void *ctx, int index, int status);
typedef struct cdc_archive cdc_archive;
int cdc_archive_new(int device, const cdc_archive_opts *opts, cdc_archive **out);
int cdc_archive_add_packfile(cdc_archive *a, const uint8_t *bytes, uint64_t len);  /* as cdc_restore_add_packfile */
int cdc_archive_add_packfile_path(cdc_archive *a, const char *path);
int cdc_archive_add_packfiles(cdc_archive *a, const cdc_packfile_src *srcs, uint32_t n, int32_t *status);  /* as cdc_restore_add_packfiles */
int cdc_archive_run(cdc_archive *a, const cdc_archive_entry *entries, int n, const char *path,
                    cdc_archive_data_fn on_data, cdc_archive_entry_fn on_entry, void *ctx, cdc_archive_stats *stats);
void cdc_archive_free(cdc_archive *a);
/* The level of later cdc_archive_run calls (compression/compression.go:12-51;
 * CDC_LEVEL_* above): the gzip member of a tar.gz and the entries of a zip
 * (cdc_archive_new_zip) are deflated with the wide match search; a plain tar
 * is not compressed and does not change. */
int cdc_archive_set_level(cdc_archive *a, int level);
/* `plakar archive -format zip` (archive.go:194-245: zip.FileInfoHeader, Method
 * = zip.Deflate, CreateHeader, io.Copy per file; directories are not written,
 * archive.go:211-213).  A context in zip mode: checked as cdc_archive_new
 * checks, except that opts->format is not read; add_packfile, run and free
 * take it as they are.  The output is archive/zip's on a non-seekable writer:
 * per file a local header (version 20, flags 0x0008 and 0x0800 for a UTF-8
 * name that needs it, method 8, DOS time and date from mtime in UTC clamped to
 * 1980..2107, zero CRC and sizes, the name without leading slashes, the
 * extended-timestamp extra), one raw DEFLATE stream (cdc_zip_pieces_device)
 * and a data descriptor; after the last entry the central directory (creator
 * 0x0314, external attributes (0100000 | mode) << 16, bit 0 for a file without
 * the owner-write bit; zip64 extras where a size or an offset needs them) and
 * the end records.  A directory entry is accepted and reported CDC_OK but not
 * written and not counted in stats->entries.  A name empty after trimming,
 * with a NUL or over 65,535 bytes, or mode bits above 07777: CDC_E_INVALID.
 * batch_bytes counts file bytes plus local headers; stats->stream_bytes is
 * their sum, output_bytes the archive's size.  Failures as cdc_archive_run's. */
int cdc_archive_new_zip(int device, const cdc_archive_opts *opts, cdc_archive **out);

/* The library's host SHA-256 (x86 SHA extensions when the CPU has them;
 * force_scalar != 0 takes the portable path).  cdc_sha256_accelerated: 1 if
 * the SHA extensions are in use. */
int cdc_sha256(const void *data, uint64_t len, int force_scalar, uint8_t out[32]);
int cdc_sha256_accelerated(void);

/* ---- pinned batch arena: files in, host cut lists out --------------------------
 * Replaces the importer's per-file os.Open + bufio reads
 * (snapshot/importer/fs/fs.go:69-71) feeding the per-file Next() loop: a
 * batch of files is read with pread(2) straight into library-owned pinned
 * host memory, then chunked by one cdc_chunk call whose host-to-device copies
 * are pinned DMA.  The bytes stay in the arena (cdc_batch_get) for the
 * per-chunk work (processChunk) until cdc_batch_reset.  A cgo caller passes
 * only file descriptors, paths and C memory: no Go pointer is stored.
 *   cdc_batch_new        arena of `capacity` bytes (buffers are 4-KiB aligned)
 *   cdc_batch_reserve    append a buffer of len bytes; *ptr = where to write it
 *   cdc_batch_add_fd     append len bytes read from fd (pread from offset 0)
 *   cdc_batch_add_files  append n whole files, read by `threads` threads;
 *   cdc_batch_chunk_files  add_files + chunking of those files, overlapped;
 *                        sizes[i] = file sizes (may be NULL).  All or nothing.
 *   cdc_batch_chunk      cdc_chunk over the arena's buffers, in order
 * Errors: CDC_E_NOSPACE (arena full), CDC_E_IO, CDC_E_NOT_INIT. */
typedef struct cdc_batch cdc_batch;
int cdc_batch_new(uint64_t capacity, cdc_batch **out);
int cdc_batch_reserve(cdc_batch *b, uint64_t len, uint8_t **ptr);
int cdc_batch_add_fd(cdc_batch *b, int fd, uint64_t len);
int cdc_batch_add_files(cdc_batch *b, const char *const *paths, int n, int threads, uint64_t *sizes);
/* cdc_batch_add_files + cdc_chunk over the n files it adds (not the arena's
 * earlier buffers), overlapped: reader threads run ahead while each
 * sub-batch of >= 256 MiB of whole files is chunked as soon as it is read.
 * out / out_counts (n entries) / out_needed as cdc_chunk. */
int cdc_batch_chunk_files(cdc_batch *b, const char *const *paths, int n, int threads, const cdc_opts *opts,
                          cdc_cut *out, uint64_t out_cap, uint64_t *out_counts, uint64_t *out_needed,
                          uint64_t *sizes);
int cdc_batch_count(const cdc_batch *b);
int cdc_batch_get(const cdc_batch *b, int i, const uint8_t **ptr, uint64_t *len);
int cdc_batch_chunk(cdc_batch *b, const cdc_opts *opts, cdc_cut *out, uint64_t out_cap,
                    uint64_t *out_counts, uint64_t *out_needed);
void cdc_batch_reset(cdc_batch *b);
void cdc_batch_free(cdc_batch *b);

/* ---- device-resident path -----------------------------------------------------
 * d_data: device pointer to len bytes (any alignment) on `device`.
 * final != 0: the buffer is a whole stream, so the last chunk ends at len.
 * final == 0: more bytes follow.  Only chunks whose cut is decided by the
 * bytes present are written, and result->consumed tells the caller where to
 * resume (the Peek(MaxSize) window of ext chunker.go).
 * d_cuts / d_result: device memory.  d_workspace: device memory of at least
 * cdc_device_workspace_size() bytes, not shared with another in-flight call.
 * Asynchronous on `stream`: enqueues kernels and returns.  Graph-capturable. */
int cdc_device_workspace_size(uint64_t len, const cdc_opts *opts, uint64_t *bytes);
int cdc_chunk_device_async(int device, const void *d_data, uint64_t len, int final,
                           const cdc_opts *opts, cdc_cut *d_cuts, uint64_t cut_cap,
                           cdc_result *d_result, void *d_workspace, uint64_t workspace_bytes,
                           void *stream);

/* Batched device path: nbufs independent device buffers chunked by one set of
 * launches.  d_cuts[i] / cut_caps[i] / d_results[i] are per buffer.  The
 * workspace must be at least cdc_device_batch_workspace_size() bytes. */
int cdc_device_batch_workspace_size(const uint64_t *lens, int nbufs, const cdc_opts *opts,
                                    uint64_t *bytes);
int cdc_chunk_device_batch_async(int device, const void *const *d_data, const uint64_t *lens,
                                 int nbufs, int final, const cdc_opts *opts,
                                 cdc_cut *const *d_cuts, const uint64_t *cut_caps,
                                 cdc_result *const *d_results, void *d_workspace,
                                 uint64_t workspace_bytes, void *stream);

/* ---- per-chunk digests: the per-chunk work of snapshot/backup.go processChunk --
 * For each chunk of a device cut list (offsets relative to d_data), the
 * SHA-256 of the chunk's bytes into d_digests (32 bytes per chunk: the
 * chunkHasher.Sum of snapshot/backup.go:604-606, hashing "SHA256" =
 * crypto/sha256, hashing/hashing.go:31-36) and, when d_hist is not NULL, the
 * chunk's byte histogram into d_hist (256 uint32 per chunk: the freq[] that
 * entropy() counts, snapshot/backup.go:548-557; the float64 entropy and the
 * normalised Distribution are the caller's, since math.Log2 defines them).
 * The chunk count is min(cut_cap, d_result->ncuts) when d_result is not NULL
 * (a cut list still on the device), else cut_cap.  An empty chunk hashes to
 * SHA-256(""), like processChunk([]byte{}) for an empty file (backup.go:631).
 * Asynchronous on `stream`; d_digests / d_hist hold cut_cap entries. */
int cdc_chunk_digests_device_async(int device, const void *d_data, uint64_t len, const cdc_cut *d_cuts,
                                   uint64_t cut_cap, const cdc_result *d_result, uint8_t *d_digests,
                                   uint32_t *d_hist, void *stream);
/* Batched form: every chunk of nbufs buffers hashes in one launch group (the
 * time of a launch is that of its longest chunk, so batch).  d_results and
 * d_hist may be NULL; d_hist entries are all NULL or all set (a buffer with
 * cut_cap 0 may pass NULL either way).  Past 32 buffers the launch group
 * reads its descriptors from device memory (one launch, one tail; the
 * descriptors travel through a ring of 16 slots, and a call waits for the
 * launch that last used the slot it takes).  Asynchronous on `stream`. */
int cdc_chunk_digests_device_batch_async(int device, const void *const *d_data, const uint64_t *lens, int nbufs,
                                         const cdc_cut *const *d_cuts, const uint64_t *cut_caps,
                                         const cdc_result *const *d_results, uint8_t *const *d_digests,
                                         uint32_t *const *d_hist, void *stream);
/* Hybrid form, synchronous: as the batched form, except that the longest
 * chunks' SHA-256 runs on `host_threads` host cores (x86 SHA extensions) while
 * the device hashes the others and computes every histogram.  A device
 * SHA-256 chain costs ~2 us per 64-B block against ~35 ns on a host core, and
 * a device launch lasts as long as its longest chunk, so a single pass over
 * long chunks ends sooner this way.  host_min_len = 0 picks the host's share
 * from the lengths (the longest chunks, as many as balance the host's bytes
 * over its cores and PCIe against the device's longest remaining chain);
 * otherwise every chunk of at least host_min_len bytes goes to the host.
 * host_threads = 0: all on the device.  Synchronous on `stream`: drains it
 * first (the cut lists must be final) and returns once every digest and
 * histogram is in device memory, also when the host's share is empty;
 * *host_chunks / *host_bytes (may be NULL) report the host's share.
 * At most 32 buffers. */
int cdc_chunk_digests_hybrid(int device, const void *const *d_data, const uint64_t *lens, int nbufs,
                             const cdc_cut *const *d_cuts, const uint64_t *cut_caps, const cdc_result *const *d_results,
                             uint8_t *const *d_digests, uint32_t *const *d_hist, int host_threads,
                             uint64_t host_min_len, void *stream, uint64_t *host_chunks, uint64_t *host_bytes);
/* entropy() of snapshot/backup.go:548-569 for `rows` histogram rows (256
 * uint32 each, as cdc_chunk_digests* writes them; a row's sum is its chunk's
 * length) into d_entropy (float64 per row): the reference's terms with Go's
 * math.Log2, one IEEE operation at a time, summed in bin order (bit-exact);
 * 0 for an all-zero row.  Asynchronous on `stream`. */
int cdc_chunk_entropy_device_async(int device, const uint32_t *d_hist, uint64_t rows, double *d_entropy,
                                   void *stream);

/* ---- streaming chunker: chunkers.NewChunker / (*Chunker).Next -----------------
 * Push model, so cgo never hands a Go pointer to asynchronous HIP work: the
 * caller appends stream bytes into a pinned staging window the library owns
 * (cdc_stream_buffer + cdc_stream_commit), then drains chunks with
 * cdc_stream_next.  A chunk pointer aliases that window and stays valid until
 * the next call on the same stream, like the slice ext (*Chunker).Next returns
 * (it aliases the bufio buffer).
 *   cdc_stream_next -> CDC_OK        chunk and len receive the next chunk
 *                   -> CDC_NEED_DATA append bytes (or commit with eof = 1)
 *                   -> CDC_EOF       no more chunks (io.EOF)
 * window_bytes = 0 picks a default (>= 2 * max_size). */
typedef struct cdc_stream cdc_stream;
int cdc_stream_new(const char *algorithm, const cdc_opts *opts, uint64_t window_bytes, int device,
                   cdc_stream **out);
int cdc_stream_buffer(cdc_stream *s, uint8_t **write_ptr, uint64_t *space);
int cdc_stream_commit(cdc_stream *s, uint64_t nbytes, int eof);
int cdc_stream_next(cdc_stream *s, const uint8_t **chunk, uint64_t *len);
void cdc_stream_free(cdc_stream *s);

/* Pull-model convenience over cdc_stream (an io.Reader as a callback):
 * read(ctx, buf, cap) returns the number of bytes read, 0 at EOF, < 0 on error. */
typedef int64_t (*cdc_read_fn)(void *ctx, void *buf, uint64_t cap);
typedef struct cdc_chunker cdc_chunker;
int cdc_chunker_new(const char *algorithm, cdc_read_fn read, void *ctx, const cdc_opts *opts,
                    cdc_chunker **out);
int cdc_chunker_next(cdc_chunker *c, const uint8_t **chunk, uint64_t *len);
void cdc_chunker_free(cdc_chunker *c);

/* ---- State: a repository's blob index, read, merged and queried on the device -----
 * Every command opens the repository with RebuildState (repository/
 * repository.go:58-164): it fetches every state file, Decodes and deserialises
 * each (repository/state/state.go:235-348) and merges them into one aggregate
 * (state.go:384-455) that answers BlobExists (:512), GetSubpartForBlob (:457),
 * ListBlobs and ListSnapshots (:649-719).  A cdc_state is that aggregate, kept
 * in device memory: what cdc_backup_opts.known, CDC_PACKFILE_ROWS and the
 * sessions' locators are filled from.
 *   A state file is Encode (PutState, repository.go:367-378) of what
 * SerializeStream writes (state.go:132-233), all little endian:
 *     u32 version | u64 timestamp ns | u8 aggregate | u64 n, n x 32 B extends
 *     u64 n, n x (id u64, time u64)          DeletedSnapshots
 *     u64 n, n x (id u64, checksum 32 B)     IdToChecksum, ids 0 .. n - 1 in any order
 *     u64 n, n x (id u64, packfile id u64, offset u32, length u32)
 *         for Chunks, Objects, Files, Directories, Children, Datas, Snapshots,
 *         Signatures and Errors, in this order
 * The smallest is 109 bytes; bytes after the last section are ignored and the
 * version is not judged, as in DeserializeStream.
 *   The merge rule is SetPackfileForBlob's (state.go:572-626): a (type,
 * checksum) already present keeps its location.  Go ranges over maps, so the
 * reference's winner among duplicates is arbitrary; here the state given first
 * wins, among the states of one call and across calls, whatever the device's
 * scheduling.  The reference reads a dangling id as the zero
 * checksum; here a state with an IdToChecksum id >= its count or given twice,
 * or a location or deleted-snapshot id with no checksum, is CDC_E_CORRUPT as a
 * whole and nothing of it is entered. */
#define CDC_STATE_PLAIN  0   /* the serialised bytes (SerializeStream) */
#define CDC_STATE_STORED 1   /* what PutState stores: Encode of them */
typedef struct cdc_state_src {
    const uint8_t *bytes;    /* host memory, read during the call only */
    uint64_t len;
    uint8_t id[32];          /* the state's checksum (its name in the repository) */
    int form;                /* CDC_STATE_* */
} cdc_state_src;
typedef struct cdc_state_row {
    uint8_t checksum[32];    /* the blob */
    uint8_t packfile[32];    /* the packfile that holds it */
    uint32_t offset, length; /* of the encoded blob in the packfile */
    uint8_t type;            /* packfile.TYPE_* (packfile/packfile.go:17-25): 0 snapshot, 1 chunk, 2 object, 3 file,
                              * 4 directory, 5 child, 6 data, 7 signature, 8 error */
    uint8_t found;           /* lookups: 1 when the state has the blob, else 0 and the location is zero */
    uint8_t reserved[6];
} cdc_state_row;             /* 80 bytes */
typedef struct cdc_state_stats {
    uint32_t struct_size;    /* set by the caller to sizeof(cdc_state_stats) */
    uint32_t reserved;
    uint64_t states, rejected;   /* sources entered, and sources whose status was not CDC_OK */
    uint64_t rows[9];            /* by type: entries of the aggregate */
    uint64_t deleted_snapshots;  /* distinct checksums in the merged states' DeletedSnapshots */
    uint64_t capacity;           /* slots of the table; it holds at most capacity / 2 records */
    uint64_t records;            /* location and deletion records entered so far, duplicates included */
    uint64_t device_bytes;       /* held between calls: the records and the table */
    double decode_s, index_s, insert_s;  /* summed over the merge calls */
} cdc_state_stats;
typedef struct cdc_state cdc_state;

/* An empty aggregate on `device` for a repository with this compression
 * (CDC_COMPRESS_*) and key (32 bytes, copied; NULL: not encrypted).  Needs no
 * cdc_init.  CDC_E_INVALID for a NULL out or a device outside 0..63. */
int cdc_state_new(int device, int compress, const uint8_t *key, cdc_state **out);
void cdc_state_free(cdc_state *s);

/* RebuildState's loop (repository.go:118-160) for n state files at once: every
 * CDC_STATE_STORED source goes through one cdc_decode_device sizing-plus-decode
 * together with the others, the plaintexts stay on the device, and three
 * kernel stages run over all of them (no launch per state): the IdToChecksum
 * records are scattered into per-state tables, every location becomes a
 * record (type, checksums, offset, length), and the records are inserted.
 * status[i] (host, n): CDC_OK, CDC_E_AUTH, CDC_E_CORRUPT, CDC_E_UNSUPPORTED (a
 * decoded state of 4 GiB or more), or the Decode error.  Only CDC_OK states are
 * entered, in source order, and their ids are appended to the extends list
 * (Extends, repository.go:159).  May be called again: earlier states keep
 * precedence; the table is rebuilt larger when the records pass half its
 * slots.  Every record entered is kept (80 bytes), a duplicate's too: the table
 * holds the winners.  Returns the call's own failure (CDC_E_INVALID: NULL
 * arguments, an unknown form, a length without bytes; CDC_E_NOMEM: the
 * aggregate is as before the call; CDC_E_DEVICE: free it), else CDC_OK.  Calls
 * on one cdc_state are serialised by the library. */
int cdc_state_merge(cdc_state *s, const cdc_state_src *srcs, uint32_t n, int32_t *status);

/* GetSubpartForBlob (state.go:457-510) for n checksums (32 bytes each) of one
 * type: out[i].checksum is the query, found 1 with the packfile's checksum,
 * offset and length, or found 0 with zeros; BlobExists is `found`.  A snapshot
 * named in DeletedSnapshots is still found, as in the reference.  The first
 * form takes and fills host arrays; the second reads digests that already lie
 * on the device (where cdc_chunk_digests_device_async leaves them) and writes
 * device rows (d_out 16-byte aligned), asynchronously on `stream`; a merge on
 * the same cdc_state must not run before that work is done.  CDC_E_INVALID for
 * a NULL argument with n > 0, a misaligned d_out or a type above 8 (the
 * reference panics), before the device is touched. */
int cdc_state_lookup(cdc_state *s, uint8_t type, const uint8_t *checksums, uint64_t n, cdc_state_row *out);
int cdc_state_lookup_device(cdc_state *s, uint8_t type, const uint8_t *d_checksums, uint64_t n, cdc_state_row *d_out,
                            void *stream);

/* ListBlobs (state.go:649-696) with the locations: the aggregate's rows of one
 * type into rows[0, cap), in no particular order.  For type 0 the snapshots
 * named in any merged state's DeletedSnapshots are left out, as ListSnapshots
 * does (state.go:698-719).  With cap too small it returns CDC_E_NOSPACE,
 * *needed (may be NULL) the count, and the first cap rows it found are set, as
 * cdc_packfile_index has it. */
int cdc_state_rows(cdc_state *s, uint8_t type, cdc_state_row *rows, uint64_t cap, uint64_t *needed);

/* Metadata.Extends of the aggregate: the ids of the states entered, in order
 * (32 bytes each).  CDC_E_NOSPACE and *needed as above. */
int cdc_state_extends(cdc_state *s, uint8_t *ids, uint64_t cap, uint64_t *needed);
int cdc_state_info(cdc_state *s, cdc_state_stats *stats);

/* SerializeStream (state.go:132-216) for the delta Snapshot.Commit stores
 * (snapshot/snapshot.go:325-334): the rows entered with SetPackfileForBlob in
 * order (ids: the packfile's first, then the blob's, each checksum once; a row
 * whose (type, checksum) was already seen is dropped), every section written
 * in ascending id, no deleted snapshot.  `found` is ignored.  The result is
 * 109 + 32 * nextends + 40 * ids + 24 * rows kept bytes; CDC_E_NOSPACE with *len
 * set when cap is smaller.  Store it through cdc_encode_device.  Host only;
 * needs no cdc_init.  CDC_E_INVALID: a NULL rows with n > 0, a NULL extends with
 * nextends > 0, a NULL len, a type above 8. */
int cdc_state_serialize(const cdc_state_row *rows, uint64_t n, int64_t timestamp_ns, int aggregate,
                        const uint8_t *extends, uint64_t nextends, uint8_t *out, uint64_t cap, uint64_t *len);

/* ---- Maintenance: rm and cleanup on the aggregate ----------------
 * State.DeleteSnapshot (state.go:628-647) for n snapshots (32 bytes each):
 * status[i] (host, n) is CDC_OK, or CDC_E_NOTFOUND when the aggregate has no
 * snapshot row for the checksum (the reference's "snapshot not found").  Each
 * one found gets a deletion record in the record store, entered into the table
 * like a DeletedSnapshots record read from a state file: cdc_state_rows of type
 * 0 leaves it out from then on and cdc_state_stats.deleted_snapshots counts
 * it.  time_ns is kept with the record; the delta that makes the deletion
 * durable is cdc_state_serialize_deleted's.  CDC_E_INVALID before the device
 * is touched for a NULL argument with n > 0. */
int cdc_state_delete_snapshots(cdc_state *s, const uint8_t *checksums, uint64_t n, int64_t time_ns, int32_t *status);

/* cdc_state_serialize with a DeletedSnapshots section (state.go:176-184):
 * ndeleted checksums (32 bytes each) with their times.  Their ids are given
 * after the rows' ids (a checksum a row already named keeps that id), a
 * checksum given twice keeps its last time, and the section is written in
 * ascending id, 16 bytes per snapshot on top of cdc_state_serialize's size.
 * With ndeleted = 0 the bytes are cdc_state_serialize's.  CDC_E_INVALID also
 * for a NULL deleted or deleted_ns with ndeleted > 0.  Host only. */
int cdc_state_serialize_deleted(const cdc_state_row *rows, uint64_t n, const uint8_t *deleted, const int64_t *deleted_ns,
                                uint64_t ndeleted, int64_t timestamp_ns, int aggregate, const uint8_t *extends,
                                uint64_t nextends, uint8_t *out, uint64_t cap, uint64_t *len);

/* Step 1 of cleanup (cmd/plakar/subcommands/cleanup/cleanup.go:35-45, "find
 * which blobs the remaining snapshots use"): mark the aggregate's rows that
 * the given references name.  refs: n records of 33 bytes, the type byte then
 * the checksum (the format of cdc_sync_opts.known), in any order, duplicates
 * welcome: what Snapshot.ListChunks, ListObjects, ListFiles, ListDirectories
 * and ListDatas yield (snapshot/snapshot.go:348-428) for every snapshot kept.
 * A reference the aggregate has marks its key's winning record (the row
 * cdc_state_lookup answers with) and gets found[i] = 1; one it does not have,
 * under this type, marks nothing and gets found[i] = 0.  found (n bytes) may
 * be NULL; *missing (may be NULL) is the count of zeros.  The device form
 * takes n digests of one type where cdc_chunk_digests_device_async left them
 * and is asynchronous on `stream`, under cdc_state_lookup_device's promise;
 * d_found (n bytes of device memory) may be NULL.  While such work is pending
 * on a caller's stream, none of the calls that write the table or that zero or
 * reallocate the bitmap may run on the same cdc_state (they drain only the
 * aggregate's own stream): cdc_state_merge, cdc_state_delete_snapshots,
 * cdc_state_clear_marks, and the first cdc_state_mark, cdc_state_mark_device
 * or cdc_state_sweep after a merge or a deletion grew the record store (it
 * grows the bitmap); a sweep also reads the marks, so it wants the work done
 * in any case.  Marks accumulate over calls,
 * and over cdc_state_merge and cdc_state_delete_snapshots, until
 * cdc_state_clear_marks.  CDC_E_INVALID before the device is touched: a NULL
 * s, a NULL refs with n > 0, a type above 8 (of any record: then nothing is
 * marked). */
int cdc_state_mark(cdc_state *s, const uint8_t *refs, uint64_t n, uint8_t *found, uint64_t *missing);
int cdc_state_mark_device(cdc_state *s, uint8_t type, const uint8_t *d_checksums, uint64_t n, uint8_t *d_found,
                          void *stream);
int cdc_state_clear_marks(cdc_state *s);

/* Steps 2 to 5 of cleanup's comment (cleanup.go:35-45) as a plan: which rows
 * stay, which packfiles go, which are rewritten.  A record of the store (type
 * 0..8, of a state that was entered) is LIVE when it is its key's winner in
 * the table, and its mark is set or bit `type` of keep_types is, and, for a
 * snapshot, no deletion names its checksum.  Every other record is dead: the
 * unmarked, the deleted, and every loser, that is, the same blob entered again
 * by a later state at another place or at the same one.
 *   Per packfile (the 32 bytes a record names): extent = the largest offset +
 * length (u64) over all its records, dead ones too; live_rows and live_bytes
 * over its live records.  Verdict: DROP when live_rows == 0; REPACK when
 * live_bytes * 1000 < extent * repack_permille; else KEEP.
 *   The plan: the packfiles, ascending in first_record (the lowest record
 * number that names each); kept rows, the live rows of KEEP packfiles in
 * record-number order; repack rows, the live rows of REPACK packfiles grouped
 * by packfile in the list's order and ascending in offset, [row_first,
 * row_first + row_count) being one packfile's.  The same aggregate and marks
 * give the same plan, byte for byte, whatever the device's scheduling.
 *   cdc_state_sweep reads the aggregate and changes nothing in it; it runs on
 * the aggregate's stream and is synchronous.  opts NULL: the defaults.
 * CDC_E_INVALID before the device is touched: NULL s or out, a struct_size
 * that is not this header's, repack_permille above 1000, a keep_types bit
 * above 8.  An aggregate without records gives an empty plan.  The accessors
 * follow cdc_state_rows: CDC_E_NOSPACE with *needed (may be NULL) the count
 * and the first cap entries set. */
#define CDC_SWEEP_KEEP   0
#define CDC_SWEEP_DROP   1
#define CDC_SWEEP_REPACK 2
typedef struct cdc_sweep_opts {
    uint32_t struct_size;     /* sizeof(cdc_sweep_opts) */
    uint32_t keep_types;      /* bit t: rows of type t are live without a mark; default 1 << 0 (snapshots) */
    uint32_t repack_permille; /* 0..1000; default 500 */
    uint32_t reserved;
} cdc_sweep_opts;
typedef struct cdc_sweep_pack {
    uint8_t packfile[32];
    uint64_t extent;          /* max(offset + length) over every record that names it */
    uint64_t live_bytes, live_rows;
    uint64_t first_record;    /* the lowest record number that names it: the order of the list */
    uint64_t row_first, row_count;  /* its slice of the repack rows (REPACK only, else 0, 0) */
    int32_t verdict;          /* CDC_SWEEP_* */
    uint32_t reserved;
} cdc_sweep_pack;             /* 88 bytes */
typedef struct cdc_sweep_stats {
    uint32_t struct_size;     /* set by the caller to sizeof(cdc_sweep_stats) */
    uint32_t reserved;
    uint64_t records;         /* location records seen (type 0..8, of states that were entered) */
    uint64_t live, dead;      /* live + dead == records */
    uint64_t losers;          /* dead because another record holds the key */
    uint64_t packs, keep, drop, repack;  /* packfiles, and how many got each verdict */
    uint64_t kept_rows, repack_rows;
    uint64_t live_bytes;         /* summed over all packfiles */
    uint64_t reclaimable_bytes;  /* sum of extent - live_bytes over DROP and REPACK packfiles */
    double packs_s, sweep_s, verdict_s, compact_s, download_s;  /* the four device stages, and the plan's way to the host */
} cdc_sweep_stats;
typedef struct cdc_sweep cdc_sweep;
void cdc_sweep_default_opts(cdc_sweep_opts *opts);
int cdc_state_sweep(cdc_state *s, const cdc_sweep_opts *opts, cdc_sweep **out);
int cdc_sweep_packs(const cdc_sweep *p, cdc_sweep_pack *packs, uint64_t cap, uint64_t *needed);
int cdc_sweep_kept_rows(const cdc_sweep *p, cdc_state_row *rows, uint64_t cap, uint64_t *needed);
int cdc_sweep_repack_rows(const cdc_sweep *p, cdc_state_row *rows, uint64_t cap, uint64_t *needed);
int cdc_sweep_info(const cdc_sweep *p, cdc_sweep_stats *stats);
void cdc_sweep_free(cdc_sweep *p);

/* ---- diagnostics ---------------------------------------------------------------
 * Kernel selection for tests: 0 = default (scan + index + speculative
 * resolution), 1 = force the sequential single-wave resolver (reference path
 * on the device, for cross-checking the fast path). */
int cdc_set_debug_mode(int mode);

/* When and how the MaskL candidate index is built: 0 = never (walkers
 * raw-scan every MaskL region), 1 = adaptive (default: while recent launch
 * groups on the device needed it, in the same pass as the MaskS index where
 * the masks admit it, else by k_scan_l; every 16th group otherwise runs the
 * selection test alone as a probe), 2 = every launch group in the fused pass,
 * 3 = every launch group by k_scan_l.  Cut points never depend on it; tests
 * use it to cover every path.  Setting a mode clears the adaptive state.
 * Initial value from the CDC_MASKL_INDEX environment variable.  Not a
 * reference interface (the Go chunker has no index).  Returns CDC_OK or
 * CDC_E_INVALID. */
int cdc_set_maskl_index_mode(int mode);

/* Adaptive MaskL state of one device (diagnostics, after a device sync):
 * *hint = 1 while the next launch groups build the MaskL index (a recent
 * group needed it), *groups = launch groups issued on the device so far.  Not a reference interface. */
int cdc_debug_maskl_state(int device, uint32_t *hint, uint64_t *groups);

/* The measured HBM stream-read rate of the device, for the roofline beside
 * the spec peak (SURVEY.md 8(d) "also report a measured stream-read peak"):
 * `reps` launches each of three read-only kernels over [d_buf, d_buf + len)
 * (16-byte aligned), interleaved and timed with hipEvents on `stream`:
 * best_us[f] / median_us[f] (microseconds) for form f = 0 plain 16-byte
 * loads, 1 nontemporal loads, 2 the scan's LDS-DMA staging.  Synchronous.
 * Diagnostic, not a reference interface. */
int cdc_debug_stream_read(int device, const void *d_buf, uint64_t len, int reps, double best_us[3], double median_us[3],
                          void *stream);

/* Per-chunk digests: the lane count the digest kernels assume the device
 * keeps resident (a launch with more chunks than this gives each lane a run
 * of ceil(chunks / lanes) consecutive chunks).  0 (the default) derives it
 * from the device's CU count; tests set small values to cover multi-chunk
 * lanes on small inputs.  Digests never depend on it.  Not a reference
 * interface.  Returns CDC_OK. */
int cdc_debug_set_digest_lanes(uint64_t lanes);

/* The state kernels' grid: at most `blocks` workgroups per launch (0, the
 * default, derives it from the device's CU count), so that a small test sends
 * their grid-stride loops round more than once.  Results never depend on it.
 * Not a reference interface.  Returns CDC_OK. */
int cdc_debug_set_state_blocks(uint32_t blocks);

/* The same for the grep kernels (k_grep_scan and the passes after it). */
int cdc_debug_set_grep_blocks(uint32_t blocks);

/* Live profiling of the device path: when enabled, every launch group records
 * hipEvents on its stream before/after the scan kernel and after the last
 * resolution kernel.  collect() waits for the recorded events, returns the
 * summed scan time, summed pipeline time, number of launch groups and input
 * bytes scanned since the last collect, and resets. */
int cdc_profile_enable(int on);
int cdc_profile_collect(double *scan_ms, double *pipeline_ms, uint64_t *launches,
                        uint64_t *scan_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PLAKAR_CDC_H */
