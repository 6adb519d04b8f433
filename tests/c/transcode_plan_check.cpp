// Stand-alone check of the transcode planner (plakar_amd/csrc/transcode_plan.h),
// built with -fsanitize=address,undefined by tests/test_transcode_cpu.py: the
// lengths around every record edge, the record counts, the output lengths of
// the four key combinations, the offsets of a mixed batch, the refusal of a
// batch whose records cannot be numbered, the spreading of a sub-batch's
// results, and random batches against a record-by-record walk.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "transcode_plan.h"

using namespace tplan;

static int g_fail = 0;
#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            ++g_fail;                                                  \
        }                                                              \
    } while (0)

struct Case {
    uint64_t len;
    int32_t status;    // with an encrypted source
    uint64_t nrec;     // of the source
    uint64_t payload;  // bytes inside the source's envelope
};

// DecryptStream's walk restated: records of min(remaining, 12 + 65,536 + 16) bytes.
static bool walk(uint64_t len, uint64_t &nrec, uint64_t &payload)
{
    nrec = payload = 0;
    if (len < 60) return false;
    uint64_t rem = len - 60;
    while (rem) {
        const uint64_t r = rem < 65564 ? rem : 65564;
        if (r < 28) return false;
        payload += r - 28;
        ++nrec;
        rem -= r;
    }
    return true;
}

int main()
{
    const uint64_t R = 65564;  // a full record: nonce 12, ciphertext 65,536, tag 16
    // The same edges 16 bytes further on (60 + 65,580 and so on, the record
    // length include/plakar_cdc.h's Decode text names): there a second record
    // has begun, so the verdicts differ, and the walk above is what decides.
    const uint64_t Q = 65580;
    const Case cases[] = {
        {0, CDC_E_CORRUPT, 0, 0},
        {59, CDC_E_CORRUPT, 0, 0},
        {60, CDC_OK, 0, 0},
        {61, CDC_E_CORRUPT, 0, 0},
        {60 + 12, CDC_E_CORRUPT, 0, 0},
        {60 + 27, CDC_E_CORRUPT, 0, 0},
        {60 + 28, CDC_OK, 1, 0},
        {60 + R, CDC_OK, 1, 65536},
        {60 + R + 12, CDC_E_CORRUPT, 0, 0},
        {60 + R + 27, CDC_E_CORRUPT, 0, 0},
        {60 + R + 28, CDC_OK, 2, 65536},
        {60 + 3 * R, CDC_OK, 3, 3 * 65536},
        {60 + Q, CDC_E_CORRUPT, 0, 0},                 // a full record and 16 bytes
        {60 + Q + 12, CDC_OK, 2, 65536},               // a full record and an empty Seal
        {60 + Q + 27, CDC_OK, 2, 65536 + 15},
        {60 + Q + 28, CDC_OK, 2, 65536 + 16},
        {60 + 3 * Q, CDC_OK, 4, 3 * 65536 + 20},
    };
    for (const Case &c : cases) {
        // both keys: the length stays; source key only: the payload
        const BlobPlan kk = plan_blob(c.len, true, true), kn = plan_blob(c.len, true, false);
        EXPECT(kk.status == c.status && kn.status == c.status);
        if (c.status == CDC_OK) {
            EXPECT(kk.nrec == c.nrec && kn.nrec == c.nrec);
            EXPECT(kk.payload == c.payload && kn.payload == c.payload);
            EXPECT(kk.out_len == c.len);
            EXPECT(kn.out_len == c.payload);
        } else {
            EXPECT(kk.out_len == 0 && kn.out_len == 0);
        }
        uint64_t wn, wp;
        EXPECT(walk(c.len, wn, wp) == (c.status == CDC_OK));
        if (c.status == CDC_OK) EXPECT(wn == c.nrec && wp == c.payload);
        // destination key only: Encode's pieces of the stored bytes; no key: a copy
        const BlobPlan nk = plan_blob(c.len, false, true), nn = plan_blob(c.len, false, false);
        EXPECT(nk.status == CDC_OK && nn.status == CDC_OK);
        EXPECT(nk.nrec == (c.len + 65535) / 65536 && nk.out_len == 60 + c.len + 28 * nk.nrec && nk.payload == c.len);
        EXPECT(nn.nrec == 0 && nn.out_len == c.len && nn.payload == c.len);
        // sealing what was opened gives the length back when every record but the last is full
        if (c.status == CDC_OK && c.len != 60 + 28 && c.len != 60 + R + 28 && c.len != 60 + Q + 12)
            EXPECT(plan_blob(kn.out_len, false, true).out_len == c.len);
    }

    // the paths
    EXPECT(choose_path(1, true, 1, true) == kPathRekey && choose_path(2, true, 2, true) == kPathRekey);
    EXPECT(choose_path(0, true, 0, true) == kPathRekey);
    EXPECT(choose_path(1, true, 1, false) == kPathOpen && choose_path(1, false, 1, true) == kPathSeal);
    EXPECT(choose_path(2, false, 2, false) == kPathCopy);
    EXPECT(choose_path(1, true, 2, true) == kPathReencode && choose_path(0, false, 1, false) == kPathReencode);
    EXPECT(choose_path(7, true, 1, true) == kPathRekey);  // every other non-zero selector means LZ4
    EXPECT(choose_path(7, true, 2, true) == kPathReencode);

    // a mixed batch: failed blobs have no records and contribute 0 bytes
    {
        const uint64_t lens[] = {60 + 28 + 5, 59, 60 + 3 * R, 60 + 12, 60, 60 + R + 28 + 100};
        BatchPlan B;
        EXPECT(plan_batch(lens, 6, true, true, B) == CDC_OK);
        const uint64_t want_off[] = {0, 93, 93, 93 + 60 + 3 * R, 93 + 60 + 3 * R, 93 + 60 + 3 * R + 60,
                                     93 + 60 + 3 * R + 60 + 60 + R + 128};
        const uint64_t want_rec[] = {0, 1, 1, 4, 4, 4};
        for (int i = 0; i < 6; ++i) EXPECT(B.out_off[i] == want_off[i] && B.rec0[i] == want_rec[i]);
        EXPECT(B.out_off[6] == want_off[6] && B.total == want_off[6] && B.nrecs == 6);
        EXPECT(B.blobs[1].status == CDC_E_CORRUPT && B.blobs[3].status == CDC_E_CORRUPT && B.blobs[1].nrec == 0);
        EXPECT(plan_batch(lens, 6, true, false, B) == CDC_OK);
        EXPECT(B.total == 5 + 3 * 65536 + 0 + 65536 + 100);
        EXPECT(plan_batch(lens, 0, true, true, B) == CDC_OK && B.out_off.size() == 1 && B.total == 0 && B.nrecs == 0);
    }

    // the record count must fit: 2^31 - 1 records pass, one more does not, in one blob or summed
    {
        BatchPlan B;
        const uint64_t most = 60 + kMaxRecords * R;
        uint64_t lens[3] = {most, 60, 60};
        EXPECT(plan_batch(lens, 3, true, true, B) == CDC_OK && B.nrecs == kMaxRecords);
        lens[2] = 60 + 28;
        EXPECT(plan_batch(lens, 3, true, true, B) == CDC_E_INVALID);
        lens[0] = most + R;
        lens[2] = 60;
        EXPECT(plan_batch(lens, 3, true, true, B) == CDC_E_INVALID);
        lens[0] = 60 + (1ull << 32) * R;  // would wrap a 32-bit count to 0
        EXPECT(plan_batch(lens, 3, true, true, B) == CDC_E_INVALID);
        lens[0] = ~0ull;
        EXPECT(plan_batch(lens, 1, true, true, B) == CDC_E_INVALID);
        lens[0] = (kMaxRecords + 1) * 65536;  // the destination's pieces count too
        EXPECT(plan_batch(lens, 1, false, true, B) == CDC_E_INVALID);
        EXPECT(plan_batch(lens, 1, false, false, B) == CDC_OK && B.total == lens[0]);
    }

    // spreading a sub-batch's results over the whole batch
    {
        const uint32_t live[] = {1, 2, 4};
        const uint64_t sub_off[] = {0, 10, 10, 25};  // the second live blob failed in the path
        const int32_t sub_st[] = {CDC_OK, CDC_E_AUTH, CDC_OK};
        uint64_t off[7];
        int32_t st[6] = {CDC_E_MISMATCH, 0, 0, CDC_E_CORRUPT, 0, CDC_E_MISMATCH};
        spread_results(live, 3, sub_off, sub_st, 6, off, st);
        const uint64_t want[] = {0, 0, 10, 10, 10, 25, 25};
        const int32_t want_st[] = {CDC_E_MISMATCH, CDC_OK, CDC_E_AUTH, CDC_E_CORRUPT, CDC_OK, CDC_E_MISMATCH};
        for (int i = 0; i < 7; ++i) EXPECT(off[i] == want[i]);
        for (int i = 0; i < 6; ++i) EXPECT(st[i] == want_st[i]);
        const uint64_t none[] = {0};
        spread_results(nullptr, 0, none, nullptr, 6, off, st);
        for (int i = 0; i < 7; ++i) EXPECT(off[i] == 0);
    }

    // random batches in exactly-sized heap buffers against the walk
    std::mt19937_64 rng(12345);
    uint64_t batches = 0;
    for (int it = 0; it < 3000; ++it) {
        const size_t n = rng() % 40;
        std::vector<uint64_t> lens(n);
        for (auto &l : lens) {
            switch (rng() % 5) {
            case 0: l = rng() % 130; break;
            case 1: l = 60 + (rng() % 4) * R + rng() % 60; break;
            case 2: l = 60 + (rng() % 3) * R + 28 + rng() % 65536; break;
            default: l = rng() % 300000; break;
            }
        }
        const bool se = rng() & 1, de = rng() & 2;
        BatchPlan B;
        EXPECT(plan_batch(lens.data(), n, se, de, B) == CDC_OK);
        uint64_t off = 0, rec = 0;
        for (size_t i = 0; i < n; ++i) {
            EXPECT(B.out_off[i] == off && B.rec0[i] == rec);
            uint64_t wn = 0, wp = lens[i];
            const bool ok = se ? walk(lens[i], wn, wp) : true;
            EXPECT((B.blobs[i].status == CDC_OK) == ok);
            if (!ok) continue;
            if (!se) wn = de ? (lens[i] + 65535) / 65536 : 0;
            const uint64_t want = se ? (de ? lens[i] : wp) : de ? 60 + lens[i] + 28 * wn : lens[i];
            EXPECT(B.blobs[i].out_len == want && B.blobs[i].nrec == wn);
            off += want;
            rec += wn;
        }
        EXPECT(B.total == off && B.nrecs == rec && B.out_off[n] == off);
        ++batches;
    }
    if (g_fail) {
        printf("%d failures\n", g_fail);
        return 1;
    }
    printf("%zu lengths, %llu batches, ok\n", sizeof(cases) / sizeof(cases[0]), (unsigned long long)batches);
    return 0;
}
