// asan_common.h - what the stand-alone sanitizer programs of the rows family share (tools/select_asan_main.cpp, judge_asan_main.cpp, adapter_asan_main.cpp,
// merge_asan_main.cpp, dedup_asan_main.cpp, profile_asan_main.cpp, screen_asan_main.cpp, kmers_asan_main.cpp, demux_asan_main.cpp, group_asan_main.cpp): the generator, a device buffer that ends with its data, the failure line, the rows of a call.  Each program is
// one translation unit.
#pragma once
#include "../include/rfq_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

// (one state per program, seeded the same and stepped in the order of its own draws: a program's rows are the same from run to run)
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

// a device buffer holding `data` `shift` bytes into its allocation, which ends with the data
struct Dev { rfq_ctx* c; void* raw = nullptr; uint8_t* p = nullptr;
    Dev(rfq_ctx* ctx, const void* data, size_t n, size_t shift = 0) : c(ctx) {
        if (rfq_dev_malloc(c, &raw, n + shift)) { fprintf(stderr, "rfq_dev_malloc failed\n"); exit(1); }
        p = (uint8_t*)raw + shift; if (n && data) rfq_copy_h2d(c, p, data, n); }
    ~Dev() { rfq_dev_free(c, raw); } };

static int fail(const char* what, const char* why) { fprintf(stderr, "%s: %s\n", what, why); return 1; }

// the rows of a call, without names (q null: no quality rows); the caller adds d_names / names_len / d_name_off where it has them
static rfq_rows_in rows_in(uint64_t n, uint32_t L, int codes, const Dev& b, const Dev* q, const Dev& l) {
    rfq_rows_in in; memset(&in, 0, sizeof in);
    in.n_rows = n; in.row_len = L; in.base_mode = codes ? RFQ_ROWS_CODE : RFQ_ROWS_ASCII; in.d_bases = b.p; in.d_quals = q ? q->p : nullptr; in.d_lens = (const int32_t*)l.p;
    return in;
}
