// text_rows_asan_main.cpp - stand-alone host program for a sanitizer run of rfq_text_rows on the SIMT-interpreter build (CPU only, no Python):
// tools/text_rows_asan.sh compiles it with the library's sources under -fsanitize=address,undefined and runs it on fixture texts a test helper wrote.
//   text_rows_asan_main TEXT.fq [TEXT.fq ...]     every text as RFQ_SE and RFQ_PE_INTERLEAVED, final and not, both base modes, the text one byte off a
//   16-byte boundary, into exact caller buffers (the blob misaligned too); a refusal with an RFQ_E_* code is a result, anything else is an error (exit 1)
#include "../include/rfq_hip.h"
#include <cstdio>
#include <cstring>
#include <vector>

static int one(rfq_ctx* ctx, const char* path, const uint8_t* d_text, size_t n, int paired, int final, int codes) {
    rfq_text_rows_args a; memset(&a, 0, sizeof a); rfq_text_rows_result q, r;
    a.d_fq1 = d_text; a.n1 = n; a.paired = paired; a.final = final;
    int rc = rfq_text_rows(ctx, &a, &q);
    if (rc) { if (rc == RFQ_E_DATA || rc == RFQ_E_UNPINNED || rc == RFQ_E_ARG) { printf("%s: refused (%d) %s\n", path, rc, rfq_last_error(ctx)); return 0; }
              fprintf(stderr, "%s: size query: %d %s\n", path, rc, rfq_last_error(ctx)); return 1; }
    const uint32_t L = ((q.max_len + 15u) & ~15u) + (codes ? 0u : 3u);      // whole groups in code mode, byte stores otherwise
    const size_t rows = (size_t)q.n_rows, rb = rows * (L ? L : 1);
    void *db = nullptr, *dq = nullptr, *dl = nullptr, *dn = nullptr, *dof = nullptr;
    if (rfq_dev_malloc(ctx, &db, rb + 1) || rfq_dev_malloc(ctx, &dq, rb + 1) || rfq_dev_malloc(ctx, &dl, rows * 4 + 4) || rfq_dev_malloc(ctx, &dn, (size_t)q.names_len + 2) ||
        rfq_dev_malloc(ctx, &dof, (rows + 1) * 8)) return 1;
    a.row_len = L ? L : 1; a.base_mode = codes ? RFQ_ROWS_CODE : RFQ_ROWS_ASCII; a.qual_offset = 33; a.pad_base = 0xEE; a.pad_qual = 0xDD;
    a.d_bases = (uint8_t*)db; a.bases_cap = rb; a.d_quals = (uint8_t*)dq; a.quals_cap = rb; a.d_lens = (int32_t*)dl; a.lens_cap = rows;
    a.d_names = (uint8_t*)dn + 1; a.names_cap = (size_t)q.names_len; a.d_name_off = (uint64_t*)dof; a.off_cap = rows + 1;
    rc = rfq_text_rows(ctx, &a, &r);
    int bad = 0;
    if (rc == RFQ_E_DATA && codes) printf("%s: refused (%d) %s\n", path, rc, rfq_last_error(ctx));
    else if (rc) { fprintf(stderr, "%s: %d %s\n", path, rc, rfq_last_error(ctx)); bad = 1; }
    else {
        std::vector<uint64_t> off(rows + 1); std::vector<int32_t> lens(rows + 1); std::vector<uint8_t> B(rb + 1);
        if (rfq_copy_d2h(ctx, off.data(), dof, off.size() * 8) || rfq_copy_d2h(ctx, lens.data(), dl, rows * 4) || rfq_copy_d2h(ctx, B.data(), db, rb)) bad = 1;
        uint64_t nb = 0; for (size_t i = 0; i < rows; i++) nb += (uint64_t)lens[i];
        if (r.n_rows != q.n_rows || r.names_len != q.names_len || off[0] != 0 || off[rows] != r.names_len || nb != r.n_bases || r.consumed1 > n) {
            fprintf(stderr, "%s: counts disagree\n", path); bad = 1; }
        printf("%s: paired %d final %d codes %d: %llu rows, %llu bases, %llu name bytes, longest %u / %u, consumed %zu of %zu, ended %d\n", path, paired, final, codes,
               (unsigned long long)r.n_rows, (unsigned long long)r.n_bases, (unsigned long long)r.names_len, r.max_len, r.max_name, r.consumed1, n, r.input_ended);
    }
    rfq_dev_free(ctx, db); rfq_dev_free(ctx, dq); rfq_dev_free(ctx, dl); rfq_dev_free(ctx, dn); rfq_dev_free(ctx, dof);
    return bad;
}

static int run(rfq_ctx* ctx, const char* path) {
    FILE* f = fopen(path, "rb"); if (!f) { fprintf(stderr, "%s: cannot open\n", path); return 1; }
    std::vector<uint8_t> text; uint8_t buf[65536]; size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) text.insert(text.end(), buf, buf + k);
    fclose(f);
    // the text one byte into its allocation, and not a byte of slack behind it
    void* d = nullptr;
    if (rfq_dev_malloc(ctx, &d, text.size() + 1) || rfq_copy_h2d(ctx, (uint8_t*)d + 1, text.data(), text.size())) return 1;
    int bad = 0;
    for (int paired = 0; paired <= 2; paired += 2) for (int final = 1; final >= 0; final--) for (int codes = 0; codes <= 1; codes++)
        bad |= one(ctx, path, (const uint8_t*)d + 1, text.size(), paired, final, codes);
    rfq_dev_free(ctx, d);
    return bad;
}

int main(int argc, char** argv) {
    rfq_ctx* ctx = nullptr;
    if (rfq_create(&ctx, 0)) { fprintf(stderr, "rfq_create failed\n"); return 1; }
    int bad = 0;
    for (int i = 1; i < argc; i++) bad |= run(ctx, argv[i]);
    rfq_destroy(ctx);
    return bad;
}
