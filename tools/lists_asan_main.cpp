// lists_asan_main.cpp - stand-alone host program for a sanitizer run of the fused decode's position-list passes (k_dec_pos_sum2 on the 16-bytes-per-lane front,
// k_dec_pos_link2, k_dec_pos_off, k_dec_pos_list) on the SIMT-interpreter build (CPU only, no Python): tools/lists_asan.sh compiles it with the library's sources
// under -fsanitize=address,undefined and runs it on the fixture images of tests/_lists.py.  Every image lies in a heap allocation that ENDS WITH ITS LAST BYTE -
// the N-position section is a chunk's last, so the last lanes' look-ahead meets the end of the allocation.
//   lists_asan_main IMAGE.rfq [IMAGE.rfq ...]     (IMAGE.fq beside it: the text it decodes to)
// per image: the whole image under RFQ_POS_SEG 1024 / 2048 / 4096 - the text must come back on the fused path -, then the image cut 1 .. 19 bytes short - every
// cut must be refused (an error code, or a decode that stops in front of the damaged chunk), nothing may be read past the allocation.  exit 1 on any failure.
#include "../include/rfq_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static bool slurp(const std::string& path, std::vector<uint8_t>* out) {
    FILE* f = fopen(path.c_str(), "rb"); if (!f) { fprintf(stderr, "%s: cannot open\n", path.c_str()); return false; }
    uint8_t buf[65536]; size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + k);
    fclose(f);
    return true;
}
// decode the first n bytes of img from an allocation of exactly n bytes; *text = what came back
static int decode(rfq_ctx* ctx, const std::vector<uint8_t>& img, size_t n, rfq_decode_result* r, std::vector<uint8_t>* text) {
    uint8_t* d = (uint8_t*)malloc(n); if (!d) return -1;
    memcpy(d, img.data(), n);
    rfq_decode_args a; memset(&a, 0, sizeof a); memset(r, 0, sizeof *r);
    a.d_rfq = d; a.n = n; a.has_header = 1; a.final = 1;
    const int rc = rfq_decode_batch(ctx, &a, r);
    text->assign((size_t)(rc ? 0 : r->n1), 0);
    if (!rc && r->n1 && rfq_copy_d2h(ctx, text->data(), r->d_fq1, r->n1)) { free(d); return -1; }
    free(d);
    return rc;
}
static bool fused(rfq_ctx* ctx) {
    const char* names[64]; float ms[64]; const int k = rfq_last_timings(ctx, names, ms, 64); bool emit = false, expanded = false;
    for (int i = 0; i < k && i < 64; i++) { if (!strcmp(names[i], "emit")) emit = true; if (!strcmp(names[i], "emit_expanded")) expanded = true; }
    return emit && !expanded;
}

static int run(rfq_ctx* ctx, const std::string& path) {
    std::vector<uint8_t> img, want, got;
    if (!slurp(path, &img) || !slurp(path.substr(0, path.size() - 4) + ".fq", &want)) return 1;
    rfq_decode_result r; int bad = 0; uint32_t n_chunks = 0;
    for (const char* seg : { "1024", "2048", "4096" }) {
        if (rfq_set_option(ctx, "RFQ_POS_SEG", seg)) { fprintf(stderr, "RFQ_POS_SEG=%s refused\n", seg); return 1; }
        const int rc = decode(ctx, img, img.size(), &r, &got);
        if (rc) { fprintf(stderr, "%s: RFQ_POS_SEG=%s: %d %s\n", path.c_str(), seg, rc, rfq_last_error(ctx)); bad = 1; continue; }
        n_chunks = r.n_chunks;
        if (got != want) { fprintf(stderr, "%s: RFQ_POS_SEG=%s: the text differs (%zu bytes, %zu expected)\n", path.c_str(), seg, got.size(), want.size()); bad = 1; }
        if (!fused(ctx)) { fprintf(stderr, "%s: RFQ_POS_SEG=%s: not on the fused path\n", path.c_str(), seg); bad = 1; }
    }
    rfq_set_option(ctx, "RFQ_POS_SEG", nullptr);
    int refused = 0, errors = 0;
    for (size_t cut = 1; cut <= 19 && cut < img.size(); cut++) {
        const int rc = decode(ctx, img, img.size() - cut, &r, &got);
        if (rc) { refused++; errors++; }
        else if (r.consumed < img.size() - cut && got.size() < want.size() && !memcmp(got.data(), want.data(), got.size())) refused++;    // (stopped in front of the cut chunk)
        else { fprintf(stderr, "%s: cut %zu bytes short: accepted (%zu bytes of text)\n", path.c_str(), cut, got.size()); bad = 1; }
    }
    printf("%s: %zu bytes, %u chunks, %zu bytes of text under three segment sizes; %d cuts refused (%d with an error code)%s\n", path.c_str(), img.size(), n_chunks, want.size(),
           refused, errors, bad ? "  FAILED" : "");
    return bad;
}

int main(int argc, char** argv) {
    rfq_ctx* ctx = nullptr;
    if (rfq_create(&ctx, 0)) { fprintf(stderr, "rfq_create failed\n"); return 1; }
    int bad = 0;
    for (int i = 1; i < argc; i++) bad |= run(ctx, argv[i]);
    rfq_destroy(ctx);
    printf("%s\n", bad ? "lists_asan: FAILED" : "lists_asan: all images decoded, all cuts refused, no sanitizer report");
    return bad;
}
