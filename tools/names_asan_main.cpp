// names_asan_main.cpp - stand-alone host program for a sanitizer run of rfq_decode_names on the SIMT-interpreter build (CPU only, no Python):
// tools/names_asan.sh compiles it with the library's sources under -fsanitize=address,undefined and runs it on fixture images a test helper wrote.
//   names_asan_main IMAGE.rfq [IMAGE.rfq ...]     prints rows / bytes / the first and last name of each image; exit 1 on any error
#include "../include/rfq_hip.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static int run(rfq_ctx* ctx, const char* path) {
    FILE* f = fopen(path, "rb"); if (!f) { fprintf(stderr, "%s: cannot open\n", path); return 1; }
    std::vector<uint8_t> img; uint8_t buf[65536]; size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) img.insert(img.end(), buf, buf + k);
    fclose(f);
    void* d = nullptr;
    if (rfq_dev_malloc(ctx, &d, img.size() + 1) || rfq_copy_h2d(ctx, d, img.data(), img.size())) return 1;
    rfq_decode_names_args a; memset(&a, 0, sizeof a); rfq_decode_names_result q, r;
    a.d_rfq = (const uint8_t*)d; a.n = img.size(); a.has_header = 1; a.final = 1; a.size_only = 1;
    int rc = rfq_decode_names(ctx, &a, &q);
    if (rc) { fprintf(stderr, "%s: size query: %d %s\n", path, rc, rfq_last_error(ctx)); return 1; }
    // exact caller buffers, the blob one byte off a 16-byte boundary
    void *db = nullptr, *dof = nullptr;
    if (rfq_dev_malloc(ctx, &db, (size_t)q.names_len + 1) || rfq_dev_malloc(ctx, &dof, (size_t)(q.n_rows + 1) * 8)) return 1;
    a.size_only = 0; a.d_names = (uint8_t*)db + 1; a.names_cap = (size_t)q.names_len; a.d_name_off = (uint64_t*)dof; a.off_cap = (size_t)q.n_rows + 1;
    rc = rfq_decode_names(ctx, &a, &r);
    if (rc) { fprintf(stderr, "%s: %d %s\n", path, rc, rfq_last_error(ctx)); return 1; }
    std::vector<uint8_t> blob((size_t)r.names_len + 1); std::vector<uint64_t> off((size_t)r.n_rows + 1);
    if (rfq_copy_d2h(ctx, blob.data(), r.d_names, (size_t)r.names_len) || rfq_copy_d2h(ctx, off.data(), r.d_name_off, off.size() * 8)) return 1;
    if (r.n_rows != q.n_rows || r.names_len != q.names_len || off[0] != 0 || off[(size_t)r.n_rows] != r.names_len) { fprintf(stderr, "%s: counts disagree\n", path); return 1; }
    // context-owned results too
    a.d_names = nullptr; a.d_name_off = nullptr; a.names_cap = a.off_cap = 0;
    rc = rfq_decode_names(ctx, &a, &r);
    if (rc) { fprintf(stderr, "%s: context-owned: %d %s\n", path, rc, rfq_last_error(ctx)); return 1; }
    const std::string first(blob.begin(), blob.begin() + (r.n_rows ? (size_t)off[1] : 0));
    const std::string last(blob.begin() + (r.n_rows ? (size_t)off[(size_t)r.n_rows - 1] : 0), blob.begin() + (size_t)r.names_len);
    printf("%s: %llu rows, %llu name bytes, longest %u, first %s, last %s\n", path, (unsigned long long)r.n_rows, (unsigned long long)r.names_len, r.max_name, first.c_str(), last.c_str());
    rfq_dev_free(ctx, d); rfq_dev_free(ctx, db); rfq_dev_free(ctx, dof);
    return 0;
}

int main(int argc, char** argv) {
    rfq_ctx* ctx = nullptr;
    if (rfq_create(&ctx, 0)) { fprintf(stderr, "rfq_create failed\n"); return 1; }
    int bad = 0;
    for (int i = 1; i < argc; i++) bad |= run(ctx, argv[i]);
    rfq_destroy(ctx);
    return bad;
}
