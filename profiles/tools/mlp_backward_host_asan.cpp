// The host half of ftl_mlp_backward under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own: the workspace query
// against the header's formula over a sweep of set layouts, and every refusal that comes before any device work.  Nothing here launches:
// each ftl_mlp_backward call is refused by a check, the last of them the workspace's alignment.  Built and run by
// profiles/tools/mlp_backward_host_asan.sh (host code only is instrumented; no GPU is needed).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "ftl.h"

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #c, ftl_last_error()); failures++; } } while (0)

static ftl_mlp net_of(const int32_t* w, int L, int32_t n_sets, int32_t eps, int32_t first) {
    ftl_mlp m;
    std::memset(&m, 0, sizeof m);
    m.params = reinterpret_cast<float*>(4096);                  // never dereferenced: the checks under test come first
    m.n_layers = L; m.n_sets = n_sets; m.envs_per_set = eps; m.env_first = first;
    for (int l = 0; l <= L && l <= FTL_MLP_MAX_LAYERS; l++) m.width[l] = w[l];
    m.set_stride = ftl_mlp_param_count(w, L);
    return m;
}

static int64_t spans_by_hand(int64_t n_blocks, int64_t n, int64_t eps, int64_t first) {
    int64_t spans = 0, r = 0;
    while (r < n) {                                             // the rows of one set after the other
        const int64_t set_end = ((first + r) / eps + 1) * eps - first, end = set_end < n ? set_end : n;
        const int64_t tiles = (end - r + 31) / 32;
        spans += (n_blocks * tiles + FTL_MLP_BWD_SPAN - 1) / FTL_MLP_BWD_SPAN;
        r = end;
    }
    return spans;
}

int main() {
    static char fake_handle[64];
    ftl_handle* h = reinterpret_cast<ftl_handle*>(fake_handle); // only its being non-null is read before the last check
    float* p = reinterpret_cast<float*>(8192);
    const int32_t w[4] = {180, 64, 64, 2};
    const int64_t count = ftl_mlp_param_count(w, 3);
    EXPECT(count == 15874);
    long queries = 0;
    const int32_t ns[] = {1, 15, 31, 32, 33, 40, 64, 65, 1000, 65536, 1 << 24}, bs[] = {1, 2, 3, 32, 63, 64, 65, 70, 65535};
    const int32_t es[] = {1, 7, 10, 11, 32, 33, 64, 1000, 65536, 1 << 30}, fs[] = {0, 1, 5, 13, 31, 32, 1000};
    for (int32_t n : ns) for (int32_t b : bs) for (int32_t e : es) for (int32_t f : fs) {
        if ((int64_t)n / e > 100000) continue;                  // (keeps the by-hand loop short)
        const ftl_mlp m = net_of(w, 3, 1 << 30, e, f);
        EXPECT(ftl_sizeof_mlp_backward_workspace(&m, b, n) == spans_by_hand(b, n, e, f) * count * 4);
        queries++;
    }
    ftl_mlp m = net_of(w, 3, 1, 6, 0);
    EXPECT(ftl_sizeof_mlp_backward_workspace(nullptr, 1, 1) == -1 && ftl_sizeof_mlp_backward_workspace(&m, 0, 1) == -1);
    EXPECT(ftl_sizeof_mlp_backward_workspace(&m, 1, -5) == -1);
    const int64_t need = ftl_sizeof_mlp_backward_workspace(&m, 2, 6), xb = 6 * 180 * 4, db = 6 * 2 * 4;
    EXPECT(need == count * 4);
    auto call = [&](const ftl_handle* hh, const ftl_mlp* mm, int32_t nb, int32_t n, const float* x, int64_t xbb, const float* dy, int64_t dbb,
                    float* grad, void* ws, int64_t wsb) { return ftl_mlp_backward(hh, mm, nb, n, x, xbb, dy, dbb, grad, ws, wsb, nullptr); };
    EXPECT(call(nullptr, &m, 2, 6, p, xb, p, db, p, p, need) == FTL_E_INVALID);
    EXPECT(call(h, nullptr, 2, 6, p, xb, p, db, p, p, need) == FTL_E_INVALID);
    EXPECT(call(h, &m, 2, 6, nullptr, xb, p, db, p, p, need) == FTL_E_INVALID);
    EXPECT(call(h, &m, 2, 6, p, xb, nullptr, db, p, p, need) == FTL_E_INVALID);
    EXPECT(call(h, &m, 2, 6, p, xb, p, db, nullptr, p, need) == FTL_E_INVALID);
    EXPECT(call(h, &m, 2, 6, p, xb, p, db, p, nullptr, need) == FTL_E_INVALID);
    EXPECT(call(h, &m, 0, 6, p, xb, p, db, p, p, need) == FTL_E_INVALID && call(h, &m, 2, 0, p, xb, p, db, p, p, need) == FTL_E_INVALID);
    EXPECT(call(h, &m, 65536, 6, p, xb, p, db, p, p, need) == FTL_E_UNSUPPORTED);
    EXPECT(call(h, &m, 2, 7, p, 7 * 180 * 4, p, 7 * 2 * 4, p, p, need) == FTL_E_INVALID);       // the last row lies beyond the last set
    EXPECT(call(h, &m, 2, 6, p, xb - 4, p, db, p, p, need) == FTL_E_INVALID && call(h, &m, 2, 6, p, xb + 2, p, db, p, p, need) == FTL_E_INVALID);
    EXPECT(call(h, &m, 2, 6, p, xb, p, db - 4, p, p, need) == FTL_E_INVALID && call(h, &m, 2, 6, p, xb, p, db + 1, p, p, need) == FTL_E_INVALID);
    EXPECT(call(h, &m, 2, 6, p, xb, p, db, p, p, need - 1) == FTL_E_INVALID && std::strstr(ftl_last_error(), "workspace_bytes"));
    EXPECT(call(h, &m, 2, 6, p + 0, xb, p, db, reinterpret_cast<float*>(8193), p, need) == FTL_E_INVALID);
    ftl_mlp bad = m; bad.activation = 7;
    EXPECT(call(h, &bad, 2, 6, p, xb, p, db, p, p, need) == FTL_E_INVALID && std::strstr(ftl_last_error(), "activation"));
    bad = m; bad.width[1] = 257;
    EXPECT(call(h, &bad, 2, 6, p, xb, p, db, p, p, need) == FTL_E_UNSUPPORTED);
    const int32_t big[2] = {7, 1};
    ftl_mlp many = net_of(big, 1, 1 << 25, 1, 0);
    EXPECT(call(h, &many, 1, 1 << 25, p, (int64_t)(1 << 25) * 28, p, (int64_t)(1 << 25) * 4, p, p, INT64_MAX) == FTL_E_UNSUPPORTED);
    ftl_mlp one = net_of(w, 3, 1, 1 << 30, 0);
    EXPECT(call(h, &one, 32, 1 << 24, p, (int64_t)(1 << 24) * 720, p, (int64_t)(1 << 24) * 8, p, p, 8) == FTL_E_INVALID);   // 2^18 spans, a valid plan: only the workspace is short
    // every check passed but the last: the workspace's alignment
    EXPECT(call(h, &m, 2, 6, p, xb, p, db, p, reinterpret_cast<void*>(8193), need) == FTL_E_INVALID && std::strstr(ftl_last_error(), "workspace must be"));
    std::printf("%ld workspace queries and the refusals of ftl_mlp_backward: %d failures\n", queries, failures);
    return failures != 0;
}
