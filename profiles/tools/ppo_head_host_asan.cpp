// The host half of ftl_ppo_head under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own: the workspace query
// against a segment count by hand over a sweep of (n_blocks, n, n_sets), and every refusal that comes before any device work.  Nothing here
// launches: each ftl_ppo_head call is refused by a check, the last of them the workspace's alignment.  Built and run by
// profiles/tools/ppo_head_host_asan.sh (host code only is instrumented; no GPU is needed).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "ftl.h"

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #c, ftl_last_error()); failures++; } } while (0)

static ftl_ppo_head_args good() {
    ftl_ppo_head_args a;
    std::memset(&a, 0, sizeof a);
    float* p = reinterpret_cast<float*>(8192);                  // never dereferenced: the checks under test come first
    a.n_blocks = 2; a.n = 12; a.n_sets = 3; a.width = 2;
    a.head_new = a.head_old = a.noise = a.sigma_old = a.sigma_new = a.log_sigma_shift = a.adv = a.ret = a.value_new = p;
    a.kind = reinterpret_cast<const uint8_t*>(p);
    a.dhead = a.dvalue = a.dlog_std = p;
    a.stats = reinterpret_cast<double*>(p);
    a.workspace = p;
    a.head_new_block_bytes = a.head_old_block_bytes = a.noise_block_bytes = a.dhead_block_bytes = 12 * 8;
    a.adv_block_bytes = a.ret_block_bytes = a.value_new_block_bytes = a.dvalue_block_bytes = 12 * 4;
    a.kind_block_bytes = 12;
    a.clip_lo = 0.8f; a.clip_hi = 1.2f; a.vf_coef = 0.5f; a.normalize = 1;
    a.workspace_bytes = ftl_sizeof_ppo_head_workspace(2, 12, 3);
    return a;
}

int main() {
    static char fake_handle[64];
    ftl_handle* h = reinterpret_cast<ftl_handle*>(fake_handle); // only its being non-null is read before the last check
    EXPECT(ftl_sizeof_ppo_head_args() == sizeof(ftl_ppo_head_args));
    long queries = 0;
    const int32_t bs[] = {1, 2, 3, 32, 65535}, sets[] = {1, 2, 3, 64, 1024, 65536};
    const int32_t rows[] = {1, 2, 63, 64, 65, FTL_PPO_SEG - 1, FTL_PPO_SEG, FTL_PPO_SEG + 1, 3 * FTL_PPO_SEG + 5, 65536};
    for (int32_t b : bs) for (int32_t s : sets) for (int32_t r : rows) {
        const int64_t n = (int64_t)s * r;
        if (n > INT32_MAX) continue;
        const int64_t segs = (int64_t)b * s * ((r + FTL_PPO_SEG - 1) / FTL_PPO_SEG);
        EXPECT(ftl_sizeof_ppo_head_workspace(b, (int32_t)n, s) == (segs > INT32_MAX ? -1 : segs * 72 + (int64_t)s * 16));
        queries++;
    }
    EXPECT(ftl_sizeof_ppo_head_workspace(0, 4, 2) == -1 && ftl_sizeof_ppo_head_workspace(1, 0, 1) == -1 && ftl_sizeof_ppo_head_workspace(1, 4, 0) == -1);
    EXPECT(ftl_sizeof_ppo_head_workspace(1, 5, 2) == -1 && ftl_sizeof_ppo_head_workspace(-1, 4, 2) == -1 && ftl_sizeof_ppo_head_workspace(1, 4, -2) == -1);
    EXPECT(ftl_sizeof_ppo_head_workspace(INT32_MAX, INT32_MAX, INT32_MAX) == -1);
    ftl_ppo_head_args a = good();
    EXPECT(a.workspace_bytes == 2 * 3 * 72 + 3 * 16);
    EXPECT(ftl_ppo_head(nullptr, &a, nullptr) == FTL_E_INVALID && ftl_ppo_head(h, nullptr, nullptr) == FTL_E_INVALID);
#define REFUSED(code, word, change) do { ftl_ppo_head_args b = good(); change; EXPECT(ftl_ppo_head(h, &b, nullptr) == code && std::strstr(ftl_last_error(), "ftl_ppo_head") && std::strstr(ftl_last_error(), word)); } while (0)
    REFUSED(FTL_E_INVALID, "head_new", b.head_new = nullptr);
    REFUSED(FTL_E_INVALID, "head_old", b.head_old = nullptr);
    REFUSED(FTL_E_INVALID, "noise", b.noise = nullptr);
    REFUSED(FTL_E_INVALID, "sigma_old", b.sigma_old = nullptr);
    REFUSED(FTL_E_INVALID, "sigma_new", b.sigma_new = nullptr);
    REFUSED(FTL_E_INVALID, "adv", b.adv = nullptr);
    REFUSED(FTL_E_INVALID, "ret", b.ret = nullptr);
    REFUSED(FTL_E_INVALID, "kind", b.kind = nullptr);
    REFUSED(FTL_E_INVALID, "dhead", b.dhead = nullptr);
    REFUSED(FTL_E_INVALID, "dlog_std", b.dlog_std = nullptr);
    REFUSED(FTL_E_INVALID, "stats", b.stats = nullptr);
    REFUSED(FTL_E_INVALID, "workspace", b.workspace = nullptr);
    REFUSED(FTL_E_INVALID, "dvalue without value_new", b.value_new = nullptr);
    REFUSED(FTL_E_INVALID, "value_new without dvalue", b.dvalue = nullptr);
    REFUSED(FTL_E_INVALID, "n_blocks and n", b.n_blocks = 0);
    REFUSED(FTL_E_INVALID, "n_blocks and n", b.n = -12);
    REFUSED(FTL_E_INVALID, "n_sets", b.n_sets = 0);
    REFUSED(FTL_E_INVALID, "n_sets", b.n_sets = 5);
    REFUSED(FTL_E_UNSUPPORTED, "Discrete(5)", b.width = 5);
    REFUSED(FTL_E_UNSUPPORTED, "width", b.width = 0);
    REFUSED(FTL_E_INVALID, "head_new_block_bytes", b.head_new_block_bytes = 12 * 8 - 8);
    REFUSED(FTL_E_INVALID, "noise_block_bytes", b.noise_block_bytes = 12 * 8 + 4);
    REFUSED(FTL_E_INVALID, "adv_block_bytes", b.adv_block_bytes = 0);
    REFUSED(FTL_E_INVALID, "ret_block_bytes", b.ret_block_bytes = 12 * 4 + 2);
    REFUSED(FTL_E_INVALID, "value_new_block_bytes", b.value_new_block_bytes = -48);
    REFUSED(FTL_E_INVALID, "kind_block_bytes", b.kind_block_bytes = 11);
    REFUSED(FTL_E_INVALID, "dhead_block_bytes", b.dhead_block_bytes = 8);
    REFUSED(FTL_E_INVALID, "dvalue_block_bytes", b.dvalue_block_bytes = 12 * 4 + 1);
    REFUSED(FTL_E_INVALID, "head_old not aligned", b.head_old = reinterpret_cast<float*>(8196));
    REFUSED(FTL_E_INVALID, "adv not aligned", b.adv = reinterpret_cast<float*>(8194));
    REFUSED(FTL_E_INVALID, "stats not aligned", b.stats = reinterpret_cast<double*>(8196));
    REFUSED(FTL_E_INVALID, "clip_lo", b.clip_lo = 1.3f);
    REFUSED(FTL_E_INVALID, "clip_lo", b.clip_hi = std::nanf(""));
    REFUSED(FTL_E_INVALID, "normalize", b.normalize = 2);
    REFUSED(FTL_E_INVALID, "workspace_bytes", b.workspace_bytes -= 1);
    REFUSED(FTL_E_UNSUPPORTED, "segments", (b.n_blocks = 1 << 20, b.n = b.n_sets = 1 << 20, b.head_new_block_bytes = b.head_old_block_bytes = b.noise_block_bytes = b.dhead_block_bytes = 1 << 23,
                                            b.adv_block_bytes = b.ret_block_bytes = b.value_new_block_bytes = b.dvalue_block_bytes = 1 << 22, b.kind_block_bytes = 1 << 20));
    // every check passed but the last: the workspace's alignment -- for both widths, with and without the optional parts
    REFUSED(FTL_E_INVALID, "workspace must be 8-byte aligned", b.workspace = reinterpret_cast<void*>(8196));
    REFUSED(FTL_E_INVALID, "workspace must be 8-byte aligned", (b.workspace = reinterpret_cast<void*>(8193), b.value_new = nullptr, b.dvalue = nullptr, b.log_sigma_shift = nullptr));
    REFUSED(FTL_E_INVALID, "workspace must be 8-byte aligned", (b.workspace = reinterpret_cast<void*>(8194), b.width = 1, b.head_new = reinterpret_cast<float*>(8196),
                                                                b.head_new_block_bytes = b.head_old_block_bytes = b.noise_block_bytes = b.dhead_block_bytes = 12 * 4));
    std::printf("%ld workspace queries and the refusals of ftl_ppo_head: %d failures\n", queries, failures);
    return failures != 0;
}
