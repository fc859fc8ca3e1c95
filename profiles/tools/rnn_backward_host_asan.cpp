// The host half of ftl_rnn_backward under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own: the workspace query
// against a by-hand count of groups and spans over a sweep of set layouts and block counts (below, at and above FTL_RNN_BWD_SPAN), and
// every refusal that comes before any device work.  Nothing here launches: each ftl_rnn_backward call is refused by a check, the last of
// them grad's alignment.  Built and run by profiles/tools/rnn_backward_host_asan.sh (host code only is instrumented; no GPU is needed).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "ftl.h"

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #c, ftl_last_error()); failures++; } } while (0)

static ftl_rnn net_of(const int32_t* w, int Lt, int32_t cell, uint32_t flags, int32_t n_sets, int32_t eps, int32_t first) {
    ftl_rnn m;
    std::memset(&m, 0, sizeof m);
    m.params = reinterpret_cast<float*>(4096);                  // never dereferenced: the checks under test come first
    m.state = reinterpret_cast<float*>(8192);
    m.n_layers = Lt; m.n_sets = n_sets; m.envs_per_set = eps; m.env_first = first; m.cell = cell; m.flags = flags;
    for (int l = 0; l <= Lt + 1 && l <= FTL_MLP_MAX_LAYERS; l++) m.width[l] = w[l];
    m.set_stride = ftl_rnn_param_count(w, Lt, cell, flags);
    m.state_stride = 2 * cell + ((flags & FTL_RNN_PREV_ACTION) ? w[Lt + 1] : 0) + 1;
    return m;
}

// groups and spans, one set after the other, one group after the other
static void plan_by_hand(int64_t B, int64_t n, int64_t eps, int64_t first, int64_t& groups, int64_t& spans) {
    const int64_t G = FTL_RNN_BWD_SPAN / B > 1 ? FTL_RNN_BWD_SPAN / B : 1;
    groups = spans = 0;
    for (int64_t r = 0; r < n;) {
        const int64_t set_end = ((first + r) / eps + 1) * eps - first, end = set_end < n ? set_end : n;
        const int64_t tiles = (end - r + 31) / 32;
        groups += (tiles + G - 1) / G;
        spans += (tiles / G) * ((G * B + FTL_RNN_BWD_SPAN - 1) / FTL_RNN_BWD_SPAN) + ((tiles % G) * B + FTL_RNN_BWD_SPAN - 1) / FTL_RNN_BWD_SPAN;
        r = end;
    }
}

int main() {
    static char fake_handle[64];
    ftl_handle* h = reinterpret_cast<ftl_handle*>(fake_handle); // only its being non-null is read before the last check
    float* p = reinterpret_cast<float*>(16384);
    const int32_t w[4] = {180, 64, 64, 2};
    const int32_t C = 64;
    const uint32_t both = FTL_RNN_PREV_ACTION | FTL_RNN_PREV_REWARD;
    const int64_t count = ftl_rnn_param_count(w, 2, C, both), U = 64 + 2 + 1 + C;
    EXPECT(count == (180 + 1) * 64 + (64 + 1) * 64 + (U + 1) * 4 * C + (C + 1) * 2);
    EXPECT(ftl_sizeof_rnn_gradient() == sizeof(ftl_rnn_gradient));
    long queries = 0;
    const int32_t ns[] = {1, 15, 31, 32, 33, 40, 64, 65, 1000, 65536, 1 << 22}, bs[] = {1, 2, 3, 21, 22, 32, 33, 63, 64, 65, 70, 128, 129, 65535};
    const int32_t es[] = {1, 7, 10, 11, 32, 33, 64, 700, 1000, 65536, 1 << 30}, fs[] = {0, 1, 5, 13, 31, 32, 1000};
    for (int32_t n : ns) for (int32_t b : bs) for (int32_t e : es) for (int32_t f : fs) {
        if ((int64_t)n / e > 100000) continue;                  // (keeps the by-hand loop short)
        const ftl_rnn m = net_of(w, 2, C, both, 1 << 30, e, f);
        int64_t groups, spans;
        plan_by_hand(b, n, e, f, groups, spans);
        EXPECT(ftl_sizeof_rnn_backward_workspace(&m, b, n) == 4 * (spans * count + (int64_t)b * n * 2 * C + groups * 32 * U));
        queries++;
    }
    ftl_rnn m = net_of(w, 2, C, both, 1, 6, 0);
    EXPECT(ftl_sizeof_rnn_backward_workspace(nullptr, 1, 1) == -1 && ftl_sizeof_rnn_backward_workspace(&m, 0, 1) == -1);
    EXPECT(ftl_sizeof_rnn_backward_workspace(&m, 1, -5) == -1);
    const int64_t need = ftl_sizeof_rnn_backward_workspace(&m, 3, 6);
    EXPECT(need == 4 * (count + 3 * 6 * 2 * C + 32 * U));
    ftl_rnn_sequence s;
    std::memset(&s, 0, sizeof s);
    s.obs = p; s.action = p; s.reward = reinterpret_cast<const double*>(p); s.kind = reinterpret_cast<const uint8_t*>(p);
    s.obs_block_bytes = 6 * 180 * 4; s.action_block_bytes = 6 * 16; s.reward_block_bytes = 6 * 8; s.kind_block_bytes = 6;
    ftl_rnn_gradient g;
    std::memset(&g, 0, sizeof g);
    g.dhead = p; g.dhead_block_bytes = 6 * 2 * 4; g.grad = p; g.workspace = p; g.workspace_bytes = need;
    auto call = [&](const ftl_handle* hh, const ftl_rnn* mm, int32_t nb, int32_t n, const ftl_rnn_sequence* ss, const ftl_rnn_gradient* gg) {
        return ftl_rnn_backward(hh, mm, nb, n, ss, gg, nullptr);
    };
    EXPECT(call(nullptr, &m, 3, 6, &s, &g) == FTL_E_INVALID && call(h, nullptr, 3, 6, &s, &g) == FTL_E_INVALID);
    EXPECT(call(h, &m, 3, 6, nullptr, &g) == FTL_E_INVALID && call(h, &m, 3, 6, &s, nullptr) == FTL_E_INVALID);
    EXPECT(call(h, &m, 0, 6, &s, &g) == FTL_E_INVALID && call(h, &m, 3, 0, &s, &g) == FTL_E_INVALID);
    EXPECT(call(h, &m, 65536, 6, &s, &g) == FTL_E_UNSUPPORTED);
    EXPECT(call(h, &m, 3, 7, &s, &g) == FTL_E_INVALID && std::strstr(ftl_last_error(), "last weight set"));
    ftl_rnn_sequence bs_ = s;
    bs_.obs = nullptr;          EXPECT(call(h, &m, 3, 6, &bs_, &g) == FTL_E_INVALID && std::strstr(ftl_last_error(), "seq->obs"));
    bs_ = s; bs_.kind = nullptr; EXPECT(call(h, &m, 3, 6, &bs_, &g) == FTL_E_INVALID && std::strstr(ftl_last_error(), "seq->kind"));
    bs_ = s; bs_.action = nullptr; EXPECT(call(h, &m, 3, 6, &bs_, &g) == FTL_E_INVALID && std::strstr(ftl_last_error(), "seq->action"));
    bs_ = s; bs_.reward = nullptr; EXPECT(call(h, &m, 3, 6, &bs_, &g) == FTL_E_INVALID && std::strstr(ftl_last_error(), "seq->reward"));
    bs_ = s; bs_.obs_block_bytes -= 4; EXPECT(call(h, &m, 3, 6, &bs_, &g) == FTL_E_INVALID && std::strstr(ftl_last_error(), "obs_block_bytes"));
    bs_ = s; bs_.action_block_bytes += 4; EXPECT(call(h, &m, 3, 6, &bs_, &g) == FTL_E_INVALID && std::strstr(ftl_last_error(), "action_block_bytes"));
    bs_ = s; bs_.reward_block_bytes -= 8; EXPECT(call(h, &m, 3, 6, &bs_, &g) == FTL_E_INVALID && std::strstr(ftl_last_error(), "reward_block_bytes"));
    bs_ = s; bs_.kind_block_bytes = 5; EXPECT(call(h, &m, 3, 6, &bs_, &g) == FTL_E_INVALID && std::strstr(ftl_last_error(), "kind_block_bytes"));
    bs_ = s; bs_.reward0 = reinterpret_cast<const double*>(16388); EXPECT(call(h, &m, 3, 6, &bs_, &g) == FTL_E_INVALID && std::strstr(ftl_last_error(), "reward0"));
    ftl_rnn_gradient bg = g;
    bg.dhead = nullptr;            EXPECT(call(h, &m, 3, 6, &s, &bg) == FTL_E_INVALID && std::strstr(ftl_last_error(), "g->dhead"));
    bg = g; bg.grad = nullptr;     EXPECT(call(h, &m, 3, 6, &s, &bg) == FTL_E_INVALID && std::strstr(ftl_last_error(), "g->grad"));
    bg = g; bg.workspace = nullptr; EXPECT(call(h, &m, 3, 6, &s, &bg) == FTL_E_INVALID && std::strstr(ftl_last_error(), "g->workspace"));
    bg = g; bg.dhead_block_bytes -= 4; EXPECT(call(h, &m, 3, 6, &s, &bg) == FTL_E_INVALID && std::strstr(ftl_last_error(), "dhead_block_bytes"));
    bg = g; bg.workspace_bytes = need - 1; EXPECT(call(h, &m, 3, 6, &s, &bg) == FTL_E_INVALID && std::strstr(ftl_last_error(), "workspace_bytes"));
    bg = g; bg.dstate_in = reinterpret_cast<const float*>(16386); EXPECT(call(h, &m, 3, 6, &s, &bg) == FTL_E_INVALID && std::strstr(ftl_last_error(), "dstate_in"));
    bg = g; bg.workspace = reinterpret_cast<void*>(16385); EXPECT(call(h, &m, 3, 6, &s, &bg) == FTL_E_INVALID && std::strstr(ftl_last_error(), "workspace must be"));
    ftl_rnn bad = m; bad.activation = 1;
    EXPECT(call(h, &bad, 3, 6, &s, &g) == FTL_E_UNSUPPORTED && std::strstr(ftl_last_error(), "ReLU"));
    bad = m; bad.cell = 129;
    EXPECT(call(h, &bad, 3, 6, &s, &g) == FTL_E_UNSUPPORTED);
    bad = m; bad.state = nullptr;
    EXPECT(call(h, &bad, 3, 6, &s, &g) == FTL_E_INVALID && std::strstr(ftl_last_error(), "state"));
    const int32_t wide[5] = {180, 256, 256, 256, 5};
    ftl_rnn big = net_of(wide, 3, 128, both, 1, 6, 0);
    ftl_rnn_sequence ws_ = s; ws_.action_block_bytes = 6 * 4;
    ftl_rnn_gradient wg = g; wg.dhead_block_bytes = 6 * 5 * 4; wg.workspace_bytes = INT64_MAX;
    EXPECT(call(h, &big, 3, 6, &ws_, &wg) == FTL_E_UNSUPPORTED && std::strstr(ftl_last_error(), "LDS"));
    const int32_t lim[4] = {180, 256, 256, 5};
    ftl_rnn fits = net_of(lim, 2, 128, both, 1, 6, 0);
    wg.grad = reinterpret_cast<float*>(16385);
    EXPECT(call(h, &fits, 3, 6, &ws_, &wg) == FTL_E_INVALID && std::strstr(ftl_last_error(), "grad must be"));
    ftl_rnn many = net_of(w, 2, C, both, 1, 1 << 29, 0);          // 2^24 tiles at B = 64: a span each, one too many
    ftl_rnn_sequence ms = s; ms.obs_block_bytes = (int64_t)(1 << 29) * 720; ms.action_block_bytes = (int64_t)(1 << 29) * 16;
    ms.reward_block_bytes = (int64_t)(1 << 29) * 8; ms.kind_block_bytes = 1 << 29;
    ftl_rnn_gradient mg = g; mg.dhead_block_bytes = (int64_t)(1 << 29) * 8; mg.workspace_bytes = INT64_MAX;
    EXPECT(call(h, &many, 64, 1 << 29, &ms, &mg) == FTL_E_UNSUPPORTED && std::strstr(ftl_last_error(), "spans"));
    // every check passed but the last: grad's alignment
    bg = g; bg.grad = reinterpret_cast<float*>(16385);
    EXPECT(call(h, &m, 3, 6, &s, &bg) == FTL_E_INVALID && std::strstr(ftl_last_error(), "grad must be"));
    std::printf("%ld workspace queries and the refusals of ftl_rnn_backward: %d failures\n", queries, failures);
    return failures != 0;
}
