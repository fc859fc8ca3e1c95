// scenario_policy_main -- ftl_generate_scenarios from a file to a file, for builds of csrc/ftl_scenario.cpp that cannot be loaded into
// python: the FTL_SCEN_DEVICE_POLICY diagnostic build under AddressSanitizer / UBSan (tests/test_scenario_gen.py).
//   in:  the bytes of an ftl_config, of an ftl_scen_params, int64 n, n int64 seeds, then fixed_route_len x 2 doubles (the params'
//        fixed_route pointer is the writer's; it is pointed at these)
//   out: static_rects, robot_pos, robot_dir, robot_rect, route, route_len, init_traj, init_traj_len (the layout of ftl_scenarios, P = n),
//        then n status bytes
// Usage: scenario_policy_main IN OUT [threads]; exit status 0, 2 on a malformed file, 3 when the generator refuses the arguments.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ftl.h"

namespace {

std::vector<char> slurp(const char* path) {
    std::vector<char> b;
    if (FILE* f = fopen(path, "rb")) {
        char buf[1 << 16];
        for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) b.insert(b.end(), buf, buf + k);
        fclose(f);
    }
    return b;
}

template <class T> bool dump(FILE* f, const std::vector<T>& v) { return fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s IN OUT [threads]\n", argv[0]); return 2; }
    const std::vector<char> in = slurp(argv[1]);
    ftl_config cfg;
    ftl_scen_params sp;
    int64_t n = 0;
    const size_t head = sizeof cfg + sizeof sp + sizeof n;
    if (in.size() < head) { fprintf(stderr, "%s: shorter than its header\n", argv[1]); return 2; }
    memcpy(&cfg, in.data(), sizeof cfg);
    memcpy(&sp, in.data() + sizeof cfg, sizeof sp);
    memcpy(&n, in.data() + sizeof cfg + sizeof sp, sizeof n);
    const size_t nfixed = sp.planner == 2 && sp.fixed_route_len > 0 ? (size_t)sp.fixed_route_len : 0;
    if (n < 0 || n > (1 << 24) || in.size() != head + (size_t)n * 8 + nfixed * 16) { fprintf(stderr, "%s: size does not match its header\n", argv[1]); return 2; }
    std::vector<int64_t> seeds((size_t)n);
    std::vector<double> fixed(nfixed * 2);
    if (n) memcpy(seeds.data(), in.data() + head, (size_t)n * 8);
    if (nfixed) memcpy(fixed.data(), in.data() + head + (size_t)n * 8, nfixed * 16);
    sp.fixed_route = nfixed ? fixed.data() : nullptr;
    if (cfg.n_static < 0 || cfg.n_bears < 0 || cfg.route_cap < 0 || cfg.init_traj_cap < 0) { fprintf(stderr, "negative capacity\n"); return 2; }
    const size_t N = (size_t)n, R = 2 + (size_t)cfg.n_bears;
    std::vector<int32_t> static_rects(N * cfg.n_static * 4), robot_rect(N * R * 4), route_len(N), init_traj_len(N);
    std::vector<float> robot_pos(N * R * 2), init_traj(N * cfg.init_traj_cap * 2);
    std::vector<double> robot_dir(N * R), route(N * cfg.route_cap * 2);
    std::vector<uint8_t> status(N);
    ftl_scenarios out{};
    out.n_scenarios = (int32_t)n;
    out.static_rects = static_rects.data(); out.robot_pos = robot_pos.data(); out.robot_dir = robot_dir.data(); out.robot_rect = robot_rect.data();
    out.route = route.data(); out.route_len = route_len.data(); out.init_traj = init_traj.data(); out.init_traj_len = init_traj_len.data();
    const int rc = ftl_generate_scenarios(&cfg, &sp, seeds.data(), (int32_t)n, argc > 3 ? atoi(argv[3]) : 1, &out, status.data());
    if (rc != FTL_OK) { fprintf(stderr, "ftl_generate_scenarios: %d\n", rc); return 3; }
    FILE* f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    const bool ok = dump(f, static_rects) && dump(f, robot_pos) && dump(f, robot_dir) && dump(f, robot_rect) && dump(f, route) &&
                    dump(f, route_len) && dump(f, init_traj) && dump(f, init_traj_len) && dump(f, status);
    if (fclose(f) != 0 || !ok) { fprintf(stderr, "%s: short write\n", argv[2]); return 2; }
    return 0;
}
