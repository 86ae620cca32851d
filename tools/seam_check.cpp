// seam_check.cpp -- the host scaffolding of csrc/snk_seam.hpp on its own, for the host sanitizers: the two id checks at
// their edges, for_variant over supported and unsupported variants, the carve arithmetic of the staging arena at its edges,
// and HostCall without a device, where every HIP call fails (the error paths).  Prints what it saw; exit status 1 if
// anything is not as expected.
//     make -C tools seam_check && tools/seam_check        (a machine WITHOUT a GPU: the HostCall part expects the failures)
#include <climits>
#include <cstdio>
#include <string>
#include <vector>

#include "../bullet-envs_amd/csrc/snk_seam.hpp"

static std::string g_msg;
static int g_bad = 0;

namespace snk {
int api_fail(const char* msg) {      // libsnk.so's is snk_api.hip's; here the message is kept for the check
    g_msg = msg;
    return 1;
}
void* stage_arena(snk_handle*, size_t need) {      // libsnk.so's is the handle's arena; here it fails, as every HIP call does
    void* d = nullptr;
    return hipMalloc(&d, need) == hipSuccess ? d : nullptr;
}
}  // namespace snk

static void expect(const char* what, int rc, int want_rc, const std::string& want_msg) {
    const bool ok = rc == want_rc && (!rc || g_msg == want_msg);
    printf("%s %-34s rc %d  %s\n", ok ? "ok  " : "BAD ", what, rc, rc ? g_msg.c_str() : "");
    if (!ok) g_bad++;
    g_msg.clear();
}

int main() {
    const int E = 4;
    const char* who = "snk_link_states_host";
    // the id checks
    const int32_t in_range[] = {0, E - 1, 0}, minus[] = {0, -1}, over[] = {E, 0}, least[] = {E - 1, INT32_MIN};
    expect("ids: empty list", snk::check_env_ids(who, "env_ids", in_range, 0, E), 0, "");
    expect("ids: no list", snk::check_env_ids(who, "env_ids", nullptr, 3, E), 0, "");
    expect("ids: 0 and n_envs - 1", snk::check_env_ids(who, "env_ids", in_range, 3, E), 0, "");
    expect("ids: -1", snk::check_env_ids(who, "env_ids", minus, 2, E), 1, "snk_link_states_host: env_ids[1] = -1 is outside 0 .. 3");
    expect("ids: n_envs", snk::check_env_ids(who, "env_ids", over, 2, E), 1, "snk_link_states_host: env_ids[0] = 4 is outside 0 .. 3");
    expect("ids: INT32_MIN", snk::check_env_ids("snk_copy_envs_host", "dst_ids", least, 2, E), 1,
           "snk_copy_envs_host: dst_ids[1] = -2147483648 is outside 0 .. 3");
    expect("count: n_envs", snk::check_count_without_ids(who, "n_rows", E, E), 0, "");
    expect("count: n_envs + 1", snk::check_count_without_ids(who, "n_rows", E + 1, E), 1,
           "snk_link_states_host: n_rows 5 without env_ids is more than the handle's 4 envs");
    expect("count: n_images", snk::check_count_without_ids("snk_render_host", "n_images", E + 1, E), 1,
           "snk_render_host: n_images 5 without env_ids is more than the handle's 4 envs");
    // for_variant: 100 n + v2 of the variant that ran
    const int variants[][3] = {{16, 1, 1601}, {16, 0, 1600}, {32, 0, 3200}, {32, 1, snk::kUnsupported}, {8, 0, snk::kUnsupported}};
    for (const auto& v : variants) {
        const int rc = snk::for_variant(v[0], v[1] != 0,
                                        [](auto n, auto v2) { return 100 * decltype(n)::value + (decltype(v2)::value ? 1 : 0); });
        printf("%s for_variant(%d, %d) -> %d\n", rc == v[2] ? "ok  " : "BAD ", v[0], v[1], rc);
        if (rc != v[2]) g_bad++;
    }
    // launch_variant: an unsupported variant launches nothing and is refused in the caller's name
    {
        int ran = 0;
        expect("launch_variant: 8 links", snk::launch_variant("snk_contacts", 8, false, [&](auto, auto) { ran++; }), 1,
               "snk_contacts: unsupported n_modules (16 or 32)");
        if (ran) { printf("BAD  launch_variant ran a launch for an unsupported variant\n"); g_bad++; }
    }
    // stage_carve: offsets in whole 256-byte units, zero-byte entries without room, the total in size_t
    {
        const size_t A = snk::kStageAlign, G = (size_t)1 << 30;
        struct Case { const char* what; std::vector<size_t> bytes, offsets; size_t total; };
        const Case cases[] = {
            {"no entries", {}, {}, 0},
            {"one zero-byte entry", {0}, {0}, 0},
            {"1 byte", {1}, {0}, A},
            {"255, 256, 257 bytes", {A - 1, A, A + 1, 4}, {0, A, 2 * A, 4 * A}, 5 * A},
            {"multiples of 256", {A, 3 * A, 2 * A}, {0, A, 4 * A}, 6 * A},
            {"null entries between", {0, 16, 0, 0, 300, 0}, {0, 0, A, A, A, 3 * A}, 3 * A},
            {"a total beyond 4 GiB", {3 * G + 1, 2 * G, 7}, {0, 3 * G + A, 5 * G + A}, 5 * G + 2 * A},
        };
        for (const Case& k : cases) {
            std::vector<size_t> off(k.bytes.size(), ~(size_t)0);
            const size_t total = snk::stage_carve(k.bytes.data(), k.bytes.size(), off.data());
            const bool ok = total == k.total && off == k.offsets;
            printf("%s stage_carve: %-24s total %zu\n", ok ? "ok  " : "BAD ", k.what, total);
            if (!ok) g_bad++;
        }
    }
    // HostCall with no device: the arena cannot be had, nothing is uploaded or downloaded, the failure is reported once by
    // finish; null host pointers stay null, and a call of nothing but nulls asks for no arena at all
    {
        const float host_in[4] = {1, 2, 3, 4};
        float host_out[4] = {0, 0, 0, 0};
        snk::HostCall nulls(nullptr);
        const auto none = nulls.in(static_cast<const float*>(nullptr), sizeof(host_in));
        const auto none_out = nulls.out(static_cast<float*>(nullptr), sizeof(host_out));
        const bool fresh = nulls.stage() && !static_cast<const float*>(none) && !static_cast<float*>(none_out);
        snk::HostCall c(nullptr);
        const auto d_in = c.in(host_in, sizeof(host_in));
        const auto d_out = c.out(host_out, sizeof(host_out));
        const auto d_both = c.inout(host_out, sizeof(host_out));
        const bool refused = fresh && !c.stage() && !static_cast<const float*>(d_in) && !static_cast<float*>(d_out) &&
                             !static_cast<float*>(d_both);
        const int rc = c.finish("snk_seam_check");
        const bool ok = refused && rc == 1 && g_msg.rfind("snk_seam_check: ", 0) == 0 && g_msg.size() > 16 && host_out[0] == 0.f;
        printf("%s HostCall without a device         rc %d  %s\n", ok ? "ok  " : "BAD ", rc, g_msg.c_str());
        if (!ok) g_bad++;
    }
    printf("%s\n", g_bad ? "FAILED" : "all as expected");
    return g_bad ? 1 : 0;
}
