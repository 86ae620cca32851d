// seam_check.cpp -- the host scaffolding of csrc/snk_seam.hpp on its own, for the host sanitizers: the two id checks at
// their edges, for_variant over supported and unsupported variants, and HostCall without a device, where every HIP call
// fails (the error paths and the destructor).  Prints what it saw; exit status 1 if anything is not as expected.
//     make -C tools seam_check && tools/seam_check        (a machine WITHOUT a GPU: the HostCall part expects the failures)
#include <climits>
#include <cstdio>
#include <string>

#include "../bullet-envs_amd/csrc/snk_seam.hpp"

static std::string g_msg;
static int g_bad = 0;

namespace snk {
int api_fail(const char* msg) {      // libsnk.so's is snk_api.hip's; here the message is kept for the check
    g_msg = msg;
    return 1;
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
    // HostCall with no device: nothing can be allocated, nothing is downloaded, the failure is reported once by finish
    {
        const float host_in[4] = {1, 2, 3, 4};
        float host_out[4] = {0, 0, 0, 0};
        snk::HostCall c;
        const float* none = c.in(static_cast<const float*>(nullptr), sizeof(host_in));
        float* none_out = c.out(static_cast<float*>(nullptr), sizeof(host_out));
        const bool fresh = c.ok() && !none && !none_out;
        const float* d_in = c.in(host_in, sizeof(host_in));
        float* d_out = c.out(host_out, sizeof(host_out));
        const bool refused = fresh && !c.ok() && !d_in && !d_out;
        const int rc = c.finish("snk_seam_check");
        const bool ok = refused && rc == 1 && g_msg.rfind("snk_seam_check: ", 0) == 0 && g_msg.size() > 16 && host_out[0] == 0.f;
        printf("%s HostCall without a device         rc %d  %s\n", ok ? "ok  " : "BAD ", rc, g_msg.c_str());
        if (!ok) g_bad++;
    }
    printf("%s\n", g_bad ? "FAILED" : "all as expected");
    return g_bad ? 1 : 0;
}
