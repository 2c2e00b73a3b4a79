// TEST INFRASTRUCTURE ONLY: a stand-alone program that runs the host-only procedures of csrc/hip/launch_buffers_plan.h with the scripted Ops of
// launch_buffers_plan_record.h -- the invariant sweep of tests/test_launch_buffers_plan.py (lb_record::sweep) and ADVICE round 6's sequence -- to be built
// with the host sanitizers and run by hand on a machine without a GPU (no test runs it):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Wno-attributes -o /tmp/launch_buffers_plan_check launch_buffers_plan_check.cpp && /tmp/launch_buffers_plan_check
// Exit status 0: every case of the sweep keeps the plan's invariants, the sequence ends with a cache for every pool slot, and no sanitizer report.
#include "hip_emu.h"
#include "../../tray_rust_amd/csrc/hip/kernels.hip"
#include "../../tray_rust_amd/csrc/hip/wavefront_plan.h"
#include "../../tray_rust_amd/csrc/hip/launch_buffers_plan.h"
#include "launch_buffers_plan_record.h"

namespace trayh { void set_error(const std::string&) {} }

int main() {
    int bad = 0;
    uint64_t failures = 0;
    std::string first;
    const uint64_t cases = lb_record::sweep(&failures, &first);
    std::printf("sweep: %llu cases, %llu broke an invariant%s%s\n", (unsigned long long)cases, (unsigned long long)failures, failures ? ": " : "", first.c_str());
    bad += failures != 0 || cases == 0;
    {   // ADVICE round 6, second finding: a per-path launch leaves a cache of 32 768 lanes, tray_scene_set_wavefront frees the pool, a table launch allocates
        // a pool of 131 072 slots, the table goes off -- the next launch has a cache for all of them
        setenv("TRAYHIP_XF_CACHE_BYTES", std::to_string((uint64_t)4 * TR_XF_REC * 4 * 32768).c_str(), 1);
        lb_record::Session s;
        s.f = tr_lbplan::Facts{64u, 1024u, true, true, 4u, 8192u, 24u, 5u, true, 0u, 0};
        bad += s.frame() != TRAY_OK || s.prepare(65536u) != TRAY_OK || s.st.pool_slots != 32768u || s.st.cache_lanes != 32768u;
        s.set_wavefront(131072u);
        s.f.table_req = 1;
        bad += s.prepare(65536u) != TRAY_OK || s.st.pool_slots != 131072u || !s.st.last_used_table || s.st.cache_lanes != 32768u;
        s.f.table_req = 0;
        bad += s.prepare(65536u) != TRAY_OK || s.st.last_used_table || !s.launchable().empty() || !s.owned().empty();
        std::printf("ADVICE round 6: %u pool slots, a cache of %u lanes%s\n", s.st.pool_slots, s.st.cache_lanes, s.st.cache_lanes >= s.st.pool_slots ? "" : " WRONG");
        unsetenv("TRAYHIP_XF_CACHE_BYTES");
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
