// TEST INFRASTRUCTURE ONLY: a stand-alone program that runs the host-only functions of csrc/hip/scene_plan.h on the hand-built flat scenes of
// tests/test_scene_plan.py, to be built with the host sanitizers and run by hand on a machine without a GPU (no test runs it):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Wno-attributes -o /tmp/scene_plan_check scene_plan_check.cpp && /tmp/scene_plan_check
// Exit status 0: every plan has the expected stack depth and layout, and no sanitizer report.
#include "hip_emu.h"
#include "../../tray_rust_amd/csrc/hip/kernels.hip"
#include "../../tray_rust_amd/csrc/hip/scene_plan.h"

namespace trayh { void set_error(const std::string&) {} }

namespace {

// spheres and meshes under a BVH<Instance>; every mesh is a chain tree of the given depth (0: the instance is a sphere)
struct HandBuilt {
    TrayFlatScene f;
    std::vector<TrayInstance> instances;
    std::vector<TrayBvhNode> top, mesh_nodes;
    std::vector<TrayMesh> meshes;
    std::vector<uint32_t> order;
    HandBuilt(std::vector<TrayBvhNode> top_nodes, const std::vector<uint32_t>& mesh_depth_of_instance) : top(std::move(top_nodes)) {
        std::memset(&f, 0, sizeof f);
        instances.resize(mesh_depth_of_instance.size());
        std::memset(instances.data(), 0, instances.size() * sizeof(TrayInstance));
        uint32_t tri0 = 0;
        for (size_t i = 0; i < instances.size(); ++i) {
            const uint32_t d = mesh_depth_of_instance[i];
            order.push_back((uint32_t)i);
            instances[i].geom_type = d ? TRAY_GEOM_MESH : TRAY_GEOM_SPHERE;
            if (!d) continue;
            instances[i].mesh_id = (uint32_t)meshes.size();
            meshes.push_back(TrayMesh{(uint32_t)mesh_nodes.size(), 2u * d - 1u, tri0, d});
            for (uint32_t level = 0; level + 1 < d; ++level) { mesh_nodes.push_back(node(2u * level + 2u, 0)); mesh_nodes.push_back(node(level, 1)); }
            mesh_nodes.push_back(node(d - 1u, 1));
            tri0 += d;
        }
        f.n_instances = (uint32_t)instances.size(); f.instances = instances.data();
        f.n_top_nodes = (uint32_t)top.size(); f.top_nodes = top.data();
        f.n_top_order = (uint32_t)order.size(); f.top_order = order.data();
        f.n_meshes = (uint32_t)meshes.size(); f.meshes = meshes.data();
        f.n_mesh_nodes = (uint32_t)mesh_nodes.size(); f.mesh_nodes = mesh_nodes.data();
        f.n_tris = tri0;
    }
    static TrayBvhNode node(uint32_t offset, uint16_t count) {
        TrayBvhNode n;
        std::memset(&n, 0, sizeof n);
        n.offset = offset; n.count = count;
        return n;
    }
};

int check(const char* what, HandBuilt& h, uint32_t want_depth, bool want_coop) {
    tr_plan::ScenePlan p;
    tr_plan::plan_motion(&h.f, p);
    tr_plan::plan_materials(std::vector<DevMaterial>(), p);
    tr_plan::plan_light_filter(&h.f, p);
    p.wavefront = tr_plan::wavefront(&h.f, true, p);
    tr_plan::plan_stacks(&h.f, tr_plan::mesh_depths(&h.f), p);
    int bad = p.depth != want_depth;
    for (int film_rows = 0; film_rows < 2; ++film_rows) {
        tr_plan::plan_lds(&h.f, true, film_rows != 0, p);
        bad += (p.coop_offset != 0u) != want_coop || (film_rows ? p.win_offset != 0u : p.win_offset * 4u + 4u * WIN_PLANE * 4u != p.stack_bytes);
    }
    std::printf("%-28s depth %2u (expected %2u), coop_offset %5u, %u B%s\n", what, p.depth, want_depth, p.coop_offset, p.stack_bytes, bad ? "  WRONG" : "");
    return bad;
}

}  // namespace

int main() {
    const TrayBvhNode root = HandBuilt::node(2, 0), left3 = HandBuilt::node(0, 3), right1 = HandBuilt::node(3, 1);
    int bad = 0;
    HandBuilt one({HandBuilt::node(0, 1)}, {1});
    bad += check("leaf under leaf", one, 4, true);
    HandBuilt spheres({root, left3, right1}, {0, 0, 0, 0});
    bad += check("three spheres and one", spheres, 5, false);
    for (uint32_t d : {1u, 2u, 3u, 7u, 40u}) {
        HandBuilt m({root, left3, right1}, {d, 0, 0, 0});
        bad += check("mesh on the first of three", m, std::max(d + 1u, std::max(4u, 3u + d) + 1u), d <= TR_COOP_MAX_TRIS);
    }
    tr_plan::Refusal no = tr_plan::refuse(&one.f, true);   // (ABI version 0: refused before anything is read)
    bad += no.rc != TRAY_E_INVALID || no.msg != "tray_scene_create: ABI version mismatch";
    return bad ? 1 : 0;
}
