// Stand-alone driver of the host tree cost for the sanitizer run of tests/test_rebuild_cpu.py: compiled together with
// path_tracing_amd/csrc/scene_build.cpp under -fsanitize=address,undefined, it reads the records a test wrote (int32 counts of
// lights, spheres, triangles and steps; the three record arrays, layouts of include/hpt.h; then per step one more triangle
// array), builds, and prints the cost of the builder's tree (step -1) and of the tree refitted to every step's records --
// hpt::tree_cost_sums_host and hpt::tree_cost_compose, which are what hpt_bvh_cost_host calls.  Doubles as their 64 bits.
#include "hpt_scene.h"
#include "../../include/hpt.h"

#include <cstdio>
#include <cstring>
#include <vector>

static void print_cost(int step, const hpt::HostScene &hs){
    hpt_tree_cost c;
    hpt::tree_cost_sums_host(hs.qnodes.data(), (uint32_t) hs.qnodes.size(), c);
    hpt::tree_cost_compose(hs.qscale, c);
    unsigned long long d[3];
    memcpy(&d[0], &c.box_visits, 8); memcpy(&d[1], &c.tri_tests, 8); memcpy(&d[2], &c.sah, 8);
    printf("step=%d inner_children=%llu leaf_children=%llu empty_children=%llu leaf_slots=%llu inner_xy=%llu inner_yz=%llu inner_zx=%llu "
           "leaf_xy=%llu leaf_yz=%llu leaf_zx=%llu rx=%u ry=%u rz=%u num_nodes=%u box_visits=%llx tri_tests=%llx sah=%llx\n", step,
           (unsigned long long) c.inner_children, (unsigned long long) c.leaf_children, (unsigned long long) c.empty_children,
           (unsigned long long) c.leaf_slots, (unsigned long long) c.inner_xy, (unsigned long long) c.inner_yz, (unsigned long long) c.inner_zx,
           (unsigned long long) c.leaf_xy, (unsigned long long) c.leaf_yz, (unsigned long long) c.leaf_zx, c.root_extent[0], c.root_extent[1],
           c.root_extent[2], c.num_nodes, d[0], d[1], d[2]);
}

int main(int argc, char **argv){
    if(argc != 2){ fprintf(stderr, "usage: cost_check RECORDS\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if(!f){ perror(argv[1]); return 2; }
    int32_t n[4];
    if(fread(n, sizeof(int32_t), 4, f) != 4 || n[0] < 0 || n[1] < 0 || n[2] < 0 || n[3] < 0){ fprintf(stderr, "bad header\n"); return 2; }
    std::vector<unsigned char> lights((size_t) n[0] * 144), spheres((size_t) n[1] * 100), tris((size_t) n[2] * 120), moved(tris.size());
    if(fread(lights.data(), 1, lights.size(), f) != lights.size() || fread(spheres.data(), 1, spheres.size(), f) != spheres.size()
       || fread(tris.data(), 1, tris.size(), f) != tris.size()){ fprintf(stderr, "short file\n"); return 2; }
    hpt::HostScene hs;
    const char *err = hpt::build_host_scene(lights.data(), n[0], spheres.data(), n[1], tris.data(), n[2], hs);
    if(err && *err){ fprintf(stderr, "build_host_scene: %s\n", err); return 1; }
    print_cost(-1, hs);
    for(int s = 0; s < n[3]; ++s){
        if(fread(moved.data(), 1, moved.size(), f) != moved.size()){ fprintf(stderr, "short file\n"); return 2; }
        err = hpt::refit_host_scene(hs, moved.data(), n[2]);
        if(err && *err){ fprintf(stderr, "refit_host_scene: %s\n", err); return 1; }
        print_cost(s, hs);
    }
    fclose(f);
    return 0;
}
