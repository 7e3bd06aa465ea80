// Stand-alone driver of the device build's host definition for the sanitizer run of tests/test_device_build_cpu.py: compiled
// together with path_tracing_amd/csrc/scene_build.cpp under -fsanitize=address,undefined, it reads the records a test wrote
// (int32 counts of lights, spheres, triangles; then the three record arrays, layouts of include/hpt.h), calls
// hpt::lbvh_host_scene, prints the size of what came out and writes the exported arrays (qnodes, then tris) to OUT.
#include "hpt_scene.h"

#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char **argv){
    if(argc != 3){ fprintf(stderr, "usage: lbvh_check RECORDS OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if(!f){ perror(argv[1]); return 2; }
    int32_t n[3];
    if(fread(n, sizeof(int32_t), 3, f) != 3 || n[0] < 0 || n[1] < 0 || n[2] < 0){ fprintf(stderr, "bad header\n"); return 2; }
    std::vector<unsigned char> lights((size_t) n[0] * 144), spheres((size_t) n[1] * 100), tris((size_t) n[2] * 120);
    if(fread(lights.data(), 1, lights.size(), f) != lights.size() || fread(spheres.data(), 1, spheres.size(), f) != spheres.size()
       || fread(tris.data(), 1, tris.size(), f) != tris.size()){ fprintf(stderr, "short file\n"); return 2; }
    fclose(f);
    hpt::HostScene hs;
    const char *err = hpt::lbvh_host_scene(lights.data(), n[0], spheres.data(), n[1], tris.data(), n[2], hs);
    if(err && *err){ fprintf(stderr, "lbvh_host_scene: %s\n", err); return 1; }
    if(hs.qnodes.size() != hs.nodes.size() || (int) hs.tris.size() != n[2] || hs.wide_src.size() != hs.wnodes.size() * 4
       || hs.level_begin.empty() || hs.level_begin.back() != hs.nodes.size()){ fprintf(stderr, "sizes disagree\n"); return 1; }
    // a refit of the tree to its own records leaves every byte
    std::vector<hpt::QBvhNode> q(hs.qnodes.begin(), hs.qnodes.end());
    std::vector<hpt::DevTriangle> t(hs.tris.begin(), hs.tris.end());
    err = hpt::refit_host_scene(hs, tris.data(), n[2]);
    if(err && *err){ fprintf(stderr, "refit_host_scene: %s\n", err); return 1; }
    if(memcmp(q.data(), hs.qnodes.data(), q.size() * sizeof(hpt::QBvhNode)) != 0 ||
       (!t.empty() && memcmp(t.data(), hs.tris.data(), t.size() * sizeof(hpt::DevTriangle)) != 0)){
        fprintf(stderr, "a refit to the build's own records changed bytes\n"); return 1;
    }
    FILE *o = fopen(argv[2], "wb");
    if(!o){ perror(argv[2]); return 2; }
    fwrite(hs.qnodes.data(), sizeof(hpt::QBvhNode), hs.qnodes.size(), o);
    if(!hs.tris.empty()) fwrite(hs.tris.data(), sizeof(hpt::DevTriangle), hs.tris.size(), o);
    fclose(o);
    printf("nodes=%zu tris=%zu depth=%d wide=%zu wide_depth=%d\n", hs.qnodes.size(), hs.tris.size(), hs.bvh_depth, hs.wnodes.size(), hs.wide_depth);
    return 0;
}
