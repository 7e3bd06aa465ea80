// Stand-alone driver of the host refit for the sanitizer run of tests/test_refit_cpu.py: compiled together with
// path_tracing_amd/csrc/scene_build.cpp under -fsanitize=address,undefined, it reads what a test wrote (int32 counts of
// lights, spheres, triangles and steps; the three record arrays, layouts of include/hpt.h; then one triangle array per
// step), builds the base scene with hpt::build_host_scene and refits it to every step IN TURN with hpt::refit_host_scene --
// a chain, as a live handle is updated -- and prints after the build and after every step the size of the tree and a digest
// of its arrays.
#include "hpt_scene.h"

#include <cstdio>
#include <cstring>
#include <vector>

static unsigned long long fnv(const void *p, size_t n, unsigned long long h = 0xcbf29ce484222325ull){
    const unsigned char *b = (const unsigned char *) p;
    for(size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

static void report(int step, const hpt::HostScene &hs, unsigned long long dead){
    unsigned long long g = fnv(hs.qorigin, sizeof hs.qorigin);
    g = fnv(hs.qscale, sizeof hs.qscale, g);
    printf("step=%d nodes=%zu tris=%zu depth=%d wide=%zu dead=%llu qnodes_fnv=%llx tris_fnv=%llx grid_fnv=%llx wnodes_fnv=%llx\n", step, hs.qnodes.size(),
           hs.tris.size(), hs.bvh_depth, hs.wnodes.size(), dead, fnv(hs.qnodes.data(), hs.qnodes.size() * sizeof(hpt::QBvhNode)),
           fnv(hs.tris.data(), hs.tris.size() * sizeof(hpt::DevTriangle)), g, fnv(hs.wnodes.data(), hs.wnodes.size() * sizeof(hpt::WideNode)));
}

int main(int argc, char **argv){
    if(argc != 2){ fprintf(stderr, "usage: refit_check RECORDS\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if(!f){ perror(argv[1]); return 2; }
    int32_t n[4];
    if(fread(n, sizeof(int32_t), 4, f) != 4 || n[0] < 0 || n[1] < 0 || n[2] < 0 || n[3] < 0){ fprintf(stderr, "bad header\n"); return 2; }
    std::vector<unsigned char> lights((size_t) n[0] * 144), spheres((size_t) n[1] * 100), tris((size_t) n[2] * 120);
    if(fread(lights.data(), 1, lights.size(), f) != lights.size() || fread(spheres.data(), 1, spheres.size(), f) != spheres.size()
       || fread(tris.data(), 1, tris.size(), f) != tris.size()){ fprintf(stderr, "short file\n"); return 2; }
    hpt::HostScene hs;
    const char *err = hpt::build_host_scene(lights.data(), n[0], spheres.data(), n[1], tris.data(), n[2], hs);
    if(err && *err){ fprintf(stderr, "build_host_scene: %s\n", err); return 1; }
    report(-1, hs, 0);
    std::vector<unsigned char> next(tris.size());
    for(int s = 0; s < n[3]; ++s){
        if(fread(next.data(), 1, next.size(), f) != next.size()){ fprintf(stderr, "short file\n"); return 2; }
        char msg[200];
        err = hpt::check_triangle_update(tris.data(), n[2], next.data(), n[2], msg, sizeof msg);
        if(err && *err){ fprintf(stderr, "check_triangle_update: %s\n", err); return 1; }
        uint64_t dead = 0;
        err = hpt::refit_host_scene(hs, next.data(), n[2], &dead);
        if(err && *err){ fprintf(stderr, "refit_host_scene: %s\n", err); return 1; }
        report(s, hs, (unsigned long long) dead);
    }
    fclose(f);
    return 0;
}
