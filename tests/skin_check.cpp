// Stand-alone driver of the host skin for the sanitizer run of tests/test_skin_cpu.py: compiled together with
// path_tracing_amd/csrc/scene_build.cpp under -fsanitize=address,undefined, it reads what a test wrote (int32 counts of
// lights, spheres, triangles, bones and skins; the three record arrays, layouts of include/hpt.h; four int32 bones and four
// float weights per corner; then 12 floats per bone and skin), builds the base scene with hpt::build_host_scene and, for
// every skin IN TURN, skins the base records with hpt::skin_host_records -- into a second array and, on a copy, in place --
// and refits the ONE HostScene to them with hpt::refit_host_scene, as a live handle is skinned.  After the build and after
// every skin it prints the size of the tree and a digest of the records and of the tree's arrays.
#include "hpt_scene.h"

#include <cstdio>
#include <cstring>
#include <vector>

static unsigned long long fnv(const void *p, size_t n, unsigned long long h = 0xcbf29ce484222325ull){
    const unsigned char *b = (const unsigned char *) p;
    for(size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

static void report(int step, const hpt::HostScene &hs, unsigned long long dead, const std::vector<unsigned char> &records){
    unsigned long long g = fnv(hs.qorigin, sizeof hs.qorigin);
    g = fnv(hs.qscale, sizeof hs.qscale, g);
    printf("step=%d nodes=%zu tris=%zu depth=%d dead=%llu records_fnv=%llx qnodes_fnv=%llx tris_fnv=%llx grid_fnv=%llx\n", step, hs.qnodes.size(),
           hs.tris.size(), hs.bvh_depth, dead, fnv(records.data(), records.size()), fnv(hs.qnodes.data(), hs.qnodes.size() * sizeof(hpt::QBvhNode)),
           fnv(hs.tris.data(), hs.tris.size() * sizeof(hpt::DevTriangle)), g);
}

int main(int argc, char **argv){
    if(argc != 2){ fprintf(stderr, "usage: skin_check RECORDS\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if(!f){ perror(argv[1]); return 2; }
    int32_t n[5];
    if(fread(n, sizeof(int32_t), 5, f) != 5 || n[0] < 0 || n[1] < 0 || n[2] < 0 || n[3] < 1 || n[4] < 0){ fprintf(stderr, "bad header\n"); return 2; }
    std::vector<unsigned char> lights((size_t) n[0] * 144), spheres((size_t) n[1] * 100), tris((size_t) n[2] * 120);
    std::vector<int32_t> bone((size_t) n[2] * 12);
    std::vector<float> weight((size_t) n[2] * 12);
    if(fread(lights.data(), 1, lights.size(), f) != lights.size() || fread(spheres.data(), 1, spheres.size(), f) != spheres.size()
       || fread(tris.data(), 1, tris.size(), f) != tris.size() || fread(bone.data(), 4, bone.size(), f) != bone.size()
       || fread(weight.data(), 4, weight.size(), f) != weight.size()){ fprintf(stderr, "short file\n"); return 2; }
    hpt::HostScene hs;
    const char *err = hpt::build_host_scene(lights.data(), n[0], spheres.data(), n[1], tris.data(), n[2], hs);
    if(err && *err){ fprintf(stderr, "build_host_scene: %s\n", err); return 1; }
    report(-1, hs, 0, tris);
    std::vector<unsigned char> skinned(tris.size()), in_place;
    std::vector<float> xforms((size_t) n[3] * 12);
    char msg[200];
    for(int s = 0; s < n[4]; ++s){
        if(fread(xforms.data(), 4, xforms.size(), f) != xforms.size()){ fprintf(stderr, "short file\n"); return 2; }
        err = hpt::skin_host_records(tris.data(), n[2], bone.data(), weight.data(), xforms.data(), n[3], skinned.data(), msg, sizeof msg);
        if(err && *err){ fprintf(stderr, "skin_host_records: %s\n", err); return 1; }
        in_place = tris;
        err = hpt::skin_host_records(in_place.data(), n[2], bone.data(), weight.data(), xforms.data(), n[3], in_place.data(), msg, sizeof msg);
        if(err && *err){ fprintf(stderr, "skin_host_records in place: %s\n", err); return 1; }
        if(in_place != skinned){ fprintf(stderr, "skin %d: skinning in place gives other bytes\n", s); return 1; }
        err = hpt::check_triangle_update(tris.data(), n[2], skinned.data(), n[2], msg, sizeof msg);
        if(err && *err){ fprintf(stderr, "check_triangle_update: %s\n", err); return 1; }
        uint64_t dead = 0;
        err = hpt::refit_host_scene(hs, skinned.data(), n[2], &dead);
        if(err && *err){ fprintf(stderr, "refit_host_scene: %s\n", err); return 1; }
        report(s, hs, (unsigned long long) dead, skinned);
    }
    fclose(f);
    return 0;
}
