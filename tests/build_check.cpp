// Stand-alone driver of the host scene builder for the sanitizer run of tests/test_build_cases_cpu.py: compiled together
// with path_tracing_amd/csrc/scene_build.cpp under -fsanitize=address,undefined, it reads the records a test wrote
// (int32 counts of lights, spheres, triangles; then the three record arrays, layouts of include/hpt.h), calls
// hpt::build_host_scene and prints the size of what came out and a digest of the exported arrays.
#include "hpt_scene.h"

#include <cstdio>
#include <cstring>
#include <vector>

static unsigned long long fnv(const void *p, size_t n){
    unsigned long long h = 0xcbf29ce484222325ull;
    const unsigned char *b = (const unsigned char *) p;
    for(size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

int main(int argc, char **argv){
    if(argc != 2){ fprintf(stderr, "usage: build_check RECORDS\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if(!f){ perror(argv[1]); return 2; }
    int32_t n[3];
    if(fread(n, sizeof(int32_t), 3, f) != 3 || n[0] < 0 || n[1] < 0 || n[2] < 0){ fprintf(stderr, "bad header\n"); return 2; }
    std::vector<unsigned char> lights((size_t) n[0] * 144), spheres((size_t) n[1] * 100), tris((size_t) n[2] * 120);
    if(fread(lights.data(), 1, lights.size(), f) != lights.size() || fread(spheres.data(), 1, spheres.size(), f) != spheres.size()
       || fread(tris.data(), 1, tris.size(), f) != tris.size()){ fprintf(stderr, "short file\n"); return 2; }
    fclose(f);
    hpt::HostScene hs;
    const char *err = hpt::build_host_scene(lights.data(), n[0], spheres.data(), n[1], tris.data(), n[2], hs);
    if(err && *err){ fprintf(stderr, "build_host_scene: %s\n", err); return 1; }
    if(hs.qnodes.size() != hs.nodes.size() || (int) hs.tris.size() != n[2]){ fprintf(stderr, "sizes disagree\n"); return 1; }
    printf("nodes=%zu tris=%zu depth=%d qnodes_fnv=%llx tris_fnv=%llx\n", hs.qnodes.size(), hs.tris.size(), hs.bvh_depth,
           fnv(hs.qnodes.data(), hs.qnodes.size() * sizeof(hpt::QBvhNode)), fnv(hs.tris.data(), hs.tris.size() * sizeof(hpt::DevTriangle)));
    return 0;
}
