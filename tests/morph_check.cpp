// Stand-alone driver of the host morph for the sanitizer run of tests/test_morph_cpu.py: compiled together with
// path_tracing_amd/csrc/scene_build.cpp under -fsanitize=address,undefined, it reads what a test wrote (int32 counts of
// lights, spheres, triangles, targets, entries and morphs; the three record arrays, layouts of include/hpt.h; target_begin,
// entry_corner and entry_delta; then one float per target and morph), builds the base scene with hpt::build_host_scene and,
// for every morph IN TURN, morphs the base records with hpt::morph_host_records -- into a second array and, on a copy, in
// place -- holds them to the per-corner form the device walks (hpt::transpose_morphs, hpt::morph_vertex_host) and refits
// the ONE HostScene to them with hpt::refit_host_scene, as a live handle is morphed.  After the build and after every morph
// it prints the size of the tree and a digest of the records and of the tree's arrays.
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
    if(argc != 2){ fprintf(stderr, "usage: morph_check RECORDS\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if(!f){ perror(argv[1]); return 2; }
    int32_t n[6];
    if(fread(n, sizeof(int32_t), 6, f) != 6 || n[0] < 0 || n[1] < 0 || n[2] < 0 || n[3] < 1 || n[4] < 0 || n[5] < 0){ fprintf(stderr, "bad header\n"); return 2; }
    const int nt = n[2], num_targets = n[3], num_entries = n[4];
    std::vector<unsigned char> lights((size_t) n[0] * 144), spheres((size_t) n[1] * 100), tris((size_t) nt * 120);
    std::vector<int32_t> begin((size_t) num_targets + 1), corner((size_t) num_entries);
    std::vector<float> delta((size_t) num_entries * 3);
    if(fread(lights.data(), 1, lights.size(), f) != lights.size() || fread(spheres.data(), 1, spheres.size(), f) != spheres.size()
       || fread(tris.data(), 1, tris.size(), f) != tris.size() || fread(begin.data(), 4, begin.size(), f) != begin.size()
       || fread(corner.data(), 4, corner.size(), f) != corner.size() || fread(delta.data(), 4, delta.size(), f) != delta.size()){
        fprintf(stderr, "short file\n"); return 2;
    }
    hpt::HostScene hs;
    const char *err = hpt::build_host_scene(lights.data(), n[0], spheres.data(), n[1], tris.data(), nt, hs);
    if(err && *err){ fprintf(stderr, "build_host_scene: %s\n", err); return 1; }
    report(-1, hs, 0, tris);
    char msg[200];
    err = hpt::check_morphs(begin.data(), corner.data(), delta.data(), num_entries, nt, num_targets, msg, sizeof msg);
    if(err && *err){ fprintf(stderr, "check_morphs: %s\n", err); return 1; }
    std::vector<uint32_t> corner_begin; std::vector<hpt::MorphEntry> entries;
    hpt::transpose_morphs(begin.data(), corner.data(), delta.data(), nt, num_targets, corner_begin, entries);
    if(corner_begin.size() != (size_t) nt * 3 + 1 || corner_begin.back() != (uint32_t) num_entries || entries.size() != (size_t) num_entries){
        fprintf(stderr, "transpose_morphs: wrong sizes\n"); return 1;
    }
    std::vector<unsigned char> morphed(tris.size()), in_place, by_corner;
    std::vector<float> weights((size_t) num_targets);
    for(int s = 0; s < n[5]; ++s){
        if(fread(weights.data(), 4, weights.size(), f) != weights.size()){ fprintf(stderr, "short file\n"); return 2; }
        err = hpt::morph_host_records(tris.data(), nt, begin.data(), corner.data(), delta.data(), num_entries, num_targets, weights.data(),
                                      morphed.data(), msg, sizeof msg);
        if(err && *err){ fprintf(stderr, "morph_host_records: %s\n", err); return 1; }
        in_place = tris;
        err = hpt::morph_host_records(in_place.data(), nt, begin.data(), corner.data(), delta.data(), num_entries, num_targets, weights.data(),
                                      in_place.data(), msg, sizeof msg);
        if(err && *err){ fprintf(stderr, "morph_host_records in place: %s\n", err); return 1; }
        if(in_place != morphed){ fprintf(stderr, "morph %d: morphing in place gives other bytes\n", s); return 1; }
        by_corner = tris;
        for(size_t c = 0; c < (size_t) nt * 3; ++c){
            float v[3]; memcpy(v, by_corner.data() + (c / 3) * 120 + (c % 3) * 12, 12);
            hpt::morph_vertex_host(entries.data() + corner_begin[c], corner_begin[c + 1] - corner_begin[c], weights.data(), v, v);
            memcpy(by_corner.data() + (c / 3) * 120 + (c % 3) * 12, v, 12);
        }
        if(by_corner != morphed){ fprintf(stderr, "morph %d: the per-corner walk gives other bytes\n", s); return 1; }
        err = hpt::check_triangle_update(tris.data(), nt, morphed.data(), nt, msg, sizeof msg);
        if(err && *err){ fprintf(stderr, "check_triangle_update: %s\n", err); return 1; }
        uint64_t dead = 0;
        err = hpt::refit_host_scene(hs, morphed.data(), nt, &dead);
        if(err && *err){ fprintf(stderr, "refit_host_scene: %s\n", err); return 1; }
        report(s, hs, (unsigned long long) dead, morphed);
    }
    fclose(f);
    return 0;
}
