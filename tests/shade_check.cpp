// Stand-alone driver of the two CPU oracles on the hostile material and light records of tests/shade_cases.py, for
// tests/test_shade_cases_cpu.py: compiled together with oracle/pt_oracle.cpp and tests/ppm_oracle.cpp (-ffp-contract=off,
// address and undefined-behaviour sanitizers, float-cast-overflow included), it renders every case of its input file with
// the path-tracing oracle in its default mode and in the replay mode that is pinned to the reference's kernel, and with the
// photon-mapping oracle, and prints one FNV-1a checksum of the image bytes per render.  The oracles are the yardstick of
// the GPU tests: a clean exit here says that their answer on NaN, infinite, negative and denormal fields is defined
// behaviour, and equal checksums say that the sanitized build computes what the shared libraries compute.
//
// usage: shade_check INPUT
// INPUT   int32 ncases; per case: int32 nl, ns, nt, W, H, depth, spp, spl; uint64 seed; float smin[3], smax[3] (the photon
//         grid's bounds); one camera record (84 bytes); the three record arrays (layouts of include/hpt.h)
// stdout  per case one line: case K pt=<hex> replay=<hex> ppm=<hex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
// oracle/pt_oracle.cpp
struct OraclePtOpts {
    uint64_t seed;
    int rng_mode, trig_mode, sample_offset, x0, y0, x1, y1, threads, glass_shadow_opaque, max_delta, output_sum, russian_roulette,
        ball_draw_reversed, rcp_nudge_ulps, rcp_nudge_mask, bsdf_draw_reversed;
};
struct OraclePtStats {
    uint64_t samples, closest_rays, shadow_rays, bounces, delta_bounces, tri_tests, sphere_tests, boxes_closest, tris_closest, boxes_shadow,
        tris_shadow, max_delta_run;
};
int oracle_pt_render(const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt, const void *camera, float *image,
                     int W, int H, int max_depth, int spp, const OraclePtOpts *opts, OraclePtStats *stats_out);
// tests/ppm_oracle.cpp
int ppm_oracle_render(const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt, const void *camera, int W, int H,
                      int eye_depth, int light_depth, int spp, int spl, float radius, const float *smin, const float *smax, uint64_t seed,
                      int sample_offset, int max_delta, int output_sum, int brute, float *image, uint64_t *stats_out, float *flux_out,
                      uint64_t *work_out, float *pos_out);
}

static uint64_t fnv1a(const void *p, size_t n){
    const unsigned char *b = (const unsigned char *) p;
    uint64_t h = 0xCBF29CE484222325ull;
    for(size_t i = 0; i < n; ++i){ h ^= b[i]; h *= 0x100000001B3ull; }
    return h;
}

static bool read_exact(FILE *f, void *p, size_t n){ return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv){
    if(argc != 2){ fprintf(stderr, "usage: shade_check INPUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if(!f){ perror(argv[1]); return 2; }
    int32_t ncases;
    if(fread(&ncases, 4, 1, f) != 1 || ncases < 0){ fprintf(stderr, "bad header\n"); return 2; }
    for(int k = 0; k < ncases; ++k){
        int32_t n[8];
        uint64_t seed;
        float bounds[6];
        unsigned char cam[84];
        if(fread(n, 4, 8, f) != 8 || fread(&seed, 8, 1, f) != 1 || fread(bounds, 4, 6, f) != 6 || fread(cam, 1, 84, f) != 84){ fprintf(stderr, "short file\n"); return 2; }
        for(int i = 0; i < 8; ++i) if(n[i] < 0 || n[i] > (1 << 20)){ fprintf(stderr, "bad case header\n"); return 2; }
        const int nl = n[0], ns = n[1], nt = n[2], W = n[3], H = n[4], depth = n[5], spp = n[6], spl = n[7];
        if(W < 1 || H < 1 || spp < 1 || W > 4096 || H > 4096){ fprintf(stderr, "bad image shape\n"); return 2; }
        std::vector<unsigned char> lights((size_t) nl * 144), spheres((size_t) ns * 100), tris((size_t) nt * 120);
        if(!read_exact(f, lights.data(), lights.size()) || !read_exact(f, spheres.data(), spheres.size()) || !read_exact(f, tris.data(), tris.size())){
            fprintf(stderr, "short file\n"); return 2;
        }
        std::vector<float> img((size_t) W * H * 3);
        uint64_t sums[3];
        for(int mode = 0; mode < 2; ++mode){
            OraclePtOpts o; memset(&o, 0, sizeof o);
            o.seed = seed; o.max_delta = 64;
            if(mode == 1){ o.rng_mode = 1; o.trig_mode = 1; o.glass_shadow_opaque = 1; o.ball_draw_reversed = 1; o.bsdf_draw_reversed = 1; o.threads = 1; }
            OraclePtStats st;
            std::fill(img.begin(), img.end(), 0.0f);
            int rc = oracle_pt_render(lights.data(), nl, spheres.data(), ns, tris.data(), nt, cam, img.data(), W, H, depth, spp, &o, &st);
            if(rc != 0){ fprintf(stderr, "case %d: oracle_pt_render failed rc=%d\n", k, rc); return 1; }
            sums[mode] = fnv1a(img.data(), img.size() * 4);
        }
        uint64_t st5[5];
        std::fill(img.begin(), img.end(), 0.0f);
        int rc = ppm_oracle_render(lights.data(), nl, spheres.data(), ns, tris.data(), nt, cam, W, H, depth, 4, 1, spl, 0.05f, bounds, bounds + 3, 11, 0, 0, 0, 0,
                                   img.data(), st5, nullptr, nullptr, nullptr);
        if(rc != 0){ fprintf(stderr, "case %d: ppm_oracle_render failed rc=%d\n", k, rc); return 1; }
        sums[2] = fnv1a(img.data(), img.size() * 4);
        printf("case %d pt=%016llx replay=%016llx ppm=%016llx\n", k, (unsigned long long) sums[0], (unsigned long long) sums[1], (unsigned long long) sums[2]);
    }
    fclose(f);
    return 0;
}
