// Stand-alone driver of the bounded device build's host definition for the sanitizer run of tests/test_bounded_build_cpu.py:
// compiled together with path_tracing_amd/csrc/scene_build.cpp under -fsanitize=address,undefined, it generates a few scenes
// (no input), runs hpt::lbvh_bounded_host_scene on each at 0 and at depths from need to 30 (every third for the larger scenes), and checks what
// the definition promises: at most D levels, the unbounded tree's bytes where no node was forced, every triangle in one leaf
// slot, and the refusal below need.  One line per scene; exit code 0 when all held.
#include "hpt_scene.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Tri { float v[9]; float old_mat[13]; float base[3], roughness, metallic, eta; int32_t type, id; };
static_assert(sizeof(Tri) == 120, "the triangle record of include/hpt.h");

uint32_t g_state = 12345u;
float rnd(){ g_state = g_state * 1664525u + 1013904223u; return (float) (g_state >> 8) * (1.0f / 16777216.0f); }

// n small triangles; kind 0: uniform in the unit cube; 1: centres in the cells 2^k of one axis each, whose keys are powers of two (a radix tree of some 60 levels); 2: all equal;
// 3: uniform with every seventh record not finite
std::vector<Tri> scene(int n, int kind){
    std::vector<Tri> t((size_t) n);
    for(int i = 0; i < n; ++i){
        Tri &r = t[(size_t) i];
        memset(&r, 0, sizeof r);
        float c[3] = { rnd(), rnd(), rnd() };
        if(kind == 1){ const int k = (i + 61) % 63; c[0] = c[1] = c[2] = std::ldexp(0.5f, -21); c[k % 3] = std::ldexp((float) (1u << (k / 3)) + 0.5f, -21); }
        if(kind == 2){ c[0] = c[1] = c[2] = 0.5f; }
        const float h = kind == 1 ? std::ldexp(1.0f, -24) : 0.01f;
        const float p[9] = { c[0] - h, c[1] - h, c[2], c[0] + h, c[1] - h, c[2], c[0], c[1] + h, c[2] };
        memcpy(r.v, p, sizeof p);
        if(kind == 3 && i % 7 == 3) r.v[4] = i % 2 ? NAN : INFINITY;
        r.base[0] = r.base[1] = r.base[2] = 0.7f; r.roughness = 1.0f; r.id = i;
    }
    if(kind == 1 && n >= 2){     // two triangles that fix the live box to the unit cube
        const float a[9] = { 0, 0, 0, 1, 0, 0, 0, 1, 0 }, b[9] = { 1, 1, 1, 0, 1, 1, 1, 0, 1 };
        memcpy(t[0].v, a, sizeof a); memcpy(t[1].v, b, sizeof b);
    }
    return t;
}

bool leaves_cover(const hpt::HostScene &hs, int nt){
    std::vector<int> seen((size_t) nt, 0);
    for(const hpt::BvhNode &nd : hs.nodes)
        for(uint32_t c : { nd.left, nd.right }){
            if(c == hpt::kEmptyChild || !(c & hpt::kLeafFlag)) continue;
            const uint32_t first = (c & ~hpt::kLeafFlag) >> 3, count = (c & 7u) + 1u;
            for(uint32_t k = 0; k < count; ++k){ if(first + k >= (uint32_t) nt) return false; seen[first + k] += 1; }
        }
    for(int s : seen) if(s != 1) return false;
    return true;
}

} // namespace

int main(){
    const int sizes[] = { 0, 1, 2, 3, 4, 5, 7, 64, 257, 1000 };
    int bad = 0;
    for(int kind = 0; kind < 4; ++kind)
        for(int n : sizes){
            std::vector<Tri> t = scene(n, kind);
            hpt::HostScene plain;
            const char *err = hpt::lbvh_host_scene(nullptr, 0, nullptr, 0, t.data(), n, plain);
            if(err && *err){ fprintf(stderr, "lbvh_host_scene: %s\n", err); return 1; }
            const int need = hpt::lbvh_need(n);
            uint32_t forced_at_0 = 0; int depth_at_0 = 0;
            for(int D = 0; D <= hpt::kMaxBvhDepth; D = D == 0 ? need : D + (n > 100 ? 3 : 1)){
                hpt::HostScene hs; hpt::BoundedInfo bi;
                err = hpt::lbvh_bounded_host_scene(nullptr, 0, nullptr, 0, t.data(), n, D, hs, bi);
                if(err && *err){ fprintf(stderr, "kind %d n %d D %d: %s\n", kind, n, D, err); return 1; }
                const int eff = D ? D : hpt::kMaxBvhDepth;
                if((int) bi.max_depth != eff || hs.bvh_depth > eff || !leaves_cover(hs, n) || hs.qnodes.size() != hs.nodes.size()
                   || hs.level_begin.back() != hs.nodes.size() || (bi.forced_nodes == 0) != (bi.first_forced_level == 0xFFFFFFFFu)){
                    fprintf(stderr, "kind %d n %d D %d: depth %d, forced %u: a promise broken\n", kind, n, D, hs.bvh_depth, bi.forced_nodes); ++bad;
                }
                if(bi.forced_nodes == 0 && (hs.nodes.size() != plain.nodes.size() || hs.bvh_depth != plain.bvh_depth
                   || memcmp(hs.qnodes.data(), plain.qnodes.data(), hs.qnodes.size() * sizeof(hpt::QBvhNode)) != 0
                   || (n && memcmp(hs.tris.data(), plain.tris.data(), (size_t) n * sizeof(hpt::DevTriangle)) != 0)
                   || hs.wide_depth != plain.wide_depth)){
                    fprintf(stderr, "kind %d n %d D %d: nothing forced, yet not the unbounded tree\n", kind, n, D); ++bad;
                }
                if(bi.forced_nodes == 0 && plain.bvh_depth > eff){ fprintf(stderr, "kind %d n %d D %d: a deeper tree, nothing forced\n", kind, n, D); ++bad; }
                if(D == 0){ forced_at_0 = bi.forced_nodes; depth_at_0 = hs.bvh_depth; }
            }
            if(need > 1){
                hpt::HostScene hs; hpt::BoundedInfo bi;
                err = hpt::lbvh_bounded_host_scene(nullptr, 0, nullptr, 0, t.data(), n, need - 1, hs, bi);
                if(!err || !*err){ fprintf(stderr, "kind %d n %d: depth %d was not refused\n", kind, n, need - 1); ++bad; }
            }
            printf("kind=%d n=%d need=%d unbounded_depth=%d depth_at_0=%d forced_at_0=%u\n", kind, n, need, plain.bvh_depth, depth_at_0, forced_at_0);
        }
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
