// Stand-alone per-ray restatement of k_trace (path_tracing_amd/csrc/pt_trace.hip) on the host, for tests/test_walk_cases_cpu.py:
// compiled together with path_tracing_amd/csrc/scene_build.cpp (-ffp-contract=off, address and undefined-behaviour sanitizers),
// it builds the scene with the library's own host builder, and walks what ONE lane of trace_chunk walks for one ray:
//
//   first launch   the sphere / light-ball loop, then the quantised binary tree (HostScene::qnodes): near / far planes picked by
//                  the sign of the ray's reciprocal, the 1.000002f slack, left_first, the unconditional store at stk[sp], the
//                  `any ? near : top` pop, the node-step budget (a ray with steps >= budget is set aside at the top of the
//                  loop, after the leaf it held), the strict `<` hit update with the ordinal tie;
//   resume walk    from that partial result as the limit, over the four-wide tree (HostScene::wnodes): key = f2u(tn) & ~3 | slot,
//                  nearest by minimum key, the other hit children stacked in slot order, the `any ? near : top` pop, leaves.
//                  The stack is one array here; what the kernel keeps in LDS (levels below kResumeLdsLevels) and what it keeps in
//                  its global-memory column (levels from there on) is told apart by the level number alone, and every access
//                  is classified the way the kernel's three pieces of code make it (fast path, level(), the leaf's pop).
//
// hit_triangle and hit_sphere are pt_device_math.h's, one float operation at a time as written.  The reciprocals are exact;
// with a nudge mask each is moved one float neighbour, up where the axis bit (1 x, 2 y, 4 z) is set and down otherwise (the
// kernel's v_rcp_f32 is within 1 ulp).
//
// usage: walk_check INPUT OUTPUT [NUDGES]      NUDGES: comma-separated, -1 = exact, 0..7 = sign mask; default -1
// INPUT   int32 nl, ns, nt, nsteps, nbudgets; the three record arrays (layouts of include/hpt.h); nbudgets int32 (0 = the
//         unsplit walk alone); then for step -1 (the builder's tree) and every further step: [steps >= 0: nt triangle records,
//         applied with refit_host_scene]; int32 nrays; nrays * 8 words: origin, direction, tmax (floats), kind (uint32: 0 closest
//         hit, 1 any hit; tmax is read by any-hit rays only)
// stdout  one line per step: num_nodes, wnodes, bvh_depth, wide_depth, fits (3 * wide_depth + 2 <= kResumeLdsLevels + kDeepLevels)
// OUTPUT  per nudge, step, ray and budget one record of kWords uint32 (struct Result below), in that nesting order
#include "hpt_scene.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// pt_kernels.h is a device header; tests/test_walk_cases_cpu.py greps these against it and against hpt_scene.h
constexpr int kResumeLdsLevels = 12;
constexpr int kDeepLevels = 48;
constexpr int kStackLevels = 256;            // the walker's own arrays: deeper than anything the kernel may hold, so an overrun is reported, not made

using hpt::kEmptyChild;
using hpt::kLeafFlag;
constexpr uint32_t kDoneCode = 0xFFFFFFFEu;
constexpr uint32_t kHitMiss = 0xFFFFFFFFu, kHitRoundFlag = 0x80000000u;
constexpr float kEps = 1e-4f;

static inline uint32_t f2u(float f){ uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float u2f(uint32_t u){ float f; memcpy(&f, &u, 4); return f; }

struct f3 { float x, y, z; };
static inline f3 mk3(float x, float y, float z){ f3 r; r.x = x; r.y = y; r.z = z; return r; }
static inline f3 operator-(f3 a, f3 b){ return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline float dot3(f3 a, f3 b){ return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline f3 cross3(f3 a, f3 b){ return mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

static bool hit_sphere(f3 ro, f3 rd, f3 center, float radius, float max_dist, float &t){
    f3 oc = ro - center;
    float b = dot3(oc, rd);
    float c = dot3(oc, oc) - radius * radius;
    float h = b * b - c;
    if(h < 0.0f) return false;
    h = sqrtf(h);
    float th = -b - h;
    if(th > kEps && th < max_dist){ t = th; return true; }
    th = -b + h;
    if(th > kEps && th < max_dist){ t = th; return true; }
    return false;
}
static bool hit_triangle(f3 ro, f3 rd, f3 v0, f3 e1, f3 e2, float max_dist, float &t){
    f3 h = cross3(rd, e2);
    float a = dot3(e1, h);
    if(a > -1e-6f && a < 1e-6f) return false;
    float f = 1.0f / a;
    f3 s = ro - v0;
    float u = f * dot3(s, h);
    if(u < 0.0f || u > 1.0f) return false;
    f3 q = cross3(s, e1);
    float v = f * dot3(rd, q);
    if(v < 0.0f || u + v > 1.0f) return false;
    float th = f * dot3(e2, q);
    if(th > kEps && th < max_dist){ t = th; return true; }
    return false;
}

// which of the resume walk's pieces of code a ray went through (Result::paths)
enum : uint32_t {
    kFastStep = 1u,          // a step with sp + 3 < kResumeLdsLevels: every level in LDS
    kSlowLds = 2u,           // level(): a step on the slow path whose stores all went to LDS levels
    kSlowMixed = 4u,         // level(): one step stored to LDS levels and to global ones
    kSlowDeep = 8u,          // level(): a step whose stores all went to global levels (at least one store)
    kTopDeep = 16u,          // level(): the step's `top` was read from a global level
    kMissPopDeep = 32u,      // `any ? near : top` took a top that came from a global level
    kMissPopLds = 64u,       // ... from an LDS level
    kLeafPopDeep = 128u,     // the leaf's pop read deep[...]
    kLeafPopLds = 256u,      // the leaf's pop read stk[...]
    // What a load from a global level decided.  Every node carries how it was come by: entered by a miss pop whose top came
    // from a global level, or by a leaf's pop from deep[] -- itself, or the node under which it was stacked or entered.
    kFinalViaMissDeep = 1u << 16,   // the final closest hit (any hit: the blocker) was found under a node come by the first way
    kFinalViaLeafDeep = 1u << 17,   // ... the second way: a wrong word from that load and the ray's result is another
};
enum : uint32_t { kViaMissDeep = 1u, kViaLeafDeep = 2u };
enum : uint32_t { kSetAside = 1u, kWideOverrun = 2u, kBinaryOverrun = 4u, kSphereBlocked = 8u };

struct Result {
    uint32_t flags;                      // kSetAside | kWideOverrun (sp passed kResumeLdsLevels + kDeepLevels) | kBinaryOverrun (a store at a level >= kStackDepth + 1) | kSphereBlocked
    uint32_t steps1, max_sp1;            // first launch: node steps, highest sp (the store at stk[sp] touches one level more)
    uint32_t part_t, part_prim, part_ord; // what the first launch hands over (closest hit) -- or its result when the ray was not set aside
    uint32_t t, ord, prim;               // final: closest hit (t bits, ordinal, leaf slot or round code) -- any hit: t = 1 when occluded
    uint32_t steps2, max_sp2;            // resume walk
    uint32_t deep_stores, deep_loads;    // stores to / loads from levels >= kResumeLdsLevels
    uint32_t hash_lo, hash_hi;           // FNV-1a over the words in levels [kResumeLdsLevels, max_sp2) when sp first reached max_sp2
    uint32_t paths;
};
constexpr int kWords = 16;
static_assert(sizeof(Result) == kWords * 4, "layout");

struct Ray { f3 ro, rd; float tmax; uint32_t any; };

struct Walk {
    const hpt::HostScene &hs;
    float ix, iy, iz, ox, oy, oz;
    bool nx, ny, nz;                     // the ray runs against the axis: its near plane is a box's upper one
    Walk(const hpt::HostScene &h, const Ray &r, int nudge) : hs(h) {
        float dx = fabsf(r.rd.x) > 1e-20f ? r.rd.x : copysignf(1e-20f, r.rd.x);
        float dy = fabsf(r.rd.y) > 1e-20f ? r.rd.y : copysignf(1e-20f, r.rd.y);
        float dz = fabsf(r.rd.z) > 1e-20f ? r.rd.z : copysignf(1e-20f, r.rd.z);
        ix = 1.0f / dx; iy = 1.0f / dy; iz = 1.0f / dz;
        if(nudge >= 0){
            ix = nextafterf(ix, (nudge & 1) ? INFINITY : -INFINITY);
            iy = nextafterf(iy, (nudge & 2) ? INFINITY : -INFINITY);
            iz = nextafterf(iz, (nudge & 4) ? INFINITY : -INFINITY);
        }
        ox = (hs.qorigin[0] - r.ro.x) * ix; oy = (hs.qorigin[1] - r.ro.y) * iy; oz = (hs.qorigin[2] - r.ro.z) * iz;
        ix *= hs.qscale[0]; iy *= hs.qscale[1]; iz *= hs.qscale[2];
        nx = ix < 0.0f; ny = iy < 0.0f; nz = iz < 0.0f;
    }
    // entry and exit distance of one quantised box: per axis its lower and upper plane
    void slab(uint32_t xl, uint32_t xh, uint32_t yl, uint32_t yh, uint32_t zl, uint32_t zh, float limit, float &tn, float &tf) const {
        const float qnx = (float) (nx ? xh : xl), qfx = (float) (nx ? xl : xh);
        const float qny = (float) (ny ? yh : yl), qfy = (float) (ny ? yl : yh);
        const float qnz = (float) (nz ? zh : zl), qfz = (float) (nz ? zl : zh);
        tn = fmaxf(fmaxf(fmaf(qnx, ix, ox), fmaf(qny, iy, oy)), fmaxf(fmaf(qnz, iz, oz), 0.0f));
        tf = fminf(fminf(fmaf(qfx, ix, ox), fmaf(qfy, iy, oy)), fminf(fmaf(qfz, iz, oz), limit));
    }
};

struct Best { float t; uint32_t prim, ord; };

// the leaf phase of trace_chunk: true when an any-hit ray is blocked
static bool leaf(const hpt::HostScene &hs, const Ray &r, uint32_t cur, Best &b, float &limit){
    const uint32_t first = (cur & 0x7FFFFFFFu) >> 3, cnt = (cur & 7u) + 1u;
    bool blocked = false;
    for(uint32_t k = 0; k < cnt; ++k){
        const hpt::DevTriangle &tr = hs.tris[first + k];
        float t;
        if(hit_triangle(r.ro, r.rd, mk3(tr.v0[0], tr.v0[1], tr.v0[2]), mk3(tr.e1[0], tr.e1[1], tr.e1[2]), mk3(tr.e2[0], tr.e2[1], tr.e2[2]),
                        r.any ? r.tmax : 1e20f, t)){
            if(r.any){
                if(t > 1e-3f && (tr.flags & 1u)) blocked = true;
            } else if(t < b.t || (t == b.t && tr.ordinal < b.ord)){
                b.t = t; b.prim = first + k; b.ord = tr.ordinal; limit = t;
            }
        }
    }
    return blocked;
}

static void walk_ray(const hpt::HostScene &hs, const Ray &r, uint32_t budget, int nudge, Result &out){
    memset(&out, 0, sizeof out);
    Best b{1e20f, kHitMiss, 0xFFFFFFFFu};
    float limit;
    bool blocked = false, finished = false;
    // ---- first launch ----
    if(r.any){
        for(int k = 0; k < hs.num_spheres; ++k){
            const hpt::DevRound &rr = hs.rounds[k];
            float t;
            if(hit_sphere(r.ro, r.rd, mk3(rr.c[0], rr.c[1], rr.c[2]), rr.r, r.tmax, t) && t > 1e-3f && (rr.flags & 1u)){ blocked = true; finished = true; }
        }
        if(blocked) out.flags |= kSphereBlocked;
        limit = r.tmax;
    } else {
        for(int k = 0; k < (int) hs.rounds.size(); ++k){
            const hpt::DevRound &rr = hs.rounds[k];
            float t;
            if(hit_sphere(r.ro, r.rd, mk3(rr.c[0], rr.c[1], rr.c[2]), rr.r, 1e20f, t) && t < b.t){
                b.t = t; b.prim = kHitRoundFlag | (uint32_t) k; b.ord = (uint32_t) k;
            }
        }
        limit = b.t;
    }
    const Walk w(hs, r, nudge);
    uint32_t stk[kStackLevels] = {0u};
    bool set_aside = false;
    if(!finished){
        uint32_t cur = 0u, steps = 0u, max_sp = 0u;
        int sp = 0;
        const uint32_t step_limit = budget != 0u ? budget : 0xFFFFFFFFu;
        for(;;){
            if(budget != 0u && steps >= budget){ set_aside = true; break; }
            while(!(cur & kLeafFlag) && steps < step_limit){
                steps += 1u;
                const hpt::QBvhNode &n = hs.qnodes[cur];
                float ln, lf, rn, rf;
                w.slab(n.plane[0][0][0], n.plane[0][1][0], n.plane[1][0][0], n.plane[1][1][0], n.plane[2][0][0], n.plane[2][1][0], limit, ln, lf);
                w.slab(n.plane[0][0][1], n.plane[0][1][1], n.plane[1][0][1], n.plane[1][1][1], n.plane[2][0][1], n.plane[2][1][1], limit, rn, rf);
                const uint32_t lc = n.left, rc = n.right;
                const bool hl = (ln <= lf * 1.000002f) && (lc != kEmptyChild);
                const bool hr = (rn <= rf * 1.000002f) && (rc != kEmptyChild);
                const bool any = hl || hr, both = hl && hr;
                const bool left_first = hl && (!hr || ln <= rn);
                const uint32_t top = stk[sp > 0 ? sp - 1 : 0];
                if(sp > hpt::kStackDepth) out.flags |= kBinaryOverrun;       // launch_trace gives at most kStackDepth + 1 levels
                stk[sp] = left_first ? rc : lc;
                const uint32_t near = left_first ? lc : rc;
                cur = any ? near : (sp > 0 ? top : kDoneCode);
                sp = any ? sp + (both ? 1 : 0) : (sp > 0 ? sp - 1 : 0);
                if((uint32_t) sp > max_sp) max_sp = (uint32_t) sp;
                if(sp + 1 >= kStackLevels){ fprintf(stderr, "binary stack past the walker's own %d levels\n", kStackLevels); exit(1); }
            }
            if(cur & kLeafFlag){
                if(cur == kDoneCode){ finished = true; break; }
                if(leaf(hs, r, cur, b, limit)){ blocked = true; finished = true; break; }
                if(sp > 0){ --sp; cur = stk[sp]; }
                else { finished = true; break; }
            }
        }
        out.steps1 = steps; out.max_sp1 = max_sp;
    }
    out.part_t = f2u(b.t); out.part_prim = b.prim; out.part_ord = b.ord;
    // ---- resume walk ----
    if(set_aside){
        out.flags |= kSetAside;
        if(!r.any) limit = b.t;                                   // (an any-hit ray restarts with its tmax)
        else limit = r.tmax;
        uint32_t cur = 0u, steps = 0u, max_sp = 0u, paths = 0u, stores = 0u, loads = 0u;
        uint64_t hash = 0ull;
        int sp = 0;
        uint32_t tagstk[kStackLevels] = {0u}, curtag = 0u, final_tag = 0u;
        finished = false;
        while(!finished){
            while(!(cur & kLeafFlag)){
                steps += 1u;
                const uint32_t *q = hs.wnodes[cur].w;
                float tn[4], tf[4];
                for(int c = 0; c < 4; ++c){
                    const int word = c >> 1, sh = (c & 1) * 16;
                    w.slab((q[0 + word] >> sh) & 0xFFFFu, (q[2 + word] >> sh) & 0xFFFFu, (q[4 + word] >> sh) & 0xFFFFu, (q[6 + word] >> sh) & 0xFFFFu,
                           (q[8 + word] >> sh) & 0xFFFFu, (q[10 + word] >> sh) & 0xFFFFu, limit, tn[c], tf[c]);
                }
                uint32_t key[4];
                for(uint32_t c = 0; c < 4u; ++c)
                    key[c] = (tn[c] <= tf[c] * 1.000002f && q[12 + c] != kEmptyChild) ? ((f2u(tn[c]) & ~3u) | c) : 0xFFFFFFFFu;
                uint32_t kmin = key[0];
                for(int c = 1; c < 4; ++c) kmin = key[c] < kmin ? key[c] : kmin;
                const bool any = kmin != 0xFFFFFFFFu;
                const uint32_t near = q[12 + (kmin & 3u)];
                const uint32_t c1 = ~kmin, c2 = c1 - 1u;
                bool e[4];
                for(int c = 0; c < 4; ++c) e[c] = (uint32_t) (key[c] + c1) < c2;      // hit and not the nearest, as the kernel computes it
                const int top_level = sp > 0 ? sp - 1 : 0;
                const uint32_t top = stk[top_level];
                const bool slow = !(sp + 3 < kResumeLdsLevels);
                if(slow && top_level >= kResumeLdsLevels){ loads += 1u; paths |= kTopDeep; }
                int p = sp, lds_stores = 0, deep_stores = 0;
                for(int c = 0; c < 4; ++c) if(e[c]){
                    if(p >= kResumeLdsLevels + kDeepLevels) out.flags |= kWideOverrun;
                    if(p >= kStackLevels){ fprintf(stderr, "four-wide stack past the walker's own %d levels\n", kStackLevels); exit(1); }
                    stk[p] = q[12 + c]; tagstk[p] = curtag;
                    if(p >= kResumeLdsLevels) ++deep_stores; else ++lds_stores;
                    ++p;
                }
                stores += (uint32_t) deep_stores;
                if(!slow) paths |= kFastStep;
                else if(deep_stores && lds_stores) paths |= kSlowMixed;
                else if(deep_stores) paths |= kSlowDeep;
                else paths |= kSlowLds;
                if(!any && sp > 0) paths |= (top_level >= kResumeLdsLevels) ? kMissPopDeep : kMissPopLds;
                if(!any && sp > 0) curtag = tagstk[top_level] | (top_level >= kResumeLdsLevels ? kViaMissDeep : 0u);
                cur = any ? near : (sp > 0 ? top : kDoneCode);
                sp = any ? p : (sp > 0 ? sp - 1 : 0);
                if((uint32_t) sp > max_sp){
                    max_sp = (uint32_t) sp;
                    hash = 0xCBF29CE484222325ull;
                    for(int l = kResumeLdsLevels; l < sp; ++l)
                        for(int byte = 0; byte < 4; ++byte){ hash ^= (stk[l] >> (8 * byte)) & 0xFFu; hash *= 0x100000001B3ull; }
                }
            }
            if(cur == kDoneCode) break;
            const uint32_t prim_before = b.prim;
            const float t_before = b.t;
            if(leaf(hs, r, cur, b, limit)){ blocked = true; final_tag = curtag; break; }
            if(b.prim != prim_before || b.t != t_before) final_tag = curtag;
            if(sp > 0){
                --sp;
                if(sp >= kResumeLdsLevels){ loads += 1u; paths |= kLeafPopDeep; } else paths |= kLeafPopLds;
                cur = stk[sp]; curtag = tagstk[sp] | (sp >= kResumeLdsLevels ? kViaLeafDeep : 0u);
            } else finished = true;
        }
        out.steps2 = steps; out.max_sp2 = max_sp; out.deep_stores = stores; out.deep_loads = loads;
        out.hash_lo = (uint32_t) hash; out.hash_hi = (uint32_t) (hash >> 32);
        out.paths = paths | ((final_tag & kViaMissDeep) ? kFinalViaMissDeep : 0u) | ((final_tag & kViaLeafDeep) ? kFinalViaLeafDeep : 0u);
    }
    if(r.any){ out.t = blocked ? 1u : 0u; out.ord = 0u; out.prim = 0u; }
    else { out.t = f2u(b.t); out.ord = b.ord; out.prim = b.prim; }
}

static bool read_exact(FILE *f, void *p, size_t n){ return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv){
    if(argc != 3 && argc != 4){ fprintf(stderr, "usage: walk_check INPUT OUTPUT [NUDGES]\n"); return 2; }
    std::vector<int> nudges;
    for(const char *p = argc == 4 ? argv[3] : "-1"; *p;){
        char *end;
        long v = strtol(p, &end, 10);
        if(end == p || v < -1 || v > 7){ fprintf(stderr, "bad nudge list\n"); return 2; }
        nudges.push_back((int) v);
        p = *end == ',' ? end + 1 : end;
        if(*end && *end != ','){ fprintf(stderr, "bad nudge list\n"); return 2; }
    }
    FILE *f = fopen(argv[1], "rb");
    if(!f){ perror(argv[1]); return 2; }
    int32_t n[5];
    if(fread(n, sizeof(int32_t), 5, f) != 5 || n[0] < 0 || n[1] < 0 || n[2] < 0 || n[3] < 0 || n[4] < 1){ fprintf(stderr, "bad header\n"); return 2; }
    std::vector<unsigned char> lights((size_t) n[0] * 144), spheres((size_t) n[1] * 100), tris((size_t) n[2] * 120), moved(tris.size());
    std::vector<int32_t> budgets((size_t) n[4]);
    if(!read_exact(f, lights.data(), lights.size()) || !read_exact(f, spheres.data(), spheres.size()) || !read_exact(f, tris.data(), tris.size())
       || !read_exact(f, budgets.data(), budgets.size() * 4)){ fprintf(stderr, "short file\n"); return 2; }
    for(int32_t b : budgets) if(b < 0){ fprintf(stderr, "bad budget\n"); return 2; }
    hpt::HostScene hs;
    const char *err = hpt::build_host_scene(lights.data(), n[0], spheres.data(), n[1], tris.data(), n[2], hs);
    if(err && *err){ fprintf(stderr, "build_host_scene: %s\n", err); return 1; }
    // the rays of every step, and the tree's figures
    std::vector<std::vector<Ray>> rays((size_t) n[3] + 1);
    std::vector<std::vector<unsigned char>> step_tris((size_t) n[3]);
    for(int s = -1; s < n[3]; ++s){
        if(s >= 0){
            step_tris[s].resize(tris.size());
            if(!read_exact(f, step_tris[s].data(), tris.size())){ fprintf(stderr, "short file\n"); return 2; }
        }
        int32_t nr;
        if(fread(&nr, 4, 1, f) != 1 || nr < 0){ fprintf(stderr, "short file\n"); return 2; }
        std::vector<uint32_t> words((size_t) nr * 8);
        if(!read_exact(f, words.data(), words.size() * 4)){ fprintf(stderr, "short file\n"); return 2; }
        rays[s + 1].resize((size_t) nr);
        for(int i = 0; i < nr; ++i){
            const uint32_t *q = &words[(size_t) i * 8];
            Ray &r = rays[s + 1][i];
            r.ro = mk3(u2f(q[0]), u2f(q[1]), u2f(q[2])); r.rd = mk3(u2f(q[3]), u2f(q[4]), u2f(q[5])); r.tmax = u2f(q[6]); r.any = q[7];
        }
    }
    fclose(f);
    FILE *out = fopen(argv[2], "wb");
    if(!out){ perror(argv[2]); return 2; }
    std::vector<Result> res;
    for(size_t k = 0; k < nudges.size(); ++k){
        if(k > 0){                                                   // every nudge walks every step's tree: start from the builder's again
            hs = hpt::HostScene();
            err = hpt::build_host_scene(lights.data(), n[0], spheres.data(), n[1], tris.data(), n[2], hs);
            if(err && *err){ fprintf(stderr, "build_host_scene: %s\n", err); return 1; }
        }
        for(int s = -1; s < n[3]; ++s){
            if(s >= 0){
                err = hpt::refit_host_scene(hs, step_tris[s].data(), n[2]);
                if(err && *err){ fprintf(stderr, "refit_host_scene: %s\n", err); return 1; }
            }
            if(k == 0)
                printf("step=%d num_nodes=%zu wnodes=%zu bvh_depth=%d wide_depth=%d fits=%d\n", s, hs.qnodes.size(), hs.wnodes.size(), hs.bvh_depth,
                       hs.wide_depth, 3 * hs.wide_depth + 2 <= kResumeLdsLevels + kDeepLevels ? 1 : 0);
            const std::vector<Ray> &rs = rays[s + 1];
            res.resize(rs.size() * budgets.size());
            for(size_t i = 0; i < rs.size(); ++i)
                for(size_t b = 0; b < budgets.size(); ++b) walk_ray(hs, rs[i], (uint32_t) budgets[b], nudges[k], res[i * budgets.size() + b]);
            if(!res.empty() && fwrite(res.data(), sizeof(Result), res.size(), out) != res.size()){ perror("write"); return 2; }
        }
    }
    if(fclose(out) != 0){ perror("close"); return 2; }
    return 0;
}
