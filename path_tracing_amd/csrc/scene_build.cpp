// Host side of scene upload: flattens the reference's AoS records into the device layout
// (hpt_scene.h) and builds a binned-SAH BVH2 over the triangles.
//
// The reference has no acceleration structure: closest-hit and shadow rays scan every
// primitive (reference include/geometric.cuh:293-388).  The BVH must therefore return
// exactly what the scan returns: leaves keep the reference scan ordinal of every
// triangle so traversal can break exact ties the way the scan's strict '<' does, and
// node boxes are padded so no hit the scan accepts is culled.
//
// Float expressions here that feed the kernels (light invariants, triangle edges) are
// evaluated in the order written, without FMA contraction (-ffp-contract=off).
#include "hpt_scene.h"
#include "../../include/hpt.h"       // hpt_tree_cost

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <array>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#ifdef __linux__
#include <sched.h>
#endif

namespace hpt {
namespace {

// ---- reference record layouts (include/hpt.h; reference include/geometric.cuh:15-78) ----
struct RefMatOld { float Kd[3], Kg[3], Ks[3], glossy, exp, refract, reflect; };
struct RefMat { float base[3], roughness, metallic, eta; int32_t type; };
struct RefSphere { float c[3], r; RefMatOld o; RefMat m; int32_t id; };
struct RefTriangle { float v0[3], v1[3], v2[3]; RefMatOld o; RefMat m; int32_t id; };
struct RefLight { float pos[3], dir[3], illum[3]; RefSphere ball; float cutoff; int32_t is_parallel; };
static_assert(sizeof(RefSphere) == 100 && sizeof(RefTriangle) == 120 && sizeof(RefLight) == 144, "layout");

constexpr float kPi = 3.14159265358979323846f;

struct Box {
    float mn[3], mx[3];
    void reset(){ for(int a = 0; a < 3; ++a){ mn[a] = INFINITY; mx[a] = -INFINITY; } }
    void grow(const float *p){ for(int a = 0; a < 3; ++a){ mn[a] = std::min(mn[a], p[a]); mx[a] = std::max(mx[a], p[a]); } }
    void grow(const Box &b){ for(int a = 0; a < 3; ++a){ mn[a] = std::min(mn[a], b.mn[a]); mx[a] = std::max(mx[a], b.mx[a]); } }
    float half_area() const {
        float dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
        if(dx < 0 || dy < 0 || dz < 0) return 0.0f;
        return dx * dy + dy * dz + dz * dx;
    }
};

struct Prim { Box box; float cen[3]; uint32_t index; };

// Host threads for the O(n) passes of a large scene: [0, n) is cut into kChunks contiguous ranges -- always the same ones,
// whatever the machine, so that nothing a pass derives from the cut depends on where it runs -- and the ranges are handed
// to a small pool of helper threads (created on first use, at most kChunks - 1) and to the caller itself, which takes
// ranges like any helper and returns when all are done: a caller never waits for a helper to START, so a pool that is
// busy (several big subtrees at once), or gone (a forked child), only costs speed.  fn(chunk, begin, end).
constexpr int kChunks = 32;
constexpr size_t kParallelForMin = 65536;

// Threads worth starting: the hardware's count cut down to the scheduler affinity mask, 64 at most.  (A cgroup CPU quota is
// deliberately NOT applied: on the 16-CPU-quota GPU boxes the 1 M-triangle build measured 700 ms on 1 thread, 330-380 on
// 16, 270-310 on 32 and 260 on 64.)
int usable_cpus(){
    static const int n = [](){
        long best = (long) std::thread::hardware_concurrency();
        if(best < 1) best = 1;
#ifdef HPT_DEV_TUNING
        if(const char *e = getenv("HPT_BUILD_THREADS")){ int v = atoi(e); if(v >= 1) return v; }
#endif
#ifdef __linux__
        cpu_set_t set; CPU_ZERO(&set);
        if(sched_getaffinity(0, sizeof set, &set) == 0){ long c = CPU_COUNT(&set); if(c > 0 && c < best) best = c; }
#endif
        return (int) std::min<long>(best, 64);
    }();
    return n;
}

class HelperPool {
public:
    static HelperPool &get(){ static HelperPool p; return p; }
    void submit(const std::function<void()> &job, int copies){
        { std::lock_guard<std::mutex> lock(mu_);
          if(workers_.empty()){
              int n = std::min(usable_cpus() - 1, kChunks - 1);
              for(int i = 0; i < n; ++i) workers_.emplace_back([this](){ run(); });
          }
          for(int i = 0; i < copies && i < (int) workers_.size(); ++i) queue_.push_back(job); }
        cv_.notify_all();
    }
    ~HelperPool(){
        { std::lock_guard<std::mutex> lock(mu_); stop_ = true; }
        cv_.notify_all();
        for(std::thread &t : workers_) t.join();
    }
private:
    void run(){
        for(;;){
            std::function<void()> job;
            { std::unique_lock<std::mutex> lock(mu_);
              cv_.wait(lock, [this](){ return stop_ || !queue_.empty(); });
              if(stop_) return;
              job = std::move(queue_.front()); queue_.pop_front(); }
            job();
        }
    }
    std::mutex mu_; std::condition_variable cv_; std::deque<std::function<void()>> queue_; std::vector<std::thread> workers_; bool stop_ = false;
};

template <typename F>
void parallel_chunks(size_t n, F fn){
    auto range = [n](int c, size_t &b, size_t &e){ b = n * (size_t) c / kChunks; e = n * (size_t) (c + 1) / kChunks; };
    if(n < kParallelForMin || usable_cpus() <= 1){
        for(int c = 0; c < kChunks; ++c){ size_t b, e; range(c, b, e); if(b < e) fn(c, b, e); }
        return;
    }
    struct Job { std::atomic<int> next{0}, done{0}; };
    auto job = std::make_shared<Job>();
    // helpers hold the job (and a copy of fn's captures by reference: valid until done == kChunks, which the caller awaits)
    auto take = [job, range, &fn](){
        for(;;){
            int c = job->next.fetch_add(1);
            if(c >= kChunks) break;
            size_t b, e; range(c, b, e);
            if(b < e) fn(c, b, e);
            job->done.fetch_add(1, std::memory_order_release);
        }
    };
    HelperPool::get().submit(take, kChunks - 1);
    take();
    while(job->done.load(std::memory_order_acquire) < kChunks) std::this_thread::yield();
}

// What a node stores for a child whose triangles span `b`: padded by an absolute slack plus two ulps so that rounding in the
// slab test and in Moeller-Trumbore can never cull a hit the brute-force scan accepts
void write_padded_box(float *mn, float *mx, const Box &b, float pad_abs){
    for(int a = 0; a < 3; ++a){
        float lo = b.mn[a] - pad_abs, hi = b.mx[a] + pad_abs;
        lo = std::nextafter(std::nextafter(lo, -INFINITY), -INFINITY);
        hi = std::nextafter(std::nextafter(hi, INFINITY), INFINITY);
        mn[a] = lo; mx[a] = hi;
    }
}

struct Builder {
    pod_vector<Prim> prims;
    pod_vector<BvhNode> nodes;        // pre-sized by the caller; slots are handed out by next_node
    pod_vector<Prim> scratch;         // the big nodes' partition buffer (sized once, by the root)
    std::atomic<uint32_t> next_node{0};
    std::atomic<int> max_depth_seen{0};
    float pad_abs = 0.0f;
    int max_leaf = kMaxLeafTris;
    uint32_t node_base = 0, tri_base = 0;     // offsets when several BVHs share one node / triangle array

    static constexpr int kBins = 16;
    // Subtrees of more than kParallelMin triangles are built on their own host thread while the parent goes on with the
    // sibling (at most as many threads at a time as the process may use CPUs).  The tree does not depend on it, nor on how
    // many CPUs there are: a subtree over prims[first, first + count) only reads and permutes that range, and which
    // primitives go left at a node is a function of the node's set alone, so every leaf gets the same SET of triangles and
    // the same range of leaf slots whichever partition ran above it.  The ORDER inside a range is not such a function -- the
    // big nodes' partition is stable and std::partition is not, and which of the two a node gets depends on the CPU count
    // -- so make_leaf puts every leaf into input order.  Node numbers, the one thing the thread schedule decides, are
    // replaced by the breadth-first renumbering afterwards.
    static constexpr int kParallelMin = 8192;
    static int parallel_levels(){ int l = 0; while((2 << l) <= usable_cpus() && l < 6) ++l; return l; }     // 2^levels subtree threads at most
    static constexpr size_t kBigNode = 131072;        // nodes this large bin and partition their range on several threads

    void write_box(float *mn, float *mx, const Box &b) const { write_padded_box(mn, mx, b, pad_abs); }

    uint32_t make_leaf(int first, int count){
        // canonical leaf order: by input index (a leaf holds 8 triangles at most: insertion sort)
        for(int i = first + 1; i < first + count; ++i)
            for(int j = i; j > first && prims[j].index < prims[j - 1].index; --j) std::swap(prims[j], prims[j - 1]);
        return kLeafFlag | (((uint32_t) first + tri_base) << 3) | (uint32_t) (count - 1);
    }

    // node slots are handed out in blocks of kSlotBlock per thread (one shared counter, touched once per block); the slots a
    // thread does not use stay empty and are dropped by the breadth-first renumbering.  The root takes slot 0.
    static constexpr uint32_t kSlotBlock = 256;
    static constexpr size_t kSlotSlack = (size_t) kSlotBlock * 160;      // > (threads that ever build a subtree) x block: 2 x 64 spawned at most
    const uint64_t id = [](){ static std::atomic<uint64_t> counter{0}; return ++counter; }();
    uint32_t alloc_node(){
        static thread_local uint64_t owner = 0;
        static thread_local uint32_t next = 0, end = 0;
        if(owner != id || next == end){ owner = id; next = next_node.fetch_add(kSlotBlock, std::memory_order_relaxed); end = next + kSlotBlock; }
        return next++;
    }

    void note_depth(int depth){
        int seen = max_depth_seen.load(std::memory_order_relaxed);
        while(depth > seen && !max_depth_seen.compare_exchange_weak(seen, depth, std::memory_order_relaxed)){}
    }

    // Bounds (primitive boxes, centroids) of prims[first, first+count): the root's only -- every other node gets its own from the
    // partition that made it.
    void range_bounds(int first, int count, Box &bb, Box &cb, bool parallel){
        bb.reset(); cb.reset();
        if(parallel && (size_t) count >= kBigNode){
            std::vector<Box> pb((size_t) kChunks), pc((size_t) kChunks);
            for(int c = 0; c < kChunks; ++c){ pb[(size_t) c].reset(); pc[(size_t) c].reset(); }
            parallel_chunks((size_t) count, [&](int c, size_t b0, size_t e0){
                for(size_t i = (size_t) first + b0; i < (size_t) first + e0; ++i){ pb[(size_t) c].grow(prims[i].box); pc[(size_t) c].grow(prims[i].cen); }
            });
            for(int c = 0; c < kChunks; ++c){ bb.grow(pb[(size_t) c]); cb.grow(pc[(size_t) c]); }
        } else
        for(int i = first; i < first + count; ++i){ bb.grow(prims[i].box); cb.grow(prims[i].cen); }
    }

    uint32_t build(int first, int count, int depth, Box &out_box, int par_levels = -1){
        if(par_levels < 0) par_levels = parallel_levels();
        if(par_levels > 0 && (size_t) count >= kBigNode && scratch.size() < prims.size()) scratch.resize(prims.size());    // before any thread is started
        Box bb, cb;
        range_bounds(first, count, bb, cb, par_levels > 0);
        out_box = bb;
        return build_node(first, count, depth, bb, cb, par_levels);
    }

    // bin of a centroid: (int) of the scaled offset clamped to [0, kBins) -- written so that a NaN or an offset beyond int
    // (centroids of records with non-finite coordinates, where a caller lets them in) is never converted: NaN goes to bin 0
    static int bin_of(float cen, float lo, float scale){
        const float f = (cen - lo) * scale;
        return f >= 1.0f ? (f < (float) kBins ? (int) f : kBins - 1) : 0;
    }

    struct Bins { Box box[3][kBins]; int cnt[3][kBins]; void reset(){ for(int a = 0; a < 3; ++a) for(int b = 0; b < kBins; ++b){ box[a][b].reset(); cnt[a][b] = 0; } } };

    // Builds the subtree over prims[first, first+count) whose primitive boxes span bb and whose centroids span cb; returns its
    // child code.  One pass bins the range on all three axes, one pass partitions it and gathers the two children's bounds.
    uint32_t build_node(int first, int count, int depth, const Box &bb, const Box &cb, int par_levels){
        note_depth(depth);
        if(count <= max_leaf) return make_leaf(first, count);

        // levels still available below this node; force balanced splits when they run short
        int remaining = kMaxBvhDepth - depth;
        int need = 0;
        { int leaves = (count + max_leaf - 1) / max_leaf; while((1 << need) < leaves) ++need; }
        bool force_median = need >= remaining;

        int axis = 0;
        float ext[3] = { cb.mx[0] - cb.mn[0], cb.mx[1] - cb.mn[1], cb.mx[2] - cb.mn[2] };
        if(ext[1] > ext[axis]) axis = 1;
        if(ext[2] > ext[axis]) axis = 2;

        const bool big = par_levels > 0 && (size_t) count >= kBigNode;        // the few nodes at the top of a large tree
        int mid = -1;
        Box lbb, lcb, rbb, rcb; lbb.reset(); lcb.reset(); rbb.reset(); rcb.reset();
        if(!force_median && ext[axis] > 0.0f){
            float scale[3]; bool use[3];
            for(int ax = 0; ax < 3; ++ax){ use[ax] = ext[ax] > 0.0f; scale[ax] = use[ax] ? (float) kBins / ext[ax] : 0.0f; }
            auto bin_range = [&](Bins &bins, size_t b0, size_t e0){
                for(size_t i = b0; i < e0; ++i){
                    const Prim &p = prims[i];
                    for(int ax = 0; ax < 3; ++ax){
                        if(!use[ax]) continue;
                        const int b = bin_of(p.cen[ax], cb.mn[ax], scale[ax]);
                        bins.box[ax][b].grow(p.box); bins.cnt[ax][b]++;
                    }
                }
            };
            Bins bins; bins.reset();
            if(big){
                // per-chunk bins merged afterwards: boxes grow by min / max and counts add, so the result is the serial one
                std::vector<Bins> part((size_t) kChunks);
                for(Bins &b : part) b.reset();
                parallel_chunks((size_t) count, [&](int c, size_t b0, size_t e0){ bin_range(part[(size_t) c], (size_t) first + b0, (size_t) first + e0); });
                for(const Bins &pb : part) for(int ax = 0; ax < 3; ++ax) for(int b = 0; b < kBins; ++b){ bins.box[ax][b].grow(pb.box[ax][b]); bins.cnt[ax][b] += pb.cnt[ax][b]; }
            } else bin_range(bins, (size_t) first, (size_t) first + (size_t) count);

            float best_cost = INFINITY; int best_axis = -1, best_bin = -1;
            for(int ax = 0; ax < 3; ++ax){
                if(!use[ax]) continue;
                float right_area[kBins]; int right_cnt[kBins];
                Box acc; acc.reset(); int c = 0;
                for(int b = kBins - 1; b > 0; --b){
                    acc.grow(bins.box[ax][b]); c += bins.cnt[ax][b];
                    right_area[b] = acc.half_area(); right_cnt[b] = c;
                }
                acc.reset(); c = 0;
                for(int b = 0; b < kBins - 1; ++b){
                    acc.grow(bins.box[ax][b]); c += bins.cnt[ax][b];
                    if(c == 0 || right_cnt[b + 1] == 0) continue;
                    float cost = acc.half_area() * (float) c + right_area[b + 1] * (float) right_cnt[b + 1];
                    if(cost < best_cost){ best_cost = cost; best_axis = ax; best_bin = b; }
                }
            }
            if(best_axis >= 0){
                const float sc = scale[best_axis], lo = cb.mn[best_axis];
                auto goes_left = [&](const Prim &p){ return bin_of(p.cen[best_axis], lo, sc) <= best_bin; };
                if(big){
                    // stable partition through a scratch copy: every chunk counts (and gathers the children's bounds), then
                    // scatters to the offsets the counts give
                    std::vector<size_t> nleft((size_t) kChunks, 0), nall((size_t) kChunks, 0);
                    std::vector<Box> cl((size_t) kChunks), ccl((size_t) kChunks), cr((size_t) kChunks), ccr((size_t) kChunks);
                    for(int c = 0; c < kChunks; ++c){ cl[(size_t) c].reset(); ccl[(size_t) c].reset(); cr[(size_t) c].reset(); ccr[(size_t) c].reset(); }
                    parallel_chunks((size_t) count, [&](int c, size_t b0, size_t e0){
                        size_t l = 0;
                        for(size_t i = (size_t) first + b0; i < (size_t) first + e0; ++i){
                            const Prim &p = prims[i];
                            if(goes_left(p)){ ++l; cl[(size_t) c].grow(p.box); ccl[(size_t) c].grow(p.cen); } else { cr[(size_t) c].grow(p.box); ccr[(size_t) c].grow(p.cen); }
                        }
                        nleft[(size_t) c] = l; nall[(size_t) c] = e0 - b0;
                    });
                    size_t total_left = 0; for(size_t l : nleft) total_left += l;
                    for(int c = 0; c < kChunks; ++c){ lbb.grow(cl[(size_t) c]); lcb.grow(ccl[(size_t) c]); rbb.grow(cr[(size_t) c]); rcb.grow(ccr[(size_t) c]); }
                    std::vector<size_t> loff((size_t) kChunks), roff((size_t) kChunks);
                    { size_t l = 0, r = total_left; for(int c = 0; c < kChunks; ++c){ loff[(size_t) c] = l; roff[(size_t) c] = r; l += nleft[(size_t) c]; r += nall[(size_t) c] - nleft[(size_t) c]; } }
                    // (the scratch range [first, first + count) belongs to this node alone: big nodes working at once are disjoint)
                    Prim *tmp = scratch.data() + first;
                    parallel_chunks((size_t) count, [&](int c, size_t b0, size_t e0){
                        size_t l = loff[(size_t) c], r = roff[(size_t) c];
                        for(size_t i = (size_t) first + b0; i < (size_t) first + e0; ++i){ if(goes_left(prims[i])) tmp[l++] = prims[i]; else tmp[r++] = prims[i]; }
                    });
                    parallel_chunks((size_t) count, [&](int, size_t b0, size_t e0){ std::copy(tmp + b0, tmp + e0, prims.begin() + first + (long) b0); });
                    mid = first + (int) total_left;
                } else {
                    // std::partition applies the predicate to every element exactly once: the children's bounds are gathered on the way
                    auto it = std::partition(prims.begin() + first, prims.begin() + first + count, [&](const Prim &p){
                        const bool l = goes_left(p);
                        if(l){ lbb.grow(p.box); lcb.grow(p.cen); } else { rbb.grow(p.box); rcb.grow(p.cen); }
                        return l;
                    });
                    mid = (int) (it - prims.begin());
                }
                if(mid == first || mid == first + count) mid = -1;
            }
        }
        if(mid < 0){
            // object median along the widest centroid axis (also the degenerate-centroid case)
            mid = first + count / 2;
            std::nth_element(prims.begin() + first, prims.begin() + mid, prims.begin() + first + count,
                             [&](const Prim &a, const Prim &b){
                                 // (a NaN centroid sorts as +inf: '<' alone is no strict weak order among NaNs)
                                 const float ca = a.cen[axis] == a.cen[axis] ? a.cen[axis] : INFINITY, cb2 = b.cen[axis] == b.cen[axis] ? b.cen[axis] : INFINITY;
                                 if(ca != cb2) return ca < cb2;
                                 return a.index < b.index;
                             });
            range_bounds(first, mid - first, lbb, lcb, false);
            range_bounds(mid, first + count - mid, rbb, rcb, false);
        }

        uint32_t me = alloc_node();
        // (children return codes that already include node_base / tri_base)
        uint32_t lc, rc;
        if(par_levels > 0 && count > kParallelMin){
            std::thread left([&](){ lc = build_node(first, mid - first, depth + 1, lbb, lcb, par_levels - 1); });
            rc = build_node(mid, first + count - mid, depth + 1, rbb, rcb, par_levels - 1);
            left.join();
        } else {
            lc = build_node(first, mid - first, depth + 1, lbb, lcb, 0);
            rc = build_node(mid, first + count - mid, depth + 1, rbb, rcb, 0);
        }
        BvhNode &n = nodes[me];
        write_box(n.lmin, n.lmax, lbb); n.left = lc;
        write_box(n.rmin, n.rmax, rbb); n.right = rc;
        n.pad0 = n.pad1 = 0;
        return me + node_base;
    }
};

void set_empty_box(float *mn, float *mx){
    for(int a = 0; a < 3; ++a){ mn[a] = INFINITY; mx[a] = -INFINITY; }
}

struct MatKey {
    uint32_t w[7];
    bool operator<(const MatKey &o) const { return memcmp(w, o.w, sizeof w) < 0; }
};

// the record's per-material constants of the shade stage, from its roughness, metallic and eta: the class bits and the GGX
// width, roughness_to_alpha (pt_device_math.h) operation for operation
void material_constants(DevMaterial &d){
    d.cls = material_class(d.roughness, d.metallic, d.eta);
    float x = fmaxf(d.roughness, 1e-3f);
    d.alpha = x * x;
}

// the table's stand-in entry of a scene without surfaces
DevMaterial blank_material(){
    DevMaterial m; memset(&m, 0, sizeof m);
    material_constants(m);
    return m;
}

uint32_t intern_material(const RefMat &m, std::map<MatKey, uint32_t> &table, std::vector<DevMaterial> &out){
    MatKey k; memcpy(k.w, &m, sizeof k.w);
    auto it = table.find(k);
    if(it != table.end()) return it->second;
    DevMaterial d;
    d.base[0] = m.base[0]; d.base[1] = m.base[1]; d.base[2] = m.base[2];
    d.roughness = m.roughness; d.metallic = m.metallic; d.eta = m.eta; d.type = (uint32_t) m.type;
    // same float operations as the kernel's `m.base / kPi * (1.0f - m.metallic)` (IEEE divide, no contraction)
    const float pi = 3.14159265358979323846f;
    for(int a = 0; a < 3; ++a){ float q = m.base[a] / pi; d.diffuse[a] = q * (1.0f - m.metallic); }
    material_constants(d);
    uint32_t idx = (uint32_t) out.size();
    out.push_back(d);
    table.emplace(k, idx);
    return idx;
}

void normalize3(const float *v, float s, float *out){
    // normalize(v * s) with the reference's float3 algebra (geometric.cuh:92,95,97,98)
    float x = v[0] * s, y = v[1] * s, z = v[2] * s;
    float len = sqrtf(x * x + y * y + z * z);
    out[0] = x / len; out[1] = y / len; out[2] = z / len;
}

// ---- the steps of a build that are functions of the vertex positions alone: the builder and the refit run these lines ----

// Dead triangles.  A record whose edge v1 - v0 or v2 - v0 has a component that is not finite -- a NaN or infinite
// coordinate, or two finite ones whose difference overflows -- is hit by no ray: in hit_triangle (pt_device_math.h; the
// reference's geometric.cuh:261-291) the determinant a = dot(e1, cross(rd, e2)) is then infinite or NaN, f = 1 / a is 0 or
// NaN, and t = f * (...) is 0 or NaN, which `t > kEps` rejects.  Such a record keeps its leaf slot (the slots are a
// permutation of the input; the scan kernels index them) but must not reach a box, pad_abs or the grid, where one
// infinity makes every plane NaN and every ray visit every node: it enters the build as a point at the low corner of the
// live triangles' box (the origin when there is none).
// set(i, box, live) is called once for every input triangle (from several threads), and once more for every dead one when
// its point is known; scene_box comes back as the box of what was set last.  Returns the number of dead triangles.
template <typename Set>
size_t triangle_boxes(const RefTriangle *tris, int nt, Box &scene_box, Set set){
    scene_box.reset();
    std::vector<Box> part((size_t) kChunks);
    std::vector<std::vector<uint32_t>> dead((size_t) kChunks);          // input indices of the dead triangles, per chunk
    for(Box &b : part) b.reset();
    parallel_chunks((size_t) nt, [&](int c, size_t b0, size_t e0){
        for(size_t i = b0; i < e0; ++i){
            const RefTriangle &t = tris[i];
            bool live = true;
            for(int a = 0; a < 3; ++a) live = live && std::isfinite(t.v1[a] - t.v0[a]) && std::isfinite(t.v2[a] - t.v0[a]);
            Box box;
            if(!live){
                // placed below, once the live triangles' box is known
                for(int a = 0; a < 3; ++a) box.mn[a] = box.mx[a] = 0.0f;
                set(i, box, false);
                dead[(size_t) c].push_back((uint32_t) i);
                continue;
            }
            box.reset();
            box.grow(t.v0); box.grow(t.v1); box.grow(t.v2);
            set(i, box, true);
            part[(size_t) c].grow(box);
        }
    });
    for(const Box &b : part) scene_box.grow(b);
    size_t ndead = 0; for(const std::vector<uint32_t> &d : dead) ndead += d.size();
    if(ndead > 0){
        Box at;
        for(int a = 0; a < 3; ++a) at.mn[a] = at.mx[a] = ndead < (size_t) nt ? scene_box.mn[a] : 0.0f;
        for(const std::vector<uint32_t> &d : dead) for(uint32_t i : d) set(i, at, false);
        scene_box.grow(at.mn);
    }
    return ndead;
}

// the absolute slack of every stored box (write_padded_box)
float box_padding(const Box &scene_box, int nt){
    float extent = 0.0f;
    if(nt > 0) for(int a = 0; a < 3; ++a){
        extent = std::max(extent, scene_box.mx[a] - scene_box.mn[a]);
        extent = std::max(extent, std::max(std::fabs(scene_box.mn[a]), std::fabs(scene_box.mx[a])));
    }
    return 2e-6f * extent;
}

inline void triangle_geometry(DevTriangle &d, const RefTriangle &t){
    for(int a = 0; a < 3; ++a){
        d.v0[a] = t.v0[a];
        d.e1[a] = t.v1[a] - t.v0[a];          // geometric.cuh:266-267
        d.e2[a] = t.v2[a] - t.v0[a];
    }
}

// grid coordinates of a stored plane (double precision; a NaN lands on 0)
inline uint32_t grid_lo(float v, float origin, float scale){ double q = std::floor(((double) v - (double) origin) / (double) scale) - 1.0; return (uint32_t) std::min(65535.0, std::max(0.0, q)); }
inline uint32_t grid_hi(float v, float origin, float scale){ double q = std::ceil(((double) v - (double) origin) / (double) scale) + 1.0; return (uint32_t) std::min(65535.0, std::max(0.0, q)); }

// quantised twin: 16-bit grid over the union of the (padded) node boxes of hs.nodes; fills qorigin, qscale and qnodes
void quantise_tree(HostScene &hs){
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    {   std::vector<Box> part((size_t) kChunks);
        for(Box &b : part) b.reset();
        parallel_chunks(hs.nodes.size(), [&](int c, size_t b0, size_t e0){
            Box &pb = part[(size_t) c];
            for(size_t i = b0; i < e0; ++i){
                const BvhNode &n = hs.nodes[i];
                if(n.left != kEmptyChild){ pb.grow(n.lmin); pb.grow(n.lmax); }
                if(n.right != kEmptyChild){ pb.grow(n.rmin); pb.grow(n.rmax); }
            }
        });
        for(const Box &b : part) for(int a = 0; a < 3; ++a){ lo[a] = std::min(lo[a], b.mn[a]); hi[a] = std::max(hi[a], b.mx[a]); }
    }
    grid_of_box(lo, hi, hs.qorigin, hs.qscale);
    hs.qnodes.resize(hs.nodes.size());
    parallel_chunks(hs.nodes.size(), [&](int, size_t b0, size_t e0){
        for(size_t i = b0; i < e0; ++i){
            const BvhNode &n = hs.nodes[i]; QBvhNode &q = hs.qnodes[i];
            for(int a = 0; a < 3; ++a){
                const float o = hs.qorigin[a], sc = hs.qscale[a];
                if(n.left != kEmptyChild){ q.plane[a][0][0] = (uint16_t) grid_lo(n.lmin[a], o, sc); q.plane[a][1][0] = (uint16_t) grid_hi(n.lmax[a], o, sc); } else { q.plane[a][0][0] = 65535; q.plane[a][1][0] = 0; }
                if(n.right != kEmptyChild){ q.plane[a][0][1] = (uint16_t) grid_lo(n.rmin[a], o, sc); q.plane[a][1][1] = (uint16_t) grid_hi(n.rmax[a], o, sc); } else { q.plane[a][0][1] = 65535; q.plane[a][1][1] = 0; }
            }
            q.left = n.left; q.right = n.right;
        }
    });
}

// four-wide twin, boxes: words 0-11 of every wide node from the stored box of the binary child each of its four children was
// collapsed from (hs.wide_src, recorded by the build), on the grid of quantise_tree; the child codes (words 12-15) are the build's
void pack_wide_boxes(HostScene &hs){
    parallel_chunks(hs.wnodes.size(), [&](int, size_t b0, size_t e0){
        for(size_t qi = b0; qi < e0; ++qi){
            WideNode &w = hs.wnodes[qi];
            uint32_t lo[3][4], hi[3][4];
            for(int k = 0; k < 4; ++k){
                const uint32_t src = hs.wide_src[qi * 4 + (size_t) k];
                if(src != kEmptyChild){
                    const BvhNode &b = hs.nodes[src >> 1];
                    const float *mn = (src & 1u) ? b.rmin : b.lmin, *mx = (src & 1u) ? b.rmax : b.lmax;
                    for(int a = 0; a < 3; ++a){ lo[a][k] = grid_lo(mn[a], hs.qorigin[a], hs.qscale[a]); hi[a][k] = grid_hi(mx[a], hs.qorigin[a], hs.qscale[a]); }
                }
                else { for(int a = 0; a < 3; ++a){ lo[a][k] = 65535u; hi[a][k] = 0u; } }
            }
            for(int a = 0; a < 3; ++a){
                w.w[a * 4 + 0] = lo[a][0] | (lo[a][1] << 16); w.w[a * 4 + 1] = lo[a][2] | (lo[a][3] << 16);
                w.w[a * 4 + 2] = hi[a][0] | (hi[a][1] << 16); w.w[a * 4 + 3] = hi[a][2] | (hi[a][3] << 16);
            }
        }
    });
}

// (defined behind build_host_scene)
void triangle_materials(const RefTriangle *tris, int nt, std::map<MatKey, uint32_t> &mat_table, std::vector<DevMaterial> &materials,
                        pod_vector<uint32_t> &mat_of);
void collapse_wide(HostScene &hs);

} // namespace

void grid_of_box(const float lo_in[3], const float hi_in[3], float qorigin[3], float qscale[3]){
    for(int a = 0; a < 3; ++a){
        float lo = lo_in[a], hi = hi_in[a];
        if(!(lo <= hi)){ lo = 0.0f; hi = 1.0f; }
        qorigin[a] = lo;
        float ext = hi - lo;
        qscale[a] = ext > 0.0f ? ext / 65535.0f : 1.0f;
        qscale[a] = std::nextafter(qscale[a], INFINITY);          // never shorter than the box
    }
}

float box_padding_of(const float scene_min[3], const float scene_max[3], int nt){
    Box b; for(int a = 0; a < 3; ++a){ b.mn[a] = scene_min[a]; b.mx[a] = scene_max[a]; }
    return box_padding(b, nt);
}

const char *flatten_rounds_host(const void *lights_v, int nl, const void *spheres_v, int ns, const uint32_t *sphere_material,
                                std::vector<DevRound> &rounds, std::vector<DevLight> &lights_out){
    if(nl < 0 || ns < 0) return "negative primitive count";
    if((nl > 0 && !lights_v) || (ns > 0 && (!spheres_v || !sphere_material))) return "null primitive array";
    const RefLight *lights = (const RefLight *) lights_v;
    const RefSphere *spheres = (const RefSphere *) spheres_v;
    // spheres then light balls: the reference's closest-hit scan order (geometric.cuh:340-368)
    rounds.clear(); rounds.reserve((size_t) ns + nl);
    for(int i = 0; i < ns; ++i){
        DevRound r; memset(&r, 0, sizeof r);
        r.c[0] = spheres[i].c[0]; r.c[1] = spheres[i].c[1]; r.c[2] = spheres[i].c[2]; r.r = spheres[i].r;
        r.material = sphere_material[i];
        r.flags = (spheres[i].m.eta <= 0.0f) ? 1u : 0u;
        rounds.push_back(r);
    }
    for(int i = 0; i < nl; ++i){
        DevRound r; memset(&r, 0, sizeof r);
        const RefSphere &b = lights[i].ball;
        r.c[0] = b.c[0]; r.c[1] = b.c[1]; r.c[2] = b.c[2]; r.r = b.r;
        r.material = (uint32_t) i;
        r.flags = 2u;
        rounds.push_back(r);
    }
    lights_out.clear(); lights_out.reserve(nl);
    for(int i = 0; i < nl; ++i){
        const RefLight &L = lights[i];
        DevLight d; memset(&d, 0, sizeof d);
        d.raw_dir[0] = L.dir[0]; d.raw_dir[1] = L.dir[1]; d.raw_dir[2] = L.dir[2];
        d.ball_c[0] = L.ball.c[0]; d.ball_c[1] = L.ball.c[1]; d.ball_c[2] = L.ball.c[2];
        d.pos[0] = L.pos[0]; d.pos[1] = L.pos[1]; d.pos[2] = L.pos[2];
        d.r = L.ball.r;
        normalize3(L.dir, 1.0f, d.main_dir);          // normalize(light.dir), pt_cu.cu:75,167
        normalize3(L.dir, -1.0f, d.neg_dir);          // normalize(light.dir * -1.0f), pt_cu.cu:131
        d.cos_cutoff = cosf(L.cutoff);                // pt_cu.cu:73,79,168
        d.cutoff = L.cutoff;
        d.illum[0] = L.illum[0]; d.illum[1] = L.illum[1]; d.illum[2] = L.illum[2];
        d.area = 4.0f * kPi * L.ball.r * L.ball.r;    // pt_cu.cu:70,179
        d.is_parallel = L.is_parallel ? 1u : 0u;
        d.cone_ratio = (1.0f - d.cos_cutoff) / 2.0f;  // pt_cu.cu:73
        d.pdf_area = 1.0f / ((float) nl * d.area);    // k_shade's area pdf of a next-event sample, as it formed it per sample; a function of the COUNT too
        lights_out.push_back(d);
    }
    return "";
}

const char *check_triangle_update(const void *kept_v, int kept_nt, const void *tris_v, int nt, char *msg, size_t msg_cap){
    if(nt < 0) return "negative triangle count";
    if(nt != kept_nt){ snprintf(msg, msg_cap, "an update keeps the triangle count: the scene has %d triangles, %d were handed over", kept_nt, nt); return msg; }
    if(nt > 0 && !tris_v) return "null triangle array";
    const RefTriangle *kept = (const RefTriangle *) kept_v, *tris = (const RefTriangle *) tris_v;
    for(int i = 0; i < nt; ++i)
        if(memcmp(&kept[i].o, &tris[i].o, sizeof(RefTriangle) - offsetof(RefTriangle, o)) != 0){
            snprintf(msg, msg_cap, "an update moves vertices only: material or id bytes of triangle %d differ from the record the scene was created from", i);
            return msg;
        }
    return "";
}

const char *check_parts(const int32_t *tri_part, int nt, int num_parts, char *msg, size_t msg_cap){
    if(nt < 0) return "negative triangle count";
    if(num_parts < 1 || num_parts > kMaxParts){ snprintf(msg, msg_cap, "the number of parts must lie in [1, %d]: %d was given", kMaxParts, num_parts); return msg; }
    if(!tri_part){
        if(num_parts != 1 && nt > 0) return "a null part map puts every triangle in part 0: the number of parts must be 1";
        return "";
    }
    for(int i = 0; i < nt; ++i)
        if(tri_part[i] < 0 || tri_part[i] >= num_parts){
            snprintf(msg, msg_cap, "part %d of triangle %d is not one of the %d parts", tri_part[i], i, num_parts);
            return msg;
        }
    return "";
}

void pose_vertex_host(const float r[12], const float in[3], float out[3]){
    static const float kIdentity[12] = { 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f };
    const float x = in[0], y = in[1], z = in[2];
    if(memcmp(r, kIdentity, sizeof kIdentity) == 0){ out[0] = x; out[1] = y; out[2] = z; return; }
    float p[3];
    for(int a = 0; a < 3; ++a){
        const float *row = r + 4 * a;
        p[a] = ((row[0] * x + row[1] * y) + row[2] * z) + row[3];
    }
    uint32_t w[3]; memcpy(w, p, 12);
    bool finite = true;
    for(int a = 0; a < 3; ++a) finite = finite && (w[a] & 0x7F800000u) != 0x7F800000u;
    if(!finite) w[0] = w[1] = w[2] = 0x7FC00000u;
    memcpy(out, w, 12);
}

const char *pose_host_records(const void *tris_v, int nt, const int32_t *tri_part, const float *xforms, int num_parts, void *out_v,
                              char *msg, size_t msg_cap){
    const char *err = check_parts(tri_part, nt, num_parts, msg, msg_cap);
    if(err && *err) return err;
    if(!xforms) return "null transform array";
    if(nt > 0 && (!tris_v || !out_v)) return "null triangle array";
    const unsigned char *tris = (const unsigned char *) tris_v;
    unsigned char *out = (unsigned char *) out_v;
    parallel_chunks((size_t) nt, [&](int, size_t b0, size_t e0){
        for(size_t i = b0; i < e0; ++i){
            if(out != tris) memcpy(out + i * sizeof(RefTriangle), tris + i * sizeof(RefTriangle), sizeof(RefTriangle));
            const float *r = xforms + (size_t) (tri_part ? tri_part[i] : 0) * 12;
            float v[9]; memcpy(v, out + i * sizeof(RefTriangle), 36);
            for(int k = 0; k < 3; ++k) pose_vertex_host(r, v + 3 * k, v + 3 * k);
            memcpy(out + i * sizeof(RefTriangle), v, 36);
        }
    });
    return "";
}

const char *check_skin(const int32_t *corner_bone, const float *corner_weight, int nt, int num_bones, char *msg, size_t msg_cap){
    if(nt < 0) return "negative triangle count";
    if(num_bones < 1 || num_bones > kMaxBones){ snprintf(msg, msg_cap, "the number of bones must lie in [1, %d]: %d was given", kMaxBones, num_bones); return msg; }
    if(nt > 0 && (!corner_bone || !corner_weight)) return "null influence array";
    for(size_t c = 0; c < (size_t) nt * 3; ++c)
        for(int j = 0; j < kSkinInfluences; ++j){
            const int32_t b = corner_bone[c * kSkinInfluences + j];
            if(b < 0 || b >= num_bones){
                snprintf(msg, msg_cap, "bone %d of triangle %zu corner %zu (influence %d) is not one of the %d bones", b, c / 3, c % 3, j, num_bones);
                return msg;
            }
            uint32_t w; memcpy(&w, corner_weight + c * kSkinInfluences + j, 4);
            if((w & 0x80000000u) || (w & 0x7F800000u) == 0x7F800000u){
                snprintf(msg, msg_cap, "weight 0x%08X of triangle %zu corner %zu (influence %d) is negative or not finite", w, c / 3, c % 3, j);
                return msg;
            }
        }
    return "";
}

namespace {
// arith(r, v): the rows of a pose, one operation at a time
inline void skin_rows(const float *r, float x, float y, float z, float p[3]){
    for(int a = 0; a < 3; ++a){
        const float *row = r + 4 * a;
        p[a] = ((row[0] * x + row[1] * y) + row[2] * z) + row[3];
    }
}
inline void skin_finish(const float p[3], float out[3]){
    uint32_t w[3]; memcpy(w, p, 12);
    bool finite = true;
    for(int a = 0; a < 3; ++a) finite = finite && (w[a] & 0x7F800000u) != 0x7F800000u;
    if(!finite) w[0] = w[1] = w[2] = 0x7FC00000u;
    memcpy(out, w, 12);
}
}

void skin_vertex_host(const int32_t bone[4], const float weight[4], const float *xforms, const float in[3], float out[3]){
    static const float kIdentity[12] = { 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f };
    uint32_t wb[kSkinInfluences]; memcpy(wb, weight, sizeof wb);
    int active = 0, last = -1;
    bool all_identity = true;
    for(int j = 0; j < kSkinInfluences; ++j){
        if(wb[j] == 0u) continue;                          // inactive: its record is never looked at
        ++active; last = j;
        if(memcmp(xforms + (size_t) bone[j] * 12, kIdentity, sizeof kIdentity) != 0) all_identity = false;
    }
    if(all_identity){ memmove(out, in, 12); return; }      // keep: the vertex's bits
    const float x = in[0], y = in[1], z = in[2];
    float p[3];
    if(active == 1 && wb[last] == 0x3F800000u){            // rigid: a pose
        skin_rows(xforms + (size_t) bone[last] * 12, x, y, z, p);
        skin_finish(p, out);
        return;
    }
    float acc[3] = { 0.0f, 0.0f, 0.0f };
    bool first = true;
    for(int j = 0; j < kSkinInfluences; ++j){              // blend, index order
        if(wb[j] == 0u) continue;
        skin_rows(xforms + (size_t) bone[j] * 12, x, y, z, p);
        for(int a = 0; a < 3; ++a){
            const float m = weight[j] * p[a];
            acc[a] = first ? m : acc[a] + m;
        }
        first = false;
    }
    skin_finish(acc, out);
}

const char *skin_host_records(const void *tris_v, int nt, const int32_t *corner_bone, const float *corner_weight, const float *xforms,
                              int num_bones, void *out_v, char *msg, size_t msg_cap){
    const char *err = check_skin(corner_bone, corner_weight, nt, num_bones, msg, msg_cap);
    if(err && *err) return err;
    if(!xforms) return "null transform array";
    if(nt > 0 && (!tris_v || !out_v)) return "null triangle array";
    const unsigned char *tris = (const unsigned char *) tris_v;
    unsigned char *out = (unsigned char *) out_v;
    parallel_chunks((size_t) nt, [&](int, size_t b0, size_t e0){
        for(size_t i = b0; i < e0; ++i){
            if(out != tris) memcpy(out + i * sizeof(RefTriangle), tris + i * sizeof(RefTriangle), sizeof(RefTriangle));
            float v[9]; memcpy(v, out + i * sizeof(RefTriangle), 36);
            for(int k = 0; k < 3; ++k){
                const size_t at = (i * 3 + (size_t) k) * kSkinInfluences;
                skin_vertex_host(corner_bone + at, corner_weight + at, xforms, v + 3 * k, v + 3 * k);
            }
            memcpy(out + i * sizeof(RefTriangle), v, 36);
        }
    });
    return "";
}

const char *check_morphs(const int32_t *target_begin, const int32_t *entry_corner, const float *entry_delta, int num_entries, int nt,
                         int num_targets, char *msg, size_t msg_cap){
    if(nt < 0) return "negative triangle count";
    if(num_targets < 1 || num_targets > kMaxMorphTargets){
        snprintf(msg, msg_cap, "the number of morph targets must lie in [1, %d]: %d was given", kMaxMorphTargets, num_targets);
        return msg;
    }
    if(num_entries < 0) return "negative morph entry count";
    if(!target_begin) return "null target_begin array";
    if(num_entries > 0 && (!entry_corner || !entry_delta)) return "null morph entry array";
    if(target_begin[0] != 0){ snprintf(msg, msg_cap, "target_begin[0] must be 0: it is %d", target_begin[0]); return msg; }
    for(int t = 0; t < num_targets; ++t)
        if(target_begin[t + 1] < target_begin[t]){
            snprintf(msg, msg_cap, "target_begin decreases at target %d: %d follows %d", t, target_begin[t + 1], target_begin[t]);
            return msg;
        }
    if(target_begin[num_targets] != num_entries){
        snprintf(msg, msg_cap, "target_begin[%d] must be the number of entries, %d: it is %d", num_targets, num_entries, target_begin[num_targets]);
        return msg;
    }
    const int64_t corners = (int64_t) nt * 3;
    for(int t = 0; t < num_targets; ++t)
        for(int32_t e = target_begin[t]; e < target_begin[t + 1]; ++e){
            const int32_t c = entry_corner[e];
            if(c < 0 || (int64_t) c >= corners){
                snprintf(msg, msg_cap, "corner %d of target %d (entry %d) is not one of the %lld corners", c, t, e, (long long) corners);
                return msg;
            }
            if(e > target_begin[t] && c <= entry_corner[e - 1]){
                snprintf(msg, msg_cap, "the corners of target %d are not strictly ascending: entry %d names corner %d after corner %d", t, e, c, entry_corner[e - 1]);
                return msg;
            }
        }
    return "";
}

void transpose_morphs(const int32_t *target_begin, const int32_t *entry_corner, const float *entry_delta, int nt, int num_targets,
                      std::vector<uint32_t> &corner_begin, std::vector<MorphEntry> &entries){
    const size_t corners = (size_t) nt * 3, n = (size_t) target_begin[num_targets];
    corner_begin.assign(corners + 1, 0u);
    entries.resize(n);
    for(size_t e = 0; e < n; ++e) corner_begin[(size_t) entry_corner[e] + 1] += 1u;
    for(size_t c = 0; c < corners; ++c) corner_begin[c + 1] += corner_begin[c];
    std::vector<uint32_t> next(corner_begin.begin(), corner_begin.end() - 1);
    for(int t = 0; t < num_targets; ++t)               // ascending targets: a corner's entries come out in target order
        for(int32_t e = target_begin[t]; e < target_begin[t + 1]; ++e){
            MorphEntry &m = entries[next[(size_t) entry_corner[e]]++];
            m.target = (uint32_t) t;
            memcpy(&m.dx, entry_delta + (size_t) e * 3, 12);
        }
}

namespace {
inline bool morph_active(float w){ uint32_t b; memcpy(&b, &w, 4); return (b << 1) != 0u; }
}

void morph_vertex_host(const MorphEntry *entries, size_t count, const float *weights, const float in[3], float out[3]){
    float acc[3]; memcpy(acc, in, 12);
    bool any = false;
    for(size_t e = 0; e < count; ++e){
        const float w = weights[entries[e].target];
        if(!morph_active(w)) continue;                     // inactive: its deltas are never looked at
        const float d[3] = { entries[e].dx, entries[e].dy, entries[e].dz };
        for(int a = 0; a < 3; ++a){
            const float m = w * d[a];
            acc[a] = acc[a] + m;
        }
        any = true;
    }
    if(!any){ memmove(out, in, 12); return; }             // keep: the vertex's bits
    skin_finish(acc, out);
}

const char *morph_host_records(const void *tris_v, int nt, const int32_t *target_begin, const int32_t *entry_corner, const float *entry_delta,
                               int num_entries, int num_targets, const float *weights, void *out_v, char *msg, size_t msg_cap){
    const char *err = check_morphs(target_begin, entry_corner, entry_delta, num_entries, nt, num_targets, msg, msg_cap);
    if(err && *err) return err;
    if(!weights) return "null weight array";
    if(nt > 0 && (!tris_v || !out_v)) return "null triangle array";
    const unsigned char *tris = (const unsigned char *) tris_v;
    unsigned char *out = (unsigned char *) out_v;
    // the definition as the caller's layout has it: target after target, ascending, each over its own ascending corners; a
    // chunk of triangles finds its run of a target's entries by bisection
    parallel_chunks((size_t) nt, [&](int, size_t b0, size_t e0){
        if(out != tris) memcpy(out + b0 * sizeof(RefTriangle), tris + b0 * sizeof(RefTriangle), (e0 - b0) * sizeof(RefTriangle));
        std::vector<unsigned char> touched((e0 - b0) * 3, 0);
        const int32_t c0 = (int32_t) (b0 * 3), c1 = (int32_t) (e0 * 3);
        for(int t = 0; t < num_targets; ++t){
            const float w = weights[t];
            if(!morph_active(w)) continue;
            const int32_t *first = entry_corner + target_begin[t], *last = entry_corner + target_begin[t + 1];
            for(const int32_t *p = std::lower_bound(first, last, c0); p < last && *p < c1; ++p){
                const size_t c = (size_t) *p;
                unsigned char *at = out + (c / 3) * sizeof(RefTriangle) + (c % 3) * 12;
                const float *d = entry_delta + (size_t) (p - entry_corner) * 3;
                float acc[3]; memcpy(acc, at, 12);
                for(int a = 0; a < 3; ++a){
                    const float m = w * d[a];
                    acc[a] = acc[a] + m;
                }
                memcpy(at, acc, 12);
                touched[c - (size_t) c0] = 1;
            }
        }
        for(size_t c = 0; c < touched.size(); ++c) if(touched[c]){
            unsigned char *at = out + (((size_t) c0 + c) / 3) * sizeof(RefTriangle) + (((size_t) c0 + c) % 3) * 12;
            float acc[3]; memcpy(acc, at, 12);
            skin_finish(acc, acc);
            memcpy(at, acc, 12);
        }
    });
    return "";
}

const char *check_rounds_update(const void *kept_spheres_v, int kept_ns, int kept_nl, const void *lights_v, int nl, const void *spheres_v, int ns,
                                char *msg, size_t msg_cap){
    if(nl < 0 || ns < 0) return "negative primitive count";
    if(nl != kept_nl || ns != kept_ns){ snprintf(msg, msg_cap, "an update keeps the counts: the scene has %d lights and %d spheres, %d and %d were handed over", kept_nl, kept_ns, nl, ns); return msg; }
    if((nl > 0 && !lights_v) || (ns > 0 && !spheres_v)) return "null primitive array";
    const RefSphere *kept = (const RefSphere *) kept_spheres_v, *spheres = (const RefSphere *) spheres_v;
    for(int i = 0; i < ns; ++i)
        if(memcmp(&kept[i].o, &spheres[i].o, sizeof(RefSphere) - offsetof(RefSphere, o)) != 0){
            snprintf(msg, msg_cap, "an update moves spheres only: material or id bytes of sphere %d differ from the record the scene was created from", i);
            return msg;
        }
    return "";
}

const char *refit_host_scene(HostScene &hs, const void *tris_v, int nt, uint64_t *dead_out){
    if(nt != hs.num_tris) return "an update keeps the triangle count";
    if(nt > 0 && !tris_v) return "null triangle array";
    if(hs.level_begin.size() < 2 || hs.wide_src.size() != hs.wnodes.size() * 4) return "internal error: the scene keeps no refit tables";
    const RefTriangle *tris = (const RefTriangle *) tris_v;
    const uint32_t num_rounds = (uint32_t) (hs.num_spheres + hs.num_lights);
    // 1. liveness and boxes per triangle, input order
    pod_vector<Box> tb((size_t) nt);
    Box scene_box;
    const size_t ndead = triangle_boxes(tris, nt, scene_box, [&](size_t i, const Box &b, bool){ tb[i] = b; });
    if(dead_out) *dead_out = ndead;
    const float pad_abs = box_padding(scene_box, nt);
    // 2. the leaf-order records: a slot keeps its triangle (ordinal, material, flags)
    parallel_chunks((size_t) nt, [&](int, size_t b0, size_t e0){
        for(size_t s = b0; s < e0; ++s) triangle_geometry(hs.tris[s], tris[hs.tris[s].ordinal - num_rounds]);
    });
    // 3. node boxes, deepest level first (children sit behind their parents): a child's exact box is the union of its
    // triangles' boxes, what the node stores is that box padded -- never a padded box padded again
    pod_vector<Box> exact(hs.nodes.size());
    for(size_t l = hs.level_begin.size() - 1; l-- > 0; ){
        const size_t first = hs.level_begin[l], cnt = hs.level_begin[l + 1] - first;
        parallel_chunks(cnt, [&](int, size_t b0, size_t e0){
            for(size_t i = first + b0; i < first + e0; ++i){
                BvhNode &n = hs.nodes[i];
                Box both; both.reset();
                for(int side = 0; side < 2; ++side){
                    const uint32_t code = side ? n.right : n.left;
                    float *mn = side ? n.rmin : n.lmin, *mx = side ? n.rmax : n.lmax;
                    if(code == kEmptyChild){ set_empty_box(mn, mx); continue; }
                    Box cb;
                    if(code & kLeafFlag){
                        cb.reset();
                        const uint32_t s0 = (code & ~kLeafFlag) >> 3, c = (code & 7u) + 1u;
                        for(uint32_t s = s0; s < s0 + c; ++s) cb.grow(tb[hs.tris[s].ordinal - num_rounds]);
                    } else cb = exact[code];
                    write_padded_box(mn, mx, cb, pad_abs);
                    both.grow(cb);
                }
                exact[i] = both;
            }
        });
    }
    // 4. the grid and the two quantised trees
    quantise_tree(hs);
    pack_wide_boxes(hs);
    return "";
}

const char *build_host_scene(const void *lights_v, int nl, const void *spheres_v, int ns,
                             const void *tris_v, int nt, HostScene &hs){
    if(nl < 0 || ns < 0 || nt < 0) return "negative primitive count";
    if((nl > 0 && !lights_v) || (ns > 0 && !spheres_v) || (nt > 0 && !tris_v)) return "null primitive array";
    if((uint64_t) nt >= (1ull << 28)) return "too many triangles (limit 2^28)";
    const RefSphere *spheres = (const RefSphere *) spheres_v;
    const RefTriangle *tris = (const RefTriangle *) tris_v;

    hs = HostScene();
    hs.num_spheres = ns; hs.num_lights = nl; hs.num_tris = nt;
    std::map<MatKey, uint32_t> mat_table;

    {   // spheres take the first material numbers, in input order
        std::vector<uint32_t> sphere_material((size_t) ns);
        for(int i = 0; i < ns; ++i) sphere_material[(size_t) i] = intern_material(spheres[i].m, mat_table, hs.materials);
        const char *e = flatten_rounds_host(lights_v, nl, spheres_v, ns, sphere_material.data(), hs.rounds, hs.lights);
        if(e && *e) return e;
    }

    auto t0 = std::chrono::steady_clock::now();
#ifdef HPT_DEV_TUNING
    auto tp = t0;
    auto lap = [&](const char *what){ auto n = std::chrono::steady_clock::now(); fprintf(stderr, "  build phase %-12s %.1f ms\n", what, std::chrono::duration<double, std::milli>(n - tp).count()); tp = n; };
#else
    auto lap = [](const char *){};
#endif
    Builder B;
#ifdef HPT_DEV_TUNING      // development builds only (`make variant EXTRA=-DHPT_DEV_TUNING`, scripts/sweep_leaf.py): the product reads no environment here
    if(const char *e = getenv("HPT_MAX_LEAF")){ int v = atoi(e); if(v >= 1 && v <= 8) B.max_leaf = v; }
#endif
    B.prims.resize(nt);
    // (dead triangles enter as a point: triangle_boxes)
    Box scene_box;
    triangle_boxes(tris, nt, scene_box, [&](size_t i, const Box &b, bool live){
        Prim &p = B.prims[i];
        p.index = (uint32_t) i;
        p.box = b;
        for(int a = 0; a < 3; ++a) p.cen[a] = live ? 0.5f * (b.mn[a] + b.mx[a]) : b.mn[a];
    });
    B.pad_abs = box_padding(scene_box, nt);
    B.nodes.resize((nt > 0 ? (size_t) nt : 1) + Builder::kSlotSlack);          // an inner node has two non-empty subtrees: fewer than nt of them
    lap("prims");

    if(nt == 0){
        BvhNode n; memset(&n, 0, sizeof n);
        set_empty_box(n.lmin, n.lmax); set_empty_box(n.rmin, n.rmax);
        n.left = n.right = kEmptyChild;
        B.nodes[0] = n; B.next_node = 1;
    } else if(nt <= B.max_leaf){
        BvhNode n; memset(&n, 0, sizeof n);
        B.nodes[0] = n; B.next_node = 1;
        Box lb;
        uint32_t lc = B.build(0, nt, 1, lb);
        B.write_box(B.nodes[0].lmin, B.nodes[0].lmax, lb); B.nodes[0].left = lc;
        set_empty_box(B.nodes[0].rmin, B.nodes[0].rmax); B.nodes[0].right = kEmptyChild;
    } else {
        Box rb;
        uint32_t root = B.build(0, nt, 0, rb);
        if(root != 0) return "internal error: BVH root is not node 0";
    }
    lap("tree");
    B.nodes.resize(B.next_node.load());
    hs.nodes.swap(B.nodes);
    hs.bvh_depth = B.max_depth_seen.load();
    {   // breadth-first renumbering: node 0 stays the root and every node of depth d precedes every node of depth d + 1,
        // so the nodes a ray can reach in its first k steps are the first 2^k - 1 at most (k_trace keeps those in LDS)
        const size_t n = hs.nodes.size();
        pod_vector<uint32_t> order(n);
        pod_vector<uint32_t> new_index(n);
        auto inner = [](uint32_t c){ return c != kEmptyChild && !(c & kLeafFlag); };
        // level by level: the inner children of a level, in order, are the next level; a level is cut into chunks that count
        // their children, a prefix sum places them, and the chunks fill their part
        size_t lvl_begin = 0, lvl_end = 1;
        order[0] = 0u;
        while(lvl_begin < lvl_end){
            hs.level_begin.push_back((uint32_t) lvl_begin);
            const size_t cnt = lvl_end - lvl_begin;
            size_t per_chunk[kChunks] = {};
            parallel_chunks(cnt, [&](int c, size_t b0, size_t e0){
                size_t k = 0;
                for(size_t i = b0; i < e0; ++i){ const BvhNode &nd = hs.nodes[order[lvl_begin + i]]; k += (inner(nd.left) ? 1u : 0u) + (inner(nd.right) ? 1u : 0u); }
                per_chunk[c] = k;
            });
            size_t offs[kChunks], total = 0;
            for(int c = 0; c < kChunks; ++c){ offs[c] = total; total += per_chunk[c]; }
            if(lvl_end + total > n) return "internal error: BVH has more reachable nodes than slots";
            parallel_chunks(cnt, [&](int c, size_t b0, size_t e0){
                size_t o = lvl_end + offs[c];
                for(size_t i = b0; i < e0; ++i){
                    const BvhNode &nd = hs.nodes[order[lvl_begin + i]];
                    if(inner(nd.left)){ new_index[nd.left] = (uint32_t) o; order[o++] = nd.left; }
                    if(inner(nd.right)){ new_index[nd.right] = (uint32_t) o; order[o++] = nd.right; }
                }
            });
            lvl_begin = lvl_end; lvl_end += total;
        }
        hs.level_begin.push_back((uint32_t) lvl_end);
        order.resize(lvl_end);
        // (slots a build thread reserved and did not use are not reachable and drop out here)
        const size_t reachable = order.size();
        pod_vector<BvhNode> sorted(reachable);
        parallel_chunks(reachable, [&](int, size_t b0, size_t e0){
            for(size_t i = b0; i < e0; ++i){
                BvhNode nd = hs.nodes[order[i]];
                if(nd.left != kEmptyChild && !(nd.left & kLeafFlag)) nd.left = new_index[nd.left];
                if(nd.right != kEmptyChild && !(nd.right & kLeafFlag)) nd.right = new_index[nd.right];
                sorted[i] = nd;
            }
        });
        hs.nodes.swap(sorted);
    }
    lap("renumber");
    quantise_tree(hs);
    if(hs.bvh_depth > kMaxBvhDepth) return "internal error: BVH deeper than the traversal stack";
    lap("quantise");
    collapse_wide(hs);

    lap("wide");
    hs.tris.resize(nt);
    pod_vector<uint32_t> mat_of((size_t) nt);
    triangle_materials(tris, nt, mat_table, hs.materials, mat_of);
    parallel_chunks((size_t) nt, [&](int, size_t b0, size_t e0){
        for(size_t s = b0; s < e0; ++s){
            const RefTriangle &t = tris[B.prims[s].index];        // leaf order = the order the build left the primitives in
            DevTriangle &d = hs.tris[s];
            triangle_geometry(d, t);
            d.ordinal = (uint32_t) (ns + nl) + B.prims[s].index;
            d.material = mat_of[B.prims[s].index];
            d.flags = (t.m.eta <= 0.0f) ? 1u : 0u;
        }
    });
    lap("triangles");
    auto t1 = std::chrono::steady_clock::now();
    hs.ms_bvh_build = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if(hs.materials.empty()) hs.materials.push_back(blank_material());
    return "";
}

namespace {

// materials are numbered in order of first appearance in the INPUT (spheres, then triangles as handed over): one sequential
// pass over the records that mostly hits its one-entry cache; the leaf-order fill looks the numbers up in mat_of
void triangle_materials(const RefTriangle *tris, int nt, std::map<MatKey, uint32_t> &mat_table, std::vector<DevMaterial> &materials,
                        pod_vector<uint32_t> &mat_of){
    RefMat last; memset(&last, 0xFF, sizeof last); uint32_t last_idx = 0; bool have = false;
    for(int i = 0; i < nt; ++i){
        const RefMat &m = tris[i].m;
        if(!have || memcmp(&m, &last, 28) != 0){ last_idx = intern_material(m, mat_table, materials); last = m; have = true; }
        mat_of[(size_t) i] = last_idx;
    }
}

// four-wide twin: greedy collapse of the binary tree hs.nodes (stored float boxes and child codes), breadth-first numbering,
// same quantised child boxes; fills wnodes, wide_src and wide_depth.  build_host_scene and lbvh_host_scene run these lines.
void collapse_wide(HostScene &hs){
    hs.wide_depth = 0;
    {
        struct Kid { const float *mn, *mx; uint32_t code, src; };      // src: binary node * 2 + side, what a refit reads the box from
        auto half_area = [](const Kid &k){ float dx = k.mx[0] - k.mn[0], dy = k.mx[1] - k.mn[1], dz = k.mx[2] - k.mn[2]; return dx * dy + dy * dz + dz * dx; };
        struct Kids { Kid k[4]; int n; uint32_t code[4]; };
        pod_vector<uint32_t> todo(hs.nodes.size() + 1);             // binary node each wide node was collapsed from (breadth-first)
        pod_vector<Kids> all(hs.nodes.size() + 1);
        todo[0] = 0u;
        // pass 1, level by level: which child boxes a wide node holds; the inner ones among them are the next level (a chunk of
        // the level counts its own, a prefix sum gives them their numbers)
        size_t lvl_begin = 0, lvl_end = 1;
        while(lvl_begin < lvl_end){
            const size_t cnt = lvl_end - lvl_begin;
            size_t per_chunk[kChunks] = {};
            parallel_chunks(cnt, [&](int c, size_t b0, size_t e0){
                size_t inner_kids = 0;
                for(size_t i = b0; i < e0; ++i){
                    Kids ks; ks.n = 0;
                    auto open = [&](uint32_t idx){
                        const BvhNode &b = hs.nodes[idx];
                        if(b.left != kEmptyChild) ks.k[ks.n++] = Kid{ b.lmin, b.lmax, b.left, idx * 2u };
                        if(b.right != kEmptyChild) ks.k[ks.n++] = Kid{ b.rmin, b.rmax, b.right, idx * 2u + 1u };
                    };
                    open(todo[lvl_begin + i]);
                    while(ks.n < 4){
                        int best = -1; float ba = -1.0f;
                        for(int k = 0; k < ks.n; ++k) if(!(ks.k[k].code & kLeafFlag)){ float a = half_area(ks.k[k]); if(a > ba){ ba = a; best = k; } }
                        if(best < 0) break;
                        // an inner binary node has two children at most: opening one replaces it by them (n grows by one at most)
                        uint32_t cc = ks.k[best].code;
                        ks.k[best] = ks.k[ks.n - 1]; --ks.n;
                        open(cc);
                    }
                    for(int k = 0; k < ks.n; ++k) if(!(ks.k[k].code & kLeafFlag)) ++inner_kids;
                    all[lvl_begin + i] = ks;
                }
                per_chunk[c] = inner_kids;
            });
            size_t offs[kChunks], total = 0;
            for(int c = 0; c < kChunks; ++c){ offs[c] = total; total += per_chunk[c]; }
            parallel_chunks(cnt, [&](int c, size_t b0, size_t e0){
                size_t o = lvl_end + offs[c];
                for(size_t i = b0; i < e0; ++i){
                    Kids &ks = all[lvl_begin + i];
                    for(int k = 0; k < 4; ++k){
                        if(k >= ks.n) ks.code[k] = kEmptyChild;
                        else if(ks.k[k].code & kLeafFlag) ks.code[k] = ks.k[k].code;
                        else { ks.code[k] = (uint32_t) o; todo[o++] = ks.k[k].code; }
                    }
                }
            });
            ++hs.wide_depth;
            lvl_begin = lvl_end; lvl_end += total;
        }
        all.resize(lvl_end);
        // pass 2: the child codes and where each child's box comes from, then quantise and pack
        hs.wnodes.resize(all.size());
        hs.wide_src.resize(all.size() * 4);
        parallel_chunks(all.size(), [&](int, size_t b0, size_t e0){
            for(size_t qi = b0; qi < e0; ++qi){
                const Kids &ks = all[qi];
                for(int k = 0; k < 4; ++k){
                    hs.wnodes[qi].w[12 + k] = ks.code[k];
                    hs.wide_src[qi * 4 + (size_t) k] = k < ks.n ? ks.k[k].src : kEmptyChild;
                }
            }
        });
        pack_wide_boxes(hs);
    }
}

// ---- device builds (include/hpt.h, "device builds"): the Morton-order linear BVH the device builds, restated on the host ----

// cell of a centroid on one axis, 21 bits: Builder::bin_of's shape -- the comparisons first, so a NaN goes to cell 0 and
// nothing out of range is converted
inline uint32_t lbvh_cell(float cen, float lo, float scale){
    const float f = (cen - lo) * scale;
    return f >= 1.0f ? (f < 2097152.0f ? (uint32_t) f : 2097151u) : 0u;
}
// bit k of a 21-bit cell to bit 3 * k
inline uint64_t lbvh_spread(uint32_t v){
    uint64_t x = v & 0x1FFFFFu;
    x = (x | x << 32) & 0x001F00000000FFFFull;
    x = (x | x << 16) & 0x001F0000FF0000FFull;
    x = (x | x << 8) & 0x100F00F00F00F00Full;
    x = (x | x << 4) & 0x10C30C30C30C30C3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// common-prefix length of the sorted pairs at positions i and j (-1 when j lies outside): of the 64-bit keys, and for equal
// keys 64 plus that of the positions as 32-bit words
inline int lbvh_delta(const uint64_t *keys, int64_t n, int64_t i, int64_t j){
    if(j < 0 || j >= n) return -1;
    const uint64_t x = keys[i] ^ keys[j];
    if(x) return __builtin_clzll(x);
    return 64 + __builtin_clz((uint32_t) i ^ (uint32_t) j);
}

// What lbvh_host_scene and lbvh_bounded_host_scene share ahead of the topology: materials, rounds and lights, the keys, the
// stable order and the leaf records in it.  keys: the sorted keys, one per leaf slot.
const char *lbvh_sorted_leaves(const void *lights_v, int nl, const void *spheres_v, int ns, const void *tris_v, int nt, HostScene &hs,
                               std::vector<uint64_t> &keys){
    if(nl < 0 || ns < 0 || nt < 0) return "negative primitive count";
    if((nl > 0 && !lights_v) || (ns > 0 && !spheres_v) || (nt > 0 && !tris_v)) return "null primitive array";
    if((uint64_t) nt >= (1ull << 28)) return "too many triangles (limit 2^28)";
    const RefSphere *spheres = (const RefSphere *) spheres_v;
    const RefTriangle *tris = (const RefTriangle *) tris_v;

    hs = HostScene();
    hs.num_spheres = ns; hs.num_lights = nl; hs.num_tris = nt;
    std::map<MatKey, uint32_t> mat_table;
    {   std::vector<uint32_t> sphere_material((size_t) ns);
        for(int i = 0; i < ns; ++i) sphere_material[(size_t) i] = intern_material(spheres[i].m, mat_table, hs.materials);
        const char *e = flatten_rounds_host(lights_v, nl, spheres_v, ns, sphere_material.data(), hs.rounds, hs.lights);
        if(e && *e) return e;
    }
    pod_vector<uint32_t> mat_of((size_t) nt);
    triangle_materials(tris, nt, mat_table, hs.materials, mat_of);
    if(hs.materials.empty()) hs.materials.push_back(blank_material());

    // keys: liveness and boxes are triangle_boxes'; the cells lie on the live triangles' box
    const size_t n = (size_t) nt;
    pod_vector<Box> tb(n);
    std::vector<unsigned char> live(n, 0);
    Box scene_box;
    triangle_boxes(tris, nt, scene_box, [&](size_t i, const Box &b, bool l){ tb[i] = b; live[i] = l ? 1 : 0; });
    float scale[3];
    for(int a = 0; a < 3; ++a){ const float ext = scene_box.mx[a] - scene_box.mn[a]; scale[a] = ext > 0.0f ? 2097152.0f / ext : 0.0f; }
    std::vector<uint64_t> key_of(n);
    for(size_t i = 0; i < n; ++i){
        if(!live[i]){ key_of[i] = ~0ull; continue; }
        uint32_t cell[3];
        for(int a = 0; a < 3; ++a){ const float c = 0.5f * (tb[i].mn[a] + tb[i].mx[a]); cell[a] = lbvh_cell(c, scene_box.mn[a], scale[a]); }
        key_of[i] = lbvh_spread(cell[0]) << 2 | lbvh_spread(cell[1]) << 1 | lbvh_spread(cell[2]);
    }
    // order: ascending key, ties by input index; the sorted position is the leaf slot
    std::vector<uint32_t> order(n);
    for(size_t i = 0; i < n; ++i) order[i] = (uint32_t) i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b){ return key_of[a] < key_of[b]; });
    keys.resize(n);
    hs.tris.resize(n);
    for(size_t s = 0; s < n; ++s){
        const uint32_t i = order[s];
        keys[s] = key_of[i];
        DevTriangle &d = hs.tris[s];
        triangle_geometry(d, tris[i]);
        d.ordinal = (uint32_t) (ns + nl) + i;
        d.material = mat_of[i];
        d.flags = (tris[i].m.eta <= 0.0f) ? 1u : 0u;
    }
    return "";
}

inline uint32_t lbvh_leaf_code(int64_t first, int64_t count){ return kLeafFlag | ((uint32_t) first << 3) | (uint32_t) (count - 1); }

// the trees of kMaxLeafTris triangles or fewer: one node
void lbvh_one_node(HostScene &hs, int nt){
    BvhNode blank; memset(&blank, 0, sizeof blank);
    hs.nodes.assign(1, blank);
    hs.nodes[0].left = nt > 0 ? lbvh_leaf_code(0, nt) : kEmptyChild;
    hs.nodes[0].right = kEmptyChild;
    hs.level_begin = { 0u, 1u };
    hs.bvh_depth = nt > 0 ? 1 : 0;
}

// numbering: breadth-first, build_host_scene's rule -- level by level, within a level the inner children in order, left
// before right; nodes no child code names drop out.  rl, rr: the child codes of every node in the topology's own numbering
// (node 0 is the root; an inner child is the number of its node there).
void lbvh_number(HostScene &hs, const std::vector<uint32_t> &rl, const std::vector<uint32_t> &rr){
    BvhNode blank; memset(&blank, 0, sizeof blank);
    std::vector<uint32_t> from(1, 0u);               // the topology's number of every node, breadth-first
    size_t lvl_begin = 0, lvl_end = 1;
    while(lvl_begin < lvl_end){
        hs.level_begin.push_back((uint32_t) lvl_begin);
        for(size_t q = lvl_begin; q < lvl_end; ++q){
            BvhNode nd = blank;
            const uint32_t c[2] = { rl[from[q]], rr[from[q]] };
            uint32_t out[2];
            for(int side = 0; side < 2; ++side){
                if(c[side] & kLeafFlag){ out[side] = c[side]; continue; }
                out[side] = (uint32_t) from.size();
                from.push_back(c[side]);
            }
            nd.left = out[0]; nd.right = out[1];
            hs.nodes.push_back(nd);
        }
        lvl_begin = lvl_end; lvl_end = from.size();
    }
    hs.level_begin.push_back((uint32_t) lvl_end);
    hs.bvh_depth = (int) hs.level_begin.size() - 1;       // the builder's count: the deepest leaf's depth, root = 0
}

// everything that is a function of the vertex positions: the refit's own lines, then the collapse over the boxes it wrote
const char *lbvh_boxes(HostScene &hs, const void *tris_v, int nt, std::chrono::steady_clock::time_point t0){
    const char *e = refit_host_scene(hs, tris_v, nt);
    if(e && *e) return e;
    collapse_wide(hs);
    hs.ms_bvh_build = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return "";
}

} // namespace

const char *lbvh_host_scene(const void *lights_v, int nl, const void *spheres_v, int ns, const void *tris_v, int nt, HostScene &hs){
    auto t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> keys;
    if(const char *e = lbvh_sorted_leaves(lights_v, nl, spheres_v, ns, tris_v, nt, hs, keys); e && *e) return e;
    const size_t n = (size_t) nt;

    // topology: the binary radix tree over the sorted pairs; child codes in radix numbering (inner node k splits its range
    // behind position gamma: the left child is inner node gamma, the right one gamma + 1, a range of kMaxLeafTris or fewer a leaf)
    if(nt <= kMaxLeafTris) lbvh_one_node(hs, nt);
    else {
        const int64_t N = (int64_t) nt;
        std::vector<uint32_t> rl(n - 1), rr(n - 1);
        for(int64_t i = 0; i < N - 1; ++i){
            const uint64_t *k = keys.data();
            const int64_t d = lbvh_delta(k, N, i, i + 1) > lbvh_delta(k, N, i, i - 1) ? 1 : -1;
            const int dmin = lbvh_delta(k, N, i, i - d);
            int64_t lmax = 2;
            while(lbvh_delta(k, N, i, i + lmax * d) > dmin) lmax *= 2;
            int64_t l = 0;
            for(int64_t t = lmax / 2; t >= 1; t /= 2) if(lbvh_delta(k, N, i, i + (l + t) * d) > dmin) l += t;
            const int64_t j = i + l * d;
            const int dnode = lbvh_delta(k, N, i, j);
            int64_t s = 0;
            for(int64_t t = (l + 1) / 2; ; t = (t + 1) / 2){
                if(lbvh_delta(k, N, i, i + (s + t) * d) > dnode) s += t;
                if(t <= 1) break;
            }
            const int64_t gamma = i + s * d + std::min<int64_t>(d, 0);
            const int64_t first = std::min(i, j), last = std::max(i, j);
            const int64_t lc = gamma - first + 1, rc = last - gamma;
            rl[(size_t) i] = lc <= kMaxLeafTris ? lbvh_leaf_code(first, lc) : (uint32_t) gamma;
            rr[(size_t) i] = rc <= kMaxLeafTris ? lbvh_leaf_code(gamma + 1, rc) : (uint32_t) (gamma + 1);
        }
        lbvh_number(hs, rl, rr);
    }
    return lbvh_boxes(hs, tris_v, nt, t0);
}

// ---- bounded device builds (include/hpt.h, "bounded device builds") --------------------------------------------------------

int lbvh_need(int64_t count){
    const int64_t leaves = (count + 1) / 2;
    int k = 1;
    while((1ll << k) < leaves) ++k;
    return k;
}

const char *lbvh_check_depth(int nt, int max_depth, int &effective, char *msg, size_t msg_cap){
    effective = max_depth == 0 ? kMaxBvhDepth : max_depth;
    const int need = lbvh_need(nt < 0 ? 0 : nt);
    if(max_depth < 0 || max_depth > kMaxBvhDepth || effective < need){
        snprintf(msg, msg_cap, "max_depth %d: must be 0 (the limit, %d) or lie in [%d, %d] for %d triangles", max_depth, kMaxBvhDepth, need, kMaxBvhDepth, nt);
        return msg;
    }
    return "";
}

const char *lbvh_bounded_host_scene(const void *lights_v, int nl, const void *spheres_v, int ns, const void *tris_v, int nt, int max_depth,
                                    HostScene &hs, BoundedInfo &bi){
    static thread_local char msg[160];
    auto t0 = std::chrono::steady_clock::now();
    bi = BoundedInfo();
    if(nt >= 0 && (uint64_t) nt < (1ull << 28)){          // (the other counts are refused below, in the shared lines)
        int D = 0;
        if(const char *e = lbvh_check_depth(nt, max_depth, D, msg, sizeof msg); *e) return e;
        bi.max_depth = (uint32_t) D;
    }
    std::vector<uint64_t> keys;
    if(const char *e = lbvh_sorted_leaves(lights_v, nl, spheres_v, ns, tris_v, nt, hs, keys); e && *e) return e;
    const int D = (int) bi.max_depth;

    // topology, top-down: a node is its range of sorted positions and its level; nodes are numbered as they are made
    if(nt <= kMaxLeafTris) lbvh_one_node(hs, nt);
    else {
        struct Range { int64_t first, count; int level; };
        std::vector<Range> todo(1, Range{ 0, (int64_t) nt, 0 });
        std::vector<uint32_t> rl, rr;
        const uint64_t *k = keys.data();
        const int64_t N = (int64_t) nt;
        for(size_t q = 0; q < todo.size(); ++q){
            const Range r = todo[q];
            const int64_t leaves = (r.count + 1) / 2;
            int64_t lc;
            if(lbvh_need(r.count) >= D - r.level){         // forced: full leaves, the left half rounded up
                lc = 2 * ((leaves + 1) / 2);
                bi.forced_nodes += 1;
                if(bi.first_forced_level == 0xFFFFFFFFu) bi.first_forced_level = (uint32_t) r.level;
            } else {                                       // Karras' split of the range: delta(first, p) does not increase with p
                const int64_t last = r.first + r.count - 1;
                const int dnode = lbvh_delta(k, N, r.first, last);
                int64_t lo = r.first, hi = last;           // delta(first, lo) > dnode >= delta(first, hi)
                while(hi - lo > 1){
                    const int64_t mid = lo + (hi - lo) / 2;
                    if(lbvh_delta(k, N, r.first, mid) > dnode) lo = mid; else hi = mid;
                }
                lc = lo - r.first + 1;
            }
            const int64_t rc = r.count - lc;
            uint32_t code[2];
            const int64_t cf[2] = { r.first, r.first + lc }, cc[2] = { lc, rc };
            for(int side = 0; side < 2; ++side){
                if(cc[side] <= kMaxLeafTris){ code[side] = lbvh_leaf_code(cf[side], cc[side]); continue; }
                code[side] = (uint32_t) todo.size();
                todo.push_back(Range{ cf[side], cc[side], r.level + 1 });
            }
            rl.push_back(code[0]); rr.push_back(code[1]);
        }
        lbvh_number(hs, rl, rr);
    }
    return lbvh_boxes(hs, tris_v, nt, t0);
}

// ---- tree cost (include/hpt.h, "tree cost") --------------------------------------------------------------------------------

void tree_cost_sums_host(const QBvhNode *q, uint32_t num_nodes, hpt_tree_cost &out){
    memset(&out, 0, sizeof out);
    out.num_nodes = num_nodes;
    for(uint32_t i = 0; i < num_nodes; ++i){
        const QBvhNode &n = q[i];
        uint32_t rlo[3] = { 0xFFFFu, 0xFFFFu, 0xFFFFu }, rhi[3] = { 0u, 0u, 0u };
        bool any = false;
        for(int c = 0; c < 2; ++c){
            const uint32_t code = c ? n.right : n.left;
            if(code == kEmptyChild){ out.empty_children += 1; continue; }
            uint64_t d[3];
            for(int a = 0; a < 3; ++a){
                const uint32_t lo = n.plane[a][0][c], hi = n.plane[a][1][c];
                d[a] = hi >= lo ? hi - lo : 0u;
                rlo[a] = std::min(rlo[a], lo); rhi[a] = std::max(rhi[a], hi);
            }
            any = true;
            if(code & kLeafFlag){
                const uint64_t k = (code & 7u) + 1u;
                out.leaf_children += 1; out.leaf_slots += k;
                out.leaf_xy += k * d[0] * d[1]; out.leaf_yz += k * d[1] * d[2]; out.leaf_zx += k * d[2] * d[0];
            } else {
                out.inner_children += 1;
                out.inner_xy += d[0] * d[1]; out.inner_yz += d[1] * d[2]; out.inner_zx += d[2] * d[0];
            }
        }
        if(i == 0) for(int a = 0; a < 3; ++a) out.root_extent[a] = any && rhi[a] >= rlo[a] ? rhi[a] - rlo[a] : 0u;
    }
}

void tree_cost_compose(const float qscale[3], hpt_tree_cost &c){
    const double Axy = (double) qscale[0] * (double) qscale[1], Ayz = (double) qscale[1] * (double) qscale[2], Azx = (double) qscale[2] * (double) qscale[0];
    const double rx = (double) c.root_extent[0], ry = (double) c.root_extent[1], rz = (double) c.root_extent[2];
    const double root_area = rx * ry * Axy + ry * rz * Ayz + rz * rx * Azx;
    c.box_visits = c.tri_tests = c.sah = 0.0;
    if(!(root_area > 0.0)) return;
    c.box_visits = 1.0 + ((double) c.inner_xy * Axy + (double) c.inner_yz * Ayz + (double) c.inner_zx * Azx) / root_area;
    c.tri_tests = ((double) c.leaf_xy * Axy + (double) c.leaf_yz * Ayz + (double) c.leaf_zx * Azx) / root_area;
    c.sah = 2.0 * c.box_visits + c.tri_tests;
}


const char *build_bdpt_host_scene(const void *lights_v, int nl, const void *spheres_v, int ns, const void *tris_v, int nt,
                                  const int32_t *obj_kind, const int32_t *obj_index, const int32_t *obj_group, int nobj,
                                  HostBdptScene &out){
    if(nl < 0 || ns < 0 || nt < 0) return "negative primitive count";
    if((nl > 0 && !lights_v) || (ns > 0 && !spheres_v) || (nt > 0 && !tris_v)) return "null primitive array";
    const RefSphere *spheres = (const RefSphere *) spheres_v;
    const RefTriangle *tris = (const RefTriangle *) tris_v;
    out = HostBdptScene();
    {   // the light records are the PT path's
        HostScene tmp;
        const char *e = build_host_scene(lights_v, nl, nullptr, 0, nullptr, 0, tmp);
        if(e && *e) return e;
        out.lights = tmp.lights;
    }
    struct Item { int kind, index; uint32_t seq; };
    std::map<int, std::vector<Item>> gm;
    uint32_t seq = 0;
    if(obj_kind && obj_index && obj_group){
        // sequence numbers follow the CPU renderer's iteration order: groups in map order, objects in insertion order
        for(int i = 0; i < nobj; ++i){
            if(obj_kind[i] == 0 ? (obj_index[i] < 0 || obj_index[i] >= ns) : (obj_index[i] < 0 || obj_index[i] >= nt)) return "object index out of range";
            gm[obj_group[i]].push_back(Item{ obj_kind[i], obj_index[i], 0u });
        }
    } else {
        for(int i = 0; i < ns; ++i) gm[0].push_back(Item{ 0, i, 0u });
        for(int i = 0; i < nt; ++i) gm[0].push_back(Item{ 1, i, 0u });
    }
    for(auto &kv : gm) for(Item &it : kv.second) it.seq = seq++;

    std::map<MatKey, uint32_t> mat_table;
    Box scene_box; scene_box.reset();
    std::vector<Box> gboxes;
    for(auto &kv : gm){
        Box gb; for(int a = 0; a < 3; ++a){ gb.mn[a] = 99999.f; gb.mx[a] = -99999.f; }       // AABB::add_obj, src/object.cpp:123-146
        for(const Item &it : kv.second){
            if(it.kind == 0){
                const RefSphere &s = spheres[it.index];
                for(int a = 0; a < 3; ++a){
                    gb.mn[a] = std::min({ gb.mn[a], s.c[a] + s.r, s.c[a] - s.r });
                    gb.mx[a] = std::max({ gb.mx[a], s.c[a] + s.r, s.c[a] - s.r });
                }
            } else {
                const RefTriangle &t = tris[it.index];
                const float *vv[3] = { t.v0, t.v1, t.v2 };
                for(int k = 0; k < 3; ++k) for(int a = 0; a < 3; ++a){ gb.mn[a] = std::min(gb.mn[a], vv[k][a]); gb.mx[a] = std::max(gb.mx[a], vv[k][a]); }
            }
        }
        // AABB::intersectAABB widens a degenerate axis in place every time it is called
        // (src/object.cpp:108-111); the box it settles on is used from the start here
        for(int a = 0; a < 3; ++a) for(int guard = 0; guard < 64 && gb.mx[a] - gb.mn[a] < 1e-6f; ++guard){ gb.mn[a] -= 0.5f * 1e-6f; gb.mx[a] += 0.5f * 1e-6f; }
        gboxes.push_back(gb);
        scene_box.grow(gb);
    }
    for(int a = 0; a < 3; ++a){ out.scene_min[a] = 1e9f; out.scene_max[a] = -1e9f; }
    for(const Box &gb : gboxes) for(int a = 0; a < 3; ++a){ out.scene_min[a] = std::min(out.scene_min[a], gb.mn[a]); out.scene_max[a] = std::max(out.scene_max[a], gb.mx[a]); }
    float extent = 0.0f;
    if(!gboxes.empty()) for(int a = 0; a < 3; ++a){
        extent = std::max(extent, scene_box.mx[a] - scene_box.mn[a]);
        extent = std::max(extent, std::max(std::fabs(scene_box.mn[a]), std::fabs(scene_box.mx[a])));
    }
    size_t gi = 0;
    for(auto &kv : gm){
        DevGroup g; memset(&g, 0, sizeof g);
        for(int a = 0; a < 3; ++a){ g.mn[a] = gboxes[gi].mn[a]; g.mx[a] = gboxes[gi].mx[a]; }
        g.sphere_first = (uint32_t) out.spheres.size();
        std::vector<Item> gtris;
        for(const Item &it : kv.second){
            if(it.kind == 0){
                const RefSphere &s = spheres[it.index];
                DevRound r; memset(&r, 0, sizeof r);
                r.c[0] = s.c[0]; r.c[1] = s.c[1]; r.c[2] = s.c[2]; r.r = s.r;
                r.material = intern_material(s.m, mat_table, out.materials);
                r.flags = (s.m.eta <= 0.0f) ? 1u : 0u;
                r.pad[0] = it.seq;
                out.spheres.push_back(r);
            } else {
                // a dead triangle (a non-finite edge, triangle_boxes' rule) stays out of the group's tree: the test the
                // bidirectional kernels make (src/object.cpp:72-95) would report a hit at t = NaN, every comparison with
                // a NaN being false, and its box would be built from whichever coordinates are finite
                const RefTriangle &t = tris[it.index];
                bool live = true;
                for(int a = 0; a < 3; ++a) live = live && std::isfinite(t.v1[a] - t.v0[a]) && std::isfinite(t.v2[a] - t.v0[a]);
                if(live) gtris.push_back(it);
            }
        }
        g.sphere_count = (uint32_t) out.spheres.size() - g.sphere_first;
        Builder B;
        B.node_base = (uint32_t) out.nodes.size(); B.tri_base = (uint32_t) out.tris.size();
        B.pad_abs = 2e-6f * extent;
        B.prims.resize(gtris.size());
        for(size_t i = 0; i < gtris.size(); ++i){
            const RefTriangle &t = tris[gtris[i].index];
            Prim &p = B.prims[i];
            p.box.reset(); p.box.grow(t.v0); p.box.grow(t.v1); p.box.grow(t.v2);
            for(int a = 0; a < 3; ++a) p.cen[a] = 0.5f * (p.box.mn[a] + p.box.mx[a]);
            p.index = (uint32_t) i;
        }
        B.nodes.resize(std::max<size_t>(gtris.size(), 1) + Builder::kSlotSlack);
        if(gtris.empty()) g.root = kEmptyChild;
        else { Box rb; g.root = B.build(0, (int) gtris.size(), 0, rb); }
        if(B.max_depth_seen.load() > kMaxBvhDepth) return "internal error: BVH deeper than the traversal stack";
        out.bvh_depth = std::max(out.bvh_depth, B.max_depth_seen.load());
        out.nodes.insert(out.nodes.end(), B.nodes.begin(), B.nodes.begin() + B.next_node.load());
        for(const Prim &pr : B.prims){
            const Item &it = gtris[pr.index];
            const RefTriangle &t = tris[it.index];
            DevTriangle d;
            for(int a = 0; a < 3; ++a){ d.v0[a] = t.v0[a]; d.e1[a] = t.v1[a] - t.v0[a]; d.e2[a] = t.v2[a] - t.v0[a]; }   // src/object.cpp:75
            d.ordinal = it.seq;
            d.material = intern_material(t.m, mat_table, out.materials);
            d.flags = (t.m.eta <= 0.0f) ? 1u : 0u;
            out.tris.push_back(d);
        }
        out.groups.push_back(g);
        ++gi;
    }
    if(out.materials.empty()) out.materials.push_back(blank_material());
    if(out.nodes.empty()){ BvhNode n; memset(&n, 0, sizeof n); out.nodes.push_back(n); }
    return "";
}

} // namespace hpt
