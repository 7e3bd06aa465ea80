// TEST INFRASTRUCTURE ONLY -- host stand-in for <cuda_runtime.h>, written for this repository.
//
// With it (and the sibling curand_kernel.h and glm/ stand-ins) the reference's own sources compile
// with plain g++ into oracle/_ref/ (oracle/Makefile, target `ref`), so that what the reference
// computes can be recorded as fixtures.  Only what those sources use is here:
//   * float3 / int3 / uint3 / dim3 as aggregates and make_float3 / make_int3;
//   * empty __global__ / __device__ / __host__ / __forceinline__;
//   * thread-local blockIdx / threadIdx / blockDim / gridDim and shim_grid, which runs a launch
//     serially, block by block and thread by thread (kernels that synchronise inside a block are not
//     supported, and none of the pinned ones does);
//   * cudaMalloc / cudaMemcpy / cudaMemset / cudaFree / cudaDeviceSynchronize over the C heap;
//   * min / max overloads and serial atomicAdd / atomicExch.
// __CUDACC__ is defined at the END, after every standard header the reference pulls in has been
// seen, so that the reference takes its device branches while libc / libstdc++ see a plain host
// compiler.
#pragma once

#include <math.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <limits>
#include <map>
#include <random>
#include <string>
#include <vector>

struct float3 { float x, y, z; };
struct int3 { int x, y, z; };
struct uint3 { unsigned x, y, z; };
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};

static inline float3 make_float3(float x, float y, float z){ float3 r; r.x = x; r.y = y; r.z = z; return r; }
static inline int3 make_int3(int x, int y, int z){ int3 r; r.x = x; r.y = y; r.z = z; return r; }

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __constant__
#define __shared__ static thread_local
#define __restrict__

inline thread_local uint3 blockIdx = {0, 0, 0};
inline thread_local uint3 threadIdx = {0, 0, 0};
inline thread_local dim3 blockDim;
inline thread_local dim3 gridDim;

// kernel<<<grid, block>>>(args) is rewritten at build time to shim_grid(grid, block).bind(kernel)(args)
struct shim_grid {
    dim3 g, b;
    shim_grid(dim3 g_, dim3 b_) : g(g_), b(b_) {}
    template <class K> auto bind(K kernel) const {
        const dim3 gg = g, bb = b;
        return [gg, bb, kernel](auto... args){
            gridDim = gg; blockDim = bb;
            for(unsigned bz = 0; bz < gg.z; ++bz) for(unsigned by = 0; by < gg.y; ++by) for(unsigned bx = 0; bx < gg.x; ++bx)
                for(unsigned tz = 0; tz < bb.z; ++tz) for(unsigned ty = 0; ty < bb.y; ++ty) for(unsigned tx = 0; tx < bb.x; ++tx){
                    blockIdx = {bx, by, bz}; threadIdx = {tx, ty, tz};
                    kernel(args...);
                }
        };
    }
};

typedef int cudaError_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };

template <class T> static inline cudaError_t cudaMalloc(T **p, size_t bytes){ *p = (T *) malloc(bytes ? bytes : 1); return *p ? 0 : 2; }
static inline cudaError_t cudaMemcpy(void *dst, const void *src, size_t bytes, cudaMemcpyKind){ if(bytes) memcpy(dst, src, bytes); return 0; }
static inline cudaError_t cudaMemset(void *dst, int v, size_t bytes){ if(bytes) memset(dst, v, bytes); return 0; }
static inline cudaError_t cudaFree(void *p){ free(p); return 0; }
static inline cudaError_t cudaDeviceSynchronize(){ return 0; }
static inline cudaError_t cudaGetLastError(){ return 0; }
static inline const char *cudaGetErrorString(cudaError_t){ return "no error"; }

static inline int min(int a, int b){ return a < b ? a : b; }
static inline int max(int a, int b){ return a > b ? a : b; }
static inline unsigned min(unsigned a, unsigned b){ return a < b ? a : b; }
static inline unsigned max(unsigned a, unsigned b){ return a > b ? a : b; }
static inline float min(float a, float b){ return fminf(a, b); }
static inline float max(float a, float b){ return fmaxf(a, b); }

template <class T> static inline T atomicAdd(T *p, T v){ T old = *p; *p = old + v; return old; }
template <class T> static inline T atomicExch(T *p, T v){ T old = *p; *p = v; return old; }

#ifndef __CUDACC__
#define __CUDACC__ 1
#endif
