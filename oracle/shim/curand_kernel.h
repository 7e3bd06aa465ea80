// TEST INFRASTRUCTURE ONLY -- host stand-in for <curand_kernel.h>, written for this repository.
//
// curandState is a REPLAYABLE stream, not cuRAND's generator: curand_init(seed, idx, ...) ignores
// its seed (the reference passes the wall clock) and seeds std::mt19937(shim_curand_probe_seed + idx);
// curand_uniform draws std::uniform_real_distribution<float>(0, 1) from it.  That is exactly what
// the oracle's rng_mode = 1 draws for pixel idx (oracle/pt_oracle.cpp), and the convention of the
// survey-stage probe whose images tests/golden/ keeps.  The driver sets shim_curand_probe_seed
// before it calls into the reference.
#pragma once
#include <cuda_runtime.h>
#include <random>

inline unsigned long long shim_curand_probe_seed = 0;

struct curandState {
    std::mt19937 mt;
};
typedef curandState curandState_t;

static inline void curand_init(unsigned long long /*clock seed, ignored*/, unsigned long long idx, unsigned long long /*offset*/,
                               curandState *st){
    st->mt.seed((uint32_t) (shim_curand_probe_seed + idx));
}

static inline float curand_uniform(curandState *st){
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    return U(st->mt);
}
