// How gram_accumulate_kernel (esn_gram.hip) and holdout_score_kernel (esn_holdout.hip) read the extended states E on
// their way to LDS: float64 or float32, 16 bytes per lane where the row length allows it, widened to float64.
#pragma once
#include "esn_common.h"

namespace esn {

typedef double stage_f64x2 __attribute__((ext_vector_type(2)));
typedef float stage_f32x4 __attribute__((ext_vector_type(4)));

// the E of a parameter block that carries one of E (float64) / E32 (float32), chosen by the kernel's element type
template <typename P> __device__ __forceinline__ const float* stage_src(const P& p, float*) { return p.E32; }
template <typename P> __device__ __forceinline__ const double* stage_src(const P& p, double*) { return p.E; }

// elements per lane and load: 16 bytes where VEC (cols % 4 == 0: every row and every unit is 16-byte aligned), else one
template <typename T, bool VEC> struct StageUnit { static constexpr int V = 1; };
template <> struct StageUnit<double, true> { static constexpr int V = 2; };
template <> struct StageUnit<float, true> { static constexpr int V = 4; };

__device__ __forceinline__ void stage_fetch(const double* p, double (&v)[1]) { v[0] = *p; }
__device__ __forceinline__ void stage_fetch(const float* p, double (&v)[1]) { v[0] = (double)*p; }
__device__ __forceinline__ void stage_fetch(const double* p, double (&v)[2]) {
    const stage_f64x2 x = *reinterpret_cast<const stage_f64x2*>(p);
    v[0] = x[0]; v[1] = x[1];
}
__device__ __forceinline__ void stage_fetch(const float* p, double (&v)[4]) {
    const stage_f32x4 x = *reinterpret_cast<const stage_f32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (double)x[i];
}

}  // namespace esn
