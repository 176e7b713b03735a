// The state noise of the float32 / fp16 / bf16 recurrence kernels, applied to one quad of activated rows: the one
// definition behind the persistent kernel (esn_recur_mfma_impl.h), the 16x16x32 skewed kernel, the clustered harvest and
// the launch-per-step GEMM.  The stream itself (noise_key / noise_quad: a pure function of seed, frame, step and row) is
// in esn_common.h; where and when a schedule derives its key is that schedule's business.  The float64 kernels add
// noise_uniform as a double and are not served from here.
#pragma once
#include "esn_mfma_traits.h"

namespace esn {

// x += amp ((byte + 1/2) / 256 - 1/2) = byte c1 + c0
struct NoiseCoef { float amp, c1, c0; };
__device__ __forceinline__ NoiseCoef noise_coef(double noise) {
    const float amp = (float)noise;
    return {amp, amp * (1.0f / 256.0f), amp * (0.5f / 256.0f - 0.5f)};
}

// v: the activated rows row .. row + 3 of one frame.  Counter mode takes the quad's four bytes; tensor mode reads
// nz[row + j] (nz: the frame's row of noise_u at this step, null for a padding frame) and is branch-free: a lane without
// noise (padding frame, row past n_res) reads element 0 of nz_safe (p.noise_u, never null in tensor mode) and drops it.
template <int NOISE>
__device__ __forceinline__ void add_state_noise(float (&v)[4], uint32_t quad, const double* nz, const double* nz_safe,
                                                int row, int n_res, const NoiseCoef& nc) {
    if (NOISE == ESN_NOISE_COUNTER) {
        v[0] = fmaf((float)(quad & 0xffU), nc.c1, v[0] + nc.c0);
        v[1] = fmaf((float)((quad >> 8) & 0xffU), nc.c1, v[1] + nc.c0);
        v[2] = fmaf((float)((quad >> 16) & 0xffU), nc.c1, v[2] + nc.c0);
        v[3] = fmaf((float)(quad >> 24), nc.c1, v[3] + nc.c0);
    } else if (NOISE == ESN_NOISE_TENSOR) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool on = nz && row + j < n_res;
            const double u = (on ? nz : nz_safe)[on ? row + j : 0];
            const float w = v[j] + nc.amp * ((float)u - 0.5f);
            v[j] = on ? w : v[j];
        }
    }
}

// fp16 + counter noise takes a packed-half tail: the four noise bytes of a quad become two pairs of halves
// 1 + byte/1024 (one v_perm_b32 each, high byte 0x3C), and   x = tanh + noise ((byte + 1/2)/256 - 1/2)   is one
// v_pk_fma_f16 per pair,
//   x = (1 + byte/1024) c1 + t,   t = half(1 - 2/(1 + 2^z) + c0 - c1),  c1 = half(4 noise)
// instead of four conversions, four adds and four fmas in float32.  (c1 is a normal half -- noise/256 itself would be
// subnormal -- and t is offset by the ROUNDED c1, so the rounding of c1 changes the noise width by 2^-11 relative and
// adds no bias.)
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
struct NoiseCoefHalf { h16x2 c1h; float t_bias; };
__device__ __forceinline__ NoiseCoefHalf noise_coef_half(const NoiseCoef& nc) {
    const _Float16 c1s = (_Float16)(1024.0f * nc.c1);
    return {h16x2{c1s, c1s}, 1.0f + nc.c0 - (float)c1s};
}
// t of a pre-activation z that carries the 2 log2 e pre-scale of the packed weights
__device__ __forceinline__ float biased_tanh(float z, const NoiseCoefHalf& nh) {
    const float e = __builtin_amdgcn_exp2f(z);
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), nh.t_bias);
}
// four biased tanh values and their quad -> the four noised states as two words of packed halves
__device__ __forceinline__ u32x2 noised_half_quad(const float (&t)[4], uint32_t quad, const NoiseCoefHalf& nh) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const h16x2 w01 = __builtin_bit_cast(h16x2, __builtin_amdgcn_perm(0x3C3C3C3Cu, quad, 0x04010400u));
    const h16x2 w23 = __builtin_bit_cast(h16x2, __builtin_amdgcn_perm(0x3C3C3C3Cu, quad, 0x04030402u));
    const h16x2 t01 = __builtin_convertvector(f32x2{t[0], t[1]}, h16x2);
    const h16x2 t23 = __builtin_convertvector(f32x2{t[2], t[3]}, h16x2);
    return u32x2{__builtin_bit_cast(uint32_t, __builtin_elementwise_fma(w01, nh.c1h, t01)),
                 __builtin_bit_cast(uint32_t, __builtin_elementwise_fma(w23, nh.c1h, t23))};
}

}  // namespace esn
