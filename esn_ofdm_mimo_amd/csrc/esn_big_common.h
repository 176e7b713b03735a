// What the two launch-per-step GEMM families (esn_big_predict.hip, esn_big_harvest.hip) both know about the state image
// and about each other: the image's addressing, its [U;F] k-groups, the wave-uniform buffer descriptor of their LDS-DMA
// streams, the pick of a kernel's noise instance and the shape clauses common to their dispatch predicates.
//
// The state image of a step holds X in MFMA fragment order, [n_slots / 32 column tiles][nkg k-groups][64 lanes][16 B]:
// the state k-groups (16 rows each, nkgS = Mp / 16 of them), then the two [U;F] k-groups, then zeros up to nkg = Kp / 16.
// Lane r + 32 h2 of a k-group holds rows 8 h2 .. 8 h2 + 7 of the group for column r of the tile.
#pragma once
#include "esn_state_noise.h"
#include "esn_launch.h"

namespace esn {

template <typename E>
__device__ __forceinline__ u32x2 pack4(float a, float b, float c, float d) {
    typedef E vec4 __attribute__((ext_vector_type(4)));
    const vec4 v = {(E)a, (E)b, (E)c, (E)d};
    return __builtin_bit_cast(u32x2, v);
}

// byte offset of the 16-byte piece of (column tile ct, k-group kg, lane) in an image of nkg k-groups
__device__ __forceinline__ size_t big_piece(int ct, int nkg, int kg, int lane) {
    return ((size_t)ct * nkg + kg) * 1024 + (size_t)lane * 16;
}

// the activated rows 32 rt + 8 q + 4 h .. + 3 of column r of tile ct: k-group 2 rt + (q >> 1), lane r + 32 (q & 1),
// bytes 8 h .. 8 h + 7 (the image is below 2 GB: the dispatch predicates)
__device__ __forceinline__ void big_store_quad(__amdgpu_buffer_rsrc_t img, u32x2 x, int ct, int nkg, int rt, int q,
                                               int r, int h) {
    const int soff = (int)big_piece(ct, nkg, 2 * rt + (q >> 1), 32 * (q & 1));
    __builtin_amdgcn_raw_buffer_store_b64(x, img, r * 16 + 8 * h, soff, 0);
}

// [U;F] of one slot -> k-groups nkgS, nkgS + 1: inputs at k - kin = 0 .. 15, feedback from k - kin = kin_p on
template <typename E>
__device__ __forceinline__ void big_write_uf(char* img, int nkg, int nkgS, int slot, const float (&uu)[16],
                                             const float (&ff)[8], int kin_p) {
    const int ct = slot >> 5, lr = slot & 31;
#pragma unroll
    for (int g2 = 0; g2 < 2; ++g2)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            float e8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int kk = 16 * g2 + 8 * hh + e;              // k - kin
                float v = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) v = (kk == i) ? uu[i] : v;
#pragma unroll
                for (int o = 0; o < 8; ++o) v = (kk == kin_p + o) ? ff[o] : v;
                e8[e] = v;
            }
            char* d = img + big_piece(ct, nkg, nkgS + g2, lr + 32 * hh);
            *reinterpret_cast<u32x2*>(d) = pack4<E>(e8[0], e8[1], e8[2], e8[3]);
            *reinterpret_cast<u32x2*>(d + 8) = pack4<E>(e8[4], e8[5], e8[6], e8[7]);
        }
}

// one descriptor per wave, built from values the compiler can PROVE wave-uniform (readfirstlane of the pointer halves
// and the size): otherwise every DMA is wrapped in a waterfall loop (guide T20)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t big_uniform_rsrc(const void* ptr, int bytes) {
    const uint64_t a = (uint64_t)reinterpret_cast<uintptr_t>(ptr);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>((uintptr_t)(((uint64_t)hi << 32) | lo)), 0,
                                             __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

// the NOISE instance of a step kernel: kernel_of(std::integral_constant<int, MODE>) names the instance of one mode
template <typename F>
const void* big_noise_instance(int noise_mode, F kernel_of) {
    return noise_mode == ESN_NOISE_NONE     ? kernel_of(std::integral_constant<int, ESN_NOISE_NONE>{})
           : noise_mode == ESN_NOISE_TENSOR ? kernel_of(std::integral_constant<int, ESN_NOISE_TENSOR>{})
                                            : kernel_of(std::integral_constant<int, ESN_NOISE_COUNTER>{});
}

// what both families ask of a shape: fp16/bf16, shared reservoir beyond 1024 units, n_in <= 16, n_out <= 8, and
// [U;F] within the two k-groups behind the state
inline bool big_gemm_serves(int precision, const RecurParams& p) {
    return (precision == ESN_F16 || precision == ESN_BF16) && p.n_wsets == 1 && p.n_res > 1024 && p.n_in <= 16 &&
           p.n_out <= 8 && p.g.Kp - p.g.Mp >= 32 && p.g.kfb - p.g.kin + round_up(p.n_out, 4) <= 32;
}

}  // namespace esn
