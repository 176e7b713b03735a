// Vector typedefs and the per-precision operand traits of the MFMA kernels (float32 / fp16 / bf16 operands, float32
// accumulate): the MFMA of a 32-byte k-group (mma32) and of a 64-byte read-out group (mma16), LDS stores / loads of the
// state element type, and the activation.  Shared by the persistent kernel (esn_recur_mfma_impl.h), the 16x16x32 skewed kernel, the clustered harvest and the launch-per-step GEMM.
#pragma once
#include <type_traits>
#include "esn_common.h"

namespace esn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 b16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 b16x4 __attribute__((ext_vector_type(4)));

struct TraitsF32 {
    typedef float elem;
    static constexpr int ES = 4;
    static constexpr int PARTS = 1;   // readout images (1 = W_out as is)
    static __device__ __forceinline__ void mma32(f32x16& c, u32x4 a, u32x4 b) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            const uint32_t ai = a[i], bi = b[i];   // copy out: bit_cast of a vector element lvalue reads lane 0
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(ai), __uint_as_float(bi), c, 0, 0, 0);
        }
    }
    // 64-byte row group, lane quarter q takes 16 B: 4 x (16x16x4)
    static __device__ __forceinline__ void mma16(f32x4& c, u32x4 a, u32x4 b) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            const uint32_t ai = a[i], bi = b[i];
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ai), __uint_as_float(bi), c, 0, 0, 0);
        }
    }
    static __device__ __forceinline__ void store4(char* dst, float v0, float v1, float v2, float v3) {
        f32x4 v = {v0, v1, v2, v3};
        *reinterpret_cast<f32x4*>(dst) = v;
    }
    static __device__ __forceinline__ void store1(char* dst, float v) { *reinterpret_cast<float*>(dst) = v; }
    static __device__ __forceinline__ void store2(char* dst, float v0, float v1) {
        *reinterpret_cast<float2*>(dst) = make_float2(v0, v1);
    }
    static __device__ __forceinline__ float load1(const char* src) { return *reinterpret_cast<const float*>(src); }
    static __device__ __forceinline__ void load4(const char* src, float (&v)[4]) {     // 16-byte aligned
        const f32x4 t = *reinterpret_cast<const f32x4*>(src);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    }
    static __device__ __forceinline__ float act(float x) { return tanh_f32(x); }
    // when every pre-activation of a wave is below TANH32_SERIES_MAX the select in tanh_f32 always takes the
    // series: evaluate only that (bit-identical result, half the instructions)
    static constexpr bool HAS_SMALL = true;
    static __device__ __forceinline__ float act_small(float x) { return tanh_f32_series(x); }
};

struct TraitsF16 {
    typedef _Float16 elem;
    static constexpr int ES = 2;
    static constexpr int PARTS = 2;   // W_out = hi + lo (two fp16 images)
    static __device__ __forceinline__ void mma32(f32x16& c, u32x4 a, u32x4 b) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, a),
                                                   __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ void mma16(f32x4& c, u32x4 a, u32x4 b) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, a),
                                                   __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ void store4(char* dst, float v0, float v1, float v2, float v3) {
        h16x4 v = {(_Float16)v0, (_Float16)v1, (_Float16)v2, (_Float16)v3};
        *reinterpret_cast<h16x4*>(dst) = v;
    }
    static __device__ __forceinline__ void store1(char* dst, float v) { *reinterpret_cast<_Float16*>(dst) = (_Float16)v; }
    static __device__ __forceinline__ void store2(char* dst, float v0, float v1) {      // 4-byte aligned
        typedef _Float16 h16x2v __attribute__((ext_vector_type(2)));
        *reinterpret_cast<h16x2v*>(dst) = h16x2v{(_Float16)v0, (_Float16)v1};
    }
    static __device__ __forceinline__ uint32_t pack2(float v0, float v1) {
        typedef _Float16 h16x2v __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(uint32_t, h16x2v{(_Float16)v0, (_Float16)v1});
    }
    static __device__ __forceinline__ void unpack2(uint32_t w, float& v0, float& v1) {
        typedef _Float16 h16x2v __attribute__((ext_vector_type(2)));
        const h16x2v h = __builtin_bit_cast(h16x2v, w);
        v0 = (float)h[0]; v1 = (float)h[1];
    }
    static __device__ __forceinline__ float load1(const char* src) { return (float)*reinterpret_cast<const _Float16*>(src); }
    static __device__ __forceinline__ void load4(const char* src, float (&v)[4]) {     // 8-byte aligned
        const h16x4 t = *reinterpret_cast<const h16x4*>(src);
        v[0] = (float)t[0]; v[1] = (float)t[1]; v[2] = (float)t[2]; v[3] = (float)t[3];
    }
    static __device__ __forceinline__ float act(float z) { return tanh_prescaled(z); }   // weights carry 2 log2 e
    static constexpr bool HAS_SMALL = false;
    static __device__ __forceinline__ float act_small(float z) { return tanh_prescaled(z); }
};

struct TraitsBF16 {
    typedef __bf16 elem;
    static constexpr int ES = 2;
    static constexpr int PARTS = 2;
    static __device__ __forceinline__ void mma32(f32x16& c, u32x4 a, u32x4 b) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(b16x8, a),
                                                    __builtin_bit_cast(b16x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ void mma16(f32x4& c, u32x4 a, u32x4 b) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b16x8, a),
                                                    __builtin_bit_cast(b16x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ void store4(char* dst, float v0, float v1, float v2, float v3) {
        b16x4 v = {(__bf16)v0, (__bf16)v1, (__bf16)v2, (__bf16)v3};
        *reinterpret_cast<b16x4*>(dst) = v;
    }
    static __device__ __forceinline__ void store1(char* dst, float v) { *reinterpret_cast<__bf16*>(dst) = (__bf16)v; }
    static __device__ __forceinline__ void store2(char* dst, float v0, float v1) {      // 4-byte aligned
        typedef __bf16 b16x2v __attribute__((ext_vector_type(2)));
        *reinterpret_cast<b16x2v*>(dst) = b16x2v{(__bf16)v0, (__bf16)v1};
    }
    static __device__ __forceinline__ uint32_t pack2(float v0, float v1) {
        typedef __bf16 b16x2v __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(uint32_t, b16x2v{(__bf16)v0, (__bf16)v1});
    }
    static __device__ __forceinline__ void unpack2(uint32_t w, float& v0, float& v1) {
        v0 = __uint_as_float(w << 16); v1 = __uint_as_float(w & 0xffff0000u);
    }
    static __device__ __forceinline__ float load1(const char* src) { return (float)*reinterpret_cast<const __bf16*>(src); }
    static __device__ __forceinline__ void load4(const char* src, float (&v)[4]) {     // 8-byte aligned
        const b16x4 t = *reinterpret_cast<const b16x4*>(src);
        v[0] = (float)t[0]; v[1] = (float)t[1]; v[2] = (float)t[2]; v[3] = (float)t[3];
    }
    static __device__ __forceinline__ float act(float z) { return tanh_prescaled(z); }   // weights carry 2 log2 e
    static constexpr bool HAS_SMALL = false;
    static __device__ __forceinline__ float act_small(float z) { return tanh_prescaled(z); }
};

}  // namespace esn
