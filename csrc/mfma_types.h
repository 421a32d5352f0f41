// 16-bit element traits for the gfx950 MFMA kernels (attention, wgrad,
// MLM head). v_mfma_f32_16x16x32_bf16 and v_mfma_f32_16x16x32_f16 share
// one shape and one fragment layout, and ds_read_b64_tr_b16 moves 16-bit
// lanes without looking at them, so a kernel written against Mfma16<T>
// instantiates for either element type with identical LDS strides, bank
// behaviour and register budget. Accumulation is fp32 in both.
#pragma once

#include <hip/hip_runtime.h>

namespace bpa {

typedef __attribute__((ext_vector_type(4))) float f32x4;

template <typename T>
struct Mfma16;

template <>
struct Mfma16<__bf16> {
  using elem = __bf16;
  // 8-wide A/B fragment of one 16x16x32 MFMA
  typedef __attribute__((ext_vector_type(8))) __bf16 frag;
  // 4-wide vector the transpose-read builtin takes and returns
  typedef __attribute__((__vector_size__(4 * sizeof(__bf16)))) __bf16 tr4;
  static constexpr const char* name = "bf16";

  static __device__ __forceinline__ f32x4 mfma(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  // ds_read_b64_tr_b16 from an LDS pointer (generic pointers into
  // __shared__ memory are cast to address space 3 here)
  static __device__ __forceinline__ tr4 tr_read(const elem* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
        (__attribute__((address_space(3))) tr4*)(p));
  }
  static __device__ __forceinline__ elem from_f32(float v) {
    return __bf16(v);
  }
  static __device__ __forceinline__ float to_f32(elem v) {
    return static_cast<float>(v);
  }
};

template <>
struct Mfma16<_Float16> {
  using elem = _Float16;
  typedef __attribute__((ext_vector_type(8))) _Float16 frag;
  // The transpose-read builtin is declared on a vector of __fp16 (the
  // storage-only half type), NOT _Float16: a _Float16 vector pointer is
  // rejected at compile time. Same bits; callers reinterpret through a
  // union with `frag`, exactly as the bf16 path does.
  typedef __attribute__((__vector_size__(4 * sizeof(__fp16)))) __fp16 tr4;
  static constexpr const char* name = "fp16";

  static __device__ __forceinline__ f32x4 mfma(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ tr4 tr_read(const elem* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4f16(
        (__attribute__((address_space(3))) tr4*)(p));
  }
  // Round-to-nearest-even; values beyond the fp16 range become +-inf
  // (never a saturated finite value): a GradScaler detects overflowed
  // steps by looking for inf.
  static __device__ __forceinline__ elem from_f32(float v) {
    return static_cast<_Float16>(v);
  }
  static __device__ __forceinline__ float to_f32(elem v) {
    return static_cast<float>(v);
  }
};

}  // namespace bpa
