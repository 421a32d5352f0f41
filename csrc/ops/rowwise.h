// Shared pieces of the row-wise kernels (layernorm.hip, fused_residual.hip,
// embedding.hip, bias_act.hip, cross_entropy.hip): the dtype dispatch, the
// block-per-row launch ladder, 16 B slice IO, the LayerNorm forward and
// backward row cores and the Philox keep-mask. Every device helper is
// __forceinline__ and keeps the evaluation order of the kernels it came
// from: inside a thread item-major, then k; column of item i =
// (i * blockDim.x + threadIdx.x) * VEC.
#pragma once

#include <torch/extension.h>

#include <type_traits>

#include "../common.h"

// scalar_t / kVec (elements per 16 B slice) for bf16, fp16 and fp32
#define DISPATCH_ROW_DTYPE(TYPE, NAME, ...)                                  \
  [&] {                                                                      \
    if (TYPE == at::kBFloat16) {                                             \
      using scalar_t = __hip_bfloat16;                                       \
      constexpr int kVec = 8;                                                \
      return __VA_ARGS__();                                                  \
    } else if (TYPE == at::kHalf) {                                          \
      using scalar_t = __half;                                               \
      constexpr int kVec = 8;                                                \
      return __VA_ARGS__();                                                  \
    } else if (TYPE == at::kFloat) {                                         \
      using scalar_t = float;                                                \
      constexpr int kVec = 4;                                                \
      return __VA_ARGS__();                                                  \
    } else {                                                                 \
      TORCH_CHECK(false, NAME, ": unsupported dtype");                       \
    }                                                                        \
  }()

namespace bpa {

template <typename T>
inline T* dptr(const torch::Tensor& t) {
  return reinterpret_cast<T*>(t.data_ptr());
}

// (threads, ITEMS) of the block-per-row kernels: ITEMS slices per thread,
// ITEMS * threads >= slices. fn(integral_constant<int, ITEMS>, threads).
template <typename LaunchFn>
inline void launch_by_items(const char* op, int slices, LaunchFn&& fn) {
  if (slices <= 256) {
    fn(std::integral_constant<int, 1>{}, ((slices + 63) / 64) * 64);
  } else if (slices <= 512) {
    fn(std::integral_constant<int, 2>{}, 256);
  } else if (slices <= 1024) {
    fn(std::integral_constant<int, 2>{}, 512);
  } else if (slices <= 2048) {
    fn(std::integral_constant<int, 4>{}, 512);
  } else {
    TORCH_CHECK(slices <= 4096, op, ": H too large");
    fn(std::integral_constant<int, 4>{}, 1024);
  }
}

// fn(std::bool_constant<flag>): a run-time flag as a template argument
template <typename Fn>
inline void by_flag(bool flag, Fn&& fn) {
  if (flag) fn(std::true_type{});
  else fn(std::false_type{});
}

// ---------------------------------------------------------------------------
// slice IO: VEC elements of T as one 16 B access (scalar accesses where
// VEC elements of T are not 16 B: fp32 at VEC = 8). The kernels convert
// to and from fp32 element by element inside their own k loops.
// ---------------------------------------------------------------------------
template <typename T, int VEC>
__device__ __forceinline__ void load_slice(const T* p, T (&t)[VEC]) {
  if (sizeof(T) * VEC == 16) {
    *reinterpret_cast<uint4*>(t) = *reinterpret_cast<const uint4*>(p);
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) t[k] = p[k];
  }
}

template <typename T, int VEC>
__device__ __forceinline__ void store_slice(T* p, const T (&t)[VEC]) {
  if (sizeof(T) * VEC == 16) {
    *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(t);
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) p[k] = t[k];
  }
}

// ---------------------------------------------------------------------------
// dropout: keep-mask bytes of one slice. Philox counter offset +
// elem_index / 4 + q yields the mask of elements 4q .. 4q+3.
// ---------------------------------------------------------------------------
template <int VEC>
__device__ __forceinline__ void keep_mask(const Philox& philox,
                                          uint64_t offset, int64_t elem_index,
                                          float p, uint8_t (&mv)[VEC]) {
#pragma unroll
  for (int q = 0; q < VEC / 4; ++q) {
    uint32_t r4[4];
    philox(offset + elem_index / 4 + q, r4);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      mv[q * 4 + j] = u32_to_uniform(r4[j]) >= p ? 1 : 0;
  }
}

template <int VEC>
__device__ __forceinline__ void load_mask(const uint8_t* p,
                                          uint8_t (&mv)[VEC]) {
  using word_t = std::conditional_t<VEC == 8, uint2, uint32_t>;
  *reinterpret_cast<word_t*>(mv) = *reinterpret_cast<const word_t*>(p);
}

template <int VEC>
__device__ __forceinline__ void store_mask(uint8_t* p,
                                           const uint8_t (&mv)[VEC]) {
  using word_t = std::conditional_t<VEC == 8, uint2, uint32_t>;
  *reinterpret_cast<word_t*>(p) = *reinterpret_cast<const word_t*>(mv);
}

// ---------------------------------------------------------------------------
// LayerNorm forward row core. The thread holds ITEMS slices of the row in
// v (slice i valid where cols[i] < H) and their sum. Two-pass variance
// over the registers: sumsq/H - mu^2 cancels catastrophically once
// |mean| >> std. red and red2 are single-use LDS buffers of the kernel
// (one per block reduction); thread 0 writes the row's mean and rstd.
// ---------------------------------------------------------------------------
struct RowStats {
  float mu, rs;
};

template <int VEC, int ITEMS>
__device__ __forceinline__ RowStats ln_row_stats(
    const float (&v)[ITEMS][VEC], const int (&cols)[ITEMS], float sum, int H,
    float eps, float* red, float* red2, float* mean, float* rstd, int row) {
  const float mu = block_reduce_sum1(sum, red) / H;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    if (cols[i] < H) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float d = v[i][k] - mu;
        sq += d * d;
      }
    }
  }
  const float var = block_reduce_sum1(sq, red2) / H;
  const float rs = rsqrtf(var + eps);
  if (threadIdx.x == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
  return {mu, rs};
}

// normalised affine value of one element
__device__ __forceinline__ float ln_affine(float v, RowStats st, float g,
                                           float b) {
  return (v - st.mu) * st.rs * g + b;
}

// y = affine(normalise(v)) for every slice of the row: the epilogue of the
// kernels that do nothing else to the normalised value
template <typename T, int VEC, int ITEMS>
__device__ __forceinline__ void ln_affine_store(
    const float (&v)[ITEMS][VEC], const int (&cols)[ITEMS], RowStats st,
    const float* gamma, const float* beta, T* y_row, int H) {
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int c = cols[i];
    if (c < H) {
      T o[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        o[k] = DTraits<T>::from_f32(
            ln_affine(v[i][k], st, gamma[c + k], beta[c + k]));
      store_slice(y_row + c, o);
    }
  }
}

// ---------------------------------------------------------------------------
// LayerNorm backward row core: dw = dy * gamma, xh = (x - mu) * rs,
// s1 = sum(dw * xh), s2 = sum(dw) over the thread's slices; then
// dz = rs * (dw - mean(dw) - xh * mean(dw * xh)). x, dy and gamma come in
// unconverted and unloaded, so that every operation keeps its place.
// ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void ln_bwd_elem(T x, T dy, const float* gamma,
                                            float mu, float rs, float& dw,
                                            float& xh, float& s1, float& s2) {
  xh = (DTraits<T>::to_f32(x) - mu) * rs;
  dw = DTraits<T>::to_f32(dy) * *gamma;
  s1 += dw * xh;
  s2 += dw;
}

// block-reduces s1, s2 to their row means; red: 32 floats, single-use
__device__ __forceinline__ void ln_bwd_row_means(float& s1, float& s2, int H,
                                                 float* red) {
  block_reduce_sum2(s1, s2, red);
  s1 /= H;
  s2 /= H;
}

__device__ __forceinline__ float ln_bwd_dz(float dw, float xh, float rs,
                                           float s1, float s2) {
  return rs * (dw - s2 - xh * s1);
}

}  // namespace bpa
