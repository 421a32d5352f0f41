// Shared pieces of the row-wise kernels (layernorm.hip, fused_residual.hip,
// embedding.hip, bias_act.hip, cross_entropy.hip): the dtype dispatch, the
// block-per-row launch ladder, 16 B slice IO, the LayerNorm forward and
// backward row cores and the Philox keep-mask. Every device helper is
// __forceinline__ and keeps the evaluation order of the kernels it came
// from: inside a thread item-major, then k; column of item i =
// (i * blockDim.x + threadIdx.x) * VEC.
#pragma once

#include <torch/extension.h>

#include <algorithm>
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
// dz = rs * (dw - mean(dw) - xh * mean(dw * xh)). x comes in unconverted,
// so that every operation keeps its place. Which products are fused into
// an fma is spelled out (only the one in dz), with contraction off
// otherwise: left to the compiler it differs from one instantiation of a
// kernel to the next, and dx has to be the same whichever of them
// computes it.
// ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void ln_bwd_elem(T x, float dy, float gamma,
                                            float mu, float rs, float& dw,
                                            float& xh, float& s1, float& s2) {
#pragma clang fp contract(off)
  xh = (DTraits<T>::to_f32(x) - mu) * rs;
  dw = dy * gamma;
  s1 += dw * xh;  // product rounded, then added: not an fma
  s2 += dw;
}

// block-reduces s1, s2 to their row means over the blockDim.x threads of
// one row; red: 32 floats, not reused before the block's next barrier
__device__ __forceinline__ void ln_bwd_row_means(float& s1, float& s2, int H,
                                                 float* red) {
  block_reduce_sum2(s1, s2, red);
  s1 /= H;
  s2 /= H;
}

__device__ __forceinline__ float ln_bwd_dz(float dw, float xh, float rs,
                                           float s1, float s2) {
#pragma clang fp contract(off)
  return rs * __builtin_fmaf(-xh, s1, dw - s2);
}

// ---------------------------------------------------------------------------
// LayerNorm-family backward, one pass: dx (and the junction's dz_res) plus
// the column gradients. A block is blockDim.y row lanes of blockDim.x
// threads (the launch_by_items mapping) and owns rows_per_block
// consecutive rows; lane y takes rows r_begin + y, + blockDim.y, ... so
// that blockDim.y rows are in flight side by side, and every thread sees
// the same columns in every row. It carries fp32 sums of dy * xh
// (dgamma), dy (dbeta) and, with HAS_BIAS, of dx as stored (dbias) across
// its rows; at the end the lanes are added in y order through the LDS
// slab and the block stores one [nsl * H] row of `part`. The caller folds
// the part rows with col_reduce_full: every order is fixed, no atomics.
//
// JUNCTION: bias + dropout + residual + LN (x is the saved z; writes
// dz_res and dx = dropout'(dz)); otherwise plain LN (writes dx only).
// HAS_DY2: the upstream gradient is dy + dy2, summed in fp32 on load.
// Narrow rows (kPipe) keep gamma in registers and load the lane's next
// row before the current row's block reduction.
// ---------------------------------------------------------------------------
constexpr int kRowGroupThreads = 512;  // blockDim.x * blockDim.y, at most
constexpr int kRowGroupBlocks = 512;   // grid, at most
constexpr int kRowGroupMinRows = 2;    // rows per lane, at least

template <typename T, int VEC, int ITEMS, bool DROP, bool DY2>
struct LnBwdRow {
  T dy[ITEMS][VEC], x[ITEMS][VEC];
  T dy2[DY2 ? ITEMS : 1][VEC];
  uint8_t keep[DROP ? ITEMS : 1][VEC];
  float mu, rs;
};

template <typename T, int VEC, int ITEMS, bool JUNCTION, bool TRAIN_DROP,
          bool HAS_BIAS, bool HAS_DY2>
__global__ void
__launch_bounds__(ITEMS <= 2 ? kRowGroupThreads : 1024, ITEMS == 2 ? 2 : 4)
ln_bwd_rows_kernel(
    const T* __restrict__ dy, const T* __restrict__ dy2,
    const T* __restrict__ x, const uint8_t* __restrict__ mask,
    const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ rstd, T* __restrict__ dx,
    T* __restrict__ dz_res, float* __restrict__ part, int rows, int H,
    int rows_per_block, float p) {
  static_assert(JUNCTION || !(TRAIN_DROP || HAS_BIAS || HAS_DY2), "");
  constexpr bool kPipe = ITEMS * VEC <= 8;
  constexpr int NSL = HAS_BIAS ? 3 : 2;
  using Row = LnBwdRow<T, VEC, ITEMS, TRAIN_DROP, HAS_DY2>;
  extern __shared__ float slab[];
  __shared__ float red[2][kRowGroupThreads / WAVE_SIZE][32];
  const int lanes = blockDim.y, y = threadIdx.y;
  const int r_begin = blockIdx.x * rows_per_block;
  const int r_end = min(r_begin + rows_per_block, rows);
  const float keep_scale = TRAIN_DROP ? 1.0f / (1.0f - p) : 1.0f;

  int cols[ITEMS];
  float g[kPipe ? ITEMS : 1][VEC];
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    cols[i] = (i * blockDim.x + threadIdx.x) * VEC;
    if (kPipe && cols[i] < H) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) g[i][k] = gamma[cols[i] + k];
    }
  }
  auto load_row = [&](Row& r, int row) {
    const int64_t base = static_cast<int64_t>(row) * H;
    r.mu = mean[row];
    r.rs = rstd[row];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
      const int c = cols[i];
      if (c < H) {
        load_slice(dy + base + c, r.dy[i]);
        if (HAS_DY2) load_slice(dy2 + base + c, r.dy2[i]);
        load_slice(x + base + c, r.x[i]);
        if (TRAIN_DROP) load_mask(mask + base + c, r.keep[i]);
      }
    }
  };

  float acc[NSL][ITEMS][VEC] = {};
  Row cur, nxt;
  int row = r_begin + y;
  if (kPipe && row < r_end) load_row(cur, row);
  for (int it = 0; r_begin + it * lanes < r_end; ++it, row += lanes) {
    const bool valid = row < r_end;
    if (kPipe) {
      if (row + lanes < r_end) load_row(nxt, row + lanes);
    } else if (valid) {
      load_row(cur, row);
    }
    float dw[ITEMS][VEC], xh[ITEMS][VEC];
    float s1 = 0.f, s2 = 0.f;
    if (valid) {
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        const int c = cols[i];
        if (c < H) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            float d = DTraits<T>::to_f32(cur.dy[i][k]);
            if (HAS_DY2) d += DTraits<T>::to_f32(cur.dy2[i][k]);
            const float gk = kPipe ? g[i][k] : gamma[c + k];
            ln_bwd_elem(cur.x[i][k], d, gk, cur.mu, cur.rs, dw[i][k],
                        xh[i][k], s1, s2);
            acc[0][i][k] += d * xh[i][k];
            acc[1][i][k] += d;
          }
        }
      }
    }
    // the buffer of iteration it - 2: every wave has passed the barrier of
    // it - 1 since it read that one
    ln_bwd_row_means(s1, s2, H, red[it & 1][y]);
    if (valid) {
      const int64_t base = static_cast<int64_t>(row) * H;
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        const int c = cols[i];
        if (c < H) {
          T dzo[VEC], dxo[VEC];
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            const float dzk = ln_bwd_dz(dw[i][k], xh[i][k], cur.rs, s1, s2);
            dzo[k] = DTraits<T>::from_f32(dzk);  // grad to residual input
            if (JUNCTION) {
              float dxk = dzk;
              if (TRAIN_DROP) {
                dxk = cur.keep[i][k] ? dzk * keep_scale : 0.f;
                // keep the product an fp32 value of its own: folded into
                // the conversion (v_fma_mixlo_f16) it is rounded once, not
                // twice, and whether the compiler folds it differs from
                // one instantiation to the next
                asm("" : "+v"(dxk));
              }
              dxo[k] = DTraits<T>::from_f32(dxk);
              // the value as stored: dbias stays the column sum of dx
              if (HAS_BIAS) acc[NSL - 1][i][k] += DTraits<T>::to_f32(dxo[k]);
            }
          }
          if (JUNCTION) {
            store_slice(dz_res + base + c, dzo);
            store_slice(dx + base + c, dxo);
          } else {
            store_slice(dx + base + c, dzo);
          }
        }
      }
    }
    if (kPipe) cur = nxt;
  }

  float* out = part + static_cast<int64_t>(blockIdx.x) * NSL * H;
#pragma unroll
  for (int sl = 0; sl < NSL; ++sl) {
    if (lanes == 1) {
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        if (cols[i] < H) {
#pragma unroll
          for (int k = 0; k < VEC; ++k)
            out[sl * H + cols[i] + k] = acc[sl][i][k];
        }
      }
      continue;
    }
    // slab[lane][item][k][thread]: consecutive threads, consecutive words
    if (sl > 0) __syncthreads();
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        slab[((y * ITEMS + i) * VEC + k) * blockDim.x + threadIdx.x] =
            acc[sl][i][k];
    }
    __syncthreads();
    if (y == sl % lanes) {
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        if (cols[i] < H) {
          float tot[VEC] = {};
          for (int j = 0; j < lanes; ++j) {
#pragma unroll
            for (int k = 0; k < VEC; ++k)
              tot[k] +=
                  slab[((j * ITEMS + i) * VEC + k) * blockDim.x + threadIdx.x];
          }
#pragma unroll
          for (int k = 0; k < VEC; ++k) out[sl * H + cols[i] + k] = tot[k];
        }
      }
    }
  }
}

// Launches ln_bwd_rows_kernel<T, VEC, ..., JUNCTION, ...> over [rows, H]
// and returns its fp32 partials [nblocks, nsl * H] (dgamma | dbeta |
// dbias), to be folded by col_reduce_full. Row lanes fill the block up to
// kRowGroupThreads; a lane takes the fewest rows that keep the grid within
// kRowGroupBlocks, and at least kRowGroupMinRows (sweep: docs/KERNELS.md).
// dy2 and mask may be undefined (no second gradient, no dropout); dz_res
// only with JUNCTION.
template <typename T, int VEC, bool JUNCTION>
inline torch::Tensor ln_bwd_rows(const char* op, const torch::Tensor& dy,
                                 const torch::Tensor& dy2,
                                 const torch::Tensor& x,
                                 const torch::Tensor& mask,
                                 const torch::Tensor& gamma_f,
                                 const torch::Tensor& mean,
                                 const torch::Tensor& rstd, torch::Tensor& dx,
                                 torch::Tensor& dz_res, double p,
                                 bool has_bias, hipStream_t stream) {
  const int rows = x.size(0), H = x.size(1);
  const int nsl = has_bias ? 3 : 2;
  auto fopts = x.options().dtype(torch::kFloat32);
  if (rows == 0) return torch::zeros({1, nsl * H}, fopts);
  const bool train_drop = JUNCTION && p > 0.0;
  const bool has_dy2 = dy2.defined();
  torch::Tensor part;
  launch_by_items(op, H / VEC, [&](auto items_c, int threads) {
    constexpr int ITEMS = decltype(items_c)::value;
    const int lanes =
        threads >= kRowGroupThreads ? 1 : kRowGroupThreads / threads;
    const int groups = (rows + lanes - 1) / lanes;
    const int rows_per_lane = std::max(
        kRowGroupMinRows, (groups + kRowGroupBlocks - 1) / kRowGroupBlocks);
    const int rows_per_block = rows_per_lane * lanes;
    const int nblocks = (rows + rows_per_block - 1) / rows_per_block;
    part = torch::empty({nblocks, nsl * H}, fopts);
    const size_t lds =
        lanes > 1 ? sizeof(float) * lanes * threads * ITEMS * VEC : 0;
    by_flag(train_drop, [&](auto train_c) {
      by_flag(has_bias, [&](auto bias_c) {
        by_flag(has_dy2, [&](auto dy2_c) {
          constexpr bool kTrain = JUNCTION && decltype(train_c)::value;
          constexpr bool kBias = JUNCTION && decltype(bias_c)::value;
          constexpr bool kDy2 = JUNCTION && decltype(dy2_c)::value;
          hipLaunchKernelGGL(
              (ln_bwd_rows_kernel<T, VEC, ITEMS, JUNCTION, kTrain, kBias,
                                  kDy2>),
              dim3(nblocks), dim3(threads, lanes), lds, stream, dptr<T>(dy),
              kDy2 ? dptr<T>(dy2) : nullptr, dptr<T>(x),
              kTrain ? mask.data_ptr<uint8_t>() : nullptr,
              gamma_f.data_ptr<float>(), mean.data_ptr<float>(),
              rstd.data_ptr<float>(), dptr<T>(dx),
              JUNCTION ? dptr<T>(dz_res) : nullptr, part.data_ptr<float>(),
              rows, H, rows_per_block, static_cast<float>(p));
        });
      });
    });
  });
  return part;
}

}  // namespace bpa
