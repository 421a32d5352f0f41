// K-FAC Kronecker-factor update for MI355X (gfx950):
//
//   factor[D,D] = beta * factor + alpha * C,   D = K + has_bias
//   C[:K,:K] = x^T @ x          x [N, K] row-major bf16 or fp16
//   C[K,:K] = C[:K,K] = column sums of x,  C[K,K] = N     (has_bias)
//
// i.e. the running covariance of [x, 1] without a materialised ones
// column, a fp32 copy of x or a separate scale/accumulate pass
// (optim/kfac.py: A factors from layer inputs, G factors from output
// gradients; the 1/N, N and loss-scale normalisations live in alpha).
//
// x^T @ x is the TN form the weight-gradient kernel computes with both
// operands equal, so the main loop is wgrad's (tn_mainloop.h, BK = 32,
// 36.8 KB LDS). The result is symmetric: the grid covers only the
// 128x128 tile pairs ti <= tj (packed index t = tj*(tj+1)/2 + ti) times
// split-K, and writes fp32 slabs part[splitk][ntri][128][128]. A second
// launch sums the slabs in slice order, applies beta/alpha and stores
// every value to factor[i][j] and factor[j][i] from the same register,
// so the factor is exactly symmetric and bitwise reproducible. The
// mirrored store goes through a 64x64 LDS tile so both stores run along
// rows of the factor (its rows are unaligned when D = K + 1: scalar
// dword stores). The bias row/column comes from the ordered col_sum
// reduction (bias_act.hip).
//
// beta and alpha are read from device memory (no host sync when they
// depend on device state such as the loss scale or an overflow check).
// alpha == 0 gates the whole update off: neither launch touches the
// factor, whatever x holds, so 0 * Inf never reaches memory.
//
// Reference op being replaced: the factor accumulation of the
// reference's kfac_pytorch dependency (run_pretraining.py:321-355).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../common.h"
#include "../ops.h"
#include "tn_mainloop.h"

namespace bpa {

namespace kf {

constexpr int kTile = 128;              // factor tile edge (= wg::kBM)
constexpr int kTileElems = kTile * kTile;
constexpr int kSub = 64;                // combine sub-tile edge
constexpr int kMaxSplitK = 64;

// packed upper-triangular index -> (ti, tj), ti <= tj
__device__ __forceinline__ void tri_decode(int t, int& ti, int& tj) {
  tj = 0;
  while ((tj + 1) * (tj + 2) / 2 <= t) ++tj;  // <= K/128 scalar steps
  ti = t - tj * (tj + 1) / 2;
}

}  // namespace kf

// grid: (ntri, splitk); block 256. x [N, K]; part [splitk, ntri, 128, 128].
template <typename T>
__global__ __launch_bounds__(256) void kfac_factor_kernel(
    const T* __restrict__ x, float* __restrict__ part,
    const float* __restrict__ coef, int N, int K, int k_slice, int ntri) {
  if (coef[1] == 0.f) return;  // gated off: the combine reads no slab
  int ti, tj;
  kf::tri_decode(blockIdx.x, ti, tj);
  const int m0 = ti * kf::kTile;
  const int n0 = tj * kf::kTile;
  const int kz0 = blockIdx.y * k_slice;
  const int kz1 = min(N, kz0 + k_slice);
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1;
  const int g = (lane >> 4), li = lane & 15;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* lds = reinterpret_cast<T*>(smem);

  f32x4 acc[4][4] = {};
  tn_mainloop<T, wg::kBK>(x, K, m0, x, K, n0, N, kz0, kz1, lds, acc);

  float* out = part + (static_cast<int64_t>(blockIdx.y) * ntri + blockIdx.x) *
                          kf::kTileElems;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int mi = wi * 64 + a * 16 + g * 4 + r;
        const int nj = wj * 64 + b * 16 + li;
        out[mi * kf::kTile + nj] = acc[a][b][r];
      }
    }
  }
}

// grid: ntri * 4 sub-tile blocks, then ceil(K/256) bias blocks when
// colsum != nullptr; block 256. Each upper-triangular element and its
// mirror belong to exactly one block, which reads the old value from
// the upper triangle only.
__global__ __launch_bounds__(256) void kfac_combine_kernel(
    const float* __restrict__ part, const float* __restrict__ colsum,
    float* __restrict__ factor, const float* __restrict__ coef, int splitk,
    int ntri, int K, int D, float nrows) {
  const float beta = coef[0], alpha = coef[1];
  if (alpha == 0.f) return;  // gated off: factor stays bit-identical
  const int tid = threadIdx.x;
  const int blk = blockIdx.x;
  // beta == 0 (first update) must not read the old value at all
  auto ema = [&](const float* old, float c) {
    return (beta == 0.f ? 0.f : beta * *old) + alpha * c;
  };

  if (blk >= ntri * 4) {  // bias row and column
    const int idx = (blk - ntri * 4) * 256 + tid;
    if (idx < K) {
      float* row = factor + static_cast<int64_t>(K) * D + idx;
      const float o = ema(row, colsum[idx]);
      *row = o;
      factor[static_cast<int64_t>(idx) * D + K] = o;
    }
    if (idx == 0) {
      float* corner = factor + static_cast<int64_t>(K) * D + K;
      *corner = ema(corner, nrows);
    }
    return;
  }

  const int t = blk >> 2, si = (blk >> 1) & 1, sj = blk & 1;
  int ti, tj;
  kf::tri_decode(t, ti, tj);
  const bool diag_tile = ti == tj;
  if (diag_tile && si > sj) return;          // lower sub-tile: mirrored
  const bool diag_sub = diag_tile && si == sj;
  const int i0 = ti * kf::kTile + si * kf::kSub;
  const int j0 = tj * kf::kTile + sj * kf::kSub;
  const float* p0 = part + static_cast<int64_t>(t) * kf::kTileElems +
                    si * kf::kSub * kf::kTile + sj * kf::kSub;
  const int64_t slab = static_cast<int64_t>(ntri) * kf::kTileElems;

  __shared__ float tile[kf::kSub][kf::kSub + 1];
  const int r = tid >> 4, c = (tid & 15) * 4;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int i = pass * 16 + r;
    const float* p = p0 + i * kf::kTile + c;
    f32x4 s = *reinterpret_cast<const f32x4*>(p);
    for (int z = 1; z < splitk; ++z) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(p + z * slab);
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] += q[k];
    }
    const float* old = factor + static_cast<int64_t>(i0 + i) * D + j0 + c;
#pragma unroll
    for (int k = 0; k < 4; ++k) tile[i][c + k] = ema(old + k, s[k]);
  }
  __syncthreads();
  // rows of the upper triangle; a diagonal sub-tile takes its lower
  // half from the upper one
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int i = pass * 16 + r;
    float* dst = factor + static_cast<int64_t>(i0 + i) * D + j0 + c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = c + k;
      dst[k] = (diag_sub && i > j) ? tile[j][i] : tile[i][j];
    }
  }
  if (!diag_sub) {  // mirror: rows j of the lower triangle, lanes along i
    const int i = tid & 63;
    for (int j = tid >> 6; j < kf::kSub; j += 4)
      factor[static_cast<int64_t>(j0 + j) * D + i0 + i] = tile[i][j];
  }
}

bool kfac_factor_supported(int64_t N, int64_t K) {
  // columns must tile exactly (whole uint4 staging reads, 128-wide
  // tiles); rows need no alignment beyond the wgrad kernel's
  return K > 0 && K % kf::kTile == 0 && N % 4 == 0 && N >= 256 &&
         N < (int64_t{1} << 30) && K <= 32768;
}

template <typename T>
static void kfac_factor_update_t(torch::Tensor x, torch::Tensor factor,
                                 torch::Tensor coef, bool has_bias,
                                 int64_t splitk_override) {
  const int N = x.size(0), K = x.size(1);
  const int D = K + (has_bias ? 1 : 0);
  const int nt = K / kf::kTile;
  const int ntri = nt * (nt + 1) / 2;
  // wgrad's occupancy rule (its sweep: tiles * splitk ~ 512-768,
  // splitk <= 8), applied to the triangular tile count
  int splitk = 1;
  while (splitk < 8 && ntri * (splitk + 1) <= 768 &&
         N / (splitk + 1) >= 8 * wg::kBK)
    ++splitk;
  if (splitk_override > 0) splitk = static_cast<int>(splitk_override);
  int k_slice =
      ((N + splitk - 1) / splitk + wg::kBK - 1) / wg::kBK * wg::kBK;
  splitk = (N + k_slice - 1) / k_slice;  // drop empty tail slices

  auto f32 = x.options().dtype(torch::kFloat32);
  auto part = torch::empty(
      {splitk, static_cast<int64_t>(ntri), kf::kTile, kf::kTile}, f32);
  torch::Tensor colsum;
  if (has_bias) colsum = col_sum(x);  // fp32 [K], fixed order
  auto stream = at::hip::getCurrentHIPStream();
  const size_t lds = 4 * wg::kBK * wg::kStride * sizeof(T);
  const float* coef_p = coef.data_ptr<float>();
  hipLaunchKernelGGL(kfac_factor_kernel<T>, dim3(ntri, splitk), dim3(256),
                     lds, stream, reinterpret_cast<const T*>(x.data_ptr()),
                     part.data_ptr<float>(), coef_p, N, K, k_slice, ntri);
  const int bias_blocks = has_bias ? (K + 255) / 256 : 0;
  hipLaunchKernelGGL(kfac_combine_kernel, dim3(ntri * 4 + bias_blocks),
                     dim3(256), 0, stream, part.data_ptr<float>(),
                     has_bias ? colsum.data_ptr<float>() : nullptr,
                     factor.data_ptr<float>(), coef_p, splitk, ntri, K, D,
                     static_cast<float>(N));
}

// factor = coef[0] * factor + coef[1] * cov([x, 1] or x), in place.
void kfac_factor_update(torch::Tensor x, torch::Tensor factor,
                        torch::Tensor coef, bool has_bias,
                        int64_t splitk_override) {
  const auto dt = x.scalar_type();
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous() &&
                  (dt == torch::kBFloat16 || dt == torch::kHalf),
              "kfac_factor_update: x must be contiguous 2D bf16 or fp16");
  TORCH_CHECK(kfac_factor_supported(x.size(0), x.size(1)),
              "kfac_factor_update: unsupported shape [", x.size(0), ", ",
              x.size(1), "]");
  const int64_t D = x.size(1) + (has_bias ? 1 : 0);
  TORCH_CHECK(factor.is_cuda() && factor.dim() == 2 &&
                  factor.is_contiguous() &&
                  factor.scalar_type() == torch::kFloat32 &&
                  factor.size(0) == D && factor.size(1) == D,
              "kfac_factor_update: factor must be contiguous fp32 [", D, ", ",
              D, "]");
  TORCH_CHECK(coef.is_cuda() && coef.is_contiguous() && coef.numel() == 2 &&
                  coef.scalar_type() == torch::kFloat32,
              "kfac_factor_update: coef must be 2 contiguous fp32 values "
              "{beta, alpha} on the device");
  TORCH_CHECK(factor.device() == x.device() && coef.device() == x.device(),
              "kfac_factor_update: tensors on different devices");
  TORCH_CHECK(splitk_override >= 0 && splitk_override <= kf::kMaxSplitK,
              "kfac_factor_update: splitk_override out of range");
  if (dt == torch::kHalf)
    kfac_factor_update_t<_Float16>(x, factor, coef, has_bias,
                                   splitk_override);
  else
    kfac_factor_update_t<__bf16>(x, factor, coef, has_bias, splitk_override);
}

}  // namespace bpa
