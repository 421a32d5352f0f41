// Fused LayerNorm forward/backward for MI355X (gfx950).
//
// Replaces Apex FusedLayerNormAffineFunction (reference call sites:
// src/modeling.py:299-335). Shapes here: rows up to ~12k (B*S), H in
// {64..4096}, eps 1e-12. Memory-bound design:
//
// * forward: one BLOCK per row; every lane loads its 16 B slice ONCE
//   into registers, mean/var via wave shuffle + tiny LDS cross-wave
//   combine, normalized output written from registers — exactly one
//   read + one write of x/y (the old one-wave-per-row version re-read
//   x after the reduction and measured 0.89 TB/s; this version 4.2).
// * backward dx: one BLOCK per row, same register-resident shape.
// * dgamma/dbeta: a separate streaming col_stats_kernel over 16-row
//   chunks (per-lane register accumulators, coalesced loads) writes
//   [n_chunks, 2H] partials folded by col_reduce_full — measured
//   faster than fusing the column accumulation into the dx grid.
//
// The row cores (two-pass mean/rstd, affine, backward sums) are in
// rowwise.h, shared with fused_residual.hip and embedding.hip; col_stats
// and col_reduce_full below are declared in ops.h for the other files.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../checks.h"
#include "../ops.h"
#include "rowwise.h"

namespace bpa {

// ITEMS = uint4 slices each thread owns (ITEMS*VEC*blockDim.x >= H).
template <typename T, int VEC, int ITEMS>
__global__ void ln_fwd_kernel(const T* __restrict__ x,
                              const float* __restrict__ gamma,
                              const float* __restrict__ beta,
                              T* __restrict__ y, float* __restrict__ mean,
                              float* __restrict__ rstd, int rows, int H,
                              float eps) {
  __shared__ float red[16], red2[16];
  const int row = blockIdx.x;
  if (row >= rows) return;
  const int64_t base = static_cast<int64_t>(row) * H;

  float v[ITEMS][VEC];
  int cols[ITEMS];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int c = (i * blockDim.x + threadIdx.x) * VEC;
    cols[i] = c;
    if (c < H) {
      T t[VEC];
      load_slice(x + base + c, t);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        v[i][k] = DTraits<T>::to_f32(t[k]);
        sum += v[i][k];
      }
    }
  }
  const RowStats st =
      ln_row_stats(v, cols, sum, H, eps, red, red2, mean, rstd, row);
  ln_affine_store<T, VEC, ITEMS>(v, cols, st, gamma, beta, y + base, H);
}

// backward dx: one BLOCK per row, the mirror of ln_fwd_kernel — dy/x
// loaded once into registers, s1/s2 via block reduce, dx written from
// registers. dgamma/dbeta are NOT computed here (a block-per-row grid
// cannot accumulate columns without atomics); see col_stats_kernel.
template <typename T, int VEC, int ITEMS>
__global__ void ln_bwd_dx_kernel(const T* __restrict__ dy,
                                 const T* __restrict__ x,
                                 const float* __restrict__ gamma,
                                 const float* __restrict__ mean,
                                 const float* __restrict__ rstd,
                                 T* __restrict__ dx, int rows, int H) {
  __shared__ float red[32];
  const int row = blockIdx.x;
  if (row >= rows) return;
  const int64_t base = static_cast<int64_t>(row) * H;
  const float mu = mean[row], rs = rstd[row];

  float dw[ITEMS][VEC], xh[ITEMS][VEC];
  int cols[ITEMS];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int c = (i * blockDim.x + threadIdx.x) * VEC;
    cols[i] = c;
    if (c < H) {
      T dt[VEC], xt[VEC];
      load_slice(dy + base + c, dt);
      load_slice(x + base + c, xt);
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        ln_bwd_elem(xt[k], dt[k], &gamma[c + k], mu, rs, dw[i][k], xh[i][k],
                    s1, s2);
    }
  }
  ln_bwd_row_means(s1, s2, H, red);
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int c = cols[i];
    if (c < H) {
      T o[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        o[k] = DTraits<T>::from_f32(
            ln_bwd_dz(dw[i][k], xh[i][k], rs, s1, s2));
      store_slice(dx + base + c, o);
    }
  }
}

// Column stats for the LN family backward: streaming column reduction
//   dgamma[c] += dy[r][c] * (z[r][c]-mu)*rs,  dbeta[c] += dy[r][c]
//   (+ dbias[c] += dx_src[r][c] when dx_src != nullptr)
// Each thread owns VEC contiguous columns and loops its row chunk with
// independent (software-pipelineable) loads; partials [n_chunks, nsl*H]
// are folded by col_reduce_full. Shared by ln_bwd and bdrl_bwd.
template <typename T, int VEC, bool HAS_BIAS>
__global__ void col_stats_kernel(const T* __restrict__ dy,
                                 const T* __restrict__ z,
                                 const T* __restrict__ dx_src,
                                 const float* __restrict__ mean,
                                 const float* __restrict__ rstd,
                                 float* __restrict__ part, int rows, int H,
                                 int rows_per_chunk) {
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (c >= H) return;
  const int r0 = blockIdx.y * rows_per_chunk;
  const int r1 = min(r0 + rows_per_chunk, rows);
  float acc_g[VEC] = {}, acc_b[VEC] = {}, acc_bias[VEC] = {};
  for (int r = r0; r < r1; ++r) {
    const int64_t base = static_cast<int64_t>(r) * H + c;
    const float mu = mean[r], rs = rstd[r];
    T dt[VEC], zt[VEC], xt[VEC];
    *reinterpret_cast<uint4*>(dt) = *reinterpret_cast<const uint4*>(dy + base);
    *reinterpret_cast<uint4*>(zt) = *reinterpret_cast<const uint4*>(z + base);
    if (HAS_BIAS)
      *reinterpret_cast<uint4*>(xt) =
          *reinterpret_cast<const uint4*>(dx_src + base);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float d = DTraits<T>::to_f32(dt[k]);
      acc_g[k] += d * (DTraits<T>::to_f32(zt[k]) - mu) * rs;
      acc_b[k] += d;
      if (HAS_BIAS) acc_bias[k] += DTraits<T>::to_f32(xt[k]);
    }
  }
  const int nsl = HAS_BIAS ? 3 : 2;
  float* p = part + static_cast<int64_t>(blockIdx.y) * nsl * H + c;
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    p[k] = acc_g[k];
    p[H + k] = acc_b[k];
    if (HAS_BIAS) p[2 * H + k] = acc_bias[k];
  }
}

// Deterministic blocked column reduce: out[j][c] = sum over the j-th
// contiguous row block of parts[p][c]. Each thread owns 4 consecutive
// fp32 columns (one uint4 per row) and streams its rows sequentially —
// coalesced across lanes AND sequential in p, so the sweep runs at HBM
// rate (the first strided-rows version thrashed; a single direct pass
// had only ~S/256 blocks). Direct store: no atomics, no zero-fill.
__global__ void col_reduce_blocked_kernel(const float* __restrict__ parts,
                                          int nparts, int S, int rows_per_j,
                                          float* __restrict__ out) {
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (c >= S) return;
  const int p0 = blockIdx.y * rows_per_j;
  const int p1 = min(p0 + rows_per_j, nparts);
  float acc[4] = {};
  for (int p = p0; p < p1; ++p) {
    const float* src = parts + static_cast<int64_t>(p) * S + c;
    if (c + 4 <= S) {
      float v[4];
      *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(src);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] += v[k];
    } else {
      for (int k = 0; c + k < S; ++k) acc[k] += src[k];
    }
  }
  float* dst = out + static_cast<int64_t>(blockIdx.y) * S + c;
  for (int k = 0; k < 4 && c + k < S; ++k) dst[k] = acc[k];
}

// One-launch variant for many partial rows: `chunk` rows per y-block,
// each y-block stores its chunk sum to tmp[y][S]; the y-block that
// arrives last at its column strip (integer ticket in counters[x]) folds
// tmp in y order. Same parallelism as accumulating with float atomics
// (fastest at the [0.7k-1.5k rows, 2-12k cols] partial shapes), but the
// summation order is fixed, so the result is bitwise identical from run
// to run; float atomics land in arrival order and are not.
__global__ void col_reduce_ordered_kernel(const float* __restrict__ parts,
                                          int nparts, int S, int chunk,
                                          float* __restrict__ tmp,
                                          unsigned int* __restrict__ counters,
                                          float* __restrict__ out) {
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const bool active = c < S;
  if (active) {
    const int p0 = blockIdx.y * chunk;
    const int p1 = min(p0 + chunk, nparts);
    float acc[4] = {};
    for (int p = p0; p < p1; ++p) {
      const float* src = parts + static_cast<int64_t>(p) * S + c;
      if (c + 4 <= S) {
        float v[4];
        *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(src);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += v[k];
      } else {
        for (int k = 0; c + k < S; ++k) acc[k] += src[k];
      }
    }
    float* dst = tmp + static_cast<int64_t>(blockIdx.y) * S + c;
    for (int k = 0; k < 4 && c + k < S; ++k) dst[k] = acc[k];
  }
  __threadfence();  // chunk sums visible device-wide before the ticket
  __shared__ bool is_last;
  __syncthreads();
  if (threadIdx.x == 0)
    is_last = atomicAdd(&counters[blockIdx.x], 1u) == gridDim.y - 1;
  __syncthreads();
  if (!is_last || !active) return;
  __threadfence();
  // The writers fenced (agent scope) before taking their ticket, and the
  // agent-scope fence above, after this block saw the last ticket,
  // invalidates this CU's vector cache; so the plain wide loads below see
  // every block's stores. kFoldBatch rows are loaded at a time so their
  // latencies overlap; they are added in y order.
  constexpr int kFoldBatch = 16;
  const int ny = static_cast<int>(gridDim.y);
  const int nk = min(4, S - c);
  float sum[4] = {};
  for (int j0 = 0; j0 < ny; j0 += kFoldBatch) {
    float v[kFoldBatch][4];
#pragma unroll
    for (int u = 0; u < kFoldBatch; ++u) {
      // rows past ny re-read the last row; their values are not added
      const int j = min(j0 + u, ny - 1);
      const float* src = tmp + static_cast<int64_t>(j) * S + c;
      if (nk == 4) {
        *reinterpret_cast<uint4*>(v[u]) =
            *reinterpret_cast<const uint4*>(src);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[u][k] = k < nk ? src[k] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < kFoldBatch; ++u)
      if (j0 + u < ny) {
        for (int k = 0; k < 4; ++k) sum[k] += v[u][k];
      }
  }
  for (int k = 0; k < nk; ++k) out[c + k] = sum[k];
}

// partial rows per y-block of col_reduce_ordered_kernel: measured best of
// 16/32/64/128 (fewer chunk sums shorten the last block's fold, longer
// chunks cost parallelism in the first phase)
constexpr int kColChunk = 32;

torch::Tensor col_reduce_full(torch::Tensor parts) {
  const int nparts = parts.size(0);
  const int S = parts.size(1);
  auto stream = at::hip::getCurrentHIPStream();
  const int xblocks = (S / 4 + 255) / 256;
  if (nparts <= 48) {
    auto out = torch::empty({S}, parts.options());
    hipLaunchKernelGGL(col_reduce_blocked_kernel, dim3(xblocks, 1),
                       dim3(256), 0, stream, parts.data_ptr<float>(), nparts,
                       S, nparts, out.data_ptr<float>());
    return out;
  }
  const int chunk = kColChunk;
  const int yblocks = (nparts + chunk - 1) / chunk;
  auto out = torch::empty({S}, parts.options());
  auto tmp = torch::empty({yblocks, S}, parts.options());
  auto counters = torch::zeros({xblocks}, parts.options().dtype(torch::kInt32));
  dim3 grid(xblocks, yblocks);
  hipLaunchKernelGGL(col_reduce_ordered_kernel, grid, dim3(256), 0, stream,
                     parts.data_ptr<float>(), nparts, S, chunk,
                     tmp.data_ptr<float>(),
                     reinterpret_cast<unsigned int*>(counters.data_ptr<int>()),
                     out.data_ptr<float>());
  return out;
}

// dgamma | dbeta (| dbias, when dx_src is defined) of the LN family
// backward as one fp32 [nsl * H] vector: col_stats_kernel partials over
// row chunks, folded by col_reduce_full.
torch::Tensor col_stats(torch::Tensor dy, torch::Tensor z,
                        torch::Tensor dx_src, torch::Tensor mean,
                        torch::Tensor rstd) {
  const int rows = z.size(0), H = z.size(1);
  const int rows_per_chunk = 16;  // halves partial-buffer traffic; 16 independent loads/thread
  const int n_chunks = (rows + rows_per_chunk - 1) / rows_per_chunk;
  const bool has_bias = dx_src.defined();
  auto part = torch::empty({n_chunks, (has_bias ? 3 : 2) * H},
                           z.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_ROW_DTYPE(z.scalar_type(), "col_stats", [&] {
    const int threads = tmin(256, ((H / kVec + 63) / 64) * 64);
    dim3 grid((H / kVec + threads - 1) / threads, n_chunks);
    by_flag(has_bias, [&](auto bias_c) {
      hipLaunchKernelGGL(
          (col_stats_kernel<scalar_t, kVec, decltype(bias_c)::value>), grid,
          dim3(threads), 0, stream, dptr<scalar_t>(dy), dptr<scalar_t>(z),
          has_bias ? dptr<scalar_t>(dx_src) : nullptr, mean.data_ptr<float>(),
          rstd.data_ptr<float>(), part.data_ptr<float>(), rows, H,
          rows_per_chunk);
    });
  });
  return col_reduce_full(part);
}

std::vector<torch::Tensor> ln_fwd(torch::Tensor x, torch::Tensor gamma,
                                  torch::Tensor beta, double eps) {
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous(), "ln_fwd: x must be 2D contiguous");
  const int rows = x.size(0), H = x.size(1);
  auto gamma_f = gamma.contiguous().to(torch::kFloat32);
  auto beta_f = beta.contiguous().to(torch::kFloat32);
  auto y = torch::empty_like(x);
  auto opts = x.options().dtype(torch::kFloat32);
  auto mean = torch::empty({rows}, opts);
  auto rstd = torch::empty({rows}, opts);
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_ROW_DTYPE(x.scalar_type(), "ln_fwd", [&] {
    TORCH_CHECK(H % kVec == 0, "ln_fwd: H must be a multiple of ", kVec);
    launch_by_items("ln_fwd", H / kVec, [&](auto items_c, int threads) {
      hipLaunchKernelGGL(
          (ln_fwd_kernel<scalar_t, kVec, decltype(items_c)::value>),
          dim3(rows), dim3(threads), 0, stream, dptr<scalar_t>(x),
          gamma_f.data_ptr<float>(), beta_f.data_ptr<float>(),
          dptr<scalar_t>(y), mean.data_ptr<float>(), rstd.data_ptr<float>(),
          rows, H, static_cast<float>(eps));
    });
  });
  return {y, mean, rstd};
}

std::vector<torch::Tensor> ln_bwd(torch::Tensor dy, torch::Tensor x,
                                  torch::Tensor gamma, torch::Tensor mean,
                                  torch::Tensor rstd) {
  check_rows_2d("ln_bwd", "x", x);
  check_like("ln_bwd", "dy", dy, "x", x);
  const int rows = x.size(0), H = x.size(1);
  check_row_stat("ln_bwd", "mean", mean, rows);
  check_row_stat("ln_bwd", "rstd", rstd, rows);
  check_param("ln_bwd", "gamma", gamma, H);
  auto gamma_f = gamma.contiguous().to(torch::kFloat32);
  auto dx = torch::empty_like(x);
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_ROW_DTYPE(x.scalar_type(), "ln_bwd", [&] {
    TORCH_CHECK(H % kVec == 0, "ln_bwd: H must be a multiple of ", kVec);
    launch_by_items("ln_bwd", H / kVec, [&](auto items_c, int threads) {
      hipLaunchKernelGGL(
          (ln_bwd_dx_kernel<scalar_t, kVec, decltype(items_c)::value>),
          dim3(rows), dim3(threads), 0, stream, dptr<scalar_t>(dy),
          dptr<scalar_t>(x), gamma_f.data_ptr<float>(),
          mean.data_ptr<float>(), rstd.data_ptr<float>(), dptr<scalar_t>(dx),
          rows, H);
    });
  });
  auto dgb = col_stats(dy, x, torch::Tensor(), mean, rstd);
  auto dgamma = dgb.narrow(0, 0, H);
  auto dbeta = dgb.narrow(0, H, H);
  if (gamma.scalar_type() != torch::kFloat32) {
    return {dx, dgamma.to(gamma.scalar_type()), dbeta.to(gamma.scalar_type())};
  }
  return {dx, dgamma.contiguous(), dbeta.contiguous()};
}

}  // namespace bpa
