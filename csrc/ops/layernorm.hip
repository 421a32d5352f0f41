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
// * backward: one pass (ln_bwd_rows_kernel, rowwise.h). A block owns a
//   group of consecutive rows, several of them in flight side by side;
//   dx is written from registers and dgamma/dbeta are accumulated in the
//   same registers across the block's rows, so dy and x are read once.
//   The [nblocks, 2H] partials are folded by col_reduce_full.
//
// The row cores (two-pass mean/rstd, affine, the backward pass) are in
// rowwise.h, shared with fused_residual.hip and embedding.hip;
// col_reduce_full below is declared in ops.h for the other files.

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

// sum[k] += rows r0 .. r1-1 of the 4-column strip at column c of a [*, S]
// fp32 matrix, added in row order (nk = min(4, S - c) columns are real).
// kStripBatch rows are loaded at a time so that their latencies overlap:
// a loop of load-then-add pays one memory round trip per row.
constexpr int kStripBatch = 16;

__device__ __forceinline__ void strip_sum(const float* __restrict__ m, int r0,
                                          int r1, int S, int c, int nk,
                                          float (&sum)[4]) {
  for (int j0 = r0; j0 < r1; j0 += kStripBatch) {
    float v[kStripBatch][4];
#pragma unroll
    for (int u = 0; u < kStripBatch; ++u) {
      // rows past r1 re-read the last row; their values are not added
      const int j = min(j0 + u, r1 - 1);
      const float* src = m + static_cast<int64_t>(j) * S + c;
      if (nk == 4) {
        *reinterpret_cast<uint4*>(v[u]) =
            *reinterpret_cast<const uint4*>(src);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[u][k] = k < nk ? src[k] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < kStripBatch; ++u)
      if (j0 + u < r1) {
        for (int k = 0; k < 4; ++k) sum[k] += v[u][k];
      }
  }
}

// Where the fold's result goes. The [S] result is cut into S / seg
// segments of seg columns (dgamma | dbeta | dbias, ...); a segment with a
// destination is ADDED to it, dst[c] = dst[c] + round(sum), the fp32 add
// autograd's gradient accumulation would make on the stored result, and a
// segment without one is stored to out. round: 0 keeps the fp32 sum, 1 / 2
// round it through bf16 / fp16 first (a gradient that reaches its fp32
// parameter through a 16-bit cast). seg is a multiple of 4 whenever a
// destination is set, so a thread's 4 columns share one segment.
struct FoldDst {
  float* d0;
  float* d1;
  float* d2;
  int seg;
  int round;
};

__device__ __forceinline__ float fold_round(float v, int round) {
  if (round == 1) return __bfloat162float(__float2bfloat16(v));
  if (round == 2) return __half2float(__float2half(v));
  return v;
}

__device__ __forceinline__ void fold_store(const FoldDst& fd, float* out,
                                           int c, int nk,
                                           const float (&sum)[4]) {
  const int s = c / fd.seg;
  float* d = s == 0 ? fd.d0 : s == 1 ? fd.d1 : s == 2 ? fd.d2 : nullptr;
  if (d != nullptr) {
    d += c - s * fd.seg;
    for (int k = 0; k < nk; ++k) d[k] = d[k] + fold_round(sum[k], fd.round);
  } else {
    for (int k = 0; k < nk; ++k) out[c + k] = sum[k];
  }
}

// Deterministic blocked column reduce: out[j][c] = sum over the j-th
// contiguous row block of parts[p][c]. Each thread owns 4 consecutive
// fp32 columns (one uint4 per row) and adds its rows in order. Direct
// store: no atomics, no zero-fill.
__global__ void col_reduce_blocked_kernel(const float* __restrict__ parts,
                                          int nparts, int S, int rows_per_j,
                                          float* __restrict__ out,
                                          FoldDst fd) {
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (c >= S) return;
  const int p0 = blockIdx.y * rows_per_j;
  const int p1 = min(p0 + rows_per_j, nparts);
  const int nk = min(4, S - c);
  float acc[4] = {};
  strip_sum(parts, p0, p1, S, c, nk, acc);
  fold_store(fd, out + static_cast<int64_t>(blockIdx.y) * S, c, nk, acc);
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
                                          float* __restrict__ out,
                                          FoldDst fd) {
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const bool active = c < S;
  const int nk = min(4, S - c);
  if (active) {
    const int p0 = blockIdx.y * chunk;
    const int p1 = min(p0 + chunk, nparts);
    float acc[4] = {};
    strip_sum(parts, p0, p1, S, c, nk, acc);
    float* dst = tmp + static_cast<int64_t>(blockIdx.y) * S + c;
    for (int k = 0; k < nk; ++k) dst[k] = acc[k];
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
  // invalidates this CU's vector cache; so the plain wide loads of
  // strip_sum see every block's stores.
  float sum[4] = {};
  strip_sum(tmp, 0, static_cast<int>(gridDim.y), S, c, nk, sum);
  fold_store(fd, out, c, nk, sum);
}

// partial rows per y-block of col_reduce_ordered_kernel: measured best of
// 16/32/64/128 (fewer chunk sums shorten the last block's fold, longer
// chunks cost parallelism in the first phase)
constexpr int kColChunk = 32;

torch::Tensor col_reduce_full(torch::Tensor parts,
                              const std::vector<c10::optional<torch::Tensor>>& dsts,
                              c10::optional<torch::ScalarType> round_to) {
  const int nparts = parts.size(0);
  const int S = parts.size(1);
  FoldDst fd{nullptr, nullptr, nullptr, S > 0 ? S : 1, 0};
  if (!dsts.empty()) {
    const int nseg = static_cast<int>(dsts.size());
    TORCH_CHECK(nseg <= 3 && S % nseg == 0 && (S / nseg) % 4 == 0,
                "col_reduce_full: ", nseg, " destinations do not cut ", S,
                " columns into segments of a multiple of 4");
    fd.seg = S / nseg;
    float** slot[3] = {&fd.d0, &fd.d1, &fd.d2};
    for (int i = 0; i < nseg; ++i) {
      if (!dsts[i].has_value()) continue;
      check_accum_dst("col_reduce_full", "destination", *dsts[i], parts,
                      fd.seg);
      *slot[i] = dsts[i]->data_ptr<float>();
    }
    if (round_to.has_value() && *round_to != torch::kFloat32) {
      TORCH_CHECK(*round_to == torch::kBFloat16 || *round_to == torch::kHalf,
                  "col_reduce_full: cannot round through ", *round_to);
      fd.round = *round_to == torch::kBFloat16 ? 1 : 2;
    }
  }
  auto stream = at::hip::getCurrentHIPStream();
  const int xblocks = (S / 4 + 255) / 256;
  auto out = torch::empty({S}, parts.options());
  if (nparts <= 48) {
    hipLaunchKernelGGL(col_reduce_blocked_kernel, dim3(xblocks, 1),
                       dim3(256), 0, stream, parts.data_ptr<float>(), nparts,
                       S, nparts, out.data_ptr<float>(), fd);
    return out;
  }
  const int chunk = kColChunk;
  const int yblocks = (nparts + chunk - 1) / chunk;
  auto tmp = torch::empty({yblocks, S}, parts.options());
  auto counters = torch::zeros({xblocks}, parts.options().dtype(torch::kInt32));
  dim3 grid(xblocks, yblocks);
  hipLaunchKernelGGL(col_reduce_ordered_kernel, grid, dim3(256), 0, stream,
                     parts.data_ptr<float>(), nparts, S, chunk,
                     tmp.data_ptr<float>(),
                     reinterpret_cast<unsigned int*>(counters.data_ptr<int>()),
                     out.data_ptr<float>(), fd);
  return out;
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
                                  torch::Tensor rstd,
                                  c10::optional<torch::Tensor> dgamma_acc,
                                  c10::optional<torch::Tensor> dbeta_acc) {
  check_rows_2d("ln_bwd", "x", x);
  check_like("ln_bwd", "dy", dy, "x", x);
  const int rows = x.size(0), H = x.size(1);
  check_row_stat("ln_bwd", "mean", mean, rows);
  check_row_stat("ln_bwd", "rstd", rstd, rows);
  check_param("ln_bwd", "gamma", gamma, H);
  check_accum_dst("ln_bwd", "dgamma_acc", dgamma_acc, x, H);
  check_accum_dst("ln_bwd", "dbeta_acc", dbeta_acc, x, H);
  // a gradient with a destination is added there and comes back undefined
  const bool fused = dgamma_acc.has_value() || dbeta_acc.has_value();
  TORCH_CHECK(!fused || gamma.scalar_type() == torch::kFloat32,
              "ln_bwd: accumulating outputs need fp32 gamma");
  auto gamma_f = gamma.contiguous().to(torch::kFloat32);
  auto dx = torch::empty_like(x);
  auto stream = at::hip::getCurrentHIPStream();
  torch::Tensor part, none;
  DISPATCH_ROW_DTYPE(x.scalar_type(), "ln_bwd", [&] {
    TORCH_CHECK(H % kVec == 0, "ln_bwd: H must be a multiple of ", kVec);
    part = ln_bwd_rows<scalar_t, kVec, false>("ln_bwd", dy, none, x, none,
                                              gamma_f, mean, rstd, dx, none,
                                              0.0, false, stream);
  });
  auto dgb = fused ? col_reduce_full(part, {dgamma_acc, dbeta_acc})
                   : col_reduce_full(part);
  auto dgamma = dgamma_acc.has_value() ? torch::Tensor() : dgb.narrow(0, 0, H);
  auto dbeta = dbeta_acc.has_value() ? torch::Tensor() : dgb.narrow(0, H, H);
  if (gamma.scalar_type() != torch::kFloat32) {
    return {dx, dgamma.to(gamma.scalar_type()), dbeta.to(gamma.scalar_type())};
  }
  return {dx, dgamma, dbeta};
}

}  // namespace bpa
