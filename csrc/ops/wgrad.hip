// Hand-written split-K MFMA weight-gradient GEMM for MI355X (gfx950).
//
// dW[M,N] = dy^T @ x with dy [K,M] and x [K,N] row-major bf16 or fp16
// (kernels templated on the element type, csrc/mfma_types.h) (the
// "TN" wgrad form of every encoder linear: QKV [3072,1024], attn-out
// [1024,1024], FFN1 [4096,1024], FFN2 [1024,4096] at K = B*S tokens).
// hipBLASLt/rocBLAS top out at ~580-790 TF/s on these shapes even
// under an exhaustive TunableOp search because the output is small:
// a 128^2-tiled launch is only 64-256 workgroups on a 256-CU chip.
// Splitting K across gridDim.z restores occupancy; fp32 partial tiles
// are summed and cast by a tiny combine kernel (fp32 accumulation
// end-to-end - tighter than the library's bf16 epilogue path).
//
// Structure per block (256 threads = 4 waves as 2x2): C tile 128x128,
// K loop in 64-deep steps; both operands staged [64][128] natural
// row-major in LDS (padded stride 144 elems = 72 dwords: the
// transpose-read's {72r*... = 8r + 2c} bank pattern covers every even
// bank exactly once - conflict-free) and their k-strided MFMA
// fragments produced by ds_read_b64_tr_b16 (frag_tr, csrc/mfma_frag.h,
// shared with csrc/ops/attention.hip; semantics probe-verified by
// tr16_probe, csrc/ops/mfma_probe.hip).
// Staging is split issue-early/write-late (T14): the next k-step's
// global loads issue before this step's 32 MFMAs per wave, so HBM
// latency hides under the matrix work; double-buffered LDS, one
// barrier pair per k-step. The k-loop itself is tn_mainloop
// (tn_mainloop.h), shared with the K-FAC factor kernel
// (kfac_factor.hip).
//
// Reference op being replaced: the implicit wgrad GEMMs of
// src/modeling.py's nn.Linear calls (SURVEY.md §2.4 "Backward of all
// of the above").

#include <torch/extension.h>
#include <cstdlib>
#include <ATen/hip/HIPContext.h>

#include "../common.h"
#include "../ops.h"
#include "tn_mainloop.h"

namespace bpa {

// grid: (M/128, N/128, splitk); block 256. BK = 32 or 64: 64 halves
// the barrier count and doubles the MFMA run per staged tile (36.8 ->
// 73.7 KB LDS, 4 -> 2 blocks/CU); which wins is per-shape (sweep in
// benchmarks/wgrad_sweep.py) and picked by the host wrapper.
template <typename T, int BK>
__global__ __launch_bounds__(256) void wgrad_tn_kernel(
    const T* __restrict__ dy,  // [K, M]
    const T* __restrict__ x,   // [K, N]
    float* __restrict__ part,       // [splitk, M, N]
    int K, int M, int N, int k_slice) {
  const int m0 = blockIdx.x * wg::kBM;
  const int n0 = blockIdx.y * wg::kBN;
  const int kz0 = blockIdx.z * k_slice;
  const int kz1 = min(K, kz0 + k_slice);
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1;  // 2x2 wave grid, 64x64 each
  const int g = (lane >> 4), li = lane & 15;

  // single LDS base + offset arithmetic: a runtime-indexed POINTER
  // ARRAY here makes hipcc lose the LDS address space and emit
  // flat_store for the staging writes (observed in the .s; 2-3x the
  // ds_write cost plus per-store 64-bit compares)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* lds = reinterpret_cast<T*>(smem);

  f32x4 acc[4][4] = {};
  tn_mainloop<T, BK>(dy, M, m0, x, N, n0, K, kz0, kz1, lds, acc);

  // epilogue: fp32 partial tile [M,N] for this k-slice
  float* out = part + static_cast<int64_t>(blockIdx.z) * M * N;
#pragma unroll
  for (int ti = 0; ti < 4; ++ti) {
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int mi = m0 + wi * 64 + ti * 16 + g * 4 + r;
        const int nj = n0 + wj * 64 + tj * 16 + li;
        out[static_cast<int64_t>(mi) * N + nj] = acc[ti][tj][r];
      }
    }
  }
}

// part [S, M, N] fp32 -> out [M, N] bf16/fp16 (sum over S). The final
// narrowing rounds to nearest-even; for fp16 a sum beyond +-65504
// becomes +-inf, never a clamped finite value (the GradScaler's
// overflow detection depends on it).
// ACC: out holds a gradient already and gets out = T(float(out) +
// float(T(sum))). The inner rounding to T is the one the plain store makes
// and the outer one is a 16-bit tensor add's, so the result is bit for bit
// that of adding the stored dW to out afterwards.
template <typename T, bool ACC>
__global__ void wgrad_combine_kernel(const float* __restrict__ part,
                                     T* __restrict__ out, int splitk,
                                     int64_t mn) {
  using Tr = Mfma16<T>;
  const int64_t i =
      (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) * 4;
  if (i >= mn) return;
  f32x4 s = *reinterpret_cast<const f32x4*>(part + i);
  for (int z = 1; z < splitk; ++z) {
    f32x4 p = *reinterpret_cast<const f32x4*>(
        part + static_cast<int64_t>(z) * mn + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += p[k];
  }
  T o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = Tr::from_f32(s[k]);
  if (ACC) {
    T a[4];
    *reinterpret_cast<uint2*>(a) = *reinterpret_cast<const uint2*>(out + i);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      o[k] = Tr::from_f32(Tr::to_f32(a[k]) + Tr::to_f32(o[k]));
  }
  *reinterpret_cast<uint2*>(out + i) = *reinterpret_cast<uint2*>(o);
}

bool wgrad_tn_supported(int64_t K, int64_t M, int64_t N) {
  // staging reads whole uint4s per row: K rows need no alignment, but
  // M/N must tile exactly and K must be large enough to amortize
  return M % wg::kBM == 0 && N % wg::kBN == 0 && K % 4 == 0 && K >= 256;
}

bool wgrad_tn_profitable(int64_t K, int64_t M, int64_t N) {
  // where this kernel MEASURED >= hipBLASLt/rocBLAS (gemm_shapes.py):
  // tall-M, N=1024 shapes (QKV/FFN1/attn-out wgrad). N > 1024 (FFN2)
  // and very tall M (MLM decoder) stay on the library.
  return wgrad_tn_supported(K, M, N) && N <= 1024 && M >= 1024 &&
         M <= 8192 && K >= 4096;
}

template <typename T>
static torch::Tensor wgrad_tn_t(torch::Tensor dy, torch::Tensor x,
                                int64_t splitk_override,
                                const c10::optional<torch::Tensor>& acc) {
  const int K = dy.size(0), M = dy.size(1), N = x.size(1);
  TORCH_CHECK(x.size(0) == K, "wgrad_tn: K mismatch");
  TORCH_CHECK(wgrad_tn_supported(K, M, N), "wgrad_tn: unsupported shape");
  const int tiles = (M / wg::kBM) * (N / wg::kBN);
  // k-step depth: 64 halves barriers / doubles the MFMA run per tile
  // at 2 blocks/CU; override with BPA_WGRAD_BK for sweeps
  const char* env_bk = getenv("BPA_WGRAD_BK");  // per-call: sweepable
  int bk = env_bk ? atoi(env_bk) : 32;
  TORCH_CHECK(bk == 32 || bk == 64, "wgrad_tn: BK must be 32 or 64");
  // split-K sweep on MI355X (benchmarks/wgrad_sweep.py): best wall time
  // lands at tiles*splitk ~ 512-768 with splitk <= 8 (beyond that the
  // fp32 slab traffic of the combine outweighs the occupancy gain):
  // QKV 127->99us (splitk 4), attn-out 56->42 (8), FFN1 ~tie (3)
  int splitk = 1;
  while (splitk < 8 && tiles * (splitk + 1) <= 768 &&
         K / (splitk + 1) >= 8 * wg::kBK)
    ++splitk;
  if (splitk_override > 0) splitk = static_cast<int>(splitk_override);
  int k_slice = ((K + splitk - 1) / splitk + bk - 1) / bk * bk;
  splitk = (K + k_slice - 1) / k_slice;  // drop empty tail slices

  auto part = torch::empty({splitk, static_cast<int64_t>(M), N},
                           dy.options().dtype(torch::kFloat32));
  // with acc the combine adds into it and nothing is returned
  auto out = acc.has_value()
                 ? *acc
                 : torch::empty({static_cast<int64_t>(M), N}, dy.options());
  auto stream = at::hip::getCurrentHIPStream();
  dim3 grid(M / wg::kBM, N / wg::kBN, splitk), block(256);
  // two double-buffered [bk][kStride] images (dy, x)
  const size_t lds = 4 * bk * wg::kStride * sizeof(T);
  auto launch = [&](auto kernel) {
    HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(kernel, grid, block, lds, stream,
                       reinterpret_cast<const T*>(dy.data_ptr()),
                       reinterpret_cast<const T*>(x.data_ptr()),
                       part.data_ptr<float>(), K, M, N, k_slice);
  };
  if (bk == 64)
    launch(&wgrad_tn_kernel<T, 64>);
  else
    launch(&wgrad_tn_kernel<T, 32>);
  const int64_t mn = static_cast<int64_t>(M) * N;
  const dim3 cgrid((mn / 4 + 255) / 256);
  if (acc.has_value()) {
    hipLaunchKernelGGL((wgrad_combine_kernel<T, true>), cgrid, dim3(256), 0,
                       stream, part.data_ptr<float>(),
                       reinterpret_cast<T*>(out.data_ptr()), splitk, mn);
    return torch::Tensor();
  }
  hipLaunchKernelGGL((wgrad_combine_kernel<T, false>), cgrid, dim3(256), 0,
                     stream, part.data_ptr<float>(),
                     reinterpret_cast<T*>(out.data_ptr()), splitk, mn);
  return out;
}

// dW = dy^T @ x; dy [K,M] row-major contiguous, x [K,N] likewise, both
// bf16 or both fp16; dW comes back in the same dtype, or, with `acc`
// ([M, N] contiguous, same dtype and device), is added to acc in place.
torch::Tensor wgrad_tn(torch::Tensor dy, torch::Tensor x,
                       int64_t splitk_override,
                       c10::optional<torch::Tensor> acc) {
  const auto dt = dy.scalar_type();
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 2 && dy.is_contiguous() &&
                  (dt == torch::kBFloat16 || dt == torch::kHalf),
              "wgrad_tn: dy must be contiguous 2D bf16 or fp16");
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous(),
              "wgrad_tn: x must be contiguous 2D");
  TORCH_CHECK(x.scalar_type() == dt, "wgrad_tn: x dtype ", x.scalar_type(),
              " does not match dy dtype ", dt);
  if (acc.has_value()) {
    TORCH_CHECK(acc->device() == dy.device(), "wgrad_tn: acc device ",
                acc->device(), " does not match dy device ", dy.device());
    TORCH_CHECK(acc->scalar_type() == dt, "wgrad_tn: acc dtype ",
                acc->scalar_type(), " does not match dy dtype ", dt);
    TORCH_CHECK(acc->dim() == 2 && acc->size(0) == dy.size(1) &&
                    acc->size(1) == x.size(1) && acc->is_contiguous(),
                "wgrad_tn: acc must be contiguous [", dy.size(1), ", ",
                x.size(1), "], got ", acc->sizes());
  }
  if (dt == torch::kHalf)
    return wgrad_tn_t<_Float16>(dy, x, splitk_override, acc);
  return wgrad_tn_t<__bf16>(dy, x, splitk_override, acc);
}

}  // namespace bpa
