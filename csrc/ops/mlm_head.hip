// Hand-written MFMA MLM-decoder GEMM with fused bias + cross-entropy
// forward for MI355X (gfx950).
//
// logits[P,V] = h[P,K] @ W[V,K]^T + bias[V], V = vocab (~30528),
// K = hidden (1024), P = gathered masked rows (B * max_preds) — the
// single biggest GEMM of the reference's MLM head
// (src/modeling.py:570-578 decoder matmul + run_pretraining.py:58-72
// CrossEntropyLoss). One kernel computes the GEMM, adds the bias, and
// produces the cross-entropy forward statistics in the epilogue:
// per-(row, 64-column-stripe) online (max, sum-exp) fp32 partials
// folded by a tiny second kernel into the per-row logsumexp + NLL
// loss. The separate full [P,V] read of a standalone CE-forward pass
// disappears; backward reuses ce_bwd (csrc/ops/cross_entropy.hip) on
// the bf16 logits this kernel stores.
//
// Tile choice (measured, see docs/KERNELS.md): 128x128 and
// stripe-persistent (W-streamed-once) structures both landed 210-300us
// against hipBLASLt's ~92us — PMC showed waves parked 5.7x their busy
// cycles; this shape is bound by on-chip operand re-reads and MFMA
// work per barrier, not HBM (the 62.5-MB W matrix is L3-resident,
// Infinity Cache = 256 MB). The library's own pick is a 256x256
// macro-tile, which quadruples FLOPs per staged byte; this kernel uses
// the same: 512 threads = 8 waves as 2(M)x4(N), each wave a 128x64
// sub-tile (acc 128 regs), BK=64 double-buffered global_load_lds
// (128 KB LDS, one block per CU), one __syncthreads per k-step.
//
// LDS images are lane-linear (glds writes wave-uniform base +
// lane*16), so the SOURCE address carries a 16-B-granule XOR swizzle:
//   LDS[row r][granule p] = global[row r][granule p ^ (r & 7)]
// A row is one 128-B cache line and the permutation stays inside it,
// so coalescing is untouched; fragment b64 reads spread each 16-lane
// group over 8 granules (2-way conflict), noise under the MFMAs.
//
// Numerics: fp32 MFMA accumulation; the CE statistics are computed
// from the bf16-ROUNDED logits (exactly the values backward re-reads),
// so forward lse and backward softmax see identical inputs. The
// kernels are templated on the 16-bit element type (csrc/mfma_types.h):
// with fp16 inputs the logits are fp16 and "bf16" above reads "fp16".
//
// Evaluation instantiation (EVAL = true, entry point mlm_head_eval): the
// same GEMM and the same statistics arithmetic, but nothing [P,V]-sized
// is written. The epilogue still rounds every logit to the 16-bit type
// (so lse and the loss equal the training kernel's bit for bit), and
//   * drops the logits store;
//   * tracks the arg-max column beside the running max: per lane in the
//     column loop, then across the 16-lane group (the lanes whose own
//     max equals the butterfly's result offer their column, a DPP
//     row-rotate min picks the lowest) and into a third word of the
//     per-(row, stripe) partial;
//   * has the one lane whose column equals labels[row] write that
//     rounded logit, widened to fp32, into a [P] buffer the fold kernel
//     reads in place of logits[row, label]. The block's 256 labels are
//     fetched before the k-loop and parked in LDS once it has drained.
// The fold kernel reduces (max, index, sum-exp) over stripes and emits
// pred[row] plus a per-row "correct" flag that mlm_sum_kernel sums
// beside loss and count. No atomics, nothing order-dependent.
// Tie rule: pred[row] is the LOWEST column index that attains the row
// maximum of the rounded logits (what torch.argmax documents on the
// CPU). Every merge keeps the smaller index on an equal max; a lane or
// stripe with no valid column carries (-inf, INT_MAX) and cannot win. A
// row with no logit above -inf (all -inf or NaN) predicts column 0.
// Tail rule: columns >= V never enter max, index or sum-exp (the cv[]
// mask), so the clamped W rows staged for them cannot be predicted.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../common.h"
#include "../ops.h"
#include "../mfma_types.h"

#include <climits>

namespace bpa {

namespace mh {

constexpr int kBM = 256;  // h-rows per block
constexpr int kBN = 256;  // vocab columns per block (4 x 64 stripes)
constexpr int kBK = 64;   // K step (two MFMA depths per staged tile)
constexpr int kATileB = kBM * kBK * 2;    // h image bytes (32 KB)
constexpr int kWTileB = kBN * kBK * 2;    // W image bytes (32 KB)
constexpr int kBufB = kATileB + kWTileB;  // one pipeline buffer (64 KB)

// element byte offset of (row r, k) inside one swizzled image
__device__ __forceinline__ int swz_off(int r, int k) {
  return r * (kBK * 2) + ((((k >> 3) ^ (r & 7)) << 4) | ((k & 7) << 1));
}

// fragment for MFMA depth base ks (0 or 32): lane (g = lane>>4,
// li = lane&15) holds row rb+li, k = ks+4g..+3 and ks+16+4g..+3 (the
// probe-verified gfx950 16x16x32 layout, shared by the bf16 and f16
// instructions). T is the 16-bit element type (csrc/mfma_types.h).
template <typename T>
__device__ __forceinline__ typename Mfma16<T>::frag frag_k(const char* img,
                                                           int rb, int ks) {
  using Tr = Mfma16<T>;
  using H4 = typename Tr::tr4;  // plain 8-byte chunk here, no transpose
  const int lane = threadIdx.x & 63;
  const int g = (lane >> 4) & 3, li = lane & 15;
  const int r = rb + li;
  union {
    typename Tr::frag v;
    H4 h[2];
  } f;
  f.h[0] = *reinterpret_cast<const H4*>(img + swz_off(r, ks + 4 * g));
  f.h[1] = *reinterpret_cast<const H4*>(img + swz_off(r, ks + 16 + 4 * g));
  return f.v;
}

// merge (m2, i2) into the running (mx, ix) arg-max: larger max wins, an
// equal max keeps the lower column
__device__ __forceinline__ int argmax_merge(float mx, int ix, float m2,
                                            int i2) {
  return m2 > mx ? i2 : (m2 == mx ? min(ix, i2) : ix);
}

// min over the 16 lanes of a DPP row (= one li-group), in every lane:
// row_ror:8/4/2/1, VALU only
__device__ __forceinline__ int row16_min(int v) {
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x128, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x124, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x122, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x121, 0xf, 0xf, false));
  return v;
}

}  // namespace mh

// grid: (P/256, ceil(V/256)); 512 threads = 8 waves as 2(M) x 4(N),
// each wave a 128x64 sub-tile. The wave's 64-col stripe is also the
// CE-partial granule, so row statistics never cross waves. EVAL: see the
// file header; logits is unused then, and labels/xlab are
// unused otherwise.
template <typename T, bool EVAL>
__global__ __launch_bounds__(512) void mlm_fwd_kernel(
    const T* __restrict__ h,     // [P, K]
    const T* __restrict__ w,     // [V, K]
    const float* __restrict__ bias,   // [V]
    T* __restrict__ logits,      // [P, V]
    float* __restrict__ part,  // [P, nStripes, 2] (max, sumexp), EVAL:
                               // [P, nStripes, 3] (.., arg-max column bits)
    int P, int V, int K, int nStripes,
    // EVAL only; last, so the training instantiation's arguments sit
    // where they always sat
    const int64_t* __restrict__ labels,  // [P]
    float* __restrict__ xlab) {       // [P] rounded logit at the label
  using Tr = Mfma16<T>;
  using F8 = typename Tr::frag;
  const int m0 = blockIdx.x * mh::kBM;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 2, wj = wave & 3;  // 2 x 4 wave grid
  const int g = (lane >> 4), li = lane & 15;
  const int stripe = blockIdx.y * 4 + wj;   // this wave's 64-col stripe
  const int n0 = blockIdx.y * mh::kBN;
  const int nw0 = n0 + wj * 64;

  extern __shared__ __attribute__((aligned(16))) char smem[];

  // per-wave column stripe is fixed: bias once, in registers
  const bool any = nw0 < V;                  // wave has valid columns
  const bool full = (nw0 + 64) <= V;
  float bv[4];
  bool cv[4];
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) {
    const int nj = nw0 + tj * 16 + li;
    cv[tj] = nj < V;
    bv[tj] = cv[tj] ? bias[nj] : 0.f;
  }

  // global_load_lds staging: per wave 4 A + 4 W calls x 8 rows x 128 B
  const int st_sub = (lane >> 3);                // row within 8-row piece
  const int st_swz = ((lane & 7) ^ st_sub) * 8;  // swizzled source granule
  auto stage = [&](int k0, int b) {
    char* base = smem + b * mh::kBufB;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int r = wave * 32 + c * 8 + st_sub;  // 0..255
      const T* ga =
          h + static_cast<int64_t>(m0 + r) * K + k0 + st_swz;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)ga,
          (__attribute__((address_space(3))) void*)(base +
                                                    (wave * 32 + c * 8) *
                                                        128),
          16, 0, 0);
      // vocab tail: clamp W row (always-legal; epilogue masks)
      const T* gw =
          w + static_cast<int64_t>(min(n0 + r, V - 1)) * K + k0 + st_swz;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)gw,
          (__attribute__((address_space(3))) void*)(base + mh::kATileB +
                                                    (wave * 32 + c * 8) *
                                                        128),
          16, 0, 0);
    }
  };

  // EVAL: row tid's label, in flight under the whole k-loop; anything
  // that is no column (ignore_index) becomes -1 and matches no lane
  int lab_own = -1;
  if constexpr (EVAL) {
    if (tid < mh::kBM) {
      const int64_t l = labels[m0 + tid];
      lab_own = (l >= 0 && l < V) ? static_cast<int>(l) : -1;
    }
  }

  f32x4 acc[8][4] = {};
  stage(0, 0);
  __syncthreads();

  int buf = 0;
  for (int k0 = 0; k0 < K; k0 += mh::kBK) {
    if (k0 + mh::kBK < K) stage(k0 + mh::kBK, buf ^ 1);  // DMA under MFMA
    const char* at = smem + buf * mh::kBufB;
    const char* wt = at + mh::kATileB;
#pragma unroll
    for (int kd = 0; kd < 2; ++kd) {  // two MFMA depths per staged tile
      F8 bfr[4];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        bfr[t] = mh::frag_k<T>(wt, wj * 64 + t * 16, kd * 32);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ti = 0; ti < 8; ++ti) {
        const F8 af = mh::frag_k<T>(at, wi * 128 + ti * 16, kd * 32);
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
          acc[ti][tj] = Tr::mfma(af, bfr[tj], acc[ti][tj]);
      }
      __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();
    buf ^= 1;
  }

  // ---- epilogue: bias, bf16 logits, per-stripe CE stats (no LDS) ----
  // EVAL: the k-loop's last barrier freed the LDS; it now holds the labels
  const int* lab_s = reinterpret_cast<const int*>(smem);
  if constexpr (EVAL) {
    if (tid < mh::kBM) reinterpret_cast<int*>(smem)[tid] = lab_own;
    __syncthreads();
  }
  if (!any) return;
#pragma unroll
  for (int ti = 0; ti < 8; ++ti) {
    int lab4[4] = {-1, -1, -1, -1};  // EVAL: labels of this lane's 4 rows
    if constexpr (EVAL) {
      const int4 l4 = *reinterpret_cast<const int4*>(
          lab_s + wi * 128 + ti * 16 + g * 4);
      lab4[0] = l4.x, lab4[1] = l4.y, lab4[2] = l4.z, lab4[3] = l4.w;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mi = m0 + wi * 128 + ti * 16 + g * 4 + r;
      float mx = -INFINITY, sx = 0.f;
      int ix = INT_MAX;  // EVAL: column of mx; INT_MAX while mx is -inf
      if constexpr (EVAL) {
        // this lane holds columns nw0 + li + {0, 16, 32, 48}: the label's
        // logit is its to write iff the label is one of them (almost
        // never, so the whole wave skips the branch)
        const int rel = lab4[r] - nw0 - li;
        if ((rel & ~48) == 0) {
          float a = acc[ti][0][r] + bv[0];
          if (rel == 16) a = acc[ti][1][r] + bv[1];
          if (rel == 32) a = acc[ti][2][r] + bv[2];
          if (rel == 48) a = acc[ti][3][r] + bv[3];
          xlab[mi] = Tr::to_f32(Tr::from_f32(a));
        }
      }
      if (full) {
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {
          const int nj = nw0 + tj * 16 + li;
          const T ob = Tr::from_f32(acc[ti][tj][r] + bv[tj]);
          if constexpr (!EVAL)
            logits[static_cast<int64_t>(mi) * V + nj] = ob;
          const float f = Tr::to_f32(ob);
          if constexpr (EVAL) {
            if (f > mx) ix = nj;  // strict: the lane's lowest column stays
          }
          if (f > mx) {
            sx *= __expf(mx - f);
            mx = f;
          }
          sx += __expf(f - mx);
        }
      } else {
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {
          const int nj = nw0 + tj * 16 + li;
          const T ob = Tr::from_f32(acc[ti][tj][r] + bv[tj]);
          if (cv[tj]) {
            if constexpr (!EVAL)
              logits[static_cast<int64_t>(mi) * V + nj] = ob;
            const float f = Tr::to_f32(ob);
            if constexpr (EVAL) {
              if (f > mx) ix = nj;
            }
            if (f > mx) {
              sx *= __expf(mx - f);
              mx = f;
            }
            sx += __expf(f - mx);
          }
        }
      }
      const float mx_own = mx;
      // butterfly over the 16-lane li-group: every lane gets the row's
      // (max, sumexp) over this wave's 64-col stripe
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        const float m2 = __shfl_xor(mx, off, 64);
        const float s2 = __shfl_xor(sx, off, 64);
        const float mn = fmaxf(mx, m2);
        sx = (sx == 0.f ? 0.f : sx * __expf(mx - mn)) +
             (s2 == 0.f ? 0.f : s2 * __expf(m2 - mn));
        mx = mn;
      }
      if constexpr (EVAL) {
        // the lanes that hold the stripe maximum offer their (lowest)
        // column; the lowest offer is the stripe's arg-max
        ix = mh::row16_min(mx_own == mx ? ix : INT_MAX);
      }
      if (li == 0) {
        float* p = part + (static_cast<int64_t>(mi) * nStripes + stripe) *
                              (EVAL ? 3 : 2);
        p[0] = mx;
        p[1] = sx;
        if constexpr (EVAL) p[2] = __int_as_float(ix);
      }
    }
  }
}

// fold per-row partials -> lse, loss: one wave per row (4 rows per
// block), coalesced 8-B lane reads over the stripe partials. EVAL also
// folds the arg-max column (lowest index on a tie), takes the label's
// logit from xlab instead of the logits, and writes pred[row] and a
// third row_out plane, the per-row "correct" flag.
template <typename T, bool EVAL>
__global__ void mlm_fold_kernel(const float* __restrict__ part,
                                const T* __restrict__ logits,
                                const int64_t* __restrict__ labels,
                                float* __restrict__ row_out,  // [2|3, rows]
                                float* __restrict__ lse_out, int rows,
                                int nStripes, int V, int64_t ignore_index,
                                // EVAL only
                                const float* __restrict__ xlab,
                                int* __restrict__ pred) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  constexpr int W = EVAL ? 3 : 2;  // words per partial
  const float* pr = part + static_cast<int64_t>(row) * nStripes * W;
  float m = -INFINITY, s = 0.f;
  int ix = INT_MAX;
  for (int t = lane; t < nStripes; t += 64) {
    const float m2 = pr[t * W], s2 = pr[t * W + 1];
    const float mn = fmaxf(m, m2);
    if constexpr (EVAL)
      ix = mh::argmax_merge(m, ix, m2, __float_as_int(pr[t * W + 2]));
    s = (s == 0.f ? 0.f : s * __expf(m - mn)) +
        (s2 == 0.f ? 0.f : s2 * __expf(m2 - mn));
    m = mn;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float m2 = __shfl_xor(m, off, 64);
    const float s2 = __shfl_xor(s, off, 64);
    const float mn = fmaxf(m, m2);
    if constexpr (EVAL)
      ix = mh::argmax_merge(m, ix, m2, __shfl_xor(ix, off, 64));
    s = (s == 0.f ? 0.f : s * __expf(m - mn)) +
        (s2 == 0.f ? 0.f : s2 * __expf(m2 - mn));
    m = mn;
  }
  if (lane == 0) {
    const float lse = m + __logf(s);
    lse_out[row] = lse;
    const int64_t label = labels[row];
    // per-row (loss, valid) instead of same-address atomics (2 x rows
    // serialized L2 atomics); mlm_sum_kernel folds them
    const bool valid = label != ignore_index;
    float xl;
    if constexpr (EVAL) {
      // no lane wrote xlab for a label outside [0, V)
      xl = (valid && label >= 0 && label < V) ? xlab[row] : 0.f;
      pred[row] = ix == INT_MAX ? 0 : ix;
      row_out[2 * rows + row] = (valid && pred[row] == label) ? 1.f : 0.f;
    } else {
      xl = valid ? Mfma16<T>::to_f32(
                       logits[static_cast<int64_t>(row) * V +
                              (valid ? label : 0)])
                 : 0.f;
    }
    row_out[row] = valid ? lse - xl : 0.f;
    row_out[rows + row] = valid ? 1.f : 0.f;
  }
}

// fold [N, rows] planes -> sums [N]: {loss_sum, count} and, for N = 3,
// correct
template <int N>
__global__ void mlm_sum_kernel(const float* __restrict__ row_out,
                               float* __restrict__ sums, int rows) {
  float a[N] = {};
  for (int i = threadIdx.x; i < rows; i += blockDim.x) {
#pragma unroll
    for (int n = 0; n < N; ++n) a[n] += row_out[n * rows + i];
  }
  __shared__ float sh[N][256];
#pragma unroll
  for (int n = 0; n < N; ++n) sh[n][threadIdx.x] = a[n];
  __syncthreads();
  for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
    if (threadIdx.x < stride) {
#pragma unroll
      for (int n = 0; n < N; ++n)
        sh[n][threadIdx.x] += sh[n][threadIdx.x + stride];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) sums[n] = sh[n][0];
  }
}

bool mlm_head_supported(int64_t P, int64_t V, int64_t K) {
  return P % mh::kBM == 0 && K % mh::kBK == 0 && K >= 64 && V >= 2;
}

// EVAL = false: {logits, loss_sum, count, lse}; EVAL = true: {loss_sum,
// count, correct, lse, pred} and no [P,V] tensor anywhere
template <typename T, bool EVAL>
static std::vector<torch::Tensor> mlm_head_run_t(torch::Tensor h,
                                                 torch::Tensor w,
                                                 torch::Tensor bias,
                                                 torch::Tensor labels,
                                                 int64_t ignore_index) {
  const int P = h.size(0), K = h.size(1), V = w.size(0);
  TORCH_CHECK(w.size(1) == K && bias.size(0) == V,
              "mlm_head: shape mismatch");
  TORCH_CHECK(mlm_head_supported(P, V, K), "mlm_head: unsupported shape");
  auto labels_c = labels.contiguous();
  TORCH_CHECK(labels_c.size(0) == P, "mlm_head: labels/P mismatch");

  const int nStripes = (V + 63) / 64;
  constexpr int kSums = EVAL ? 3 : 2;
  auto fopts = h.options().dtype(torch::kFloat32);
  auto iopts = h.options().dtype(torch::kInt32);
  torch::Tensor logits, xlab, pred;
  if constexpr (EVAL) {
    xlab = torch::empty({P}, fopts);
    pred = torch::empty({P}, iopts);
  } else {
    logits = torch::empty({P, V}, h.options());
  }
  auto part = torch::empty({P, nStripes, EVAL ? 3 : 2}, fopts);
  auto row_out = torch::empty({kSums, P}, fopts);
  auto sums = torch::empty({kSums}, fopts);  // {loss_sum, count[, correct]}
  auto lse = torch::empty({P}, fopts);
  auto stream = at::hip::getCurrentHIPStream();

  T* logits_p = EVAL ? nullptr : reinterpret_cast<T*>(logits.data_ptr());
  float* xlab_p = EVAL ? xlab.data_ptr<float>() : nullptr;
  int* pred_p = EVAL ? pred.data_ptr<int>() : nullptr;

  const size_t lds = 2 * mh::kBufB;
  HIP_CHECK(hipFuncSetAttribute(
      reinterpret_cast<const void*>(&mlm_fwd_kernel<T, EVAL>),
      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL((mlm_fwd_kernel<T, EVAL>),
                     dim3(P / mh::kBM, (V + mh::kBN - 1) / mh::kBN),
                     dim3(512), lds, stream,
                     reinterpret_cast<const T*>(h.data_ptr()),
                     reinterpret_cast<const T*>(w.data_ptr()),
                     bias.data_ptr<float>(), logits_p,
                     part.data_ptr<float>(), P, V, K, nStripes,
                     labels_c.data_ptr<int64_t>(), xlab_p);
  hipLaunchKernelGGL((mlm_fold_kernel<T, EVAL>), dim3((P + 3) / 4),
                     dim3(256), 0, stream, part.data_ptr<float>(), logits_p,
                     labels_c.data_ptr<int64_t>(), row_out.data_ptr<float>(),
                     lse.data_ptr<float>(), P, nStripes, V, ignore_index,
                     xlab_p, pred_p);
  hipLaunchKernelGGL(mlm_sum_kernel<kSums>, dim3(1), dim3(256), 0, stream,
                     row_out.data_ptr<float>(), sums.data_ptr<float>(), P);
  if constexpr (EVAL)
    return {sums.select(0, 0), sums.select(0, 1), sums.select(0, 2), lse,
            pred};
  else
    return {logits, sums.select(0, 0), sums.select(0, 1), lse};
}

static void mlm_head_check(const char* name, const torch::Tensor& h,
                           const torch::Tensor& w,
                           const torch::Tensor& bias) {
  const auto dt = h.scalar_type();
  TORCH_CHECK(h.is_cuda() && h.dim() == 2 && h.is_contiguous() &&
                  (dt == torch::kBFloat16 || dt == torch::kHalf),
              name, ": h must be contiguous 2D bf16 or fp16");
  TORCH_CHECK(w.is_cuda() && w.dim() == 2 && w.is_contiguous(), name,
              ": w must be contiguous 2D");
  TORCH_CHECK(w.scalar_type() == dt, name, ": w dtype ", w.scalar_type(),
              " does not match h dtype ", dt);
  TORCH_CHECK(bias.is_cuda() && bias.dim() == 1 &&
                  bias.scalar_type() == torch::kFloat32,
              name, ": bias must be 1D fp32");
}

// h [P,K] and w [V,K] both bf16 or both fp16, bias [V] fp32, labels [P]
// int64 -> {logits [P,V] in the input dtype, loss_sum f32, count f32,
// lse [P] f32}
std::vector<torch::Tensor> mlm_head_fwd(torch::Tensor h, torch::Tensor w,
                                        torch::Tensor bias,
                                        torch::Tensor labels,
                                        int64_t ignore_index) {
  mlm_head_check("mlm_head_fwd", h, w, bias);
  if (h.scalar_type() == torch::kHalf)
    return mlm_head_run_t<_Float16, false>(h, w, bias, labels, ignore_index);
  return mlm_head_run_t<__bf16, false>(h, w, bias, labels, ignore_index);
}

// same inputs -> {loss_sum f32, count f32, correct f32, lse [P] f32,
// pred [P] i32}: the logits-free evaluation instantiation. Labels are
// ignore_index or in [0, V).
std::vector<torch::Tensor> mlm_head_eval(torch::Tensor h, torch::Tensor w,
                                         torch::Tensor bias,
                                         torch::Tensor labels,
                                         int64_t ignore_index) {
  mlm_head_check("mlm_head_eval", h, w, bias);
  if (h.scalar_type() == torch::kHalf)
    return mlm_head_run_t<_Float16, true>(h, w, bias, labels, ignore_index);
  return mlm_head_run_t<__bf16, true>(h, w, bias, labels, ignore_index);
}

}  // namespace bpa
