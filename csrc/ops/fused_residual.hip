// Fused bias + dropout + residual-add + LayerNorm for MI355X (gfx950).
//
// One kernel for the residual junction the reference runs as 4 ops
// (BertSelfOutput/BertOutput: src/modeling.py:432-443, 468-479):
//   z = dropout(x + bias) + residual ; y = LN(z) * gamma + beta
// Dropout uses Philox4x32-10 (seed, offset) keyed by element index, and
// stores the keep-mask as bytes so backward is exact.
//
// Memory-bound design (same as layernorm.hip, row cores in rowwise.h):
// * forward: one BLOCK per row; x/residual loaded once into registers,
//   z kept in registers through the mean/var block reduction, y written
//   from registers — no re-read of z after the reduction.
// * backward: one pass (ln_bwd_rows_kernel, rowwise.h, shared with
//   ln_bwd). A block owns a group of consecutive rows; dz_res and dx are
//   written from registers and dgamma/dbeta/dbias are accumulated in the
//   same registers across the block's rows; the [nblocks, 3H] partials
//   are folded by col_reduce_full (layernorm.hip).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../checks.h"
#include "../ops.h"
#include "rowwise.h"

namespace bpa {

template <typename T, int VEC, int ITEMS, bool HAS_BIAS, bool TRAIN_DROP>
__global__ void bdrl_fwd_kernel(
    const T* __restrict__ x, const float* __restrict__ bias,
    const T* __restrict__ residual, const float* __restrict__ gamma,
    const float* __restrict__ beta, T* __restrict__ y, T* __restrict__ z,
    uint8_t* __restrict__ mask, float* __restrict__ mean,
    float* __restrict__ rstd, int rows, int H, float p, float eps,
    uint64_t seed, uint64_t offset) {
  __shared__ float red[16], red2[16];
  const int row = blockIdx.x;
  if (row >= rows) return;
  const int64_t base = static_cast<int64_t>(row) * H;
  const float keep_scale = TRAIN_DROP ? 1.0f / (1.0f - p) : 1.0f;
  Philox philox(seed);

  float zv[ITEMS][VEC];
  int cols[ITEMS];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int c = (i * blockDim.x + threadIdx.x) * VEC;
    cols[i] = c;
    if (c < H) {
      T xv[VEC], rv[VEC], zt[VEC];
      load_slice(x + base + c, xv);
      load_slice(residual + base + c, rv);
      uint8_t mv[VEC];
      if (TRAIN_DROP) keep_mask(philox, offset, base + c, p, mv);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float t = DTraits<T>::to_f32(xv[k]);
        if (HAS_BIAS) t += bias[c + k];
        if (TRAIN_DROP) t = mv[k] ? t * keep_scale : 0.f;
        t += DTraits<T>::to_f32(rv[k]);
        zv[i][k] = t;
        zt[k] = DTraits<T>::from_f32(t);
        sum += t;
      }
      store_slice(z + base + c, zt);
      if (TRAIN_DROP) store_mask(mask + base + c, mv);
    }
  }
  const RowStats st =
      ln_row_stats(zv, cols, sum, H, eps, red, red2, mean, rstd, row);
  ln_affine_store<T, VEC, ITEMS>(zv, cols, st, gamma, beta, y + base, H);
}

std::vector<torch::Tensor> bias_dropout_residual_ln_fwd(
    torch::Tensor x, c10::optional<torch::Tensor> bias, torch::Tensor residual,
    torch::Tensor gamma, torch::Tensor beta, double p, double eps,
    int64_t seed, int64_t offset) {
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous(), "bdrl_fwd: bad x");
  const int rows = x.size(0), H = x.size(1);
  auto res_c = residual.contiguous();
  TORCH_CHECK(res_c.scalar_type() == x.scalar_type(),
              "bdrl_fwd: residual dtype must match x");
  auto gamma_f = gamma.contiguous().to(torch::kFloat32);
  auto beta_f = beta.contiguous().to(torch::kFloat32);
  torch::Tensor bias_f;
  const bool has_bias = bias.has_value();
  if (has_bias) bias_f = bias->contiguous().to(torch::kFloat32);
  const bool train_drop = p > 0.0;

  auto y = torch::empty_like(x);
  auto z = torch::empty_like(x);
  auto fopts = x.options().dtype(torch::kFloat32);
  auto mask = train_drop
                  ? torch::empty({rows, H}, x.options().dtype(torch::kUInt8))
                  : torch::empty({0}, x.options().dtype(torch::kUInt8));
  auto mean = torch::empty({rows}, fopts);
  auto rstd = torch::empty({rows}, fopts);
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_ROW_DTYPE(x.scalar_type(), "bdrl_fwd", [&] {
    TORCH_CHECK(H % kVec == 0, "bdrl_fwd: H % ", kVec, " != 0");
    launch_by_items("bdrl_fwd", H / kVec, [&](auto items_c, int threads) {
      by_flag(has_bias, [&](auto has_bias_c) {
        by_flag(train_drop, [&](auto train_c) {
          hipLaunchKernelGGL(
              (bdrl_fwd_kernel<scalar_t, kVec, decltype(items_c)::value,
                               decltype(has_bias_c)::value,
                               decltype(train_c)::value>),
              dim3(rows), dim3(threads), 0, stream, dptr<scalar_t>(x),
              has_bias ? bias_f.data_ptr<float>() : nullptr,
              dptr<scalar_t>(res_c), gamma_f.data_ptr<float>(),
              beta_f.data_ptr<float>(), dptr<scalar_t>(y), dptr<scalar_t>(z),
              train_drop ? mask.data_ptr<uint8_t>() : nullptr,
              mean.data_ptr<float>(), rstd.data_ptr<float>(), rows, H,
              static_cast<float>(p), static_cast<float>(eps),
              static_cast<uint64_t>(seed), static_cast<uint64_t>(offset));
        });
      });
    });
  });
  return {y, z, mask, mean, rstd};
}

std::vector<torch::Tensor> bias_dropout_residual_ln_bwd(
    torch::Tensor dy, torch::Tensor z, torch::Tensor mask, torch::Tensor gamma,
    torch::Tensor mean, torch::Tensor rstd, double p, bool has_bias,
    c10::optional<torch::Tensor> dy2, c10::optional<torch::Tensor> dgamma_acc,
    c10::optional<torch::Tensor> dbeta_acc,
    c10::optional<torch::Tensor> dbias_acc) {
  check_rows_2d("bdrl_bwd", "z", z);
  check_like("bdrl_bwd", "dy", dy, "z", z);
  if (dy2.has_value()) {
    TORCH_CHECK(dy2->device() == z.device(), "bdrl_bwd: dy2 device ",
                dy2->device(), " does not match z device ", z.device());
    check_like("bdrl_bwd", "dy2", *dy2, "z", z);
  }
  const int rows = z.size(0), H = z.size(1);
  check_row_stat("bdrl_bwd", "mean", mean, rows);
  check_row_stat("bdrl_bwd", "rstd", rstd, rows);
  check_param("bdrl_bwd", "gamma", gamma, H);
  if (p > 0.0) check_drop_mask("bdrl_bwd", mask, rows, H);
  check_accum_dst("bdrl_bwd", "dgamma_acc", dgamma_acc, z, H);
  check_accum_dst("bdrl_bwd", "dbeta_acc", dbeta_acc, z, H);
  check_accum_dst("bdrl_bwd", "dbias_acc", dbias_acc, z, H);
  // a gradient with a destination is added there and comes back undefined
  const bool fused = dgamma_acc.has_value() || dbeta_acc.has_value() ||
                     dbias_acc.has_value();
  TORCH_CHECK(!fused || gamma.scalar_type() == torch::kFloat32,
              "bdrl_bwd: accumulating outputs need fp32 parameters");
  TORCH_CHECK(!dbias_acc.has_value() || has_bias,
              "bdrl_bwd: dbias_acc without a bias");
  auto gamma_f = gamma.contiguous().to(torch::kFloat32);
  auto dx = torch::empty_like(z);
  auto dz_res = torch::empty_like(z);
  auto fopts = z.options().dtype(torch::kFloat32);
  auto stream = at::hip::getCurrentHIPStream();
  torch::Tensor part;
  DISPATCH_ROW_DTYPE(z.scalar_type(), "bdrl_bwd", [&] {
    TORCH_CHECK(H % kVec == 0, "bdrl_bwd: H % ", kVec, " != 0");
    part = ln_bwd_rows<scalar_t, kVec, true>(
        "bdrl_bwd", dy, dy2.has_value() ? *dy2 : torch::Tensor(), z, mask,
        gamma_f, mean, rstd, dx, dz_res, p, has_bias, stream);
  });
  torch::Tensor out;
  if (fused) {
    // the partials are [nblocks, 3H] with a bias and [nblocks, 2H] without
    std::vector<c10::optional<torch::Tensor>> dsts = {dgamma_acc, dbeta_acc};
    if (has_bias) dsts.push_back(dbias_acc);
    out = col_reduce_full(part, dsts);
  } else {
    out = col_reduce_full(part);
  }
  auto dgamma = dgamma_acc.has_value() ? torch::Tensor() : out.narrow(0, 0, H);
  auto dbeta = dbeta_acc.has_value() ? torch::Tensor() : out.narrow(0, H, H);
  auto dbias = !has_bias              ? torch::empty({0}, fopts)
               : dbias_acc.has_value() ? torch::Tensor()
                                       : out.narrow(0, 2 * H, H);
  if (gamma.scalar_type() != torch::kFloat32) {
    dgamma = dgamma.to(gamma.scalar_type());
    dbeta = dbeta.to(gamma.scalar_type());
    if (has_bias) dbias = dbias.to(gamma.scalar_type());
  }
  return {dx, dbias, dz_res, dgamma, dbeta};
}

}  // namespace bpa
