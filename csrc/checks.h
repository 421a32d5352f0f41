// Host-side operand checks shared by the row-wise and attention backward
// entry points. The kernels reinterpret every operand as the dtype of
// the saved activation and index it by that tensor's shape, so a
// mismatch reads or writes out of bounds; these run before any launch.
#pragma once

#include <torch/extension.h>

namespace bpa {

// `t` must have the dtype and shape of `like` and be contiguous.
inline void check_like(const char* op, const char* name,
                       const torch::Tensor& t, const char* like_name,
                       const torch::Tensor& like) {
  TORCH_CHECK(t.scalar_type() == like.scalar_type(), op, ": ", name,
              " dtype ", t.scalar_type(), " does not match ", like_name,
              " dtype ", like.scalar_type());
  TORCH_CHECK(t.sizes() == like.sizes(), op, ": ", name, " shape ",
              t.sizes(), " does not match ", like_name, " shape ",
              like.sizes());
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
}

// 2D contiguous activation the kernels index as [rows, H]
inline void check_rows_2d(const char* op, const char* name,
                          const torch::Tensor& t) {
  TORCH_CHECK(t.dim() == 2 && t.is_contiguous(), op, ": ", name,
              " must be 2D contiguous");
}

// per-row fp32 statistic (mean, rstd, lse)
inline void check_row_stat(const char* op, const char* name,
                           const torch::Tensor& t, int64_t rows) {
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, op, ": ", name,
              " dtype ", t.scalar_type(), " must be ", torch::kFloat32);
  TORCH_CHECK(t.numel() == rows && t.is_contiguous(), op, ": ", name,
              " must be contiguous with ", rows, " elements, got ",
              t.sizes());
}

// byte keep-mask of a [rows, H] activation
inline void check_drop_mask(const char* op, const torch::Tensor& mask,
                            int64_t rows, int64_t H) {
  TORCH_CHECK(mask.scalar_type() == torch::kUInt8, op,
              ": mask dtype ", mask.scalar_type(), " must be ", torch::kUInt8);
  TORCH_CHECK(mask.dim() == 2 && mask.size(0) == rows && mask.size(1) == H &&
                  mask.is_contiguous(),
              op, ": mask must be contiguous [", rows, ", ", H, "], got ",
              mask.sizes());
}

// bit-packed attention keep-mask: one bit per score of `heads` [S, S]
// score matrices, as int32 words, every row padded to whole words
inline void check_bit_mask(const char* op, const torch::Tensor& mask,
                           int64_t heads, int64_t S) {
  TORCH_CHECK(mask.scalar_type() == torch::kInt32, op,
              ": keep-mask dtype ", mask.scalar_type(), " must be ",
              torch::kInt32);
  const int64_t Sw = (S + 31) / 32;
  TORCH_CHECK(mask.numel() == heads * S * Sw && mask.is_contiguous(), op,
              ": keep-mask must be contiguous [", heads, ", ", S, ", ", Sw,
              "], got ", mask.sizes());
}

// fp32 per-column parameter of length H (after the entry point's cast)
inline void check_param(const char* op, const char* name,
                        const torch::Tensor& t, int64_t H) {
  TORCH_CHECK(t.numel() == H, op, ": ", name, " must have ", H,
              " elements, got ", t.sizes());
}

// fp32 gradient buffer of length H that a backward entry point adds its
// column sums into; `like` is a tensor of the launch (device)
inline void check_accum_dst(const char* op, const char* name,
                            const torch::Tensor& t, const torch::Tensor& like,
                            int64_t H) {
  TORCH_CHECK(t.device() == like.device(), op, ": ", name, " device ",
              t.device(), " does not match ", like.device());
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, op, ": ", name, " dtype ",
              t.scalar_type(), " must be ", torch::kFloat32);
  TORCH_CHECK(t.dim() == 1 && t.numel() == H && t.is_contiguous(), op, ": ",
              name, " must be contiguous [", H, "], got ", t.sizes());
}

inline void check_accum_dst(const char* op, const char* name,
                            const c10::optional<torch::Tensor>& t,
                            const torch::Tensor& like, int64_t H) {
  if (t.has_value()) check_accum_dst(op, name, *t, like, H);
}

}  // namespace bpa
