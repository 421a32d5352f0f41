// Row pack / unpack for the padding-free encoder (MI355X, gfx950).
//
// The unpadded mode (ops/varlen.py, models/bert.py) runs the encoder on
// the valid tokens of a batch only: pack_rows moves row i of the padded
// [B*S, H] activation to row dest[i] of a packed [T_pad, H] matrix and
// unpack_rows moves it back. dest[i] < 0 marks a padded position, which
// pack drops and unpack fills with zeros; rows of the packed matrix that
// no dest names (the [T, T_pad) tail) are zero. dest is injective on
// the kept rows, so every output element has exactly one writer: no
// atomics, and results are bitwise repeatable. Each kernel is the
// other's backward.
//
// Both are pure row copies, memory-bound: one 16-byte chunk per lane
// (the kernels see rows as uint4 chunks, so bf16, fp16 and fp32 share
// one instantiation), flat 1-D grid over all chunks, not capped. The
// lanes of a row touch contiguous bytes on both sides; only the row
// index is indirect.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../common.h"
#include "../ops.h"

namespace bpa {

// y[dest[i]] = x[i] for dest[i] in [0, t_pad); y starts zeroed.
__global__ void pack_rows_kernel(const uint4* __restrict__ x,
                                 const int* __restrict__ dest,
                                 uint4* __restrict__ y, int64_t chunks,
                                 int chunks_per_row, int t_pad) {
  const int64_t idx =
      static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= chunks) return;
  const int64_t row = idx / chunks_per_row;
  const int c = static_cast<int>(idx - row * chunks_per_row);
  const int d = dest[row];
  if (d < 0 || d >= t_pad) return;
  y[static_cast<int64_t>(d) * chunks_per_row + c] = x[idx];
}

// x[i] = y[dest[i]] for dest[i] in [0, t_pad), zero otherwise.
__global__ void unpack_rows_kernel(const uint4* __restrict__ y,
                                   const int* __restrict__ dest,
                                   uint4* __restrict__ x, int64_t chunks,
                                   int chunks_per_row, int t_pad) {
  const int64_t idx =
      static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= chunks) return;
  const int64_t row = idx / chunks_per_row;
  const int c = static_cast<int>(idx - row * chunks_per_row);
  const int d = dest[row];
  uint4 v{0, 0, 0, 0};
  if (d >= 0 && d < t_pad) v = y[static_cast<int64_t>(d) * chunks_per_row + c];
  x[idx] = v;
}

// chunks per row, after checking everything both entry points share
static int check_rows_args(const torch::Tensor& m, const torch::Tensor& dest,
                           int64_t padded_rows, const char* who) {
  TORCH_CHECK(m.is_cuda() && m.dim() == 2 && m.is_contiguous(), who,
              ": expected a contiguous 2-D device matrix");
  const auto dt = m.scalar_type();
  TORCH_CHECK(dt == torch::kBFloat16 || dt == torch::kHalf ||
                  dt == torch::kFloat32,
              who, ": dtype must be bf16, fp16 or fp32, got ", dt);
  TORCH_CHECK(dest.dim() == 1 && dest.scalar_type() == torch::kInt32 &&
                  dest.is_contiguous() && dest.device() == m.device(),
              who, ": dest must be a contiguous int32 vector on the same "
                   "device");
  TORCH_CHECK(dest.size(0) == padded_rows, who, ": dest has ", dest.size(0),
              " entries for ", padded_rows, " padded rows");
  const int64_t row_bytes = m.size(1) * m.element_size();
  TORCH_CHECK(row_bytes > 0 && row_bytes % 16 == 0, who,
              ": row size must be a multiple of 16 bytes, got ", row_bytes);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(m.data_ptr()) % 16 == 0, who,
              ": matrix is not 16-byte aligned");
  TORCH_CHECK(m.size(0) < (int64_t{1} << 31), who, ": too many rows");
  return static_cast<int>(row_bytes / 16);
}

// x [B*S, H], dest [B*S] int32 -> [T_pad, H]
torch::Tensor pack_rows(torch::Tensor x, torch::Tensor dest, int64_t t_pad) {
  const int cpr = check_rows_args(x, dest, x.size(0), "pack_rows");
  TORCH_CHECK(t_pad >= 0 && t_pad < (int64_t{1} << 31),
              "pack_rows: bad T_pad ", t_pad);
  auto y = torch::zeros({t_pad, x.size(1)}, x.options());
  const int64_t chunks = x.size(0) * cpr;
  if (chunks == 0 || t_pad == 0) return y;
  const int64_t blocks = (chunks + 255) / 256;
  TORCH_CHECK(blocks < (int64_t{1} << 31), "pack_rows: input too large");
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(pack_rows_kernel, dim3(static_cast<uint32_t>(blocks)),
                     dim3(256), 0, stream,
                     reinterpret_cast<const uint4*>(x.data_ptr()),
                     dest.data_ptr<int>(),
                     reinterpret_cast<uint4*>(y.data_ptr()), chunks, cpr,
                     static_cast<int>(t_pad));
  return y;
}

// y [T_pad, H], dest [B*S] int32 -> [B*S, H]
torch::Tensor unpack_rows(torch::Tensor y, torch::Tensor dest,
                          int64_t padded_rows) {
  const int cpr = check_rows_args(y, dest, padded_rows, "unpack_rows");
  auto x = torch::empty({padded_rows, y.size(1)}, y.options());
  const int64_t chunks = padded_rows * cpr;
  if (chunks == 0) return x;
  const int64_t blocks = (chunks + 255) / 256;
  TORCH_CHECK(blocks < (int64_t{1} << 31), "unpack_rows: output too large");
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(unpack_rows_kernel, dim3(static_cast<uint32_t>(blocks)),
                     dim3(256), 0, stream,
                     reinterpret_cast<const uint4*>(y.data_ptr()),
                     dest.data_ptr<int>(),
                     reinterpret_cast<uint4*>(x.data_ptr()), chunks, cpr,
                     static_cast<int>(y.size(0)));
  return x;
}

}  // namespace bpa
