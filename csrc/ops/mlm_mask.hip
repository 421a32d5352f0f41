// Dynamic MLM masking on the device: raw shard rows in, model inputs and the
// padded-gather MLM positions out, in one launch.
//
// The mask of a row is a pure function of (seed, epoch, sample index,
// position): every candidate position j draws Philox4x32-10 words at the
// counter (j, epoch, lo32(index), hi32(index) | 2^31) under the key `seed`,
// the n candidates with the smallest (w0 << 32 | j) are selected, and w1 / w2
// decide keep / random token / mask token. docs/KERNELS.md has the full
// definition; tests/test_gpu_mlm_mask.py holds a numpy twin the kernel is
// bit-equal to.
//
// One workgroup per row. A row's first output slot is the number of masked
// tokens in the rows before it, which every block recomputes from the
// `special` entries of those rows (three integers and a table lookup per
// row), so there is no communication between workgroups and no atomic. The
// last block also fills the unused tail of the slot budget. Nothing is read
// back to the host.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../common.h"
#include "../ops.h"

namespace bpa {

namespace {

constexpr int kMaskMaxS = 1024;
constexpr int kMaskThreads = 256;

// Masked tokens of a row, from its specials alone. Candidates are the
// positions below `last` = clamp(s[2], 0, S-1) that no special names; s[2]
// itself is never below `last`, and a special below `last` is inside the
// row, so any content of `s` is safe. The result is clamped to
// [0, min(max_pred, candidates)] whatever the table holds.
__device__ __forceinline__ int row_mask_count(const int32_t* __restrict__ s,
                                              const int32_t* __restrict__ table,
                                              int S, int max_pred) {
  const int s0 = s[0], s1 = s[1], s2 = s[2];
  const int last = min(max(s2, 0), S - 1);
  int c = last;
  if (s0 >= 0 && s0 < last) --c;
  if (s1 >= 0 && s1 < last && s1 != s0) --c;
  return max(0, min(table[c], min(max_pred, c)));  // 0 <= c <= S-1
}

__global__ __launch_bounds__(kMaskThreads) void mlm_mask_kernel(
    const int32_t* __restrict__ ids, const int32_t* __restrict__ special,
    const int64_t* __restrict__ sample_index,
    const int32_t* __restrict__ table, int64_t* __restrict__ out_ids,
    int64_t* __restrict__ out_tt, int64_t* __restrict__ out_am,
    int64_t* __restrict__ positions, int64_t* __restrict__ gathered,
    int64_t* __restrict__ dense,  // may be null
    int B, int S, int max_pred, uint64_t seed, uint32_t epoch,
    uint32_t vocab_m1, int64_t mask_token, uint64_t t_keep,
    uint64_t t_keep_rand) {
  __shared__ uint64_t keys[kMaskMaxS];
  __shared__ uint32_t w1s[kMaskMaxS];
  __shared__ uint32_t w2s[kMaskMaxS];
  __shared__ uint8_t sel[kMaskMaxS];
  __shared__ int wave_sums[kMaskThreads / WAVE_SIZE];

  const int b = blockIdx.x;
  const int tid = threadIdx.x;

  // first output slot of this row
  int part = 0;
  for (int r = tid; r < b; r += kMaskThreads)
    part += row_mask_count(special + 3 * r, table, S, max_pred);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, WAVE_SIZE);
  if ((tid & (WAVE_SIZE - 1)) == 0) wave_sums[tid / WAVE_SIZE] = part;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int w = 0; w < kMaskThreads / WAVE_SIZE; ++w) base += wave_sums[w];

  const int32_t* sp = special + 3 * b;
  const int s0 = sp[0], s1 = sp[1], s2 = sp[2];
  const int last = min(max(s2, 0), S - 1);
  const int n = row_mask_count(sp, table, S, max_pred);

  const uint64_t index = static_cast<uint64_t>(sample_index[b]);
  const uint32_t c2 = static_cast<uint32_t>(index);
  const uint32_t c3 =
      (static_cast<uint32_t>(index >> 32) & 0x7FFFFFFFu) | 0x80000000u;
  const Philox philox(seed);

  // 1. draw: candidates get their sort key, everything else the maximum
  for (int j = tid; j < S; j += kMaskThreads) {
    const bool cand = j < last && j != s0 && j != s1;
    uint64_t key = ~uint64_t{0};
    if (cand) {
      uint32_t w[4];
      philox.words(static_cast<uint32_t>(j), epoch, c2, c3, w);
      key = (static_cast<uint64_t>(w[0]) << 32) | static_cast<uint32_t>(j);
      w1s[j] = w[1];
      w2s[j] = w[2];
    }
    keys[j] = key;
  }
  __syncthreads();

  // 2. select: a candidate's rank is the number of smaller keys (keys are
  // distinct: the position is their low word)
  for (int j = tid; j < S; j += kMaskThreads) {
    const uint64_t key = keys[j];
    bool chosen = false;
    if (key != ~uint64_t{0} && n > 0) {
      int rank = 0;
      for (int i = 0; i < S; ++i) rank += keys[i] < key ? 1 : 0;
      chosen = rank < n;
    }
    sel[j] = chosen ? 1 : 0;
  }
  __syncthreads();

  // 3. write the row; a selected position also takes its slot, in
  // ascending position order
  const int64_t row = static_cast<int64_t>(b) * S;
  for (int j = tid; j < S; j += kMaskThreads) {
    int64_t id = ids[row + j];
    int64_t label = -1;
    if (sel[j]) {
      label = id;
      const uint64_t w1 = w1s[j];
      if (w1 < t_keep) {
        // keep the original token
      } else if (w1 < t_keep_rand) {
        id = static_cast<int64_t>(
            (static_cast<uint64_t>(w2s[j]) * vocab_m1) >> 32);
      } else {
        id = mask_token;
      }
      int before = 0;
      for (int i = 0; i < j; ++i) before += sel[i];
      const int slot = base + before;  // < base + n <= B * max_pred
      positions[slot] = row + j;
      gathered[slot] = label;
    }
    out_ids[row + j] = id;
    out_tt[row + j] = (j > s1 && j <= s2) ? 1 : 0;
    out_am[row + j] = j <= last ? 1 : 0;
    if (dense != nullptr) dense[row + j] = label;
  }

  // 4. the slots no row used
  if (b == B - 1) {
    const int cap = B * max_pred;
    for (int s = base + n + tid; s < cap; s += kMaskThreads) {
      positions[s] = 0;
      gathered[s] = -1;
    }
  }
}

}  // namespace

std::vector<torch::Tensor> mlm_mask(torch::Tensor input_ids,
                                    torch::Tensor special,
                                    torch::Tensor sample_index,
                                    torch::Tensor count_table, int64_t seed,
                                    int64_t epoch, int64_t max_pred,
                                    int64_t vocab_size, int64_t mask_token,
                                    int64_t t_keep, int64_t t_rand,
                                    bool dense_labels) {
  TORCH_CHECK(input_ids.is_cuda() && input_ids.dim() == 2 &&
                  input_ids.scalar_type() == torch::kInt32,
              "mlm_mask: input_ids must be a 2D int32 GPU tensor, got ",
              input_ids.scalar_type(), " ", input_ids.sizes());
  TORCH_CHECK(input_ids.is_contiguous(),
              "mlm_mask: input_ids must be contiguous");
  const int64_t B = input_ids.size(0), S = input_ids.size(1);
  TORCH_CHECK(S >= 1 && S <= kMaskMaxS, "mlm_mask: sequence length ", S,
              " must be in [1, 1024]");
  TORCH_CHECK(max_pred >= 1 && max_pred <= S, "mlm_mask: max_pred ", max_pred,
              " must be in [1, S = ", S, "]");
  TORCH_CHECK(special.device() == input_ids.device() &&
                  special.scalar_type() == torch::kInt32 &&
                  special.dim() == 2 && special.size(0) == B &&
                  special.size(1) == 3 && special.is_contiguous(),
              "mlm_mask: special must be contiguous int32 [", B,
              ", 3] on the device of input_ids, got ", special.scalar_type(),
              " ", special.sizes());
  TORCH_CHECK(sample_index.device() == input_ids.device() &&
                  sample_index.scalar_type() == torch::kInt64 &&
                  sample_index.dim() == 1 && sample_index.size(0) == B &&
                  sample_index.is_contiguous(),
              "mlm_mask: sample_index must be contiguous int64 [", B,
              "] on the device of input_ids, got ",
              sample_index.scalar_type(), " ", sample_index.sizes());
  TORCH_CHECK(count_table.device() == input_ids.device() &&
                  count_table.scalar_type() == torch::kInt32 &&
                  count_table.dim() == 1 && count_table.size(0) == S + 1 &&
                  count_table.is_contiguous(),
              "mlm_mask: count_table must be contiguous int32 [", S + 1,
              "] on the device of input_ids, got ", count_table.scalar_type(),
              " ", count_table.sizes());
  TORCH_CHECK(vocab_size >= 2 && vocab_size <= (int64_t{1} << 31),
              "mlm_mask: bad vocab_size ", vocab_size);
  TORCH_CHECK(mask_token >= 0 && mask_token < (int64_t{1} << 31),
              "mlm_mask: bad mask_token ", mask_token);
  constexpr int64_t kTwo32 = int64_t{1} << 32;
  TORCH_CHECK(t_keep >= 0 && t_rand >= 0 && t_keep <= kTwo32 &&
                  t_rand <= kTwo32 && t_keep + t_rand <= kTwo32,
              "mlm_mask: thresholds ", t_keep, " + ", t_rand,
              " must lie in [0, 2^32]");
  TORCH_CHECK(B * S < (int64_t{1} << 31), "mlm_mask: batch too large");

  auto opts = input_ids.options().dtype(torch::kInt64);
  auto out_ids = torch::empty({B, S}, opts);
  auto out_tt = torch::empty({B, S}, opts);
  auto out_am = torch::empty({B, S}, opts);
  auto positions = torch::empty({B * max_pred}, opts);
  auto gathered = torch::empty({B * max_pred}, opts);
  std::vector<torch::Tensor> out = {out_ids, out_tt, out_am, positions,
                                    gathered};
  torch::Tensor dense;
  if (dense_labels) {
    dense = torch::empty({B, S}, opts);
    out.push_back(dense);
  }
  if (B == 0) return out;

  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(
      mlm_mask_kernel, dim3(static_cast<uint32_t>(B)), dim3(kMaskThreads), 0,
      stream, input_ids.data_ptr<int32_t>(), special.data_ptr<int32_t>(),
      sample_index.data_ptr<int64_t>(), count_table.data_ptr<int32_t>(),
      out_ids.data_ptr<int64_t>(), out_tt.data_ptr<int64_t>(),
      out_am.data_ptr<int64_t>(), positions.data_ptr<int64_t>(),
      gathered.data_ptr<int64_t>(),
      dense_labels ? dense.data_ptr<int64_t>() : nullptr, static_cast<int>(B),
      static_cast<int>(S), static_cast<int>(max_pred),
      static_cast<uint64_t>(seed), static_cast<uint32_t>(epoch),
      static_cast<uint32_t>(vocab_size - 1), mask_token,
      static_cast<uint64_t>(t_keep), static_cast<uint64_t>(t_keep + t_rand));
  HIP_CHECK(hipGetLastError());
  return out;
}

}  // namespace bpa
