// Dynamic MLM masking on the device: raw shard rows in, model inputs and the
// padded-gather MLM positions out. Nothing is read back to the host, there is
// no atomic and no waiting between workgroups.
//
// The mask of a row is a pure function of (seed, epoch, sample index,
// position): every candidate position j draws Philox4x32-10 words at the
// counter (j, epoch, lo32(index), hi32(index) | 2^31) under the key `seed`,
// the n candidates with the smallest (w0 << 32 | j) are selected, and w1 / w2
// decide keep / random token / mask token. docs/KERNELS.md has the full
// definition; tests/mlm_mask_spec.py and tests/mlm_span_spec.py hold the
// numpy and plain-Python twins the kernel is bit-equal to.
//
// One row kernel, mlm_mask_row_kernel<MODE>: one workgroup of 256
// threads per row. Position j belongs to thread j % 256 in every phase, so
// what a position draws stays in that thread's registers, and a wave's
// ballot is the 64-bit word j / 64 of a row-wide bit mask in LDS. Header,
// draw, the count-smaller rank, the selected bits, the substitution, the
// [B,S] stores and a selected position's index among the row's selected
// (popcounts over the bit mask) are the same code for every instantiation.
// The template switch changes two things:
//
//   * which candidates are selected. Token-level: the ones of rank < n.
//     Whole words: a uint8 [vocab_size] table of continuation pieces groups
//     the candidates into words, the words are ordered by the key of their
//     first position and fill the budget greedily, whole words only.
//     Spans: the same words in the same order, but a word that is taken
//     grows over the words that follow it, up to a length drawn from w3 and
//     a host-built table, and the whole span shares the anchor's keep /
//     random / mask decision.
//   * where a row's masked tokens go. Token-level: a row's count is a
//     function of its specials, so every block recomputes its first slot
//     from the `special` entries of the rows before it (three integers and a
//     table lookup per row) and stores to `positions` / `gathered` directly;
//     the last block fills the unused tail of the slot budget. One launch.
//     Whole words and spans: the count is known only after the selection,
//     so the row kernel writes the row's count and a compact list, and
//     mlm_mask_scatter_kernel, a second launch on the same stream, sums the
//     counts of the rows before its own, moves the lists to their slots and
//     fills the tail.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../common.h"
#include "../ops.h"

namespace bpa {

namespace {

constexpr int kMaskMaxS = 1024;
constexpr int kMaskThreads = 256;
constexpr int kMaskPerThread = kMaskMaxS / kMaskThreads;  // 4
constexpr int kMaskWords = kMaskMaxS / WAVE_SIZE;         // 16

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

// Sum of count(r) over the rows r < rows, on every thread of the block
// (strided over the block, wave shuffle + LDS sum). Holds one barrier.
template <typename F>
__device__ __forceinline__ int block_sum_before(int rows, F count) {
  __shared__ int wave_sums[kMaskThreads / WAVE_SIZE];
  const int tid = threadIdx.x;
  int part = 0;
  for (int r = tid; r < rows; r += kMaskThreads) part += count(r);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, WAVE_SIZE);
  if ((tid & (WAVE_SIZE - 1)) == 0) wave_sums[tid / WAVE_SIZE] = part;
  __syncthreads();
  int sum = 0;
#pragma unroll
  for (int w = 0; w < kMaskThreads / WAVE_SIZE; ++w) sum += wave_sums[w];
  return sum;
}

// the slots no row used: [first, cap)
__device__ __forceinline__ void fill_unused_slots(
    int64_t* __restrict__ positions, int64_t* __restrict__ gathered, int first,
    int cap) {
  for (int s = first + threadIdx.x; s < cap; s += kMaskThreads) {
    positions[s] = 0;
    gathered[s] = -1;
  }
}

// A key's rank is the number of smaller keys (keys are distinct: the
// position is their low word).
__device__ __forceinline__ int count_smaller(const uint64_t* keys, int S,
                                             uint64_t key) {
  int rank = 0;
  for (int i = 0; i < S; ++i) rank += keys[i] < key ? 1 : 0;
  return rank;
}

// first set bit above position j, kMaskMaxS if there is none
__device__ __forceinline__ int next_set_after(const uint64_t* bits, int j) {
  int w = j >> 6;
  uint64_t m = bits[w] & ~((uint64_t{2} << (j & 63)) - 1);
  while (m == 0 && ++w < kMaskWords) m = bits[w];
  return m != 0 ? (w << 6) + __builtin_ctzll(m) : kMaskMaxS;
}

// last set bit at or below position j, -1 if there is none
__device__ __forceinline__ int last_set_upto(const uint64_t* bits, int j) {
  int w = j >> 6;
  uint64_t m = bits[w] & ((uint64_t{2} << (j & 63)) - 1);
  while (m == 0 && --w >= 0) m = bits[w];
  return m != 0 ? (w << 6) + 63 - __builtin_clzll(m) : -1;
}

enum class MaskMode { kToken, kWholeWord, kSpan };

// decision of a span, the byte its words carry in word_sel
constexpr uint32_t kSpanKeep = 1, kSpanRandom = 2, kSpanMask = 3;

// Whole words and spans read word_continues and write row_count / row_pos /
// row_label; token-level reads `special` of the rows before and writes
// positions / gathered. Only spans read span_table (span_max entries). The
// pointers of the other instantiations are never touched.
template <MaskMode MODE>
__global__ __launch_bounds__(kMaskThreads) void mlm_mask_row_kernel(
    const int32_t* __restrict__ ids, const int32_t* __restrict__ special,
    const int64_t* __restrict__ sample_index,
    const int32_t* __restrict__ table,
    const uint8_t* __restrict__ word_continues,
    const int64_t* __restrict__ span_table, int span_max,
    int64_t* __restrict__ out_ids, int64_t* __restrict__ out_tt,
    int64_t* __restrict__ out_am,
    int64_t* __restrict__ dense,  // may be null
    int64_t* __restrict__ positions, int64_t* __restrict__ gathered,
    int32_t* __restrict__ row_count, int32_t* __restrict__ row_pos,
    int32_t* __restrict__ row_label, int B, int S, int max_pred, uint64_t seed,
    uint32_t epoch, uint32_t vocab_size, int64_t mask_token, uint64_t t_keep,
    uint64_t t_keep_rand) {
  constexpr bool WHOLE_WORD = MODE != MaskMode::kToken;  // grouped into words
  constexpr bool SPAN = MODE == MaskMode::kSpan;
  __shared__ uint64_t keys[kMaskMaxS];
  __shared__ uint64_t sel_bits[kMaskWords];

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);

  // token-level: first output slot of this row
  int base = 0;
  if constexpr (!WHOLE_WORD) {
    base = block_sum_before(b, [&](int r) {
      return row_mask_count(special + 3 * r, table, S, max_pred);
    });
  }

  const int32_t* sp = special + 3 * b;
  const int s0 = sp[0], s1 = sp[1], s2 = sp[2];
  const int last = min(max(s2, 0), S - 1);
  const int n = row_mask_count(sp, table, S, max_pred);
  // positions at and above S are never candidates: last < S
  auto is_cand = [&](int j) { return j < last && j != s0 && j != s1; };

  const uint64_t index = static_cast<uint64_t>(sample_index[b]);
  const uint32_t c2 = static_cast<uint32_t>(index);
  const uint32_t c3 =
      (static_cast<uint32_t>(index >> 32) & 0x7FFFFFFFu) | 0x80000000u;
  const Philox philox(seed);
  const int64_t row = static_cast<int64_t>(b) * S;

  int32_t id_r[kMaskPerThread];
  uint32_t w1_r[kMaskPerThread], w2_r[kMaskPerThread];
  uint32_t w3_r[kMaskPerThread];    // spans only
  uint32_t code_r[kMaskPerThread];  // spans only: the span's decision
  bool cand_r[kMaskPerThread], sel_r[kMaskPerThread];

  // draw: candidates get their sort key, everything else the maximum
#pragma unroll
  for (int k = 0; k < kMaskPerThread; ++k) {
    const int j = k * kMaskThreads + tid;
    const bool cand = is_cand(j);
    uint64_t key = ~uint64_t{0};
    w1_r[k] = w2_r[k] = 0;
    if (cand) {
      uint32_t w[4];
      philox.words(static_cast<uint32_t>(j), epoch, c2, c3, w);
      key = (static_cast<uint64_t>(w[0]) << 32) | static_cast<uint32_t>(j);
      w1_r[k] = w[1];
      w2_r[k] = w[2];
      if constexpr (SPAN) w3_r[k] = w[3];
    }
    id_r[k] = j < S ? ids[row + j] : 0;
    cand_r[k] = cand;
    keys[j] = key;
  }

  if constexpr (WHOLE_WORD) {
    __shared__ uint32_t order[kMaskMaxS];  // first | len << 16, by rank
    __shared__ uint8_t word_sel[kMaskMaxS];
    __shared__ uint64_t start_bits[kMaskWords];
    __shared__ uint64_t break_bits[kMaskWords];
    bool start_r[kMaskPerThread];

    // word starts: a candidate that does not continue a candidate (an id
    // outside the table continues nothing). A break is a start or a
    // non-candidate; only starts keep their key.
#pragma unroll
    for (int k = 0; k < kMaskPerThread; ++k) {
      const int j = k * kMaskThreads + tid;
      const bool continues = cand_r[k] &&
                             static_cast<uint32_t>(id_r[k]) < vocab_size &&
                             word_continues[id_r[k]] == 1;
      const bool start = cand_r[k] && !(continues && j > 0 && is_cand(j - 1));
      if (cand_r[k] && !start) keys[j] = ~uint64_t{0};
      start_r[k] = start;
      word_sel[j] = 0;
      const uint64_t cmask = __ballot(cand_r[k]);
      const uint64_t smask = __ballot(start);
      if (lane == 0) {
        start_bits[j >> 6] = smask;
        break_bits[j >> 6] = ~cmask | smask;
      }
    }
    __syncthreads();

    // a word's length is the distance to the next break (position `last`
    // is one). The words go to `order` by the rank of their key. A span
    // anchor adds its decision (bits 10-11) and the words it may still
    // append (bits 26-30): one for every table entry its w3 reaches.
#pragma unroll
    for (int k = 0; k < kMaskPerThread; ++k) {
      const int j = k * kMaskThreads + tid;
      if (start_r[k] && n > 0) {
        const int len = next_set_after(break_bits, j) - j;
        uint32_t entry =
            static_cast<uint32_t>(j) | static_cast<uint32_t>(len) << 16;
        if constexpr (SPAN) {
          const uint64_t w1 = w1_r[k], w3 = w3_r[k];
          uint32_t more = 0;
          for (int i = 0; i < span_max - 1; ++i)  // i < span_max: in the table
            more += w3 >= static_cast<uint64_t>(span_table[i]) ? 1 : 0;
          const uint32_t code = w1 < t_keep        ? kSpanKeep
                                : w1 < t_keep_rand ? kSpanRandom
                                                   : kSpanMask;
          entry |= code << 10 | more << 26;  // j, len < 1024; more < 32
        }
        order[count_smaller(keys, S, keys[j])] = entry;
      }
    }
    __syncthreads();

    // greedy fill on the first wave, 64 words of the list at a time. While
    // words are skipped the room left does not change, so the next word taken
    // is the first pending one that fits: one step per selected word.
    if (tid < WAVE_SIZE && n > 0) {
      int words = 0;
#pragma unroll
      for (int w = 0; w < kMaskWords; ++w) words += __popcll(start_bits[w]);
      int m = 0;
      for (int c = 0; c < words && m < n; c += WAVE_SIZE) {
        const bool valid = c + lane < words;
        const uint32_t entry = valid ? order[c + lane] : 0;
        if constexpr (SPAN) {
          // Taking a span selects the words it grows over, so the whole-word
          // shortcut below does not hold: after every span the pending lanes
          // test again whether their word is still free and still fits. The
          // span itself is walked by all lanes alike (every value is
          // wave-uniform, every lane stores the same bytes), so a lane reads
          // back what it stored itself and no lane waits for another.
          const int first = static_cast<int>(entry & 0x3FFu);
          const int len = static_cast<int>(entry >> 16 & 0x3FFu);
          uint64_t pending = ~uint64_t{0};
          while (true) {
            const uint64_t fits =
                __ballot(valid && len <= n - m && word_sel[first] == 0) &
                pending;
            if (fits == 0) break;
            const int pick = __builtin_ctzll(fits);
            const uint32_t anchor = static_cast<uint32_t>(
                __builtin_amdgcn_readlane(static_cast<int>(entry), pick));
            const uint8_t code = static_cast<uint8_t>(anchor >> 10 & 3u);
            const int more = static_cast<int>(anchor >> 26);
            int x = static_cast<int>(anchor & 0x3FFu);  // the span's last word
            int xlen = static_cast<int>(anchor >> 16 & 0x3FFu);
            int t = xlen;
            word_sel[x] = code;
            for (int i = 0; i < more; ++i) {
              // the word that starts where x ends, if one does: a special or
              // `last` is no start. y <= last < S; checked before it indexes.
              // The three LDS reads do not depend on each other: one round
              // trip per step, not three
              const int y = x + xlen;
              if (y >= S) break;
              const bool starts = (start_bits[y >> 6] >> (y & 63) & 1) != 0;
              const bool taken = word_sel[y] != 0;
              const int ylen = next_set_after(break_bits, y) - y;
              if (!starts || taken || m + t + ylen > n) break;
              word_sel[y] = code;
              t += ylen;
              x = y;
              xlen = ylen;
            }
            m += t;
            pending = pick == 63 ? 0 : ~uint64_t{0} << (pick + 1);
          }
          continue;
        }
        const int len = static_cast<int>(entry >> 16);
        bool take = false;
        uint64_t pending = ~uint64_t{0};
        while (true) {
          const uint64_t fits = __ballot(valid && len <= n - m) & pending;
          if (fits == 0) break;
          const int pick = __builtin_ctzll(fits);
          if (lane == pick) take = true;
          m += __builtin_amdgcn_readlane(len, pick);
          pending = pick == 63 ? 0 : ~uint64_t{0} << (pick + 1);
        }
        if (take) word_sel[entry & 0xFFFFu] = 1;
      }
    }
    __syncthreads();

    // a candidate is selected with the word it belongs to (and takes the
    // decision of the span that word is in)
#pragma unroll
    for (int k = 0; k < kMaskPerThread; ++k) {
      const int j = k * kMaskThreads + tid;
      uint8_t mark = 0;
      if (cand_r[k]) {
        const int head = last_set_upto(start_bits, j);
        if (head >= 0) mark = word_sel[head];
      }
      sel_r[k] = mark != 0;
      if constexpr (SPAN) code_r[k] = mark;
    }
  } else {
    __syncthreads();
    // the n candidates with the smallest keys
#pragma unroll
    for (int k = 0; k < kMaskPerThread; ++k) {
      const int j = k * kMaskThreads + tid;
      sel_r[k] = cand_r[k] && n > 0 && count_smaller(keys, S, keys[j]) < n;
    }
  }

#pragma unroll
  for (int k = 0; k < kMaskPerThread; ++k) {
    const int j = k * kMaskThreads + tid;
    const uint64_t mask = __ballot(sel_r[k]);
    if (lane == 0) sel_bits[j >> 6] = mask;
  }
  __syncthreads();

  // write the row; a selected position also takes its place among the row's
  // selected, in ascending position order (at most n <= max_pred of them)
#pragma unroll
  for (int k = 0; k < kMaskPerThread; ++k) {
    const int j = k * kMaskThreads + tid;
    if (j >= S) continue;
    int64_t id = id_r[k];
    int64_t label = -1;
    if (sel_r[k]) {
      label = id;
      const uint64_t w1 = w1_r[k];
      if (SPAN ? code_r[k] == kSpanKeep : w1 < t_keep) {
        // keep the original token
      } else if (SPAN ? code_r[k] == kSpanRandom : w1 < t_keep_rand) {
        id = static_cast<int64_t>(
            (static_cast<uint64_t>(w2_r[k]) * (vocab_size - 1)) >> 32);
      } else {
        id = mask_token;
      }
      int before = __popcll(sel_bits[j >> 6] & ((uint64_t{1} << (j & 63)) - 1));
      for (int w = 0; w < (j >> 6); ++w) before += __popcll(sel_bits[w]);
      if constexpr (WHOLE_WORD) {
        if (before < max_pred) {
          row_pos[b * max_pred + before] = static_cast<int32_t>(row + j);
          row_label[b * max_pred + before] = static_cast<int32_t>(label);
        }
      } else {
        const int slot = base + before;  // < base + n <= B * max_pred
        positions[slot] = row + j;
        gathered[slot] = label;
      }
    }
    out_ids[row + j] = id;
    out_tt[row + j] = (j > s1 && j <= s2) ? 1 : 0;
    out_am[row + j] = j <= last ? 1 : 0;
    if (dense != nullptr) dense[row + j] = label;
  }

  if constexpr (WHOLE_WORD) {
    if (tid == 0) {
      int total = 0;
#pragma unroll
      for (int w = 0; w < kMaskWords; ++w) total += __popcll(sel_bits[w]);
      row_count[b] = total;
    }
  } else {
    if (b == B - 1) fill_unused_slots(positions, gathered, base + n, B * max_pred);
  }
}

// Whole words, second launch: row b's first slot is the sum of the counts of
// the rows before it; its compact list moves there, and the last block fills
// the slots no row used.
__global__ __launch_bounds__(kMaskThreads) void mlm_mask_scatter_kernel(
    const int32_t* __restrict__ row_count, const int32_t* __restrict__ row_pos,
    const int32_t* __restrict__ row_label, int64_t* __restrict__ positions,
    int64_t* __restrict__ gathered, int B, int max_pred) {
  const int b = blockIdx.x;
  auto count_of = [&](int r) { return min(max(row_count[r], 0), max_pred); };
  const int base = block_sum_before(b, count_of);
  const int count = count_of(b);
  for (int i = threadIdx.x; i < count; i += kMaskThreads) {
    positions[base + i] = row_pos[b * max_pred + i];  // base + i < B * max_pred
    gathered[base + i] = row_label[b * max_pred + i];
  }
  if (b == B - 1)
    fill_unused_slots(positions, gathered, base + count, B * max_pred);
}

// Checks the arguments, allocates {masked_ids, token_type_ids,
// attention_mask, positions, gathered_labels (, dense labels)} and launches:
// whole words when `word_continues` is given, spans of whole words when
// `span_table` is given as well, token-level otherwise.
std::vector<torch::Tensor> mlm_mask_launch(
    const torch::Tensor& input_ids, const torch::Tensor& special,
    const torch::Tensor& sample_index, const torch::Tensor& count_table,
    const torch::Tensor* word_continues, const torch::Tensor* span_table,
    int64_t seed, int64_t epoch, int64_t max_pred, int64_t vocab_size,
    int64_t mask_token, int64_t t_keep, int64_t t_rand, bool dense_labels) {
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
  if (word_continues != nullptr) {
    TORCH_CHECK(word_continues->device() == input_ids.device() &&
                    word_continues->scalar_type() == torch::kUInt8 &&
                    word_continues->dim() == 1 &&
                    word_continues->size(0) == vocab_size &&
                    word_continues->is_contiguous(),
                "mlm_mask: word_continues must be contiguous uint8 [",
                vocab_size, "] on the device of input_ids, got ",
                word_continues->scalar_type(), " ", word_continues->sizes());
  }
  if (span_table != nullptr) {
    TORCH_CHECK(word_continues != nullptr,
                "mlm_mask: span_table needs word_continues");
    TORCH_CHECK(span_table->device() == input_ids.device() &&
                    span_table->scalar_type() == torch::kInt64 &&
                    span_table->dim() == 1 && span_table->size(0) >= 1 &&
                    span_table->size(0) <= 32 && span_table->is_contiguous(),
                "mlm_mask: span_table must be contiguous int64 [Lmax], 1 <= "
                "Lmax <= 32, on the device of input_ids, got ",
                span_table->scalar_type(), " ", span_table->sizes());
  }

  auto opts = input_ids.options().dtype(torch::kInt64);
  std::vector<torch::Tensor> out = {
      torch::empty({B, S}, opts), torch::empty({B, S}, opts),
      torch::empty({B, S}, opts), torch::empty({B * max_pred}, opts),
      torch::empty({B * max_pred}, opts)};
  if (dense_labels) out.push_back(torch::empty({B, S}, opts));
  if (B == 0) return out;

  // whole words, per row: its count, then max_pred positions and max_pred
  // labels
  torch::Tensor scratch;
  int32_t *row_count = nullptr, *row_pos = nullptr, *row_label = nullptr;
  if (word_continues != nullptr) {
    scratch = torch::empty({B * (2 * max_pred + 1)},
                           input_ids.options().dtype(torch::kInt32));
    row_count = scratch.data_ptr<int32_t>();
    row_pos = row_count + B;
    row_label = row_pos + B * max_pred;
  }

  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid(static_cast<uint32_t>(B)), block(kMaskThreads);
  const auto row_kernel =
      span_table != nullptr       ? mlm_mask_row_kernel<MaskMode::kSpan>
      : word_continues != nullptr ? mlm_mask_row_kernel<MaskMode::kWholeWord>
                                  : mlm_mask_row_kernel<MaskMode::kToken>;
  hipLaunchKernelGGL(
      row_kernel, grid, block, 0, stream, input_ids.data_ptr<int32_t>(),
      special.data_ptr<int32_t>(), sample_index.data_ptr<int64_t>(),
      count_table.data_ptr<int32_t>(),
      word_continues != nullptr ? word_continues->data_ptr<uint8_t>() : nullptr,
      span_table != nullptr ? span_table->data_ptr<int64_t>() : nullptr,
      span_table != nullptr ? static_cast<int>(span_table->size(0)) : 0,
      out[0].data_ptr<int64_t>(), out[1].data_ptr<int64_t>(),
      out[2].data_ptr<int64_t>(),
      dense_labels ? out[5].data_ptr<int64_t>() : nullptr,
      out[3].data_ptr<int64_t>(), out[4].data_ptr<int64_t>(), row_count,
      row_pos, row_label, static_cast<int>(B), static_cast<int>(S),
      static_cast<int>(max_pred), static_cast<uint64_t>(seed),
      static_cast<uint32_t>(epoch), static_cast<uint32_t>(vocab_size),
      mask_token, static_cast<uint64_t>(t_keep),
      static_cast<uint64_t>(t_keep + t_rand));
  HIP_CHECK(hipGetLastError());
  if (word_continues != nullptr) {
    hipLaunchKernelGGL(mlm_mask_scatter_kernel, grid, block, 0, stream,
                       row_count, row_pos, row_label,
                       out[3].data_ptr<int64_t>(), out[4].data_ptr<int64_t>(),
                       static_cast<int>(B), static_cast<int>(max_pred));
    HIP_CHECK(hipGetLastError());
  }
  return out;
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
  return mlm_mask_launch(input_ids, special, sample_index, count_table, nullptr,
                         nullptr, seed, epoch, max_pred, vocab_size, mask_token, t_keep,
                         t_rand, dense_labels);
}

std::vector<torch::Tensor> mlm_mask_whole_word(
    torch::Tensor input_ids, torch::Tensor special, torch::Tensor sample_index,
    torch::Tensor count_table, torch::Tensor word_continues, int64_t seed,
    int64_t epoch, int64_t max_pred, int64_t vocab_size, int64_t mask_token,
    int64_t t_keep, int64_t t_rand, bool dense_labels) {
  return mlm_mask_launch(input_ids, special, sample_index, count_table,
                         &word_continues, nullptr, seed, epoch, max_pred,
                         vocab_size, mask_token, t_keep, t_rand, dense_labels);
}

std::vector<torch::Tensor> mlm_mask_span(
    torch::Tensor input_ids, torch::Tensor special, torch::Tensor sample_index,
    torch::Tensor count_table, torch::Tensor word_continues,
    torch::Tensor span_table, int64_t seed, int64_t epoch, int64_t max_pred,
    int64_t vocab_size, int64_t mask_token, int64_t t_keep, int64_t t_rand,
    bool dense_labels) {
  return mlm_mask_launch(input_ids, special, sample_index, count_table,
                         &word_continues, &span_table, seed, epoch, max_pred,
                         vocab_size, mask_token, t_keep, t_rand, dense_labels);
}

}  // namespace bpa
