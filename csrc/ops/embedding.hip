// Fused embedding gather + add + LayerNorm + dropout for MI355X (gfx950).
//
// BertEmbeddings in one kernel (reference: src/modeling.py:338-373):
//   z = word[ids] + pos[s] (+ tok[tt]) ; y = dropout(LN(z))
// Tables may be fp32 (autocast mode) or bf16/fp16 (pure-bf16 master-
// weight mode); the output is emitted in the requested dtype. Backward:
// dz from LN-backward (stored to a fp32 buffer), then pos/token-type
// reductions and a sorted, fixed-order scatter-add into a dense fp32
// word-embedding gradient (cast to the table dtype by the Python
// wrapper when the tables are low-precision). No float atomics: every
// gradient is bitwise identical from run to run.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../checks.h"
#include "../ops.h"
#include "rowwise.h"

namespace bpa {

template <typename T, typename TW, int VEC, bool HAS_TOK, bool TRAIN_DROP>
__global__ void embed_fwd_kernel(
    const int64_t* __restrict__ ids, const int64_t* __restrict__ tt,
    const TW* __restrict__ word, const TW* __restrict__ pos,
    const TW* __restrict__ tok, const float* __restrict__ gamma,
    const float* __restrict__ beta, T* __restrict__ y, float* __restrict__ z,
    uint8_t* __restrict__ mask, float* __restrict__ mean,
    float* __restrict__ rstd, int rows, int seq_len, int H, float p, float eps,
    uint64_t seed, uint64_t offset) {
  // one BLOCK per row; ITEMS slices per thread held in registers
  // through the mean/var reduction (row core: rowwise.h). Keeps its own
  // ITEMS and thread count, not launch_by_items.
  __shared__ float red[16], red2[16];
  const int row = blockIdx.x;
  if (row >= rows) return;
  const int64_t base = static_cast<int64_t>(row) * H;
  const int s = row % seq_len;
  const int64_t wid = ids[row];
  const int64_t tid_ = HAS_TOK ? tt[row] : 0;
  const TW* wrow = word + wid * H;
  const TW* prow = pos + static_cast<int64_t>(s) * H;
  const TW* trow = HAS_TOK ? tok + tid_ * H : nullptr;
  const float keep_scale = TRAIN_DROP ? 1.0f / (1.0f - p) : 1.0f;
  Philox philox(seed);

  constexpr int ITEMS = 2;  // covers H <= 2*blockDim*VEC
  float zv[ITEMS][VEC];
  int cols[ITEMS];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int c = (i * blockDim.x + threadIdx.x) * VEC;
    cols[i] = c;
    if (c < H) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float t = DTraits<TW>::to_f32(wrow[c + k]) +
                  DTraits<TW>::to_f32(prow[c + k]);
        if (HAS_TOK) t += DTraits<TW>::to_f32(trow[c + k]);
        zv[i][k] = t;
        sum += t;
      }
      store_slice(z + base + c, zv[i]);
    }
  }
  const RowStats st =
      ln_row_stats(zv, cols, sum, H, eps, red, red2, mean, rstd, row);
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int c = cols[i];
    if (c < H) {
      T ov[VEC];
      uint8_t mv[VEC];
      if (TRAIN_DROP) keep_mask(philox, offset, base + c, p, mv);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float t = ln_affine(zv[i][k], st, gamma[c + k], beta[c + k]);
        if (TRAIN_DROP) t = mv[k] ? t * keep_scale : 0.f;
        ov[k] = DTraits<T>::from_f32(t);
      }
      store_slice(y + base + c, ov);
      if (TRAIN_DROP) store_mask(mask + base + c, mv);
    }
  }
}

// backward stage 1: dz = LN_bwd(dropout_bwd(dy)); per-block dgamma/dbeta
template <typename T, int VEC, int NW, bool TRAIN_DROP>
__global__ void embed_bwd_dz_kernel(
    const T* __restrict__ dy, const float* __restrict__ z,
    const uint8_t* __restrict__ mask, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    float* __restrict__ dz, float* __restrict__ part_dgamma,
    float* __restrict__ part_dbeta, int rows, int H, float p,
    int rows_per_block) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lg = reinterpret_cast<float*>(smem_raw) + wave * 2 * H;  // [NW][2H]
  float* lb = lg + H;
  for (int c = lane; c < 2 * H; c += WAVE_SIZE) lg[c] = 0.f;
  const float keep_scale = TRAIN_DROP ? 1.0f / (1.0f - p) : 1.0f;

  const int row0 = blockIdx.x * rows_per_block;
  const int row_end = min(row0 + rows_per_block, rows);
  for (int r = row0 + wave; r < row_end; r += NW) {
    const int64_t base = static_cast<int64_t>(r) * H;
    const float mu = mean[r], rs = rstd[r];
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane * VEC; c < H; c += WAVE_SIZE * VEC) {
      T dv[VEC];
      *reinterpret_cast<uint4*>(dv) = *reinterpret_cast<const uint4*>(dy + base + c);
      uint8_t mv[VEC];
      if (TRAIN_DROP) {
        if (VEC == 8)
          *reinterpret_cast<uint2*>(mv) =
              *reinterpret_cast<const uint2*>(mask + base + c);
        else
          *reinterpret_cast<uint32_t*>(mv) =
              *reinterpret_cast<const uint32_t*>(mask + base + c);
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float d = DTraits<T>::to_f32(dv[k]);
        if (TRAIN_DROP) d = mv[k] ? d * keep_scale : 0.f;
        float zh = (z[base + c + k] - mu) * rs;
        float dw = d * gamma[c + k];
        s1 += dw * zh;
        s2 += dw;
        lg[c + k] += d * zh;
        lb[c + k] += d;
        dz[base + c + k] = dw;  // stash dw; finalized below after row sums
      }
    }
    s1 = wave_reduce_sum(s1) / H;
    s2 = wave_reduce_sum(s2) / H;
    for (int c = lane * VEC; c < H; c += WAVE_SIZE * VEC) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float zh = (z[base + c + k] - mu) * rs;
        dz[base + c + k] = rs * (dz[base + c + k] - s2 - zh * s1);
      }
    }
  }
  __syncthreads();
  float* slab0 = reinterpret_cast<float*>(smem_raw);
  for (int c = threadIdx.x; c < H; c += blockDim.x) {
    float ag = 0.f, ab = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      ag += slab0[w * 2 * H + c];
      ab += slab0[w * 2 * H + H + c];
    }
    part_dgamma[static_cast<int64_t>(blockIdx.x) * H + c] = ag;
    part_dbeta[static_cast<int64_t>(blockIdx.x) * H + c] = ab;
  }
}

// backward stage 2a: word-embedding scatter-add in a fixed order, so that
// rows of a repeated id ([MASK], [CLS], ...) sum bitwise identically from
// run to run (float atomics add in arrival order and do not). The ids
// come stably sorted (`sorted`, with `perm` the source row of each
// position). Block b walks positions [b*kWordRows, (b+1)*kWordRows): a run
// of one id that lies strictly inside is stored to d_word directly; the
// piece that begins at the block's first position goes to head[b], the
// piece that reaches its last position to tail[b] (head[b] if the whole
// block is one run). embed_bwd_word_join_kernel then folds the pieces of
// each run that touches a block edge, in block order. One writer per id.
constexpr int kWordRows = 16;

__global__ void embed_bwd_word_runs_kernel(const float* __restrict__ dz,
                                           const int64_t* __restrict__ sorted,
                                           const int64_t* __restrict__ perm,
                                           float* __restrict__ d_word,
                                           float* __restrict__ head,
                                           float* __restrict__ tail, int rows,
                                           int H) {
  const int p0 = blockIdx.x * kWordRows;
  const int p1 = min(p0 + kWordRows, rows);
  const int64_t boff = static_cast<int64_t>(blockIdx.x) * H;
  for (int c = threadIdx.x; c < H; c += blockDim.x) {
    float acc = 0.f;
    int run_start = p0;
    for (int i = p0; i < p1; ++i) {
      const int64_t id = sorted[i];
      acc += dz[perm[i] * H + c];
      const bool to_end = i + 1 == p1;
      if (to_end || sorted[i + 1] != id) {
        if (run_start == p0) head[boff + c] = acc;
        else if (to_end) tail[boff + c] = acc;
        else d_word[id * H + c] = acc;
        acc = 0.f;
        run_start = i + 1;
      }
    }
  }
}

__global__ void embed_bwd_word_join_kernel(const int64_t* __restrict__ sorted,
                                           const float* __restrict__ head,
                                           const float* __restrict__ tail,
                                           float* __restrict__ d_word,
                                           int rows, int H, int nblocks) {
  const int b = blockIdx.x;
  const int p0 = b * kWordRows;
  const int p1 = min(p0 + kWordRows, rows);
  const int64_t first = sorted[p0];
  const int64_t last = sorted[p1 - 1];
  for (int cand = 0; cand < 2; ++cand) {
    int64_t id;
    const float* piece;
    if (cand == 0) {
      // the run that begins exactly at this block's first position
      if (b > 0 && sorted[p0 - 1] == first) continue;
      id = first;
      piece = head + static_cast<int64_t>(b) * H;
    } else {
      // the run that begins inside this block and reaches its end
      if (last == first) continue;
      id = last;
      piece = tail + static_cast<int64_t>(b) * H;
    }
    // The run reaches this block's end, so it may go on: its last
    // position is upper_bound(id) - 1 (binary search; the fold below then
    // has no data-dependent branch and its loads pipeline). Every block
    // up to the one holding that position begins with `id`, i.e. its
    // head piece belongs to this run.
    int bb_end = b;
    if (last == id) {
      int lo = p1, hi = rows;  // first position in [p1, rows] with sorted != id
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sorted[mid] == id) lo = mid + 1;
        else hi = mid;
      }
      bb_end = (lo - 1) / kWordRows;
    }
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
      float acc = piece[c];
      for (int bb = b + 1; bb <= bb_end; ++bb)
        acc += head[static_cast<int64_t>(bb) * H + c];
      d_word[id * H + c] = acc;
    }
  }
}

// backward stage 2b: position-embedding reduce over batch (deterministic)
__global__ void embed_bwd_pos_kernel(const float* __restrict__ dz,
                                     float* __restrict__ d_pos, int batch,
                                     int seq_len, int H) {
  const int64_t total = static_cast<int64_t>(seq_len) * H;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int s = static_cast<int>(i / H);
    const int c = static_cast<int>(i % H);
    float acc = 0.f;
    for (int b = 0; b < batch; ++b)
      acc += dz[(static_cast<int64_t>(b) * seq_len + s) * H + c];
    d_pos[static_cast<int64_t>(s) * H + c] = acc;
  }
}

// backward stage 2c: token-type reduce (few types; per-block LDS partials)
template <int NW>
__global__ void embed_bwd_tok_kernel(const float* __restrict__ dz,
                                     const int64_t* __restrict__ tt,
                                     float* __restrict__ parts, int rows, int H,
                                     int n_types, int rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lt = reinterpret_cast<float*>(smem_raw);  // [n_types][H]
  for (int c = threadIdx.x; c < n_types * H; c += blockDim.x) lt[c] = 0.f;
  __syncthreads();
  const int row0 = blockIdx.x * rows_per_block;
  const int row_end = min(row0 + rows_per_block, rows);
  // each thread owns its columns and walks the rows in order: no two
  // threads touch one LDS cell, so the sum order is fixed (no atomics)
  for (int c = threadIdx.x; c < H; c += blockDim.x) {
    for (int r = row0; r < row_end; ++r) {
      const int t = static_cast<int>(tt[r]);
      lt[t * H + c] += dz[static_cast<int64_t>(r) * H + c];
    }
  }
  __syncthreads();
  float* out = parts + static_cast<int64_t>(blockIdx.x) * n_types * H;
  for (int c = threadIdx.x; c < n_types * H; c += blockDim.x) out[c] = lt[c];
}

std::vector<torch::Tensor> embedding_ln_dropout_fwd(
    torch::Tensor ids, c10::optional<torch::Tensor> tt, torch::Tensor word,
    torch::Tensor pos, c10::optional<torch::Tensor> tok, torch::Tensor gamma,
    torch::Tensor beta, double p, double eps, int64_t seed, int64_t offset,
    torch::ScalarType out_dtype) {
  TORCH_CHECK(ids.dim() == 2, "embed_fwd: ids must be [B, S]");
  TORCH_CHECK(pos.scalar_type() == word.scalar_type() &&
                  (!tok.has_value() ||
                   tok->scalar_type() == word.scalar_type()),
              "embed_fwd: all tables must share a dtype");
  const int batch = ids.size(0), seq_len = ids.size(1);
  const int rows = batch * seq_len;
  const int H = word.size(1);
  auto ids_c = ids.contiguous();
  const bool has_tok = tok.has_value() && tt.has_value();
  torch::Tensor tt_c;
  if (has_tok) tt_c = tt->contiguous();
  auto gamma_f = gamma.contiguous().to(torch::kFloat32);
  auto beta_f = beta.contiguous().to(torch::kFloat32);
  const bool train_drop = p > 0.0;

  auto y = torch::empty({batch, seq_len, H},
                        word.options().dtype(out_dtype));
  auto fopts = word.options().dtype(torch::kFloat32);
  auto z = torch::empty({rows, H}, fopts);
  auto mask = train_drop
                  ? torch::empty({rows, H}, word.options().dtype(torch::kUInt8))
                  : torch::empty({0}, word.options().dtype(torch::kUInt8));
  auto mean = torch::empty({rows}, fopts);
  auto rstd = torch::empty({rows}, fopts);
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_ROW_DTYPE(out_dtype, "embed_fwd", [&] {
    using out_t = scalar_t;  // the inner dispatch re-binds scalar_t, kVec
    constexpr int kVecOut = kVec;
    TORCH_CHECK(H % kVec == 0, "embed_fwd: H % ", kVec, " != 0");
    const int slices = H / kVec;
    const int threads =
        tmin(1024, (((slices + 1) / 2 + WAVE_SIZE - 1) / WAVE_SIZE) *
                       WAVE_SIZE);
    TORCH_CHECK(slices <= 2 * threads, "embed_fwd: H too large");
    DISPATCH_ROW_DTYPE(word.scalar_type(), "embed_fwd_table", [&] {
      using tw_t = scalar_t;
      by_flag(has_tok, [&](auto tok_c) {
        by_flag(train_drop, [&](auto train_c) {
          hipLaunchKernelGGL(
              (embed_fwd_kernel<out_t, tw_t, kVecOut, decltype(tok_c)::value,
                                decltype(train_c)::value>),
              dim3(rows), dim3(threads), 0, stream, ids_c.data_ptr<int64_t>(),
              has_tok ? tt_c.data_ptr<int64_t>() : nullptr, dptr<tw_t>(word),
              dptr<tw_t>(pos), has_tok ? dptr<tw_t>(*tok) : nullptr,
              gamma_f.data_ptr<float>(), beta_f.data_ptr<float>(),
              dptr<out_t>(y), z.data_ptr<float>(),
              train_drop ? mask.data_ptr<uint8_t>() : nullptr,
              mean.data_ptr<float>(), rstd.data_ptr<float>(), rows, seq_len,
              H, static_cast<float>(p), static_cast<float>(eps),
              static_cast<uint64_t>(seed), static_cast<uint64_t>(offset));
        });
      });
    });
  });
  return {y, z, mask, mean, rstd};
}

std::vector<torch::Tensor> embedding_ln_dropout_bwd(
    torch::Tensor dy, torch::Tensor ids, c10::optional<torch::Tensor> tt,
    torch::Tensor z, torch::Tensor mask, torch::Tensor gamma,
    torch::Tensor mean, torch::Tensor rstd, double p, int64_t vocab,
    int64_t max_pos, int64_t n_types) {
  const int batch = ids.size(0), seq_len = ids.size(1);
  const int rows = batch * seq_len;
  TORCH_CHECK(z.scalar_type() == torch::kFloat32, "embed_bwd: z dtype ",
              z.scalar_type(), " must be ", torch::kFloat32);
  TORCH_CHECK(z.dim() == 2 && z.size(0) == rows && z.is_contiguous(),
              "embed_bwd: z must be contiguous [", rows, ", H], got ",
              z.sizes());
  const int H = z.size(1);
  TORCH_CHECK(dy.numel() == static_cast<int64_t>(rows) * H &&
                  dy.size(-1) == H && dy.is_contiguous(),
              "embed_bwd: dy must be contiguous [", batch, ", ", seq_len,
              ", ", H, "], got ", dy.sizes());
  check_row_stat("embed_bwd", "mean", mean, rows);
  check_row_stat("embed_bwd", "rstd", rstd, rows);
  check_param("embed_bwd", "gamma", gamma, H);
  if (p > 0.0) check_drop_mask("embed_bwd", mask, rows, H);
  TORCH_CHECK(seq_len <= max_pos, "embed_bwd: sequence length ", seq_len,
              " exceeds max_pos ", max_pos);
  auto ids_c = ids.contiguous();
  auto gamma_f = gamma.contiguous().to(torch::kFloat32);
  auto dy2 = dy.view({rows, H});
  const bool train_drop = p > 0.0;
  const bool has_tok = tt.has_value() && n_types > 0;

  auto fopts = z.options();
  auto dz = torch::empty({rows, H}, fopts);
  constexpr int NW = 4;
  const int rows_per_block = 16;
  const int nblocks = (rows + rows_per_block - 1) / rows_per_block;
  auto part_g = torch::empty({nblocks, H}, fopts);
  auto part_b = torch::empty({nblocks, H}, fopts);
  auto stream = at::hip::getCurrentHIPStream();
  const size_t lds = NW * 2 * static_cast<size_t>(H) * sizeof(float);
  DISPATCH_ROW_DTYPE(dy.scalar_type(), "embed_bwd", [&] {
    TORCH_CHECK(H % kVec == 0, "embed_bwd: H % ", kVec, " != 0");
    by_flag(train_drop, [&](auto train_c) {
      auto kernel =
          &embed_bwd_dz_kernel<scalar_t, kVec, NW, decltype(train_c)::value>;
      if (lds > 48 * 1024) {
        HIP_CHECK(hipFuncSetAttribute(
            reinterpret_cast<const void*>(kernel),
            hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      }
      hipLaunchKernelGGL(
          kernel, dim3(nblocks), dim3(NW * WAVE_SIZE), lds, stream,
          dptr<scalar_t>(dy2), z.data_ptr<float>(),
          train_drop ? mask.data_ptr<uint8_t>() : nullptr,
          gamma_f.data_ptr<float>(), mean.data_ptr<float>(),
          rstd.data_ptr<float>(), dz.data_ptr<float>(),
          part_g.data_ptr<float>(), part_b.data_ptr<float>(), rows, H,
          static_cast<float>(p), rows_per_block);
    });
  });

  auto d_word = torch::zeros({vocab, H}, fopts);
  // zeros: embed_bwd_pos_kernel writes rows [0, seq_len) only, and the
  // positions past seq_len must get a zero gradient, not leftover memory
  auto d_pos = seq_len < max_pos ? torch::zeros({max_pos, H}, fopts)
                                 : torch::empty({max_pos, H}, fopts);
  auto d_tok = has_tok ? torch::empty({n_types, H}, fopts)
                       : torch::empty({0}, fopts);
  auto dgamma = col_reduce_full(part_g);
  auto dbeta = col_reduce_full(part_b);

  if (rows > 0) {
    auto sorted_perm = ids_c.view({-1}).sort(/*stable=*/true, /*dim=*/0,
                                            /*descending=*/false);
    auto sorted = std::get<0>(sorted_perm).contiguous();
    auto perm = std::get<1>(sorted_perm).contiguous();
    const int wblocks = (rows + kWordRows - 1) / kWordRows;
    auto head = torch::empty({wblocks, H}, fopts);
    auto tail = torch::empty({wblocks, H}, fopts);
    hipLaunchKernelGGL(embed_bwd_word_runs_kernel, dim3(wblocks), dim3(256), 0,
                       stream, dz.data_ptr<float>(),
                       sorted.data_ptr<int64_t>(), perm.data_ptr<int64_t>(),
                       d_word.data_ptr<float>(), head.data_ptr<float>(),
                       tail.data_ptr<float>(), rows, H);
    hipLaunchKernelGGL(embed_bwd_word_join_kernel, dim3(wblocks), dim3(256), 0,
                       stream, sorted.data_ptr<int64_t>(),
                       head.data_ptr<float>(), tail.data_ptr<float>(),
                       d_word.data_ptr<float>(), rows, H, wblocks);
  }
  const int64_t ptotal = static_cast<int64_t>(seq_len) * H;
  const int pblocks = static_cast<int>(std::min<int64_t>((ptotal + 255) / 256, 2048));
  hipLaunchKernelGGL(embed_bwd_pos_kernel, dim3(pblocks), dim3(256), 0,
                     stream, dz.data_ptr<float>(), d_pos.data_ptr<float>(),
                     batch, seq_len, H);
  if (has_tok) {
    auto tt_c = tt->contiguous();
    auto tparts = torch::empty({nblocks, n_types * H}, fopts);
    const size_t tlds = static_cast<size_t>(n_types) * H * sizeof(float);
    hipLaunchKernelGGL((embed_bwd_tok_kernel<NW>), dim3(nblocks),
                       dim3(NW * WAVE_SIZE), tlds, stream,
                       dz.data_ptr<float>(), tt_c.data_ptr<int64_t>(),
                       tparts.data_ptr<float>(), rows, H,
                       static_cast<int>(n_types), rows_per_block);
    d_tok = col_reduce_full(tparts).view({n_types, H});
  }
  return {d_word, d_pos, d_tok, dgamma, dbeta};
}

}  // namespace bpa
