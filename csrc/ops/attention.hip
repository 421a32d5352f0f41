// Fused scaled-dot-product attention (flash-style) for MI355X (gfx950).
//
// Replaces the reference's 5-op attention path (QK^T, +mask, softmax,
// dropout, PV — src/modeling.py:403-429) with MFMA kernels built on
// v_mfma_f32_16x16x32_bf16 / v_mfma_f32_16x16x32_f16 (one source,
// templated on the 16-bit element type - csrc/mfma_types.h):
//
// Forward: grid (S/128 q-tiles, B*heads); 4 waves/block, 2x16 q-rows
// per wave. K and V staged NATURALLY in LDS (K at a 72-elem stride for
// conflict-free b64 row reads; V at an 80-elem stride for conflict-free
// ds_read_b64_tr_b16 hardware-transpose fragment reads - no transposed
// image is ever built); online softmax with the swapped-QK^T trick
// (S^T = mfma(K, Q)) so each lane's P scores chain directly into the
// PV A-fragment; the padding mask enters as per-sequence valid
// lengths. Dropout keep-masks
// are pre-generated once per forward by dropout_mask_kernel (Philox
// 4x32-10, one BIT per score, rows padded to whole 32-bit words) and
// the [B*NH, S, ceil(S/32)] word tensor is read by forward and both
// backward kernels — measurably cheaper than regenerating the RNG
// stream in each of the three consumers, and 8x less mask traffic
// than the byte-mask variant.
//
// Backward (flash-2 style, atomic-free): two MFMA kernels.
// * attn_bwd_kernel: grid (S/64 kv-tiles, B*heads); each block owns one
//   K/V tile, loops over q-tiles; recomputes P from the saved
//   logsumexp; accumulates dK/dV in registers, written once,
//   exclusively, straight into dqkv.
// * attn_dq_kernel: grid (S/64 q-tiles, B*heads); mirrors the forward's
//   wave-owns-q structure, recomputes S^T/dP^T per K/V tile and chains
//   dS^T fragments into dQ += dS.K MFMAs against K^T staged in LDS —
//   dQ lands in registers and is written once (the previous design
//   pushed ~1k fp32 atomicAdds per wave per q-iter into an fp32
//   workspace plus a pack kernel; that was the backward bottleneck).
//
// Variable-length (packed) layout: the three MFMA kernels take a
// `bool VARLEN` template parameter. With it the batch is one
// [T_pad, 3H] matrix of back-to-back sequences addressed through
// cu_seqlens[B+1]; each sequence's own length bounds its loads, stores
// and tile loops, so padded rows are neither computed nor read (see
// seq_row0/seq_rows below and the attention_varlen_* host wrappers).
// VARLEN=false is the padded layout described above, unchanged.
//
// Fragment convention (consistent A/B slot mapping):
//   A[i][k]/B[k][j]: i|j = lane&15, k = (lane>>4)*4 + (e&3) + 16*(e>>2)
//   C/D[i][j]:       j = lane&15,   i = (lane>>4)*4 + reg
// Only A/B consistency matters for correctness (the contraction is
// permutation-invariant when both sides agree); C/D is the documented
// gfx950 layout.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cmath>
#include <utility>

#include "../common.h"
#include "../ops.h"
#include "../mfma_types.h"

namespace bpa {

// Every MFMA kernel below is templated on the 16-bit element type T
// (__bf16 or _Float16); Tr = Mfma16<T> supplies the fragment vector F8,
// the MFMA, the transpose read and the fp32 conversions. Softmax, lse
// and delta math is fp32 for both.

constexpr int kPad = 8;        // 16-bit row pad: 72-element stride, bank-clean
constexpr int kStride = 64 + kPad;
// Stride for LDS images read with ds_read_b64_tr_b16: 80 elements (40
// dwords) makes the hardware transpose read conflict-free within its
// 32-lane groups ({40r+2c} for r 0..7, c 0..3 covers every even bank
// exactly once). Row-fragment (b64) reads of the same image are 2-way
// (rows r and r+8 share a bank) - acceptable where it saves a whole
// second image (no stride satisfies both patterns: rows need
// gcd(stride_dw,64)=4, tr needs gcd=8).
constexpr int kTrStride = 80;

// Build an A/B fragment from a row-major 16-bit row pointer: elements at
// k = base + g*4 + (e&3) + 16*(e>>2), loaded as two 8-byte chunks.
template <typename T>
__device__ __forceinline__ typename Mfma16<T>::frag frag_row(const T* row,
                                                             int base,
                                                             int g) {
  union {
    typename Mfma16<T>::frag v;
    uint2 u[2];
  } r;
  r.u[0] = *reinterpret_cast<const uint2*>(row + base + g * 4);
  r.u[1] = *reinterpret_cast<const uint2*>(row + base + 16 + g * 4);
  return r.v;
}

// Transposed A/B fragment via gfx950's hardware transpose read, straight
// from a NATURAL row-major [rows][kTrStride] bf16 LDS image: element
// e = M[rb + g*4 + (e&3) + 16*(e>>2)][cb + li] - i.e. the fragment the
// old code read from a separately-built transposed image. Semantics
// probe-verified on hardware (tr16_probe): within each 16-lane group,
// out[lane i][j] = mem[addr_of_lane(4j + (i>>2)) + (i&3)], so lane
// (g, t) points at 4 contiguous elements of row rb + g*4 + (t>>2) and
// the instruction delivers the group-transposed fragment. Replaces the
// per-thread 16x ds_write_b16 transpose scatter at staging time.
template <typename T>
__device__ __forceinline__ typename Mfma16<T>::frag frag_tr(const T* img,
                                                            int rb, int cb) {
  using Tr = Mfma16<T>;
  const int lane = threadIdx.x & 63;
  const int g = (lane >> 4) & 3, t = lane & 15;
  const T* p0 =
      img + (rb + g * 4 + (t >> 2)) * kTrStride + cb + (t & 3) * 4;
  union {
    typename Tr::frag v;
    typename Tr::tr4 h[2];
  } r;
  r.h[0] = Tr::tr_read(p0);
  r.h[1] = Tr::tr_read(p0 + 16 * kTrStride);
  return r.v;
}

// Dropout keep-mask generation, BIT-packed: one keep decision per BIT
// (LSB-first within each uint32 word), one thread per word. Each of
// the eight 32-bit Philox outputs (two calls) yields four decisions by
// comparing its bytes against an 8-bit threshold t = round(p*256).
// The host quantizes p to t/256 first (quantize_drop_p) and every
// consumer's 1/(1-p) uses the SAME quantized p, so dropout stays
// exactly unbiased; the ~2^-8 quantization of the drop probability
// itself (0.1 -> 0.1016) is training-irrelevant. History: the original
// one-Philox-per-4-BYTES version was VALU-bound at ~1.4 TB/s and 2.9%
// of phase-2 GPU time; bytes->bits also cuts the mask footprint and
// the three consumers' read traffic 8x (24 layers x [B*NH,S,S] masks
// alive per micro-batch = 1.6 GB at phase 2 as bytes, 200 MB as bits).
// Rows are padded to whole words (stride Sw = ceil(S/32)) so no quad
// ever straddles a word. Counter for word i is offset + 2i (+1),
// deterministic in (seed, offset). Running this as its own elementwise
// kernel keeps the MFMA kernels free of RNG VALU work.
__global__ void dropout_mask_kernel(uint32_t* __restrict__ mask,
                                    int64_t words, uint32_t thresh,
                                    uint64_t seed, uint64_t offset) {
  const int64_t i =
      static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= words) return;
  Philox philox(seed);
  uint32_t r[8];
  philox(offset + 2 * i, r);
  philox(offset + 2 * i + 1, r + 4);
  uint32_t bits = 0;
#pragma unroll
  for (int j = 0; j < 32; ++j)
    bits |= (((r[j >> 2] >> (8 * (j & 3))) & 0xFFu) >= thresh ? 1u : 0u)
            << j;
  mask[i] = bits;
}

// Quantize a dropout probability to the 8-bit threshold grid the mask
// kernel samples on. Both the threshold and every keep-scale are
// derived from the returned pair so the expectation is exact.
static inline std::pair<uint32_t, float> quantize_drop_p(double p) {
  uint32_t t = static_cast<uint32_t>(std::lround(p * 256.0));
  if (t > 255) t = 255;
  return {t, static_cast<float>(t) / 256.0f};
}

// Variable-length (packed) addressing. The MFMA kernels below take a
// `bool VARLEN` template parameter: false is the padded [B, S] layout,
// where `seqlens[b]` only masks keys and every sequence owns S rows
// starting at row b*S; true is the packed [T_pad] layout, where the
// same pointer argument carries cu_seqlens[B+1] - sequence b owns rows
// cu_seqlens[b] .. cu_seqlens[b+1]-1 and that length replaces S in
// every load/store guard, the query-row clamp and both tile loops. S
// (= max_seqlen) keeps addressing lse, delta and the dropout bit-mask,
// whose layouts do not change. The length is clamped to S so a bad
// index can not push an lse/delta/mask access past its [.., S] row.
template <bool VARLEN>
__device__ __forceinline__ int64_t seq_row0(const int* __restrict__ seqlens,
                                            int b, int S) {
  if constexpr (VARLEN) return static_cast<int64_t>(seqlens[b]);
  return static_cast<int64_t>(b) * S;
}

template <bool VARLEN>
__device__ __forceinline__ int seq_rows(const int* __restrict__ seqlens,
                                        int b, int S) {
  if constexpr (VARLEN) return min(seqlens[b + 1] - seqlens[b], S);
  return S;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <typename T, bool TRAIN_DROP, bool VARLEN = false>
__global__ __launch_bounds__(256) void attn_fwd_kernel(
    const T* __restrict__ qkv, const int* __restrict__ seqlens,
    T* __restrict__ out, float* __restrict__ lse_out,
    const uint32_t* __restrict__ dmask, int B, int S, int NH, float p,
    float scale, uint64_t seed, uint64_t offset) {
  using Tr = Mfma16<T>;
  using F8 = typename Tr::frag;
  // 4 waves x 32 q-rows (two 16-row subtiles per wave): the K/V tile is
  // staged once per 128 q-rows, each K/V fragment read feeds TWO
  // independent MFMA chains, and the softmax work of the two subtiles
  // interleaves - targeting the measured issue-stall/parked time.
  const int bh = blockIdx.y;
  const int b = bh / NH, h = bh % NH;
  const int q0 = blockIdx.x * 128;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int g = (lane >> 4), li = lane & 15;
  const int H = NH * 64;
  const int rs3 = 3 * H;  // qkv row stride
  const int64_t row0 = seq_row0<VARLEN>(seqlens, b, S);
  const int L = seq_rows<VARLEN>(seqlens, b, S);  // row bound of this sequence
  const T* qbase = qkv + row0 * rs3 + h * 64;
  const T* kbase = qbase + H;
  const T* vbase = qbase + 2 * H;
  const int slen = VARLEN ? L : seqlens[b];
  const float inv_keep = TRAIN_DROP ? 1.f / (1.f - p) : 1.f;
  const int Sw = (S + 31) >> 5;  // mask row stride in words
  const uint32_t* mask_base =
      TRAIN_DROP ? dmask + static_cast<int64_t>(bh) * S * Sw : nullptr;

  // packed layout: a q-tile at or past this sequence's end has no rows
  if (VARLEN && q0 >= L) return;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* K_lds = reinterpret_cast<T*>(smem);             // [64][72]
  T* V_lds = K_lds + 64 * kStride;   // [64][80] natural, tr-read
  float* alpha_lds = reinterpret_cast<float*>(V_lds + 64 * kTrStride);  // [4][2][16]
  float* stat_lds = alpha_lds + 4 * 2 * 16;                    // [4][2][16]
  // keep-mask words for the current kv-tile, [128 q][2 words]: staged
  // coalesced (one word per thread) instead of per-lane scattered 4-byte
  // global reads in the softmax loop
  uint32_t* mk_lds = reinterpret_cast<uint32_t*>(stat_lds + 4 * 2 * 16);

  // this wave's two q-subtiles: rows q0 + wave*32 + sub*16 + li
  int q_row[2];
  F8 qfrag[2][2];
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
    q_row[sub] = q0 + wave * 32 + sub * 16 + li;
    const int q_ld = min(q_row[sub], L - 1);
#pragma unroll
    for (int c = 0; c < 2; ++c)
      qfrag[sub][c] =
          frag_row(qbase + static_cast<int64_t>(q_ld) * rs3, 32 * c, g);
  }

  float m_run[2] = {-1e30f, -1e30f}, l_run[2] = {0.f, 0.f};
  f32x4 acc_o[2][4] = {};

  const int n_kv = (L + 63) / 64;
  for (int kt = 0; kt < n_kv; ++kt) {
    const int k0 = kt * 64;
    __syncthreads();
    // stage K natural + V transposed; 4 threads per row, 16 cols each
    {
      const int row = tid >> 2, colc = (tid & 3) * 16;
      const int krow = k0 + row;
      if (krow < L) {
        const uint4* src =
            reinterpret_cast<const uint4*>(kbase + static_cast<int64_t>(krow) * rs3 + colc);
        *reinterpret_cast<uint4*>(&K_lds[row * kStride + colc]) = src[0];
        *reinterpret_cast<uint4*>(&K_lds[row * kStride + colc + 8]) = src[1];
        const uint4* vsrc =
            reinterpret_cast<const uint4*>(vbase + static_cast<int64_t>(krow) * rs3 + colc);
        *reinterpret_cast<uint4*>(&V_lds[row * kTrStride + colc]) = vsrc[0];
        *reinterpret_cast<uint4*>(&V_lds[row * kTrStride + colc + 8]) = vsrc[1];
      } else {
        uint4 zero{0, 0, 0, 0};
        *reinterpret_cast<uint4*>(&K_lds[row * kStride + colc]) = zero;
        *reinterpret_cast<uint4*>(&K_lds[row * kStride + colc + 8]) = zero;
        *reinterpret_cast<uint4*>(&V_lds[row * kTrStride + colc]) = zero;
        *reinterpret_cast<uint4*>(&V_lds[row * kTrStride + colc + 8]) = zero;
      }
      if (TRAIN_DROP) {
        const int qrow_m = q0 + (tid >> 1);
        const int kw = (k0 >> 5) + (tid & 1);  // 2 words cover 64 keys
        uint32_t bits = 0xFFFFFFFFu;
        if (qrow_m < L && kw < Sw)
          bits = mask_base[static_cast<int64_t>(qrow_m) * Sw + kw];
        mk_lds[tid] = bits;
      }
    }
    __syncthreads();

    // S^T tiles: one K-fragment pair feeds both subtiles' MFMA chains
    f32x4 s_acc[2][4];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const T* krow = &K_lds[(t * 16 + li) * kStride];
      const F8 kf0 = frag_row(krow, 0, g);
      const F8 kf1 = frag_row(krow, 32, g);
      f32x4 a0 = {}, a1 = {};
      a0 = Tr::mfma(kf0, qfrag[0][0], a0);
      a1 = Tr::mfma(kf0, qfrag[1][0], a1);
      a0 = Tr::mfma(kf1, qfrag[0][1], a0);
      a1 = Tr::mfma(kf1, qfrag[1][1], a1);
      s_acc[0][t] = a0;
      s_acc[1][t] = a1;
    }
    __builtin_amdgcn_s_setprio(0);

    float sv[2][4][4];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      float tmax = -1e30f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + t * 16 + g * 4 + r;
          const bool valid = key < slen && key < L;
          sv[sub][t][r] = valid ? s_acc[sub][t][r] * scale : -1e30f;
          tmax = fmaxf(tmax, sv[sub][t][r]);
        }
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
      const float m_new = fmaxf(m_run[sub], tmax);
      const float alpha = __expf(m_run[sub] - m_new);
      float rowsum = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sv[sub][t][r] = __expf(sv[sub][t][r] - m_new);
          rowsum += sv[sub][t][r];
        }
      rowsum += __shfl_xor(rowsum, 16, 64);
      rowsum += __shfl_xor(rowsum, 32, 64);
      l_run[sub] = l_run[sub] * alpha + rowsum;
      m_run[sub] = m_new;
      if (g == 0) alpha_lds[(wave * 2 + sub) * 16 + li] = alpha;
    }
    __builtin_amdgcn_s_waitcnt(0);  // lgkmcnt(0): same-wave LDS visibility
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc_o[sub][n][r] *= alpha_lds[(wave * 2 + sub) * 16 + g * 4 + r];

    if (TRAIN_DROP) {
      // keep-mask pre-generated by dropout_mask_kernel (no RNG VALU
      // work in the MFMA kernels). k0 is a multiple of 64, so TWO
      // 32-bit words cover this kv-tile's keys for the whole t-loop -
      // one b64 LDS read per subtile replaces per-lane global loads.
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const int q_loc = wave * 32 + sub * 16 + li;
        uint32_t mw[2];
        *reinterpret_cast<uint2*>(mw) =
            *reinterpret_cast<const uint2*>(&mk_lds[q_loc * 2]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int kk = t * 16 + g * 4;  // key offset within the tile
          const uint32_t nib = (mw[kk >> 5] >> (kk & 31)) & 0xF;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            sv[sub][t][j] = (nib >> j) & 1 ? sv[sub][t][j] * inv_keep : 0.f;
        }
      }
    }

    // P fragments chain from sv; one V^T fragment feeds both subtiles
    F8 pa[2][2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        union {
          F8 v;
          T e[8];
        } pk;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          pk.e[e] = Tr::from_f32(sv[sub][2 * c + (e >> 2)][e & 3]);
        pa[sub][c] = pk.v;
      }
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const F8 vf0 = frag_tr(V_lds, 0, n * 16);
      const F8 vf1 = frag_tr(V_lds, 32, n * 16);
      acc_o[0][n] = Tr::mfma(pa[0][0], vf0, acc_o[0][n]);
      acc_o[1][n] = Tr::mfma(pa[1][0], vf0, acc_o[1][n]);
      acc_o[0][n] = Tr::mfma(pa[0][1], vf1, acc_o[0][n]);
      acc_o[1][n] = Tr::mfma(pa[1][1], vf1, acc_o[1][n]);
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // epilogue: normalize rows by l (broadcast per-wave through LDS)
#pragma unroll
  for (int sub = 0; sub < 2; ++sub)
    if (g == 0) stat_lds[(wave * 2 + sub) * 16 + li] = l_run[sub];
  __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qr = q0 + wave * 32 + sub * 16 + g * 4 + r;
        if (qr < L) {
          const float l = stat_lds[(wave * 2 + sub) * 16 + g * 4 + r];
          const float o = acc_o[sub][n][r] / (l > 0.f ? l : 1.f);
          out[(row0 + qr) * H + h * 64 + n * 16 + li] =
              Tr::from_f32(o);
        }
      }
    }
    if (g == 0 && q_row[sub] < L)
      lse_out[static_cast<int64_t>(bh) * S + q_row[sub]] =
          m_run[sub] + __logf(l_run[sub] > 0.f ? l_run[sub] : 1.f);
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
// delta[bh][q] = rowsum(dO * O) over the 64-wide head dim.
// 8 rows per wave: lane l covers row l/8, elements (l%8)*8..+7 as one
// 16-byte load from each of dO and O — coalesced (the 8 lanes of a row
// touch 128 contiguous bytes), and the row sum needs only 3 xor-shuffle
// rounds within the 8-lane group (the old wave-per-row version was
// reduce-latency-bound at 0.17 TB/s).
template <typename T>
__global__ void attn_delta_kernel(const T* __restrict__ dout,
                                  const T* __restrict__ out,
                                  float* __restrict__ delta, int B, int S,
                                  int NH) {
  const int H = NH * 64;
  const int64_t rows = static_cast<int64_t>(B) * NH * S;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int sub = lane >> 3;          // 8-row group index in wave
  const int part = lane & 7;          // 8-element slice within the row
  const int64_t row =
      (static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + wave) * 8 + sub;
  if (row >= rows) return;
  const int64_t bh = row / S;
  const int q = static_cast<int>(row % S);
  const int b = static_cast<int>(bh) / NH, h = static_cast<int>(bh) % NH;
  const int64_t base =
      (static_cast<int64_t>(b) * S + q) * H + h * 64 + part * 8;
  using Tr = Mfma16<T>;
  T dv[8], ov[8];
  *reinterpret_cast<uint4*>(dv) = *reinterpret_cast<const uint4*>(dout + base);
  *reinterpret_cast<uint4*>(ov) = *reinterpret_cast<const uint4*>(out + base);
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) acc += Tr::to_f32(dv[k]) * Tr::to_f32(ov[k]);
#pragma unroll
  for (int off = 4; off > 0; off >>= 1) acc += __shfl_xor(acc, off, WAVE_SIZE);
  if (part == 0) delta[row] = acc;
}

// Packed-layout delta: the same lane mapping and the same [B*NH, S]
// delta rows, with the dO/O row found through cu_seqlens. Slots past a
// sequence's length have no dO/O row; they are skipped (the 8 lanes of
// a row leave together) and never read by the backward kernels. A
// kernel of its own so that the padded kernel above stays byte-for-byte
// what it was.
template <typename T>
__global__ void attn_delta_varlen_kernel(const T* __restrict__ dout,
                                         const T* __restrict__ out,
                                         float* __restrict__ delta,
                                         const int* __restrict__ cu_seqlens,
                                         int B, int S, int NH) {
  const int H = NH * 64;
  const int64_t rows = static_cast<int64_t>(B) * NH * S;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int sub = lane >> 3;
  const int part = lane & 7;
  const int64_t row =
      (static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + wave) * 8 + sub;
  if (row >= rows) return;
  const int64_t bh = row / S;
  const int q = static_cast<int>(row % S);
  const int b = static_cast<int>(bh) / NH, h = static_cast<int>(bh) % NH;
  if (q >= seq_rows<true>(cu_seqlens, b, S)) return;
  const int64_t base =
      (seq_row0<true>(cu_seqlens, b, S) + q) * H + h * 64 + part * 8;
  using Tr = Mfma16<T>;
  T dv[8], ov[8];
  *reinterpret_cast<uint4*>(dv) = *reinterpret_cast<const uint4*>(dout + base);
  *reinterpret_cast<uint4*>(ov) = *reinterpret_cast<const uint4*>(out + base);
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) acc += Tr::to_f32(dv[k]) * Tr::to_f32(ov[k]);
#pragma unroll
  for (int off = 4; off > 0; off >>= 1) acc += __shfl_xor(acc, off, WAVE_SIZE);
  if (part == 0) delta[row] = acc;
}

// dQ kernel: wave-owns-q structure copied from attn_fwd_kernel.
// Per K/V tile: recompute S^T = K.Q^T and dP^T = V.dO^T via MFMA,
// P = exp(S*scale - lse), dS^T = P*(dP - delta)*scale, then chain dS^T
// lane registers into A-fragments for dQ += dS.K against K^T in LDS
// (exactly how the forward chains P into the PV product). dQ stays in
// registers until the single epilogue store into dqkv's Q slots.
template <typename T, bool TRAIN_DROP, bool VARLEN = false>
__global__ __launch_bounds__(256) void attn_dq_kernel(
    const T* __restrict__ dout, const T* __restrict__ qkv,
    const int* __restrict__ seqlens, const float* __restrict__ lse,
    const float* __restrict__ delta, const uint32_t* __restrict__ dmask,
    T* __restrict__ dqkv, int B, int S, int NH, float p, float scale,
    uint64_t seed, uint64_t offset) {
  using Tr = Mfma16<T>;
  using F8 = typename Tr::frag;
  // 4 waves x 32 q-rows (two 16-row subtiles per wave), mirroring
  // attn_fwd_kernel: K/V/K^T staged once per 128 q-rows, every staged
  // fragment feeds two independent MFMA chains.
  const int bh = blockIdx.y;
  const int b = bh / NH, h = bh % NH;
  const int q0 = blockIdx.x * 128;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int g = (lane >> 4), li = lane & 15;
  const int H = NH * 64;
  const int rs3 = 3 * H;
  const int64_t row0 = seq_row0<VARLEN>(seqlens, b, S);
  const int L = seq_rows<VARLEN>(seqlens, b, S);  // row bound of this sequence
  const T* qbase = qkv + row0 * rs3 + h * 64;
  const T* kbase = qbase + H;
  const T* vbase = qbase + 2 * H;
  const T* dobase = dout + row0 * H + h * 64;
  const int slen = VARLEN ? L : seqlens[b];
  const float inv_keep = TRAIN_DROP ? 1.f / (1.f - p) : 1.f;
  const int Sw = (S + 31) >> 5;  // mask row stride in words
  const uint32_t* mask_base =
      TRAIN_DROP ? dmask + static_cast<int64_t>(bh) * S * Sw : nullptr;

  if (VARLEN && q0 >= L) return;  // tile past this sequence's end

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // K natural at kTrStride: serves BOTH the S^T-recompute row fragments
  // (2-way bank conflicts, tolerated) and the dQ chain's K^T fragments
  // via hardware transpose reads - no separate transposed image.
  T* K_lds = reinterpret_cast<T*>(smem);   // [64][80] natural
  T* V_lds = K_lds + 64 * kTrStride;            // [64][72] natural
  uint32_t* mk_lds = reinterpret_cast<uint32_t*>(V_lds + 64 * kStride);

  // this wave's two q-subtiles: Q/dO fragments + lse/delta in registers
  int q_row[2];
  F8 qfrag[2][2], dofrag[2][2];
  float lse_q[2], dlt_q[2];
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
    q_row[sub] = q0 + wave * 32 + sub * 16 + li;
    const int q_ld = min(q_row[sub], L - 1);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      qfrag[sub][c] =
          frag_row(qbase + static_cast<int64_t>(q_ld) * rs3, 32 * c, g);
      dofrag[sub][c] =
          frag_row(dobase + static_cast<int64_t>(q_ld) * H, 32 * c, g);
    }
    lse_q[sub] =
        (q_row[sub] < L) ? lse[static_cast<int64_t>(bh) * S + q_row[sub]] : 0.f;
    dlt_q[sub] =
        (q_row[sub] < L) ? delta[static_cast<int64_t>(bh) * S + q_row[sub]] : 0.f;
  }

  f32x4 acc_dq[2][4] = {};

  const int n_kv = (L + 63) / 64;
  for (int kt = 0; kt < n_kv; ++kt) {
    const int k0 = kt * 64;
    __syncthreads();
    {
      const int row = tid >> 2, colc = (tid & 3) * 16;
      const int krow = k0 + row;
      if (krow < L) {
        const uint4* ks = reinterpret_cast<const uint4*>(
            kbase + static_cast<int64_t>(krow) * rs3 + colc);
        *reinterpret_cast<uint4*>(&K_lds[row * kTrStride + colc]) = ks[0];
        *reinterpret_cast<uint4*>(&K_lds[row * kTrStride + colc + 8]) = ks[1];
        const uint4* vs = reinterpret_cast<const uint4*>(
            vbase + static_cast<int64_t>(krow) * rs3 + colc);
        *reinterpret_cast<uint4*>(&V_lds[row * kStride + colc]) = vs[0];
        *reinterpret_cast<uint4*>(&V_lds[row * kStride + colc + 8]) = vs[1];
      } else {
        uint4 zero{0, 0, 0, 0};
        *reinterpret_cast<uint4*>(&K_lds[row * kTrStride + colc]) = zero;
        *reinterpret_cast<uint4*>(&K_lds[row * kTrStride + colc + 8]) = zero;
        *reinterpret_cast<uint4*>(&V_lds[row * kStride + colc]) = zero;
        *reinterpret_cast<uint4*>(&V_lds[row * kStride + colc + 8]) = zero;
      }
      if (TRAIN_DROP) {
        const int qrow_m = q0 + (tid >> 1);
        const int kw = (k0 >> 5) + (tid & 1);
        uint32_t bits = 0xFFFFFFFFu;
        if (qrow_m < L && kw < Sw)
          bits = mask_base[static_cast<int64_t>(qrow_m) * Sw + kw];
        mk_lds[tid] = bits;
      }
    }
    __syncthreads();

    // S^T and dP^T tiles (C[key][q], q = li); K/V fragments shared.
    // dS packs straight into its A-fragment slots (element
    // e = (t&1)*4 + r of chunk t>>1) - no [2][4][4] staging array.
    union FB {
      F8 v;
      T e[8];
    };
    FB dsfrag[2][2];
    // (setprio brackets are inside the loops below)
    // keep-mask words for this kv-tile (two words cover keys
    // k0..k0+63 for each q-subtile; k0 is a multiple of 64)
    uint32_t mw[2][2] = {{0xFFFFFFFFu, 0xFFFFFFFFu},
                         {0xFFFFFFFFu, 0xFFFFFFFFu}};
    if (TRAIN_DROP) {
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const int q_loc = wave * 32 + sub * 16 + li;
        *reinterpret_cast<uint2*>(mw[sub]) =
            *reinterpret_cast<const uint2*>(&mk_lds[q_loc * 2]);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const T* krow = &K_lds[(t * 16 + li) * kTrStride];
      const T* vrow = &V_lds[(t * 16 + li) * kStride];
      const F8 kf0 = frag_row(krow, 0, g), kf1 = frag_row(krow, 32, g);
      const F8 vf0 = frag_row(vrow, 0, g), vf1 = frag_row(vrow, 32, g);
      f32x4 sacc[2] = {}, dpacc[2] = {};
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        sacc[sub] = Tr::mfma(kf0, qfrag[sub][0], sacc[sub]);
        sacc[sub] = Tr::mfma(kf1, qfrag[sub][1], sacc[sub]);
        dpacc[sub] = Tr::mfma(vf0, dofrag[sub][0], dpacc[sub]);
        dpacc[sub] = Tr::mfma(vf1, dofrag[sub][1], dpacc[sub]);
      }
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const int kk = t * 16 + g * 4;  // key offset within the tile
        const uint32_t nib = (mw[sub][kk >> 5] >> (kk & 31)) & 0xF;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + t * 16 + g * 4 + r;
          const bool valid = key < slen && key < L && q_row[sub] < L;
          const float pr =
              valid ? __expf(sacc[sub][r] * scale - lse_q[sub]) : 0.f;
          float dpd = dpacc[sub][r];
          if (TRAIN_DROP) {
            dpd = (nib >> r) & 1 ? dpd * inv_keep : 0.f;
          }
          dsfrag[sub][t >> 1].e[(t & 1) * 4 + r] =
              Tr::from_f32(pr * (dpd - dlt_q[sub]) * scale);
        }
      }
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const F8 ktf0 = frag_tr(K_lds, 0, n * 16);
      const F8 ktf1 = frag_tr(K_lds, 32, n * 16);
      acc_dq[0][n] = Tr::mfma(dsfrag[0][0].v, ktf0, acc_dq[0][n]);
      acc_dq[1][n] = Tr::mfma(dsfrag[1][0].v, ktf0, acc_dq[1][n]);
      acc_dq[0][n] = Tr::mfma(dsfrag[0][1].v, ktf1, acc_dq[0][n]);
      acc_dq[1][n] = Tr::mfma(dsfrag[1][1].v, ktf1, acc_dq[1][n]);
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // epilogue: one store per element into dqkv Q slots
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qr = q0 + wave * 32 + sub * 16 + g * 4 + r;
        if (qr < L) {
          dqkv[(row0 + qr) * rs3 + h * 64 + n * 16 +
               li] = Tr::from_f32(acc_dq[sub][n][r]);
        }
      }
    }
  }
}

template <typename T, bool TRAIN_DROP, bool VARLEN = false>
__global__ __launch_bounds__(256) void attn_bwd_kernel(
    const T* __restrict__ dout, const T* __restrict__ qkv,
    const int* __restrict__ seqlens, const float* __restrict__ lse,
    const float* __restrict__ delta, const uint32_t* __restrict__ dmask,
    T* __restrict__ dqkv, int B, int S, int NH, float p, float scale,
    uint64_t seed, uint64_t offset) {
  using Tr = Mfma16<T>;
  using F8 = typename Tr::frag;
  // 4 waves x 32 keys (two 16-key subtiles per wave): the heavy per-
  // q-tile staging of Q/Q^T/dO/dO^T is amortized over 128 keys, and
  // every staged Q/dO/Q^T/dO^T fragment feeds two MFMA chains.
  const int bh = blockIdx.y;
  const int b = bh / NH, h = bh % NH;
  const int k0 = blockIdx.x * 128;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int g = (lane >> 4), li = lane & 15;
  const int H = NH * 64;
  const int rs3 = 3 * H;
  const int64_t row0 = seq_row0<VARLEN>(seqlens, b, S);
  const int L = seq_rows<VARLEN>(seqlens, b, S);  // row bound of this sequence
  const T* qbase = qkv + row0 * rs3 + h * 64;
  const T* kbase = qbase + H;
  const T* vbase = qbase + 2 * H;
  const T* dobase = dout + row0 * H + h * 64;
  const int slen = VARLEN ? L : seqlens[b];
  const float inv_keep = TRAIN_DROP ? 1.f / (1.f - p) : 1.f;
  const int Sw = (S + 31) >> 5;  // mask row stride in words
  const uint32_t* mask_base =
      TRAIN_DROP ? dmask + static_cast<int64_t>(bh) * S * Sw : nullptr;

  if (VARLEN && k0 >= L) return;  // key tile past this sequence's end

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // Q and dO at kTrStride serve BOTH row fragments (S/dP recompute;
  // 2-way conflicts) and the dK/dV chains' transposed fragments via
  // hardware transpose reads - the Qt/dOt images and their 16-scalar-
  // write-per-thread transpose scatters are gone.
  T* K_lds = reinterpret_cast<T*>(smem);   // [128][72] natural
  T* V_lds = K_lds + 128 * kStride;             // [128][72] natural
  T* Q_lds = V_lds + 128 * kStride;             // [64][80] natural
  T* dO_lds = Q_lds + 64 * kTrStride;           // [64][80] natural
  float* lse_lds = reinterpret_cast<float*>(dO_lds + 64 * kTrStride);  // [64]
  float* dlt_lds = lse_lds + 64;                                      // [64]
  // keep-mask tile [64 q][128 keys] as bits, [4 words][64 q], staged per
  // q-tile (raw global reads were byte columns - latency-bound at this
  // kernel's occupancy; 16 lanes share each word via LDS broadcast)
  uint32_t* mk_lds = reinterpret_cast<uint32_t*>(dlt_lds + 64);

  // stage K and V (natural) once: two 64-row passes
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int row = pass * 64 + (tid >> 2), colc = (tid & 3) * 16;
    const int krow = k0 + row;
    T kv[16], vv[16];
    if (krow < L) {
      const uint4* ks =
          reinterpret_cast<const uint4*>(kbase + static_cast<int64_t>(krow) * rs3 + colc);
      *reinterpret_cast<uint4*>(&kv[0]) = ks[0];
      *reinterpret_cast<uint4*>(&kv[8]) = ks[1];
      const uint4* vs =
          reinterpret_cast<const uint4*>(vbase + static_cast<int64_t>(krow) * rs3 + colc);
      *reinterpret_cast<uint4*>(&vv[0]) = vs[0];
      *reinterpret_cast<uint4*>(&vv[8]) = vs[1];
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) kv[j] = vv[j] = Tr::from_f32(0.f);
    }
    *reinterpret_cast<uint4*>(&K_lds[row * kStride + colc]) =
        *reinterpret_cast<uint4*>(&kv[0]);
    *reinterpret_cast<uint4*>(&K_lds[row * kStride + colc + 8]) =
        *reinterpret_cast<uint4*>(&kv[8]);
    *reinterpret_cast<uint4*>(&V_lds[row * kStride + colc]) =
        *reinterpret_cast<uint4*>(&vv[0]);
    *reinterpret_cast<uint4*>(&V_lds[row * kStride + colc + 8]) =
        *reinterpret_cast<uint4*>(&vv[8]);
  }
  __syncthreads();

  f32x4 dv_acc[2][4] = {};  // dV^T[sub][dh-tile] for the wave's 2x16 keys
  f32x4 dk_acc[2][4] = {};

  // async-STAGE split (T14): each q-tile's Q/dO/lse/delta/mask global
  // loads are ISSUED one iteration early, so their HBM latency hides
  // under the previous tile's 64-MFMA recompute instead of sitting
  // serialized between the two staging barriers. The +16 VGPRs of
  // in-flight data keep this kernel at its LDS-bound 2 waves/SIMD.
  const int st_row = tid >> 2, st_colc = (tid & 3) * 16;
  uint4 pf_q0, pf_q1, pf_d0, pf_d1;
  auto issue_loads = [&](int q0t) {
    const int qrow = q0t + st_row;
    if (qrow < L) {
      const uint4* qs = reinterpret_cast<const uint4*>(
          qbase + static_cast<int64_t>(qrow) * rs3 + st_colc);
      pf_q0 = qs[0];
      pf_q1 = qs[1];
      const uint4* ds = reinterpret_cast<const uint4*>(
          dobase + static_cast<int64_t>(qrow) * H + st_colc);
      pf_d0 = ds[0];
      pf_d1 = ds[1];
    } else {
      pf_q0 = pf_q1 = pf_d0 = pf_d1 = uint4{0, 0, 0, 0};
    }
  };
  issue_loads(0);

  const int n_q = (L + 63) / 64;
  for (int qt = 0; qt < n_q; ++qt) {
    const int q0 = qt * 64;
    __syncthreads();  // all waves done reading the previous tile's Q/dO
    // stage this q-tile from the prefetched registers
    {
      *reinterpret_cast<uint4*>(&Q_lds[st_row * kTrStride + st_colc]) = pf_q0;
      *reinterpret_cast<uint4*>(&Q_lds[st_row * kTrStride + st_colc + 8]) =
          pf_q1;
      *reinterpret_cast<uint4*>(&dO_lds[st_row * kTrStride + st_colc]) =
          pf_d0;
      *reinterpret_cast<uint4*>(&dO_lds[st_row * kTrStride + st_colc + 8]) =
          pf_d1;
      if (tid < 64) {
        const int qr = q0 + tid;
        lse_lds[tid] = (qr < L) ? lse[static_cast<int64_t>(bh) * S + qr] : 0.f;
        dlt_lds[tid] = (qr < L) ? delta[static_cast<int64_t>(bh) * S + qr] : 0.f;
      }
      if (TRAIN_DROP) {
        // keep-mask tile [64 q][128 keys] bits, transposed [word][row]
        // so a q-subtile's 4 row-words are one aligned b128 read below;
        // words past the row end are ones (those keys are zeroed by the
        // kvalid/slen guards)
        const int kw = (k0 >> 5) + (tid & 3);  // k0 is a multiple of 128
        const int qrow_m = q0 + st_row;
        uint32_t bits = 0xFFFFFFFFu;
        if (qrow_m < L && kw < Sw)
          bits = mask_base[static_cast<int64_t>(qrow_m) * Sw + kw];
        mk_lds[(tid & 3) * 64 + st_row] = bits;
      }
    }
    __syncthreads();
    if (qt + 1 < n_q) issue_loads(q0 + 64);

    // recompute S tiles for the wave's 2x16 keys x 64 q-rows:
    // S[q][key]: A = Q rows, B = K^T (natural K rows); C col = key = li.
    // Q/dO fragments are shared across the two key subtiles.
    const int key_local0 = wave * 32 + li;
    const int key_local1 = wave * 32 + 16 + li;
    // P and dS go STRAIGHT into their B-fragment slots as each q-tile
    // is produced (element e = (mq&1)*4 + r of chunk mq>>1) - no
    // [2][4][4] staging arrays (they cost ~64 VGPRs and halved
    // occupancy at 324 VGPRs/wave)
    union FB {
      F8 v;
      T e[8];
    };
    FB pfrag[2][2], dsfrag[2][2];
#pragma unroll
    for (int mq = 0; mq < 4; ++mq) {
      const T* qrow_n = &Q_lds[(mq * 16 + li) * kTrStride];
      const T* dorow = &dO_lds[(mq * 16 + li) * kTrStride];
      const F8 qa0 = frag_row(qrow_n, 0, g), qa1 = frag_row(qrow_n, 32, g);
      const F8 da0 = frag_row(dorow, 0, g), da1 = frag_row(dorow, 32, g);
      f32x4 acc[2] = {}, dp[2] = {};
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const int key_local = sub ? key_local1 : key_local0;
        const T* krow_n = &K_lds[key_local * kStride];
        const T* vrow = &V_lds[key_local * kStride];
        acc[sub] = Tr::mfma(qa0, frag_row(krow_n, 0, g), acc[sub]);
        acc[sub] = Tr::mfma(qa1, frag_row(krow_n, 32, g), acc[sub]);
        dp[sub] = Tr::mfma(da0, frag_row(vrow, 0, g), dp[sub]);
        dp[sub] = Tr::mfma(da1, frag_row(vrow, 32, g), dp[sub]);
      }
      uint32_t mrow4[4];  // keep-mask words for rows mq*16+g*4+0..3
      if (TRAIN_DROP)     // both key subtiles live in word column `wave`
        *reinterpret_cast<uint4*>(mrow4) = *reinterpret_cast<const uint4*>(
            &mk_lds[wave * 64 + mq * 16 + g * 4]);
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const int key_abs = k0 + (sub ? key_local1 : key_local0);
        const bool kvalid = key_abs < slen && key_abs < L;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q_abs = q0 + mq * 16 + g * 4 + r;
          const float row_lse = lse_lds[mq * 16 + g * 4 + r];
          const float d_row = dlt_lds[mq * 16 + g * 4 + r];
          float pr = (kvalid && q_abs < L)
                         ? __expf(acc[sub][r] * scale - row_lse)
                         : 0.f;
          float dpd = dp[sub][r];
          float pkeep = pr;
          if (TRAIN_DROP) {
            const int key_l = sub ? key_local1 : key_local0;
            const bool keep = (mrow4[r] >> (key_l & 31)) & 1;
            dpd = keep ? dpd * inv_keep : 0.f;
            pkeep = keep ? pr * inv_keep : 0.f;  // dropped P feeds dV
          }
          pfrag[sub][mq >> 1].e[(mq & 1) * 4 + r] = Tr::from_f32(pkeep);
          dsfrag[sub][mq >> 1].e[(mq & 1) * 4 + r] =
              Tr::from_f32(pr * (dpd - d_row) * scale);
        }
      }
    }

    // dV^T += dO^T x P ; dK^T += Q^T x dS — dO^T/Q^T fragments shared
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const F8 dt0 = frag_tr(dO_lds, 0, m * 16);
      const F8 dt1 = frag_tr(dO_lds, 32, m * 16);
      const F8 qt0 = frag_tr(Q_lds, 0, m * 16);
      const F8 qt1 = frag_tr(Q_lds, 32, m * 16);
      dv_acc[0][m] = Tr::mfma(dt0, pfrag[0][0].v, dv_acc[0][m]);
      dv_acc[1][m] = Tr::mfma(dt0, pfrag[1][0].v, dv_acc[1][m]);
      dv_acc[0][m] = Tr::mfma(dt1, pfrag[0][1].v, dv_acc[0][m]);
      dv_acc[1][m] = Tr::mfma(dt1, pfrag[1][1].v, dv_acc[1][m]);
      dk_acc[0][m] = Tr::mfma(qt0, dsfrag[0][0].v, dk_acc[0][m]);
      dk_acc[1][m] = Tr::mfma(qt0, dsfrag[1][0].v, dk_acc[1][m]);
      dk_acc[0][m] = Tr::mfma(qt1, dsfrag[0][1].v, dk_acc[0][m]);
      dk_acc[1][m] = Tr::mfma(qt1, dsfrag[1][1].v, dk_acc[1][m]);
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // write dK/dV straight into dqkv (this block owns keys k0..k0+127)
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int dh = m * 16 + g * 4 + r;  // C row = dh/d index
        const int key_abs = k0 + wave * 32 + sub * 16 + li;
        if (key_abs < L) {
          const int64_t rowb = row0 + key_abs;
          dqkv[rowb * rs3 + H + h * 64 + dh] = Tr::from_f32(dk_acc[sub][m][r]);
          dqkv[rowb * rs3 + 2 * H + h * 64 + dh] = Tr::from_f32(dv_acc[sub][m][r]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// ds_read_b64_tr_b16 semantics probe (debug utility; used once per ROCm
// bump to verify the lane->element mapping the PV/dK/dV fragment reads
// rely on). LDS is filled with the identity pattern (element i = i) and
// each lane reads at its own 8-byte-aligned address (8*lane bytes);
// out[l][j] then IS the element index lane l's slot j received.
// ---------------------------------------------------------------------------
__global__ void tr16_probe_kernel(float* __restrict__ out, int addr_mode) {
  __shared__ __bf16 lds[1024];
  const int t = threadIdx.x;
  for (int i = t; i < 1024; i += 64) lds[i] = __bf16(static_cast<float>(i));
  __syncthreads();
  typedef __attribute__((__vector_size__(4 * sizeof(__bf16)))) __bf16 bf16x4v;
  int elem_off;
  switch (addr_mode) {
    case 0: elem_off = t * 4; break;           // 8 B per lane, contiguous
    case 1: elem_off = 0; break;               // uniform base
    case 2: elem_off = (t & 15) * 4; break;    // repeats per 16-lane group
    default: elem_off = (t >> 4) * 4; break;   // group-constant
  }
  auto p = (__attribute__((address_space(3))) bf16x4v*)(&lds[elem_off]);
  bf16x4v v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) out[t * 4 + j] = static_cast<float>(v[j]);
}

torch::Tensor tr16_probe(int64_t addr_mode) {
  auto out = torch::empty({64, 4}, torch::TensorOptions()
                                       .dtype(torch::kFloat32)
                                       .device(torch::kCUDA));
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(tr16_probe_kernel, dim3(1), dim3(64), 0, stream,
                     out.data_ptr<float>(), static_cast<int>(addr_mode));
  return out;
}

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------
template <typename T>
static std::vector<torch::Tensor> attention_fwd_t(torch::Tensor qkv,
                                                  torch::Tensor seqlens,
                                                  int64_t num_heads, double p,
                                                  int64_t seed,
                                                  int64_t offset) {
  const int B = qkv.size(0), S = qkv.size(1);
  const int H = qkv.size(2) / 3;
  const int NH = static_cast<int>(num_heads);
  TORCH_CHECK(H == NH * 64, "attn_fwd: head_dim must be 64");
  TORCH_CHECK(S % 16 == 0, "attn_fwd: S must be a multiple of 16");
  auto seql = seqlens.to(qkv.device(), torch::kInt32).contiguous();
  auto out = torch::empty({B, S, H}, qkv.options());
  auto lse = torch::empty({B * NH, S}, qkv.options().dtype(torch::kFloat32));
  const bool train_drop = p > 0.0;
  // keep-mask BITS [B*NH, S, ceil(S/32)] int32 words: written once
  // here, read (not regenerated) by both backward kernels
  const int Sw = (S + 31) / 32;
  auto dmask = train_drop
                   ? torch::empty({static_cast<int64_t>(B) * NH, S, Sw},
                                  qkv.options().dtype(torch::kInt32))
                   : torch::empty({0}, qkv.options().dtype(torch::kInt32));
  const float scale = 1.0f / sqrtf(64.f);
  auto stream = at::hip::getCurrentHIPStream();
  dim3 grid((S + 127) / 128, B * NH), block(256);  // 128 q-rows per block
  const size_t lds = (64 * kStride + 64 * kTrStride) * sizeof(T) +
                     4 * 64 * sizeof(float) + 128 * 2 * sizeof(uint32_t);
  if (train_drop) {
    const auto [thresh, p_q] = quantize_drop_p(p);
    const int64_t words = static_cast<int64_t>(B) * NH * S * Sw;
    hipLaunchKernelGGL(dropout_mask_kernel,
                       dim3((words + 255) / 256), dim3(256), 0, stream,
                       reinterpret_cast<uint32_t*>(dmask.data_ptr<int>()),
                       words, thresh, static_cast<uint64_t>(seed),
                       static_cast<uint64_t>(offset));
    hipLaunchKernelGGL((attn_fwd_kernel<T, true>), grid, block, lds, stream,
                       reinterpret_cast<const T*>(qkv.data_ptr()),
                       seql.data_ptr<int>(),
                       reinterpret_cast<T*>(out.data_ptr()),
                       lse.data_ptr<float>(),
                       reinterpret_cast<const uint32_t*>(
                           dmask.data_ptr<int>()),
                       B, S, NH, p_q, scale,
                       static_cast<uint64_t>(seed),
                       static_cast<uint64_t>(offset));
  } else {
    hipLaunchKernelGGL((attn_fwd_kernel<T, false>), grid, block, lds, stream,
                       reinterpret_cast<const T*>(qkv.data_ptr()),
                       seql.data_ptr<int>(),
                       reinterpret_cast<T*>(out.data_ptr()),
                       lse.data_ptr<float>(), nullptr, B, S, NH,
                       static_cast<float>(p), scale,
                       static_cast<uint64_t>(seed),
                       static_cast<uint64_t>(offset));
  }
  return {out, lse, dmask};
}

// qkv [B,S,3H] bf16 or fp16 -> {out [B,S,H] same dtype, lse fp32, keep-mask}
std::vector<torch::Tensor> attention_fwd(torch::Tensor qkv,
                                         torch::Tensor seqlens,
                                         int64_t num_heads, double p,
                                         int64_t seed, int64_t offset) {
  TORCH_CHECK(qkv.dim() == 3 && qkv.is_contiguous(), "attn_fwd: bad qkv");
  const auto dt = qkv.scalar_type();
  TORCH_CHECK(dt == torch::kBFloat16 || dt == torch::kHalf,
              "attn_fwd: qkv must be bf16 or fp16, got ", dt);
  if (dt == torch::kHalf)
    return attention_fwd_t<_Float16>(qkv, seqlens, num_heads, p, seed,
                                     offset);
  return attention_fwd_t<__bf16>(qkv, seqlens, num_heads, p, seed, offset);
}

template <typename T>
static torch::Tensor attention_bwd_t(torch::Tensor dout, torch::Tensor qkv,
                                     torch::Tensor seqlens, torch::Tensor out,
                                     torch::Tensor lse, torch::Tensor dmask,
                                     int64_t num_heads, double p,
                                     int64_t seed, int64_t offset) {
  const int B = qkv.size(0), S = qkv.size(1);
  const int H = qkv.size(2) / 3;
  const int NH = static_cast<int>(num_heads);
  auto seql = seqlens.to(qkv.device(), torch::kInt32).contiguous();
  auto dqkv = torch::empty_like(qkv);
  auto fopts = qkv.options().dtype(torch::kFloat32);
  auto delta = torch::empty({static_cast<int64_t>(B) * NH * S}, fopts);
  auto stream = at::hip::getCurrentHIPStream();
  auto dout_c = dout.contiguous();

  const int64_t rows = static_cast<int64_t>(B) * NH * S;
  const int64_t delta_waves = (rows + 7) / 8;  // 8 rows per wave
  hipLaunchKernelGGL(attn_delta_kernel<T>, dim3((delta_waves + 3) / 4),
                     dim3(256), 0, stream,
                     reinterpret_cast<const T*>(dout_c.data_ptr()),
                     reinterpret_cast<const T*>(out.data_ptr()),
                     delta.data_ptr<float>(), B, S, NH);

  dim3 grid((S + 127) / 128, B * NH), block(256);  // 128 keys per bwd block
  dim3 grid_dq((S + 127) / 128, B * NH);           // 128 q-rows per dq block
  // K/V hold 128 rows at kStride; Q/dO 64 rows at kTrStride (tr-read);
  // + 1 KB bit-mask tile -> ~59 KB (over the 64 KB default dynamic-LDS
  // cap; MI355X has 160 KB per CU)
  const size_t lds = (4 * 64 * kStride + 2 * 64 * kTrStride) *
                         sizeof(T) +
                     2 * 64 * sizeof(float) + 64 * 4 * sizeof(uint32_t);
  const size_t lds_dq = (64 * kStride + 64 * kTrStride) * sizeof(T) +
                        128 * 2 * sizeof(uint32_t);
  HIP_CHECK(hipFuncSetAttribute(
      reinterpret_cast<const void*>(&attn_bwd_kernel<T, true>),
      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  HIP_CHECK(hipFuncSetAttribute(
      reinterpret_cast<const void*>(&attn_bwd_kernel<T, false>),
      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const float scale = 1.0f / sqrtf(64.f);
  const bool train_drop = p > 0.0;
  // same 8-bit quantization as the forward's mask generation, so the
  // backward keep-scale matches the stored mask's statistics exactly
  const float p_q = quantize_drop_p(p).second;
  const uint32_t* mask_ptr =
      train_drop ? reinterpret_cast<const uint32_t*>(dmask.data_ptr<int>())
                 : nullptr;
  auto args = [&](auto kernel, dim3 g, size_t lds_bytes) {
    hipLaunchKernelGGL(kernel, g, block, lds_bytes, stream,
                       reinterpret_cast<const T*>(dout_c.data_ptr()),
                       reinterpret_cast<const T*>(qkv.data_ptr()),
                       seql.data_ptr<int>(), lse.data_ptr<float>(),
                       delta.data_ptr<float>(), mask_ptr,
                       reinterpret_cast<T*>(dqkv.data_ptr()), B, S, NH,
                       p_q, scale,
                       static_cast<uint64_t>(seed),
                       static_cast<uint64_t>(offset));
  };
  if (train_drop) {
    args(attn_bwd_kernel<T, true>, grid, lds);
    args(attn_dq_kernel<T, true>, grid_dq, lds_dq);
  } else {
    args(attn_bwd_kernel<T, false>, grid, lds);
    args(attn_dq_kernel<T, false>, grid_dq, lds_dq);
  }
  return dqkv;
}

// dout/qkv/out must share one dtype (bf16 or fp16); checked before any
// launch so a mixed call cannot reinterpret one operand's bits.
torch::Tensor attention_bwd(torch::Tensor dout, torch::Tensor qkv,
                            torch::Tensor seqlens, torch::Tensor out,
                            torch::Tensor lse, torch::Tensor dmask,
                            int64_t num_heads, double p, int64_t seed,
                            int64_t offset) {
  const auto dt = qkv.scalar_type();
  TORCH_CHECK(dt == torch::kBFloat16 || dt == torch::kHalf,
              "attn_bwd: qkv must be bf16 or fp16, got ", dt);
  TORCH_CHECK(dout.scalar_type() == dt,
              "attn_bwd: dout dtype ", dout.scalar_type(),
              " does not match qkv dtype ", dt);
  TORCH_CHECK(out.scalar_type() == dt, "attn_bwd: out dtype ",
              out.scalar_type(), " does not match qkv dtype ", dt);
  if (dt == torch::kHalf)
    return attention_bwd_t<_Float16>(dout, qkv, seqlens, out, lse, dmask,
                                     num_heads, p, seed, offset);
  return attention_bwd_t<__bf16>(dout, qkv, seqlens, out, lse, dmask,
                                 num_heads, p, seed, offset);
}

// ---------------------------------------------------------------------------
// variable-length (packed) host wrappers
// ---------------------------------------------------------------------------
// qkv is the packed [T_pad, 3H] QKV GEMM output of a batch whose valid
// tokens sit back to back; cu_seqlens[B+1] int32 (device) is the
// exclusive prefix sum of the B lengths, so T = cu_seqlens[B] <= T_pad
// and every length is <= max_seqlen. Neither is checked here (that
// would be a device-to-host read); ops/varlen.py builds both from one
// mask. lse and the keep-mask keep the padded kernel's layout with
// S := max_seqlen, so dropout_mask_kernel is reused unchanged and the
// mask equals the padded call's for the same (seed, offset, B, NH, S).
// Rows [T, T_pad) belong to no sequence: no attention block reads or
// writes them, and zero_tail_rows_kernel sets them to zero in out /
// dqkv (every row below T is written by exactly one attention block,
// so a memset of the whole tensor would only add traffic). lse slots
// past a sequence's length are left unwritten.

// Zero rows [cu_seqlens[B], t_pad) of a [t_pad, chunks_per_row] matrix
// of 16-byte chunks. T is only known on the device, so the grid is a
// fixed size and strides over the tail (under 128 rows when T_pad comes
// from ops/varlen.py; any size is handled).
__global__ void zero_tail_rows_kernel(uint4* __restrict__ x,
                                      const int* __restrict__ cu_seqlens,
                                      int B, int64_t t_pad,
                                      int chunks_per_row) {
  const int64_t first = max(cu_seqlens[B], 0);
  const int64_t begin = first * chunks_per_row;
  const int64_t end = t_pad * chunks_per_row;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = begin + static_cast<int64_t>(blockIdx.x) * blockDim.x +
                   threadIdx.x;
       i < end; i += stride)
    x[i] = uint4{0, 0, 0, 0};
}

static void zero_tail_rows(torch::Tensor& x, const torch::Tensor& cu_seqlens,
                           hipStream_t stream) {
  // rows are 128 (out) or 384 (dqkv) bytes per head: whole 16 B chunks
  const int cpr = static_cast<int>(x.size(1) * x.element_size() / 16);
  hipLaunchKernelGGL(zero_tail_rows_kernel, dim3(128), dim3(256), 0, stream,
                     reinterpret_cast<uint4*>(x.data_ptr()),
                     cu_seqlens.data_ptr<int>(),
                     static_cast<int>(cu_seqlens.size(0)) - 1, x.size(0),
                     cpr);
}

static void check_varlen_args(const torch::Tensor& qkv,
                              const torch::Tensor& cu_seqlens,
                              int64_t max_seqlen, int64_t num_heads,
                              const char* who) {
  TORCH_CHECK(qkv.dim() == 2 && qkv.is_contiguous(), who,
              ": qkv must be a contiguous [T_pad, 3H] matrix");
  TORCH_CHECK(qkv.size(1) == 3 * num_heads * 64, who,
              ": head_dim must be 64");
  TORCH_CHECK(cu_seqlens.dim() == 1 && cu_seqlens.size(0) >= 1 &&
                  cu_seqlens.scalar_type() == torch::kInt32 &&
                  cu_seqlens.is_contiguous() &&
                  cu_seqlens.device() == qkv.device(),
              who, ": cu_seqlens must be a contiguous int32 [B+1] tensor "
                   "on qkv's device");
  TORCH_CHECK(max_seqlen >= 1, who, ": max_seqlen must be positive");
  TORCH_CHECK((cu_seqlens.size(0) - 1) * num_heads <= 65535, who,
              ": B * num_heads exceeds the grid's y limit");
}

template <typename T>
static std::vector<torch::Tensor> attention_varlen_fwd_t(
    torch::Tensor qkv, torch::Tensor cu_seqlens, int64_t max_seqlen,
    int64_t num_heads, double p, int64_t seed, int64_t offset) {
  const int64_t T_pad = qkv.size(0);
  const int B = static_cast<int>(cu_seqlens.size(0)) - 1;
  const int S = static_cast<int>(max_seqlen);
  const int NH = static_cast<int>(num_heads);
  const int H = NH * 64;
  auto out = torch::empty({T_pad, H}, qkv.options());
  auto lse = torch::empty({static_cast<int64_t>(B) * NH, S},
                          qkv.options().dtype(torch::kFloat32));
  const bool train_drop = p > 0.0;
  const int Sw = (S + 31) / 32;
  auto dmask = train_drop
                   ? torch::empty({static_cast<int64_t>(B) * NH, S, Sw},
                                  qkv.options().dtype(torch::kInt32))
                   : torch::empty({0}, qkv.options().dtype(torch::kInt32));
  auto stream = at::hip::getCurrentHIPStream();
  if (T_pad > 0) zero_tail_rows(out, cu_seqlens, stream);
  if (B == 0) return {out, lse, dmask};
  const float scale = 1.0f / sqrtf(64.f);
  dim3 grid((S + 127) / 128, B * NH), block(256);
  const size_t lds = (64 * kStride + 64 * kTrStride) * sizeof(T) +
                     4 * 64 * sizeof(float) + 128 * 2 * sizeof(uint32_t);
  if (train_drop) {
    const auto [thresh, p_q] = quantize_drop_p(p);
    const int64_t words = static_cast<int64_t>(B) * NH * S * Sw;
    hipLaunchKernelGGL(dropout_mask_kernel,
                       dim3((words + 255) / 256), dim3(256), 0, stream,
                       reinterpret_cast<uint32_t*>(dmask.data_ptr<int>()),
                       words, thresh, static_cast<uint64_t>(seed),
                       static_cast<uint64_t>(offset));
    hipLaunchKernelGGL((attn_fwd_kernel<T, true, true>), grid, block, lds,
                       stream, reinterpret_cast<const T*>(qkv.data_ptr()),
                       cu_seqlens.data_ptr<int>(),
                       reinterpret_cast<T*>(out.data_ptr()),
                       lse.data_ptr<float>(),
                       reinterpret_cast<const uint32_t*>(
                           dmask.data_ptr<int>()),
                       B, S, NH, p_q, scale,
                       static_cast<uint64_t>(seed),
                       static_cast<uint64_t>(offset));
  } else {
    hipLaunchKernelGGL((attn_fwd_kernel<T, false, true>), grid, block, lds,
                       stream, reinterpret_cast<const T*>(qkv.data_ptr()),
                       cu_seqlens.data_ptr<int>(),
                       reinterpret_cast<T*>(out.data_ptr()),
                       lse.data_ptr<float>(), nullptr, B, S, NH,
                       static_cast<float>(p), scale,
                       static_cast<uint64_t>(seed),
                       static_cast<uint64_t>(offset));
  }
  return {out, lse, dmask};
}

// qkv [T_pad,3H] bf16 or fp16, cu_seqlens [B+1] int32 ->
// {out [T_pad,H], lse fp32 [B*NH,max_seqlen], keep-mask}
std::vector<torch::Tensor> attention_varlen_fwd(
    torch::Tensor qkv, torch::Tensor cu_seqlens, int64_t max_seqlen,
    int64_t num_heads, double p, int64_t seed, int64_t offset) {
  const auto dt = qkv.scalar_type();
  TORCH_CHECK(dt == torch::kBFloat16 || dt == torch::kHalf,
              "attn_varlen_fwd: qkv must be bf16 or fp16, got ", dt);
  check_varlen_args(qkv, cu_seqlens, max_seqlen, num_heads,
                    "attn_varlen_fwd");
  if (dt == torch::kHalf)
    return attention_varlen_fwd_t<_Float16>(qkv, cu_seqlens, max_seqlen,
                                            num_heads, p, seed, offset);
  return attention_varlen_fwd_t<__bf16>(qkv, cu_seqlens, max_seqlen,
                                        num_heads, p, seed, offset);
}

template <typename T>
static torch::Tensor attention_varlen_bwd_t(
    torch::Tensor dout, torch::Tensor qkv, torch::Tensor cu_seqlens,
    int64_t max_seqlen, torch::Tensor out, torch::Tensor lse,
    torch::Tensor dmask, int64_t num_heads, double p, int64_t seed,
    int64_t offset) {
  const int B = static_cast<int>(cu_seqlens.size(0)) - 1;
  const int S = static_cast<int>(max_seqlen);
  const int NH = static_cast<int>(num_heads);
  auto dqkv = torch::empty_like(qkv);
  auto stream = at::hip::getCurrentHIPStream();
  if (qkv.size(0) > 0) zero_tail_rows(dqkv, cu_seqlens, stream);
  if (B == 0) return dqkv;
  auto fopts = qkv.options().dtype(torch::kFloat32);
  const int64_t rows = static_cast<int64_t>(B) * NH * S;
  auto delta = torch::empty({rows}, fopts);

  const int64_t delta_waves = (rows + 7) / 8;  // 8 rows per wave
  hipLaunchKernelGGL(attn_delta_varlen_kernel<T>,
                     dim3((delta_waves + 3) / 4), dim3(256), 0, stream,
                     reinterpret_cast<const T*>(dout.data_ptr()),
                     reinterpret_cast<const T*>(out.data_ptr()),
                     delta.data_ptr<float>(), cu_seqlens.data_ptr<int>(),
                     B, S, NH);

  dim3 grid((S + 127) / 128, B * NH), block(256);
  const size_t lds = (4 * 64 * kStride + 2 * 64 * kTrStride) *
                         sizeof(T) +
                     2 * 64 * sizeof(float) + 64 * 4 * sizeof(uint32_t);
  const size_t lds_dq = (64 * kStride + 64 * kTrStride) * sizeof(T) +
                        128 * 2 * sizeof(uint32_t);
  HIP_CHECK(hipFuncSetAttribute(
      reinterpret_cast<const void*>(&attn_bwd_kernel<T, true, true>),
      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  HIP_CHECK(hipFuncSetAttribute(
      reinterpret_cast<const void*>(&attn_bwd_kernel<T, false, true>),
      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const float scale = 1.0f / sqrtf(64.f);
  const bool train_drop = p > 0.0;
  const float p_q = quantize_drop_p(p).second;
  const uint32_t* mask_ptr =
      train_drop ? reinterpret_cast<const uint32_t*>(dmask.data_ptr<int>())
                 : nullptr;
  auto args = [&](auto kernel, size_t lds_bytes) {
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream,
                       reinterpret_cast<const T*>(dout.data_ptr()),
                       reinterpret_cast<const T*>(qkv.data_ptr()),
                       cu_seqlens.data_ptr<int>(), lse.data_ptr<float>(),
                       delta.data_ptr<float>(), mask_ptr,
                       reinterpret_cast<T*>(dqkv.data_ptr()), B, S, NH,
                       p_q, scale,
                       static_cast<uint64_t>(seed),
                       static_cast<uint64_t>(offset));
  };
  if (train_drop) {
    args(attn_bwd_kernel<T, true, true>, lds);
    args(attn_dq_kernel<T, true, true>, lds_dq);
  } else {
    args(attn_bwd_kernel<T, false, true>, lds);
    args(attn_dq_kernel<T, false, true>, lds_dq);
  }
  return dqkv;
}

// Packed backward -> dqkv [T_pad,3H]. All operands are checked for
// dtype, shape and contiguity before any launch.
torch::Tensor attention_varlen_bwd(torch::Tensor dout, torch::Tensor qkv,
                                   torch::Tensor cu_seqlens,
                                   int64_t max_seqlen, torch::Tensor out,
                                   torch::Tensor lse, torch::Tensor dmask,
                                   int64_t num_heads, double p,
                                   int64_t seed, int64_t offset) {
  const auto dt = qkv.scalar_type();
  TORCH_CHECK(dt == torch::kBFloat16 || dt == torch::kHalf,
              "attn_varlen_bwd: qkv must be bf16 or fp16, got ", dt);
  check_varlen_args(qkv, cu_seqlens, max_seqlen, num_heads,
                    "attn_varlen_bwd");
  TORCH_CHECK(dout.scalar_type() == dt,
              "attn_varlen_bwd: dout dtype ", dout.scalar_type(),
              " does not match qkv dtype ", dt);
  TORCH_CHECK(out.scalar_type() == dt, "attn_varlen_bwd: out dtype ",
              out.scalar_type(), " does not match qkv dtype ", dt);
  const int64_t T_pad = qkv.size(0), H = qkv.size(1) / 3;
  const int64_t bnh = (cu_seqlens.size(0) - 1) * num_heads;
  TORCH_CHECK(dout.dim() == 2 && dout.size(0) == T_pad &&
                  dout.size(1) == H && out.sizes() == dout.sizes(),
              "attn_varlen_bwd: dout and out must be [T_pad, H]");
  TORCH_CHECK(out.is_contiguous(), "attn_varlen_bwd: out not contiguous");
  TORCH_CHECK(lse.scalar_type() == torch::kFloat32 && lse.is_contiguous() &&
                  lse.numel() == bnh * max_seqlen,
              "attn_varlen_bwd: lse must be fp32 [B*NH, max_seqlen]");
  if (p > 0.0)
    TORCH_CHECK(dmask.scalar_type() == torch::kInt32 &&
                    dmask.is_contiguous() &&
                    dmask.numel() ==
                        bnh * max_seqlen * ((max_seqlen + 31) / 32),
                "attn_varlen_bwd: keep-mask does not match "
                "[B*NH, max_seqlen, ceil(max_seqlen/32)]");
  auto dout_c = dout.contiguous();
  if (dt == torch::kHalf)
    return attention_varlen_bwd_t<_Float16>(dout_c, qkv, cu_seqlens,
                                            max_seqlen, out, lse, dmask,
                                            num_heads, p, seed, offset);
  return attention_varlen_bwd_t<__bf16>(dout_c, qkv, cu_seqlens, max_seqlen,
                                        out, lse, dmask, num_heads, p, seed,
                                        offset);
}

}  // namespace bpa
