// The k-loop of the TN MFMA GEMMs: C[128,128] += a[k, m0:m0+128]^T @
// b[k, n0:n0+128] over k in [kz0, kz1), both operands row-major 16-bit
// with k as the row index. Shared by the weight-gradient kernel
// (csrc/ops/wgrad.hip: a = dy, b = x) and the K-FAC factor kernel
// (csrc/ops/kfac_factor.hip: a = b = x); the structure is described at
// the top of wgrad.hip.
//
// Block contract: 256 threads = 4 waves as 2x2, each wave owns a 64x64
// quarter of the tile as acc[4][4] 16x16 MFMA accumulators (C/D layout
// of csrc/mfma_frag.h); lds holds 4 * BK * kStride elements (two
// double-buffered [BK][kStride] images per operand) and must be
// 16-byte aligned.
#pragma once

#include "../mfma_frag.h"

namespace bpa {

namespace wg {

constexpr int kBM = 128;   // C tile rows (M)
constexpr int kBN = 128;   // C tile cols (N)
constexpr int kBK = 32;    // K step (32-deep: 36.8 KB LDS -> 4 blocks/CU)
constexpr int kStride = 144;  // LDS row stride (elems), tr-conflict-free

}  // namespace wg

// a [K, lda], b [K, ldb]; the caller guarantees m0 + 128 <= lda,
// n0 + 128 <= ldb and kz0 < kz1 <= K. BK = 32 or 64.
template <typename T, int BK>
__device__ __forceinline__ void tn_mainloop(const T* __restrict__ a, int lda,
                                            int m0, const T* __restrict__ b,
                                            int ldb, int n0, int K, int kz0,
                                            int kz1, T* lds,
                                            f32x4 (&acc)[4][4]) {
  using Tr = Mfma16<T>;
  using F8 = typename Tr::frag;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1;  // 2x2 wave grid, 64x64 each

  constexpr int kTile = BK * wg::kStride;
  constexpr int kTPR = 256 / BK;      // staging threads per k-row
  constexpr int kSlots = BK / 16;     // uint4 slots per thread per matrix

  // staging map: thread -> (row r, kSlots 8-elem slots 8*kTPR apart);
  // at BK=32 each ds_write_b128's 8-lane group covers one 128-B row
  // (conflict-free); at BK=64 it covers two half-rows (2-way on half
  // the banks - measured cheaper than the extra barriers it replaces)
  const int st_r = tid / kTPR;
  const int st_c = (tid % kTPR) * 8;

  // Prefetch loads are UNCONDITIONAL with the row clamped to the last
  // valid one (a conditional load/zero branch inside the loop-carried
  // lambda segfaults hipcc/ROCm 7.2's gfx950 optimizer at -O2/-O3);
  // rows past the slice end are zeroed at LDS-write time instead.
  uint4 pf_a[kSlots], pf_b[kSlots];
  auto issue_loads = [&](int k0) {
    const int krow = min(k0 + st_r, K - 1);  // clamp: always legal memory
    const uint4* as = reinterpret_cast<const uint4*>(
        a + static_cast<int64_t>(krow) * lda + m0 + st_c);
    const uint4* bs = reinterpret_cast<const uint4*>(
        b + static_cast<int64_t>(krow) * ldb + n0 + st_c);
#pragma unroll
    for (int q = 0; q < kSlots; ++q) {
      pf_a[q] = as[q * kTPR];
      pf_b[q] = bs[q * kTPR];
    }
  };

  issue_loads(kz0);

  int buf = 0;
  for (int k0 = kz0; k0 < kz1; k0 += BK) {
    // write the in-flight k-step into buf (T14 write-late); zero rows
    // past the slice end so the clamped prefetch cannot contaminate
    if (k0 + st_r >= kz1) {
#pragma unroll
      for (int q = 0; q < kSlots; ++q) pf_a[q] = pf_b[q] = uint4{0, 0, 0, 0};
    }
    const int boff = buf * 2 * kTile;
#pragma unroll
    for (int q = 0; q < kSlots; ++q) {
      *reinterpret_cast<uint4*>(
          &lds[boff + st_r * wg::kStride + st_c + 8 * kTPR * q]) = pf_a[q];
      *reinterpret_cast<uint4*>(
          &lds[boff + kTile + st_r * wg::kStride + st_c + 8 * kTPR * q]) =
          pf_b[q];
    }
    __syncthreads();
    issue_loads(k0 + BK < kz1 ? k0 + BK : k0);  // T14 issue-early

    const T* at = lds + boff;
    const T* bt = lds + boff + kTile;
#pragma unroll
    for (int kd = 0; kd < BK / 32; ++kd) {
      F8 af[4], bfr[4];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        af[t] = frag_tr<wg::kStride>(at, kd * 32, wi * 64 + t * 16);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        bfr[t] = frag_tr<wg::kStride>(bt, kd * 32, wj * 64 + t * 16);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
          acc[ti][tj] = Tr::mfma(af[ti], bfr[tj], acc[ti][tj]);
      __builtin_amdgcn_s_setprio(0);
    }
    // no trailing barrier: the next iteration writes the OTHER buffer,
    // whose last readers finished before this iteration's barrier
    buf ^= 1;
  }
}

}  // namespace bpa
