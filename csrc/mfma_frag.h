// A/B fragment builders for the gfx950 16x16x32 MFMA kernels (attention,
// wgrad; the MLM head addresses a swizzled image and keeps its own
// frag_k).
//
// Fragment convention (consistent A/B slot mapping):
//   A[i][k]/B[k][j]: i|j = lane&15, k = (lane>>4)*4 + (e&3) + 16*(e>>2)
//   C/D[i][j]:       j = lane&15,   i = (lane>>4)*4 + reg
// Only A/B consistency matters for correctness (the contraction is
// permutation-invariant when both sides agree); C/D is the documented
// gfx950 layout.
#pragma once

#include "mfma_types.h"

namespace bpa {

// One 8-element fragment seen as the MFMA operand, as its 16-bit
// elements, as two 8-byte chunks, or as the two halves the transpose
// read returns.
template <typename T>
union FragBits {
  typename Mfma16<T>::frag v;
  T e[8];
  uint2 u[2];
  typename Mfma16<T>::tr4 h[2];
};

// Build an A/B fragment from a row-major 16-bit row pointer: elements at
// k = base + g*4 + (e&3) + 16*(e>>2), loaded as two 8-byte chunks.
template <typename T>
__device__ __forceinline__ typename Mfma16<T>::frag frag_row(const T* row,
                                                             int base,
                                                             int g) {
  FragBits<T> r;
  r.u[0] = *reinterpret_cast<const uint2*>(row + base + g * 4);
  r.u[1] = *reinterpret_cast<const uint2*>(row + base + 16 + g * 4);
  return r.v;
}

// Transposed A/B fragment via gfx950's hardware transpose read
// (ds_read_b64_tr_b16), straight from a NATURAL row-major
// [rows][STRIDE] 16-bit LDS image: element
// e = img[rb + g*4 + (e&3) + 16*(e>>2)][cb + li] - the fragment a
// separately built transposed image would give a row read. Semantics
// verified on hardware by tr16_probe (csrc/ops/mfma_probe.hip,
// tests/test_gpu_mfma_probe.py): within each 16-lane group,
// out[lane i][j] = mem[addr_of_lane(4j + (i>>2)) + (i&3)], so lane
// (g, t) points at 4 contiguous elements of row rb + g*4 + (t>>2) and
// the instruction delivers the group-transposed fragment. No transposed
// image and no per-thread 16x ds_write_b16 scatter at staging time.
// STRIDE decides the bank behaviour: stride_dw = 8 mod 16 (80 or 144
// elements) is conflict-free.
template <int STRIDE, typename T>
__device__ __forceinline__ typename Mfma16<T>::frag frag_tr(const T* img,
                                                            int rb, int cb) {
  using Tr = Mfma16<T>;
  const int lane = threadIdx.x & 63;
  const int g = (lane >> 4) & 3, t = lane & 15;
  const T* p0 =
      img + (rb + g * 4 + (t >> 2)) * STRIDE + cb + (t & 3) * 4;
  FragBits<T> r;
  r.h[0] = Tr::tr_read(p0);
  r.h[1] = Tr::tr_read(p0 + 16 * STRIDE);
  return r.v;
}

}  // namespace bpa
