// ds_read_b64_tr_b16 semantics probe: verifies the lane->element mapping
// that every frag_tr user (csrc/mfma_frag.h: attention PV/dQ/dK/dV,
// wgrad) relies on. tests/test_gpu_mfma_probe.py checks all four address
// modes against the documented rule, so a ROCm or hardware change that
// moved the mapping fails the suite instead of the kernels' numerics.
//
// LDS is filled with the identity pattern (element i = i) and each lane
// reads at the element offset its addr_mode gives it; out[l][j] then IS
// the element index lane l's slot j received. The rule: within each
// 16-lane group, out[lane i][j] = mem[addr_of_lane(4j + (i>>2)) + (i&3)]
// (lane numbers relative to the group).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../ops.h"

namespace bpa {

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

// one wave, one launch -> [64 lanes, 4 slots] fp32 element indices
torch::Tensor tr16_probe(int64_t addr_mode) {
  auto out = torch::empty({64, 4}, torch::TensorOptions()
                                       .dtype(torch::kFloat32)
                                       .device(torch::kCUDA));
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(tr16_probe_kernel, dim3(1), dim3(64), 0, stream,
                     out.data_ptr<float>(), static_cast<int>(addr_mode));
  return out;
}

}  // namespace bpa
