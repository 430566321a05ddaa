// residual_loss.hip -- mo_residual_loss_eval: the robust loss of every residual block of a layout.
//   residual_loss_kernel   per block b: s_b = |r_b|^2, w_b = rho_b'(s_b) repeated over the block's rows; per problem 0.5 sum_b rho_b(s_b)
// A workgroup per problem in turn, a lane per block: the hand-out, the order of every sum and the arithmetic are those of the fused robust
// linearise (blocks_linearize_kernel<.., kL>), both through mo_loss_device.h -- the two routes give the same bits.
#include "mo_loss_device.h"

namespace mo {
namespace {

template <typename T>
__global__ __launch_bounds__(kThreads) void residual_loss_kernel(const LossArgs a) {
  __shared__ T red[kThreads / 64];
  const int tid = threadIdx.x;
  for (long long p = blockIdx.x; p < a.batch; p += gridDim.x) {
    const T* r = (const T*)a.r + p * a.r_stride;
    T* w = a.weights_out ? (T*)a.weights_out + p * a.weights_stride : nullptr;
    T part = loss_blocks<T>(a.blk, (const T*)a.scale, a.num_blocks, r, w, nullptr, tid);
    if (a.rho_out) {
      part = loss_rho_sum(part, red);
      if (tid == 0) ((T*)a.rho_out)[p * a.rho_stride] = (T)0.5 * part;
      __syncthreads();  // the next problem overwrites the reduction slots
    }
  }
}

}  // namespace

hipError_t launch_residual_loss(const LossArgs& a, int dtype, int num_cus, hipStream_t stream) {
  if (a.batch <= 0) return hipSuccess;
  const dim3 g(grid_for(a.batch, num_cus, 0)), b(kThreads);
  if (dtype == MO_F64) hipLaunchKernelGGL(residual_loss_kernel<double>, g, b, 0, stream, a);
  else hipLaunchKernelGGL(residual_loss_kernel<float>, g, b, 0, stream, a);
  return hipGetLastError();
}

}  // namespace mo
