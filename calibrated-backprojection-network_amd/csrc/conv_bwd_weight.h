// conv_bwd_weight.h -- the one weight-gradient family of the trainable networks' convs (conv_bwd_weight.hip: the kernel
// conv_bwd_weight_kernel<KS, STRIDE, MB>, its split plan and the launch that adds the split planes), as the two extern "C" pairs
// call it:
//   kbn_conv2d_s2_backward_weight   posenet_backward.hip         k in {3, 5, 7} at stride 2
//   kbn_conv2d_backward_weight      conv_affine_backward.hip     (3, 1), (1, 1), (1, 2)
// Each entry point keeps its own case check and hands the verdict in: the argument checks that precede it stay in front of it.
#pragma once

#include "pose_igemm.h"

namespace kbn {

// The weight gradient of conv_{k x k, stride, padding k / 2}(cat(srcs)) for (k, stride) in {(3, 1), (1, 1), (1, 2), (3, 2), (5, 2),
// (7, 2)}: argument checks, `case_ok` (false: KBN_ERR_UNSUPPORTED), the sources, the plan, the scratch size, the launch, the split sum.
int conv_bwd_weight(bool case_ok, const kbn_conv_src* srcs, int n_src, const float* grad_out, long long grad_out_batch_stride,
                    float* grad_weight, int n, int out_channels, int kernel_size, int stride, int in_height, int in_width, int splits,
                    float* scratch, size_t scratch_bytes, hipStream_t stream);

// Bytes of `scratch` the call above needs at these arguments: 0 for one split or a shape the plan refuses
size_t conv_bwd_weight_scratch_bytes(int n, int out_channels, int in_channels, int kernel_size, int stride, int in_height, int in_width,
                                     int splits);

}  // namespace kbn
