// Pillow-exact 8-bit bicubic resize of packed RGB images to one or two target sizes, with the /255 and ImageNet normalisation of
// the matcher's host path: see preprocess.hip and roma_op_preprocess in include/roma_hip.h.
#pragma once
#include "common.h"

namespace roma {
// bytes of workspace for a batch; -1 (with the error text set) for a batch that roma_op_preprocess would refuse
long preprocess_workspace_bytes(const long long* desc_host, int n_images, const int* targets_hw, int n_targets);
int preprocess_launch(const unsigned char* src, long long src_bytes, const long long* desc_host, const long long* desc_dev,
                      int n_images, const int* targets_hw, int n_targets, int normalize, float* out0, float* out1, void* workspace,
                      hipStream_t s);
}  // namespace roma
