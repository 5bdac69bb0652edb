// hopsx: geometry of the flagship MNIST CNN that the training kernel (mnist_persist.hip) and the evaluation
// kernel (mnist_eval.hip) must agree on.  Each kernel keeps its own LDS map, tile sizes and Args.
#pragma once

namespace mnist_cnn {

constexpr int C1 = 32, C2 = 64, HID = 128, NCLS = 10;
constexpr int PH = 13, NPOS = PH * PH;  // pooled positions
constexpr int KIN = NPOS * C2;          // 10816 fc1 inputs (NHWC flatten: (ph*13 + pw)*64 + c)

// LDS row strides (bf16 elements) of the images both kernels read MFMA fragments from.  The rule: the row's
// K extent padded by 16 B (8 elements) against bank conflicts of the fragment reads; rows stay 16-B aligned.
constexpr int row_stride(int k) { return k + 8; }
constexpr int W1S = row_stride(C2);      // 72:  fc1 slice of one position, [128 n][64 c]
constexpr int W2S = row_stride(4 * C1);  // 136: conv2 weights, [64 co][4 taps x 32 ci] (OHWI rows)
constexpr int C1S = row_stride(C1);      // 40:  conv1 output, [32 b][9 pos][32 ci]
constexpr int PLS = row_stride(C2);      // 72:  pooled, [32 b][64 c]
static_assert(W1S == 72 && W2S == 136 && C1S == 40 && PLS == 72, "strides the kernels were tuned with");

}  // namespace mnist_cnn
