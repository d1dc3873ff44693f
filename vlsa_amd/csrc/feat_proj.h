// Shared between feat_proj.hip (the packer and the forward) and mlp_backward.hip (the projecter's backward): the layout of the
// prepared Feat_Projecter block (see vlsa_prepare_featproj) and the constants it is made of.
#pragma once
#include "bag_table.h"

namespace vlsa {

namespace fp {
constexpr int kD = 512;                           // input and output width
constexpr int kSteps = 16;                        // K steps of 32
constexpr int kNF = 8;                            // weight fragments per step and wave: 4 column tiles x (hi, lo)
}  // namespace fp

struct FeatProjLayout {
    size_t wpack, bias, gamma, beta, total;
    __host__ __device__ FeatProjLayout() {
        wpack = 0;
        bias = wpack + (size_t)8 * fp::kSteps * fp::kNF * 1024;   // 1 MiB
        gamma = bias + fp::kD * 4;
        beta = gamma + fp::kD * 4;
        total = beta + fp::kD * 4;
    }
};

}  // namespace vlsa
