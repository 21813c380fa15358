// K37's instances for the MLP form of the conditioner (kernel: affine_resnet_wide_kernel.hpp; entry point and the
// ResidualNet form: affine_resnet_wide.hip) -- a translation unit of their own so that the two forms compile side by side.

#include "affine_resnet_wide_kernel.hpp"

using namespace nfa::k37;

AffineWideKernelFn nfa::k37::affine_wide_mlp(bool inverse, bool additive) {
    return inverse ? (additive ? affine_resnet_wide_kernel<true, true, false> : affine_resnet_wide_kernel<true, false, false>)
                   : (additive ? affine_resnet_wide_kernel<false, true, false> : affine_resnet_wide_kernel<false, false, false>);
}
