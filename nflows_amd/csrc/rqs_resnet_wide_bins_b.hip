// Instances of K32's kernel (rqs_resnet_wide_kernel.hpp; entry point in rqs_resnet_wide.hip) for 6 .. 11 bins (two 32-row
// tiles per pair of features): a translation unit of their own, beside rqs_resnet_wide_bins_a.hip.
#include "rqs_resnet_wide_kernel.hpp"

namespace nfa {
namespace k32 {

#define NFA_K32_CASE(K) case K: return inverse ? rqs_resnet_wide_kernel<true, K> : rqs_resnet_wide_kernel<false, K>
WideKernelFn wide_bins_mid(int K, bool inverse) {
    switch (K) {
        NFA_K32_CASE(6);
        NFA_K32_CASE(7);
        NFA_K32_CASE(8);
        NFA_K32_CASE(9);
        NFA_K32_CASE(10);
        NFA_K32_CASE(11);
    }
    return nullptr;
}

}  // namespace k32
}  // namespace nfa
