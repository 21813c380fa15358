// Instances of K32's kernel (rqs_resnet_wide_kernel.hpp; entry point in rqs_resnet_wide.hip) for 2 .. 5 bins (one 32-row
// tile per pair of features) and 12 .. 16 bins (three): a translation unit of their own, as made_rqs_bins_*.hip are for
// K29, so that the two compile side by side.
#include "rqs_resnet_wide_kernel.hpp"

namespace nfa {
namespace k32 {

#define NFA_K32_CASE(K) case K: return inverse ? rqs_resnet_wide_kernel<true, K> : rqs_resnet_wide_kernel<false, K>
WideKernelFn wide_bins_low(int K, bool inverse) {
    switch (K) {
        NFA_K32_CASE(2);
        NFA_K32_CASE(3);
        NFA_K32_CASE(4);
        NFA_K32_CASE(5);
        NFA_K32_CASE(12);
        NFA_K32_CASE(13);
        NFA_K32_CASE(14);
        NFA_K32_CASE(15);
        NFA_K32_CASE(16);
    }
    return nullptr;
}

}  // namespace k32
}  // namespace nfa
