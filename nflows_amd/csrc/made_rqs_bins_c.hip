// Instances of K29's kernel (made_rqs_kernel.hpp; entry point in made_rqs.hip) for 12 .. 16 bins (three 32-row tiles per pair of features): a translation unit of
// their own, as rqs_resnet_bins.hip is for K8, so that the three compile side by side.
#include "made_rqs_kernel.hpp"

namespace nfa {

MadeRqsKernelFn made_rqs_bins_high(int K) {
    switch (K) {
        case 12: return made_rqs_kernel<12>;
        case 13: return made_rqs_kernel<13>;
        case 14: return made_rqs_kernel<14>;
        case 15: return made_rqs_kernel<15>;
        case 16: return made_rqs_kernel<16>;
    }
    return nullptr;
}

}  // namespace nfa
