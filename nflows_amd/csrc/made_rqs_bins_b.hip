// Instances of K29's kernel (made_rqs_kernel.hpp; entry point in made_rqs.hip) for 6 .. 11 bins (two 32-row tiles per pair of features): a translation unit of
// their own, as rqs_resnet_bins.hip is for K8, so that the three compile side by side.
#include "made_rqs_kernel.hpp"

namespace nfa {

MadeRqsKernelFn made_rqs_bins_mid(int K) {
    switch (K) {
        case 6: return made_rqs_kernel<6>;
        case 7: return made_rqs_kernel<7>;
        case 8: return made_rqs_kernel<8>;
        case 9: return made_rqs_kernel<9>;
        case 10: return made_rqs_kernel<10>;
        case 11: return made_rqs_kernel<11>;
    }
    return nullptr;
}

}  // namespace nfa
