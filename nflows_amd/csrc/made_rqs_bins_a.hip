// Instances of K29's kernel (made_rqs_kernel.hpp; entry point in made_rqs.hip) for 2 .. 5 bins (one 32-row tile per pair of features): a translation unit of
// their own, as rqs_resnet_bins.hip is for K8, so that the three compile side by side.
#include "made_rqs_kernel.hpp"

namespace nfa {

MadeRqsKernelFn made_rqs_bins_low(int K) {
    switch (K) {
        case 2: return made_rqs_kernel<2>;
        case 3: return made_rqs_kernel<3>;
        case 4: return made_rqs_kernel<4>;
        case 5: return made_rqs_kernel<5>;
    }
    return nullptr;
}

}  // namespace nfa
