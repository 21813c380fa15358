// Instances of K34's kernel (made_rqs_wide_kernel.hpp; entry point in made_rqs_wide.hip) for 2 .. 5 bins (one 32-row tile
// per pair of features) and 12 .. 16 bins (three): a translation unit of their own, as rqs_resnet_wide_bins_*.hip are for
// K32, so that the two compile side by side.
#include "made_rqs_wide_kernel.hpp"

namespace nfa {
namespace k34 {

#define NFA_K34_CASE(K) case K: return made_rqs_wide_kernel<K>
MadeWideKernelFn made_wide_bins_low(int K) {
    switch (K) {
        NFA_K34_CASE(2);
        NFA_K34_CASE(3);
        NFA_K34_CASE(4);
        NFA_K34_CASE(5);
        NFA_K34_CASE(12);
        NFA_K34_CASE(13);
        NFA_K34_CASE(14);
        NFA_K34_CASE(15);
        NFA_K34_CASE(16);
    }
    return nullptr;
}

}  // namespace k34
}  // namespace nfa
