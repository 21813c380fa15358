// Instances of K34's kernel (made_rqs_wide_kernel.hpp; entry point in made_rqs_wide.hip) for 6 .. 11 bins (two 32-row
// tiles per pair of features): a translation unit of their own, beside made_rqs_wide_bins_a.hip.
#include "made_rqs_wide_kernel.hpp"

namespace nfa {
namespace k34 {

#define NFA_K34_CASE(K) case K: return made_rqs_wide_kernel<K>
MadeWideKernelFn made_wide_bins_mid(int K) {
    switch (K) {
        NFA_K34_CASE(6);
        NFA_K34_CASE(7);
        NFA_K34_CASE(8);
        NFA_K34_CASE(9);
        NFA_K34_CASE(10);
        NFA_K34_CASE(11);
    }
    return nullptr;
}

}  // namespace k34
}  // namespace nfa
