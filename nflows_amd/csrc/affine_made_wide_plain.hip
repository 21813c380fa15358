// The instance of K36's kernel (affine_made_wide_kernel.hpp; entry point in affine_made_wide.hip) without a context: a
// translation unit of its own, as made_rqs_wide_bins_*.hip are for K34, so that the two instances compile side by side.
#include "affine_made_wide_kernel.hpp"

namespace nfa {
namespace k36 {

AffineWideKernelFn affine_wide_plain() { return affine_made_wide_kernel<false>; }

}  // namespace k36
}  // namespace nfa
