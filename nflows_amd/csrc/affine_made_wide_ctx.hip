// The instance of K36's kernel (affine_made_wide_kernel.hpp; entry point in affine_made_wide.hip) with MADE's context terms:
// a translation unit of its own, so that the two instances compile side by side.
#include "affine_made_wide_kernel.hpp"

namespace nfa {
namespace k36 {

AffineWideKernelFn affine_wide_context() { return affine_made_wide_kernel<true>; }

}  // namespace k36
}  // namespace nfa
