// reduce_tree_int_narrow.hip -- the fused expression-tree kernels for the 8- and 16-bit integer kernel types
// (kTuTreeIntNarrow in kernel_table.hpp); the other half of the integer trees is reduce_tree_int_wide.hip.
#include <hip/hip_runtime.h>

#include "reduce_tree.hpp"

namespace chr {

hipError_t launch_tree_int_narrow(const TreeArgs& a, const TreeScalarArgs* sa, int kdt, int kop, hipStream_t s) {
    return launch_tree_tu<kTuTreeIntNarrow>(a, sa, kdt, kop, s);
}

}  // namespace chr
