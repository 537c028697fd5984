// reduce_tree_int_wide.hip -- the fused expression-tree kernels for the 32- and 64-bit kernel types beyond the
// core arithmetic: uint32 / int64 / uint64, the logical and bitwise ops on int32 and the logical ops on float /
// double (kTuTreeIntWide in kernel_table.hpp; see reduce_int.hip for the type mapping and reduce_tree.hpp for the
// kernel).  The 8- and 16-bit half is reduce_tree_int_narrow.hip, so the two build in parallel.
#include <hip/hip_runtime.h>

#include "reduce_tree.hpp"

namespace chr {

hipError_t launch_tree_int_wide(const TreeArgs& a, const TreeScalarArgs* sa, int kdt, int kop, hipStream_t s) {
    return launch_tree_tu<kTuTreeIntWide>(a, sa, kdt, kop, s);
}

}  // namespace chr
