// reduce_tree_pair.hip -- the fused expression-tree kernel for MPI's pair types under MAXLOC /
// MINLOC and the C complex types under SUM / PROD (see reduce_pair.hip for the types and
// reduce_tree.hpp for the kernel).  The swap bits of a program pick MPICH_do_reduce's operand order
// per combine, which matters for every pair type but 2INT (order_sensitive in reduce_tree.hpp).
#include <hip/hip_runtime.h>

#include "reduce_tree.hpp"

namespace chr {

hipError_t launch_tree_pair(const TreeArgs& a, const TreeScalarArgs* sa, int kdt, int kop, hipStream_t s) {
    return launch_tree_tu<kTuTreePair>(a, sa, kdt, kop, s);
}

}  // namespace chr
