// reduce_pair.hip -- the fused bucket reduction for MPI's pair types under MAXLOC / MINLOC
// (MPI_FLOAT_INT, MPI_DOUBLE_INT, MPI_LONG_INT, MPI_2INT, MPI_SHORT_INT) and the C complex types
// under SUM / PROD (MPI_C_FLOAT_COMPLEX, MPI_C_DOUBLE_COMPLEX).  The reference is generic over
// MPI_Datatype x MPI_Op (all_reduce_radix_batch.cpp:202-204) and reduces with MPICH's
// MPI_Reduce_local (:332, :364, :446, :529), which accepts exactly these pairs for these types
// (tests/golden/pairs_manifest.json).  Element semantics: reduce_common.hpp apply<> (MPICH's loops,
// pinned by tests/golden/pairs_reduce_local.npz and nan_reduce_local.npz).  Same kernels and policy shapes as reduce_int.hip:
// an element is 8 or 16 bytes, so one 16-B vector holds two or one of them.
#include <hip/hip_runtime.h>

#include "reduce_vec.hpp"

namespace chr {

hipError_t launch_vec_pair(const VecArgs& a, int kdt, int kop, int m, hipStream_t s) {
    return launch_vec_tu<kTuPair>(a, kdt, kop, m, s);
}
hipError_t launch_scalar_pair(const ScalarArgs& a, int kdt, int kop, hipStream_t s) {
    return launch_scalar_tu<kTuPair>(a, kdt, kop, s);
}

}  // namespace chr
