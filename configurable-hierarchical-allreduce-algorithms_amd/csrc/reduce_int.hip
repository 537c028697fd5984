// reduce_int.hip -- the fused bucket reduction for the MPI integer types beyond int32
// arithmetic: (u)int8/16/64 and uint32, the logical (LAND/LOR/LXOR) and bitwise (BAND/BOR/BXOR)
// ops on every integer type, and the logical ops on float/double (MPICH accepts them).  The
// reference is generic over MPI_Datatype and MPI_Op (all_reduce_radix_batch.cpp:202-204,
// MPI_Type_size at :234-277); its arithmetic is
// MPICH's MPI_Reduce_local loop for the pair.  Same kernels as reduce_kernels.hip (reduce_vec.hpp),
// compiled here in the two policy shapes only, so this translation unit builds in parallel with
// the floating-point one.  Kernel types come from canon_op: signedness only matters to MAX/MIN,
// everything else runs on the unsigned type of the width (int32's kernels for 32-bit).
#include <hip/hip_runtime.h>

#include "reduce_vec.hpp"

namespace chr {

hipError_t launch_vec_int(const VecArgs& a, int kdt, int kop, int m, hipStream_t s) {
    return launch_vec_tu<kTuInt>(a, kdt, kop, m, s);
}
hipError_t launch_scalar_int(const ScalarArgs& a, int kdt, int kop, hipStream_t s) {
    return launch_scalar_tu<kTuInt>(a, kdt, kop, s);
}

}  // namespace chr
