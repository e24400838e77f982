// smx_align.hip -- the alignment kernels behind smx_align and smx_align_batch (smx_calls.cpp): the demux kernel's column
// step (smx_align_core.h) on targets of any length, one lane per alignment.  The lane's work is smx_align_lane.h, which the
// CPU twin compiles too.
#include <hip/hip_runtime.h>
#include "smx_internal.h"
#include "smx_align_lane.h"

namespace smx {

// Single alignment (smx_align): one lane, arbitrary target length.
__global__ void align_kernel(const unsigned long long *peq, const unsigned long long *rpeq, int m,
                             const unsigned char *tcodes, int n, int k, int mode, int *out_dist,
                             unsigned char *endflag, int *starts) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    align_lane(peq, rpeq, m, tcodes, n, k, mode, out_dist, endflag, starts);
}

// Many alignments per launch (smx_align_batch): one lane per alignment.
__global__ __launch_bounds__(64) void align_batch_kernel(const unsigned long long *__restrict__ q_peq, const int *__restrict__ q_len,
                                                        const unsigned *__restrict__ qidx, const unsigned char *__restrict__ tcodes,
                                                        const unsigned long long *__restrict__ toff, const int *__restrict__ kk,
                                                        const unsigned char *__restrict__ modes, unsigned n, unsigned char *ws,
                                                        int *__restrict__ out_dist, int *__restrict__ out_nloc,
                                                        int *__restrict__ out_starts, int *__restrict__ out_ends, unsigned cap) {
    const unsigned i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    align_batch_lane(i, q_peq, q_len, qidx, tcodes, toff, kk, modes, ws, out_dist, out_nloc, out_starts, out_ends, cap);
}

}  // namespace smx

extern "C" int smx_launch_align(void *stream, const unsigned long long *d_peq, const unsigned long long *d_rpeq, int m,
                                const unsigned char *d_tcodes, int n, int k, int mode, int *d_dist,
                                unsigned char *d_endflag, int *d_starts) {
    hipLaunchKernelGGL(smx::align_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_peq, d_rpeq, m, d_tcodes, n, k,
                       mode, d_dist, d_endflag, d_starts);
    return (int)hipGetLastError();
}

extern "C" int smx_launch_align_batch(void *stream, const unsigned long long *d_qpeq, const int *d_qlen, const unsigned *d_qidx,
                                      const unsigned char *d_tcodes, const unsigned long long *d_toff, const int *d_k,
                                      const unsigned char *d_modes, unsigned n, unsigned char *d_ws, int *d_dist, int *d_nloc,
                                      int *d_starts, int *d_ends, unsigned cap) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(smx::align_batch_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, d_qpeq, d_qlen, d_qidx,
                       d_tcodes, d_toff, d_k, d_modes, n, d_ws, d_dist, d_nloc, d_starts, d_ends, cap);
    return (int)hipGetLastError();
}
