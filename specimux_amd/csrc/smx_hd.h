// smx_hd.h -- SMX_HD: the qualifier of the small functions that the kernels, the host code and the CPU simulations
// (tests/cpu, plain g++) share.
#ifndef SMX_HD_H
#define SMX_HD_H

#if defined(__HIPCC__)
#define SMX_HD __host__ __device__ __forceinline__
#else
#define SMX_HD inline
#endif

#endif
