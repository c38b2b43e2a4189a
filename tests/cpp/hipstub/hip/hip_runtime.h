/* What kmernator_amd/csrc/kmr_dump.hpp needs of the HIP runtime, for a host compiler: tests/cpp/dump_line_test.cpp calls the
 * header's device functions as plain functions, one "lane" at a time.  Not a runtime: the kernels compile and are never launched. */
#ifndef KMR_TEST_HIP_RUNTIME_STUB_H_
#define KMR_TEST_HIP_RUNTIME_STUB_H_
#include <stdint.h>

#define __device__
#define __global__
#define __shared__ static
#define __forceinline__ inline
#define __launch_bounds__(...)

struct stub_dim3 { unsigned x, y, z; };
static const stub_dim3 threadIdx = {0, 0, 0}, blockIdx = {0, 0, 0}, blockDim = {1, 1, 1}, gridDim = {1, 1, 1};
struct uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { uint4 v = {x, y, z, w}; return v; }
inline void __syncthreads() {}
inline uint32_t atomicOr(uint32_t *p, uint32_t v) { const uint32_t old = *p; *p = old | v; return old; }
inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) { const unsigned long long old = *p; *p = old + v; return old; }
template <class T> inline T __shfl_down(T, int) { return T(); }      /* a wavefront of one lane: nothing comes from the lanes above */
#endif
