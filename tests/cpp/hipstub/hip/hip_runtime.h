/* What kmernator_amd/csrc/kmr_dump.hpp, kmr_pairs.hpp, kmr_dedup.hpp and kmr_select.hpp need of the HIP runtime, for a host compiler:
 * tests/cpp/dump_line_test.cpp, tests/cpp/dedup_key_test.cpp and tests/cpp/select_record_test.cpp call the headers' device functions, and kernels whose lanes do not
 * talk to each other, as plain functions: a grid of one block of one thread, a wavefront of one lane.  Not a runtime. */
#ifndef KMR_TEST_HIP_RUNTIME_STUB_H_
#define KMR_TEST_HIP_RUNTIME_STUB_H_
#include <stddef.h>
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
template <class T> inline T __shfl_xor(T, int, int) { return T(); }    /* ... nor from any other lane: a wave sum is the lane's own value */
inline unsigned long long atomicOr(unsigned long long *p, unsigned long long v) { const unsigned long long old = *p; *p = old | v; return old; }
inline unsigned long long __brevll(unsigned long long x) { unsigned long long r = 0; for (int i = 0; i < 64; i++) r |= ((x >> i) & 1ull) << (63 - i); return r; }
template <class T> inline T __shfl_up(T, int) { return T(); }
template <class T> inline T __shfl(T v, int) { return v; }              /* lane 0 asks lane 0 */
inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { const uint32_t old = *p; *p = old + v; return old; }
inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
inline unsigned long long __ballot(int predicate) { return predicate ? 1ull : 0ull; }
inline int __ffsll(long long x) { return __builtin_ffsll(x); }
#define __builtin_amdgcn_fence(...) ((void)0)      /* one lane: nothing to order, nobody to wait for */
#define __builtin_amdgcn_wave_barrier() ((void)0)
#endif
