/*
 * kmr_compare.hpp -- HIP kernels (gfx950) of CompareSpectrums (apps/CompareSpectrums.cpp): how many distinct k-mers and how many
 * k-mer occurrences two read sets share, set against set (countCommonKmers :146-162, evaluate :225-242) or every sequence of
 * set 1 on its own against the whole of set 2 (evaluatePerRead :243-257, which rebuilds a KmerSpectrum per read).
 *
 * Every figure is an integer sum, so no order matters.  A map is what KmerSpectrum::getCount(kmer, false) answers from
 * (src/KmerSpectrum.h:642-695): the weak entries with their u16 count and the singleton entries with count 1.
 *
 *  Whole form   compare_totals_kernel   size and count sum of a map, and its entries of count 65535
 *               compare_maps_kernel     strides over map 1's entries, map_find in map 2 (weak, then singleton); sums per
 *                                       wavefront, then one 64-bit atomic per wavefront and field
 *  Per read     CompareOp               extract_kernel's Op: the canonical key of every k-mer that passes the build's weight
 *                                       test (TrackingData::isDiscard) to slot koff[read] + position of a staging array that
 *                                       was filled with the all-ones key, which no canonical k-mer equals
 *               compare_reads_lds_kernel  reads of at most `cap` k-mers: one wavefront per read, the read's slots in LDS,
 *                                       distinct keys and multiplicities by comparing every key with every other, one lookup per
 *                                       distinct key, the record reduced across the wavefront; no atomics, nothing but the
 *                                       record leaves the CU
 *               compare_long_*_kernel   longer reads (contigs, genomes): (read, key) ordered by sort_by_columns (kmr_sort.hip),
 *                                       one pass per key word and one for the read, heads flagged, one lookup per head
 *                                       added into the read's record (one atomic per wavefront and field while a wavefront's
 *                                       heads belong to one read)
 *
 * LDS of compare_reads_lds_kernel: CMP_WAVES * cap * W * 8 bytes per block.  At the default cap of 256 that is 8 KiB (W = 1) to
 * 32 KiB (W = 4) per 4-wave block: of the 160 KiB of a CU, five blocks (20 wavefronts) at W = 4 and the full 32 wavefronts at
 * W <= 2.  The keys live in LDS only: a lane holds its own key in W registers and reads the others by broadcast.
 */
#ifndef KMR_COMPARE_HPP_
#define KMR_COMPARE_HPP_

#include "kmr_kernels.hpp"

namespace kmr {

/* kmr_compare_counts as the kernels add into it */
struct CompareRec { unsigned long long size1, size2, common, common_count1, common_count2, total_count1, total_count2, saturated; };
/* what compare_totals_kernel leaves of a map */
enum { CMP_T_SIZE = 0, CMP_T_TOTAL = 1, CMP_T_SATURATED = 2, CMP_T_WORDS = 3 };

static const int CMP_WAVES = 4;
static const uint32_t CMP_CAP = 256, CMP_CAP_MOST = 512;       /* k-mers of a read the LDS kernel takes (kmr_tune "compare_lds_kmers") */
static const uint64_t CMP_STAGE_SLOTS = 1ull << 26;            /* staging slots of one run (kmr_tune "compare_stage_kmers") */
static const uint32_t CMP_COUNT_MAX = 65535u;                  /* where a stored count stops */

template <int W> struct CompareOp {
	uint64_t *stage;               /* [slots of the run][W], all ones before the launch */
	const uint64_t *koff;          /* per read of the batch: its first slot */
	uint64_t slot_base;            /* koff of the run's first read */
	static const bool NEEDS_WEIGHT = true;      /* the build's own weight test decides which k-mers a read's map holds */
	static const bool COUNTS_STATS = false;
	static const bool NEEDS_HASH = false;
	struct State {};
	__device__ __forceinline__ void wave_begin(State &, int) const {}
	__device__ __forceinline__ void wave_end(State &, int) const {}
	__device__ __forceinline__ void tile_begin(State &, uint32_t *, uint64_t, int) const {}
	__device__ __forceinline__ void tile_end(State &, uint64_t, int) const {}
	__device__ __forceinline__ void emit(State &, bool valid, const DevParams &, const Key<W> &key, uint64_t, const Occurrence &,
	                                     uint64_t readIdx, uint32_t pos, unsigned &, bool &) const {
		if (valid) {
			uint64_t *d = stage + (koff[readIdx] - slot_base + pos) * W;
#pragma unroll
			for (int i = 0; i < W; i++) d[i] = key.w[i];
		}
	}
};
template <int W> __device__ __forceinline__ bool op_keeps_all_owners(const CompareOp<W> &) { return true; }
template <int W> __device__ __forceinline__ uint32_t op_fail_code(const CompareOp<W> &) { return 0; }

template <int W> __device__ __forceinline__ bool cmp_is_sentinel(const Key<W> &key) {
	bool s = true;
#pragma unroll
	for (int i = 0; i < W; i++) s = s && key.w[i] == ~0ull;
	return s;
}
/* getCount(kmer, false) of map 2 and whether the map holds the key at all */
template <int W> __device__ __forceinline__ bool cmp_lookup(const MapView<W> &weak, const MapView<W> &sing, const Key<W> &key, uint32_t kb, uint32_t &c2) {
	const uint64_t hash = key_hash<W>(key, kb);
	int64_t e = map_find<W>(weak, key, hash);
	if (e >= 0) { c2 = weak.vals[(uint64_t)e * weak.vw] & 0xffffu; return true; }
	e = map_find<W>(sing, key, hash);
	if (e >= 0) { c2 = sing.sweight[e] == 0 ? 0u : 1u; return true; }
	c2 = 0;
	return false;
}

#ifndef KMR_INSTANCE_TU
/* k-mers per read, max(L - k + 1, 0), and the most of any read */
__global__ void compare_nk_kernel(const uint64_t *offsets, uint64_t n, uint32_t k, uint32_t *nk, unsigned int *most, uint32_t *err) {
	unsigned int mx = 0;
	for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t L = offsets[r + 1] - offsets[r];
		const uint64_t c = L >= k ? L - k + 1 : 0;
		if (c > 0xffffffffull) { atomicOr(err, 1u); nk[r] = 0; continue; }
		nk[r] = (uint32_t)c;
		mx = (unsigned int)c > mx ? (unsigned int)c : mx;
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) { unsigned int o = __shfl_xor(mx, off, 64); mx = o > mx ? o : mx; }
	if ((threadIdx.x & 63) == 0 && mx > __hip_atomic_load(most, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(most, mx);
}

__global__ void compare_totals_kernel(const uint32_t *wvals, uint32_t vw, uint64_t nw, const uint8_t *sweight, uint64_t ns, unsigned long long *tot) {
	unsigned long long size = 0, total = 0, sat = 0;
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nw + ns; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t c = i < nw ? (wvals[i * vw] & 0xffffu) : (sweight[i - nw] == 0 ? 0u : 1u);
		size++; total += c; sat += c == CMP_COUNT_MAX ? 1u : 0u;
	}
	size = wave_sum(size); total = wave_sum(total); sat = wave_sum(sat);
	if ((threadIdx.x & 63) == 0 && size) { atomicAdd(&tot[CMP_T_SIZE], size); atomicAdd(&tot[CMP_T_TOTAL], total); if (sat) atomicAdd(&tot[CMP_T_SATURATED], sat); }
}

/* reads [r0, r0 + m) that the sorted path takes (more than cap k-mers; every read when cap == 0): their slots, and their records
 * cleared apart from map 2's figures */
__global__ void compare_long_count_kernel(const uint64_t *koff, uint64_t r0, uint64_t m, uint32_t cap, const unsigned long long *tot2, uint32_t *cnt, CompareRec *out) {
	for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < m; r += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t nk = koff[r0 + r + 1] - koff[r0 + r];
		const bool lng = cap == 0 || nk > cap;
		cnt[r] = lng ? (uint32_t)nk : 0u;
		if (lng) {
			CompareRec z; z.size1 = z.common = z.common_count1 = z.common_count2 = z.total_count1 = 0;
			z.size2 = tot2[CMP_T_SIZE]; z.total_count2 = tot2[CMP_T_TOTAL]; z.saturated = tot2[CMP_T_SATURATED];
			out[r0 + r] = z;
		}
	}
}
/* slot j of the sorted path: the staging slot it reads (src), its read of the run (rid), and the identity permutation */
__global__ void compare_long_fill_kernel(const uint64_t *koff, uint64_t r0, uint64_t m, const uint64_t *loff, uint64_t c, uint32_t *src, uint32_t *rid, uint32_t *perm) {
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < c; j += (uint64_t)gridDim.x * blockDim.x) {
		uint64_t lo = 0, hi = m;                   /* the last read r with loff[r] <= j: its own slots are not empty, since loff[r + 1] > j */
		while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (loff[mid] <= j) lo = mid; else hi = mid; }
		src[j] = (uint32_t)(koff[r0 + lo] - koff[r0] + (j - loff[lo]));
		rid[j] = (uint32_t)lo;
		perm[j] = (uint32_t)j;
	}
}
/* head[j]: the slot opens a run of one (read, key) */
__global__ void compare_long_heads_kernel(const uint64_t *stage, uint32_t words, const uint32_t *src, const uint32_t *rid, const uint32_t *perm, uint64_t c, uint32_t *head) {
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < c; j += (uint64_t)gridDim.x * blockDim.x) {
		bool h = j == 0;
		if (!h) {
			const uint32_t p = perm[j], q = perm[j - 1];
			h = rid[p] != rid[q];
			for (uint32_t w = 0; w < words && !h; w++) h = stage[(uint64_t)src[p] * words + w] != stage[(uint64_t)src[q] * words + w];
		}
		head[j] = h ? 1u : 0u;
	}
}
#endif

/* map 1 entry by entry against map 2 */
template <int W>
__global__ void compare_maps_kernel(MapView<W> w1, uint64_t nw1, MapView<W> s1, uint64_t ns1, MapView<W> w2, MapView<W> s2, uint32_t kb, CompareRec *acc) {
	unsigned long long size1 = 0, total1 = 0, common = 0, cc1 = 0, cc2 = 0, sat = 0;
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nw1 + ns1; i += (uint64_t)gridDim.x * blockDim.x) {
		const bool weak = i < nw1;
		const uint64_t e = weak ? i : i - nw1;
		const uint64_t *kp = (weak ? w1.keys : s1.keys) + e * W;
		Key<W> key;
#pragma unroll
		for (int j = 0; j < W; j++) key.w[j] = kp[j];
		const uint32_t c1 = weak ? (w1.vals[e * w1.vw] & 0xffffu) : (s1.sweight[e] == 0 ? 0u : 1u);
		size1++; total1 += c1; sat += c1 == CMP_COUNT_MAX ? 1u : 0u;
		uint32_t c2;
		if (cmp_lookup<W>(w2, s2, key, kb, c2)) { common++; cc1 += c1; cc2 += c2; }
	}
	size1 = wave_sum(size1); total1 = wave_sum(total1); common = wave_sum(common); cc1 = wave_sum(cc1); cc2 = wave_sum(cc2); sat = wave_sum(sat);
	if ((threadIdx.x & 63) == 0 && size1) {
		atomicAdd(&acc->size1, size1); atomicAdd(&acc->total_count1, total1);
		if (common) { atomicAdd(&acc->common, common); atomicAdd(&acc->common_count1, cc1); atomicAdd(&acc->common_count2, cc2); }
		if (sat) atomicAdd(&acc->saturated, sat);
	}
}

/* reads [r0, r0 + m) of at most cap k-mers: one wavefront per read (see the head of this file) */
template <int W>
__global__ __launch_bounds__(CMP_WAVES * 64)
void compare_reads_lds_kernel(const uint64_t *stage, const uint64_t *koff, uint64_t r0, uint64_t m, uint32_t cap, MapView<W> weak, MapView<W> sing, uint32_t kb,
                              const unsigned long long *tot2, CompareRec *out) {
	extern __shared__ __attribute__((aligned(16))) uint8_t cmp_smem[];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	uint64_t *my = (uint64_t *)cmp_smem + (size_t)wave * cap * W;
	const uint64_t base = koff[r0];
	for (uint64_t r = (uint64_t)blockIdx.x * CMP_WAVES + wave; r < m; r += (uint64_t)gridDim.x * CMP_WAVES) {
		const uint64_t s = koff[r0 + r], nk = koff[r0 + r + 1] - s;
		if (nk > cap) continue;                       /* the sorted path's */
		const uint32_t n = (uint32_t)nk;
		const uint64_t *g = stage + (s - base) * W;
		for (uint32_t i = lane; i < n * W; i += 64) my[i] = g[i];
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		unsigned long long size1 = 0, total1 = 0, common = 0, cc1 = 0, cc2 = 0;
		for (uint32_t i = lane; i < n; i += 64) {
			Key<W> key;
#pragma unroll
			for (int w = 0; w < W; w++) key.w[w] = my[i * W + w];
			if (cmp_is_sentinel<W>(key)) continue;
			uint32_t before = 0, mult = 0;
			for (uint32_t j = 0; j < n; j++) {
				bool eq = true;
#pragma unroll
				for (int w = 0; w < W; w++) eq = eq && my[j * W + w] == key.w[w];
				mult += eq ? 1u : 0u;
				before += (eq && j < i) ? 1u : 0u;
			}
			if (before) continue;                     /* counted at its first occurrence */
			size1++; total1 += mult;
			uint32_t c2;
			if (cmp_lookup<W>(weak, sing, key, kb, c2)) { common++; cc1 += mult; cc2 += c2; }
		}
		size1 = wave_sum(size1); total1 = wave_sum(total1); common = wave_sum(common); cc1 = wave_sum(cc1); cc2 = wave_sum(cc2);
		if (lane == 0) {
			CompareRec z; z.size1 = size1; z.size2 = tot2[CMP_T_SIZE]; z.common = common; z.common_count1 = cc1; z.common_count2 = cc2;
			z.total_count1 = total1; z.total_count2 = tot2[CMP_T_TOTAL]; z.saturated = tot2[CMP_T_SATURATED];
			out[r0 + r] = z;
		}
		__builtin_amdgcn_wave_barrier();              /* all lanes are done with the slots before the next read's arrive */
	}
}

/* sorted path: every head looks its key up and adds to its read's record */
template <int W>
__global__ void compare_long_add_kernel(const uint64_t *stage, const uint32_t *src, const uint32_t *rid, const uint32_t *perm, const uint32_t *head, const uint64_t *hscan,
                                        const uint64_t *start, uint64_t c, uint64_t r0, MapView<W> weak, MapView<W> sing, uint32_t kb, CompareRec *out) {
	const uint64_t c64 = (c + 63) & ~63ull;         /* whole wavefronts walk the loop together */
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < c64; j += (uint64_t)gridDim.x * blockDim.x) {
		unsigned long long size1 = 0, total1 = 0, common = 0, cc1 = 0, cc2 = 0;
		uint32_t r = 0xffffffffu;
		if (j < c) {
			const uint32_t p = perm[j];
			r = rid[p];
			if (head[j]) {
				Key<W> key;
#pragma unroll
				for (int w = 0; w < W; w++) key.w[w] = stage[(uint64_t)src[p] * W + w];
				if (!cmp_is_sentinel<W>(key)) {
					const unsigned long long mult = start[hscan[j] + 1] - j;
					size1 = 1; total1 = mult;
					uint32_t c2;
					if (cmp_lookup<W>(weak, sing, key, kb, c2)) { common = 1; cc1 = mult; cc2 = c2; }
				}
			}
		}
		const uint32_t rfirst = __shfl(r, 0, 64);
		if (__all(r == rfirst || r == 0xffffffffu)) {      /* one read (the tail's idle lanes aside): one atomic per field */
			size1 = wave_sum(size1); total1 = wave_sum(total1); common = wave_sum(common); cc1 = wave_sum(cc1); cc2 = wave_sum(cc2);
			if ((threadIdx.x & 63) != 0) size1 = 0;
			r = rfirst;
		}
		if (size1) {
			CompareRec *o = out + r0 + r;
			atomicAdd(&o->size1, size1); atomicAdd(&o->total_count1, total1);
			if (common) { atomicAdd(&o->common, common); atomicAdd(&o->common_count1, cc1); atomicAdd(&o->common_count2, cc2); }
		}
	}
}

}  // namespace kmr
#endif
