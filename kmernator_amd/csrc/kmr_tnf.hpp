/*
 * kmr_tnf.hpp -- HIP kernels (gfx950) of TnfDistance (apps/TnfDistance.cpp): per-sequence and per-window counts of the canonical
 * k-mers of a very small k (1 - 6, "tetranucleotide frequency" at the default 4), and the distances between such vectors.
 *
 * Vectors.  The build's own extraction (extract_kernel with CompareOp<1>, launched by kmr_api.hip's tnf_stage_core) leaves one
 * 8-byte slot per k-mer position of the batch: the canonical key word where the k-mer passes the weight test, all ones where it does
 * not.  A vector is a range of those slots -- a whole sequence, or the window - k + 1 positions of a window --, cut into pieces:
 *
 *   tnf_hist_kernel      a wavefront takes a run of consecutive pieces.  While they belong to one vector it counts into its own
 *                        LDS histogram of 4^k u32 bins indexed by the 2k-bit code (one ds_add_u32 per k-mer); where the vector
 *                        changes, and at the end of its run, it adds every non-zero bin to the vector's column (one global atomic
 *                        per non-zero bin, vector and wavefront).  Many short sequences share a workgroup, one long contig is
 *                        spread over as many wavefronts as it has pieces.
 *   tnf_win_*            shredReadByWindow (:486-494): windows per sequence, then every window's slots and origin
 *   tnf_rowsum / keep / compact / bounds      purgeShortTNFS (:506-518), input order kept
 *   tnf_group_sum_kernel the vectors of a group added as u64 (wholeTnfs, :717)
 *
 * LDS of tnf_hist_kernel: TNF_WAVES * 4^k * 4 bytes, 64 KiB at k = 6 (two blocks a CU), 4 KiB at k = 4.
 *
 * Distances.  What depends on one vector only is made once per vector (tnf_len2 / tnf_quot / tnf_rank / tnf_x2 kernels): the squared
 * length, the fp64 quotients value / length, the ranks less their mean and the running sum of their squares.  Both are stored
 * column-major ([column][vector]), so that a tile of 64 vectors is 512 (256) contiguous bytes per column.
 *
 *   tnf_pairs_kernel     a 256-thread block takes a tile of 64 x 64 pairs, each lane a 4 x 4 block of them in registers.  D is
 *                        walked in slices of TNF_SLICE columns held in LDS for both sides; per pair and column: one fp64 subtraction,
 *                        one conversion, one fp32 product, one fp32 sum (Euclidean), or one product and one sum (Spearman) -- never
 *                        contracted.  A pair's sum stays in its lane from column 0 to D - 1.  The tile is a part of a rectangle
 *                        (rows of a against all of b) or of the strict lower triangle of a; the distance goes to the matrix, or
 *                        (HIST) into one of two histograms chosen by whether the two vectors belong to one group, counted per
 *                        block in LDS and added once per block and non-zero bin.
 *
 * LDS of tnf_pairs_kernel: 2 * TNF_SLICE * 64 * 8 bytes = 32 KiB (Euclidean; half for Spearman) + 4 (bins + 2) bytes with HIST.
 */
#ifndef KMR_TNF_HPP_
#define KMR_TNF_HPP_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace kmr {

static const uint32_t TNF_MAX_K = 6;
static const int TNF_WAVES = 4;
static const uint32_t TNF_PIECE_BASES = 4096;      /* bases of one piece (kmr_tune "tnf_piece_bases") */
static const int TNF_TILE = 64, TNF_SLICE = 32, TNF_BLOCK = 256;
static const uint32_t TNF_MAX_BINS = 4094;         /* likelihood bins: bins + 2 u32 counters in LDS */
static const uint32_t TNF_NO_COLUMN = 0xffffu;

__device__ __forceinline__ void tnf_wave_sync() {
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ unsigned long long tnf_wave_sum(unsigned long long v) {
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
	return v;
}
/* the last index i of a non-decreasing off[0 .. n] with off[i] <= x (off[0] <= x < off[n]) */
__device__ __forceinline__ uint64_t tnf_owner(const uint64_t *off, uint64_t n, uint64_t x) {
	uint64_t lo = 0, hi = n;
	while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (off[mid] <= x) lo = mid; else hi = mid; }
	return lo;
}

/* ---- vectors --------------------------------------------------------------------------------------------------------------- */

/* one vector per sequence: its slots are the sequence's, its origin the whole sequence */
__global__ void tnf_reads_desc_kernel(const uint64_t *offsets, const uint64_t *koff, uint64_t n, uint64_t *vslot, uint32_t *vnk, uint64_t *origin) {
	for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
		vslot[r] = koff[r]; vnk[r] = (uint32_t)(koff[r + 1] - koff[r]);
		origin[3 * r] = r; origin[3 * r + 1] = 0; origin[3 * r + 2] = offsets[r + 1] - offsets[r];
	}
}
/* windows of a sequence of L bases: i = 0, step, 2 step, ... while i < L - window */
__global__ void tnf_win_count_kernel(const uint64_t *offsets, uint64_t n, uint64_t window, uint64_t step, uint32_t *nwin, uint32_t *err) {
	for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t L = offsets[r + 1] - offsets[r];
		const uint64_t c = L > window ? (L - window + step - 1) / step : 0;
		if (c > 0xffffffffull) { atomicOr(err, 1u); nwin[r] = 0; continue; }
		nwin[r] = (uint32_t)c;
	}
}
__global__ void tnf_win_desc_kernel(const uint64_t *koff, const uint64_t *woff, uint64_t n, uint64_t nw, uint64_t window, uint64_t step, uint32_t k,
                                    uint64_t *vslot, uint32_t *vnk, uint64_t *origin) {
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < nw; j += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t r = tnf_owner(woff, n, j);
		const uint64_t start = (j - woff[r]) * step;
		vslot[j] = koff[r] + start; vnk[j] = window >= k ? (uint32_t)(window - k + 1) : 0u;      /* start + window < L: the slots exist */
		origin[3 * j] = r; origin[3 * j + 1] = start; origin[3 * j + 2] = window;
	}
}
__global__ void tnf_piece_count_kernel(const uint32_t *vnk, uint64_t n, uint32_t piece, uint32_t *pcnt) {
	for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < n; v += (uint64_t)gridDim.x * blockDim.x) pcnt[v] = (vnk[v] + piece - 1) / piece;
}

/* pieces [w * per_wave, (w + 1) * per_wave) are wavefront w's; piece p of vector v covers k-mers [(p - poff[v]) * piece, ...) */
__global__ __launch_bounds__(TNF_WAVES * 64)
void tnf_hist_kernel(const uint64_t *stage, const uint64_t *vslot, const uint32_t *vnk, const uint64_t *poff, uint64_t n_vec, uint64_t n_pieces, uint64_t per_wave,
                     uint32_t piece, uint32_t k, const uint16_t *col_of_code, uint32_t D, uint32_t *counts) {
	extern __shared__ __attribute__((aligned(16))) uint32_t tnf_smem[];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint32_t bins = 1u << (2 * k), shift = 64 - 2 * k;
	uint32_t *hist = tnf_smem + (size_t)wave * bins;
	for (uint32_t b = lane; b < bins; b += 64) hist[b] = 0;
	tnf_wave_sync();
	const uint64_t p0 = ((uint64_t)blockIdx.x * TNF_WAVES + wave) * per_wave;
	const uint64_t p1 = p0 + per_wave < n_pieces ? p0 + per_wave : n_pieces;
	if (p0 >= p1) return;
	uint64_t v = tnf_owner(poff, n_vec, p0);
	for (uint64_t p = p0; p < p1;) {
		const uint64_t vfirst = poff[v], vend = poff[v + 1];
		const uint64_t pend = vend < p1 ? vend : p1;
		const uint32_t nk = vnk[v];
		const uint64_t first = (p - vfirst) * piece;
		uint64_t last = (pend - vfirst) * piece; if (last > nk) last = nk;
		const uint64_t *s = stage + vslot[v];
		for (uint64_t j = first + lane; j < last; j += 64) {
			const uint64_t key = s[j];
			if (key != ~0ull) atomicAdd(&hist[(uint32_t)(key >> shift) & (bins - 1)], 1u);
		}
		tnf_wave_sync();
		for (uint32_t b = lane; b < bins; b += 64) {
			const uint32_t c = hist[b];
			if (c) {
				hist[b] = 0;
				const uint32_t col = col_of_code[b];
				if (col < D) atomicAdd(&counts[v * D + col], c);
			}
		}
		tnf_wave_sync();
		p = pend;
		do v++; while (v < n_vec && poff[v + 1] == poff[v]);      /* vectors without a k-mer have no piece */
	}
}

/* one wavefront per vector: the sum of its counts */
__global__ void tnf_rowsum_kernel(const uint32_t *counts, uint64_t n, uint32_t D, unsigned long long *sums) {
	const int lane = threadIdx.x & 63;
	for (uint64_t v = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6; v < n; v += ((uint64_t)gridDim.x * blockDim.x) >> 6) {
		unsigned long long s = 0;
		for (uint32_t c = lane; c < D; c += 64) s += counts[v * D + c];
		s = tnf_wave_sum(s);
		if (lane == 0) sums[v] = s;
	}
}
/* purgeShortTNFS: getCount() < minimumCount goes */
__global__ void tnf_keep_kernel(const unsigned long long *sums, uint64_t n, long long min_count, uint32_t *keep) {
	for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < n; v += (uint64_t)gridDim.x * blockDim.x)
		keep[v] = (min_count > 0 && sums[v] < (unsigned long long)min_count) ? 0u : 1u;
}
__global__ void tnf_compact_kernel(const uint32_t *counts, const uint64_t *origin, const uint32_t *keep, const uint64_t *kpos, uint64_t n, uint32_t D,
                                   uint32_t *counts_out, uint64_t *origin_out) {
	const uint64_t total = n * (D + 3);      /* D counts and the three origin words of every vector */
	for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t v = e / (D + 3); const uint32_t c = (uint32_t)(e - v * (D + 3));
		if (!keep[v]) continue;
		const uint64_t o = kpos[v];
		if (c < D) counts_out[o * D + c] = counts[v * D + c];
		else origin_out[3 * o + (c - D)] = origin[3 * v + (c - D)];
	}
}
/* group g begins at the first surviving window of sequence starts[g] */
__global__ void tnf_bounds_kernel(const uint64_t *starts, uint32_t n_groups, const uint64_t *woff, const uint64_t *kpos, uint64_t *bounds) {
	for (uint32_t g = threadIdx.x; g <= n_groups; g += blockDim.x) bounds[g] = kpos[woff[starts[g]]];
}
/* blockIdx.y = group, blockIdx.x = a run of 256 of its vectors; threads stride the columns */
__global__ void tnf_group_sum_kernel(const uint32_t *counts, const uint64_t *bounds, uint32_t D, unsigned long long *sums) {
	const uint32_t g = blockIdx.y;
	const uint64_t v0 = bounds[g] + (uint64_t)blockIdx.x * 256, vend = bounds[g + 1];
	const uint64_t v1 = v0 + 256 < vend ? v0 + 256 : vend;
	if (v0 >= v1) return;
	for (uint32_t c = threadIdx.x; c < D; c += blockDim.x) {
		unsigned long long s = 0;
		for (uint64_t v = v0; v < v1; v++) s += counts[v * D + c];
		if (s) atomicAdd(&sums[(uint64_t)g * D + c], s);
	}
}

/* ---- per vector: length, quotients, ranks ---------------------------------------------------------------------------------------- */

template <class T> __device__ __forceinline__ float tnf_value(const T *counts, uint64_t i) { return (float)counts[i]; }

/* calcLength (:396-411) up to the root: l += (double)(v[i] * v[i]), the product in float, in column order; and the columns above 2^24 */
template <class T>
__global__ void tnf_len2_kernel(const T *counts, uint64_t n, uint32_t D, double *len2, unsigned long long *inexact) {
#pragma clang fp contract(off)
	unsigned long long bad = 0;
	for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < n; v += (uint64_t)gridDim.x * blockDim.x) {
		double l = 0.0;
		for (uint32_t c = 0; c < D; c++) {
			const T raw = counts[v * D + c];
			bad += raw > (T)(1u << 24) ? 1u : 0u;
			const float x = (float)raw;
			const float xx = x * x;
			l = l + (double)xx;
		}
		len2[v] = l;
	}
	bad = tnf_wave_sum(bad);
	if ((threadIdx.x & 63) == 0 && bad) atomicAdd(inexact, bad);
}
/* (double)v[i] / (double)length, column-major */
template <class T>
__global__ void tnf_quot_kernel(const T *counts, const float *len, uint64_t n, uint32_t D, double *qt) {
	const uint64_t total = n * D;
	for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t c = e / n, v = e - c * n;
		qt[e] = (double)(float)counts[v * D + c] / (double)len[v];
	}
}
/* RankVector (src/Utils.h:2105-2131) less the mean of getSpearmanDistance (:2146-2150): one block per vector, its values in LDS.  With L
 * values smaller and E equal (itself included) the rank is (float)(L E + E (E + 1) / 2) / (float)E, which is L + 1 for E = 1 */
template <class T>
__global__ __launch_bounds__(256)
void tnf_rank_kernel(const T *counts, uint64_t n, uint32_t D, float *xt) {
	extern __shared__ __attribute__((aligned(16))) uint32_t tnf_smem[];
	float *val = (float *)tnf_smem;
	const float mean = (float)((D + 1) / 2);
	for (uint64_t v = blockIdx.x; v < n; v += gridDim.x) {
		for (uint32_t c = threadIdx.x; c < D; c += blockDim.x) val[c] = (float)counts[v * D + c];
		__syncthreads();
		for (uint32_t c = threadIdx.x; c < D; c += blockDim.x) {
			const float x = val[c];
			int L = 0, E = 0;
			for (uint32_t j = 0; j < D; j++) { const float y = val[j]; L += y < x ? 1 : 0; E += y == x ? 1 : 0; }
			const float rank = (float)(L * E + E * (E + 1) / 2) / (float)E;
			xt[(uint64_t)c * n + v] = rank - mean;
		}
		__syncthreads();
	}
}
/* sum_x2 of getSpearmanDistance: a float sum of float products in column order */
__global__ void tnf_x2_kernel(const float *xt, uint64_t n, uint32_t D, float *x2) {
#pragma clang fp contract(off)
	for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < n; v += (uint64_t)gridDim.x * blockDim.x) {
		float s = 0.0f;
		for (uint32_t c = 0; c < D; c++) { const float x = xt[(uint64_t)c * n + v]; const float xx = x * x; s = s + xx; }
		x2[v] = s;
	}
}

/* ---- pairs --------------------------------------------------------------------------------------------------------------------- */

struct TnfSide {
	const void *t;             /* column-major [D][n]: double quotients (Euclidean) or float ranks less the mean (Spearman) */
	const float *x2;           /* Spearman: sum_x2 per vector */
	const uint32_t *group;     /* HIST: the group of every vector */
	uint64_t n;
};
struct TnfPairs {
	uint32_t D;
	int triangle;              /* pairs j < i of side a with itself (b = a) */
	uint64_t first_row, n_rows;      /* rows of a the call takes */
	float *out;                /* !HIST: the matrix (rectangle: n_rows x b.n; triangle: row i holds j < i, rows packed) */
	/* HIST (GenericHistogram, src/Utils.h:2163-2254): */
	unsigned long long *hist;  /* [2][bins + 2]: same group (where intra_ok says so), other group */
	const uint8_t *intra_ok;   /* per group of a: its same-group pairs count */
	uint32_t bins; float end, step;
};

__device__ __forceinline__ uint32_t tnf_bin(float v, float end, float step, uint32_t bins) {
	if (!(v >= 0.0f)) return 0u;                    /* v < _start; a NaN (undefined in the reference) is counted here */
	if (v > end) return bins + 1;
	const uint32_t idx = (uint32_t)(int)(v / step) + 1u;
	return idx > bins + 1 ? bins + 1 : idx;
}

template <bool SPEARMAN, bool HIST>
__global__ __launch_bounds__(TNF_BLOCK)
void tnf_pairs_kernel(TnfSide a, TnfSide b, TnfPairs P) {
#pragma clang fp contract(off)
	typedef typename std::conditional<SPEARMAN, float, double>::type T;
	extern __shared__ __attribute__((aligned(16))) uint32_t tnf_smem[];
	T *As = (T *)tnf_smem, *Bs = As + TNF_SLICE * TNF_TILE;
	uint32_t *lh = (uint32_t *)(Bs + TNF_SLICE * TNF_TILE);
	const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
	const uint32_t nbin = P.bins + 2;
	if (HIST) { for (uint32_t i = tid; i < 2 * nbin; i += TNF_BLOCK) lh[i] = 0; }
	const uint64_t row_tiles = (P.n_rows + TNF_TILE - 1) / TNF_TILE, col_tiles = (b.n + TNF_TILE - 1) / TNF_TILE;
	const uint64_t tiles = row_tiles * col_tiles;
	const T *at = (const T *)a.t, *bt = (const T *)b.t;
	for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
		const uint64_t tr = tile / col_tiles, tc = tile - tr * col_tiles;
		const uint64_t i0 = P.first_row + tr * TNF_TILE, j0 = tc * TNF_TILE;
		const uint64_t iend = P.first_row + P.n_rows;
		if (P.triangle && j0 + 1 > (i0 + TNF_TILE - 1 < iend - 1 ? i0 + TNF_TILE - 1 : iend - 1)) continue;      /* no j < i in this tile (block-uniform) */
		float acc[4][4];
#pragma unroll
		for (int i = 0; i < 4; i++)
#pragma unroll
			for (int j = 0; j < 4; j++) acc[i][j] = 0.0f;
		for (uint32_t c0 = 0; c0 < P.D; c0 += TNF_SLICE) {
			const uint32_t sl = P.D - c0 < (uint32_t)TNF_SLICE ? P.D - c0 : (uint32_t)TNF_SLICE;
			__syncthreads();                        /* the last slice has been read (and the LDS counters are cleared) */
			for (uint32_t e = tid; e < sl * TNF_TILE; e += TNF_BLOCK) {
				const uint32_t c = e >> 6, r = e & 63;
				const uint64_t ia = i0 + r, jb = j0 + r;
				As[e] = ia < iend ? at[(uint64_t)(c0 + c) * a.n + ia] : (T)0;
				Bs[e] = jb < b.n ? bt[(uint64_t)(c0 + c) * b.n + jb] : (T)0;
			}
			__syncthreads();
			for (uint32_t c = 0; c < sl; c++) {
				T av[4], bv[4];
#pragma unroll
				for (int i = 0; i < 4; i++) { av[i] = As[c * TNF_TILE + ty * 4 + i]; bv[i] = Bs[c * TNF_TILE + tx * 4 + i]; }
#pragma unroll
				for (int i = 0; i < 4; i++)
#pragma unroll
					for (int j = 0; j < 4; j++) {
						if (SPEARMAN) { const float xy = (float)av[i] * (float)bv[j]; acc[i][j] = acc[i][j] + xy; }
						else { const float d = (float)((double)av[i] - (double)bv[j]); const float dd = d * d; acc[i][j] = acc[i][j] + dd; }
					}
			}
		}
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const uint64_t ia = i0 + ty * 4 + i;
			if (ia >= iend) continue;
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const uint64_t jb = j0 + tx * 4 + j;
				if (jb >= b.n || (P.triangle && jb >= ia)) continue;
				float dist;
				if (SPEARMAN) { const float r = acc[i][j] / sqrtf(a.x2[ia] * b.x2[jb]); dist = (1.0f - r) / 2.0f; }
				else dist = sqrtf(acc[i][j]);
				if (HIST) {
					const uint32_t ga = a.group[ia];
					const bool same = ga == b.group[jb];
					if (same && !P.intra_ok[ga]) continue;
					atomicAdd(&lh[(same ? 0u : nbin) + tnf_bin(dist, P.end, P.step, P.bins)], 1u);
				} else if (P.triangle) P.out[ia * (ia - 1) / 2 - P.first_row * (P.first_row - (P.first_row ? 1 : 0)) / 2 + jb] = dist;
				else P.out[(ia - P.first_row) * b.n + jb] = dist;
			}
		}
	}
	if (HIST) {
		__syncthreads();
		for (uint32_t i = tid; i < 2 * nbin; i += TNF_BLOCK) { const uint32_t c = lh[i]; if (c) atomicAdd(&P.hist[i], (unsigned long long)c); }
	}
}

}  // namespace kmr
#endif
