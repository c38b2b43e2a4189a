/*
 * kmr_match.hpp -- HIP kernels (gfx950) of KmerMatch (src/KmerMatch.h:93-185 with src/MatcherInterface.h:280-346, :683-816): for every
 * contig the reads that share a k-mer with one of its two edge windows, sampled where there are too many, with their mates, sorted.
 *
 * The reference asks a spectrum whose values hold every (read, position) instance of a k-mer (TrackingDataWithAllReads).  Here the
 * join is turned around: the contigs' edge k-mers are a small table (a few hundred KB, resident in L2), and the reads stream through
 * the build's extraction once, probing it.  Everything is an integer join, so no order matters until the final sort.
 *
 *  Create   match_edge_count_kernel   considered k-mers of every contig (the edge rule of KmerMatch.h:124-149, match_edge_shape)
 *           match_edge_keys_kernel    one thread per considered k-mer: its canonical key from the packed sequence (a non-ACGT base is
 *                                     code 0, as KmerWeights(twoBit, len, true) sees it) and its contig -- a long contig is spread
 *                                     over as many lanes as it has edge k-mers
 *           sort_by_columns           (kmr_sort.hip) one stable radix pass for the contig, then one per key word, last word first
 *           match_flags_kernel        per sorted record: first of its key, first of its (key, contig), and whether the spectrum holds
 *                                     the key (map_find on the weak map, then on the singleton map)
 *           match_table_fill_kernel   the contigs of every kept key, distinct and contiguous, and the key into the table
 *  Stream   MatchOp                   extract_kernel's Op: every k-mer that passes the build's weight test probes the table; a hit
 *                                     appends one record per contig of the key that is not the lane's previous contig
 *  Finish   (KMR_MATCH_FINISH, kmr_stages.hip) match_heads_kernel .. match_emit_kernel, see below
 *
 * The table: open addressing in steps of one over 2^log2cap slots of W key words and one value word (first contig << 32 | contigs), at
 * most half full, an empty slot marked by the all-ones value word.  A hit record: (contig << MATCH_READ_BITS | global read) and the
 * global index of the read's mate or MATCH_NO_MATE, two u64.
 *
 * Registers and LDS of MatchOp: its State is one register (the lane's previous contig); it uses no LDS beyond the extraction's tiles,
 * so the occupancy of extract_kernel (two 4-wave blocks per CU) is unchanged.  The probe of a miss is one load of the value word of
 * one slot -- 8 bytes of a table that stays in L2 --; a slot that is taken costs the W key words too.
 */
#ifndef KMR_MATCH_HPP_
#define KMR_MATCH_HPP_

#include <stdint.h>

namespace kmr {

static const int MATCH_READ_BITS = 40;                          /* a packed record: the contig above, the global read index below */
static const uint64_t MATCH_READ_MASK = (1ull << MATCH_READ_BITS) - 1;
static const uint64_t MATCH_MAX_CONTIGS = 1ull << (64 - MATCH_READ_BITS);
static const uint64_t MATCH_NO_MATE = ~0ull;
static const uint64_t MATCH_HIT_CAP = 1ull << 20;               /* hit records the buffers hold at first (kmr_tune "match_hit_capacity") */

}  // namespace kmr

#ifndef KMR_MATCH_FINISH
/* ------------------------------------------------------------------ the table, the Op and the kernels of kmr_match_create (kmr_api.hip) */
#include "kmr_kernels.hpp"

namespace kmr {

template <int W> struct MatchTable {
	const uint64_t *slots;         /* [2^(64 - shift)][W + 1] */
	const uint32_t *contigs;       /* the contigs of every key, one after the other */
	uint32_t shift;                /* 64 - log2cap, log2cap >= 6 */
};

/* the slot a key starts at: multiplications carry every bit of the left-justified key into the top bits that are kept */
template <int W> __host__ __device__ __forceinline__ uint64_t match_slot(const Key<W> &key, uint32_t shift) {
	uint64_t x = key.w[0];
#pragma unroll
	for (int i = 1; i < W; i++) x = (x * 0xD6E8FEB86659FD93ull) ^ (x >> 32) ^ key.w[i];
	return (x * 0x9E3779B97F4A7C15ull) >> shift;
}

template <int W> __device__ __forceinline__ bool match_probe(const MatchTable<W> &t, const Key<W> &key, uint32_t &first, uint32_t &count) {
	const uint64_t mask = (1ull << (64 - t.shift)) - 1;
	uint64_t s = match_slot<W>(key, t.shift);
	for (;;) {                                      /* the table is at most half full: an empty slot ends every walk */
		const uint64_t *p = t.slots + s * (W + 1);
		const uint64_t v = p[W];
		if (v == ~0ull) return false;
		bool eq = true;
#pragma unroll
		for (int i = 0; i < W; i++) eq = eq && p[i] == key.w[i];
		if (eq) { first = (uint32_t)(v >> 32); count = (uint32_t)v; return true; }
		s = (s + 1) & mask;
	}
}

template <int W> struct MatchOp {
	MatchTable<W> table;
	unsigned long long *hit_key, *hit_mate;      /* [cap] */
	unsigned long long *count;                   /* records appended so far; what lies beyond cap is counted and not written */
	uint64_t cap;
	const int64_t *mate;                         /* per read of the batch its mate in the batch or -1; NULL: no mates */
	uint64_t first_global;                       /* global index of the batch's first read */
	static const bool NEEDS_WEIGHT = true;       /* the build's own weight test decides which k-mers the spectrum saw of a read */
	static const bool COUNTS_STATS = false;
	static const bool NEEDS_HASH = false;
	struct State { uint32_t prev; };             /* the contig of the lane's last record: a lane walks one read, and most of a read's hits repeat it */
	__device__ __forceinline__ void wave_begin(State &st, int) const { st.prev = 0xffffffffu; }
	__device__ __forceinline__ void wave_end(State &, int) const {}
	__device__ __forceinline__ void tile_begin(State &st, uint32_t *, uint64_t, int) const { st.prev = 0xffffffffu; }
	__device__ __forceinline__ void tile_end(State &, uint64_t, int) const {}
	__device__ __forceinline__ void emit(State &st, bool valid, const DevParams &, const Key<W> &key, uint64_t, const Occurrence &,
	                                     uint64_t readIdx, uint32_t, unsigned &, bool &) const {
		if (!valid) return;
		uint32_t first, n;
		if (!match_probe<W>(table, key, first, n)) return;
		for (uint32_t i = 0; i < n; i++) {
			const uint32_t c = table.contigs[first + i];
			if (c == st.prev) continue;
			st.prev = c;
			const unsigned long long at = atomicAdd(count, 1ull);      /* hits are rare: one atomic each */
			if (at < cap) {
				hit_key[at] = ((unsigned long long)c << MATCH_READ_BITS) | (first_global + readIdx);
				const int64_t m = mate ? mate[readIdx] : -1;
				hit_mate[at] = m >= 0 ? first_global + (uint64_t)m : MATCH_NO_MATE;
			}
		}
	}
};
template <int W> __device__ __forceinline__ bool op_keeps_all_owners(const MatchOp<W> &) { return true; }
template <int W> __device__ __forceinline__ uint32_t op_fail_code(const MatchOp<W> &) { return 0; }

/* The edge rule (KmerMatch.h:124-149): with M = max_positions_from_edge - k + 1 as an int and n k-mers, k-mer j is considered if
 * j <= (unsigned)M || j >= upperMinKmer, upperMinKmer = n - M if (int)n > M and 0 otherwise.  M < 0 makes (unsigned)M huge: every
 * k-mer.  Otherwise the left side takes M + 1 k-mers and the right side M, or all of them where the two meet.  Returns the number
 * considered; *split: the middle is skipped (then k-mer t of the considered ones is j = t for t <= M and n - M + (t - M - 1) beyond) */
__host__ __device__ __forceinline__ uint64_t match_edge_shape(uint64_t n, int32_t M, bool *split) {
	*split = false;
	if (M < 0 || n <= (uint64_t)M || n - (uint64_t)M <= (uint64_t)M + 1) return n;
	*split = true;
	return 2 * (uint64_t)M + 1;
}

#ifndef KMR_INSTANCE_TU
__global__ void match_edge_count_kernel(const uint64_t *offsets, uint64_t nc, uint32_t k, int32_t M, uint32_t *cnt, uint32_t *err) {
	for (uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; c < nc; c += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t L = offsets[c + 1] - offsets[c];
		if (L >= 0x7fffffffull) { atomicOr(err, 1u); cnt[c] = 0; continue; }      /* (int) kmers.size() of the reference */
		bool split;
		cnt[c] = (uint32_t)match_edge_shape(L >= k ? L - k + 1 : 0, M, &split);
	}
}
#endif

/* record e of the table's input: the contig it lies in (eoff: first record of every contig, nc + 1), its k-mer, the canonical key */
template <int W>
__global__ void match_edge_keys_kernel(const uint8_t *bases, const uint64_t *offsets, uint64_t nc, uint32_t k, int32_t M, const uint64_t *eoff, uint64_t E,
                                       uint64_t *keys, uint32_t *contig, uint32_t *perm) {
	for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < E; e += (uint64_t)gridDim.x * blockDim.x) {
		uint64_t lo = 0, hi = nc;                     /* the last contig c with eoff[c] <= e: it has records, since eoff[c + 1] > e */
		while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (eoff[mid] <= e) lo = mid; else hi = mid; }
		const uint64_t b = offsets[lo], n = offsets[lo + 1] - b - k + 1, t = e - eoff[lo];
		bool split;
		match_edge_shape(n, M, &split);
		const uint64_t j = (!split || t <= (uint64_t)M) ? t : n - (uint64_t)M + (t - (uint64_t)M - 1);
		Roller<W> roll;
		roll.init(k);
		for (uint32_t i = 0; i < k; i++) { uint32_t code = base_code(bases[b + j + i]); if (code == 4) code = 0; roll.push(code); }
		const Key<W> kf = roll.getFwd(), kr = roll.getRc();
		const Key<W> canon = key_le<W>(kf, kr) ? kf : kr;
#pragma unroll
		for (int i = 0; i < W; i++) keys[e * W + i] = canon.w[i];
		contig[e] = (uint32_t)lo;
		perm[e] = (uint32_t)e;
	}
}

/* sorted record j: khead = the first of its key, kkept = that and the spectrum holds the key, phead = the first of its (key, contig)
 * of a key the spectrum holds */
template <int W>
__global__ void match_flags_kernel(const uint64_t *keys, const uint32_t *contig, const uint32_t *perm, uint64_t E, MapView<W> weak, MapView<W> sing, uint32_t kb,
                                   uint32_t *khead, uint32_t *kkept, uint32_t *phead) {
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < E; j += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t p = perm[j];
		Key<W> key;
#pragma unroll
		for (int i = 0; i < W; i++) key.w[i] = keys[(uint64_t)p * W + i];
		bool newkey = j == 0, newpair = j == 0;
		if (j) {
			const uint32_t q = perm[j - 1];
#pragma unroll
			for (int i = 0; i < W; i++) newkey = newkey || keys[(uint64_t)q * W + i] != key.w[i];
			newpair = newkey || contig[q] != contig[p];
		}
		const uint64_t hash = key_hash<W>(key, kb);
		const bool held = map_find<W>(weak, key, hash) >= 0 || map_find<W>(sing, key, hash) >= 0;
		khead[j] = newkey ? 1u : 0u; kkept[j] = (newkey && held) ? 1u : 0u; phead[j] = (newpair && held) ? 1u : 0u;
	}
}

/* the contig list (pscan: exclusive scan of phead, E + 1) and, per kept key, its slot: claimed by compare-and-swap on the value word,
 * the key words written by the winner -- the keys are distinct and nothing reads the table before the kernel has ended */
template <int W>
__global__ void match_table_fill_kernel(const uint64_t *keys, const uint32_t *contig, const uint32_t *perm, uint64_t E, const uint32_t *khead, const uint32_t *kkept,
                                        const uint32_t *phead, const uint64_t *pscan, uint64_t *slots, uint32_t shift, uint32_t *tcontig) {
	const uint64_t mask = (1ull << (64 - shift)) - 1;
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < E; j += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t p = perm[j];
		if (phead[j]) tcontig[pscan[j]] = contig[p];
		if (!kkept[j]) continue;
		uint64_t je = j + 1;
		while (je < E && !khead[je]) je++;
		Key<W> key;
#pragma unroll
		for (int i = 0; i < W; i++) key.w[i] = keys[(uint64_t)p * W + i];
		const unsigned long long val = ((unsigned long long)pscan[j] << 32) | (unsigned long long)(pscan[je] - pscan[j]);
		uint64_t s = match_slot<W>(key, shift);
		for (;;) {
			uint64_t *sl = slots + s * (W + 1);
			if (atomicCAS((unsigned long long *)&sl[W], ~0ull, val) == ~0ull) {
#pragma unroll
				for (int i = 0; i < W; i++) sl[i] = key.w[i];
				break;
			}
			s = (s + 1) & mask;
		}
	}
}

}  // namespace kmr

#else
/* ------------------------------------------------------------------------------- the kernels of kmr_match_finish (kmr_stages.hip)
 *  match_heads_kernel     sorted packed records: the first of every (contig, read)
 *  match_compact_kernel   the distinct records and their mates
 *  match_bounds_kernel    per contig the first record at or above (contig << MATCH_READ_BITS): set sizes, CSR offsets
 *  match_sample_kernel    sampleMatches (MatcherInterface.h:280-287) per set of more than 2 * max_read_matches reads, the random
 *                         number from Philox; how many records a read leaves (itself and, where wanted, its mate)
 *  match_emit_kernel      those records
 *  match_final_kernel     sorted again: the first of every (contig, read) whose read is not discarded (getLocalReads :311-321)
 *  match_output_kernel    the read indices of the result
 */
#include "kmr_normalize.hpp"      /* philox4x32_10 */

namespace kmr {

/* the discard flags of the batches fed so far: batch b holds global reads [first[b], first[b] + n[b]), flags[b] may be NULL */
struct MatchBatches { const uint64_t *first, *n; const uint8_t *const *flags; uint32_t nb; };

__device__ __forceinline__ bool match_discarded(const MatchBatches &B, uint64_t read) {
	for (uint32_t b = 0; b < B.nb; b++)
		if (read >= B.first[b] && read - B.first[b] < B.n[b]) { if (B.flags[b] && B.flags[b][read - B.first[b]]) return true; }
	return false;
}

/* u of a read in a contig's set: (float)(draw >> 8) * 2^-24, draw = word 0 of Philox4x32-10 over (read lo, read hi, contig, 1) */
__host__ __device__ __forceinline__ float match_uniform(uint64_t seed, uint64_t read, uint32_t contig) {
	uint32_t c[4] = {(uint32_t)read, (uint32_t)(read >> 32), contig, 1u};
	philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
	return (float)(c[0] >> 8) * (1.0f / 16777216.0f);
}

__global__ void match_iota_kernel(uint32_t *perm, uint64_t n) {
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) perm[j] = (uint32_t)j;
}
__global__ void match_heads_kernel(const unsigned long long *key, uint64_t n, uint32_t *head) {
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) head[j] = (j == 0 || key[j] != key[j - 1]) ? 1u : 0u;
}
__global__ void match_compact_kernel(const unsigned long long *key, const uint32_t *perm, const unsigned long long *mate_in, const uint32_t *head, const uint64_t *hscan, uint64_t n,
                                     unsigned long long *ukey, unsigned long long *umate) {
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x)
		if (head[j]) { ukey[hscan[j]] = key[j]; umate[hscan[j]] = mate_in[perm[j]]; }
}
/* bound[c], c <= nc: the first of the n ascending records that is not below (c << MATCH_READ_BITS) */
__global__ void match_bounds_kernel(const unsigned long long *key, uint64_t n, uint64_t nc, uint64_t *bound) {
	for (uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; c <= nc; c += (uint64_t)gridDim.x * blockDim.x) {
		uint64_t lo = 0, hi = n;
		if (c >= nc) lo = n;
		const unsigned long long want = (unsigned long long)c << MATCH_READ_BITS;
		while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (key[mid] < want) lo = mid + 1; else hi = mid; }
		bound[c] = lo;
	}
}
/* keep[u]: the read stays in its set; cnt[u]: the records it leaves */
__global__ void match_sample_kernel(const unsigned long long *ukey, const unsigned long long *umate, uint64_t nu, const uint64_t *bound, uint32_t max_read_matches, uint32_t include_mate,
                                    uint64_t seed, uint32_t *keep, uint32_t *cnt) {
	const float maxHits = (float)(2.0 * (double)max_read_matches);      /* float maxHits = 2 * getMaxReadMatches() (KmerMatch.h:127) */
	for (uint64_t u = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; u < nu; u += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t c = (uint32_t)(ukey[u] >> MATCH_READ_BITS);
		const uint64_t size = bound[c + 1] - bound[c];
		bool k = true;
		if (max_read_matches && (float)(long long)size > maxHits)      /* size > maxHits, a long against a float (:168) */
			k = match_uniform(seed, ukey[u] & MATCH_READ_MASK, c) <= __fdiv_rn(maxHits, (float)(long long)size);
		keep[u] = k ? 1u : 0u;
		cnt[u] = k ? ((include_mate && umate[u] != MATCH_NO_MATE) ? 2u : 1u) : 0u;
	}
}
__global__ void match_emit_kernel(const unsigned long long *ukey, const unsigned long long *umate, uint64_t nu, const uint32_t *cnt, const uint64_t *escan, unsigned long long *out) {
	for (uint64_t u = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; u < nu; u += (uint64_t)gridDim.x * blockDim.x) {
		if (!cnt[u]) continue;
		out[escan[u]] = ukey[u];
		if (cnt[u] > 1) out[escan[u] + 1] = (ukey[u] & ~MATCH_READ_MASK) | umate[u];
	}
}
/* size[c] = scan[bound[c + 1]] - scan[bound[c]] (sizes after sampling: scan of keep; CSR offsets: with bound alone) */
__global__ void match_sizes_kernel(const uint64_t *bound, const uint64_t *scan, uint64_t nc, uint64_t *before, uint64_t *after) {
	for (uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; c < nc; c += (uint64_t)gridDim.x * blockDim.x) {
		before[c] = bound[c + 1] - bound[c];
		after[c] = scan[bound[c + 1]] - scan[bound[c]];
	}
}
__global__ void match_final_kernel(const unsigned long long *key, uint64_t n, MatchBatches B, uint32_t *flag) {
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x)
		flag[j] = ((j == 0 || key[j] != key[j - 1]) && !match_discarded(B, key[j] & MATCH_READ_MASK)) ? 1u : 0u;
}
__global__ void match_output_kernel(const unsigned long long *key, uint64_t n, const uint32_t *flag, const uint64_t *fscan, uint64_t *read_ids) {
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x)
		if (flag[j]) read_ids[fscan[j]] = key[j] & MATCH_READ_MASK;
}
/* offsets[c] = fscan[bound[c]], c <= nc */
__global__ void match_offsets_kernel(const uint64_t *bound, const uint64_t *fscan, uint64_t nc, uint64_t *offsets) {
	for (uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; c <= nc; c += (uint64_t)gridDim.x * blockDim.x) offsets[c] = fscan[bound[c]];
}

}  // namespace kmr
#endif

#endif
