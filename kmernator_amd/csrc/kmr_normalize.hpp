/*
 * kmr_normalize.hpp -- coverage normalization of FilterReads' output on the device: the `if (maximumKmerDepth > 0)` branch of
 * selectReads (apps/FilterReads.h:178-206, --max-kmer-output-depth) with --normalization-method RANDOM.
 *
 * Replaces ReadSelector::pickCoverageNormalizedSubset and chooseRead (src/ReadSelector.h:661-749), optimizePickOrder (:1212-1221)
 * and writePicks (:1242-1262).  Unlike the two branches of kmr_select.hpp a pick is a PAIR here: it is written read1 then read2,
 * picks are ordered by the lower read index of the pair (Pair::operator<, src/ReadSet.h:118-123), so the output interleaves mates
 * whatever their indices are, and every record goes to the file of its own read's input.  The decision draws random numbers: the
 * reference's come from one mt19937 per OpenMP thread seeded with the time; here draw(g) is word 0 of Philox4x32-10 over the counter
 * (g, 0, 0) and the key seed, g the global index of a read, so that a result depends on (seed, g) alone.
 *
 *   normalize_mark_kernel      per pair of the list: its indices are -1 or inside the batch and not both -1; every read it names is
 *                              counted (a read no pair names is a half pair of its own, a read two pairs name is an error)
 *   normalize_classify_kernel  per pair, and per read no pair names: the decision; every read of a pick goes to slot
 *                              2 * (lower read index of the pick) + (0 for the read1 side, 1 for the read2 side) with its input
 *                              file, record bytes and printed name length (sel_measure)
 *   normalize_count_kernel     per unit of slots the picks and bytes of every input file, summed in LDS
 *   partition_scan_kernel      (kmr_select.hpp) exclusive scan of the [input][unit] matrices, the segment table and the totals
 *   partition_rank_kernel      (kmr_select.hpp) over slots instead of reads: a slot's pick index and byte offset; pick_read takes
 *                              the read of the slot
 *   select_write_kernel        (kmr_select.hpp) unchanged
 * Slots in ascending order are the picks in the reference's order, read1 before read2 inside a pick; split by input file that is a
 * stable partition of the 2 n slots, which the units of kmr_select.hpp already compute for reads.  Five memsets, five launches and
 * the writer whatever the batch; one host wait for the totals.
 */
#ifndef KMR_NORMALIZE_HPP_
#define KMR_NORMALIZE_HPP_

#include "kmr_select.hpp"

namespace kmr {

/* Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of two 32 x 32 -> 64
 * multiplications, the key bumped by the Weyl constants between rounds.  Integers only, no table. */
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
	for (int r = 0; r < 10; r++) {
		const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
		const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
		c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
		k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
	}
}
/* the draw of global read index g: what IntRand::rand() is to chooseRead (:665) */
__host__ __device__ __forceinline__ uint32_t norm_draw(uint64_t seed, uint64_t g) {
	uint32_t c[4] = {(uint32_t)g, (uint32_t)(g >> 32), 0u, 0u};
	philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
	return c[0];
}

struct NormalizeParams {
	const int64_t *read1, *read2;      /* the pair list, -1 = no read on that side; not read when n_pairs is 0 */
	uint64_t n_pairs;
	uint64_t target, seed, first_global;
	uint32_t by_pair;
};

/* (long) of a read's score (:685-686).  The cast truncates; a float beyond the range of a long, where the reference's cast is
 * undefined, saturates */
__device__ __forceinline__ long long norm_score(const SelectParams &P, int64_t i) {
	if (i < 0 || !sel_passing(P, (uint64_t)i)) return -1;
	const float s = P.score[i];
	if (s >= 9223372036854775808.0f) return 0x7fffffffffffffffll;
	if (s <= -9223372036854775808.0f) return -0x7fffffffffffffffll - 1;
	return (long long)s;
}
/* chooseRead(score, targetDepth, false) (:661-672) for a score > 0: kept for certain up to the target, else with the inclusive
 * compare of :669.  cnt[1] counts the calls, cnt[2] those that drew */
__device__ __forceinline__ bool norm_choose(const NormalizeParams &N, long long s, uint64_t read, unsigned long long *cnt) {
	cnt[1]++;
	if ((uint64_t)s <= N.target) return true;
	cnt[2]++;
	return (uint64_t)norm_draw(N.seed, N.first_global + read) % (uint64_t)s <= N.target;
}
__device__ __forceinline__ bool norm_index_ok(int64_t r, uint64_t n) { return r >= -1 && (r < 0 || (uint64_t)r < n); }

__global__ __launch_bounds__(256)
void normalize_mark_kernel(NormalizeParams N, uint64_t n, uint32_t *named, uint32_t *err) {
	for (uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; p < N.n_pairs; p += (uint64_t)gridDim.x * blockDim.x) {
		const int64_t a = N.read1[p], b = N.read2[p];
		if (!norm_index_ok(a, n) || !norm_index_ok(b, n) || (a < 0 && b < 0)) { atomicOr(err, (uint32_t)SEL_ERR_PAIR); continue; }
		if (a >= 0 && atomicAdd(&named[a], 1u)) atomicOr(err, (uint32_t)SEL_ERR_TWICE);
		if (b >= 0 && atomicAdd(&named[b], 1u)) atomicOr(err, (uint32_t)SEL_ERR_TWICE);
	}
}

/* Items are the pairs of the list and then the reads of the batch, of which those no pair names stand as (read, -1).  counters:
 * picks (pairs, the reference's return value), chooseRead calls, draws.  picked is zero, read_seg and slot_seg are -1 on entry. */
__global__ __launch_bounds__(256)
void normalize_classify_kernel(SelectParams P, NormalizeParams N, PartitionParams Q, const uint32_t *named, uint32_t *slot_read, int32_t *slot_seg, uint32_t *slot_len,
                               uint32_t *name_printed, uint8_t *picked, int32_t *read_seg, unsigned long long *counters, uint32_t *err) {
	unsigned long long cnt[3] = {0, 0, 0};
	for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < N.n_pairs + P.n; t += (uint64_t)gridDim.x * blockDim.x) {
		int64_t a, b = -1;
		if (t < N.n_pairs) {
			a = N.read1[t]; b = N.read2[t];
			if (!norm_index_ok(a, P.n) || !norm_index_ok(b, P.n) || (a < 0 && b < 0)) continue;      /* reported by normalize_mark_kernel */
		} else {
			a = (int64_t)(t - N.n_pairs);
			if (named[a]) continue;
		}
		const long long s1 = norm_score(P, a), s2 = norm_score(P, b);
		bool keep1 = false, keep2 = false;
		if (N.by_pair) {
			const bool p1 = a >= 0 && sel_passing(P, (uint64_t)a), p2 = b >= 0 && sel_passing(P, (uint64_t)b);
			if (!((a >= 0 && b >= 0 && P.both_pass) ? (p1 && p2) : (p1 || p2))) continue;      /* isPassingPair :558-568 */
			if (P.both_pass && (s1 <= 0 || s2 <= 0)) continue;                                  /* :697-702: also every half pair */
			if (s1 <= 0 && s2 <= 0) continue;                                                   /* :703-706 */
			const uint64_t lower = a < 0 ? (uint64_t)b : (b < 0 ? (uint64_t)a : (uint64_t)(a < b ? a : b));
			if (!norm_choose(N, s1 > s2 ? s1 : s2, lower, cnt)) continue;
			keep1 = a >= 0; keep2 = b >= 0;      /* the whole pair, a failed or discarded mate included */
		} else {
			keep1 = s1 > 0 && norm_choose(N, s1, (uint64_t)a, cnt);      /* :716-733 */
			keep2 = s2 > 0 && norm_choose(N, s2, (uint64_t)b, cnt);
			if (!keep1 && !keep2) continue;
		}
		cnt[0]++;
		const uint64_t lower = !keep1 ? (uint64_t)b : (!keep2 ? (uint64_t)a : (uint64_t)(a < b ? a : b));      /* Pair::lesser over the pick's reads */
		for (int side = 0; side < 2; side++) {
			if (!(side ? keep2 : keep1)) continue;
			const uint64_t r = (uint64_t)(side ? b : a), slot = 2 * lower + side;
			int32_t seg = 0;
			if (Q.n_inputs > 1) {      /* the last input that starts at or before r */
				uint32_t lo = 0, hi = Q.n_inputs;
				while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (Q.input_starts[mid] <= r) lo = mid; else hi = mid; }
				seg = (int32_t)lo;
			}
			uint32_t nlen = 0;
			const uint32_t bytes = sel_measure(P, r, &nlen, err);
			slot_read[slot] = (uint32_t)r; slot_seg[slot] = seg; slot_len[slot] = bytes;
			name_printed[r] = nlen; picked[r] = 1; read_seg[r] = seg;
		}
	}
	for (int k = 0; k < 3; k++) {
		unsigned long long v = cnt[k];
		for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
		if ((threadIdx.x & 63) == 0 && v) atomicAdd(&counters[k], v);
	}
}

/* what partition_classify_kernel leaves per unit, over slots: unit_cnt / unit_bytes [input][unit] */
__global__ __launch_bounds__(SEL_UNIT)
void normalize_count_kernel(const int32_t *slot_seg, const uint32_t *slot_len, uint64_t n_slots, PartitionParams Q, uint32_t *unit_cnt, unsigned long long *unit_bytes) {
	__shared__ uint32_t s_cnt[SEL_MAX_SEGMENTS];
	__shared__ unsigned long long s_bytes[SEL_MAX_SEGMENTS];
	const uint32_t lane = threadIdx.x, u = blockIdx.x;
	for (uint32_t s = lane; s < Q.n_segments; s += SEL_UNIT) { s_cnt[s] = 0; s_bytes[s] = 0; }
	__syncthreads();
	const uint64_t lo = (uint64_t)u * Q.per_unit, hi = lo + Q.per_unit < n_slots ? lo + Q.per_unit : n_slots;
	for (uint64_t i = lo + lane; i < hi; i += SEL_UNIT) {
		const int32_t seg = slot_seg[i];
		if (seg >= 0) { atomicAdd(&s_cnt[seg], 1u); atomicAdd(&s_bytes[seg], (unsigned long long)slot_len[i]); }
	}
	__syncthreads();
	for (uint32_t s = lane; s < Q.n_segments; s += SEL_UNIT) { unit_cnt[(size_t)s * Q.n_units + u] = s_cnt[s]; unit_bytes[(size_t)s * Q.n_units + u] = s_bytes[s]; }
}

}  // namespace kmr
#endif
