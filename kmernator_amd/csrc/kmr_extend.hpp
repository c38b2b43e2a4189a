/*
 * kmr_extend.hpp -- HIP kernels (gfx950) of ContigExtender (src/ContigExtender.h:157-247 with minKmerSize == maxKmerSize, the way
 * apps/DistributedNucleatingAssembler.cpp:230-275 calls it, over KmerSpectrum::extendContig, src/KmerSpectrum.h:2311-2373): every
 * contig walks outwards base by base while the spectrum of its own pool of reads agrees.
 *
 * The reference builds a KmerSpectrum per contig and k, serially.  Here all (contig, pool) pairs of a call are one batched problem:
 *
 *  Gather   extend_item_kernel       item i of the gathered batch: the pool reads of contig c in pool order, then contig c itself
 *                                    (the "solid source"), i = pool_offsets[c] + c + slot; its length, contig and source
 *           extend_gather_kernel     the items' bases and qualities as one read batch, dealt out by output bytes (64 per thread);
 *                                    a contig, and a pool without qualities, gets Read::REF_QUAL throughout
 *  Extract  ExtendOp                 extract_kernel's Op: the canonical key and the f32 weight of every k-mer that passes the
 *                                    build's weight test (TrackingData::isDiscard) to slot koff[item] + position of a staging array
 *                                    of W + 1 words a slot that was filled with ones -- CompareOp's staging plus a weight word
 *  Order    extend_fill_kernel and sort_by_columns (kmr_sort.hip): (contig, source, key words), one stable pass per key word,
 *                                    the last word first, then one for (contig, source); stability keeps a key's sightings in
 *                                    arrival order (pool order, then position)
 *  Reduce   extend_reduce_kernel     one lane per (contig, source, key) run: count and weightedCount as the serial build makes them
 *                                    (src/KmerSpectrum.h:1590-1640, src/KmerTrackingData.h:427-448, :641-659): one f32 addition
 *                                    after the other, the first sighting quantised through the singleton map's byte where that
 *                                    map is on, nothing added from 65535 sightings on.  A longer run is the same loop, only slower
 *           extend_compact_kernel    per contig a table of weak entries and a table of solid keys, both ascending by key
 *           extend_bounds_kernel     where every contig's tables begin
 *  Extend   extend_contigs_kernel    one wavefront per contig, see below
 *  Result   extend_newlen_kernel, extend_result_kernel  the new sequences as a read batch of quality Read::REF_QUAL
 *
 * extend_contigs_kernel.  Both edge k-mers live in registers as Roller<W> (the left one reverse-complemented, so that a base in
 * front of it is a push too) and roll by one base per step; nothing is cut from the sequence again.  A step: lane 0 holds the edge
 * key, lanes 1-4 the four one-base extensions in the order A, C, G, T (KmerWeights::extendKmer(tmp, toRight, true), src/Kmer.h:
 * 1456-1480), each canonical; the five binary-search the contig's weak table; the values go to every lane by shuffle and every lane
 * makes the same decision in f64 (IEEE division __ddiv_rn, additions __dadd_rn: nothing to contract).  The exclusion test is a binary
 * search in the contig's solid table plus a wavefront-wide compare over the keys recorded in this call (recordKmer: the new edge
 * k-mer of every successful step, which is the candidate key itself), at most 2 * max_extend keys.
 * LDS: the recorded keys, 2 * max_extend * W * 8 bytes per wavefront, EXT_WAVES wavefronts per block: 3.1 KiB (W = 1) to 12.5 KiB
 * (W = 4) per block at the default max_extend of 50, so LDS never limits occupancy there; above EXT_LDS_WAVE_BYTES per wavefront the
 * list lives in global scratch instead (one piece per wavefront of the grid).  The kernel is a dependent chain of at most
 * 2 * max_extend steps of five table walks each: it is bound by latency, and only the number of contigs fills the device.
 *
 * A non-ACGT base of a contig is the 2-bit code 0 ('A'), as TwoBitSequence::compressSequence packs it (src/TwoBitSequence.cpp:242-
 * 269); a lower-case base is its upper-case one.
 */
#ifndef KMR_EXTEND_HPP_
#define KMR_EXTEND_HPP_

#include "kmr_kernels.hpp"

namespace kmr {

static const int EXT_WAVES = 4;
static const uint32_t EXT_LDS_WAVE_BYTES = 8192;               /* recorded keys of one wavefront that stay in LDS */
static const uint64_t EXT_STAGE_SLOTS = 1ull << 24;            /* staging slots of one run of whole contigs (kmr_tune "extend_stage_kmers") */
static const uint32_t EXT_COUNT_MAX = 65535u;
/* kmr_extend_stop_reason */
enum { EXT_STOP_LIMIT = 0, EXT_STOP_SHORT = 1, EXT_STOP_NO_EDGE = 2, EXT_STOP_COVERAGE = 3, EXT_STOP_AMBIGUOUS = 4, EXT_STOP_REPEAT = 5, EXT_STOP_INACTIVE = 6 };
enum { EXT_VALS = 6 };                                          /* edge, A, C, G, T, total */

template <int W> struct ExtendOp {
	uint64_t *stage;               /* [slots of the run][W + 1], all ones before the launch */
	const uint64_t *koff;          /* per item of the gathered batch: its first slot */
	uint64_t slot_base;            /* koff of the run's first item */
	static const bool NEEDS_WEIGHT = true;
	static const bool COUNTS_STATS = false;
	static const bool NEEDS_HASH = false;
	struct State {};
	__device__ __forceinline__ void wave_begin(State &, int) const {}
	__device__ __forceinline__ void wave_end(State &, int) const {}
	__device__ __forceinline__ void tile_begin(State &, uint32_t *, uint64_t, int) const {}
	__device__ __forceinline__ void tile_end(State &, uint64_t, int) const {}
	__device__ __forceinline__ void emit(State &, bool valid, const DevParams &, const Key<W> &key, uint64_t, const Occurrence &o,
	                                     uint64_t readIdx, uint32_t pos, unsigned &, bool &) const {
		if (valid) {
			uint64_t *d = stage + (koff[readIdx] - slot_base + pos) * (W + 1);
#pragma unroll
			for (int i = 0; i < W; i++) d[i] = key.w[i];
			d[W] = (uint64_t)__float_as_uint(o.w);
		}
	}
};
template <int W> __device__ __forceinline__ bool op_keeps_all_owners(const ExtendOp<W> &) { return true; }
template <int W> __device__ __forceinline__ uint32_t op_fail_code(const ExtendOp<W> &) { return 0; }

/* what extend_contigs_kernel reads and writes; contig c of the call is c0 + its index in the run */
struct ExtendArgs {
	const uint8_t *cbases; const uint64_t *coff; const uint8_t *active;
	uint64_t c0, m;
	const uint64_t *wkeys; const uint32_t *wcnt; const float *wval; const uint64_t *skeys;
	const uint64_t *bounds;        /* [m][4]: weak begin, weak end, solid begin, solid end */
	uint32_t k, max_extend, use_weights;
	double min_consensus, min_coverage, max_delta;
	uint8_t *seq;                  /* contig c's bases start at coff[c] + 2 * max_extend * c + max_extend */
	uint32_t *left, *right, *reason; double *vals;
	uint64_t *rec_global;          /* NULL: the recorded keys are in LDS */
};

#ifndef KMR_INSTANCE_TU
/* err bit 0: the offsets do not start at 0 or descend */
__global__ void extend_check_offsets_kernel(const uint64_t *po, uint64_t nc, uint32_t *err) {
	for (uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; c <= nc; c += (uint64_t)gridDim.x * blockDim.x)
		if (c == 0 ? po[0] != 0 : po[c] < po[c - 1]) atomicOr(err, 1u);
}
/* the contig of item i: the last c with po[c] + c <= i */
__device__ __forceinline__ uint64_t ext_item_contig(const uint64_t *po, uint64_t nc, uint64_t i) {
	uint64_t lo = 0, hi = nc;
	while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (po[mid] + mid <= i) lo = mid; else hi = mid; }
	return lo;
}
/* length, (contig << 1 | source) of every item; err bit 1: a pool index out of range, bit 2: a sequence of 2^31 - 1 bases or more */
__global__ void extend_item_kernel(const uint64_t *po, const uint64_t *pr, const uint8_t *active, const uint64_t *roff, uint64_t n_reads, const uint64_t *coff, uint64_t nc,
                                   uint64_t n_items, uint32_t *len, uint32_t *grp, uint32_t *err) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_items; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t c = ext_item_contig(po, nc, i);
		const bool self = i == po[c + 1] + c;
		uint64_t L = 0;
		if (self) L = coff[c + 1] - coff[c];
		else {
			const uint64_t r = pr[i - c];
			if (r >= n_reads) atomicOr(err, 2u); else L = roff[r + 1] - roff[r];
		}
		if (L >= 0x7fffffffull) { atomicOr(err, 4u); L = 0; }
		len[i] = (active && !active[c]) ? 0u : (uint32_t)L;
		grp[i] = (uint32_t)(c << 1) | (self ? 1u : 0u);
	}
}
/* the gathered batch: 64 output bytes per thread */
__global__ void extend_gather_kernel(const uint64_t *goff, uint64_t n_items, uint64_t total, const uint64_t *po, const uint64_t *pr, const uint32_t *grp,
                                     const uint8_t *rbases, const uint8_t *rquals, const uint64_t *roff, const uint8_t *cbases, const uint64_t *coff, uint8_t *ob, uint8_t *oq) {
	const uint64_t chunks = (total + 63) >> 6;
	for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < chunks; t += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t b0 = t << 6, b1 = b0 + 64 < total ? b0 + 64 : total;
		uint64_t lo = 0, hi = n_items;                /* the last item with goff[item] <= b0 */
		while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (goff[mid] <= b0) lo = mid; else hi = mid; }
		uint64_t i = lo;
		for (uint64_t b = b0; b < b1;) {
			while (goff[i + 1] <= b) i++;             /* empty items are stepped over; goff[n_items] = total > b */
			const uint32_t g = grp[i];
			const uint64_t c = g >> 1, e = goff[i + 1] < b1 ? goff[i + 1] : b1;
			const bool self = g & 1u;
			const uint64_t src = (self ? coff[c] : roff[pr[i - c]]) + (b - goff[i]);
			const uint8_t *sb = self ? cbases : rbases;
			const uint8_t *sq = (self || !rquals) ? nullptr : rquals;
			for (uint64_t x = 0; x < e - b; x++) { ob[b + x] = sb[src + x]; oq[b + x] = sq ? sq[src + x] : (uint8_t)127; }
			b = e;
		}
	}
}
/* slot j of the run: the item it lies in -- its group -- and the identity permutation */
__global__ void extend_fill_kernel(const uint64_t *koff, uint64_t i0, uint64_t mi, const uint32_t *grp, uint64_t S, uint32_t *sgrp, uint32_t *perm) {
	const uint64_t base = koff[i0];
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < S; j += (uint64_t)gridDim.x * blockDim.x) {
		uint64_t lo = 0, hi = mi;                     /* the last item of the run whose first slot is not behind j: it has slots */
		while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (koff[i0 + mid] - base <= j) lo = mid; else hi = mid; }
		sgrp[j] = grp[i0 + lo];
		perm[j] = (uint32_t)j;
	}
}
__device__ __forceinline__ bool ext_same_run(const uint64_t *stage, uint32_t words, const uint32_t *sgrp, uint32_t p, uint32_t q) {
	bool same = sgrp[p] == sgrp[q];
	for (uint32_t w = 0; w < words && same; w++) same = stage[(uint64_t)p * (words + 1) + w] == stage[(uint64_t)q * (words + 1) + w];
	return same;
}
/* sorted slot j that opens a run: the run's count and weightedCount; wflag: a weak entry of its contig's pool spectrum, sflag: a key
 * of its contig's solid spectrum.  singletons: a key seen once lives in the singleton map, which extendContig does not read */
__global__ void extend_reduce_kernel(const uint64_t *stage, uint32_t words, const uint32_t *sgrp, const uint32_t *perm, uint64_t S, uint32_t singletons,
                                     uint32_t *wflag, uint32_t *sflag, uint32_t *cnt, float *val) {
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < S; j += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t p = perm[j];
		uint32_t wf = 0, sf = 0;
		bool head = j == 0 || !ext_same_run(stage, words, sgrp, p, perm[j - 1]);
		if (head) {
			bool sentinel = true;
			for (uint32_t w = 0; w < words; w++) sentinel = sentinel && stage[(uint64_t)p * (words + 1) + w] == ~0ull;
			head = !sentinel;
		}
		if (head && (sgrp[p] & 1u)) sf = 1;
		else if (head) {
			const float w0 = __uint_as_float((uint32_t)stage[(uint64_t)p * (words + 1) + words]);
			uint32_t n = 1; float wc;
			if (singletons) {                         /* TrackingDataSingleton::track, then weak = singleton at the second sighting */
				const uint32_t q = ((uint32_t)(unsigned char)__dmul_rn((double)w0, 254.0) + 1u) & 0xffu;
				wc = q == 0 ? 0.0f : (float)__ddiv_rn((double)(q - 1), 254.0);
				if (q == 0) n = 0;
			} else wc = __fadd_rn(0.0f, w0);
			uint64_t sightings = 1;
			for (uint64_t x = j + 1; x < S && ext_same_run(stage, words, sgrp, p, perm[x]); x++) {
				sightings++;
				if (n < EXT_COUNT_MAX) { n++; wc = __fadd_rn(wc, __uint_as_float((uint32_t)stage[(uint64_t)perm[x] * (words + 1) + words])); }
			}
			if (!singletons || sightings > 1) { wf = 1; cnt[j] = n; val[j] = wc; }
		}
		wflag[j] = wf; sflag[j] = sf;
	}
}
__global__ void extend_compact_kernel(const uint64_t *stage, uint32_t words, const uint32_t *perm, uint64_t S, const uint32_t *wflag, const uint32_t *sflag, const uint64_t *wscan,
                                      const uint64_t *sscan, const uint32_t *cnt, const float *val, uint64_t *wkeys, uint32_t *wcnt, float *wval, uint64_t *skeys) {
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < S; j += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t *key = stage + (uint64_t)perm[j] * (words + 1);
		if (wflag[j]) { const uint64_t d = wscan[j]; for (uint32_t w = 0; w < words; w++) wkeys[d * words + w] = key[w]; wcnt[d] = cnt[j]; wval[d] = val[j]; }
		if (sflag[j]) { const uint64_t d = sscan[j]; for (uint32_t w = 0; w < words; w++) skeys[d * words + w] = key[w]; }
	}
}
/* sgsorted: the groups of the sorted slots, ascending.  bounds[r] of contig c0 + r: its weak entries and its solid keys */
__global__ void extend_bounds_kernel(const unsigned long long *sgsorted, uint64_t S, const uint64_t *wscan, const uint64_t *sscan, uint64_t c0, uint64_t m, uint64_t *bounds) {
	for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < m; r += (uint64_t)gridDim.x * blockDim.x) {
		uint64_t at[3];
		for (int t = 0; t < 3; t++) {
			const unsigned long long want = ((unsigned long long)(c0 + r) << 1) + (unsigned)t;
			uint64_t lo = 0, hi = S;
			while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (sgsorted[mid] < want) lo = mid + 1; else hi = mid; }
			at[t] = lo;
		}
		bounds[4 * r] = wscan[at[0]]; bounds[4 * r + 1] = wscan[at[1]]; bounds[4 * r + 2] = sscan[at[1]]; bounds[4 * r + 3] = sscan[at[2]];
	}
}
__global__ void extend_newlen_kernel(const uint64_t *coff, uint64_t nc, const uint32_t *left, const uint32_t *right, uint32_t *newlen, unsigned long long *info) {
	unsigned long long ext = 0, added = 0;
	for (uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; c < nc; c += (uint64_t)gridDim.x * blockDim.x) {
		newlen[c] = (uint32_t)(coff[c + 1] - coff[c]) + left[c] + right[c];
		ext += (left[c] + right[c]) ? 1u : 0u; added += left[c] + right[c];
	}
	ext = wave_sum(ext); added = wave_sum(added);
	if ((threadIdx.x & 63) == 0 && ext) { atomicAdd(&info[0], ext); atomicAdd(&info[1], added); }
}
/* the result batch: 64 output bytes per thread */
__global__ void extend_result_kernel(const uint64_t *noff, uint64_t nc, uint64_t total, const uint8_t *seq, const uint64_t *coff, const uint32_t *left, uint32_t max_extend, uint8_t *ob, uint8_t *oq) {
	const uint64_t chunks = (total + 63) >> 6;
	for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < chunks; t += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t b0 = t << 6, b1 = b0 + 64 < total ? b0 + 64 : total;
		uint64_t lo = 0, hi = nc;
		while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (noff[mid] <= b0) lo = mid; else hi = mid; }
		uint64_t c = lo;
		for (uint64_t b = b0; b < b1;) {
			while (noff[c + 1] <= b) c++;
			const uint64_t e = noff[c + 1] < b1 ? noff[c + 1] : b1;
			const uint64_t src = coff[c] + 2ull * max_extend * c + max_extend - left[c] + (b - noff[c]);
			for (uint64_t x = 0; x < e - b; x++) { ob[b + x] = seq[src + x]; oq[b + x] = (uint8_t)127; }
			b = e;
		}
	}
}
#endif

/* a base as Read::getFasta gives it back: a base that packs to two bits in upper case, '.' as 'N', any other markup as it is */
__device__ __forceinline__ uint8_t ext_fasta_char(uint8_t ch) {
	if (base_code(ch) != 4) return (uint8_t)(ch & 0xDFu);
	return ch == '.' ? (uint8_t)'N' : ch;
}
template <int W> __device__ __forceinline__ Key<W> ext_canonical(const Roller<W> &r) {
	const Key<W> kf = r.getFwd(), kr = r.getRc();
	return key_le<W>(kf, kr) ? kf : kr;
}
/* the first of the ascending keys [lo, hi) at `keys` that is not below `key` (hi: there is none) */
template <int W> __device__ __forceinline__ uint64_t ext_find(const uint64_t *keys, uint64_t lo, uint64_t hi, const Key<W> &key) {
	while (lo < hi) {
		const uint64_t mid = (lo + hi) >> 1;
		Key<W> t;
#pragma unroll
		for (int i = 0; i < W; i++) t.w[i] = keys[mid * W + i];
		if (key_lt<W>(t, key)) lo = mid + 1; else hi = mid;
	}
	return lo;
}

/* One step of KmerSpectrum::extendContig for one side, the same in every lane.  roll: the side's edge k-mer (the left one reverse-
 * complemented).  Returns true and rolls on where the contig grew by `base`; else `reason` says why not.  v: the step's values */
template <int W>
__device__ __forceinline__ bool ext_step(const ExtendArgs &A, Roller<W> &roll, bool toRight, uint64_t len, uint64_t wlo, uint64_t whi, uint64_t slo, uint64_t shi,
                                         uint64_t *rec, uint32_t &nrec, int lane, uint32_t &reason, double *v, uint32_t &base) {
#pragma unroll
	for (int i = 0; i < EXT_VALS; i++) v[i] = 0.0;
	if (len <= A.k) { reason = EXT_STOP_SHORT; return false; }
	const uint32_t mine = (uint32_t)(lane - 1) & 3u;
	Roller<W> cand = roll;
	cand.push(toRight ? mine : 3u - mine);
	const Key<W> key = lane == 0 ? ext_canonical<W>(roll) : ext_canonical<W>(cand);
	double val = 0.0;
	if (lane < 5) {
		const uint64_t e = (uint64_t)ext_find<W>(A.wkeys, wlo, whi, key);
		bool hit = e < whi;
		if (hit) {
#pragma unroll
			for (int i = 0; i < W; i++) hit = hit && A.wkeys[e * W + i] == key.w[i];
		}
		if (hit) val = A.use_weights ? (double)A.wval[e] : (double)A.wcnt[e];
	}
	const double edge = __shfl(val, 0, 64);
	if (edge == 0.0) { reason = EXT_STOP_NO_EDGE; return false; }
	double ext[4], total = 0.0;
#pragma unroll
	for (int i = 0; i < 4; i++) { ext[i] = __shfl(val, 1 + i, 64); total = __dadd_rn(total, ext[i]); }
	v[0] = edge; v[1] = ext[0]; v[2] = ext[1]; v[3] = ext[2]; v[4] = ext[3]; v[5] = total;
	if (!(total >= A.min_coverage && __ddiv_rn(total, edge) > A.max_delta)) { reason = EXT_STOP_COVERAGE; return false; }
	int pick = -1;
#pragma unroll
	for (int i = 0; i < 4; i++) if (pick < 0 && __ddiv_rn(ext[i], total) >= A.min_consensus) pick = i;
	if (pick < 0) { reason = EXT_STOP_AMBIGUOUS; return false; }
	Key<W> ck;
#pragma unroll
	for (int i = 0; i < W; i++) ck.w[i] = __shfl((unsigned long long)key.w[i], 1 + pick, 64);
	/* do not allow repeats: the contig's own solid k-mers, and the edge k-mers this call has recorded for it on either side */
	bool repeat = false;
	{
		const uint64_t e = (uint64_t)ext_find<W>(A.skeys, slo, shi, ck);
		bool hit = e < shi;
		if (hit) {
#pragma unroll
			for (int i = 0; i < W; i++) hit = hit && A.skeys[e * W + i] == ck.w[i];
		}
		bool seen = false;
		for (uint32_t r = (uint32_t)lane; r < nrec; r += 64) {
			bool eq = true;
#pragma unroll
			for (int i = 0; i < W; i++) eq = eq && rec[(uint64_t)r * W + i] == ck.w[i];
			seen = seen || eq;
		}
		repeat = hit || __any(seen ? 1 : 0);
	}
	if (repeat) { reason = EXT_STOP_REPEAT; return false; }
	roll.push(toRight ? (uint32_t)pick : 3u - (uint32_t)pick);
	if (lane == 0) {
#pragma unroll
		for (int i = 0; i < W; i++) rec[(uint64_t)nrec * W + i] = ck.w[i];
	}
	nrec++;
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	base = (uint32_t)pick;
	return true;
}

/* ContigExtender::extendContigs for the contigs of one run: one wavefront per contig (see the head of this file) */
template <int W>
__global__ __launch_bounds__(EXT_WAVES * 64)
void extend_contigs_kernel(ExtendArgs A) {
	extern __shared__ __attribute__((aligned(16))) uint8_t ext_smem[];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint64_t rec_words = 2ull * A.max_extend * W;
	uint64_t *rec = A.rec_global ? A.rec_global + ((uint64_t)blockIdx.x * EXT_WAVES + wave) * rec_words : (uint64_t *)ext_smem + (uint64_t)wave * rec_words;
	for (uint64_t r = (uint64_t)blockIdx.x * EXT_WAVES + wave; r < A.m; r += (uint64_t)gridDim.x * EXT_WAVES) {
		const uint64_t c = A.c0 + r, b = A.coff[c], L = A.coff[c + 1] - b;
		uint8_t *out = A.seq + b + 2ull * A.max_extend * c + A.max_extend;
		for (uint64_t i = (uint64_t)lane; i < L; i += 64) out[i] = ext_fasta_char(A.cbases[b + i]);
		uint32_t reasonL = EXT_STOP_LIMIT, reasonR = EXT_STOP_LIMIT, lt = 0, rt = 0, nrec = 0;
		double vL[EXT_VALS], vR[EXT_VALS];
#pragma unroll
		for (int i = 0; i < EXT_VALS; i++) vL[i] = vR[i] = 0.0;
		if (A.active && !A.active[c]) reasonL = reasonR = EXT_STOP_INACTIVE;
		else if (L < A.k) { if (A.max_extend) reasonL = reasonR = EXT_STOP_SHORT; }      /* the loop's `len < minKmerSize` break: no step is tried */
		else {
			const uint64_t wlo = A.bounds[4 * r], whi = A.bounds[4 * r + 1], slo = A.bounds[4 * r + 2], shi = A.bounds[4 * r + 3];
			Roller<W> rollL, rollR;
			rollL.init(A.k); rollR.init(A.k);
			for (uint32_t i = 0; i < A.k; i++) {
				uint32_t cl = base_code(A.cbases[b + (A.k - 1 - i)]), cr = base_code(A.cbases[b + L - A.k + i]);
				if (cl == 4) cl = 0;
				if (cr == 4) cr = 0;
				rollL.push(3u - cl); rollR.push(cr);
			}
			bool goL = true, goR = true;
			uint32_t iteration = 0;
			uint64_t len = L;
			while (iteration++ < A.max_extend && (goL || goR)) {
				uint32_t base;
				if (goL) {
					goL = ext_step<W>(A, rollL, false, len, wlo, whi, slo, shi, rec, nrec, lane, reasonL, vL, base);
					if (goL) { lt++; len++; if (lane == 0) out[-(int64_t)lt] = (uint8_t)"ACGT"[base]; }
				}
				if (goR) {
					goR = ext_step<W>(A, rollR, true, len, wlo, whi, slo, shi, rec, nrec, lane, reasonR, vR, base);
					if (goR) { if (lane == 0) out[L + rt] = (uint8_t)"ACGT"[base]; rt++; len++; }
				}
			}
		}
		if (lane == 0) {
			A.left[c] = lt; A.right[c] = rt;
			A.reason[2 * c] = reasonL; A.reason[2 * c + 1] = reasonR;
#pragma unroll
			for (int i = 0; i < EXT_VALS; i++) { A.vals[(2 * c) * EXT_VALS + i] = vL[i]; A.vals[(2 * c + 1) * EXT_VALS + i] = vR[i]; }
		}
		__builtin_amdgcn_wave_barrier();              /* all lanes are done with the recorded keys before the next contig's arrive */
	}
}

}  // namespace kmr
#endif
