/*
 * kmr_dedup.hpp -- DuplicateFragmentFilter::_filterDuplicateFragments (src/DuplicateFragmentFilter.h:505-559) of one
 * device-resident batch on the device, with edit distance 0, consensus on and cutoff 2: fragments whose first bases agree
 * are collapsed to consensus reads and their reads are discarded.  One call is one pass (the paired one or the --dedup-single
 * one) over the pair list kmr_identify_pairs* left on the device, in the order a single-threaded reference visits it.
 *
 *   dedup_key_kernel        one lane per pair record (_buildDuplicateFragmentMap, :194-279): the skip tests (discarded, shorter
 *                           than start_offset + L up to the first X, unpaired for this pass), the 2-bit key of the window(s), its
 *                           reverse complement on the key words, the canonical choice of dedup_mode 2 and the flip flag
 *   (scan of the candidate flags, dedup_compact_kernel: candidate -> its position in the pair list)
 *   sort_by_columns         (kmr_sort.hip) one stable radix sort per key word from the last to the first, the payload being the
 *                           pair position, which gathers the next word: members of one key end up adjacent and in ascending
 *                           pair position (the instance order of a serial build, src/KmerTrackingData.h:810-841)
 *   dedup_heads_kernel      where the key changes
 *   (scan) group_starts, dedup_keep_kernel, (scan) dedup_kept_kernel: group sizes, the groups of 2 and more, each with the
 *                           pair position of its first member (the smallest of the group, the sort being stable)
 *   (sort of (first member, group): the order the consensus reads come out in)
 *   dedup_size_kernel       per (group, side): the longest member, the exact length of the name "C<m>-<name of the first member>"
 *   (two scans: base offsets and name offsets of the consensus batch; one copy brings the totals back)
 *   dedup_consensus_kernel  one wavefront per (group, side): ReadSet::getConsensusRead (src/ReadSet.cpp:572-629 over
 *                           Read::getProbabilityBases and ProbabilityBase, src/Sequence.cpp:563-582, 807-967), lanes taking
 *                           consecutive positions, members walked in order with the sums in fp64 registers; and the name
 *   dedup_discard_kernel    every read of every member of a collapsed group becomes discarded (:475-491)
 *
 * ProbabilityBase as the kernel restates it, per position and member in member order: the copy constructor inside operator+
 * (src/Sequence.h:313-315) first raises `top` to the largest of the running sums (setTop(*this)); a member that is still being
 * read at this position (no quality below the minimum at or before it: the loop of getProbabilityBases breaks there) adds prob
 * to the base it shows and (1 - prob) / 3.0 to the other three, one to count, and setTop(other) raises `top` to its largest
 * single contribution.  prob and (1 - prob) / 3.0 come from a 256-entry table made on the host, and getQualChar's
 * (char)(-10. * log10(1.0 - prob)) is a comparison against the 39 doubles at which that expression steps (kmr_consensus_qual):
 * the device neither divides nor takes a logarithm.
 *
 * One wavefront walks a whole group and one lane a whole group's sizes, so a batch in which very many fragments share one key is
 * slow (not wrong).  The number of launches and stream waits does not depend on the number of reads.
 *
 * Not covered: the order of the consensus reads among themselves (the reference's follows the bucket iteration of its map and,
 * under OpenMP, the thread that met the group; here: ascending position of the first member); dedup-edit-distance 1;
 * dedup-consensus 0; keys of more than 128 bases; the artifact filter's run over the new reads and reads.append (the caller's).
 */
#ifndef KMR_DEDUP_HPP_
#define KMR_DEDUP_HPP_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmr_pairs.hpp"

namespace kmr {

enum { DEDUP_ERR_NAME = 1 };
/* totals block (uint64 each): the four skip counters in the order of kmr_dedup_info, affected reads, the error word */
enum { DEDUP_T_DISCARD = 0, DEDUP_T_SHORT, DEDUP_T_UNPAIRED, DEDUP_T_INVALID, DEDUP_T_AFFECTED, DEDUP_T_ERR, DEDUP_T_WORDS };
static const int DEDUP_THREADS = 256, DEDUP_WAVES = DEDUP_THREADS / 64, DEDUP_QUALS = 39;

struct DedupParams {
	const uint8_t *bases, *quals;            /* the batch */
	const uint64_t *offsets, *name_off;
	const uint32_t *name_len;
	const uint8_t *text; uint64_t text_len;  /* what name_off / name_len point into */
	uint64_t n, total;                       /* reads, bases */
	const int64_t *read1, *read2; uint64_t np;      /* the pair list */
	const uint8_t *discarded;                /* per read, may be null */
	uint32_t paired, mode2;
	uint32_t L, so, W;                       /* bases of one window (dedup_length, or twice that in the single pass), start offset, key words */
	uint32_t sides;                          /* 2 in the paired pass, 1 in the single pass */
	uint32_t min_q;                          /* first quality character that is read: fastq_start_char + min_quality_score */
	uint32_t start_char;
};

/* what the host makes once per handle: prob[q] = max(qualityToProbability[q], 0.2501), other[q] = (1.0 - prob[q]) / 3.0, and
 * step[i] = the smallest double p with (char)(-10. * log10(1.0 - p)) >= i + 1 */
struct DedupTables { double prob[256], other[256], step[DEDUP_QUALS]; };

__device__ __forceinline__ uint32_t dedup_code(uint8_t c) {      /* TwoBitSequence::compressBase; anything else packs as 0 (compressSequence) */
	switch (c) { case 'C': case 'c': return 1u; case 'G': case 'g': return 2u; case 'T': case 't': return 3u; default: return 0u; }
}

/* Up to 128 bases as four big-endian words, base 0 in the two highest bits of k[0] (the byte order of TwoBitSequence), held in
 * four named registers: every index below is a compile-time constant */
struct DedupKey { uint64_t k[4]; };

/* The window [so, so + L) of read rid packed left-aligned into K; false if the read is shorter than so + L up to its first X
 * (getFirstMarkupXLength, src/Sequence.cpp:432-439).  Only the first so + L bases are read. */
__device__ __forceinline__ bool dedup_window(const DedupParams &P, uint64_t rid, DedupKey &K) {
	const uint64_t off = P.offsets[rid], len = P.offsets[rid + 1] - off;
	const uint32_t need = P.so + P.L;
	K.k[0] = K.k[1] = K.k[2] = K.k[3] = 0;
	if (len < need || off > P.total || len > P.total - off) return false;
	PairsBytes B(P.bases, P.total);
	for (uint32_t pos = 0; pos < need; pos++) {
		const uint8_t c = B.at(off + pos);
		if (c == 'X' || c == 'x') return false;
		if (pos < P.so) continue;
		const uint32_t t = pos - P.so;
		const uint64_t v = (uint64_t)dedup_code(c) << (62 - 2 * (t & 31));
		const uint32_t w = t >> 5;
		K.k[0] |= w == 0 ? v : 0; K.k[1] |= w == 1 ? v : 0; K.k[2] |= w == 2 ? v : 0; K.k[3] |= w == 3 ? v : 0;
	}
	return true;
}

__device__ __forceinline__ uint64_t dedup_rev2(uint64_t x) {      /* the 32 two-bit groups of x in reverse order */
	x = __brevll(x);
	return ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
}
/* K shifted right / left by s bits as one 256-bit number, s a multiple of 8 in [0, 256] */
__device__ __forceinline__ DedupKey dedup_shr(const DedupKey &K, uint32_t s) {
	const uint32_t ws = s >> 6, bs = s & 63;
	DedupKey R;
#pragma unroll
	for (int i = 0; i < 4; i++) {
		uint64_t hi = 0, lo = 0;      /* word i takes the low part of K[i - ws] and, if bs, the spill of K[i - ws - 1] */
#pragma unroll
		for (int j = 0; j < 4; j++) { lo = (uint32_t)(i - j) == ws ? K.k[j] : lo; hi = (uint32_t)(i - j) == ws + 1 ? K.k[j] : hi; }
		R.k[i] = bs ? (lo >> bs) | (hi << (64 - bs)) : lo;
	}
	return R;
}
__device__ __forceinline__ DedupKey dedup_shl(const DedupKey &K, uint32_t s) {
	const uint32_t ws = s >> 6, bs = s & 63;
	DedupKey R;
#pragma unroll
	for (int i = 0; i < 4; i++) {
		uint64_t hi = 0, lo = 0;
#pragma unroll
		for (int j = 0; j < 4; j++) { hi = (uint32_t)(j - i) == ws ? K.k[j] : hi; lo = (uint32_t)(j - i) == ws + 1 ? K.k[j] : lo; }
		R.k[i] = bs ? (hi << bs) | (lo >> (64 - bs)) : hi;
	}
	return R;
}
/* the reverse complement of the first `bases` bases of K, left-aligned again (TwoBitSequence::reverseComplement) */
__device__ __forceinline__ DedupKey dedup_revcomp(const DedupKey &K, uint32_t bases) {
	DedupKey R;
	R.k[0] = dedup_rev2(~K.k[3]); R.k[1] = dedup_rev2(~K.k[2]); R.k[2] = dedup_rev2(~K.k[1]); R.k[3] = dedup_rev2(~K.k[0]);
	return dedup_shl(R, 256 - 2 * bases);      /* the complemented padding leaves at the top */
}
__device__ __forceinline__ DedupKey dedup_or(const DedupKey &A, const DedupKey &B) {
	DedupKey R;
#pragma unroll
	for (int i = 0; i < 4; i++) R.k[i] = A.k[i] | B.k[i];
	return R;
}
/* memcmp order of the key bytes: A < B */
__device__ __forceinline__ bool dedup_less(const DedupKey &A, const DedupKey &B) {
	bool less = false, decided = false;
#pragma unroll
	for (int i = 0; i < 4; i++) { less = (!decided && A.k[i] < B.k[i]) ? true : less; decided = decided || A.k[i] != B.k[i]; }
	return less;
}

__device__ __forceinline__ bool dedup_is_discarded(const DedupParams &P, uint64_t rid) { return P.discarded && P.discarded[rid] != 0; }

/* keys: W planes of np words, plane w holding word w of every record's key; cand[i] = 1 if record i takes part; flip[i] = 1 if its
 * key is the reverse complement's (the member's read2 is side 1) */
__global__ __launch_bounds__(256)
void dedup_key_kernel(DedupParams P, unsigned long long *keys, uint32_t *cand, uint8_t *flip, uint64_t *totals) {
	uint32_t n_disc = 0, n_short = 0, n_unp = 0, n_inv = 0;
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < P.np; i += (uint64_t)gridDim.x * blockDim.x) {
		const int64_t r1 = P.read1[i], r2 = P.read2[i];
		const bool has1 = r1 >= 0, has2 = r2 >= 0;
		DedupKey K; K.k[0] = K.k[1] = K.k[2] = K.k[3] = 0;
		bool ok = false, fl = false;
		if (P.paired && has1 && has2) {
			DedupKey A, B;
			if ((uint64_t)r1 >= P.n || (uint64_t)r2 >= P.n) n_inv++;
			else if (dedup_is_discarded(P, (uint64_t)r1) || dedup_is_discarded(P, (uint64_t)r2)) n_disc++;
			else if (!dedup_window(P, (uint64_t)r1, A) || !dedup_window(P, (uint64_t)r2, B)) n_short++;      /* read 1 is tested first; one count per pair */
			else {
				/* read1's window, then the reverse complement of read2's (:217-226); the whole key's reverse complement is read2's
				 * window followed by the reverse complement of read1's */
				K = dedup_or(A, dedup_shr(dedup_revcomp(B, P.L), 2 * P.L));
				if (P.mode2) {
					const DedupKey R = dedup_or(B, dedup_shr(dedup_revcomp(A, P.L), 2 * P.L));
					if (dedup_less(R, K)) { K = R; fl = true; }      /* buildLeastComplement (src/Kmer.h:356-364): a tie keeps the forward key */
				}
				ok = true;
			}
		} else if (!P.paired && has1 != has2) {
			const uint64_t rid = (uint64_t)(has1 ? r1 : r2);
			if (rid >= P.n) n_inv++;
			else if (dedup_is_discarded(P, rid)) n_disc++;
			else if (!dedup_window(P, rid, K)) n_short++;
			else ok = true;
		} else n_unp++;
		cand[i] = ok ? 1u : 0u; flip[i] = fl ? 1 : 0;
		if (ok) {
			keys[i] = K.k[0];
			if (P.W > 1) keys[P.np + i] = K.k[1];
			if (P.W > 2) keys[2 * P.np + i] = K.k[2];
			if (P.W > 3) keys[3 * P.np + i] = K.k[3];
		}
	}
	n_disc = pairs_wave_sum(n_disc); n_short = pairs_wave_sum(n_short); n_unp = pairs_wave_sum(n_unp); n_inv = pairs_wave_sum(n_inv);
	if ((threadIdx.x & 63) == 0) {
		if (n_disc) atomicAdd((unsigned long long *)(totals + DEDUP_T_DISCARD), (unsigned long long)n_disc);
		if (n_short) atomicAdd((unsigned long long *)(totals + DEDUP_T_SHORT), (unsigned long long)n_short);
		if (n_unp) atomicAdd((unsigned long long *)(totals + DEDUP_T_UNPAIRED), (unsigned long long)n_unp);
		if (n_inv) atomicAdd((unsigned long long *)(totals + DEDUP_T_INVALID), (unsigned long long)n_inv);
	}
}

/* candidate -> its pair position, in ascending order: the payload the sorts carry */
__global__ __launch_bounds__(256)
void dedup_compact_kernel(const uint32_t *cand, const uint64_t *cand_scan, uint64_t np, uint32_t *perm) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < np; i += (uint64_t)gridDim.x * blockDim.x)
		if (cand[i]) perm[cand_scan[i]] = (uint32_t)i;
}

/* perm: the c candidates sorted by key, ascending pair position inside a key; head[j] = 1 where a new key begins */
__global__ __launch_bounds__(256)
void dedup_heads_kernel(const unsigned long long *keys, uint64_t np, uint32_t W, const uint32_t *perm, uint64_t c, uint32_t *head) {
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < c; j += (uint64_t)gridDim.x * blockDim.x) {
		bool h = j == 0;
		if (!h) { const uint32_t a = perm[j], b = perm[j - 1]; for (uint32_t w = 0; w < W; w++) h = h || keys[w * np + a] != keys[w * np + b]; }
		head[j] = h ? 1u : 0u;
	}
}

/* head_scan: exclusive scan of head, so head_scan[c] = the number of groups G; start (group_starts): start[g] = sorted index of group g's
 * first member, start[G] = c.  keep[g] = group g has at least two members (cutoffThreshold 2); 0 behind the last group */
__global__ __launch_bounds__(256)
void dedup_keep_kernel(const uint64_t *head_scan, const uint64_t *start, uint64_t c, uint32_t *keep) {
	const uint64_t G = head_scan[c];
	for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; g < c; g += (uint64_t)gridDim.x * blockDim.x)
		keep[g] = (g < G && start[g + 1] - start[g] >= 2) ? 1u : 0u;
}

/* the kept groups: (pair position of the first member, group) */
__global__ __launch_bounds__(256)
void dedup_kept_kernel(const uint32_t *keep, const uint64_t *keep_scan, const uint64_t *start, const uint32_t *perm, uint64_t c, unsigned long long *first, uint32_t *group) {
	for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; g < c; g += (uint64_t)gridDim.x * blockDim.x)
		if (keep[g]) { const uint64_t p = keep_scan[g]; first[p] = perm[start[g]]; group[p] = (uint32_t)g; }
}

/* what the later kernels need of the grouping */
struct DedupGroups {
	const uint32_t *perm; const uint8_t *flip;      /* sorted candidate -> pair position; per pair position */
	const uint64_t *start;                          /* group -> sorted index of its first member */
	const uint32_t *ogroup; uint64_t K;             /* the kept groups in output order */
};

/* the read a member (pair position pos) contributes to `side`: side 0 is read1, or read2 of a flipped member (:450-457) */
__device__ __forceinline__ uint64_t dedup_member_read(const DedupParams &P, const DedupGroups &G, uint32_t pos, uint32_t side) {
	const int64_t r1 = P.read1[pos], r2 = P.read2[pos];
	if (!P.paired) return (uint64_t)(r1 >= 0 ? r1 : r2);
	return (uint64_t)(((side != 0) != (G.flip[pos] != 0)) ? r2 : r1);
}
__device__ __forceinline__ uint32_t dedup_digits(uint64_t v) { uint32_t d = 1; for (; v >= 10; v /= 10) d++; return d; }

/* per (kept group, side) t: length of the consensus read, bytes of its name with the newline behind it; per kept group: first member and size */
__global__ __launch_bounds__(256)
void dedup_size_kernel(DedupParams P, DedupGroups G, uint32_t *len, uint32_t *name_bytes, uint64_t *group_first, uint32_t *group_size, uint64_t *totals) {
	uint32_t affected = 0;
	for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < G.K * P.sides; t += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t og = t / P.sides; const uint32_t side = (uint32_t)(t % P.sides);
		const uint32_t g = G.ogroup[og];
		const uint64_t j0 = G.start[g], j1 = G.start[g + 1];
		uint64_t longest = 0;
		for (uint64_t j = j0; j < j1; j++) {
			const uint64_t rid = dedup_member_read(P, G, G.perm[j], side);
			const uint64_t l = P.offsets[rid + 1] - P.offsets[rid];
			longest = l > longest ? l : longest;
		}
		const uint64_t first = dedup_member_read(P, G, G.perm[j0], side);
		const uint64_t no = P.name_off[first]; const uint32_t nl = P.name_len[first];
		uint32_t nlen = 0;
		if (P.text_len == 0) nlen = 0;      /* a batch without names */
		else if (no > P.text_len || nl > P.text_len - no) atomicOr((unsigned long long *)(totals + DEDUP_T_ERR), (unsigned long long)DEDUP_ERR_NAME);
		else while (nlen < nl && P.text[no + nlen] != ' ' && P.text[no + nlen] != '\t') nlen++;
		len[t] = (uint32_t)longest; name_bytes[t] = 1 + dedup_digits(j1 - j0) + 1 + nlen + 1;
		if (side == 0) { group_first[og] = G.perm[j0]; group_size[og] = (uint32_t)(j1 - j0); affected += (uint32_t)(j1 - j0) * P.sides; }
	}
	affected = pairs_wave_sum(affected);
	if ((threadIdx.x & 63) == 0 && affected) atomicAdd((unsigned long long *)(totals + DEDUP_T_AFFECTED), (unsigned long long)affected);
}

/* ProbabilityBase::setTop (src/Sequence.cpp:886-903): strict <, in the order A C G T */
__device__ __forceinline__ void dedup_set_top(double &top, uint32_t &best, double a, double c, double g, double t) {
	if (top < a) { top = a; best = 'A'; }
	if (top < c) { top = c; best = 'C'; }
	if (top < g) { top = g; best = 'G'; }
	if (top < t) { top = t; best = 'T'; }
}

/* BaseQual::getQualChar (src/Sequence.cpp:811-819) without its offset: 40 from 0.9999, else how many of the steps prob has reached */
__device__ __forceinline__ uint32_t dedup_qual(const double *step, double prob) {
	if (prob >= 0.9999) return 40u;
	uint32_t q = 0;
	while (q < (uint32_t)DEDUP_QUALS && step[q] <= prob) q++;
	return q;
}

/* what the position loop needs of one member's read on one side, resolved once: where its bases lie, its length, and the position
 * at which the loop of Read::getProbabilityBases leaves it (the first quality below the minimum, or its length) */
struct DedupMember { uint64_t off; uint32_t len, stop; };

/* One wavefront per (kept group, side) t.  members: scratch of one DedupMember per (sorted candidate, side), written by the first
 * pass over the group and read by the position loop, so that the chain sorted position -> pair position -> read index -> offset
 * is walked once per member and not once per round of 64 positions.
 * offsets: base offsets of the consensus batch; name_scan: byte offsets of the names. */
__global__ __launch_bounds__(DEDUP_THREADS)
void dedup_consensus_kernel(DedupParams P, DedupGroups G, const DedupTables *T, const uint64_t *offsets, const uint64_t *name_scan, DedupMember *members,
                            uint8_t *out_bases, uint8_t *out_quals, uint8_t *names, uint64_t *out_name_off, uint32_t *out_name_len) {
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	for (uint64_t t = (uint64_t)blockIdx.x * DEDUP_WAVES + wave; t < G.K * P.sides; t += (uint64_t)gridDim.x * DEDUP_WAVES) {
		const uint64_t og = t / P.sides; const uint32_t side = (uint32_t)(t % P.sides);
		const uint32_t g = G.ogroup[og];
		const uint64_t j0 = G.start[g], j1 = G.start[g + 1];
		/* where each member stops being read */
		for (uint64_t j = j0; j < j1; j++) {
			const uint64_t rid = dedup_member_read(P, G, G.perm[j], side);
			const uint64_t off = P.offsets[rid]; const uint32_t l = (uint32_t)(P.offsets[rid + 1] - off);
			uint32_t s = l;
			for (uint32_t base = 0; base < l; base += 64) {
				const uint32_t pos = base + lane;
				const bool low = pos < l && P.quals[off + pos] < P.min_q;
				const unsigned long long b = __ballot(low);
				if (b) { s = base + (uint32_t)__ffsll((long long)b) - 1; break; }
			}
			if (lane == 0) { DedupMember M; M.off = off; M.len = l; M.stop = s; members[j * P.sides + side] = M; }
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
		const uint64_t o0 = offsets[t]; const uint32_t clen = (uint32_t)(offsets[t + 1] - o0);
		for (uint32_t base = 0; base < clen; base += 64) {
			const uint32_t pos = base + lane;
			double a = 0.0, c = 0.0, gg = 0.0, tt = 0.0, top = 0.0; uint32_t best = ' ', count = 0;
			for (uint64_t j = j0; j < j1; j++) {
				const DedupMember M = members[j * P.sides + side];
				if (pos >= M.len) continue;
				dedup_set_top(top, best, a, c, gg, tt);      /* the copy inside operator+ */
				if (pos >= M.stop) continue;      /* an empty ProbabilityBase is added */
				const uint8_t nuc = P.bases[M.off + pos], q = P.quals[M.off + pos];
				const double p = T->prob[q], o = T->other[q];
				double oa = 0.0, oc = 0.0, ogq = 0.0, ot = 0.0;
				switch (nuc) {      /* ProbabilityBase::observe (:870-884): any other character adds nothing but counts */
				case 'A': case 'a': oa = p; oc = o; ogq = o; ot = o; break;
				case 'C': case 'c': oc = p; oa = o; ogq = o; ot = o; break;
				case 'G': case 'g': ogq = p; oa = o; oc = o; ot = o; break;
				case 'T': case 't': ot = p; oa = o; oc = o; ogq = o; break;
				}
				a += oa; c += oc; gg += ogq; tt += ot; count++;
				dedup_set_top(top, best, oa, oc, ogq, ot);
			}
			if (pos < clen) {
				/* getBaseQual (:930-965) and getA .. getT (:905-928); count is a short */
				const double cnt = (double)(int16_t)count;
				uint32_t nuc; double x;
				if (a > c) { if (a > gg) { if (a > tt) { nuc = 'A'; x = a; } else { nuc = 'T'; x = tt; } } else { if (gg > tt) { nuc = 'G'; x = gg; } else { nuc = 'T'; x = tt; } } }
				else { if (c > gg) { if (c > tt) { nuc = 'C'; x = c; } else { nuc = 'T'; x = tt; } } else { if (gg > tt) { nuc = 'G'; x = gg; } else { nuc = 'T'; x = tt; } } }
				const double v = (best == nuc && top < x * cnt) ? top : x;
				out_bases[o0 + pos] = (uint8_t)nuc;
				out_quals[o0 + pos] = (uint8_t)(P.start_char + dedup_qual(T->step, v));
			}
		}
		/* the name: "C", the member count, "-", the first member's name to its first blank or tab, and a newline */
		const uint64_t n0 = name_scan[t]; const uint32_t nb = (uint32_t)(name_scan[t + 1] - n0);
		const uint64_t m = j1 - j0; const uint32_t d = dedup_digits(m);
		const uint64_t first = dedup_member_read(P, G, G.perm[j0], side);
		const uint64_t no = P.name_off[first];
		for (uint32_t p = lane; p < nb; p += 64) {
			uint8_t ch;
			if (p == 0) ch = 'C';
			else if (p <= d) { uint64_t v = m; for (uint32_t k = d - p; k > 0; k--) v /= 10; ch = (uint8_t)('0' + v % 10); }
			else if (p == d + 1) ch = '-';
			else if (p + 1 < nb) ch = P.text[no + p - d - 2];
			else ch = '\n';
			names[n0 + p] = ch;
		}
		if (lane == 0) { out_name_off[t] = n0; out_name_len[t] = nb - 1; }
	}
}

/* head_scan[j + 1] - 1 = the group of sorted candidate j; the reads of a kept group's members become discarded.  A read belongs to
 * one pair record, so no two lanes store to one byte. */
__global__ __launch_bounds__(256)
void dedup_discard_kernel(DedupParams P, const uint32_t *perm, const uint64_t *head_scan, const uint32_t *keep, uint64_t c, uint8_t *disc) {
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < c; j += (uint64_t)gridDim.x * blockDim.x) {
		if (!keep[head_scan[j + 1] - 1]) continue;
		const uint32_t pos = perm[j];
		const int64_t r1 = P.read1[pos], r2 = P.read2[pos];
		if (r1 >= 0) disc[r1] = 1;
		if (r2 >= 0) disc[r2] = 1;
	}
}

}  // namespace kmr
#endif
