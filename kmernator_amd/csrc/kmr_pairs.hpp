/*
 * kmr_pairs.hpp -- ReadSet::identifyPairs (src/ReadSet.cpp:446-570) of one device-resident batch on the device: which reads
 * are the two ends of one fragment, found from their names.  One call equals one identifyPairs() on a fresh ReadSet that holds
 * the batch's reads in batch order (no earlier pairs, previousReadName empty).
 *
 * A read's name and comment are what trimName (src/Utils.h:561-598) makes of its name line (the span name_off / name_len of the
 * batch into the FASTQ text, without the marker): the name runs to the first blank, tab, CR or LF; the comment is the rest if
 * at least one character follows the separator.  With store_comment == 0 a Casava-1.8 comment (isCommentCasava18, :678-685) on
 * a name that does not already end in "/x" rewrites the name to name/1 or name/2 and the comment is dropped; with
 * store_comment != 0 the comment is kept and the name is left alone.  readNum (:689-713) is 1 or 2 from a Casava comment, else
 * from a trailing /1 /A /F or /2 /B /R, else 0; commonName (:669-676) drops the last character of a name longer than 2 whose
 * second-to-last character is '/'.  The common name is never materialised: it is a span of the text plus at most one virtual '/'
 * (the rewritten name without its digit).
 *
 *   pairs_parse_kernel     per read: name end, Casava test, rewrite, readNum, extent of the common name and a 64-bit hash
 *                          (FNV-1a with a finaliser) of its bytes, in one pass over the name line
 * Phase 1, sequential pairs (:467-478 over _isSequentialPair, :94-118).  The reference keeps one pending read; read i pairs with
 * i - 1 exactly when the link i-1 ~ i holds (isPair, src/Utils.h:719-733: same common name, different non-zero read numbers) and
 * i lies at an odd distance from the start of its maximal run of consecutive links:
 *   pairs_link_kernel      link[i] and its negation (the breaks)
 *   (scan of the breaks: the run a read belongs to)
 *   pairs_runstart_kernel  run -> index of its break
 *   pairs_seq_kernel       second-of-a-pair flag, unpaired flag, mate of the phase-1 pairs
 *   (scans of both flags)
 * Phase 2, by name (:500-565), over the reads phase 1 left unpaired:
 *   pairs_keys_kernel      unpaired read -> (hash truncated to pair_hash_bits, index)
 *   (stable radix sort by hash, kmr_sort.hip: index order inside a key comes with it)
 *   pairs_group_kernel     one lane per run of equal hashes walks the reference's map for every distinct common name of the run,
 *                          names compared byte for byte, so a hash collision changes nothing: a read whose common name has no
 *                          entry pushes a half pair (as read2 if readNum == 2, else read1) and becomes the entry if readNum > 0;
 *                          one that meets an entry fills the free side (readNum == 2 -> read2, anything else -> read1) and erases
 *                          it, or, if that side is taken, erases it and pushes a half pair of its own (the two warning branches)
 *   (scan of the push flags)
 *   pairs_scatter_kernel   the pair list: phase-1 pairs ascending, then the records in the order of the reads that pushed them
 *
 * A run of equal hashes is walked by one lane, so a batch in which very many reads share one common name is slow (not wrong).
 * The number of launches does not depend on the number of reads.
 *
 * Not covered: a second identifyPairs() on a set that already has pairs (the reference stores a read index where it reads back
 * a pair index, :492-495 against :520); the per-file identifyPairs and re-ordering of appendAllFiles (:216-239) -- one call over
 * the concatenated batch gives the same pairs for an R1 file followed by an R2 file; printing name/1 for rewritten names in
 * writePicks.
 */
#ifndef KMR_PAIRS_HPP_
#define KMR_PAIRS_HPP_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kmr {

enum { PAIRS_ERR_NAME = 1 };
/* per-read flags of pairs_parse_kernel */
enum { PAIRS_RN = 3 /* readNum */, PAIRS_VIRT = 4 /* the common name ends in a '/' that is not in the text */, PAIRS_NAMED = 8 /* the name is not empty */ };
/* totals block (uint64 each) */
enum { PAIRS_T_SEQ = 0, PAIRS_T_UNPAIRED, PAIRS_T_ERR, PAIRS_T_PUSHED, PAIRS_T_FULL2, PAIRS_T_CONFLICT1, PAIRS_T_CONFLICT2, PAIRS_T_COLLISIONS, PAIRS_T_WORDS };

struct PairsParams {
	const uint64_t *name_off; const uint32_t *name_len;      /* the batch's name spans ... */
	const uint8_t *text; uint64_t text_len;                  /* ... into this text */
	uint64_t n;
	uint32_t store_comment;
};
/* what pairs_parse_kernel leaves per read */
struct PairsNames { const uint64_t *hash; const uint32_t *cn_len; const uint8_t *flags; };

static const uint64_t PAIRS_FNV_OFFSET = 0xcbf29ce484222325ull, PAIRS_FNV_PRIME = 0x100000001b3ull;
__device__ __forceinline__ uint64_t pairs_fnv(uint64_t h, uint8_t c) { return (h ^ c) * PAIRS_FNV_PRIME; }
__device__ __forceinline__ uint64_t pairs_mix(uint64_t h) {      /* so that the low pair_hash_bits of the key are as good as any */
	h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
	return h;
}

/* Bytes of the text at ascending positions: one aligned dword load per four of them where the text allows it (names lie at any
 * alignment; a lane reads its own name, so neighbouring lanes are a record apart and nothing coalesces) */
struct PairsBytes {
	const uint8_t *text; uint64_t len; bool aligned; uint64_t word; uint32_t w;
	__device__ __forceinline__ PairsBytes(const uint8_t *t, uint64_t l) : text(t), len(l), aligned(((uintptr_t)t & 3) == 0), word(~0ull), w(0) {}
	__device__ __forceinline__ uint8_t at(uint64_t pos) {      /* pos < len */
		const uint64_t wi = pos >> 2;
		if (!aligned || 4 * wi + 4 > len) return text[pos];
		if (wi != word) { word = wi; w = ((const uint32_t *)text)[wi]; }
		return (uint8_t)(w >> (8 * (pos & 3)));
	}
};

__device__ __forceinline__ bool pairs_is_sep(uint8_t c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }
__device__ __forceinline__ uint32_t pairs_suffix_num(uint8_t c) {      /* readNum's switch (src/Utils.h:699-711) */
	return (c == '1' || c == 'A' || c == 'F') ? 1u : ((c == '2' || c == 'B' || c == 'R') ? 2u : 0u);
}

__global__ __launch_bounds__(256)
void pairs_parse_kernel(PairsParams P, uint64_t *hash, uint32_t *cn_len, uint8_t *flags, uint64_t *totals) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < P.n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t off = P.name_off[i]; const uint32_t nl = P.name_len[i];
		if (off > P.text_len || nl > P.text_len - off) {
			atomicOr((unsigned long long *)(totals + PAIRS_T_ERR), (unsigned long long)PAIRS_ERR_NAME);
			hash[i] = 0; cn_len[i] = 0; flags[i] = 0;
			continue;
		}
		PairsBytes B(P.text, P.text_len);
		/* the name: h = hash of name[0, L), hprev = hash of name[0, L - 1), last / prev2 = its last two characters */
		uint64_t h = PAIRS_FNV_OFFSET, hprev = PAIRS_FNV_OFFSET;
		uint32_t L = nl; uint8_t last = 0, prev2 = 0;
		for (uint32_t k = 0; k < nl; k++) {
			const uint8_t c = B.at(off + k);
			if (pairs_is_sep(c)) { L = k; break; }
			hprev = h; h = pairs_fnv(h, c); prev2 = last; last = c;
		}
		/* the comment, if at least one character follows the separator; isCommentCasava18 looks at its first six */
		bool casava = false; uint8_t c0 = 0;
		if (L < nl && nl - L - 1 >= 6) {
			uint8_t c[6];
#pragma unroll
			for (int t = 0; t < 6; t++) c[t] = B.at(off + L + 1 + t);
			casava = c[1] == ':' && c[3] == ':' && c[5] == ':' && (c[0] == '1' || c[0] == '2') && (c[2] == 'Y' || c[2] == 'N');
			c0 = c[0];
		}
		const bool slash = L >= 2 && prev2 == '/';
		uint32_t rn, cl, fl;
		uint64_t hv;
		if (casava && !P.store_comment && (L <= 2 || prev2 != '/')) {      /* trimName's rewrite to name/1 or name/2: the common name is name + '/' */
			rn = c0 == '2' ? 2u : 1u; cl = L; hv = pairs_fnv(h, (uint8_t)'/'); fl = PAIRS_VIRT | PAIRS_NAMED;
		} else {
			rn = (casava && P.store_comment) ? (c0 == '2' ? 2u : 1u) : (slash ? pairs_suffix_num(last) : 0u);
			if (L > 2 && slash) { cl = L - 1; hv = hprev; } else { cl = L; hv = h; }
			fl = L ? (uint32_t)PAIRS_NAMED : 0u;
		}
		hash[i] = pairs_mix(hv); cn_len[i] = cl; flags[i] = (uint8_t)(rn | fl);
	}
}

/* are the common names of reads a and b the same bytes?  (their hashes have been compared by the caller or are equal by construction) */
__device__ __forceinline__ bool pairs_same_name(const PairsParams &P, const PairsNames &N, uint64_t a, uint64_t b) {
	const uint32_t la = N.cn_len[a], lb = N.cn_len[b];
	const uint32_t va = (N.flags[a] & PAIRS_VIRT) ? 1u : 0u, vb = (N.flags[b] & PAIRS_VIRT) ? 1u : 0u;
	if (la + va != lb + vb) return false;
	const uint8_t *ta = P.text + P.name_off[a], *tb = P.text + P.name_off[b];
	const uint32_t both = la < lb ? la : lb;
	for (uint32_t k = 0; k < both; k++) if (ta[k] != tb[k]) return false;
	if (la > lb) return ta[lb] == '/';      /* b's virtual '/' against a's real one */
	if (lb > la) return tb[la] == '/';
	return true;
}

/* link[i]: would read i pair with a pending read i - 1?  brk = !link (read 0 never links) */
__global__ __launch_bounds__(256)
void pairs_link_kernel(PairsParams P, PairsNames N, uint8_t *link, uint32_t *brk) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < P.n; i += (uint64_t)gridDim.x * blockDim.x) {
		bool l = false;
		if (i > 0) {
			const uint32_t fa = N.flags[i - 1], fb = N.flags[i];
			l = (fa & PAIRS_RN) && (fb & PAIRS_RN) && (fa & PAIRS_RN) != (fb & PAIRS_RN) && (fa & PAIRS_NAMED)      /* an empty previousReadName means "none pending" (:103) */
			    && N.hash[i - 1] == N.hash[i] && pairs_same_name(P, N, i - 1, i);
		}
		link[i] = l ? 1 : 0; brk[i] = l ? 0u : 1u;
	}
}

/* brk_scan: exclusive scan of brk, so brk_scan[i + 1] = the run of read i (1-based); run_start[run] = index of the break that opens it */
__global__ __launch_bounds__(256)
void pairs_runstart_kernel(const uint8_t *link, const uint64_t *brk_scan, uint64_t n, uint32_t *run_start) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
		if (!link[i]) run_start[brk_scan[i + 1]] = (uint32_t)i;
}

__device__ __forceinline__ bool pairs_is_second(const uint8_t *link, const uint64_t *brk_scan, const uint32_t *run_start, uint64_t i) {
	return link[i] && ((i - run_start[brk_scan[i + 1]]) & 1);
}
/* sec[i] = read i closes the phase-1 pair (i - 1, i); unp[i] = phase 1 left read i unpaired; mate of the phase-1 pairs, -1 elsewhere */
__global__ __launch_bounds__(256)
void pairs_seq_kernel(const uint8_t *link, const uint64_t *brk_scan, const uint32_t *run_start, uint64_t n, uint32_t *sec, uint32_t *unp, int64_t *mate) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const bool s = pairs_is_second(link, brk_scan, run_start, i);
		const bool f = !s && i + 1 < n && pairs_is_second(link, brk_scan, run_start, i + 1);
		sec[i] = s ? 1u : 0u; unp[i] = (s || f) ? 0u : 1u;
		mate[i] = s ? (int64_t)i - 1 : (f ? (int64_t)i + 1 : -1);
	}
}

/* the reads phase 1 left unpaired, in index order: (hash & mask, index) */
__global__ __launch_bounds__(256)
void pairs_keys_kernel(const uint32_t *unp, const uint64_t *unp_scan, const uint64_t *hash, uint64_t mask, uint64_t n, unsigned long long *keys, uint32_t *vals) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
		if (unp[i]) { const uint64_t p = unp_scan[i]; keys[p] = hash[i] & mask; vals[p] = (uint32_t)i; }
}

__device__ __forceinline__ uint32_t pairs_wave_sum(uint32_t v) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}

/* keys / vals: the m unpaired reads sorted by (hash, index).  The lane at the head of a run of equal hashes walks the run once per
 * distinct common name in it (almost always one), taking that name's reads in index order through the reference's map logic.
 * side[r] (0 on entry) = 1 + (readNum == 2) once read r has been taken; push[r] = 1 if it made a pair record. */
__global__ __launch_bounds__(256)
void pairs_group_kernel(PairsParams P, PairsNames N, const unsigned long long *keys, const uint32_t *vals, uint64_t m, int64_t *mate, uint32_t *push, uint8_t *side, uint64_t *totals) {
	uint32_t n_full = 0, n_c1 = 0, n_c2 = 0, n_coll = 0;
	for (uint64_t base = blockIdx.x * (uint64_t)blockDim.x; base < m; base += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t j = base + threadIdx.x;
		if (j >= m || (j > 0 && keys[j] == keys[j - 1])) continue;
		const unsigned long long key = keys[j];
		uint64_t end = j + 1;
		while (end < m && keys[end] == key) end++;
		uint64_t remaining = end - j;
		bool collided = false;
		for (uint64_t a = j; a < end && remaining; a++) {
			const uint32_t ra = vals[a];
			if (side[ra]) continue;
			if (a != j && !collided) { collided = true; n_coll++; }      /* reads are left after the first name's pass: this run holds another name */
			int64_t entry = -1; uint32_t entry_side = 0;      /* the map's entry for this common name: the read that pushed it, the side it took */
			for (uint64_t b = a; b < end; b++) {
				const uint32_t rb = vals[b];
				if (b != a && (side[rb] || !pairs_same_name(P, N, ra, rb))) continue;
				const uint32_t rn = N.flags[rb] & PAIRS_RN, want = rn == 2 ? 2u : 1u;
				side[rb] = (uint8_t)want; remaining--;
				if (entry < 0) {                                    /* no entry: a new half pair, :551-560 */
					push[rb] = 1;
					if (rn > 0) { entry = rb; entry_side = want; }
				} else if (want != entry_side) {                    /* fills the free side, :532 / :544-549 */
					mate[rb] = entry; mate[entry] = rb; n_full++;
					entry = -1;
				} else {                                            /* conflicting read2 / read1, :522-543 */
					if (want == 2) n_c2++; else n_c1++;
					push[rb] = 1;
					entry = -1;
				}
			}
		}
	}
	n_full = pairs_wave_sum(n_full); n_c1 = pairs_wave_sum(n_c1); n_c2 = pairs_wave_sum(n_c2); n_coll = pairs_wave_sum(n_coll);
	if ((threadIdx.x & 63) == 0) {
		if (n_full) atomicAdd((unsigned long long *)(totals + PAIRS_T_FULL2), (unsigned long long)n_full);
		if (n_c1) atomicAdd((unsigned long long *)(totals + PAIRS_T_CONFLICT1), (unsigned long long)n_c1);
		if (n_c2) atomicAdd((unsigned long long *)(totals + PAIRS_T_CONFLICT2), (unsigned long long)n_c2);
		if (n_coll) atomicAdd((unsigned long long *)(totals + PAIRS_T_COLLISIONS), (unsigned long long)n_coll);
	}
}

/* The pair list (-1 = MAX_READ_IDX): record q < n_seq is the phase-1 pair closed by the q-th `sec` read; record n_seq + q belongs to
 * the q-th pushing read, on the side it took, with the read that later filled the other side (its mate) if any. */
__global__ __launch_bounds__(256)
void pairs_scatter_kernel(const uint32_t *sec, const uint64_t *sec_scan, const uint32_t *push, const uint64_t *push_scan, const uint8_t *side, const int64_t *mate,
                          uint64_t n, uint64_t n_seq, int64_t *read1, int64_t *read2) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		if (sec[i]) { const uint64_t q = sec_scan[i]; read1[q] = (int64_t)i - 1; read2[q] = (int64_t)i; }
		else if (push && push[i]) {
			const uint64_t q = n_seq + push_scan[i];
			const bool second = side[i] == 2;
			read1[q] = second ? mate[i] : (int64_t)i; read2[q] = second ? (int64_t)i : mate[i];
		}
	}
}

/* a batch without names (text_len == 0): every read is a half pair of its own */
__global__ __launch_bounds__(256)
void pairs_single_kernel(uint64_t n, int64_t *mate, int64_t *read1, int64_t *read2) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) { mate[i] = -1; read1[i] = (int64_t)i; read2[i] = -1; }
}

}  // namespace kmr
#endif
