/*
 * kmr_artifact_report.hpp -- what FilterKnownOddities' Recorder makes of the artifact filter's decisions, on the device
 * (src/FilterKnownOddities.h: Recorder :296-353, recordAffectedRead :551-640, applyFilter :663-732): the -Artifact.fastq and
 * -PhiX.fastq records and the per-sequence counters Discarded / Affected / BasesRemoved.
 *
 * A unit is one entry of the pair list (read1, then read2, either may be absent) or, without a list, one read.  Its reads stand in
 * slots as kmr_normalize.hpp lays them out -- slot 2p is read1 of unit p, slot 2p + 1 read2; without a list slot i is read i -- so
 * that slots in ascending order are the records in the order one thread of the reference writes them, read1 before read2 also where
 * read1 has the higher index.  A record goes to the file of the input that the unit's read1 belongs to (read2's if read1 is absent):
 * segment = row * n_inputs + input, row 0 Artifact, row 1 PhiX, and the output is the stable partition of the slots by segment that
 * the units of kmr_select.hpp compute.
 *
 *   normalize_mark_kernel         (kmr_normalize.hpp) the pair list's indices, every read counted that a pair names
 *   artifact_pairs_kernel         per read: named exactly once (identifyPairs never leaves a read out)
 *   artifact_mate_kernel          the fused form only: mate[] of the apply step from the pair list
 *   artifact_classify_kernel      per slot: the unit's rule, the three counters, segment, printed name length, label and record bytes;
 *                                 per unit the records and bytes of every segment, summed in LDS (as partition_classify_kernel)
 *   partition_scan_kernel, partition_rank_kernel   (kmr_select.hpp) as they stand, over slots
 *   artifact_write_kernel         one wavefront per record through sel_put_record: the label read from the filter's name table, the
 *                                 base line N (or the read's bases), the quality line all of the read's qualities
 * The counters are integer sums, so atomics are order-free: a unit privatises them in LDS while 3 x 8 x (n_sequences + 1) bytes fit
 * ART_REPORT_LDS_CAP and flushes what is not zero; above the cap every hit goes to a global 64-bit atomic.
 * The number of launches does not depend on the batch.
 */
#ifndef KMR_ARTIFACT_REPORT_HPP_
#define KMR_ARTIFACT_REPORT_HPP_

#include "kmr_normalize.hpp"

namespace kmr {

/* 6 KiB = 256 sequence indices: with the 3 KiB of the segment sums a unit (one wavefront) asks for 9 KiB, so 17 units still fit a CU's
 * 160 KiB; the reference's built-in artifact set stays below, an --artifact-reference-file of thousands of sequences goes above */
static const uint32_t ART_REPORT_LDS_CAP = 6144;
static const uint32_t ART_REPORT_LDS_MOST = 48 * 1024;      /* what kmr_tune "artifact_report_lds" 1 can force */

struct ArtReportParams {
	const uint8_t *bases, *quals;            /* the batch the filter was applied to */
	const uint64_t *offsets, *name_off;
	const uint32_t *name_len;
	const uint8_t *text; uint64_t text_len;
	uint64_t n;
	const int64_t *read1, *read2;            /* null: every read is a unit */
	uint64_t n_pairs;
	const uint32_t *value, *min_pass, *max_pass;      /* kmr_artifact_filter_apply's decisions */
	const uint8_t *action;
	const uint8_t *label_bytes;              /* the filter's names, each with its leading blank (none for an empty name) */
	const uint64_t *label_off;               /* [n_seq + 2]: index n_seq is MinQualityTrim<q> */
	uint32_t n_seq, phix;
	uint32_t artifact_output, phix_output, print_bases;
	uint32_t out_base; int32_t qual_shift;
};

__global__ __launch_bounds__(256)
void artifact_pairs_kernel(const uint32_t *named, uint64_t n, uint32_t *err) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
		if (named[i] == 0) atomicOr(err, (uint32_t)SEL_ERR_UNNAMED);
}
/* mate is -1 everywhere on entry; a list that is refused (normalize_mark_kernel) leaves something in range */
__global__ __launch_bounds__(256)
void artifact_mate_kernel(const int64_t *read1, const int64_t *read2, uint64_t n_pairs, uint64_t n, int64_t *mate) {
	for (uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * blockDim.x) {
		const int64_t a = read1[p], b = read2[p];
		if (a < 0 || b < 0 || (uint64_t)a >= n || (uint64_t)b >= n) continue;
		mate[a] = b; mate[b] = a;
	}
}

/* What is printed of read r: N (or its bases) over all of its qualities; a read of at most one base as the selection prints a
 * masked one (Sequence::getFastaNoMarkup src/Sequence.cpp:290-296, Read::getQuals :729-759 with unmasked = true) */
__device__ __forceinline__ void art_report_slice(const ArtReportParams &A, uint32_t len, uint32_t *base_len, uint32_t *qual_len) {
	*base_len = (A.print_bases && len > 1) ? len : 1u;
	*qual_len = len > 1 ? len : 1u;
}

/* ctr: [3][n_seq + 1] discarded, trimmed, bases; LDS_CTR: the unit sums them in 24 * (n_seq + 1) bytes of dynamic LDS first.
 * item_seg, read_seg are -1 and picked is 0 on entry. */
template <bool LDS_CTR> __global__ __launch_bounds__(SEL_UNIT)
void artifact_classify_kernel(ArtReportParams A, PartitionParams Q, uint64_t n_items, uint32_t *slot_read, int32_t *item_seg, uint32_t *item_len, uint32_t *name_printed,
                              uint32_t *read_label, uint8_t *picked, int32_t *read_seg, uint32_t *unit_cnt, unsigned long long *unit_bytes, unsigned long long *ctr, uint32_t *err) {
	__shared__ uint32_t s_cnt[SEL_MAX_SEGMENTS];
	__shared__ unsigned long long s_bytes[SEL_MAX_SEGMENTS];
	extern __shared__ __attribute__((aligned(16))) unsigned long long s_ctr[];
	const uint32_t lane = threadIdx.x, u = blockIdx.x, rows = A.n_seq + 1;
	for (uint32_t s = lane; s < Q.n_segments; s += SEL_UNIT) { s_cnt[s] = 0; s_bytes[s] = 0; }
	if (LDS_CTR) for (uint32_t s = lane; s < 3 * rows; s += SEL_UNIT) s_ctr[s] = 0;
	__syncthreads();
	unsigned long long *const c = LDS_CTR ? s_ctr : ctr;
	const uint64_t lo = (uint64_t)u * Q.per_unit, hi = lo + Q.per_unit < n_items ? lo + Q.per_unit : n_items;
	for (uint64_t t = lo + lane; t < hi; t += SEL_UNIT) {
		int64_t a = (int64_t)t, b = -1, r = (int64_t)t;
		if (A.read1) {
			a = A.read1[t >> 1]; b = A.read2[t >> 1]; r = (t & 1) ? b : a;
			if (!norm_index_ok(a, A.n) || !norm_index_ok(b, A.n) || (a < 0 && b < 0)) continue;      /* reported by normalize_mark_kernel */
		}
		if (r < 0) continue;
		const uint32_t va = a >= 0 ? A.value[a] : 0u, vb = b >= 0 ? A.value[b] : 0u, v = A.value[r];
		if (va > A.n_seq || vb > A.n_seq) { atomicOr(err, (uint32_t)SEL_ERR_VALUE); continue; }
		if (va == 0 && vb == 0) continue;
		const uint32_t len = (uint32_t)(A.offsets[r + 1] - A.offsets[r]);
		const bool phix = A.phix != 0 && (va == A.phix || vb == A.phix);
		int32_t row = -1; uint32_t label = 0;
		if (phix) {      /* every present read of the unit, a clean mate included (:569-587) */
			atomicAdd(&c[A.phix], 1ull); atomicAdd(&c[2 * rows + A.phix], (unsigned long long)len);
			if (A.phix_output) row = 1;
		} else if (v != 0) {
			const uint8_t act = A.action[r];
			if (act == 2) {
				atomicAdd(&c[v], 1ull); atomicAdd(&c[2 * rows + v], (unsigned long long)len);
				if (A.artifact_output) { row = 0; label = v; }
			} else if (act == 1) {
				atomicAdd(&c[rows + v], 1ull); atomicAdd(&c[2 * rows + v], (unsigned long long)(len - (A.max_pass[r] - A.min_pass[r])));
			}
		}
		if (row < 0) continue;
		const uint64_t first = (uint64_t)(a >= 0 ? a : b);
		uint32_t input = 0;
		if (Q.n_inputs > 1) {      /* the last input that starts at or before the unit's first read */
			uint32_t x = 0, y = Q.n_inputs;
			while (y - x > 1) { const uint32_t mid = x + (y - x) / 2; if (Q.input_starts[mid] <= first) x = mid; else y = mid; }
			input = x;
		}
		const int32_t seg = row * (int32_t)Q.n_inputs + (int32_t)input;
		const uint32_t nlen = sel_name_printed(A.text, A.text_len, A.name_off[r], A.name_len[r], err);
		uint32_t base_len, qual_len;
		art_report_slice(A, len, &base_len, &qual_len);
		const uint32_t bytes = sel_record_bytes(false, nlen, (uint32_t)(A.label_off[label + 1] - A.label_off[label]), base_len, qual_len);
		atomicAdd(&s_cnt[seg], 1u); atomicAdd(&s_bytes[seg], (unsigned long long)bytes);
		if (slot_read) slot_read[t] = (uint32_t)r;
		item_seg[t] = seg; item_len[t] = bytes;
		name_printed[r] = nlen; read_label[r] = label; picked[r] = 1; read_seg[r] = seg;
	}
	__syncthreads();
	for (uint32_t s = lane; s < Q.n_segments; s += SEL_UNIT) { unit_cnt[(size_t)s * Q.n_units + u] = s_cnt[s]; unit_bytes[(size_t)s * Q.n_units + u] = s_bytes[s]; }
	if (LDS_CTR) for (uint32_t s = lane; s < 3 * rows; s += SEL_UNIT) if (s_ctr[s]) atomicAdd(&ctr[s], s_ctr[s]);
}

__global__ __launch_bounds__(SEL_THREADS)
void artifact_write_kernel(ArtReportParams A, const uint32_t *name_printed, const uint32_t *read_label, const uint32_t *pick_read, const uint64_t *pick_off, uint64_t n_picked, uint8_t *out) {
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	for (uint64_t p = (uint64_t)blockIdx.x * SEL_WAVES + wave; p < n_picked; p += (uint64_t)gridDim.x * SEL_WAVES) {
		const uint64_t rs = pick_off[p];
		const uint32_t r = pick_read[p], label = read_label[r];
		const uint64_t b0 = A.offsets[r];
		const uint32_t len = (uint32_t)(A.offsets[r + 1] - b0);
		SelRecord R;
		R.name = A.text + A.name_off[r]; R.nlen = name_printed[r];
		R.label = A.label_bytes + A.label_off[label]; R.lablen = (uint32_t)(A.label_off[label + 1] - A.label_off[label]);
		art_report_slice(A, len, &R.base_len, &R.qual_len);
		R.bases = A.bases + b0; R.quals = A.quals + b0; R.no_bases = !(A.print_bases && len > 1); R.no_quals = len <= 1;
		R.qual_shift = A.qual_shift; R.masked_qual = (uint8_t)(A.out_base + 1); R.fasta = false;
		sel_put_record(R, (uint32_t)(pick_off[p + 1] - rs), out + rs, lane);
	}
}

}  // namespace kmr
#endif
