/*
 * kmr_select.hpp -- read selection and FASTQ / FASTA output of FilterReads on the device.
 *
 * Replaces selectReads (apps/FilterReads.h:159-279) with max-kmer-output-depth off, plain or partitioned (--partition-by-depth,
 * --remainder-trim, one output per input file): ReadSelector::pickAllPassingReads / pickAllPassingPairs (src/ReadSelector.h:547-596),
 * optimizePickOrder (:1212-1221) and writePicks (:1242-1262) = Read::toFastq / toFasta (src/Sequence.cpp:761-779) of every picked
 * read in ascending read index, over the per-read results of the artifact filter and of scoreAndTrimReads.
 *
 * The first half of this file is what a record is: isPassingRead (passesLength :209-228 in float as the reference computes it), the
 * label, the printed length of a name and the exact byte count of a record (decimal digits are counted, not printed), and
 *   select_write_kernel    one wavefront per record: name, label with integer-to-decimal, base slice, shifted quality slice,
 *                          consecutive lanes taking consecutive bytes of the record
 * (sel_put_record, sel_name_printed and sel_record_bytes are what a record is to any writer; kmr_artifact_report.hpp prints its own through them)
 * A second writer, which assembled 16 KiB tiles of the output in LDS and stored them as 16-byte vectors, was measured against this
 * one and lost ("Read selection and output text"); it is not kept.
 * The second half is which reads are picked and where their records go: one stable partition by (round, input file), of which the
 * plain selection is the case of one round and one input.
 *
 * The number of launches does not depend on the number of reads.
 */
#ifndef KMR_SELECT_HPP_
#define KMR_SELECT_HPP_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmr_select_rounds.hpp"

namespace kmr {

enum { SEL_ERR_MATE = 1, SEL_ERR_NAME = 2, SEL_ERR_PAIR = 4, SEL_ERR_TWICE = 8,      /* the last two: the pair list of kmr_normalize.hpp */
       SEL_ERR_UNNAMED = 16, SEL_ERR_VALUE = 32 };                                    /* kmr_artifact_report.hpp: a read no pair names, a value above n_sequences */
static const uint8_t SEL_REF_QUAL = 127, SEL_PRINT_REF_QUAL = 103;      /* Read::REF_QUAL, Read::PRINT_REF_QUAL (src/config.h:140-141) */
static const int SEL_THREADS = 256, SEL_WAVES = SEL_THREADS / 64, SEL_LABEL_CAP = 128;
/* the longest label sel_label writes, part by part, each with its leading blank:
 *   " AFTrim:" u32 "+" i64 of a difference of two u32       8 + 10 + 1 + 11
 *   " InvBimodal@" u32 ":" u16 "/" u16                     12 + 10 + 1 + 5 + 1 + 5
 *   " Trim:" u32 "+" u32                                     6 + 10 + 1 + 10
 *   " MedianScore:" i32 (the longest of the five names)     13 + 11 */
static const int SEL_LABEL_MOST = (8 + 10 + 1 + 11) + (12 + 10 + 1 + 5 + 1 + 5) + (6 + 10 + 1 + 10) + (13 + 11);
static_assert(SEL_LABEL_MOST <= SEL_LABEL_CAP, "a label must fit the wavefront's LDS buffer");

struct SelectParams {
	const uint8_t *bases, *quals;            /* the batch */
	const uint64_t *offsets, *name_off;
	const uint32_t *name_len;
	const uint8_t *text; uint64_t text_len;  /* what name_off / name_len point into */
	const int64_t *mate;                     /* may be null */
	const uint8_t *af_action;                /* the three may be null together */
	const uint32_t *af_min, *af_max;
	const uint32_t *trim_off, *trim_len;
	const float *score;
	const uint8_t *was_trimmed;
	const uint64_t *bimodal;                 /* bimodal_trim_kernel's word per read; null: --bimodal-sigmas off */
	uint64_t n;
	float min_score, min_read_length;
	uint32_t both_pass, fasta, scoring;
	uint32_t out_base;                       /* 33 or 64 */
	int32_t qual_shift;                      /* out_base - the batch's quality base */
};

/* ReadSelectorUtil::passesLength (src/ReadSelector.h:219-228), all in float */
__device__ __forceinline__ bool sel_passes_length(float length, uint32_t read_length, float minimum) {
	if (length <= 1.0f) return false;
	if (minimum <= 1.0f) return (float)read_length * minimum <= length;
	return minimum <= length;
}
__device__ __forceinline__ bool sel_discarded(const SelectParams &P, uint64_t i) { return P.af_action && P.af_action[i] == 2; }
/* isPassingRead(readIdx, minimumScore, minimumLength) (:550-557), the thresholds being those of one round of selectReads
 * (a row of the round table; P.min_score / P.min_read_length where there is one round, kmr_normalize.hpp) */
__device__ __forceinline__ bool sel_passing(const SelectParams &P, uint64_t i, float min_score, float min_read_length) {
	if (sel_discarded(P, i)) return false;
	const uint32_t len = (uint32_t)(P.offsets[i + 1] - P.offsets[i]);
	return P.score[i] >= min_score && sel_passes_length((float)P.trim_len[i], len, min_read_length);
}
__device__ __forceinline__ bool sel_passing(const SelectParams &P, uint64_t i) { return sel_passing(P, i, P.min_score, P.min_read_length); }

__device__ __forceinline__ uint32_t sel_put_char(uint8_t *dst, uint32_t at, char c, bool write) { if (write) dst[at] = (uint8_t)c; return at + 1; }
__device__ __forceinline__ uint32_t sel_put_str(uint8_t *dst, uint32_t at, const char *s, bool write) {
	for (; *s; s++) at = sel_put_char(dst, at, *s, write);
	return at;
}
__device__ __forceinline__ uint32_t sel_put_int(uint8_t *dst, uint32_t at, int64_t sv, bool write) {
	if (sv < 0) { at = sel_put_char(dst, at, '-', write); sv = -sv; }
	uint64_t v = (uint64_t)sv;
	uint32_t d = 1;
	for (uint64_t t = v; t >= 10; t /= 10) d++;
	if (write) for (uint32_t j = d; j-- > 0;) { dst[at + j] = (uint8_t)('0' + v % 10); v /= 10; }
	return at + d;
}
/* getKmerScoringTypeLabel (src/ReadSelector.h:248-257) */
__device__ __forceinline__ const char *sel_score_label(uint32_t scoring) {
	switch (scoring) { case 0: return "Score:"; case 1: return "MedianScore:"; case 2: return "MinScore:"; case 3: return "MaxScore:"; default: return "AvgScore:"; }
}
/* The label of read i with its leading blank (Read::LABEL_SEP), as FilterKnownOddities (AFTrim) and setTrimHeaders
 * (src/ReadSelector.h:1015-1036) compose it; a discarded read has none.  Returns the length; writes only when asked to
 * (at most SEL_LABEL_MOST bytes).  The tag of the bimodal cut (src/ReadSelector.h:987-1005) stands between AFTrim and Trim: the
 * trim label holds it before setTrimHeaders appends. */
__device__ __forceinline__ uint32_t sel_label(const SelectParams &P, uint64_t i, uint8_t *dst, bool write) {
	if (sel_discarded(P, i)) return 0;
	uint32_t at = 0;
	if (P.af_action && P.af_action[i] == 1) {
		at = sel_put_str(dst, at, " AFTrim:", write);
		at = sel_put_int(dst, at, P.af_min[i], write); at = sel_put_char(dst, at, '+', write); at = sel_put_int(dst, at, (int64_t)P.af_max[i] - (int64_t)P.af_min[i], write);
	}
	const uint64_t bm = P.bimodal ? P.bimodal[i] : 0;
	if (bm) {
		const uint32_t m1 = (uint32_t)(bm >> 32) & 0xffffu, m2 = (uint32_t)(bm >> 48);
		at = sel_put_str(dst, at, m1 < m2 ? " InvBimodal@" : " Bimodal@", write);
		at = sel_put_int(dst, at, (int64_t)(bm & 0xffffffffu), write); at = sel_put_char(dst, at, ':', write);
		at = sel_put_int(dst, at, m1, write); at = sel_put_char(dst, at, '/', write); at = sel_put_int(dst, at, m2, write);
	}
	if (P.was_trimmed[i]) {
		at = sel_put_str(dst, at, " Trim:", write);
		at = sel_put_int(dst, at, P.trim_off[i], write); at = sel_put_char(dst, at, '+', write); at = sel_put_int(dst, at, P.trim_len[i], write);
	}
	at = sel_put_char(dst, at, ' ', write);
	at = sel_put_str(dst, at, sel_score_label(P.scoring), write);
	double s = (double)P.score[i] + 0.5;      /* (int)(score + 0.5), src/ReadSelector.h:1032 */
	/* where that cast is undefined in C++ the rule is this library's own (kmernator_amd.h): a NaN prints 0, a sum outside int the nearest int */
	s = s != s ? 0.0 : (s > 2147483647.0 ? 2147483647.0 : (s < -2147483648.0 ? -2147483648.0 : s));
	at = sel_put_int(dst, at, (int64_t)(int32_t)s, write);
	return at;
}

/* What is printed of read i's bases: masked = the single base N with quality out_base + 1 (a discarded read, or a trim of
 * at most one base: Sequence::getFasta src/Sequence.cpp:305-311, Read::getQuals :729-733); otherwise `len` bases from `from`. */
struct SelSlice { uint64_t from; uint32_t len; bool masked; };
__device__ __forceinline__ SelSlice sel_slice(const SelectParams &P, uint64_t i) {
	SelSlice s;
	const uint64_t b0 = P.offsets[i], L = P.offsets[i + 1] - b0;
	const uint64_t to = P.trim_off[i]; uint64_t tl = P.trim_len[i];
	if (to >= L) tl = 0; else if (tl > L - to) tl = L - to;      /* getQuals clamps the same way (:738-739) */
	s.masked = sel_discarded(P, i) || tl <= 1;
	s.from = b0 + to; s.len = s.masked ? 1u : (uint32_t)tl;
	return s;
}
/* A record as its writer sees it (sel_put_record): the lead character, `nlen` bytes of the name, a label WITH its leading blank,
 * `base_len` bases (no_bases: the single base N), and for FASTQ `qual_len` qualities shifted by qual_shift (no_quals: `qual_len`
 * times the quality `masked_qual`).  The selection prints as many qualities as bases; the artifact report (kmr_artifact_report.hpp) prints N over
 * all of a read's qualities. */
struct SelRecord {
	const uint8_t *name, *label, *bases, *quals;
	uint32_t nlen, lablen, base_len, qual_len;
	int32_t qual_shift;
	uint8_t masked_qual; bool fasta, no_bases, no_quals;
};
__device__ __forceinline__ uint32_t sel_record_bytes(bool fasta, uint32_t nlen, uint32_t lablen, uint32_t base_len, uint32_t qual_len) {
	return 1 + nlen + lablen + 1 + base_len + 1 + (fasta ? 0u : 2u + qual_len + 1u);
}
/* the printed length of a name: up to its first blank or tab; a span outside the text is an error and prints nothing */
__device__ __forceinline__ uint32_t sel_name_printed(const uint8_t *text, uint64_t text_len, uint64_t no, uint32_t nl, uint32_t *err) {
	uint32_t nlen = 0;
	if (no > text_len || nl > text_len - no) atomicOr(err, (uint32_t)SEL_ERR_NAME);
	else while (nlen < nl && text[no + nlen] != ' ' && text[no + nlen] != '\t') nlen++;
	return nlen;
}

/* the printed length of picked read i's name and the exact byte count of its record */
__device__ __forceinline__ uint32_t sel_measure(const SelectParams &P, uint64_t i, uint32_t *name_printed, uint32_t *err) {
	const uint32_t nlen = sel_name_printed(P.text, P.text_len, P.name_off[i], P.name_len[i], err), len = sel_slice(P, i).len;
	*name_printed = nlen;
	return sel_record_bytes(P.fasta != 0, nlen, sel_label(P, i, nullptr, false), len, len);
}

/* The `bytes` bytes of record R, by one wavefront, to dst.  Consecutive lanes take consecutive bytes, so the loads from the name, the
 * bases and the qualities and the stores coalesce. */
__device__ __forceinline__ void sel_put_record(const SelRecord &R, uint32_t bytes, uint8_t *dst, int lane) {
	const uint32_t hdr = 1 + R.nlen + R.lablen + 1;
	for (uint32_t p = lane; p < bytes; p += 64) {
		uint8_t c;
		if (p < hdr) {
			if (p == 0) c = R.fasta ? '>' : '@';
			else if (p <= R.nlen) c = R.name[p - 1];
			else if (p < hdr - 1) c = R.label[p - 1 - R.nlen];
			else c = '\n';
		} else {
			uint32_t q = p - hdr;
			if (q < R.base_len) c = R.no_bases ? (uint8_t)'N' : R.bases[q];
			else if (q == R.base_len) c = '\n';
			else {
				q -= R.base_len + 1;      /* FASTQ only: "+\n", the qualities, "\n" */
				if (q == 0) c = '+';
				else if (q == 1) c = '\n';
				else if (q - 2 < R.qual_len) c = R.no_quals ? R.masked_qual : (uint8_t)(R.quals[q - 2] + R.qual_shift);
				else c = '\n';
			}
		}
		dst[p] = c;
	}
}

/* Read i's record of `bytes` bytes, by one wavefront, to dst; s_label: SEL_LABEL_CAP bytes of LDS of this wavefront. */
__device__ __forceinline__ void sel_emit(const SelectParams &P, uint64_t i, uint32_t nlen, uint32_t bytes, uint8_t *dst, int lane, uint8_t *s_label) {
	const uint32_t lablen = sel_label(P, i, s_label, lane == 0);
	const SelSlice sl = sel_slice(P, i);
	SelRecord R;
	R.name = P.text + P.name_off[i]; R.nlen = nlen; R.label = s_label; R.lablen = lablen;
	R.bases = P.bases + sl.from; R.quals = P.quals + sl.from; R.base_len = R.qual_len = sl.len; R.no_bases = R.no_quals = sl.masked;
	R.qual_shift = P.qual_shift; R.masked_qual = (uint8_t)(P.out_base + 1); R.fasta = P.fasta != 0;
	/* A read whose first quality is Read::REF_QUAL has none (Read::setRead src/Sequence.cpp:652-655), and getQuals prints PRINT_REF_QUAL
	 * for every base of such a read and of a slice that starts on a REF_QUAL (:744-746), whatever the output base */
	if (!R.fasta && !sl.masked && (P.quals[P.offsets[i]] == SEL_REF_QUAL || P.quals[sl.from] == SEL_REF_QUAL)) { R.no_quals = true; R.masked_qual = SEL_PRINT_REF_QUAL; }
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
	sel_put_record(R, bytes, dst, lane);
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();      /* s_label is rewritten for the next record */
}

__global__ __launch_bounds__(SEL_THREADS)
void select_write_kernel(SelectParams P, const uint32_t *name_printed, const uint32_t *pick_read, const uint64_t *pick_off, uint64_t n_picked, uint8_t *out) {
	__shared__ uint8_t s_label[SEL_WAVES][SEL_LABEL_CAP];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	for (uint64_t p = (uint64_t)blockIdx.x * SEL_WAVES + wave; p < n_picked; p += (uint64_t)gridDim.x * SEL_WAVES) {
		const uint64_t rs = pick_off[p];
		const uint32_t r = pick_read[p];
		sel_emit(P, r, name_printed[r], (uint32_t)(pick_off[p + 1] - rs), out + rs, lane, s_label[wave]);
	}
}

/* ---- the rounds of selectReads (apps/FilterReads.h:209-278): --partition-by-depth, --remainder-trim and one output per input
 * file; without them one round and one segment.  A read belongs to the first round of the table (kmr_select_rounds.hpp) whose pair decision picks it -- a pick
 * makes a read unavailable to every later round (pickIfNew, src/ReadSelector.h:513-542), and both reads of a pair are picked
 * together -- and to the input file its index falls into.  Segment = round * n_inputs + input; the output is the segments in that
 * order, ascending read index inside each (optimizePickOrder sorts the picks of one round only), which is a stable multi-way
 * partition of the reads:
 *   partition_classify_kernel  per read its segment (or -1), name length and record bytes; per unit the picks and bytes of every
 *                              segment, summed in LDS
 *   partition_scan_kernel      one block: exclusive scan of the [segment][unit] matrices in that (segment-major) order; the
 *                              segment table, the totals and the sentinel of pick_off
 *   partition_rank_kernel      per unit again: a read's pick index = its unit's base for the segment + the reads of that segment
 *                              before it in the unit, likewise its byte offset; fills the (pick_read, pick_off) select_write_kernel
 *                              reads.  With slot_read it ranks slots that hold reads (kmr_normalize.hpp): pick_read takes the slot's read
 * A unit is one wavefront (a block of 64 threads) over a CONTIGUOUS range of reads, walked 64 reads at a time: consecutive
 * lanes still read consecutive elements, as in a grid stride, but a unit's reads are all before the next unit's, which is what
 * makes the partition stable.  The LDS atomics only add integers (order-free sums); ranks come from ballots and wave scans.
 * Three launches whatever the number of reads, rounds and inputs. */
static const int SEL_MAX_SEGMENTS = 256;      /* rounds x inputs: 3 KiB of LDS per unit (4 + 8 bytes a segment), so that 32 units fit a CU's 160 KiB */
static const int SEL_UNIT = 64, SEL_SCAN_THREADS = 1024, SEL_SCAN_ITEMS = 4;

struct PartitionParams {
	const uint64_t *input_starts;      /* device memory, n_inputs + 1 read indices; not read when n_inputs is 1 */
	uint32_t n_inputs, n_segments;
	uint32_t n_units;
	uint64_t per_unit;                 /* reads of a unit, a multiple of SEL_UNIT */
};

__global__ __launch_bounds__(SEL_UNIT)
void partition_classify_kernel(SelectParams P, SelRounds R, PartitionParams Q, int32_t *read_seg, uint32_t *rec_len, uint32_t *name_printed, uint8_t *picked,
                               uint32_t *unit_cnt, unsigned long long *unit_bytes, uint32_t *err) {
	__shared__ uint32_t s_cnt[SEL_MAX_SEGMENTS];
	__shared__ unsigned long long s_bytes[SEL_MAX_SEGMENTS];
	const uint32_t lane = threadIdx.x, u = blockIdx.x;
	for (uint32_t s = lane; s < Q.n_segments; s += SEL_UNIT) { s_cnt[s] = 0; s_bytes[s] = 0; }
	__syncthreads();
	const uint64_t lo = (uint64_t)u * Q.per_unit, hi = lo + Q.per_unit < P.n ? lo + Q.per_unit : P.n;
	for (uint64_t i = lo + lane; i < hi; i += SEL_UNIT) {
		const int64_t m = P.mate ? P.mate[i] : -1;
		const bool paired = m >= 0 && (uint64_t)m < P.n;
		if (m >= 0 && !paired) atomicOr(err, (uint32_t)SEL_ERR_MATE);
		int32_t seg = -1;
		for (uint32_t r = 0; r < R.n && seg < 0; r++) {
			bool pick = sel_passing(P, i, R.min_score[r], R.min_read_length[r]);
			if (paired) { const bool other = sel_passing(P, (uint64_t)m, R.min_score[r], R.min_read_length[r]); pick = R.both_pass[r] ? (pick && other) : (pick || other); }      /* isPassingPair :558-568 */
			if (pick) seg = (int32_t)r;
		}
		uint32_t bytes = 0, nlen = 0;
		if (seg >= 0) {
			if (Q.n_inputs > 1) {      /* the last input that starts at or before i (input_starts[0] = 0, [n_inputs] = n > i) */
				uint32_t a = 0, b = Q.n_inputs;
				while (b - a > 1) { const uint32_t mid = a + (b - a) / 2; if (Q.input_starts[mid] <= i) a = mid; else b = mid; }
				seg = seg * (int32_t)Q.n_inputs + (int32_t)a;
			}
			bytes = sel_measure(P, i, &nlen, err);
			atomicAdd(&s_cnt[seg], 1u); atomicAdd(&s_bytes[seg], (unsigned long long)bytes);
		}
		read_seg[i] = seg; picked[i] = seg >= 0 ? 1 : 0; rec_len[i] = bytes; name_printed[i] = nlen;
	}
	__syncthreads();
	for (uint32_t s = lane; s < Q.n_segments; s += SEL_UNIT) { unit_cnt[(size_t)s * Q.n_units + u] = s_cnt[s]; unit_bytes[(size_t)s * Q.n_units + u] = s_bytes[s]; }
}

/* In place: unit_cnt / unit_bytes become exclusive prefixes over the matrix in segment-major order.  seg_table: one row of four
 * per segment {first pick, picks, first byte, bytes}; totals[0] = picks, totals[1] = bytes (totals[2] = the error word of the
 * classification); pick_off[picks] = bytes, the end of the last record. */
__global__ __launch_bounds__(SEL_SCAN_THREADS)
void partition_scan_kernel(uint32_t *unit_cnt, unsigned long long *unit_bytes, uint32_t n_segments, uint32_t n_units, uint64_t *seg_table, uint64_t *pick_off, uint64_t *totals) {
	__shared__ unsigned long long s_wc[SEL_SCAN_THREADS / 64], s_wb[SEL_SCAN_THREADS / 64];
	const uint64_t M = (uint64_t)n_segments * n_units;
	const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	unsigned long long carry_c = 0, carry_b = 0;      /* the same in every thread */
	for (uint64_t base = 0; base < M; base += (uint64_t)SEL_SCAN_THREADS * SEL_SCAN_ITEMS) {
		const uint64_t j0 = base + (uint64_t)tid * SEL_SCAN_ITEMS;
		uint32_t c[SEL_SCAN_ITEMS]; unsigned long long b[SEL_SCAN_ITEMS];
		unsigned long long tc = 0, tb = 0;
		for (int k = 0; k < SEL_SCAN_ITEMS; k++) { const bool in = j0 + k < M; c[k] = in ? unit_cnt[j0 + k] : 0u; b[k] = in ? unit_bytes[j0 + k] : 0ull; tc += c[k]; tb += b[k]; }
		unsigned long long ic = tc, ib = tb;
		for (int d = 1; d < 64; d <<= 1) { const unsigned long long x = __shfl_up(ic, d), y = __shfl_up(ib, d); if ((int)lane >= d) { ic += x; ib += y; } }
		if (lane == 63) { s_wc[wave] = ic; s_wb[wave] = ib; }
		__syncthreads();
		unsigned long long ec = carry_c + ic - tc, eb = carry_b + ib - tb;
		for (uint32_t w = 0; w < SEL_SCAN_THREADS / 64; w++) { if (w < wave) { ec += s_wc[w]; eb += s_wb[w]; } carry_c += s_wc[w]; carry_b += s_wb[w]; }
		for (int k = 0; k < SEL_SCAN_ITEMS; k++) if (j0 + k < M) { unit_cnt[j0 + k] = (uint32_t)ec; unit_bytes[j0 + k] = eb; ec += c[k]; eb += b[k]; }
		__syncthreads();      /* s_wc / s_wb are rewritten by the next tile; after the last one the prefixes are read back below */
	}
	for (uint32_t s = tid; s < n_segments; s += SEL_SCAN_THREADS) {
		const uint64_t fp = unit_cnt[(size_t)s * n_units], fb = unit_bytes[(size_t)s * n_units];
		const uint64_t ep = s + 1 < n_segments ? unit_cnt[(size_t)(s + 1) * n_units] : carry_c, eb = s + 1 < n_segments ? unit_bytes[(size_t)(s + 1) * n_units] : carry_b;
		seg_table[4 * s] = fp; seg_table[4 * s + 1] = ep - fp; seg_table[4 * s + 2] = fb; seg_table[4 * s + 3] = eb - fb;
	}
	if (tid == 0) { totals[0] = carry_c; totals[1] = carry_b; pick_off[carry_c] = carry_b; }
}

__global__ __launch_bounds__(SEL_UNIT)
void partition_rank_kernel(const int32_t *read_seg, const uint32_t *rec_len, uint64_t n, PartitionParams Q, const uint32_t *unit_cnt, const unsigned long long *unit_bytes,
                           uint32_t *pick_read, uint64_t *pick_off, const uint32_t *slot_read) {
	__shared__ uint32_t s_cnt[SEL_MAX_SEGMENTS];            /* where the unit's next read of the segment goes */
	__shared__ unsigned long long s_bytes[SEL_MAX_SEGMENTS];
	const uint32_t lane = threadIdx.x, u = blockIdx.x;
	for (uint32_t s = lane; s < Q.n_segments; s += SEL_UNIT) { s_cnt[s] = unit_cnt[(size_t)s * Q.n_units + u]; s_bytes[s] = unit_bytes[(size_t)s * Q.n_units + u]; }
	__syncthreads();
	const uint64_t lo = (uint64_t)u * Q.per_unit, hi = lo + Q.per_unit < n ? lo + Q.per_unit : n;
	for (uint64_t t = lo; t < hi; t += SEL_UNIT) {      /* the whole wavefront takes every turn */
		const uint64_t i = t + lane;
		const int32_t seg = i < hi ? read_seg[i] : -1;
		const unsigned long long len = i < hi ? rec_len[i] : 0u;
		unsigned long long todo = __ballot(seg >= 0);
		while (todo) {      /* one turn per segment present among the 64 reads */
			const int leader = __ffsll(todo) - 1;
			const int32_t s0 = __shfl(seg, leader);
			const bool mine = seg == s0;
			const unsigned long long members = __ballot(mine);
			unsigned long long inc = mine ? len : 0ull;
			for (int d = 1; d < 64; d <<= 1) { const unsigned long long x = __shfl_up(inc, d); if ((int)lane >= d) inc += x; }
			const unsigned long long all = __shfl(inc, 63);
			const uint32_t at = s_cnt[s0]; const unsigned long long byte_at = s_bytes[s0];
			if (mine) { const uint32_t p = at + (uint32_t)__popcll(members & ((1ull << lane) - 1)); pick_read[p] = slot_read ? slot_read[i] : (uint32_t)i; pick_off[p] = byte_at + inc - len; }
			__syncthreads();
			if ((int)lane == leader) { s_cnt[s0] = at + (uint32_t)__popcll(members); s_bytes[s0] = byte_at + all; }
			__syncthreads();
			todo &= ~members;
		}
	}
}

}  // namespace kmr
#endif
