/*
 * kmr_stages.hip -- the read stages of include/kmernator_amd.h: FASTQ ingest and the kmr_reads batch, its two-bit form, the artifact
 * filter and its report, read selection, coverage normalization and their output text, identifyPairs, duplicate-fragment collapse, the mercount / mergraph text, TnfDistance's vectors and distances, KmerMatch's entry points with its finish, and ContigExtender's entry points.
 *
 * Host logic only, as kmr_api.hip (the spectrum, which these stages read through kmr_host.hpp); the kernels are the stage headers',
 * each of which this translation unit alone includes.  A stage costs its kernels and a page here: what the stages share is below --
 * the call's temporaries (Scratch, with the scratch of kmr_sort.hip's sorts), inputs from host or device memory (to_device), result
 * objects (make_result, free_on_device, copy_out).
 */
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>

#include "kmr_host.hpp"
#include "kmr_ingest.hpp"
#include "kmr_artifact.hpp"
#include "kmr_select.hpp"
#include "kmr_normalize.hpp"
#include "kmr_artifact_report.hpp"
#include "kmr_pairs.hpp"
#include "kmr_dedup.hpp"
#include "kmr_dump.hpp"
#include "kmr_tnf.hpp"
#define KMR_MATCH_FINISH      /* the finish kernels; the table and the Op are kmr_api.hip's */
#include "kmr_match.hpp"

static const int EXT_VALS = 6;      /* values of a stop record (kmr_extend.hpp, whose kernels are kmr_api.hip's): edge, A, C, G, T, total */

using namespace kmr;

namespace {

/* The temporaries of one call on the handle's stream: take() allocates a block of n elements of T (alloc_n: one allocation, 256 bytes
 * at least) that lives until the call returns.  A return with work still queued -- an error path -- waits for the stream before the
 * blocks go; a call that has waited for its last work itself says done().  sort: the scratch of the call's sorts (sort_reserve,
 * sort_pairs, sort_by_columns of kmr_sort.hip), of which tmp is held whenever any is. */
class Scratch {
public:
	explicit Scratch(kmr_handle *h) : h_(h) {}
	~Scratch() { if (armed_ && (!bufs_.empty() || sort.tmp)) hipStreamSynchronize(h_->stream); }
	template <class T> hipError_t take(T **p, size_t n) { bufs_.emplace_back(); return alloc_n(bufs_.back(), p, n); }
	void done() { armed_ = false; }
	SortBufs sort;
private:
	kmr_handle *h_; std::vector<DevBuf> bufs_; bool armed_ = true;
};

/* an input array as device memory: as it is if it lives there (on_device), else copied into a block of tmp on the stream; an absent
 * or empty host array is null */
template <class T> int to_device(kmr_handle *h, Scratch &tmp, const T *src, uint64_t n, const T **dev, bool on_device = false) {
	*dev = on_device ? src : nullptr;
	if (on_device || !src || !n) return 0;
	T *p = nullptr;
	HIPCHK(h, tmp.take(&p, n));
	HIPCHK(h, hipMemcpyAsync(p, src, sizeof(T) * n, hipMemcpyHostToDevice, h->stream));
	*dev = p;
	return 0;
}

const char *const NAME_SPAN_ERROR = "a read's name span lies outside the text handed in (pass the text the batch was ingested from)";

/* Result objects (kmr_reads, kmr_picks, ...: OnDevice): made on the handle's device and owned until released to the caller; deleted
 * with that device current, where their buffers are freed; copied out array by array */
template <class T> void free_on_device(T *x) { if (!x) return; hipSetDevice(x->device); delete x; }
template <class T> std::unique_ptr<T, void (*)(T *)> make_result(kmr_handle *h) {
	std::unique_ptr<T, void (*)(T *)> x(new T, free_on_device<T>);
	x->device = h->device;
	return x;
}
/* copy_out(e, dst, buf, n): n elements of buf to the host array dst, if there is one and nothing failed before */
template <class T> void copy_out(hipError_t &e, T *dst, const DevBuf &buf, uint64_t n) {
	if (dst && n && e == hipSuccess) e = hipMemcpy(dst, buf.get<T>(), sizeof(T) * n, hipMemcpyDeviceToHost);
}

}  // namespace

/* the two-bit launches of the spectrum's packed feed path (kmr_add_reads_twobit_dev) */
namespace kmr_host {
int twobit_byte_offsets(kmr_handle *h, const uint64_t *offsets, uint64_t n, uint32_t *len, uint64_t *off) {
	LAUNCH(h, twobit_bytes_kernel, dim3(grid_for(n)), dim3(256), 0, offsets, n, len);
	return exclusive_scan(h, len, n, off);
}
int twobit_rel_offsets(kmr_handle *h, const uint64_t *offsets, uint64_t n, uint64_t *rel) {
	LAUNCH(h, offsets_rel_kernel, dim3(grid_for(n + 1)), dim3(256), 0, offsets, n, rel);
	return 0;
}
int twobit_unpack(kmr_handle *h, const uint8_t *twobit, const uint64_t *twobit_off, const uint64_t *offsets, const uint64_t *mk_off, const uint32_t *mk_pos, const uint8_t *mk_char,
                  uint64_t n, uint8_t *bases, uint64_t *rel) {
	LAUNCH(h, twobit_unpack_kernel, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)num_cus(h) * 32)), dim3(256), 0, twobit, twobit_off, offsets, n, bases, rel);
	if (mk_off) {
		LAUNCH(h, twobit_markup_kernel, dim3(grid_for(n)), dim3(256), 0, mk_off, mk_pos, mk_char, (const uint64_t *)rel, n, bases);
	}
	return 0;
}
}  // namespace kmr_host

extern "C" {

/* ---- f2: FASTQ ingest on the device (kmr_ingest.hpp) ------------------------ */
static int ingest_dev(kmr_handle *h, const uint8_t *text, uint64_t len, uint32_t input_base, int store_comment, kmr_reads **out) {
	const uint32_t start = h->cfg.fastq_start_char;
	if (input_base == 0) input_base = start;
	if ((input_base != 33 && input_base != 64) || (start != 33 && start != 64))
		return fail(h, KMR_ERR_INVALID_ARG, "fastq quality base must be 33 or 64 (src/Options.h:490)");
	auto R = make_result<kmr_reads>(h);
	R->input_base = input_base;
	DevBuf blk, derr, llen, keep, klen, bbase, lstart, kidx, boff;      /* scratch of this call */
	const uint64_t nblk = (len + (uint64_t)ING_THREADS * ING_BYTES - 1) / ((uint64_t)ING_THREADS * ING_BYTES);
	uint64_t n_lines = 0;
	HIPCHK(h, derr.alloc(8)); HIPCHK(h, hipMemsetAsync(derr.get<uint32_t>(), 0, 8, h->stream));
	if (nblk) {
		if (nblk > 0x7fffffffull) return fail(h, KMR_ERR_INVALID_ARG, "FASTQ block too large for one call");
		HIPCHK(h, blk.alloc(4 * nblk)); HIPCHK(h, bbase.alloc(8 * (nblk + 1)));
		LAUNCH(h, ingest_count_lines, dim3((unsigned)nblk), dim3(ING_THREADS), 0, text, len, blk.get<uint32_t>());
		{ int rc = exclusive_scan(h, blk.get<uint32_t>(), nblk, bbase.get<uint64_t>()); if (rc) return rc; }
		HIPCHK(h, hipMemcpy(&n_lines, bbase.get<uint64_t>() + nblk, 8, hipMemcpyDeviceToHost));
	}
	if (n_lines % 4 != 0) return fail(h, KMR_ERR_INVALID_ARG, "malformed FASTQ: " + std::to_string(n_lines) + " non-empty lines is not a multiple of 4 (truncated record)");
	const uint64_t nrec = n_lines / 4;
	uint64_t n_kept = 0, total = 0;
	if (nrec) {
		HIPCHK(h, lstart.alloc(8 * n_lines)); HIPCHK(h, llen.alloc(4 * n_lines));
		LAUNCH(h, ingest_index_lines, dim3((unsigned)nblk), dim3(ING_THREADS), 0, text, len, bbase.get<uint64_t>(), lstart.get<uint64_t>());
		LAUNCH(h, ingest_line_lengths, dim3(grid_for(n_lines)), dim3(256), 0, text, len, lstart.get<uint64_t>(), n_lines, llen.get<uint32_t>(), derr.get<uint32_t>(), false);
		HIPCHK(h, keep.alloc(4 * nrec)); HIPCHK(h, klen.alloc(4 * nrec));
		HIPCHK(h, kidx.alloc(8 * (nrec + 1))); HIPCHK(h, boff.alloc(8 * (nrec + 1)));
		LAUNCH(h, ingest_records, dim3(grid_for(nrec)), dim3(256), 0, text, lstart.get<uint64_t>(), llen.get<uint32_t>(), nrec, store_comment, keep.get<uint32_t>(), klen.get<uint32_t>(), derr.get<uint32_t>());
		{ int rc = exclusive_scan(h, keep.get<uint32_t>(), nrec, kidx.get<uint64_t>()); if (rc) return rc; }
		{ int rc = exclusive_scan(h, klen.get<uint32_t>(), nrec, boff.get<uint64_t>()); if (rc) return rc; }
		uint32_t e = 0;
		HIPCHK(h, hipMemcpy(&e, derr.get<uint32_t>(), 4, hipMemcpyDeviceToHost));
		if (e) {
			std::string why;
			if (e & ING_ERR_NAME) why += " a record does not start with '@' or has an empty name;";
			if (e & ING_ERR_BLANK) why += " an empty line inside a record;";
			if (e & ING_ERR_PLUS) why += " missing '+' line;";
			if (e & ING_ERR_LEN) why += " number of bases and quals not equal;";
			return fail(h, KMR_ERR_INVALID_ARG, "malformed FASTQ:" + why);
		}
		HIPCHK(h, hipMemcpy(&n_kept, kidx.get<uint64_t>() + nrec, 8, hipMemcpyDeviceToHost)); HIPCHK(h, hipMemcpy(&total, boff.get<uint64_t>() + nrec, 8, hipMemcpyDeviceToHost));
	}
	R->n = n_kept; R->total = total; R->filtered = nrec - n_kept;
	HIPCHK(h, R->bases.alloc(total + 64)); HIPCHK(h, R->quals.alloc(total + 64)); HIPCHK(h, R->offsets.alloc(8 * (n_kept + 1)));
	HIPCHK(h, R->name_off.alloc(8 * std::max<uint64_t>(1, n_kept))); HIPCHK(h, R->name_len.alloc(4 * std::max<uint64_t>(1, n_kept)));
	HIPCHK(h, hipMemsetAsync(R->bases.get<uint8_t>() + total, 0, 64, h->stream)); HIPCHK(h, hipMemsetAsync(R->quals.get<uint8_t>() + total, 0, 64, h->stream));
	HIPCHK(h, hipMemcpyAsync(R->offsets.get<uint64_t>() + n_kept, &total, 8, hipMemcpyHostToDevice, h->stream));
	if (nrec) {
		/* appendFasta rescales every read from the input base to Read::FASTQ_START_CHAR as it is read (src/ReadSet.cpp:324,336) */
		LAUNCH(h, ingest_copy, dim3(grid_for(nrec, 4, 1 << 16)), dim3(256), 0, text, len, lstart.get<uint64_t>(), llen.get<uint32_t>(), nrec, keep.get<uint32_t>(), kidx.get<uint64_t>(), boff.get<uint64_t>(),
		       (int)start - (int)input_base, start, R->bases.get<uint8_t>(), R->quals.get<uint8_t>(), R->offsets.get<uint64_t>(), R->name_off.get<uint64_t>(), R->name_len.get<uint32_t>(), derr.get<uint32_t>() + 1);
		uint32_t flip = 0;
		HIPCHK(h, fetch(h, &flip, derr.get<uint32_t>() + 1));
		const uint32_t want = start == 33 ? 64u : 33u;        /* __setFastqStart(the other base), src/ReadSet.h:174-186 */
		if (flip && want != input_base) {
			if (total) LAUNCH(h, ingest_shift_quals, dim3(grid_for(total)), dim3(256), 0, R->quals.get<uint8_t>(), total, (int)input_base - (int)want);
			R->input_base = want;
		}
	}
	HIPCHK(h, hipStreamSynchronize(h->stream));
	*out = R.release();
	return KMR_OK;
}

int kmr_ingest_fastq_dev(kmr_handle *h, const void *dev_text, uint64_t len, uint32_t input_quality_base, int store_comment, kmr_reads **out) {
	if (!h || !out || (len && !dev_text)) return KMR_ERR_INVALID_ARG;
	*out = nullptr;
	hipSetDevice(h->device);
	return ingest_dev(h, (const uint8_t *)dev_text, len, input_quality_base, store_comment, out);
}
int kmr_ingest_fastq(kmr_handle *h, const char *text, uint64_t len, uint32_t input_quality_base, int store_comment, kmr_reads **out) {
	if (!h || !out || (len && !text)) return KMR_ERR_INVALID_ARG;
	*out = nullptr;
	hipSetDevice(h->device);
	DevBuf d;
	HIPCHK(h, d.alloc(len + 16));
	hipError_t e = hipMemcpy(d.get(), text, len, hipMemcpyHostToDevice);
	if (e != hipSuccess) { h->err = std::string("hipMemcpy(FASTQ text): ") + hipGetErrorString(e); return KMR_ERR_HIP; }
	return ingest_dev(h, d.get<uint8_t>(), len, input_quality_base, store_comment, out);
}
/* ---- FASTA and FASTA+QUAL ingest on the device (kmr_ingest.hpp) ------------- */
}  // extern "C"

namespace {

/* several arrays out of one grow-only block of the handle (kmr_handle::fasta_buf, as score_buf serves the scoring calls: a device
 * allocation of more than 2 MB costs the host more than all kernels of a 16 MiB call together): take() every array, then reserve() */
struct Piece { uint8_t *p = nullptr; template <class T> T *get() const { return (T *)p; } };
struct Pieces {
	std::vector<std::pair<Piece *, size_t>> taken; size_t total = 0;
	void take(Piece &x, size_t bytes) { taken.emplace_back(&x, total); total += (bytes + 255) & ~(size_t)255; }
	int reserve(kmr_handle *h, DevBuf &buf) {
		const int rc = buf.reserve(h, "FASTA ingest scratch", std::max<size_t>(total, 256));
		if (!rc) for (auto &t : taken) t.first->p = buf.get<uint8_t>() + t.second;
		return rc;
	}
};

/* the lines and records of a FASTA or QUAL text, in three blocks (per 4 KB block, per line, per record): starts and lengths of the
 * non-empty lines, header flags and their exclusive scan (a header's value = its record), the header line of every record.  FASTA
 * only: keep[r] = the Casava filter passes it, kidx its scan; klen = a line's length in the output, loff its scan.  QUAL only: numbers
 * per block and their scan, the running count at a line start, where a line's first number goes and to which read */
struct FastaIndex {
	Pieces per_block, per_line, per_record;
	Piece blk, bbase, lstart, llen, ishdr, hidx, recline, keep, kidx, klen, loff, btok, tbase, tline, lout, lread;
	uint64_t nblk = 0, n_lines = 0, nrec = 0;
};

std::string fasta_why(uint32_t e) {
	std::string why;
	if (e & FA_ERR_LEAD) why += " text or an empty line before the first header;";
	if (e & FA_ERR_HDR_HDR) why += " a header followed by a header;";
	if (e & FA_ERR_HDR_END) why += " a header at the end of the text;";
	if (e & FA_ERR_BLANK) why += " an empty line before or between the lines of a record;";
	if (e & ING_ERR_NAME) why += " an empty name;";
	if (e & FA_ERR_QBYTE) why += " a byte that is no digit, blank or tab in a quality line;";
	if (e & FA_ERR_QDIGITS) why += " a quality of more than 3 digits;";
	if (e & FA_ERR_QGLUE) why += " a quality line ends in a digit and the next one starts with a digit;";
	if (e & FA_ERR_QNAME) why += " fasta and quals have different names;";
	if (e & FA_ERR_QCOUNT) why += " number of bases and quals not equal;";
	return why;
}

/* what the error word at derr holds after the work queued so far: 0, or the call's return code with its message */
int fasta_check(kmr_handle *h, const uint32_t *derr, const char *what) {
	uint32_t e = 0;
	HIPCHK(h, fetch(h, &e, derr));
	if (e & (FA_ERR_LONG | ING_ERR_LEN)) return fail(h, KMR_ERR_UNSUPPORTED, std::string(what) + ": a line or record of more than 2^32 - 2 bytes (SequenceLengthType)");
	if (e) return fail(h, KMR_ERR_INVALID_ARG, std::string("malformed ") + what + ":" + fasta_why(e));
	return 0;
}

int fasta_index(kmr_handle *h, const uint8_t *text, uint64_t len, int store_comment, bool is_fasta, uint32_t *derr, const char *what, FastaIndex &X) {
	DevBuf *const bufs = h->fasta_buf[is_fasta ? 0 : 1];
	X.nblk = (len + (uint64_t)ING_THREADS * ING_BYTES - 1) / ((uint64_t)ING_THREADS * ING_BYTES);
	if (!X.nblk) return 0;
	if (X.nblk > 0x7fffffffull) return fail(h, KMR_ERR_INVALID_ARG, std::string(what) + " text too large for one call");
	X.per_block.take(X.blk, 4 * X.nblk); X.per_block.take(X.bbase, 8 * (X.nblk + 1));
	if (!is_fasta) { X.per_block.take(X.btok, 4 * X.nblk); X.per_block.take(X.tbase, 8 * (X.nblk + 1)); }
	{ int rc = X.per_block.reserve(h, bufs[0]); if (rc) return rc; }
	LAUNCH(h, ingest_count_lines, dim3((unsigned)X.nblk), dim3(ING_THREADS), 0, text, len, X.blk.get<uint32_t>());
	{ int rc = exclusive_scan(h, X.blk.get<uint32_t>(), X.nblk, X.bbase.get<uint64_t>()); if (rc) return rc; }
	HIPCHK(h, hipMemcpy(&X.n_lines, X.bbase.get<uint64_t>() + X.nblk, 8, hipMemcpyDeviceToHost));
	if (!X.n_lines) return fail(h, KMR_ERR_INVALID_ARG, std::string("malformed ") + what + ":" + fasta_why(FA_ERR_LEAD));      /* newlines only */
	const uint64_t nl = X.n_lines;
	X.per_line.take(X.lstart, 8 * nl); X.per_line.take(X.llen, 4 * nl); X.per_line.take(X.ishdr, 4 * nl); X.per_line.take(X.hidx, 8 * (nl + 1));
	if (is_fasta) { X.per_line.take(X.klen, 4 * nl); X.per_line.take(X.loff, 8 * (nl + 1)); }
	else { X.per_line.take(X.tline, 8 * (nl + 1)); X.per_line.take(X.lout, 8 * nl); X.per_line.take(X.lread, 4 * nl); }
	{ int rc = X.per_line.reserve(h, bufs[1]); if (rc) return rc; }
	LAUNCH(h, ingest_index_lines, dim3((unsigned)X.nblk), dim3(ING_THREADS), 0, text, len, X.bbase.get<uint64_t>(), X.lstart.get<uint64_t>());
	LAUNCH(h, ingest_line_lengths, dim3(grid_for(nl)), dim3(256), 0, text, len, X.lstart.get<uint64_t>(), nl, X.llen.get<uint32_t>(), derr, true);
	LAUNCH(h, fasta_classify, dim3(grid_for(nl)), dim3(256), 0, text, X.lstart.get<uint64_t>(), X.llen.get<uint32_t>(), nl, X.ishdr.get<uint32_t>(), derr);
	{ int rc = exclusive_scan(h, X.ishdr.get<uint32_t>(), nl, X.hidx.get<uint64_t>()); if (rc) return rc; }
	{ int rc = fasta_check(h, derr, what); if (rc) return rc; }
	HIPCHK(h, hipMemcpy(&X.nrec, X.hidx.get<uint64_t>() + nl, 8, hipMemcpyDeviceToHost));
	X.per_record.take(X.recline, 8 * X.nrec);
	if (is_fasta) { X.per_record.take(X.keep, 4 * X.nrec); X.per_record.take(X.kidx, 8 * (X.nrec + 1)); }
	{ int rc = X.per_record.reserve(h, bufs[2]); if (rc) return rc; }
	LAUNCH(h, fasta_headers, dim3(grid_for(nl)), dim3(256), 0, text, X.lstart.get<uint64_t>(), X.llen.get<uint32_t>(), X.ishdr.get<uint32_t>(), X.hidx.get<uint64_t>(), nl,
	       store_comment, X.recline.get<uint64_t>(), X.keep.get<uint32_t>(), derr);
	return 0;
}

int ingest_fasta_dev(kmr_handle *h, const uint8_t *text, uint64_t len, const uint8_t *qtext, uint64_t qlen, bool with_qual, int store_comment, kmr_reads **out) {
	const uint32_t start = h->cfg.fastq_start_char;
	if (start != 33 && start != 64) return fail(h, KMR_ERR_INVALID_ARG, "fastq quality base must be 33 or 64 (src/Options.h:490)");
	auto R = make_result<kmr_reads>(h);
	R->input_base = start;
	FastaIndex F, Q;
	DevBuf derr;
	HIPCHK(h, derr.alloc(16)); HIPCHK(h, hipMemsetAsync(derr.get<uint32_t>(), 0, 16, h->stream));
	uint32_t *ferr = derr.get<uint32_t>(), *qerr = ferr + 1, *flip = ferr + 2;
	{ int rc = fasta_index(h, text, len, store_comment, true, ferr, "FASTA", F); if (rc) return rc; }
	if (with_qual) {
		int rc = fasta_index(h, qtext, qlen, store_comment, false, qerr, "QUAL", Q); if (rc) return rc;
		if (Q.nrec != F.nrec) return fail(h, KMR_ERR_INVALID_ARG, "malformed QUAL: " + std::to_string(Q.nrec) + " records for the " + std::to_string(F.nrec) + " of the FASTA");
	}
	const uint64_t nl = F.n_lines, nrec = F.nrec;
	uint64_t n_kept = 0, total = 0;
	if (nrec) {
		LAUNCH(h, fasta_kept_lengths, dim3(grid_for(nl)), dim3(256), 0, F.llen.get<uint32_t>(), F.ishdr.get<uint32_t>(), F.hidx.get<uint64_t>(), F.keep.get<uint32_t>(), nl, F.klen.get<uint32_t>());
		{ int rc = exclusive_scan(h, F.keep.get<uint32_t>(), nrec, F.kidx.get<uint64_t>()); if (rc) return rc; }
		{ int rc = exclusive_scan(h, F.klen.get<uint32_t>(), nl, F.loff.get<uint64_t>()); if (rc) return rc; }
		{ int rc = fasta_check(h, ferr, "FASTA"); if (rc) return rc; }      /* the names */
		HIPCHK(h, hipMemcpy(&n_kept, F.kidx.get<uint64_t>() + nrec, 8, hipMemcpyDeviceToHost)); HIPCHK(h, hipMemcpy(&total, F.loff.get<uint64_t>() + nl, 8, hipMemcpyDeviceToHost));
	}
	R->n = n_kept; R->total = total; R->filtered = nrec - n_kept;
	HIPCHK(h, R->bases.alloc(total + 64)); HIPCHK(h, R->quals.alloc(total + 64)); HIPCHK(h, R->offsets.alloc(8 * (n_kept + 1)));
	HIPCHK(h, R->name_off.alloc(8 * std::max<uint64_t>(1, n_kept))); HIPCHK(h, R->name_len.alloc(4 * std::max<uint64_t>(1, n_kept)));
	HIPCHK(h, hipMemsetAsync(R->bases.get<uint8_t>() + total, 0, 64, h->stream)); HIPCHK(h, hipMemsetAsync(R->quals.get<uint8_t>() + total, 0, 64, h->stream));
	HIPCHK(h, hipMemcpyAsync(R->offsets.get<uint64_t>() + n_kept, &total, 8, hipMemcpyHostToDevice, h->stream));
	if (nrec) {
		LAUNCH(h, fasta_records, dim3(grid_for(nrec)), dim3(256), 0, F.lstart.get<uint64_t>(), F.llen.get<uint32_t>(), F.recline.get<uint64_t>(), F.keep.get<uint32_t>(), F.kidx.get<uint64_t>(),
		       F.loff.get<uint64_t>(), nrec, nl, R->offsets.get<uint64_t>(), R->name_off.get<uint64_t>(), R->name_len.get<uint32_t>(), ferr);
	}
	if (total) {
		const uint64_t nb = (total + (uint64_t)ING_THREADS * ING_BYTES - 1) / ((uint64_t)ING_THREADS * ING_BYTES);
		if (nb > 0x7fffffffull) return fail(h, KMR_ERR_INVALID_ARG, "FASTA text too large for one call");
		LAUNCH(h, fasta_copy, dim3((unsigned)nb), dim3(ING_THREADS), 0, text, len, F.lstart.get<uint64_t>(), F.loff.get<uint64_t>(), nl, total, R->bases.get<uint8_t>());
	}
	if (!with_qual) {
		if (total) HIPCHK(h, hipMemsetAsync(R->quals.get<uint8_t>(), 127, total, h->stream));      /* Read::REF_QUAL, src/ReadFileReader.h:892,901 */
	} else if (nrec) {
		const uint64_t ql = Q.n_lines, n_window = std::min<uint64_t>(n_kept, ING_VALIDATE_READS - 1);
		DevBuf inrange;
		HIPCHK(h, inrange.alloc(4 * std::max<uint64_t>(1, n_window))); HIPCHK(h, hipMemsetAsync(inrange.get<uint32_t>(), 0, 4 * std::max<uint64_t>(1, n_window), h->stream));
		auto tokens = [&](auto mode) -> int {
			LAUNCH(h, fasta_qual_tokens<decltype(mode)::value>, dim3((unsigned)Q.nblk), dim3(ING_THREADS), 0, qtext, qlen, Q.bbase.get<uint64_t>(), Q.ishdr.get<uint32_t>(), ql,
			       Q.btok.get<uint32_t>(), Q.tbase.get<uint64_t>(), Q.tline.get<uint64_t>(), Q.lout.get<uint64_t>(), Q.lread.get<uint32_t>(), start, R->quals.get<uint8_t>(), inrange.get<uint32_t>(), qerr);
			return 0;
		};
		{ int rc = tokens(int_c<0>()); if (rc) return rc; }
		{ int rc = exclusive_scan(h, Q.btok.get<uint32_t>(), Q.nblk, Q.tbase.get<uint64_t>()); if (rc) return rc; }
		{ int rc = tokens(int_c<1>()); if (rc) return rc; }
		LAUNCH(h, fasta_qual_lines, dim3(grid_for(ql)), dim3(256), 0, qtext, Q.lstart.get<uint64_t>(), Q.llen.get<uint32_t>(), Q.ishdr.get<uint32_t>(), Q.hidx.get<uint64_t>(), Q.recline.get<uint64_t>(), ql,
		       Q.tline.get<uint64_t>(), text, F.lstart.get<uint64_t>(), F.llen.get<uint32_t>(), F.recline.get<uint64_t>(), F.keep.get<uint32_t>(), F.kidx.get<uint64_t>(), R->offsets.get<uint64_t>(), nrec,
		       store_comment, Q.lout.get<uint64_t>(), Q.lread.get<uint32_t>(), qerr);
		/* every kept record has as many numbers as bases before a single one is written */
		{ int rc = fasta_check(h, qerr, "QUAL"); if (rc) return rc; }
		{ int rc = tokens(int_c<2>()); if (rc) return rc; }
		if (n_window) LAUNCH(h, fasta_qual_flip, dim3(grid_for(n_window)), dim3(256), 0, inrange.get<uint32_t>(), n_window, flip);
		uint32_t f = 0;
		HIPCHK(h, fetch(h, &f, flip));
		if (f) {      /* __setFastqStart(the other base), src/ReadSet.h:174-186, with the input base equal to the start character */
			const uint32_t want = start == 33 ? 64u : 33u;
			if (total) LAUNCH(h, ingest_shift_quals, dim3(grid_for(total)), dim3(256), 0, R->quals.get<uint8_t>(), total, (int)start - (int)want);
			R->input_base = want;
		}
	}
	{ int rc = fasta_check(h, ferr, "FASTA"); if (rc) return rc; }      /* a record too long; waits for the stream */
	*out = R.release();
	return KMR_OK;
}

/* the text as the kernels like it: a fresh aligned copy with slack behind it */
int fasta_upload(kmr_handle *h, const char *text, uint64_t len, const char *what, DevBuf &d) {
	HIPCHK(h, d.alloc(len + 16));
	const hipError_t e = len ? hipMemcpy(d.get(), text, len, hipMemcpyHostToDevice) : hipSuccess;
	if (e != hipSuccess) { h->err = std::string("hipMemcpy(") + what + " text): " + hipGetErrorString(e); return KMR_ERR_HIP; }
	return 0;
}

}  // namespace

extern "C" {

int kmr_ingest_fasta_dev(kmr_handle *h, const void *dev_text, uint64_t len, const void *dev_qual_text, uint64_t qual_len, int store_comment, kmr_reads **out) {
	if (out) *out = nullptr;
	if (!h || !out || (len && !dev_text) || (qual_len && !dev_qual_text)) return KMR_ERR_INVALID_ARG;
	hipSetDevice(h->device);
	return ingest_fasta_dev(h, (const uint8_t *)dev_text, len, (const uint8_t *)dev_qual_text, qual_len, dev_qual_text != nullptr, store_comment, out);
}
int kmr_ingest_fasta(kmr_handle *h, const char *text, uint64_t len, const char *qual_text, uint64_t qual_len, int store_comment, kmr_reads **out) {
	if (out) *out = nullptr;
	if (!h || !out || (len && !text) || (qual_len && !qual_text)) return KMR_ERR_INVALID_ARG;
	hipSetDevice(h->device);
	DevBuf d, q;
	{ int rc = fasta_upload(h, text, len, "FASTA", d); if (rc) return rc; }
	if (qual_text) { int rc = fasta_upload(h, qual_text, qual_len, "QUAL", q); if (rc) return rc; }
	return ingest_fasta_dev(h, d.get<uint8_t>(), len, q.get<uint8_t>(), qual_len, qual_text != nullptr, store_comment, out);
}

/* a device-resident batch from reads the host already parsed (the reference's ReadSet flattened as for kmr_add_reads) */
int kmr_reads_from_host(kmr_handle *h, const char *bases, const char *quals, const uint64_t *offsets, uint64_t n_reads, kmr_reads **out) {
	if (!h || !out || !offsets || (n_reads && (!bases || !quals))) return KMR_ERR_INVALID_ARG;
	*out = nullptr;
	hipSetDevice(h->device);
	const uint64_t first = offsets[0], total = offsets[n_reads] - first;
	auto r = make_result<kmr_reads>(h);
	r->n = n_reads; r->total = total; r->input_base = h->cfg.fastq_start_char;
	HIPCHK(h, r->bases.alloc(total + 64)); HIPCHK(h, r->quals.alloc(total + 64));
	HIPCHK(h, r->offsets.alloc(8 * (n_reads + 1)));
	HIPCHK(h, r->name_off.alloc(8 * std::max<uint64_t>(n_reads, 1))); HIPCHK(h, r->name_len.alloc(4 * std::max<uint64_t>(n_reads, 1)));
	HIPCHK(h, hipMemset(r->bases.get<uint8_t>() + total, 0, 64)); HIPCHK(h, hipMemset(r->quals.get<uint8_t>() + total, 0, 64));
	HIPCHK(h, hipMemset(r->name_off.get<uint64_t>(), 0, 8 * std::max<uint64_t>(n_reads, 1))); HIPCHK(h, hipMemset(r->name_len.get<uint32_t>(), 0, 4 * std::max<uint64_t>(n_reads, 1)));
	if (total) { HIPCHK(h, hipMemcpy(r->bases.get<uint8_t>(), bases + first, total, hipMemcpyHostToDevice)); HIPCHK(h, hipMemcpy(r->quals.get<uint8_t>(), quals + first, total, hipMemcpyHostToDevice)); }
	std::vector<uint64_t> rel(n_reads + 1);
	for (uint64_t i = 0; i <= n_reads; i++) rel[i] = offsets[i] - first;
	HIPCHK(h, hipMemcpy(r->offsets.get<uint64_t>(), rel.data(), 8 * (n_reads + 1), hipMemcpyHostToDevice));
	*out = r.release();
	return KMR_OK;
}
void kmr_reads_free(kmr_reads *r) { free_on_device(r); }
int kmr_reads_info(const kmr_reads *r, uint64_t *n_reads, uint64_t *total_bases, uint32_t *input_quality_base, uint64_t *n_filtered) {
	if (!r) return KMR_ERR_INVALID_ARG;
	if (n_reads) *n_reads = r->n; if (total_bases) *total_bases = r->total;
	if (input_quality_base) *input_quality_base = r->input_base; if (n_filtered) *n_filtered = r->filtered;
	return KMR_OK;
}
int kmr_reads_device_ptrs(const kmr_reads *r, void **bases, void **quals, void **offsets) {
	if (!r) return KMR_ERR_INVALID_ARG;
	if (bases) *bases = r->bases.get<uint8_t>(); if (quals) *quals = r->quals.get<uint8_t>(); if (offsets) *offsets = r->offsets.get<uint64_t>();
	return KMR_OK;
}
int kmr_reads_copy(const kmr_reads *r, char *bases, char *quals, uint64_t *offsets, uint64_t *name_off, uint32_t *name_len) {
	if (!r) return KMR_ERR_INVALID_ARG;
	hipSetDevice(r->device);
	hipError_t e = hipSuccess;
	copy_out(e, (uint8_t *)bases, r->bases, r->total); copy_out(e, (uint8_t *)quals, r->quals, r->total); copy_out(e, offsets, r->offsets, r->n + 1);
	copy_out(e, name_off, r->name_off, r->n); copy_out(e, name_len, r->name_len, r->n);
	return e == hipSuccess ? KMR_OK : KMR_ERR_HIP;
}

/* ReadSet::circularize (src/ReadSet.cpp:120-130) */
int kmr_reads_circularize(kmr_handle *h, const kmr_reads *in, uint32_t extra_length, kmr_reads **out) {
	if (out) *out = nullptr;
	if (!h || !in || !out) return fail(h, KMR_ERR_INVALID_ARG, "kmr_reads_circularize: NULL argument");
	if (in->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "read batch lives on another device");
	hipSetDevice(h->device);
	const uint64_t n = in->n, n1 = std::max<uint64_t>(n, 1);
	auto r = make_result<kmr_reads>(h);
	r->n = n; r->input_base = in->input_base; r->filtered = in->filtered;
	Scratch tmp(h);
	uint32_t *len, *err; uint64_t *off;
	HIPCHK(h, tmp.take(&len, n1)); HIPCHK(h, tmp.take(&err, (size_t)1));
	HIPCHK(h, alloc_n(r->offsets, &off, n + 1));
	HIPCHK(h, r->name_off.alloc(8 * n1)); HIPCHK(h, r->name_len.alloc(4 * n1));
	HIPCHK(h, hipMemsetAsync(err, 0, 4, h->stream)); HIPCHK(h, hipMemsetAsync(off, 0, 8, h->stream));
	HIPCHK(h, hipMemsetAsync(r->name_off.get(), 0, 8 * n1, h->stream)); HIPCHK(h, hipMemsetAsync(r->name_len.get(), 0, 4 * n1, h->stream));
	uint32_t herr = 0;
	if (n) {
		HIPCHK(h, hipMemcpyAsync(r->name_off.get(), in->name_off.get(), 8 * n, hipMemcpyDeviceToDevice, h->stream));
		HIPCHK(h, hipMemcpyAsync(r->name_len.get(), in->name_len.get(), 4 * n, hipMemcpyDeviceToDevice, h->stream));
		LAUNCH(h, circularize_lengths_kernel, dim3(grid_for(n)), dim3(256), 0, in->offsets.get<uint64_t>(), n, extra_length, len, err);
		int rc = exclusive_scan(h, len, n, off); if (rc) return rc;
		HIPCHK(h, hipMemcpy(&r->total, off + n, 8, hipMemcpyDeviceToHost));
		HIPCHK(h, hipMemcpy(&herr, err, 4, hipMemcpyDeviceToHost));
		if (herr) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_reads_circularize: a read of 2^32 bases or more");
	}
	uint8_t *cb, *cq;
	HIPCHK(h, alloc_n(r->bases, &cb, r->total + 64)); HIPCHK(h, alloc_n(r->quals, &cq, r->total + 64));
	HIPCHK(h, hipMemsetAsync(cb + r->total, 0, 64, h->stream)); HIPCHK(h, hipMemsetAsync(cq + r->total, 0, 64, h->stream));
	if (r->total) {
		LAUNCH(h, circularize_copy_kernel, dim3((unsigned)std::min<uint64_t>((n + 3) / 4, (uint64_t)num_cus(h) * 32)), dim3(256), 0,
		       in->bases.get<uint8_t>(), in->quals.get<uint8_t>(), in->offsets.get<uint64_t>(), n, (const uint64_t *)off, cb, cq);
	}
	HIPCHK(h, hipStreamSynchronize(h->stream));
	tmp.done();
	*out = r.release();
	return KMR_OK;
}

/* ---- CompareSpectrums (apps/CompareSpectrums.cpp; kernels: kmr_compare.hpp, launched by kmr_api.hip's compare_*_core) ---- */
int kmr_compare_spectrums(kmr_handle *h1, kmr_handle *h2, kmr_compare_counts *out) {
	if (!h1 || !h2 || !out) return fail(h2, KMR_ERR_INVALID_ARG, "kmr_compare_spectrums: NULL argument");
	if (!h1->finalized || !h2->finalized) return fail(h2, KMR_ERR_STATE, "kmr_compare_spectrums before kmr_finalize");
	if (h1->device != h2->device) return fail(h2, KMR_ERR_INVALID_ARG, "kmr_compare_spectrums: the spectra live on different devices");
	if (h1->k != h2->k || h1->cfg.hash_kind != h2->cfg.hash_kind) return fail(h2, KMR_ERR_INVALID_ARG, "kmr_compare_spectrums: the spectra differ in k or hash_kind");
	hipSetDevice(h2->device);
	return compare_spectrums_core(h1, h2, out);
}
static int compare_reads_check(kmr_handle *h2, const kmr_reads *set1, const void *dst) {
	if (!h2 || !set1 || (set1->n && !dst)) return fail(h2, KMR_ERR_INVALID_ARG, "kmr_compare_reads: NULL argument");
	if (!h2->finalized) return fail(h2, KMR_ERR_STATE, "kmr_compare_reads before kmr_finalize");
	if (set1->device != h2->device) return fail(h2, KMR_ERR_INVALID_ARG, "read batch lives on another device");
	if (h2->cfg.world_size > 1 || h2->cfg.num_parts > 1 || h2->cfg.kmer_subsample > 1)
		return fail(h2, KMR_ERR_UNSUPPORTED, "kmr_compare_reads: a handle with world_size > 1, num_parts > 1 or kmer_subsample > 1 holds a part of the spectrum only");
	return KMR_OK;
}
int kmr_compare_reads_dev(kmr_handle *h2, const kmr_reads *set1, void *dev_per_read) {
	int rc = compare_reads_check(h2, set1, dev_per_read); if (rc) return rc;
	if (set1->n == 0) return KMR_OK;
	hipSetDevice(h2->device);
	return compare_reads_core(h2, set1->bases.get<uint8_t>(), set1->quals.get<uint8_t>(), set1->offsets.get<uint64_t>(), set1->n, dev_per_read);
}
int kmr_compare_reads(kmr_handle *h2, const kmr_reads *set1, kmr_compare_counts *per_read) {
	int rc = compare_reads_check(h2, set1, per_read); if (rc) return rc;
	if (set1->n == 0) return KMR_OK;
	hipSetDevice(h2->device);
	Scratch tmp(h2);
	kmr_compare_counts *d;
	HIPCHK(h2, tmp.take(&d, set1->n));
	rc = compare_reads_core(h2, set1->bases.get<uint8_t>(), set1->quals.get<uint8_t>(), set1->offsets.get<uint64_t>(), set1->n, d); if (rc) return rc;
	HIPCHK(h2, hipMemcpyAsync(per_read, d, sizeof(kmr_compare_counts) * set1->n, hipMemcpyDeviceToHost, h2->stream));
	HIPCHK(h2, hipStreamSynchronize(h2->stream));
	tmp.done();
	return KMR_OK;
}
/* one line of the table (:234-241); needs no device */
int kmr_compare_line(const kmr_compare_counts *c, const char *label, uint64_t label_len, char *dst, uint64_t cap, uint64_t *bytes) {
	if (!c || !bytes || (label_len && !label) || (cap && !dst)) return KMR_ERR_INVALID_ARG;
	char buf[256];
	int n = snprintf(buf, sizeof(buf), "%llu\t%llu\t%llu", (unsigned long long)c->size1, (unsigned long long)c->size2, (unsigned long long)c->common);
	const uint64_t num[4] = {c->common, c->common_count1, c->common, c->common_count2}, den[4] = {c->size1, c->total_count1, c->size2, c->total_count2};
	for (int i = 0; i < 4; i++) {
		/* 0.0 / 0.0 in the reference: "-nan" from an x86-64 glibc build, written as that on every host */
		if (den[i] == 0) n += snprintf(buf + n, sizeof(buf) - n, "\t-nan");
		else n += snprintf(buf + n, sizeof(buf) - n, "\t%.4g", (double)num[i] * 100.0 / (double)den[i]);
	}
	*bytes = (uint64_t)n + 1 + label_len + 1;
	if (cap < *bytes) return KMR_ERR_CAPACITY;
	memcpy(dst, buf, n); dst[n] = '\t';
	if (label_len) memcpy(dst + n + 1, label, label_len);
	dst[n + 1 + label_len] = '\n';
	return KMR_OK;
}

/* ---- KmerMatch (src/KmerMatch.h, src/MatcherInterface.h; kernels: kmr_match.hpp; the table and the streaming pass are kmr_api.hip's match_*_core) ---- */
int kmr_match_config_init(kmr_match_config *c) {
	if (!c) return KMR_ERR_INVALID_ARG;
	memset(c, 0, sizeof(*c));
	c->struct_size = (uint32_t)sizeof(kmr_match_config);
	c->max_positions_from_edge = 500;      /* --match-max-positions-from-edge, KmerMatch.h:60 */
	c->max_read_matches = 450;             /* --max-read-matches, MatcherInterface.h:77 */
	c->include_mate = 1;                   /* --include-mate, MatcherInterface.h:71 */
	c->seed = 0;
	return KMR_OK;
}
/* KmerMatch's constructor and the contig side of _matchLocal (KmerMatch.h:100-107, :124-149) */
int kmr_match_create(kmr_handle *h, const kmr_reads *contigs, const kmr_match_config *cfg, kmr_match **out) {
	if (out) *out = nullptr;
	if (!h || !contigs || !cfg || !out) return fail(h, KMR_ERR_INVALID_ARG, "kmr_match_create: NULL argument");
	if (cfg->struct_size != sizeof(kmr_match_config)) return fail(h, KMR_ERR_INVALID_ARG, "kmr_match_config: struct_size " + std::to_string(cfg->struct_size) + " is not " + std::to_string(sizeof(kmr_match_config)));
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_match_create before kmr_finalize");
	if (contigs->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "kmr_match_create: the contigs live on another device");
	if (h->cfg.world_size > 1 || h->cfg.num_parts > 1 || h->cfg.kmer_subsample > 1)
		return fail(h, KMR_ERR_UNSUPPORTED, "kmr_match_create: a handle with world_size > 1, num_parts > 1 or kmer_subsample > 1 holds a part of the spectrum only");
	if (contigs->n > MATCH_MAX_CONTIGS) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_match_create: more than 2^24 contigs");
	hipSetDevice(h->device);
	auto m = make_result<kmr_match>(h);
	m->h = h; m->cfg = *cfg;
	const int rc = match_create_core(h, m.get(), contigs->bases.get<uint8_t>(), contigs->offsets.get<uint64_t>(), contigs->n); if (rc) return rc;
	*out = m.release();
	return KMR_OK;
}
int kmr_match_edge_info(const kmr_match *m, uint64_t *n_contigs, uint64_t *n_edge_kmers, uint64_t *n_distinct_keys, uint64_t *n_keys_in_spectrum) {
	if (!m) return KMR_ERR_INVALID_ARG;
	if (n_contigs) *n_contigs = m->n_contigs;
	if (n_edge_kmers) *n_edge_kmers = m->n_edge_kmers;
	if (n_distinct_keys) *n_distinct_keys = m->n_distinct_keys;
	if (n_keys_in_spectrum) *n_keys_in_spectrum = m->n_keys_in_spectrum;
	return KMR_OK;
}
/* the reads' side of _matchLocal's lookups (KmerMatch.h:151-161) and the mate of every hit (MatcherInterface.h:785-791) */
int kmr_match_add_read_batch(kmr_match *m, const kmr_reads *reads, uint64_t first_global_read_idx, const kmr_pairs *pairs, const uint8_t *discarded) {
	if (!m) return KMR_ERR_INVALID_ARG;
	kmr_handle *h = m->h;
	if (!reads) return fail(h, KMR_ERR_INVALID_ARG, "kmr_match_add_read_batch: NULL argument");
	if (m->finished) return fail(h, KMR_ERR_STATE, "kmr_match_add_read_batch after kmr_match_finish");
	if (reads->device != m->device || (pairs && pairs->device != m->device)) return fail(h, KMR_ERR_INVALID_ARG, "kmr_match_add_read_batch: the batch or its pairing lives on another device");
	if (pairs && pairs->n != reads->n) return fail(h, KMR_ERR_INVALID_ARG, "kmr_match_add_read_batch: the pairing is of another number of reads");
	if (first_global_read_idx > MATCH_READ_MASK || reads->n > MATCH_READ_MASK - first_global_read_idx) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_match_add_read_batch: a global read index of 2^40 or more");
	if (reads->n == 0) return KMR_OK;
	hipSetDevice(m->device);
	kmr_match::Batch b;      /* kept only if the batch went through */
	b.first = first_global_read_idx; b.n = reads->n;
	if (discarded) {
		HIPCHK(h, b.discarded.alloc(std::max<size_t>(reads->n, 256)));
		HIPCHK(h, hipMemcpy(b.discarded.get(), discarded, reads->n, hipMemcpyHostToDevice));
	}
	const int rc = match_add_core(h, m, reads->bases.get<uint8_t>(), reads->quals.get<uint8_t>(), reads->offsets.get<uint64_t>(), reads->n, first_global_read_idx,
	                              (pairs && m->cfg.include_mate) ? pairs->mate.get<int64_t>() : nullptr, b.discarded.get<uint8_t>());      /* (waits for the stream) */
	if (rc) return rc;
	m->batches.push_back(std::move(b));
	return KMR_OK;
}
/* the end of _matchLocal (KmerMatch.h:163-171), exchangeGlobalReadIdxs' mates (MatcherInterface.h:772-792) and getLocalReads' sorted,
 * undiscarded reads (:311-321) */
int kmr_match_finish(kmr_match *m) {
	if (!m) return KMR_ERR_INVALID_ARG;
	kmr_handle *h = m->h;
	if (m->finished) return fail(h, KMR_ERR_STATE, "kmr_match_finish twice");
	hipSetDevice(m->device);
	const uint64_t nc = m->n_contigs, nh = m->n_hits;
	if (nh >= 0xffffffffull) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_match_finish: 2^32 - 1 hit records or more");
	const dim3 block(256);
	Scratch tmp(h);
	uint64_t *offsets, *before, *after, *bound, *bound2;
	HIPCHK(h, alloc_n(m->offsets, &offsets, nc + 1)); HIPCHK(h, alloc_n(m->size_before, &before, std::max<uint64_t>(nc, 1))); HIPCHK(h, alloc_n(m->size_after, &after, std::max<uint64_t>(nc, 1)));
	HIPCHK(h, hipMemsetAsync(offsets, 0, 8 * (nc + 1), h->stream)); HIPCHK(h, hipMemsetAsync(before, 0, 8 * std::max<uint64_t>(nc, 1), h->stream)); HIPCHK(h, hipMemsetAsync(after, 0, 8 * std::max<uint64_t>(nc, 1), h->stream));
	m->n_reads_total = 0; m->n_sampled = 0;
	uint64_t n_out = 0;
	if (nh && nc) {
		/* 1: the records in (contig, read) order, made unique */
		unsigned long long *k1, *ukey, *umate; uint32_t *p0, *p1, *flag; uint64_t *scan;
		HIPCHK(h, tmp.take(&k1, nh)); HIPCHK(h, tmp.take(&ukey, nh)); HIPCHK(h, tmp.take(&umate, nh)); HIPCHK(h, tmp.take(&p0, nh)); HIPCHK(h, tmp.take(&p1, nh));
		HIPCHK(h, tmp.take(&flag, 2 * nh)); HIPCHK(h, tmp.take(&scan, 2 * (nh + 1))); HIPCHK(h, tmp.take(&bound, nc + 1)); HIPCHK(h, tmp.take(&bound2, nc + 1));
		int rc = sort_reserve(h, tmp.sort, nh, "kmr_match_finish"); if (rc) return rc;
		const dim3 hgrid(grid_for(nh)), cgrid(grid_for(nc + 1));
		LAUNCH(h, match_iota_kernel, hgrid, block, 0, p0, nh);
		rc = sort_pairs(h, tmp.sort, m->hit_key.get<unsigned long long>(), k1, p0, p1, nh, "kmr_match_finish"); if (rc) return rc;
		LAUNCH(h, match_heads_kernel, hgrid, block, 0, (const unsigned long long *)k1, nh, flag);
		rc = exclusive_scan_queue(h, flag, nh, scan); if (rc) return rc;
		LAUNCH(h, match_compact_kernel, hgrid, block, 0, (const unsigned long long *)k1, (const uint32_t *)p1, m->hit_mate.get<unsigned long long>(), (const uint32_t *)flag,
		       (const uint64_t *)scan, nh, ukey, umate);
		uint64_t nu = 0;
		HIPCHK(h, fetch(h, &nu, scan + nh));
		/* 2: the sets' sizes, the sampling, the mates of the reads that stay */
		const dim3 ugrid(grid_for(nu));
		uint32_t *keep = flag, *cnt = flag + nh; uint64_t *kscan = scan, *escan = scan + (nh + 1);
		LAUNCH(h, match_bounds_kernel, cgrid, block, 0, (const unsigned long long *)ukey, nu, nc, bound);
		LAUNCH(h, match_sample_kernel, ugrid, block, 0, (const unsigned long long *)ukey, (const unsigned long long *)umate, nu, (const uint64_t *)bound, m->cfg.max_read_matches,
		       m->cfg.include_mate, m->cfg.seed, keep, cnt);
		rc = exclusive_scan_queue(h, keep, nu, kscan); if (rc) return rc;
		rc = exclusive_scan_queue(h, cnt, nu, escan); if (rc) return rc;
		LAUNCH(h, match_sizes_kernel, cgrid, block, 0, (const uint64_t *)bound, (const uint64_t *)kscan, nc, before, after);
		uint64_t ne = 0;
		HIPCHK(h, fetch(h, &ne, escan + nu));
		if (ne >= 0xffffffffull) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_match_finish: 2^32 - 1 reads and mates or more");
		if (ne) {
			unsigned long long *e0, *e1; uint32_t *q0, *q1, *fflag; uint64_t *fscan;
			HIPCHK(h, tmp.take(&e0, ne)); HIPCHK(h, tmp.take(&e1, ne)); HIPCHK(h, tmp.take(&q0, ne)); HIPCHK(h, tmp.take(&q1, ne)); HIPCHK(h, tmp.take(&fflag, ne)); HIPCHK(h, tmp.take(&fscan, ne + 1));
			const dim3 egrid(grid_for(ne));
			LAUNCH(h, match_emit_kernel, ugrid, block, 0, (const unsigned long long *)ukey, (const unsigned long long *)umate, nu, (const uint32_t *)cnt, (const uint64_t *)escan, e0);
			LAUNCH(h, match_iota_kernel, egrid, block, 0, q0, ne);
			/* 3: sorted and made unique again, without the discarded reads */
			rc = sort_reserve(h, tmp.sort, ne, "kmr_match_finish"); if (rc) return rc;
			rc = sort_pairs(h, tmp.sort, e0, e1, q0, q1, ne, "kmr_match_finish"); if (rc) return rc;
			const uint32_t nb = (uint32_t)m->batches.size();
			std::vector<uint64_t> bf(nb), bn(nb); std::vector<const uint8_t *> bp(nb);
			for (uint32_t i = 0; i < nb; i++) { bf[i] = m->batches[i].first; bn[i] = m->batches[i].n; bp[i] = m->batches[i].discarded.get<uint8_t>(); }
			MatchBatches B; B.nb = nb;
			const uint64_t *dbf, *dbn; const uint8_t *const *dbp;
			rc = to_device(h, tmp, (const uint64_t *)bf.data(), (uint64_t)nb, &dbf); if (rc) return rc;
			rc = to_device(h, tmp, (const uint64_t *)bn.data(), (uint64_t)nb, &dbn); if (rc) return rc;
			rc = to_device(h, tmp, (const uint8_t *const *)bp.data(), (uint64_t)nb, &dbp); if (rc) return rc;
			B.first = dbf; B.n = dbn; B.flags = dbp;
			LAUNCH(h, match_final_kernel, egrid, block, 0, (const unsigned long long *)e1, ne, B, fflag);
			rc = exclusive_scan_queue(h, fflag, ne, fscan); if (rc) return rc;
			HIPCHK(h, fetch(h, &n_out, fscan + ne));      /* (bf, bn, bp have been read) */
			uint64_t *ids;
			HIPCHK(h, alloc_n(m->read_ids, &ids, std::max<uint64_t>(n_out, 1)));
			LAUNCH(h, match_bounds_kernel, cgrid, block, 0, (const unsigned long long *)e1, ne, nc, bound2);
			LAUNCH(h, match_output_kernel, egrid, block, 0, (const unsigned long long *)e1, ne, (const uint32_t *)fflag, (const uint64_t *)fscan, ids);
			LAUNCH(h, match_offsets_kernel, cgrid, block, 0, (const uint64_t *)bound2, (const uint64_t *)fscan, nc, offsets);
		}
		/* the sets that were sampled: the sizes are small, the host counts them */
		std::vector<uint64_t> hb(nc);
		HIPCHK(h, fetch(h, hb.data(), before, nc));
		const float maxHits = (float)(2.0 * (double)m->cfg.max_read_matches);
		if (m->cfg.max_read_matches) for (uint64_t c = 0; c < nc; c++) if ((float)(long long)hb[c] > maxHits) m->n_sampled++;
	}
	if (!m->read_ids) { uint64_t *ids; HIPCHK(h, alloc_n(m->read_ids, &ids, (size_t)1)); }
	HIPCHK(h, hipStreamSynchronize(h->stream));
	tmp.done();
	m->n_reads_total = n_out;
	m->hit_key.reset(); m->hit_mate.reset(); m->batches.clear();      /* the stream is idle */
	m->finished = true;
	return KMR_OK;
}
int kmr_match_info(const kmr_match *m, uint64_t *n_contigs, uint64_t *n_reads_total, uint64_t *n_sampled_contigs) {
	if (!m) return KMR_ERR_INVALID_ARG;
	if (!m->finished) return fail(m->h, KMR_ERR_STATE, "kmr_match_info before kmr_match_finish");
	if (n_contigs) *n_contigs = m->n_contigs;
	if (n_reads_total) *n_reads_total = m->n_reads_total;
	if (n_sampled_contigs) *n_sampled_contigs = m->n_sampled;
	return KMR_OK;
}
int kmr_match_copy(const kmr_match *m, uint64_t *offsets, uint64_t *read_ids, uint64_t *size_before_sampling, uint64_t *size_after_sampling) {
	if (!m) return KMR_ERR_INVALID_ARG;
	if (!m->finished) return fail(m->h, KMR_ERR_STATE, "kmr_match_copy before kmr_match_finish");
	hipSetDevice(m->device);
	hipError_t e = hipSuccess;
	copy_out(e, offsets, m->offsets, m->n_contigs + 1);
	copy_out(e, read_ids, m->read_ids, m->n_reads_total);
	copy_out(e, size_before_sampling, m->size_before, m->n_contigs);
	copy_out(e, size_after_sampling, m->size_after, m->n_contigs);
	HIPCHK(m->h, e);
	return KMR_OK;
}
int kmr_match_device_ptrs(const kmr_match *m, void **dev_offsets, void **dev_read_ids, void **dev_size_before_sampling, void **dev_size_after_sampling) {
	if (!m) return KMR_ERR_INVALID_ARG;
	if (!m->finished) return fail(m->h, KMR_ERR_STATE, "kmr_match_device_ptrs before kmr_match_finish");
	if (dev_offsets) *dev_offsets = m->offsets.get();
	if (dev_read_ids) *dev_read_ids = m->read_ids.get();
	if (dev_size_before_sampling) *dev_size_before_sampling = m->size_before.get();
	if (dev_size_after_sampling) *dev_size_after_sampling = m->size_after.get();
	return KMR_OK;
}
void kmr_match_free(kmr_match *m) { free_on_device(m); }

/* ---- ContigExtender (src/ContigExtender.h, src/KmerSpectrum.h:2311-2373; kernels: kmr_extend.hpp, launched by kmr_api.hip's extend_core) ---- */
int kmr_extend_config_init(kmr_extend_config *c) {
	if (!c) return KMR_ERR_INVALID_ARG;
	memset(c, 0, sizeof(*c));
	c->struct_size = (uint32_t)sizeof(kmr_extend_config);
	c->max_extend = 50;                    /* extendContigs' maxExtend, ContigExtender.h:152 */
	c->minimum_consensus = 85;             /* _ContigExtenderBaseOptions, ContigExtender.h:63 */
	c->minimum_coverage = 4.8;
	c->maximum_delta_ratio = 0.33;
	c->use_weights = 1;
	return KMR_OK;
}
static int extend_any(kmr_handle *h, const kmr_reads *contigs, const kmr_reads *reads, const uint64_t *pool_offsets, const uint64_t *pool_reads, const uint8_t *active, bool on_device,
                      const kmr_extend_config *cfg, kmr_extend **out) {
	if (out) *out = nullptr;
	if (!h || !contigs || !reads || !cfg || !out || !pool_offsets) return fail(h, KMR_ERR_INVALID_ARG, "kmr_extend_contigs: NULL argument");
	if (cfg->struct_size != sizeof(kmr_extend_config)) return fail(h, KMR_ERR_INVALID_ARG, "kmr_extend_config: struct_size " + std::to_string(cfg->struct_size) + " is not " + std::to_string(sizeof(kmr_extend_config)));
	if (contigs->device != h->device || reads->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "kmr_extend_contigs: the contigs or the reads live on another device");
	if (cfg->max_extend > KMR_EXTEND_MAX_EXTEND) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_extend_contigs: max_extend above " + std::to_string(KMR_EXTEND_MAX_EXTEND));
	if (cfg->minimum_consensus != cfg->minimum_consensus || cfg->minimum_coverage != cfg->minimum_coverage || cfg->maximum_delta_ratio != cfg->maximum_delta_ratio)
		return fail(h, KMR_ERR_INVALID_ARG, "kmr_extend_config: a NaN option");
	if (contigs->n >= 0x7fffffffull) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_extend_contigs: 2^31 - 1 contigs or more");
	hipSetDevice(h->device);
	Scratch tmp(h);
	const uint64_t nc = contigs->n;
	const uint64_t *dpo, *dpr; const uint8_t *dact;
	uint64_t P = 0;
	if (!on_device) {      /* the host sees the offsets: what the device would refuse is refused before anything is copied */
		if (pool_offsets[0] != 0) return fail(h, KMR_ERR_INVALID_ARG, "kmr_extend_contigs: pool_offsets does not start at 0 or does not ascend");
		for (uint64_t c = 0; c < nc; c++) if (pool_offsets[c + 1] < pool_offsets[c]) return fail(h, KMR_ERR_INVALID_ARG, "kmr_extend_contigs: pool_offsets does not start at 0 or does not ascend");
		P = pool_offsets[nc];
		if (P && !pool_reads) return fail(h, KMR_ERR_INVALID_ARG, "kmr_extend_contigs: NULL argument");
	}
	int rc = to_device(h, tmp, pool_offsets, nc + 1, &dpo, on_device); if (rc) return rc;
	rc = to_device(h, tmp, pool_reads, P, &dpr, on_device); if (rc) return rc;
	rc = to_device(h, tmp, active, nc, &dact, on_device); if (rc) return rc;
	auto e = make_result<kmr_extend>(h);
	rc = extend_core(h, contigs, reads, dpo, dpr, dact, cfg, e.get()); if (rc) return rc;      /* (waits for the stream) */
	tmp.done();
	*out = e.release();
	return KMR_OK;
}
int kmr_extend_contigs(kmr_handle *h, const kmr_reads *contigs, const kmr_reads *reads, const uint64_t *pool_offsets, const uint64_t *pool_reads, const uint8_t *active,
                       const kmr_extend_config *cfg, kmr_extend **out) {
	return extend_any(h, contigs, reads, pool_offsets, pool_reads, active, false, cfg, out);
}
int kmr_extend_contigs_dev(kmr_handle *h, const kmr_reads *contigs, const kmr_reads *reads, const void *dev_pool_offsets, const void *dev_pool_reads, const void *dev_active,
                           const kmr_extend_config *cfg, kmr_extend **out) {
	return extend_any(h, contigs, reads, (const uint64_t *)dev_pool_offsets, (const uint64_t *)dev_pool_reads, (const uint8_t *)dev_active, true, cfg, out);
}
int kmr_extend_info(const kmr_extend *e, uint64_t *n_contigs, uint64_t *n_extended, uint64_t *bases_added) {
	if (!e) return KMR_ERR_INVALID_ARG;
	if (n_contigs) *n_contigs = e->n;
	if (n_extended) *n_extended = e->n_extended;
	if (bases_added) *bases_added = e->bases_added;
	return KMR_OK;
}
int kmr_extend_copy(const kmr_extend *e, uint32_t *new_len, uint32_t *left, uint32_t *right, kmr_extend_stop *stops) {
	if (!e) return KMR_ERR_INVALID_ARG;
	hipSetDevice(e->device);
	hipError_t err = hipSuccess;
	copy_out(err, new_len, e->newlen, e->n); copy_out(err, left, e->left, e->n); copy_out(err, right, e->right, e->n);
	if (stops && e->n) {
		std::vector<uint32_t> reason(2 * e->n); std::vector<double> vals(2 * e->n * EXT_VALS);
		copy_out(err, reason.data(), e->reason, 2 * e->n); copy_out(err, vals.data(), e->vals, 2 * e->n * EXT_VALS);
		for (uint64_t i = 0; i < 2 * e->n && err == hipSuccess; i++) {
			kmr_extend_stop &s = stops[i];
			const double *v = &vals[i * EXT_VALS];
			s.reason = reason[i]; s.reserved = 0; s.edge = v[0]; s.ext[0] = v[1]; s.ext[1] = v[2]; s.ext[2] = v[3]; s.ext[3] = v[4]; s.total = v[5];
		}
	}
	return err == hipSuccess ? KMR_OK : KMR_ERR_HIP;
}
int kmr_extend_reads(const kmr_extend *e, const kmr_reads **reads) {
	if (!e || !reads) return KMR_ERR_INVALID_ARG;
	*reads = e->result;
	return KMR_OK;
}
void kmr_extend_free(kmr_extend *e) { free_on_device(e); }
/* ContigExtender::getNewName (ContigExtender.h:249-268) */
int kmr_extend_new_name(const char *old_name, uint64_t left, uint64_t right, char *buf, uint64_t cap) {
	if (!old_name || !buf) return KMR_ERR_INVALID_ARG;
	const std::string oldName(old_name);
	std::string newName = oldName;
	if (left + right != 0) {
		std::string::size_type preLeft = 0, preRight = 0;
		const std::string::size_type pos = oldName.find_last_of("-l");      /* the last '-' or 'l' */
		if (pos != std::string::npos) {
			const std::string::size_type pos2 = oldName.find_first_of("r", pos);
			if (pos2 != std::string::npos) {
				preLeft = (std::string::size_type)atoi(oldName.substr(pos + 1, pos2 - pos - 1).c_str());
				preRight = (std::string::size_type)atoi(oldName.substr(pos2 + 1).c_str());
				newName = oldName.substr(0, pos - 1);      /* (pos == 0: npos characters, the whole name) */
			}
		}
		newName = newName + "-l" + std::to_string(left + preLeft) + "r" + std::to_string(right + preRight);
	}
	if (newName.size() + 1 > cap) return KMR_ERR_CAPACITY;
	memcpy(buf, newName.c_str(), newName.size() + 1);
	return KMR_OK;
}
/* ContigExtender::getMinMaxKmerSize (ContigExtender.h:269-279), SequenceLengthType being 32 bits wide */
int kmr_extend_min_max_kmer_size(uint32_t kmer_size, uint32_t max_sequence_length, uint64_t base_count, uint64_t n_reads, uint32_t max_steps,
                                 uint32_t *min_kmer_size, uint32_t *max_kmer_size, uint32_t *kmer_step) {
	if (!n_reads || !max_steps || !min_kmer_size || !max_kmer_size || !kmer_step) return KMR_ERR_INVALID_ARG;
	const uint32_t minK = kmer_size;
	const uint32_t maxLen = std::min<uint32_t>(max_sequence_length, (uint32_t)(base_count / n_reads));
	uint32_t maxK = std::min<uint32_t>((uint32_t)(maxLen * 0.95), maxLen - 1u);
	maxK = std::max(minK, maxK);
	uint32_t step = (maxK - minK) / max_steps;
	step = (step & 1u) == 1u ? step + 1u : step;
	step = std::max<uint32_t>(2u, step);
	*min_kmer_size = minK; *max_kmer_size = maxK; *kmer_step = step;
	return KMR_OK;
}

}  // extern "C"

/* ---- TnfDistance (apps/TnfDistance.cpp; kernels: kmr_tnf.hpp; the k-mers come out of kmr_api.hip's tnf_stage_core) ---- */
namespace {

uint32_t tnf_dims(uint32_t k) { const uint32_t all = 1u << (2 * k); return (k & 1) ? all / 2 : (all + (1u << k)) / 2; }
uint32_t tnf_revcomp(uint32_t code, uint32_t k) { uint32_t r = 0; for (uint32_t i = 0; i < k; i++) { r = (r << 2) | (3u - (code & 3u)); code >>= 2; } return r; }

/* column -> code, in the iteration order of TNF::stdMap: bucket = hash & 4095, ascending key within a bucket */
std::vector<uint16_t> tnf_columns(uint32_t k, uint32_t hash_kind) {
	std::vector<std::pair<uint32_t, uint32_t> > e;
	const uint32_t kb = (k + 3) / 4;
	for (uint32_t code = 0; code < (1u << (2 * k)); code++) {
		if (code > tnf_revcomp(code, k)) continue;
		const uint32_t w16 = code << (16 - 2 * k);      /* left-justified, pad bits zero (TwoBitSequence) */
		const uint8_t key[2] = {(uint8_t)(w16 >> 8), (uint8_t)w16};
		e.push_back(std::make_pair((uint32_t)(kmr_hash_of_kind(key, kb, hash_kind) & 4095u), code));
	}
	std::sort(e.begin(), e.end());
	std::vector<uint16_t> codes;
	for (const auto &p : e) codes.push_back((uint16_t)p.second);
	return codes;
}

int tnf_check_k(kmr_handle *h, const char *who) {
	if (h->k > TNF_MAX_K) return fail(h, KMR_ERR_UNSUPPORTED, std::string(who) + ": k = " + std::to_string(h->k) + " (TnfDistance is built for k <= 6)");
	return KMR_OK;
}

/* the group bounds of a call as a checked host vector */
int tnf_starts(kmr_handle *h, const char *who, const uint64_t *input_starts, uint32_t n_inputs, uint64_t n, std::vector<uint64_t> &starts) {
	if (!input_starts) {
		if (n_inputs > 1) return fail(h, KMR_ERR_INVALID_ARG, std::string(who) + ": input_starts is NULL for " + std::to_string(n_inputs) + " inputs");
		starts = {0, n};
		return KMR_OK;
	}
	if (n_inputs == 0) return fail(h, KMR_ERR_INVALID_ARG, std::string(who) + ": input_starts without n_inputs");
	if (n_inputs > 65535) return fail(h, KMR_ERR_UNSUPPORTED, std::string(who) + ": more than 65535 inputs");
	bool ok = false;
	const uint32_t at = sel_check_input_starts(input_starts, n_inputs, &ok);
	if (!ok) return fail(h, KMR_ERR_INVALID_ARG, std::string(who) + ": input_starts[" + std::to_string(at) + "]: the sequence indices start at 0 and ascend");
	if (input_starts[n_inputs] != n) return fail(h, KMR_ERR_INVALID_ARG, std::string(who) + ": input_starts ends at " + std::to_string(input_starts[n_inputs]) + ", the batch holds " + std::to_string(n) + " sequences");
	starts.assign(input_starts, input_starts + n_inputs + 1);
	return KMR_OK;
}

/* lengths, the inexact columns and the group of every vector: what every kmr_tnf has from the start.  The root is taken on the host:
 * the radicand is a sum of n doubles per set, and the host's sqrt is the correctly rounded one the reference calls */
template <class T> int tnf_finish_t(kmr_handle *h, kmr_tnf *t) {
	Scratch tmp(h);
	double *l2; unsigned long long *bad;
	HIPCHK(h, tmp.take(&l2, t->n)); HIPCHK(h, tmp.take(&bad, (size_t)1));
	HIPCHK(h, hipMemsetAsync(bad, 0, 8, h->stream));
	LAUNCH(h, tnf_len2_kernel<T>, dim3(grid_for(t->n, 64)), dim3(64), 0, t->counts.get<T>(), t->n, t->D, l2, bad);
	std::vector<double> hl(t->n); unsigned long long hbad = 0;
	HIPCHK(h, fetch_queue(h, hl.data(), l2, t->n));
	HIPCHK(h, fetch_queue(h, &hbad, bad));
	HIPCHK(h, stream_wait(h));
	tmp.done();
	t->inexact = hbad;
	std::vector<float> len(t->n);
	for (uint64_t v = 0; v < t->n; v++) { float f = (float)std::sqrt(hl[v]); if (f == 0.0f) f = 1.0f; len[v] = f; }
	std::vector<uint32_t> grp(t->n);
	for (size_t g = 0; g + 1 < t->bounds.size(); g++) for (uint64_t v = t->bounds[g]; v < t->bounds[g + 1]; v++) grp[v] = (uint32_t)g;
	HIPCHK(h, t->len.alloc(4 * t->n)); HIPCHK(h, t->group.alloc(4 * t->n));
	HIPCHK(h, hipMemcpy(t->len.get(), len.data(), 4 * t->n, hipMemcpyHostToDevice));
	HIPCHK(h, hipMemcpy(t->group.get(), grp.data(), 4 * t->n, hipMemcpyHostToDevice));
	return KMR_OK;
}
int tnf_finish(kmr_handle *h, kmr_tnf *t) {
	if (t->n == 0) return KMR_OK;
	return t->wide ? tnf_finish_t<unsigned long long>(h, t) : tnf_finish_t<uint32_t>(h, t);
}

/* the vectors of a batch: one per sequence, or (windows) one per surviving window */
int tnf_count(kmr_handle *h, const char *who, const kmr_reads *r, const std::vector<uint64_t> &starts, bool windows, uint64_t window, uint64_t step, int64_t min_count, kmr_tnf *t) {
	const uint64_t n = r->n;
	const uint32_t k = h->k, D = tnf_dims(k), n_groups = (uint32_t)starts.size() - 1;
	t->k = k; t->D = D; t->hash_kind = h->cfg.hash_kind; t->wide = false; t->n = 0;
	t->bounds.assign(n_groups + 1, 0);
	if (n == 0) return KMR_OK;
	Scratch tmp(h);
	const dim3 block(256);
	/* windows carry reference quality (Kmernator::PRINT_REF_QUAL, :491) */
	const uint8_t *quals = r->quals.get<uint8_t>();
	if (windows) {
		uint8_t *q; HIPCHK(h, tmp.take(&q, r->total + 64));
		HIPCHK(h, hipMemsetAsync(q, 127, r->total + 64, h->stream));
		quals = q;
	}
	const uint64_t *offsets = r->offsets.get<uint64_t>(), *koff = nullptr, *stage = nullptr; uint64_t slots = 0;
	int rc = tnf_stage_core(h, r->bases.get<uint8_t>(), quals, offsets, n, &koff, &stage, &slots); if (rc) return rc;
	/* the vectors: their slots and origins */
	uint64_t nv = n; uint64_t *woff = nullptr;
	if (windows) {
		uint32_t *nwin, *werr;
		HIPCHK(h, tmp.take(&nwin, n)); HIPCHK(h, tmp.take(&werr, (size_t)1)); HIPCHK(h, tmp.take(&woff, n + 1));
		HIPCHK(h, hipMemsetAsync(werr, 0, 4, h->stream));
		LAUNCH(h, tnf_win_count_kernel, dim3(grid_for(n)), block, 0, offsets, n, window, step, nwin, werr);
		rc = exclusive_scan_queue(h, nwin, n, woff); if (rc) return rc;
		uint32_t herr = 0;
		HIPCHK(h, fetch_queue(h, &nv, woff + n));
		HIPCHK(h, fetch_queue(h, &herr, werr));
		HIPCHK(h, stream_wait(h));
		if (herr) return fail(h, KMR_ERR_UNSUPPORTED, std::string(who) + ": a sequence of 2^32 windows or more");
		if (nv == 0) { tmp.done(); return KMR_OK; }
	}
	DevBuf counts, origin;
	uint64_t *vslot, *poff; uint32_t *vnk, *pcnt;
	HIPCHK(h, tmp.take(&vslot, nv)); HIPCHK(h, tmp.take(&vnk, nv)); HIPCHK(h, tmp.take(&pcnt, nv)); HIPCHK(h, tmp.take(&poff, nv + 1));
	HIPCHK(h, counts.alloc(std::max<size_t>(4 * nv * D, 256))); HIPCHK(h, origin.alloc(24 * nv));
	HIPCHK(h, hipMemsetAsync(counts.get(), 0, 4 * nv * D, h->stream));
	if (windows) LAUNCH(h, tnf_win_desc_kernel, dim3(grid_for(nv)), block, 0, koff, (const uint64_t *)woff, n, nv, window, step, k, vslot, vnk, origin.get<uint64_t>());
	else LAUNCH(h, tnf_reads_desc_kernel, dim3(grid_for(nv)), block, 0, offsets, koff, n, vslot, vnk, origin.get<uint64_t>());
	uint32_t piece = h->tune.tnf_piece_bases ? h->tune.tnf_piece_bases : TNF_PIECE_BASES;
	piece = piece > k - 1 ? piece - (k - 1) : 1;      /* pieces of bases overlap by k - 1: as many k-mers begin in one */
	LAUNCH(h, tnf_piece_count_kernel, dim3(grid_for(nv)), block, 0, (const uint32_t *)vnk, nv, piece, pcnt);
	rc = exclusive_scan_queue(h, pcnt, nv, poff); if (rc) return rc;
	uint64_t n_pieces = 0;
	HIPCHK(h, fetch(h, &n_pieces, poff + nv));
	if (n_pieces && slots) {
		const std::vector<uint16_t> codes = tnf_columns(k, h->cfg.hash_kind);
		std::vector<uint16_t> col(1u << (2 * k), (uint16_t)TNF_NO_COLUMN);
		for (uint32_t c = 0; c < D; c++) col[codes[c]] = (uint16_t)c;
		uint16_t *dcol; HIPCHK(h, tmp.take(&dcol, col.size()));
		HIPCHK(h, hipMemcpyAsync(dcol, col.data(), 2 * col.size(), hipMemcpyHostToDevice, h->stream));
		uint64_t blocks = std::min<uint64_t>((n_pieces + TNF_WAVES - 1) / TNF_WAVES, (uint64_t)num_cus(h) * 8);
		const uint64_t per_wave = (n_pieces + blocks * TNF_WAVES - 1) / (blocks * TNF_WAVES);
		blocks = (n_pieces + per_wave * TNF_WAVES - 1) / (per_wave * TNF_WAVES);
		const size_t smem = (size_t)TNF_WAVES * 4 << (2 * k);
		HIPCHK(h, hipFuncSetAttribute((const void *)tnf_hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)TNF_WAVES * 4 << (2 * TNF_MAX_K))));
		LAUNCH(h, tnf_hist_kernel, dim3((unsigned)blocks), dim3(TNF_WAVES * 64), smem, stage, (const uint64_t *)vslot, (const uint32_t *)vnk, (const uint64_t *)poff, nv, n_pieces,
		       per_wave, piece, k, (const uint16_t *)dcol, D, counts.get<uint32_t>());
		HIPCHK(h, hipStreamSynchronize(h->stream));      /* col leaves with this scope */
	}
	if (!windows) {
		t->n = nv; t->counts = std::move(counts); t->origin = std::move(origin); t->bounds = starts;
		tmp.done();
		return KMR_OK;
	}
	/* purgeShortTNFS, the input order kept */
	unsigned long long *sums; uint32_t *keep; uint64_t *kpos, *dstarts, *dbounds;
	HIPCHK(h, tmp.take(&sums, nv)); HIPCHK(h, tmp.take(&keep, nv)); HIPCHK(h, tmp.take(&kpos, nv + 1));
	HIPCHK(h, tmp.take(&dstarts, starts.size())); HIPCHK(h, tmp.take(&dbounds, starts.size()));
	HIPCHK(h, hipMemcpyAsync(dstarts, starts.data(), 8 * starts.size(), hipMemcpyHostToDevice, h->stream));
	LAUNCH(h, tnf_rowsum_kernel, dim3(grid_for(nv * 64)), block, 0, counts.get<uint32_t>(), nv, D, sums);
	LAUNCH(h, tnf_keep_kernel, dim3(grid_for(nv)), block, 0, (const unsigned long long *)sums, nv, (long long)min_count, keep);
	rc = exclusive_scan_queue(h, keep, nv, kpos); if (rc) return rc;
	LAUNCH(h, tnf_bounds_kernel, dim3(1), block, 0, (const uint64_t *)dstarts, n_groups, (const uint64_t *)woff, (const uint64_t *)kpos, dbounds);
	std::vector<uint64_t> hb(starts.size());
	HIPCHK(h, fetch(h, hb.data(), dbounds, hb.size()));
	const uint64_t kept = hb[n_groups];
	if (kept) {
		HIPCHK(h, t->counts.alloc(std::max<size_t>(4 * kept * D, 256))); HIPCHK(h, t->origin.alloc(24 * kept));
		LAUNCH(h, tnf_compact_kernel, dim3(grid_for(nv * (D + 3))), block, 0, counts.get<uint32_t>(), origin.get<uint64_t>(), (const uint32_t *)keep, (const uint64_t *)kpos, nv, D,
		       t->counts.get<uint32_t>(), t->origin.get<uint64_t>());
		HIPCHK(h, hipStreamSynchronize(h->stream));
	}
	t->n = kept; t->bounds = hb;
	tmp.done();
	return KMR_OK;
}

int tnf_vectors(kmr_handle *h, const char *who, const kmr_reads *reads, const uint64_t *input_starts, uint32_t n_inputs, bool windows, uint64_t window, uint64_t step, int64_t min_count, kmr_tnf **out) {
	if (!h || !reads || !out) return fail(h, KMR_ERR_INVALID_ARG, std::string(who) + ": NULL argument");
	*out = nullptr;
	int rc = tnf_check_k(h, who); if (rc) return rc;
	if (reads->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "read batch lives on another device");
	if (windows && step == 0) return fail(h, KMR_ERR_INVALID_ARG, std::string(who) + ": a window step of 0");
	std::vector<uint64_t> starts;
	rc = tnf_starts(h, who, input_starts, n_inputs, reads->n, starts); if (rc) return rc;
	hipSetDevice(h->device);
	auto t = make_result<kmr_tnf>(h);
	rc = tnf_count(h, who, reads, starts, windows, window, step, min_count, t.get()); if (rc) return rc;
	rc = tnf_finish(h, t.get()); if (rc) return rc;
	*out = t.release();
	return KMR_OK;
}

int tnf_group_sums(kmr_handle *h, const kmr_tnf *in, kmr_tnf *t) {
	const uint32_t G = (uint32_t)in->bounds.size() - 1, D = in->D;
	t->k = in->k; t->D = D; t->hash_kind = in->hash_kind; t->wide = true; t->n = G;
	t->bounds.resize(G + 1);
	for (uint32_t g = 0; g <= G; g++) t->bounds[g] = g;
	if (G == 0) return KMR_OK;
	HIPCHK(h, t->counts.alloc(std::max<size_t>(8ull * G * D, 256))); HIPCHK(h, t->origin.alloc(24ull * G));
	HIPCHK(h, hipMemsetAsync(t->counts.get(), 0, 8ull * G * D, h->stream));
	std::vector<uint64_t> org(3ull * G, 0); uint64_t most = 0;
	for (uint32_t g = 0; g < G; g++) { org[3 * g] = g; most = std::max(most, in->bounds[g + 1] - in->bounds[g]); }
	HIPCHK(h, hipMemcpy(t->origin.get(), org.data(), 24ull * G, hipMemcpyHostToDevice));
	if (most) {
		Scratch tmp(h);
		uint64_t *db; HIPCHK(h, tmp.take(&db, (size_t)G + 1));
		HIPCHK(h, hipMemcpyAsync(db, in->bounds.data(), 8ull * (G + 1), hipMemcpyHostToDevice, h->stream));
		LAUNCH(h, tnf_group_sum_kernel, dim3((unsigned)((most + 255) / 256), G), dim3(256), 0, in->counts.get<uint32_t>(), (const uint64_t *)db, D, t->counts.get<unsigned long long>());
		HIPCHK(h, hipStreamSynchronize(h->stream));
		tmp.done();
	}
	return KMR_OK;
}

/* the per-vector part of a formula, made once per set */
template <class T> int tnf_prepare_t(kmr_handle *h, const kmr_tnf *t, int formula) {
	const uint64_t n = t->n; const uint32_t D = t->D;
	if (formula == KMR_TNF_EUCLIDEAN) {
		if (t->qt) return KMR_OK;
		DevBuf q; HIPCHK(h, q.alloc(8 * n * D));
		LAUNCH(h, tnf_quot_kernel<T>, dim3(grid_for(n * D)), dim3(256), 0, t->counts.get<T>(), t->len.get<float>(), n, D, q.get<double>());
		HIPCHK(h, hipStreamSynchronize(h->stream));
		t->qt = std::move(q);
		return KMR_OK;
	}
	if (t->xt) return KMR_OK;
	DevBuf x, s; HIPCHK(h, x.alloc(4 * n * D)); HIPCHK(h, s.alloc(4 * n));
	LAUNCH(h, tnf_rank_kernel<T>, dim3((unsigned)std::min<uint64_t>(n, (uint64_t)num_cus(h) * 16)), dim3(256), 4 * D, t->counts.get<T>(), n, D, x.get<float>());
	LAUNCH(h, tnf_x2_kernel, dim3(grid_for(n, 64)), dim3(64), 0, x.get<float>(), n, D, s.get<float>());
	HIPCHK(h, hipStreamSynchronize(h->stream));
	t->xt = std::move(x); t->x2 = std::move(s);
	return KMR_OK;
}
int tnf_prepare(kmr_handle *h, const kmr_tnf *t, int formula) {
	if (t->n == 0) return KMR_OK;
	return t->wide ? tnf_prepare_t<unsigned long long>(h, t, formula) : tnf_prepare_t<uint32_t>(h, t, formula);
}

TnfSide tnf_side(const kmr_tnf *t, int formula) {
	TnfSide s;
	s.t = formula == KMR_TNF_SPEARMAN ? t->xt.get() : t->qt.get(); s.x2 = t->x2.get<float>(); s.group = t->group.get<uint32_t>(); s.n = t->n;
	return s;
}

/* rows [first_row, first_row + n_rows) of a against b (triangle: against a itself, j < i), on h's stream */
int tnf_pairs(kmr_handle *h, const kmr_tnf *a, const kmr_tnf *b, int formula, TnfPairs P) {
	if (P.n_rows == 0 || b->n == 0) return KMR_OK;
	int rc = tnf_prepare(h, a, formula); if (rc) return rc;
	rc = tnf_prepare(h, b, formula); if (rc) return rc;
	const bool hist = P.hist != nullptr, sp = formula == KMR_TNF_SPEARMAN;
	const uint64_t tiles = ((P.n_rows + TNF_TILE - 1) / TNF_TILE) * ((b->n + TNF_TILE - 1) / TNF_TILE);
	/* blocks walk the tiles; with HIST a block's u32 counters in LDS must hold its pairs: fewer than 2^19 tiles of 4096 a block */
	const uint64_t blocks = std::max<uint64_t>(std::min<uint64_t>(tiles, (uint64_t)num_cus(h) * 32), (tiles + (1u << 19) - 1) >> 19);
	if (blocks > 0x7fffffffull) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_tnf: too many pairs for one call (take fewer rows)");
	const size_t smem = (size_t)2 * TNF_SLICE * TNF_TILE * (sp ? 4 : 8) + (hist ? (size_t)8 * (P.bins + 2) : 0);
	const void *kern = sp ? (hist ? (const void *)tnf_pairs_kernel<true, true> : (const void *)tnf_pairs_kernel<true, false>)
	                      : (hist ? (const void *)tnf_pairs_kernel<false, true> : (const void *)tnf_pairs_kernel<false, false>);
	HIPCHK(h, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
	const TnfSide sa = tnf_side(a, formula), sb = tnf_side(b, formula);
	const dim3 grid((unsigned)blocks), block(TNF_BLOCK);
	if (sp) { if (hist) LAUNCH(h, (tnf_pairs_kernel<true, true>), grid, block, smem, sa, sb, P); else LAUNCH(h, (tnf_pairs_kernel<true, false>), grid, block, smem, sa, sb, P); }
	else { if (hist) LAUNCH(h, (tnf_pairs_kernel<false, true>), grid, block, smem, sa, sb, P); else LAUNCH(h, (tnf_pairs_kernel<false, false>), grid, block, smem, sa, sb, P); }
	return KMR_OK;
}

int tnf_distances_check(kmr_handle *h, const kmr_tnf *a, const kmr_tnf *b, int formula, uint64_t first_row, uint64_t n_rows, const void *out, uint64_t *floats) {
	if (!h || !a) return fail(h, KMR_ERR_INVALID_ARG, "kmr_tnf_distances: NULL argument");
	if (formula != KMR_TNF_EUCLIDEAN && formula != KMR_TNF_SPEARMAN) return fail(h, KMR_ERR_INVALID_ARG, "kmr_tnf_distances: formula is 0 (Euclidean) or 1 (Spearman)");
	if (a->device != h->device || (b && b->device != h->device)) return fail(h, KMR_ERR_INVALID_ARG, "kmr_tnf_distances: the vectors live on another device");
	if (b && (b->D != a->D || b->hash_kind != a->hash_kind)) return fail(h, KMR_ERR_INVALID_ARG, "kmr_tnf_distances: the two sets differ in k or hash_kind");
	if (first_row > a->n || n_rows > a->n - first_row) return fail(h, KMR_ERR_INVALID_ARG, "kmr_tnf_distances: rows beyond the " + std::to_string(a->n) + " vectors of a");
	const uint64_t e = first_row + n_rows;
	*floats = b ? n_rows * b->n : (e ? e * (e - 1) / 2 : 0) - (first_row ? first_row * (first_row - 1) / 2 : 0);
	if (*floats && !out) return fail(h, KMR_ERR_INVALID_ARG, "kmr_tnf_distances: NULL argument");
	return KMR_OK;
}
int tnf_distances_queue(kmr_handle *h, const kmr_tnf *a, const kmr_tnf *b, int formula, uint64_t first_row, uint64_t n_rows, float *dev_out) {
	TnfPairs P{};
	P.D = a->D; P.triangle = b ? 0 : 1; P.first_row = first_row; P.n_rows = n_rows; P.out = dev_out;
	return tnf_pairs(h, a, b ? b : a, formula, P);
}

}  // namespace

extern "C" {

int kmr_tnf_dims(uint32_t k, uint32_t *dims) {
	if (!dims) return KMR_ERR_INVALID_ARG;
	if (k < 1 || k > TNF_MAX_K) return KMR_ERR_UNSUPPORTED;
	*dims = tnf_dims(k);
	return KMR_OK;
}
int kmr_tnf_columns(uint32_t k, uint32_t hash_kind, uint16_t *codes) {
	if (!codes || hash_kind > KMR_HASH_LOOKUP8) return KMR_ERR_INVALID_ARG;
	if (k < 1 || k > TNF_MAX_K) return KMR_ERR_UNSUPPORTED;
	const std::vector<uint16_t> c = tnf_columns(k, hash_kind);
	memcpy(codes, c.data(), 2 * c.size());
	return KMR_OK;
}
int kmr_tnf_header(uint32_t k, uint32_t hash_kind, char *dst, uint64_t cap, uint64_t *bytes) {
	if (!bytes || (cap && !dst) || hash_kind > KMR_HASH_LOOKUP8) return KMR_ERR_INVALID_ARG;
	if (k < 1 || k > TNF_MAX_K) return KMR_ERR_UNSUPPORTED;
	std::string s = "Count\tLength";
	for (uint16_t code : tnf_columns(k, hash_kind)) { s.push_back('\t'); for (uint32_t i = 0; i < k; i++) s.push_back("ACGT"[(code >> (2 * (k - 1 - i))) & 3]); }
	*bytes = s.size();
	if (cap < s.size()) return KMR_ERR_CAPACITY;
	memcpy(dst, s.data(), s.size());
	return KMR_OK;
}
int kmr_tnf_reads(kmr_handle *h, const kmr_reads *reads, const uint64_t *input_starts, uint32_t n_inputs, kmr_tnf **out) {
	return tnf_vectors(h, "kmr_tnf_reads", reads, input_starts, n_inputs, false, 0, 0, 0, out);
}
int kmr_tnf_windows(kmr_handle *h, const kmr_reads *reads, const uint64_t *input_starts, uint32_t n_inputs, uint64_t window, uint64_t step, int64_t min_count, kmr_tnf **out) {
	return tnf_vectors(h, "kmr_tnf_windows", reads, input_starts, n_inputs, true, window, step, min_count, out);
}
int kmr_tnf_group_sums(kmr_handle *h, const kmr_tnf *tnf, kmr_tnf **out) {
	if (!h || !tnf || !out) return fail(h, KMR_ERR_INVALID_ARG, "kmr_tnf_group_sums: NULL argument");
	*out = nullptr;
	if (tnf->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "kmr_tnf_group_sums: the vectors live on another device");
	if (tnf->wide) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_tnf_group_sums: the vectors are group sums already");
	hipSetDevice(h->device);
	auto t = make_result<kmr_tnf>(h);
	int rc = tnf_group_sums(h, tnf, t.get()); if (rc) return rc;
	rc = tnf_finish(h, t.get()); if (rc) return rc;
	*out = t.release();
	return KMR_OK;
}
int kmr_tnf_info(const kmr_tnf *t, uint64_t *n, uint32_t *dims, uint32_t *n_groups, uint64_t *inexact) {
	if (!t) return KMR_ERR_INVALID_ARG;
	if (n) *n = t->n;
	if (dims) *dims = t->D;
	if (n_groups) *n_groups = (uint32_t)t->bounds.size() - 1;
	if (inexact) *inexact = t->inexact;
	return KMR_OK;
}
int kmr_tnf_copy(const kmr_tnf *t, uint64_t *counts, float *lengths, uint64_t *origin, uint64_t *group_bounds) {
	if (!t) return KMR_ERR_INVALID_ARG;
	hipSetDevice(t->device);
	hipError_t e = hipSuccess;
	const uint64_t cells = t->n * t->D;
	if (counts && cells && !t->wide) {
		std::vector<uint32_t> c(cells);
		e = hipMemcpy(c.data(), t->counts.get(), 4 * cells, hipMemcpyDeviceToHost);
		for (uint64_t i = 0; i < cells; i++) counts[i] = c[i];
	} else copy_out(e, counts, t->counts, cells);
	copy_out(e, lengths, t->len, t->n);
	copy_out(e, origin, t->origin, 3 * t->n);
	if (group_bounds) memcpy(group_bounds, t->bounds.data(), 8 * t->bounds.size());
	return e == hipSuccess ? KMR_OK : KMR_ERR_HIP;
}
void kmr_tnf_free(kmr_tnf *t) { free_on_device(t); }

int kmr_tnf_distances_dev(kmr_handle *h, const kmr_tnf *a, const kmr_tnf *b, int formula, uint64_t first_row, uint64_t n_rows, void *dev_out) {
	uint64_t floats = 0;
	int rc = tnf_distances_check(h, a, b, formula, first_row, n_rows, dev_out, &floats); if (rc) return rc;
	if (!floats) return KMR_OK;
	hipSetDevice(h->device);
	rc = tnf_distances_queue(h, a, b, formula, first_row, n_rows, (float *)dev_out);
	if (rc) hipStreamSynchronize(h->stream);
	return rc;
}
int kmr_tnf_distances(kmr_handle *h, const kmr_tnf *a, const kmr_tnf *b, int formula, uint64_t first_row, uint64_t n_rows, float *out) {
	uint64_t floats = 0;
	int rc = tnf_distances_check(h, a, b, formula, first_row, n_rows, out, &floats); if (rc) return rc;
	if (!floats) return KMR_OK;
	hipSetDevice(h->device);
	Scratch tmp(h);
	float *d; HIPCHK(h, tmp.take(&d, floats));
	rc = tnf_distances_queue(h, a, b, formula, first_row, n_rows, d); if (rc) return rc;
	HIPCHK(h, hipMemcpyAsync(out, d, 4 * floats, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, hipStreamSynchronize(h->stream));
	tmp.done();
	return KMR_OK;
}

int kmr_tnf_likelihood_config_init(kmr_tnf_likelihood_config *c) {
	if (!c) return KMR_ERR_INVALID_ARG;
	memset(c, 0, sizeof(*c));
	c->struct_size = sizeof(*c); c->formula = KMR_TNF_EUCLIDEAN; c->window = 10000; c->step = 1000; c->window2 = 10000; c->step2 = 1000; c->bins = 100; c->max_samples = INT64_MAX;
	return KMR_OK;
}
int kmr_tnf_likelihoods(kmr_handle *h, const kmr_reads *reads, const uint64_t *input_starts, uint32_t n_inputs, const kmr_tnf_likelihood_config *cfg, uint64_t *out) {
	const char *who = "kmr_tnf_likelihoods";
	if (!h || !reads || !cfg || !out) return fail(h, KMR_ERR_INVALID_ARG, std::string(who) + ": NULL argument");
	if (cfg->struct_size != sizeof(*cfg)) return fail(h, KMR_ERR_INVALID_ARG, std::string(who) + ": kmr_tnf_likelihood_config.struct_size mismatch (ABI)");
	if (cfg->formula > KMR_TNF_SPEARMAN) return fail(h, KMR_ERR_INVALID_ARG, std::string(who) + ": formula is 0 (Euclidean) or 1 (Spearman)");
	if (cfg->bins < 1 || cfg->bins > TNF_MAX_BINS) return fail(h, KMR_ERR_INVALID_ARG, std::string(who) + ": 1 <= bins <= 4094");
	if (cfg->step == 0) return fail(h, KMR_ERR_INVALID_ARG, std::string(who) + ": a window step of 0");
	int rc = tnf_check_k(h, who); if (rc) return rc;
	if (reads->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "read batch lives on another device");
	std::vector<uint64_t> starts;
	rc = tnf_starts(h, who, input_starts, n_inputs, reads->n, starts); if (rc) return rc;
	const uint64_t window = cfg->window;
	uint64_t window2 = cfg->window2, step2 = cfg->step2;
	if (window2 < window) { window2 = window; step2 = cfg->step; }      /* _parseOptions :198-203 */
	if (step2 == 0) return fail(h, KMR_ERR_INVALID_ARG, std::string(who) + ": a window2 step of 0");
	const bool equal = window == window2;
	const uint32_t G = (uint32_t)starts.size() - 1, nbin = cfg->bins + 2;
	hipSetDevice(h->device);
	auto R = make_result<kmr_tnf>(h), W1 = make_result<kmr_tnf>(h), W2 = make_result<kmr_tnf>(h), whole = make_result<kmr_tnf>(h);
	rc = tnf_count(h, who, reads, starts, true, window, cfg->step, (int64_t)(window * 3 / 4), W1.get()); if (rc) return rc;
	rc = tnf_finish(h, W1.get()); if (rc) return rc;
	if (!equal) {
		rc = tnf_count(h, who, reads, starts, true, window2, step2, (int64_t)(window2 * 3 / 4), W2.get()); if (rc) return rc;
		rc = tnf_finish(h, W2.get()); if (rc) return rc;
	}
	const kmr_tnf *w1 = W1.get(), *w2 = equal ? W1.get() : W2.get();
	/* the blocks the reference would subsample (:689-691, :750, :781, :827-832, :857) */
	auto size1 = [&](uint32_t g) { return (long long)(w1->bounds[g + 1] - w1->bounds[g]); };
	auto size2 = [&](uint32_t g) { return (long long)(w2->bounds[g + 1] - w2->bounds[g]); };
	const long long max_samples = cfg->max_samples, inputs = G;
	long long max_intra = max_samples / inputs; if (inputs > 1) max_intra += 1;
	long long max_inter = max_samples / inputs;
	if (inputs >= 2) { max_inter = max_samples / (inputs * (inputs - 1) / 2); if (inputs > 2) max_inter += 1; }
	std::vector<uint8_t> intra_ok(G, 0);
	for (uint32_t g = 0; g < G; g++) {
		if (size1(g) <= 1) continue;
		intra_ok[g] = 1;
		const long long samples = equal ? size1(g) * (size1(g) - 1) / 2 : size1(g) * size2(g);
		if (!(samples < max_intra)) return fail(h, KMR_ERR_UNSUPPORTED, std::string(who) + ": the reference would subsample the intra block of input " + std::to_string(g) + " (" + std::to_string(samples) + " pairs, max_samples allows fewer than " + std::to_string(max_intra) + "): not built");
	}
	for (uint32_t i = 0; i < G; i++) for (uint32_t j = 0; j < (equal ? i : G); j++) {
		if (i == j) continue;
		const long long samples = size1(i) * size2(j);
		if (!(samples < max_inter)) return fail(h, KMR_ERR_UNSUPPORTED, std::string(who) + ": the reference would subsample the inter block of inputs " + std::to_string(i) + " and " + std::to_string(j) + " (" + std::to_string(samples) + " pairs, max_samples allows fewer than " + std::to_string(max_inter) + "): not built");
	}
	rc = tnf_count(h, who, reads, starts, false, 0, 0, 0, R.get()); if (rc) return rc;
	rc = tnf_group_sums(h, R.get(), whole.get()); if (rc) return rc;
	rc = tnf_finish(h, whole.get()); if (rc) return rc;
	Scratch tmp(h);
	unsigned long long *dh; uint8_t *dok;
	HIPCHK(h, tmp.take(&dh, (size_t)4 * nbin)); HIPCHK(h, tmp.take(&dok, (size_t)G));
	HIPCHK(h, hipMemsetAsync(dh, 0, 8ull * 4 * nbin, h->stream));
	HIPCHK(h, hipMemcpyAsync(dok, intra_ok.data(), G, hipMemcpyHostToDevice, h->stream));
	TnfPairs P{};
	P.D = w1->D; P.first_row = 0; P.n_rows = w1->n; P.out = nullptr; P.intra_ok = dok; P.bins = cfg->bins;
	P.end = cfg->formula == KMR_TNF_EUCLIDEAN ? (float)std::sqrt(2.0) : 1.0f;
	P.step = (P.end - 0.0f) / (float)(int)cfg->bins;
	P.triangle = equal ? 1 : 0; P.hist = dh;
	rc = tnf_pairs(h, w1, w2, (int)cfg->formula, P); if (rc) return rc;
	P.triangle = 0; P.hist = dh + 2 * nbin;
	rc = tnf_pairs(h, w1, whole.get(), (int)cfg->formula, P); if (rc) return rc;
	HIPCHK(h, hipMemcpyAsync(out, dh, 8ull * 4 * nbin, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, hipStreamSynchronize(h->stream));
	tmp.done();
	return KMR_OK;
}

/* ---- f4: artifact filter (FilterKnownOddities) --------------------------- */
}  // extern "C"

struct kmr_artifact_filter : OnDevice {
	kmr_artifact_config cfg;
	uint32_t n_seq = 0, remaining_edits = 0, log2cap = 0;
	uint64_t n_keys = 0;
	DevBuf d_keys, d_vals;                                         /* open-addressed lookup table */
	DevBuf d_bits;                                                 /* presence filter in front of it (ART_FILTER_LOG2 bits) */
	std::vector<uint64_t> keys; std::vector<uint32_t> vals;        /* the same entries on the host, ascending keys */
	/* getFilterName (:543-550) of every index: [0] empty, [1, n_seq) the FASTA headers up to the first blank or tab, [n_seq]
	 * "MinQualityTrim<min_quality>"; on the device each with its leading blank (Read::LABEL_SEP; none for an empty name) as
	 * d_label_bytes behind the n_seq + 2 offsets of d_label_off (kmr_artifact_report.hpp) */
	std::vector<std::string> names;
	DevBuf d_label_bytes, d_label_off;
};

namespace {

uint32_t art_log2cap(uint64_t n) { uint32_t l = 10; while ((1ull << l) < 2 * n + 16) l++; return l; }

uint64_t art_pack(const char *s, uint32_t len) {      /* TwoBitSequence::compressSequence: anything but ACGT packs as A */
	uint64_t v = 0;
	for (uint32_t i = 0; i < len; i++) { const char c = s[i]; v = (v << 2) | (uint64_t)((c == 'C') ? 1 : (c == 'G') ? 2 : (c == 'T') ? 3 : 0); }
	return v;
}
uint64_t art_revcomp_host(uint64_t v, uint32_t len) { uint64_t r = 0; for (uint32_t i = 0; i < len; i++) { r = (r << 2) | (3 - (v & 3)); v >>= 2; } return r; }

/* (re)build the lookup table of the filter from its host entries */
int art_upload(kmr_handle *h, kmr_artifact_filter *f) {
	f->d_keys.reset(); f->d_vals.reset();
	f->n_keys = f->keys.size();
	f->log2cap = art_log2cap(f->n_keys);
	const uint64_t cap = 1ull << f->log2cap;
	HIPCHK(h, f->d_keys.alloc(8 * cap)); HIPCHK(h, f->d_vals.alloc(4 * cap));
	if (!f->d_bits) HIPCHK(h, f->d_bits.alloc((1u << ART_FILTER_LOG2) / 8));
	HIPCHK(h, hipMemsetAsync(f->d_bits.get<uint32_t>(), 0, (1u << ART_FILTER_LOG2) / 8, h->stream));
	Scratch tmp(h); uint64_t *dk; uint32_t *dv;
	HIPCHK(h, tmp.take(&dk, f->n_keys)); HIPCHK(h, tmp.take(&dv, f->n_keys));
	if (f->n_keys) { HIPCHK(h, hipMemcpyAsync(dk, f->keys.data(), 8 * f->n_keys, hipMemcpyHostToDevice, h->stream)); HIPCHK(h, hipMemcpyAsync(dv, f->vals.data(), 4 * f->n_keys, hipMemcpyHostToDevice, h->stream)); }
	ArtifactTable t{f->d_keys.get<uint64_t>(), f->d_vals.get<uint32_t>(), nullptr, f->log2cap, f->d_bits.get<uint32_t>()};
	LAUNCH(h, artifact_fill, dim3(1024), dim3(256), 0, f->d_keys.get<uint64_t>(), (uint32_t *)nullptr, cap);
	if (f->n_keys) LAUNCH(h, artifact_insert, dim3((unsigned)std::min<uint64_t>((f->n_keys + 255) / 256, 4096)), dim3(256), 0, t, dk, dv, f->n_keys);
	HIPCHK(h, hipStreamSynchronize(h->stream));
	tmp.done();
	return KMR_OK;
}

/* the label table of the report's writer */
int art_upload_names(kmr_handle *h, kmr_artifact_filter *f) {
	std::vector<uint64_t> off(1, 0); std::string bytes;
	for (const std::string &nm : f->names) { if (!nm.empty()) { bytes.push_back(' '); bytes += nm; } off.push_back(bytes.size()); }
	HIPCHK(h, f->d_label_off.alloc(8 * off.size())); HIPCHK(h, f->d_label_bytes.alloc(std::max<size_t>(bytes.size(), 256)));
	HIPCHK(h, hipMemcpy(f->d_label_off.get<uint64_t>(), off.data(), 8 * off.size(), hipMemcpyHostToDevice));
	if (!bytes.empty()) HIPCHK(h, hipMemcpy(f->d_label_bytes.get<uint8_t>(), bytes.data(), bytes.size(), hipMemcpyHostToDevice));
	return KMR_OK;
}

/* one round of prepareMaps' edit loop (src/FilterKnownOddities.h:264-282) on the device */
int art_build_round(kmr_handle *h, kmr_artifact_filter *f) {
	const uint32_t L = f->cfg.match_length, kb = L / 4;
	const uint64_t n = f->keys.size();
	/* the map's iteration order: bucket by bucket (KmerMap(512*1024): 512*1024/32+1 buckets rounded up to 2^15), sorted inside */
	const uint64_t mask = resize_buckets(512 * 1024 / 32 + 1) - 1;
	std::vector<std::pair<uint64_t, uint64_t>> order(n);
	for (uint64_t i = 0; i < n; i++) {
		uint8_t b[8];
		for (uint32_t j = 0; j < kb; j++) b[j] = (uint8_t)(f->keys[i] >> (8 * (kb - 1 - j)));
		order[i] = std::make_pair(kmr_hash(b, kb) & mask, i);
	}
	std::sort(order.begin(), order.end());       /* ties inside a bucket: ascending index = ascending key */
	std::vector<uint64_t> sk(n); std::vector<uint32_t> sv(n);
	for (uint64_t i = 0; i < n; i++) { sk[i] = f->keys[order[i].second]; sv[i] = f->vals[order[i].second]; }
	const uint64_t worst = n * (3ull * L + 1);
	if (worst > (1ull << 32)) return fail(h, KMR_ERR_UNSUPPORTED, "artifact filter: an edit round over " + std::to_string(n) + " keys does not fit the build table");
	const uint32_t log2cap = art_log2cap(worst);
	const uint64_t cap = 1ull << log2cap;
	Scratch tmp(h); uint64_t *tk, *dk, *ok; uint32_t *tv, *tr, *dv, *ov; unsigned long long *cnt;
	HIPCHK(h, tmp.take(&tk, cap)); HIPCHK(h, tmp.take(&tv, cap)); HIPCHK(h, tmp.take(&tr, cap));
	HIPCHK(h, tmp.take(&dk, n)); HIPCHK(h, tmp.take(&dv, n)); HIPCHK(h, tmp.take(&cnt, 1));
	HIPCHK(h, hipMemcpyAsync(dk, sk.data(), 8 * n, hipMemcpyHostToDevice, h->stream));
	HIPCHK(h, hipMemcpyAsync(dv, sv.data(), 4 * n, hipMemcpyHostToDevice, h->stream));
	HIPCHK(h, hipMemsetAsync(cnt, 0, 8, h->stream));
	ArtifactTable t{tk, tv, tr, log2cap, nullptr};
	LAUNCH(h, artifact_fill, dim3(2048), dim3(256), 0, tk, tr, cap);
	LAUNCH(h, artifact_insert, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, t, dk, dv, n);
	LAUNCH(h, artifact_neighbours, dim3((unsigned)std::min<uint64_t>((n * L + 255) / 256, 1u << 20)), dim3(256), 0, t, dk, n, L);
	HIPCHK(h, hipStreamSynchronize(h->stream));
	/* the table is sparse (<= 50 % by construction, a few % in practice): count first, then compact */
	HIPCHK(h, tmp.take(&ok, worst)); HIPCHK(h, tmp.take(&ov, worst));
	LAUNCH(h, artifact_compact, dim3(2048), dim3(256), 0, t, dv, ok, ov, cnt);
	unsigned long long m = 0;
	HIPCHK(h, fetch(h, &m, cnt));
	std::vector<uint64_t> nk(m); std::vector<uint32_t> nv(m);
	HIPCHK(h, hipMemcpy(nk.data(), ok, 8 * m, hipMemcpyDeviceToHost)); HIPCHK(h, hipMemcpy(nv.data(), ov, 4 * m, hipMemcpyDeviceToHost));
	tmp.done();
	std::vector<uint64_t> idx(m);
	for (uint64_t i = 0; i < m; i++) idx[i] = i;
	std::sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) { return nk[a] < nk[b]; });
	f->keys.resize(m); f->vals.resize(m);
	for (uint64_t i = 0; i < m; i++) { f->keys[i] = nk[idx[i]]; f->vals[i] = nv[idx[i]]; }
	return KMR_OK;
}

}  // namespace

extern "C" {

void kmr_artifact_config_init(kmr_artifact_config *c) {
	if (!c) return;
	memset(c, 0, sizeof(*c));
	c->match_length = 24; c->edit_distance = 2; c->build_edits = 2;      /* _FilterKnownOdditiesOptions(), src/FilterKnownOddities.h:72-75 */
	c->min_quality = 3; c->fastq_start_char = 33; c->min_read_length = 0.40f;
}

int kmr_artifact_filter_create(kmr_handle *h, const kmr_artifact_config *cfg, const char *fasta, uint64_t len, kmr_artifact_filter **out) {
	if (!h || !cfg || !out || (len && !fasta)) return KMR_ERR_INVALID_ARG;
	*out = nullptr;
	if (cfg->match_length == 0 || cfg->match_length > 28 || (cfg->match_length & 3))
		return fail(h, KMR_ERR_INVALID_ARG, "artifact match length must be a multiple of 4 and <= 28 (src/FilterKnownOddities.h:207-209,244)");
	hipSetDevice(h->device);
	auto f = make_result<kmr_artifact_filter>(h);
	f->cfg = *cfg;
	const uint32_t L = cfg->match_length;
	/* sequences: read 0 is the empty "no match" read, then the FASTA records in file order (:213-231) */
	std::vector<std::string> seqs(1);
	f->names.assign(1, std::string());
	for (uint64_t i = 0; i < len;) {
		uint64_t e = i; while (e < len && fasta[e] != '\n') e++;
		uint64_t le = e; if (le > i && fasta[le - 1] == '\r') le--;
		if (le > i) {
			if (fasta[i] == '>') {
				seqs.push_back(std::string());
				uint64_t ne = i + 1; while (ne < le && fasta[ne] != ' ' && fasta[ne] != '\t') ne++;
				f->names.push_back(std::string(fasta + i + 1, fasta + ne));
			}
			else if (seqs.size() > 1) for (uint64_t j = i; j < le; j++) seqs.back().push_back((char)toupper((unsigned char)fasta[j]));
		}
		i = e + 1;
	}
	f->n_seq = (uint32_t)seqs.size();
	std::vector<std::pair<uint64_t, uint32_t>> kv;
	for (uint32_t s = 1; s < f->n_seq; s++) {
		std::string q = seqs[s];
		if (cfg->reference_begin == 0 || s < cfg->reference_begin) q += seqs[s].substr(0, L);      /* ReadSet::circularize, src/ReadSet.cpp:120-130 */
		for (size_t j = 0; j + L <= q.size(); j++) {
			const uint64_t v = art_pack(q.data() + j, L), r = art_revcomp_host(v, L);
			kv.push_back(std::make_pair(r < v ? r : v, s));
		}
	}
	std::sort(kv.begin(), kv.end());                  /* getOrSetElement in sequence order: the lowest sequence index keeps a key */
	for (size_t i = 0; i < kv.size(); i++) if (i == 0 || kv[i].first != kv[i - 1].first) { f->keys.push_back(kv[i].first); f->vals.push_back(kv[i].second); }
	int edits = (int)cfg->edit_distance;
	const int maxErrors = edits;
	for (int error = 0; error < maxErrors; error++) {
		if (cfg->build_edits == 1 || (cfg->build_edits == 2 && f->keys.size() < 750000)) {
			edits--;
			if (!f->keys.empty()) { const int rc = art_build_round(h, f.get()); if (rc) return rc; }
		}
	}
	if (edits > 2) return fail(h, KMR_ERR_UNSUPPORTED, "artifact filter: more than two edits left for query time");
	f->remaining_edits = (uint32_t)edits;
	int rc = art_upload(h, f.get());
	if (rc) return rc;
	f->names.push_back("MinQualityTrim" + std::to_string(cfg->min_quality));
	rc = art_upload_names(h, f.get());
	if (rc) return rc;
	*out = f.release();
	return KMR_OK;
}
int kmr_artifact_filter_info(const kmr_artifact_filter *f, uint64_t *n_sequences, uint64_t *n_filter_kmers, uint32_t *remaining_edits) {
	if (!f) return KMR_ERR_INVALID_ARG;
	if (n_sequences) *n_sequences = f->n_seq; if (n_filter_kmers) *n_filter_kmers = f->n_keys; if (remaining_edits) *remaining_edits = f->remaining_edits;
	return KMR_OK;
}
int kmr_artifact_filter_entries(const kmr_artifact_filter *f, uint64_t *keys, uint32_t *values, uint64_t cap) {
	if (!f) return KMR_ERR_INVALID_ARG;
	if (cap < f->keys.size()) return KMR_ERR_CAPACITY;
	if (keys) memcpy(keys, f->keys.data(), 8 * f->keys.size());
	if (values) memcpy(values, f->vals.data(), 4 * f->vals.size());
	return KMR_OK;
}
void kmr_artifact_filter_free(kmr_artifact_filter *f) { free_on_device(f); }

/* the decisions of one apply step in device memory, good while the call's temporaries live */
struct ArtDecisions { const uint32_t *value, *min_pass, *max_pass; const uint8_t *action; };

/* kmr_artifact_filter_apply with mate in device memory (or null) and the temporaries the caller's: *keep takes the decisions */
static int art_apply_core(kmr_handle *h, Scratch &tmp, const kmr_artifact_filter *f, const kmr_reads *in, const int64_t *dmate,
                          uint32_t *value, uint32_t *min_pass, uint32_t *max_pass, uint8_t *action,
                          uint32_t *remnant_off, uint32_t *remnant_len, kmr_reads **out, ArtDecisions *keep) {
	const uint64_t n = in->n;
	ArtifactTable t{f->d_keys.get<uint64_t>(), f->d_vals.get<uint32_t>(), nullptr, f->log2cap, f->d_bits.get<uint32_t>()};
	ArtifactParams P;
	P.length = f->cfg.match_length; P.nSeq = f->n_seq; P.numErrors = f->remaining_edits;
	P.srBegin = f->cfg.simple_repeat_begin; P.srEnd = f->cfg.simple_repeat_end; P.phix = f->cfg.phix_idx; P.refBegin = f->cfg.reference_begin;
	P.minQualChar = (int32_t)(int8_t)(uint8_t)(f->cfg.fastq_start_char + f->cfg.min_quality);
	P.minReadLength = f->cfg.min_read_length;
	uint32_t *dval, *dmin, *dmax, *dro, *drl, *dlen, *dflag; uint8_t *dact; uint64_t *dridx, *dsrc;
	HIPCHK(h, tmp.take(&dval, n)); HIPCHK(h, tmp.take(&dmin, n)); HIPCHK(h, tmp.take(&dmax, n)); HIPCHK(h, tmp.take(&dro, n)); HIPCHK(h, tmp.take(&drl, n));
	HIPCHK(h, tmp.take(&dact, n)); HIPCHK(h, tmp.take(&dflag, n)); HIPCHK(h, tmp.take(&dridx, n + 1));
	if (keep) { keep->value = dval; keep->min_pass = dmin; keep->max_pass = dmax; keep->action = dact; }
	uint64_t n_rem = 0;
	if (n) {
		const unsigned blocks = (unsigned)((n + 255) / 256);
		LAUNCH(h, artifact_screen, dim3(blocks), dim3(256), 0, in->bases.get<uint8_t>(), in->quals.get<uint8_t>(), in->offsets.get<uint64_t>(), n, t, P, dval, dmin, dmax, dro, drl);
	}
	/* lengths after the filter: n reads, then the remnants */
	HIPCHK(h, tmp.take(&dlen, 2 * n + 1));
	if (n) {
		const unsigned blocks = (unsigned)((n + 255) / 256);
		LAUNCH(h, artifact_action, dim3(blocks), dim3(256), 0, in->offsets.get<uint64_t>(), n, dmate, P, dval, dmin, dmax, drl, dact, dlen, dflag);
		int rc = exclusive_scan(h, dflag, n, dridx); if (rc) return rc;
		HIPCHK(h, hipMemcpy(&n_rem, dridx + n, 8, hipMemcpyDeviceToHost));
	}
	HIPCHK(h, tmp.take(&dsrc, n_rem));
	if (n_rem) {
		LAUNCH(h, artifact_remnants, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, n, drl, dridx, dlen, dsrc);
	}
	HIPCHK(h, hipStreamSynchronize(h->stream));
	hipError_t e = hipSuccess;
	if (n) {
		if (value && e == hipSuccess) e = hipMemcpy(value, dval, 4 * n, hipMemcpyDeviceToHost);
		if (min_pass && e == hipSuccess) e = hipMemcpy(min_pass, dmin, 4 * n, hipMemcpyDeviceToHost);
		if (max_pass && e == hipSuccess) e = hipMemcpy(max_pass, dmax, 4 * n, hipMemcpyDeviceToHost);
		if (action && e == hipSuccess) e = hipMemcpy(action, dact, n, hipMemcpyDeviceToHost);
		if (remnant_off && e == hipSuccess) e = hipMemcpy(remnant_off, dro, 4 * n, hipMemcpyDeviceToHost);
		if (remnant_len && e == hipSuccess) e = hipMemcpy(remnant_len, drl, 4 * n, hipMemcpyDeviceToHost);
	}
	HIPCHK(h, e);
	if (!out) return KMR_OK;
	const uint64_t n_out = n + n_rem;
	auto r = make_result<kmr_reads>(h);
	r->n = n_out; r->input_base = in->input_base; r->filtered = in->filtered;
	HIPCHK(h, r->offsets.alloc(8 * (n_out + 1)));
	if (n_out) { int rc = exclusive_scan(h, dlen, n_out, r->offsets.get<uint64_t>()); if (rc) return rc; HIPCHK(h, hipMemcpy(&r->total, r->offsets.get<uint64_t>() + n_out, 8, hipMemcpyDeviceToHost)); }
	else HIPCHK(h, hipMemset(r->offsets.get<uint64_t>(), 0, 8));
	HIPCHK(h, r->bases.alloc(r->total + 64)); HIPCHK(h, r->quals.alloc(r->total + 64));
	HIPCHK(h, hipMemsetAsync(r->bases.get<uint8_t>() + r->total, 0, 64, h->stream)); HIPCHK(h, hipMemsetAsync(r->quals.get<uint8_t>() + r->total, 0, 64, h->stream));
	HIPCHK(h, r->name_off.alloc(8 * std::max<uint64_t>(n_out, 1))); HIPCHK(h, r->name_len.alloc(4 * std::max<uint64_t>(n_out, 1)));
	if (n_out) {
		LAUNCH(h, artifact_gather, dim3((unsigned)std::min<uint64_t>((n_out + 3) / 4, 1u << 16)), dim3(256), 0,
		       in->bases.get<uint8_t>(), in->quals.get<uint8_t>(), in->offsets.get<uint64_t>(), in->name_off.get<uint64_t>(), in->name_len.get<uint32_t>(), n, n_out, dact, dmin, dro, dsrc, r->offsets.get<uint64_t>(), r->bases.get<uint8_t>(), r->quals.get<uint8_t>(), r->name_off.get<uint64_t>(), r->name_len.get<uint32_t>());
	}
	HIPCHK(h, hipStreamSynchronize(h->stream));
	*out = r.release();
	return KMR_OK;
}

int kmr_artifact_filter_apply(kmr_handle *h, const kmr_artifact_filter *f, const kmr_reads *in, const int64_t *mate,
                              uint32_t *value, uint32_t *min_pass, uint32_t *max_pass, uint8_t *action,
                              uint32_t *remnant_off, uint32_t *remnant_len, kmr_reads **out) {
	if (!h || !f || !in) return KMR_ERR_INVALID_ARG;
	if (out) *out = nullptr;
	if (f->device != h->device || in->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "filter, reads and handle must live on one device");
	hipSetDevice(h->device);
	Scratch tmp(h);
	const int64_t *dmate;
	int rc = to_device(h, tmp, mate, in->n, &dmate); if (rc) return rc;
	rc = art_apply_core(h, tmp, f, in, dmate, value, min_pass, max_pass, action, remnant_off, remnant_len, out, nullptr);
	if (!rc) tmp.done();      /* the core has waited for its last work */
	return rc;
}
int kmr_artifact_filter_name(const kmr_artifact_filter *f, uint32_t idx, char *dst, uint64_t capacity) {
	if (!f || !dst || idx == 0 || idx >= f->names.size()) return KMR_ERR_INVALID_ARG;
	const std::string &nm = f->names[idx];
	if (capacity < nm.size() + 1) return KMR_ERR_CAPACITY;
	memcpy(dst, nm.c_str(), nm.size() + 1);
	return KMR_OK;
}

/* ---- selectReads / writePicks on the device (kmr_select.hpp) ---------------- */
int kmr_select_config_init(kmr_select_config *c) {
	if (!c) return KMR_ERR_INVALID_ARG;
	memset(c, 0, sizeof(*c));
	c->struct_size = (uint32_t)sizeof(kmr_select_config);
	c->minimum_score = 2.0;            /* --min-depth, apps/FilterReads.cpp:197-199 */
	c->min_read_length = 0.40f;        /* --min-read-length, src/ReadSelector.h:72 */
	c->both_pass = 0;                  /* --min-passing-in-pair 1, src/ReadSelector.h:72 */
	c->output_quality_base = 33;       /* --fastq-output-base-quality */
	c->format = 0;                     /* --format-output 0 = FASTQ */
	c->scoring_type = KMR_SCORE_MEDIAN;
	return KMR_OK;
}

static int select_check_config(kmr_handle *h, const kmr_select_config *c) {
	if (!c) return fail(h, KMR_ERR_INVALID_ARG, "kmr_select_config: NULL");
	if (c->struct_size != sizeof(kmr_select_config)) return fail(h, KMR_ERR_INVALID_ARG, "kmr_select_config: struct_size " + std::to_string(c->struct_size) + " is not " + std::to_string(sizeof(kmr_select_config)));
	if (c->format > 1) return fail(h, KMR_ERR_INVALID_ARG, "kmr_select_config: format must be 0 (FASTQ) or 1 (FASTA)");
	if (c->output_quality_base != 33 && c->output_quality_base != 64) return fail(h, KMR_ERR_INVALID_ARG, "kmr_select_config: output_quality_base must be 33 or 64");
	if (c->scoring_type > 4) return fail(h, KMR_ERR_INVALID_ARG, "kmr_select_config: bad scoring_type");
	if (!(c->min_read_length >= 0.0f)) return fail(h, KMR_ERR_INVALID_ARG, "kmr_select_config: min_read_length must not be negative");
	return 0;
}

typedef EventTimer<3> SelectTimer;

/* What one of the twelve selecting entry points was called with, by name.  Every array but a text that lies on the device is the
 * host's; an absent one is null.  The plain and the partitioned four pass mate, the normalizing four the pair list in its place. */
struct SelectCall {
	const char *who;
	bool fused;                                  /* the read_batch forms: the four trim arrays are scored here */
	const kmr_reads *r;
	const void *text; uint64_t text_len; bool text_on_device;
	const int64_t *mate, *read1, *read2; uint64_t n_pairs;
	const uint8_t *af_action; const uint32_t *af_min, *af_max;
	const uint32_t *trim_offset, *trim_length; const float *score; const uint8_t *was_trimmed;
	const uint64_t *input_starts; uint32_t n_inputs;      /* as the caller gave them; the check makes n_inputs 1 for no input_starts */
	/* by the check of the entry point's config: */
	const kmr_select_config *cfg; SelRounds R; const kmr_normalize_config *norm;
	bool plain;                                  /* the picks hold no per-read segments (they follow from the flags) */
};

/* every pointer is device memory (mate and the three af_* may be null) */
static SelectParams select_params(kmr_handle *h, const kmr_reads *r, const uint8_t *dtext, uint64_t text_len, const int64_t *dmate, const uint8_t *dact, const uint32_t *dmin,
                                  const uint32_t *dmax, const uint32_t *dto, const uint32_t *dtl, const float *dsc, const uint8_t *dwt, const uint64_t *dbm, const kmr_select_config *cfg) {
	SelectParams P;
	P.bases = r->bases.get<uint8_t>(); P.quals = r->quals.get<uint8_t>(); P.offsets = r->offsets.get<uint64_t>(); P.name_off = r->name_off.get<uint64_t>(); P.name_len = r->name_len.get<uint32_t>();
	P.text = dtext; P.text_len = text_len; P.mate = dmate; P.af_action = dact; P.af_min = dmin; P.af_max = dmax;
	P.trim_off = dto; P.trim_len = dtl; P.score = dsc; P.was_trimmed = dwt; P.bimodal = dbm; P.n = r->n;
	P.min_score = (float)cfg->minimum_score; P.min_read_length = cfg->min_read_length; P.both_pass = cfg->both_pass ? 1u : 0u; P.fasta = cfg->format; P.scoring = cfg->scoring_type;
	P.out_base = cfg->output_quality_base; P.qual_shift = (int32_t)cfg->output_quality_base - (int32_t)h->cfg.fastq_start_char;
	return P;
}

/* the units of the partition: at most `most` wavefronts -- 4096 over reads, 8192 over the slots of the normalization, whose kernels do
 * less per item (4 and 8 a SIMD on 256 CUs; each measured against the other and against 1024 and 2048) --, fewer when many
 * segments make the [segment][unit] matrices large (never above 2^18 entries beyond 1024 units; kmr_tune "partition_units" sets them
 * for tests and sweeps), each over a multiple of 64 items */
static void partition_units(const kmr_handle *h, uint64_t n, uint32_t n_segments, uint64_t most, PartitionParams &Q) {
	most = h->tune.partition_units ? h->tune.partition_units : std::min<uint64_t>(most, std::max<uint64_t>(1024, (1u << 18) / n_segments));
	Q.per_unit = (((n + most - 1) / most) + SEL_UNIT - 1) / SEL_UNIT * SEL_UNIT;
	Q.n_units = (uint32_t)((n + Q.per_unit - 1) / Q.per_unit);
}

/* what partition_run hands to a branch's classification */
struct PartitionWork {
	PartitionParams Q;
	uint8_t *picked; int32_t *read_seg; uint32_t *name_printed;      /* per read */
	uint64_t n_items; int32_t *item_seg; uint32_t *item_len, *slot_read;      /* per item; read_seg is item_seg where the items are the reads */
	uint32_t *unit_cnt; unsigned long long *unit_bytes;                  /* [segment][unit] */
	uint32_t *err; unsigned long long *extra;                            /* the error word; the branch's own counters, zero */
};

/* the writer of a partition_run: queues the kernel that prints pick p = read pread[p] at byte poff[p] of the picks' text */
typedef std::function<int(const PartitionWork &, const uint32_t *pread, const uint64_t *poff, kmr_picks *pk)> PartitionWriter;
static PartitionWriter select_writer(kmr_handle *h, const SelectParams &P) {
	return [h, &P](const PartitionWork &W, const uint32_t *pread, const uint64_t *poff, kmr_picks *pk) -> int {
		LAUNCH(h, select_write_kernel, dim3((unsigned)std::min<uint64_t>((pk->n_picked + SEL_WAVES - 1) / SEL_WAVES, (uint64_t)num_cus(h) * 8)), dim3(SEL_THREADS), 0, P,
		                   (const uint32_t *)W.name_printed, pread, poff, pk->n_picked, pk->text.get<uint8_t>());
		return 0;
	};
}

/* A selection from its classification on: the stable partition of the picked items by segment, and their text.  The items are the
 * n reads (the partitioned and the plain entry points), or n_items slots that hold reads (`slots`: two a read for the normalizing
 * entry points, two a pair of the list for the artifact report).
 * `classify` queues the kernels that leave every item's segment (-1: not picked) and record bytes, every picked read's printed name
 * length, every read's flag and segment, and the picks and bytes of every segment per unit.  After it partition_scan_kernel,
 * partition_rank_kernel, the call's one copy of sizes -- picks, bytes, the error word, the segment table, n_extra counters of the
 * branch -- and the writer (select_writer, or the report's).  keep_read_seg: the picks keep the per-read segments. */
static int partition_run(kmr_handle *h, Scratch &tmp, uint64_t n, uint64_t n_items, const SelRounds &R, uint32_t n_inputs, uint32_t n_segments, const uint64_t *dstarts, bool slots,
                         bool keep_read_seg, uint64_t *extra, size_t n_extra, kmr_picks *pk,
                         const std::function<int(const PartitionWork &)> &classify, const PartitionWriter &write) {
	const uint32_t S = n_segments;
	pk->n = n; pk->n_rounds = R.n; pk->n_inputs = n_inputs;
	for (uint32_t r = 0; r < R.n; r++) { pk->round_depth[r] = R.min_score[r]; pk->round_is_remainder[r] = R.is_remainder[r]; }
	pk->seg_table.assign((size_t)4 * S, 0);
	h->last_select_ms = h->last_write_ms = 0;
	if (n == 0) return KMR_OK;
	PartitionWork W;
	HIPCHK(h, alloc_n(pk->picked, &W.picked, n));
	HIPCHK(h, keep_read_seg ? alloc_n(pk->read_seg, &W.read_seg, n) : tmp.take(&W.read_seg, n));
	if (S == 0) {      /* --partition-by-depth below --min-depth: no round runs */
		HIPCHK(h, hipMemsetAsync(W.picked, 0, n, h->stream)); HIPCHK(h, hipMemsetAsync(W.read_seg, 0xff, 4 * n, h->stream)); HIPCHK(h, hipStreamSynchronize(h->stream));
		return KMR_OK;
	}
	W.n_items = n_items; W.item_seg = W.read_seg; W.slot_read = nullptr;
	W.Q.input_starts = dstarts; W.Q.n_inputs = n_inputs; W.Q.n_segments = S;
	partition_units(h, W.n_items, S, slots ? 8192 : 4096, W.Q);
	const size_t cells = (size_t)S * W.Q.n_units, n_tot = 3 + (size_t)4 * S + n_extra;
	uint32_t *pread; uint64_t *poff, *tot;
	if (slots) { HIPCHK(h, tmp.take(&W.item_seg, W.n_items)); HIPCHK(h, tmp.take(&W.slot_read, W.n_items)); }
	/* pread / poff: an item each -- a pair list that names a read twice (refused below) can fill more than n slots */
	HIPCHK(h, tmp.take(&W.name_printed, n + W.n_items)); HIPCHK(h, tmp.take(&pread, W.n_items)); HIPCHK(h, tmp.take(&poff, W.n_items + 1));
	W.item_len = W.name_printed + n;      /* one block */
	HIPCHK(h, tmp.take(&W.unit_cnt, cells)); HIPCHK(h, tmp.take(&W.unit_bytes, cells)); HIPCHK(h, tmp.take(&tot, n_tot));
	W.err = (uint32_t *)(tot + 2); W.extra = (unsigned long long *)(tot + 3 + (size_t)4 * S);
	SelectTimer timer(h->tune.select_timing);
	timer.mark(0, h->stream);
	HIPCHK(h, hipMemsetAsync(tot, 0, 8 * n_tot, h->stream));
	int rc = classify(W); if (rc) return rc;
	LAUNCH(h, partition_scan_kernel, dim3(1), dim3(SEL_SCAN_THREADS), 0, W.unit_cnt, W.unit_bytes, S, W.Q.n_units, tot + 3, poff, tot);
	LAUNCH(h, partition_rank_kernel, dim3(W.Q.n_units), dim3(SEL_UNIT), 0, (const int32_t *)W.item_seg, (const uint32_t *)W.item_len, W.n_items, W.Q, (const uint32_t *)W.unit_cnt,
	       (const unsigned long long *)W.unit_bytes, pread, poff, (const uint32_t *)W.slot_read);
	std::vector<uint64_t> host_tot(n_tot, 0);
	HIPCHK(h, fetch(h, host_tot.data(), tot, n_tot));
	if (host_tot[2] & SEL_ERR_MATE) return fail(h, KMR_ERR_INVALID_ARG, "a mate index lies outside the batch");
	if (host_tot[2] & SEL_ERR_NAME) return fail(h, KMR_ERR_INVALID_ARG, NAME_SPAN_ERROR);
	if (host_tot[2] & SEL_ERR_PAIR) return fail(h, KMR_ERR_INVALID_ARG, "the pair list holds an index outside the batch or a pair without a read");
	if (host_tot[2] & SEL_ERR_TWICE) return fail(h, KMR_ERR_INVALID_ARG, "the pair list names a read twice");
	if (host_tot[2] & SEL_ERR_UNNAMED) return fail(h, KMR_ERR_INVALID_ARG, "the pair list leaves a read out (identifyPairs names every read, a single one as a pair with one side)");
	if (host_tot[2] & SEL_ERR_VALUE) return fail(h, KMR_ERR_INVALID_ARG, "a value lies above the filter's n_sequences");
	pk->n_picked = host_tot[0]; pk->bytes = host_tot[1];
	timer.mark(1, h->stream);
	if (pk->bytes) {
		HIPCHK(h, pk->text.alloc((pk->bytes + 15) & ~(uint64_t)15));
		{ int rc = write(W, pread, poff, pk); if (rc) return rc; }
	}
	timer.mark(2, h->stream);
	HIPCHK(h, hipStreamSynchronize(h->stream));
	tmp.done();
	h->last_select_ms = timer.ms(0, 2); h->last_write_ms = timer.ms(1, 2);
	std::copy(host_tot.begin() + 3, host_tot.end() - n_extra, pk->seg_table.begin());
	std::copy(host_tot.end() - n_extra, host_tot.end(), extra);
	return KMR_OK;
}

/* the plain and the partitioned entry points: P's three thresholds are not read, R the rounds, dstarts the inputs' first reads in
 * device memory (null for one input) */
static int partition_core(kmr_handle *h, Scratch &tmp, const SelectParams &P, const SelRounds &R, const uint64_t *dstarts, uint32_t n_inputs, bool keep_read_seg, kmr_picks *pk) {
	return partition_run(h, tmp, P.n, P.n, R, n_inputs, R.n * n_inputs, dstarts, false, keep_read_seg, nullptr, 0, pk, [&](const PartitionWork &W) -> int {
		LAUNCH(h, partition_classify_kernel, dim3(W.Q.n_units), dim3(SEL_UNIT), 0, P, R, W.Q, W.read_seg, W.item_len, W.name_printed, W.picked, W.unit_cnt, W.unit_bytes, W.err);
		return 0;
	}, select_writer(h, P));
}

/* the one round of a kmr_select_config (checked): what the plain entry points pick, and the partitioned ones with partition_by_depth 0 */
static void select_one_round(const kmr_select_config &c, SelRounds *R) {
	R->n = 1; R->min_score[0] = (float)c.minimum_score; R->min_read_length[0] = c.min_read_length; R->both_pass[0] = c.both_pass ? 1 : 0; R->is_remainder[0] = 0;
}

/* cfg, the input boundaries and the table of rounds, all without a device.  *n_inputs: 1 for input_starts NULL */
static int partition_check(kmr_handle *h, const kmr_partition_config *c, const uint64_t *input_starts, SelRounds *R, uint32_t *n_inputs) {
	if (!c) return fail(h, KMR_ERR_INVALID_ARG, "kmr_partition_config: NULL");
	if (c->struct_size != sizeof(kmr_partition_config)) return fail(h, KMR_ERR_INVALID_ARG, "kmr_partition_config: struct_size " + std::to_string(c->struct_size) + " is not " + std::to_string(sizeof(kmr_partition_config)));
	int rc = select_check_config(h, &c->select); if (rc) return rc;
	if (input_starts) {
		if (*n_inputs == 0) return fail(h, KMR_ERR_INVALID_ARG, "input_starts without n_inputs");
		bool ok;
		const uint32_t at = sel_check_input_starts(input_starts, *n_inputs, &ok);
		if (!ok) return fail(h, KMR_ERR_INVALID_ARG, "input_starts[" + std::to_string(at) + "]: the read indices start at 0 and ascend");
	} else if (*n_inputs > 1) return fail(h, KMR_ERR_INVALID_ARG, "input_starts is NULL for " + std::to_string(*n_inputs) + " inputs");
	else *n_inputs = 1;
	if (c->partition_by_depth == 0) select_one_round(c->select, R);
	else {
		const double d = c->select.minimum_score;      /* selectReads takes minDepth as an unsigned int */
		if (!(d >= 0.0 && d <= 4294967295.0) || d != std::floor(d)) return fail(h, KMR_ERR_INVALID_ARG, "kmr_partition_config: with partition_by_depth set, minimum_score is a whole number below 2^32");
		if (sel_round_table((unsigned int)d, c->partition_by_depth, c->remainder_trim, c->select.min_read_length, c->select.both_pass != 0, *R))
			return fail(h, KMR_ERR_UNSUPPORTED, "kmr_partition_config: more than " + std::to_string((int)SEL_MAX_ROUNDS) + " rounds");
	}
	if ((uint64_t)R->n * *n_inputs > (uint64_t)SEL_MAX_SEGMENTS)
		return fail(h, KMR_ERR_UNSUPPORTED, std::to_string(R->n) + " rounds x " + std::to_string(*n_inputs) + " inputs: more than " + std::to_string((int)SEL_MAX_SEGMENTS) + " segments");
	return 0;
}

/* ---- the normalizing branch (kmr_normalize.hpp) ---------------- */
/* cfg, the pair list's shape and the input boundaries, all without a device.  R: the one round.  *n_inputs: 1 for input_starts NULL */
static int normalize_check(kmr_handle *h, const kmr_normalize_config *c, const int64_t *read1, const int64_t *read2, const uint64_t *input_starts, SelRounds *R, uint32_t *n_inputs) {
	if (!c) return fail(h, KMR_ERR_INVALID_ARG, "kmr_normalize_config: NULL");
	if (c->struct_size != sizeof(kmr_normalize_config)) return fail(h, KMR_ERR_INVALID_ARG, "kmr_normalize_config: struct_size " + std::to_string(c->struct_size) + " is not " + std::to_string(sizeof(kmr_normalize_config)));
	if (c->method != 0) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_normalize_config: method 0 (RANDOM) only; OPTIMAL is a serial greedy heap over a shared count map");
	if (c->use_logscale) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_normalize_config: use_logscale (the reference's expression has no pinned value)");
	if (c->target_depth == 0) return fail(h, KMR_ERR_INVALID_ARG, "kmr_normalize_config: target_depth must be above 0");
	if ((read1 != nullptr) != (read2 != nullptr)) return fail(h, KMR_ERR_INVALID_ARG, "the pair list: read1 and read2 go together");
	kmr_partition_config pc;
	kmr_partition_config_init(&pc);
	pc.select = c->select;
	return partition_check(h, &pc, input_starts, R, n_inputs);
}

/* P with mate null; dr1 / dr2 the pair list and dstarts the inputs' first reads in device memory (null for none).  A segment is
 * an input */
static int normalize_core(kmr_handle *h, Scratch &tmp, const SelectParams &P, const SelRounds &R, const kmr_normalize_config *c, const int64_t *dr1, const int64_t *dr2, uint64_t n_pairs,
                          const uint64_t *dstarts, uint32_t n_inputs, kmr_picks *pk) {
	const uint64_t n = P.n;
	NormalizeParams N;
	N.read1 = dr1; N.read2 = dr2; N.n_pairs = n_pairs; N.target = c->target_depth; N.seed = c->seed; N.first_global = c->first_global_read_idx; N.by_pair = c->by_pair ? 1u : 0u;
	uint32_t *named = nullptr;      /* reads named by a pair */
	if (n) HIPCHK(h, tmp.take(&named, n));
	pk->normalized = true;
	return partition_run(h, tmp, n, 2 * n, R, n_inputs, n_inputs, dstarts, true, true, pk->norm_info, 3, pk, [&](const PartitionWork &W) -> int {
		HIPCHK(h, hipMemsetAsync(named, 0, 4 * n, h->stream)); HIPCHK(h, hipMemsetAsync(W.item_seg, 0xff, 4 * W.n_items, h->stream));
		HIPCHK(h, hipMemsetAsync(W.read_seg, 0xff, 4 * n, h->stream)); HIPCHK(h, hipMemsetAsync(W.picked, 0, n, h->stream));
		if (n_pairs) LAUNCH(h, normalize_mark_kernel, dim3(grid_for(n_pairs)), dim3(256), 0, N, n, named, W.err);
		LAUNCH(h, normalize_classify_kernel, dim3(grid_for(n_pairs + n)), dim3(256), 0, P, N, W.Q, (const uint32_t *)named, W.slot_read, W.item_seg, W.item_len, W.name_printed, W.picked,
		       W.read_seg, W.extra, W.err);
		LAUNCH(h, normalize_count_kernel, dim3(W.Q.n_units), dim3(SEL_UNIT), 0, (const int32_t *)W.item_seg, (const uint32_t *)W.item_len, W.n_items, W.Q, W.unit_cnt, W.unit_bytes);
		return 0;
	}, select_writer(h, P));
}

static int select_check_args(kmr_handle *h, const SelectCall &c, kmr_picks **out) {
	const std::string who = c.who;
	if (out) *out = nullptr;
	int rc = select_check_config(h, c.cfg); if (rc) return rc;
	if (!h) return fail(h, KMR_ERR_INVALID_ARG, who + ": NULL handle");
	if (!c.r || !out || (c.text_len && !c.text)) return fail(h, KMR_ERR_INVALID_ARG, who + ": NULL argument");
	if ((c.af_action != nullptr) != (c.af_min != nullptr) || (c.af_action != nullptr) != (c.af_max != nullptr)) return fail(h, KMR_ERR_INVALID_ARG, who + ": af_action, af_min_pass and af_max_pass go together");
	if (c.r->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "read batch lives on another device");
	if (c.r->n >= 0xffffffffull) return fail(h, KMR_ERR_UNSUPPORTED, who + ": a batch holds fewer than 2^32 - 1 reads (pick indices are 32-bit)");
	if (c.input_starts && c.input_starts[c.n_inputs] != c.r->n)
		return fail(h, KMR_ERR_INVALID_ARG, who + ": input_starts ends at " + std::to_string(c.input_starts[c.n_inputs]) + ", the batch holds " + std::to_string(c.r->n) + " reads");
	if (c.read1 && c.n_pairs && !c.r->n) return fail(h, KMR_ERR_INVALID_ARG, who + ": a pair list for an empty batch");
	if (c.fused) { if (!h->finalized) return fail(h, KMR_ERR_STATE, who + " before kmr_finalize"); }
	else if (c.r->n && (!c.trim_offset || !c.trim_length || !c.score || !c.was_trimmed)) return fail(h, KMR_ERR_INVALID_ARG, who + ": NULL argument");
	return 0;
}

/* a call whose config is checked: the arguments to the device, the scores of the fused form, the pipeline */
static int select_run(kmr_handle *h, const SelectCall &c, kmr_picks **out) {
	int rc = select_check_args(h, c, out); if (rc) return rc;
	hipSetDevice(h->device);
	const kmr_reads *r = c.r;
	const uint64_t n = r->n, n_pairs = c.read1 ? c.n_pairs : 0;
	auto pk = make_result<kmr_picks>(h);      /* (ahead of tmp, as in every stage: a failed call waits for the stream before the result's buffers go too) */
	Scratch tmp(h);
	const uint8_t *dtext, *dact, *dwt = nullptr; const int64_t *dmate, *dr1, *dr2; const uint32_t *dmin, *dmax, *dto = nullptr, *dtl = nullptr; const float *dsc = nullptr; const uint64_t *dstarts, *dbm = nullptr;
	/* the tags kmr_select_bimodal left for this call (the host-array forms; a fused call scores, and tags, its reads itself) */
	std::vector<uint64_t> tags; bool tagged = false;
	if (!c.fused) { tags.swap(h->sel_bimodal); tagged = h->sel_bimodal_set; h->sel_bimodal_set = false; }
	if (tagged && tags.size() != n) return fail(h, KMR_ERR_INVALID_ARG, std::string(c.who) + ": kmr_select_bimodal gave " + std::to_string(tags.size()) + " words, the batch holds " + std::to_string(n) + " reads");
	rc = to_device(h, tmp, (const uint8_t *)c.text, c.text_len, &dtext, c.text_on_device); if (rc) return rc;
	rc = to_device(h, tmp, c.mate, n, &dmate); if (rc) return rc;
	rc = to_device(h, tmp, c.af_action, n, &dact); if (rc) return rc;
	rc = to_device(h, tmp, c.af_min, n, &dmin); if (rc) return rc;
	rc = to_device(h, tmp, c.af_max, n, &dmax); if (rc) return rc;
	h->last_score_ms = 0;
	if (c.fused && n) {
		SelectTimer timer(h->tune.select_timing);
		timer.mark(0, h->stream);
		ScoreDev sd;
		rc = score_reads_core(h, r->bases.get<uint8_t>(), r->offsets.get<uint64_t>(), n, c.cfg->minimum_score, (int)c.cfg->scoring_type, nullptr, nullptr, nullptr, nullptr, &sd); if (rc) return rc;
		timer.mark(1, h->stream);
		if (timer.on) { HIPCHK(h, hipStreamSynchronize(h->stream)); h->last_score_ms = timer.ms(0, 1); }
		dto = sd.trim_offset; dtl = sd.trim_length; dsc = sd.score; dwt = sd.was_trimmed; dbm = sd.bimodal;
	} else if (!c.fused) {
		rc = to_device(h, tmp, c.trim_offset, n, &dto); if (rc) return rc;
		rc = to_device(h, tmp, c.trim_length, n, &dtl); if (rc) return rc;
		rc = to_device(h, tmp, c.score, n, &dsc); if (rc) return rc;
		rc = to_device(h, tmp, c.was_trimmed, n, &dwt); if (rc) return rc;
		rc = to_device(h, tmp, tagged && n ? tags.data() : nullptr, n, &dbm); if (rc) return rc;
	}
	rc = to_device(h, tmp, c.n_inputs > 1 ? c.input_starts : nullptr, (uint64_t)c.n_inputs + 1, &dstarts); if (rc) return rc;
	rc = to_device(h, tmp, c.read1, n_pairs, &dr1); if (rc) return rc;
	rc = to_device(h, tmp, c.read2, n_pairs, &dr2); if (rc) return rc;
	const SelectParams P = select_params(h, r, dtext, c.text_len, dmate, dact, dmin, dmax, dto, dtl, dsc, dwt, dbm, c.cfg);
	if (c.norm) rc = normalize_core(h, tmp, P, c.R, c.norm, dr1, dr2, n_pairs, dstarts, c.n_inputs, pk.get());
	else rc = partition_core(h, tmp, P, c.R, dstarts, c.n_inputs, !c.plain, pk.get());
	if (!rc) *out = pk.release();
	return rc;
}

/* the three kinds of entry point: each checks its config, which gives the call its rounds, and runs the call */
static int select_plain(kmr_handle *h, SelectCall &c, const kmr_select_config *cfg, kmr_picks **out) {
	if (out) *out = nullptr;
	int rc = select_check_config(h, cfg); if (rc) return rc;
	c.cfg = cfg; c.plain = true; c.n_inputs = 1;
	select_one_round(*cfg, &c.R);
	return select_run(h, c, out);
}
static int select_partitioned(kmr_handle *h, SelectCall &c, const kmr_partition_config *cfg, kmr_picks **out) {
	if (out) *out = nullptr;
	int rc = partition_check(h, cfg, c.input_starts, &c.R, &c.n_inputs); if (rc) return rc;
	c.cfg = &cfg->select;
	return select_run(h, c, out);
}
static int select_normalized(kmr_handle *h, SelectCall &c, const kmr_normalize_config *cfg, kmr_picks **out) {
	if (out) *out = nullptr;
	int rc = normalize_check(h, cfg, c.read1, c.read2, c.input_starts, &c.R, &c.n_inputs); if (rc) return rc;
	c.cfg = &cfg->select; c.norm = cfg;
	return select_run(h, c, out);
}

/* the words kmr_bimodal_copy returned for the trims of the next kmr_select_reads* / kmr_partition_reads* / kmr_normalize_reads* on the handle:
 * their tags go into the labels that call prints.  The call consumes them; NULL takes them back. */
int kmr_select_bimodal(kmr_handle *h, const uint64_t *words, uint64_t n_reads) {
	if (!h) return KMR_ERR_INVALID_ARG;
	h->sel_bimodal.clear(); h->sel_bimodal_set = false;
	if (!words) return KMR_OK;
	h->sel_bimodal.assign(words, words + n_reads); h->sel_bimodal_set = true;
	return KMR_OK;
}
int kmr_select_reads(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, const int64_t *mate, const uint8_t *af_action, const uint32_t *af_min_pass,
                     const uint32_t *af_max_pass, const uint32_t *trim_offset, const uint32_t *trim_length, const float *score, const uint8_t *was_trimmed,
                     const kmr_select_config *cfg, kmr_picks **out) {
	SelectCall c = {};
	c.who = "kmr_select_reads"; c.r = reads; c.text = text; c.text_len = text_len; c.mate = mate; c.af_action = af_action; c.af_min = af_min_pass; c.af_max = af_max_pass;
	c.trim_offset = trim_offset; c.trim_length = trim_length; c.score = score; c.was_trimmed = was_trimmed;
	return select_plain(h, c, cfg, out);
}
int kmr_select_reads_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, const int64_t *mate, const uint8_t *af_action, const uint32_t *af_min_pass,
                         const uint32_t *af_max_pass, const uint32_t *trim_offset, const uint32_t *trim_length, const float *score, const uint8_t *was_trimmed,
                         const kmr_select_config *cfg, kmr_picks **out) {
	SelectCall c = {};
	c.who = "kmr_select_reads_dev"; c.r = reads; c.text = dev_text; c.text_len = text_len; c.text_on_device = true; c.mate = mate; c.af_action = af_action; c.af_min = af_min_pass; c.af_max = af_max_pass;
	c.trim_offset = trim_offset; c.trim_length = trim_length; c.score = score; c.was_trimmed = was_trimmed;
	return select_plain(h, c, cfg, out);
}
int kmr_filter_read_batch(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, const int64_t *mate, const uint8_t *af_action, const uint32_t *af_min_pass,
                          const uint32_t *af_max_pass, const kmr_select_config *cfg, kmr_picks **out) {
	SelectCall c = {};
	c.who = "kmr_filter_read_batch"; c.fused = true; c.r = reads; c.text = text; c.text_len = text_len; c.mate = mate; c.af_action = af_action; c.af_min = af_min_pass; c.af_max = af_max_pass;
	return select_plain(h, c, cfg, out);
}
int kmr_filter_read_batch_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, const int64_t *mate, const uint8_t *af_action, const uint32_t *af_min_pass,
                              const uint32_t *af_max_pass, const kmr_select_config *cfg, kmr_picks **out) {
	SelectCall c = {};
	c.who = "kmr_filter_read_batch_dev"; c.fused = true; c.r = reads; c.text = dev_text; c.text_len = text_len; c.text_on_device = true; c.mate = mate;
	c.af_action = af_action; c.af_min = af_min_pass; c.af_max = af_max_pass;
	return select_plain(h, c, cfg, out);
}

/* ---- the partitioned branch: the same four with the rounds of kmr_partition_config and the inputs' boundaries ---------------- */
int kmr_partition_config_init(kmr_partition_config *c) {
	if (!c) return KMR_ERR_INVALID_ARG;
	memset(c, 0, sizeof(*c));
	c->struct_size = (uint32_t)sizeof(kmr_partition_config);
	kmr_select_config_init(&c->select);
	c->partition_by_depth = 0;         /* --partition-by-depth -1, src/ReadSelector.h:72: off */
	c->remainder_trim = -1.0f;         /* --remainder-trim -1, src/ReadSelector.h:72: off */
	return KMR_OK;
}
int kmr_partition_rounds(const kmr_partition_config *cfg, uint32_t *n_rounds, float *round_depth, float *round_min_read_length, uint32_t *round_both_pass, uint8_t *round_is_remainder) {
	SelRounds R; uint32_t n_inputs = 0;
	int rc = partition_check(nullptr, cfg, nullptr, &R, &n_inputs); if (rc) return rc;
	if (n_rounds) *n_rounds = R.n;
	for (uint32_t r = 0; r < R.n; r++) {
		if (round_depth) round_depth[r] = R.min_score[r]; if (round_min_read_length) round_min_read_length[r] = R.min_read_length[r];
		if (round_both_pass) round_both_pass[r] = R.both_pass[r]; if (round_is_remainder) round_is_remainder[r] = R.is_remainder[r];
	}
	return KMR_OK;
}
int kmr_partition_reads(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, const int64_t *mate, const uint8_t *af_action, const uint32_t *af_min_pass,
                        const uint32_t *af_max_pass, const uint32_t *trim_offset, const uint32_t *trim_length, const float *score, const uint8_t *was_trimmed,
                        const uint64_t *input_starts, uint32_t n_inputs, const kmr_partition_config *cfg, kmr_picks **out) {
	SelectCall c = {};
	c.who = "kmr_partition_reads"; c.r = reads; c.text = text; c.text_len = text_len; c.mate = mate; c.af_action = af_action; c.af_min = af_min_pass; c.af_max = af_max_pass;
	c.trim_offset = trim_offset; c.trim_length = trim_length; c.score = score; c.was_trimmed = was_trimmed; c.input_starts = input_starts; c.n_inputs = n_inputs;
	return select_partitioned(h, c, cfg, out);
}
int kmr_partition_reads_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, const int64_t *mate, const uint8_t *af_action, const uint32_t *af_min_pass,
                            const uint32_t *af_max_pass, const uint32_t *trim_offset, const uint32_t *trim_length, const float *score, const uint8_t *was_trimmed,
                            const uint64_t *input_starts, uint32_t n_inputs, const kmr_partition_config *cfg, kmr_picks **out) {
	SelectCall c = {};
	c.who = "kmr_partition_reads_dev"; c.r = reads; c.text = dev_text; c.text_len = text_len; c.text_on_device = true; c.mate = mate; c.af_action = af_action; c.af_min = af_min_pass; c.af_max = af_max_pass;
	c.trim_offset = trim_offset; c.trim_length = trim_length; c.score = score; c.was_trimmed = was_trimmed; c.input_starts = input_starts; c.n_inputs = n_inputs;
	return select_partitioned(h, c, cfg, out);
}
int kmr_partition_read_batch(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, const int64_t *mate, const uint8_t *af_action, const uint32_t *af_min_pass,
                             const uint32_t *af_max_pass, const uint64_t *input_starts, uint32_t n_inputs, const kmr_partition_config *cfg, kmr_picks **out) {
	SelectCall c = {};
	c.who = "kmr_partition_read_batch"; c.fused = true; c.r = reads; c.text = text; c.text_len = text_len; c.mate = mate; c.af_action = af_action; c.af_min = af_min_pass; c.af_max = af_max_pass;
	c.input_starts = input_starts; c.n_inputs = n_inputs;
	return select_partitioned(h, c, cfg, out);
}
int kmr_partition_read_batch_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, const int64_t *mate, const uint8_t *af_action, const uint32_t *af_min_pass,
                                 const uint32_t *af_max_pass, const uint64_t *input_starts, uint32_t n_inputs, const kmr_partition_config *cfg, kmr_picks **out) {
	SelectCall c = {};
	c.who = "kmr_partition_read_batch_dev"; c.fused = true; c.r = reads; c.text = dev_text; c.text_len = text_len; c.text_on_device = true; c.mate = mate;
	c.af_action = af_action; c.af_min = af_min_pass; c.af_max = af_max_pass; c.input_starts = input_starts; c.n_inputs = n_inputs;
	return select_partitioned(h, c, cfg, out);
}
/* ---- the normalizing branch: the same four with the pair list in place of mate, and the draws' parameters ---------------- */
int kmr_normalize_config_init(kmr_normalize_config *c) {
	if (!c) return KMR_ERR_INVALID_ARG;
	memset(c, 0, sizeof(*c));
	c->struct_size = (uint32_t)sizeof(kmr_normalize_config);
	kmr_select_config_init(&c->select);
	c->target_depth = 0;               /* --max-kmer-output-depth -1, src/ReadSelector.h:72: off; the caller sets it */
	c->by_pair = 0;                    /* selectReads passes reads.hasPairs() (apps/FilterReads.h:184) */
	return KMR_OK;
}
int kmr_normalize_reads(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, const int64_t *read1, const int64_t *read2, uint64_t n_pairs,
                        const uint8_t *af_action, const uint32_t *af_min_pass, const uint32_t *af_max_pass, const uint32_t *trim_offset, const uint32_t *trim_length, const float *score,
                        const uint8_t *was_trimmed, const uint64_t *input_starts, uint32_t n_inputs, const kmr_normalize_config *cfg, kmr_picks **out) {
	SelectCall c = {};
	c.who = "kmr_normalize_reads"; c.r = reads; c.text = text; c.text_len = text_len; c.read1 = read1; c.read2 = read2; c.n_pairs = n_pairs; c.af_action = af_action; c.af_min = af_min_pass; c.af_max = af_max_pass;
	c.trim_offset = trim_offset; c.trim_length = trim_length; c.score = score; c.was_trimmed = was_trimmed; c.input_starts = input_starts; c.n_inputs = n_inputs;
	return select_normalized(h, c, cfg, out);
}
int kmr_normalize_reads_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, const int64_t *read1, const int64_t *read2, uint64_t n_pairs,
                            const uint8_t *af_action, const uint32_t *af_min_pass, const uint32_t *af_max_pass, const uint32_t *trim_offset, const uint32_t *trim_length, const float *score,
                            const uint8_t *was_trimmed, const uint64_t *input_starts, uint32_t n_inputs, const kmr_normalize_config *cfg, kmr_picks **out) {
	SelectCall c = {};
	c.who = "kmr_normalize_reads_dev"; c.r = reads; c.text = dev_text; c.text_len = text_len; c.text_on_device = true; c.read1 = read1; c.read2 = read2; c.n_pairs = n_pairs;
	c.af_action = af_action; c.af_min = af_min_pass; c.af_max = af_max_pass;
	c.trim_offset = trim_offset; c.trim_length = trim_length; c.score = score; c.was_trimmed = was_trimmed; c.input_starts = input_starts; c.n_inputs = n_inputs;
	return select_normalized(h, c, cfg, out);
}
int kmr_normalize_read_batch(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, const int64_t *read1, const int64_t *read2, uint64_t n_pairs,
                             const uint8_t *af_action, const uint32_t *af_min_pass, const uint32_t *af_max_pass, const uint64_t *input_starts, uint32_t n_inputs,
                             const kmr_normalize_config *cfg, kmr_picks **out) {
	SelectCall c = {};
	c.who = "kmr_normalize_read_batch"; c.fused = true; c.r = reads; c.text = text; c.text_len = text_len; c.read1 = read1; c.read2 = read2; c.n_pairs = n_pairs;
	c.af_action = af_action; c.af_min = af_min_pass; c.af_max = af_max_pass; c.input_starts = input_starts; c.n_inputs = n_inputs;
	return select_normalized(h, c, cfg, out);
}
int kmr_normalize_read_batch_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, const int64_t *read1, const int64_t *read2, uint64_t n_pairs,
                                 const uint8_t *af_action, const uint32_t *af_min_pass, const uint32_t *af_max_pass, const uint64_t *input_starts, uint32_t n_inputs,
                                 const kmr_normalize_config *cfg, kmr_picks **out) {
	SelectCall c = {};
	c.who = "kmr_normalize_read_batch_dev"; c.fused = true; c.r = reads; c.text = dev_text; c.text_len = text_len; c.text_on_device = true; c.read1 = read1; c.read2 = read2; c.n_pairs = n_pairs;
	c.af_action = af_action; c.af_min = af_min_pass; c.af_max = af_max_pass; c.input_starts = input_starts; c.n_inputs = n_inputs;
	return select_normalized(h, c, cfg, out);
}
int kmr_normalize_info(const kmr_picks *p, uint64_t *n_picks, uint64_t *n_candidates, uint64_t *n_draws) {
	if (!p || !p->normalized) return KMR_ERR_INVALID_ARG;
	if (n_picks) *n_picks = p->norm_info[0]; if (n_candidates) *n_candidates = p->norm_info[1]; if (n_draws) *n_draws = p->norm_info[2];
	return KMR_OK;
}
int kmr_picks_segments_info(const kmr_picks *p, uint32_t *n_rounds, uint32_t *n_inputs) {
	if (!p) return KMR_ERR_INVALID_ARG;
	if (n_rounds) *n_rounds = p->n_rounds; if (n_inputs) *n_inputs = p->n_inputs;
	return KMR_OK;
}
int kmr_picks_segments_copy(const kmr_picks *p, float *round_depth, uint8_t *round_is_remainder, uint64_t *seg_first_pick, uint64_t *seg_picks, uint64_t *seg_first_byte,
                            uint64_t *seg_bytes, int32_t *read_segment) {
	if (!p) return KMR_ERR_INVALID_ARG;
	for (uint32_t r = 0; r < p->n_rounds; r++) { if (round_depth) round_depth[r] = p->round_depth[r]; if (round_is_remainder) round_is_remainder[r] = p->round_is_remainder[r]; }
	const uint64_t *t = p->seg_table.data();
	for (size_t s = 0; s < p->seg_table.size() / 4; s++) {
		if (seg_first_pick) seg_first_pick[s] = t[4 * s]; if (seg_picks) seg_picks[s] = t[4 * s + 1];
		if (seg_first_byte) seg_first_byte[s] = t[4 * s + 2]; if (seg_bytes) seg_bytes[s] = t[4 * s + 3];
	}
	if (!read_segment || !p->n) return KMR_OK;
	hipSetDevice(p->device);
	hipError_t e = hipSuccess;
	if (p->read_seg) copy_out(e, read_segment, p->read_seg, p->n);
	else {
		std::vector<uint8_t> flags(p->n, 0);
		if (p->picked) copy_out(e, flags.data(), p->picked, p->n);
		for (uint64_t i = 0; i < p->n; i++) read_segment[i] = flags[i] ? 0 : -1;
	}
	return e == hipSuccess ? KMR_OK : KMR_ERR_HIP;
}
int kmr_picks_info(const kmr_picks *p, uint64_t *n_picked, uint64_t *bytes) {
	if (!p) return KMR_ERR_INVALID_ARG;
	if (n_picked) *n_picked = p->n_picked; if (bytes) *bytes = p->bytes;
	return KMR_OK;
}
int kmr_picks_copy(const kmr_picks *p, char *dst, uint64_t capacity, uint8_t *picked_flags) {
	if (!p || (p->bytes && !dst)) return KMR_ERR_INVALID_ARG;
	if (capacity < p->bytes) return KMR_ERR_CAPACITY;
	hipSetDevice(p->device);
	hipError_t e = hipSuccess;
	copy_out(e, (uint8_t *)dst, p->text, p->bytes); copy_out(e, picked_flags, p->picked, p->n);
	return e == hipSuccess ? KMR_OK : KMR_ERR_HIP;
}
int kmr_picks_device_ptr(const kmr_picks *p, void **dev_text) {
	if (!p || !dev_text) return KMR_ERR_INVALID_ARG;
	*dev_text = p->text.get<uint8_t>();
	return KMR_OK;
}
void kmr_picks_free(kmr_picks *p) { free_on_device(p); }

/* ---- the artifact filter's report (kmr_artifact_report.hpp) ---------------- */
}  // extern "C"

struct kmr_artifact_report : OnDevice {
	kmr_picks picks;                      /* the records; segment = row * n_inputs + input, row 0 Artifact, row 1 PhiX */
	uint32_t n_seq = 0;
	std::vector<uint64_t> counts;         /* [3][n_seq + 1]: discarded, trimmed, bases */
};

extern "C" {

int kmr_artifact_report_config_init(kmr_artifact_report_config *c) {
	if (!c) return KMR_ERR_INVALID_ARG;
	memset(c, 0, sizeof(*c));
	c->struct_size = (uint32_t)sizeof(kmr_artifact_report_config);
	c->artifact_output = 1; c->phix_output = 1;      /* --filter-output, --phix-output */
	c->output_quality_base = 33;                     /* --fastq-output-base-quality */
	c->print_bases = 0;                              /* N, as the reference writes it */
	return KMR_OK;
}

/* What one of the four reporting entry points was called with.  Every array but a text that lies on the device is the host's. */
struct ReportCall {
	const char *who;
	const kmr_artifact_filter *f; const kmr_reads *in;
	const void *text; uint64_t text_len; bool text_on_device;
	const int64_t *read1, *read2; uint64_t n_pairs;
	const uint64_t *input_starts; uint32_t n_inputs;
	const kmr_artifact_report_config *cfg;
};

/* everything that needs no device; makes n_inputs 1 for no input_starts */
static int report_check(kmr_handle *h, ReportCall &c, kmr_artifact_report **report) {
	const std::string who = c.who;
	if (report) *report = nullptr;
	if (!c.cfg) return fail(h, KMR_ERR_INVALID_ARG, "kmr_artifact_report_config: NULL");
	if (c.cfg->struct_size != sizeof(kmr_artifact_report_config))
		return fail(h, KMR_ERR_INVALID_ARG, "kmr_artifact_report_config: struct_size " + std::to_string(c.cfg->struct_size) + " is not " + std::to_string(sizeof(kmr_artifact_report_config)));
	if (c.cfg->output_quality_base != 33 && c.cfg->output_quality_base != 64) return fail(h, KMR_ERR_INVALID_ARG, "kmr_artifact_report_config: output_quality_base must be 33 or 64");
	if (!h) return fail(h, KMR_ERR_INVALID_ARG, who + ": NULL handle");
	if (!c.f || !c.in || !report || (c.text_len && !c.text)) return fail(h, KMR_ERR_INVALID_ARG, who + ": NULL argument");
	if (c.f->device != h->device || c.in->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "filter, reads and handle must live on one device");
	if (c.cfg->phix_output && c.f->cfg.phix_idx == 0) return fail(h, KMR_ERR_INVALID_ARG, who + ": phix_output with a filter whose phix_idx is 0");
	if ((c.read1 != nullptr) != (c.read2 != nullptr)) return fail(h, KMR_ERR_INVALID_ARG, "the pair list: read1 and read2 go together");
	const uint64_t n = c.in->n;
	if (n >= 0xffffffffull) return fail(h, KMR_ERR_UNSUPPORTED, who + ": a batch holds fewer than 2^32 - 1 reads (pick indices are 32-bit)");
	if (c.read1 && c.n_pairs && !n) return fail(h, KMR_ERR_INVALID_ARG, who + ": a pair list for an empty batch");
	if (c.read1 && !c.n_pairs && n) return fail(h, KMR_ERR_INVALID_ARG, "the pair list leaves a read out (it is empty)");
	if (c.input_starts) {
		if (c.n_inputs == 0) return fail(h, KMR_ERR_INVALID_ARG, "input_starts without n_inputs");
		bool ok;
		const uint32_t at = sel_check_input_starts(c.input_starts, c.n_inputs, &ok);
		if (!ok) return fail(h, KMR_ERR_INVALID_ARG, "input_starts[" + std::to_string(at) + "]: the read indices start at 0 and ascend");
		if (c.input_starts[c.n_inputs] != n) return fail(h, KMR_ERR_INVALID_ARG, who + ": input_starts ends at " + std::to_string(c.input_starts[c.n_inputs]) + ", the batch holds " + std::to_string(n) + " reads");
	} else if (c.n_inputs > 1) return fail(h, KMR_ERR_INVALID_ARG, "input_starts is NULL for " + std::to_string(c.n_inputs) + " inputs");
	else c.n_inputs = 1;
	if (2ull * c.n_inputs > (uint64_t)SEL_MAX_SEGMENTS) return fail(h, KMR_ERR_UNSUPPORTED, who + ": more than " + std::to_string(SEL_MAX_SEGMENTS / 2) + " inputs");
	return 0;
}

/* the pair list and the input boundaries of a checked call in device memory (null for none) */
static int report_args(kmr_handle *h, Scratch &tmp, const ReportCall &c, const uint8_t **dtext, const int64_t **dr1, const int64_t **dr2, const uint64_t **dstarts) {
	int rc = to_device(h, tmp, (const uint8_t *)c.text, c.text_len, dtext, c.text_on_device); if (rc) return rc;
	rc = to_device(h, tmp, c.read1, c.n_pairs, dr1); if (rc) return rc;
	rc = to_device(h, tmp, c.read2, c.n_pairs, dr2); if (rc) return rc;
	return to_device(h, tmp, c.n_inputs > 1 ? c.input_starts : nullptr, (uint64_t)c.n_inputs + 1, dstarts);
}

/* A checked call from the decisions in device memory on: the pair list's check, the classification with the counters, the stable
 * partition by (row, input) and the writer.  One wait, for the totals. */
static int report_core(kmr_handle *h, Scratch &tmp, const ReportCall &c, const uint8_t *dtext, const int64_t *dr1, const int64_t *dr2, const uint64_t *dstarts, const ArtDecisions &D,
                       kmr_artifact_report *rep) {
	const kmr_artifact_filter *f = c.f; const kmr_reads *in = c.in;
	const uint64_t n = in->n, n_pairs = c.read1 ? c.n_pairs : 0;
	const uint32_t rows = f->n_seq + 1;
	rep->n_seq = f->n_seq; rep->counts.assign((size_t)3 * rows, 0);
	rep->picks.device = h->device;
	ArtReportParams A;
	A.bases = in->bases.get<uint8_t>(); A.quals = in->quals.get<uint8_t>(); A.offsets = in->offsets.get<uint64_t>(); A.name_off = in->name_off.get<uint64_t>(); A.name_len = in->name_len.get<uint32_t>();
	A.text = dtext; A.text_len = c.text_len; A.n = n; A.read1 = c.read1 ? dr1 : nullptr; A.read2 = c.read1 ? dr2 : nullptr; A.n_pairs = n_pairs;
	A.value = D.value; A.min_pass = D.min_pass; A.max_pass = D.max_pass; A.action = D.action;
	A.label_bytes = f->d_label_bytes.get<uint8_t>(); A.label_off = f->d_label_off.get<uint64_t>();
	A.n_seq = f->n_seq; A.phix = f->cfg.phix_idx; A.artifact_output = c.cfg->artifact_output ? 1u : 0u; A.phix_output = c.cfg->phix_output ? 1u : 0u; A.print_bases = c.cfg->print_bases ? 1u : 0u;
	A.out_base = c.cfg->output_quality_base; A.qual_shift = (int32_t)c.cfg->output_quality_base - (int32_t)h->cfg.fastq_start_char;
	const size_t ctr_bytes = (size_t)24 * rows;
	const bool lds = h->tune.artifact_report_lds < 0 ? ctr_bytes <= ART_REPORT_LDS_CAP : (h->tune.artifact_report_lds == 1 && ctr_bytes <= ART_REPORT_LDS_MOST);
	h->last_artifact_report_lds = lds ? 1 : 0;
	uint32_t *named = nullptr, *read_label = nullptr;
	if (n) { HIPCHK(h, tmp.take(&read_label, n)); if (A.read1) HIPCHK(h, tmp.take(&named, n)); }
	SelRounds R = {}; R.n = 2;
	const bool slots = A.read1 != nullptr;
	return partition_run(h, tmp, n, slots ? 2 * n_pairs : n, R, c.n_inputs, 2 * c.n_inputs, dstarts, slots, true, rep->counts.data(), rep->counts.size(), &rep->picks,
		[&](const PartitionWork &W) -> int {
			HIPCHK(h, hipMemsetAsync(W.item_seg, 0xff, 4 * W.n_items, h->stream)); HIPCHK(h, hipMemsetAsync(W.read_seg, 0xff, 4 * n, h->stream)); HIPCHK(h, hipMemsetAsync(W.picked, 0, n, h->stream));
			if (slots) {
				NormalizeParams N = {}; N.read1 = dr1; N.read2 = dr2; N.n_pairs = n_pairs;
				HIPCHK(h, hipMemsetAsync(named, 0, 4 * n, h->stream));
				LAUNCH(h, normalize_mark_kernel, dim3(grid_for(n_pairs)), dim3(256), 0, N, n, named, W.err);
				LAUNCH(h, artifact_pairs_kernel, dim3(grid_for(n)), dim3(256), 0, (const uint32_t *)named, n, W.err);
			}
			if (lds) LAUNCH(h, artifact_classify_kernel<true>, dim3(W.Q.n_units), dim3(SEL_UNIT), ctr_bytes, A, W.Q, W.n_items, W.slot_read, W.item_seg, W.item_len, W.name_printed, read_label,
			                W.picked, W.read_seg, W.unit_cnt, W.unit_bytes, W.extra, W.err);
			else LAUNCH(h, artifact_classify_kernel<false>, dim3(W.Q.n_units), dim3(SEL_UNIT), 0, A, W.Q, W.n_items, W.slot_read, W.item_seg, W.item_len, W.name_printed, read_label,
			            W.picked, W.read_seg, W.unit_cnt, W.unit_bytes, W.extra, W.err);
			return 0;
		},
		[&](const PartitionWork &W, const uint32_t *pread, const uint64_t *poff, kmr_picks *pk) -> int {
			LAUNCH(h, artifact_write_kernel, dim3((unsigned)std::min<uint64_t>((pk->n_picked + SEL_WAVES - 1) / SEL_WAVES, (uint64_t)num_cus(h) * 8)), dim3(SEL_THREADS), 0, A,
			                   (const uint32_t *)W.name_printed, (const uint32_t *)read_label, pread, poff, pk->n_picked, pk->text.get<uint8_t>());
			return 0;
		});
}

static int report_from_host(kmr_handle *h, ReportCall &c, const uint32_t *value, const uint8_t *action, const uint32_t *min_pass, const uint32_t *max_pass, kmr_artifact_report **report) {
	int rc = report_check(h, c, report); if (rc) return rc;
	const uint64_t n = c.in->n;
	if (n && (!value || !action || !min_pass || !max_pass)) return fail(h, KMR_ERR_INVALID_ARG, std::string(c.who) + ": NULL argument");
	hipSetDevice(h->device);
	auto rep = make_result<kmr_artifact_report>(h);
	Scratch tmp(h);
	const uint8_t *dtext; const int64_t *dr1, *dr2; const uint64_t *dstarts;
	rc = report_args(h, tmp, c, &dtext, &dr1, &dr2, &dstarts); if (rc) return rc;
	ArtDecisions D;
	rc = to_device(h, tmp, value, n, &D.value); if (rc) return rc;
	rc = to_device(h, tmp, min_pass, n, &D.min_pass); if (rc) return rc;
	rc = to_device(h, tmp, max_pass, n, &D.max_pass); if (rc) return rc;
	rc = to_device(h, tmp, action, n, &D.action); if (rc) return rc;
	rc = report_core(h, tmp, c, dtext, dr1, dr2, dstarts, D, rep.get());
	if (!rc) *report = rep.release();
	return rc;
}

/* the fused form: mate from the pair list, the apply step, the report from its decisions */
static int report_fused(kmr_handle *h, ReportCall &c, uint32_t *value, uint32_t *min_pass, uint32_t *max_pass, uint8_t *action, uint32_t *remnant_off, uint32_t *remnant_len, kmr_reads **out,
                        kmr_artifact_report **report) {
	if (out) *out = nullptr;
	int rc = report_check(h, c, report); if (rc) return rc;
	const uint64_t n = c.in->n, n_pairs = c.read1 ? c.n_pairs : 0;
	hipSetDevice(h->device);
	auto rep = make_result<kmr_artifact_report>(h);
	Scratch tmp(h);
	const uint8_t *dtext; const int64_t *dr1, *dr2; const uint64_t *dstarts;
	rc = report_args(h, tmp, c, &dtext, &dr1, &dr2, &dstarts); if (rc) return rc;
	int64_t *dmate = nullptr;
	if (n_pairs) {
		HIPCHK(h, tmp.take(&dmate, n)); HIPCHK(h, hipMemsetAsync(dmate, 0xff, 8 * n, h->stream));
		LAUNCH(h, artifact_mate_kernel, dim3(grid_for(n_pairs)), dim3(256), 0, dr1, dr2, n_pairs, n, dmate);
	}
	ArtDecisions D;
	kmr_reads *made = nullptr;
	rc = art_apply_core(h, tmp, c.f, c.in, dmate, value, min_pass, max_pass, action, remnant_off, remnant_len, out ? &made : nullptr, &D); if (rc) return rc;
	rc = report_core(h, tmp, c, dtext, dr1, dr2, dstarts, D, rep.get());
	if (rc) { free_on_device(made); return rc; }
	if (out) *out = made;
	*report = rep.release();
	return KMR_OK;
}

int kmr_artifact_filter_report(kmr_handle *h, const kmr_artifact_filter *f, const kmr_reads *in, const char *text, uint64_t text_len, const int64_t *read1, const int64_t *read2, uint64_t n_pairs,
                               const uint32_t *value, const uint8_t *action, const uint32_t *min_pass, const uint32_t *max_pass, const uint64_t *input_starts, uint32_t n_inputs,
                               const kmr_artifact_report_config *cfg, kmr_artifact_report **report) {
	ReportCall c = {"kmr_artifact_filter_report", f, in, text, text_len, false, read1, read2, n_pairs, input_starts, n_inputs, cfg};
	return report_from_host(h, c, value, action, min_pass, max_pass, report);
}
int kmr_artifact_filter_report_dev(kmr_handle *h, const kmr_artifact_filter *f, const kmr_reads *in, const void *dev_text, uint64_t text_len, const int64_t *read1, const int64_t *read2, uint64_t n_pairs,
                                   const uint32_t *value, const uint8_t *action, const uint32_t *min_pass, const uint32_t *max_pass, const uint64_t *input_starts, uint32_t n_inputs,
                                   const kmr_artifact_report_config *cfg, kmr_artifact_report **report) {
	ReportCall c = {"kmr_artifact_filter_report_dev", f, in, dev_text, text_len, true, read1, read2, n_pairs, input_starts, n_inputs, cfg};
	return report_from_host(h, c, value, action, min_pass, max_pass, report);
}
int kmr_artifact_filter_apply_report(kmr_handle *h, const kmr_artifact_filter *f, const kmr_reads *in, const char *text, uint64_t text_len, const int64_t *read1, const int64_t *read2, uint64_t n_pairs,
                                     uint32_t *value, uint32_t *min_pass, uint32_t *max_pass, uint8_t *action, uint32_t *remnant_off, uint32_t *remnant_len, kmr_reads **out,
                                     const uint64_t *input_starts, uint32_t n_inputs, const kmr_artifact_report_config *cfg, kmr_artifact_report **report) {
	ReportCall c = {"kmr_artifact_filter_apply_report", f, in, text, text_len, false, read1, read2, n_pairs, input_starts, n_inputs, cfg};
	return report_fused(h, c, value, min_pass, max_pass, action, remnant_off, remnant_len, out, report);
}
int kmr_artifact_filter_apply_report_dev(kmr_handle *h, const kmr_artifact_filter *f, const kmr_reads *in, const void *dev_text, uint64_t text_len, const int64_t *read1, const int64_t *read2,
                                         uint64_t n_pairs, uint32_t *value, uint32_t *min_pass, uint32_t *max_pass, uint8_t *action, uint32_t *remnant_off, uint32_t *remnant_len, kmr_reads **out,
                                         const uint64_t *input_starts, uint32_t n_inputs, const kmr_artifact_report_config *cfg, kmr_artifact_report **report) {
	ReportCall c = {"kmr_artifact_filter_apply_report_dev", f, in, dev_text, text_len, true, read1, read2, n_pairs, input_starts, n_inputs, cfg};
	return report_fused(h, c, value, min_pass, max_pass, action, remnant_off, remnant_len, out, report);
}
int kmr_artifact_report_counts(const kmr_artifact_report *report, uint64_t *discarded, uint64_t *trimmed, uint64_t *bases, uint64_t capacity) {
	if (!report) return KMR_ERR_INVALID_ARG;
	const size_t rows = (size_t)report->n_seq + 1;
	if (capacity < rows) return KMR_ERR_CAPACITY;
	const uint64_t *c = report->counts.data();
	if (discarded) memcpy(discarded, c, 8 * rows); if (trimmed) memcpy(trimmed, c + rows, 8 * rows); if (bases) memcpy(bases, c + 2 * rows, 8 * rows);
	return KMR_OK;
}
int kmr_artifact_report_picks(const kmr_artifact_report *report, const kmr_picks **picks) {
	if (!report || !picks) return KMR_ERR_INVALID_ARG;
	*picks = &report->picks;
	return KMR_OK;
}
void kmr_artifact_report_free(kmr_artifact_report *report) { free_on_device(report); }

/* ---- ReadSet::identifyPairs on the device (kmr_pairs.hpp) ---------------- */
/* dtext: device memory */
static int pairs_core(kmr_handle *h, Scratch &tmp, const kmr_reads *r, const uint8_t *dtext, uint64_t text_len, int store_comment, kmr_pairs *pr) {
	const uint64_t n = r->n;
	pr->n = n;
	h->last_pairs_ms = h->last_pairs_parse_ms = h->last_pairs_sort_ms = 0; h->last_pair_hash_collisions = 0;
	if (n == 0) return KMR_OK;
	PairsParams P;
	P.name_off = r->name_off.get<uint64_t>(); P.name_len = r->name_len.get<uint32_t>(); P.text = dtext; P.text_len = text_len; P.n = n; P.store_comment = store_comment ? 1u : 0u;
	const dim3 grid(grid_for(n)), block(256);
	uint64_t *hash, *bscan, *sscan, *uscan, *tot; uint32_t *cn, *brk, *run, *sec, *unp; uint8_t *fl, *link; int64_t *mate;
	HIPCHK(h, tmp.take(&hash, n)); HIPCHK(h, tmp.take(&cn, n)); HIPCHK(h, tmp.take(&fl, n)); HIPCHK(h, tmp.take(&tot, (size_t)PAIRS_T_WORDS));
	HIPCHK(h, alloc_n(pr->mate, &mate, n));
	EventTimer<5> timer(h->tune.pairs_timing);
	timer.mark(0, h->stream);
	HIPCHK(h, hipMemsetAsync(tot, 0, 8 * PAIRS_T_WORDS, h->stream));
	LAUNCH(h, pairs_parse_kernel, grid, block, 0, P, hash, cn, fl, tot);
	timer.mark(1, h->stream);
	uint64_t totals[PAIRS_T_WORDS] = {0};
	if (text_len == 0) {      /* no names (kmr_reads_from_host, kmr_reads_from_twobit): every read is a half pair of its own */
		int64_t *r1, *r2;
		HIPCHK(h, alloc_n(pr->read1, &r1, n)); HIPCHK(h, alloc_n(pr->read2, &r2, n));
		LAUNCH(h, pairs_single_kernel, grid, block, 0, n, mate, r1, r2);
		HIPCHK(h, fetch(h, totals, tot, PAIRS_T_WORDS));
		if (totals[PAIRS_T_ERR] & PAIRS_ERR_NAME) return fail(h, KMR_ERR_INVALID_ARG, NAME_SPAN_ERROR);
		pr->n_pairs = n;
		tmp.done();
		return KMR_OK;
	}
	const PairsNames N = {hash, cn, fl};
	/* phase 1 */
	HIPCHK(h, tmp.take(&link, n)); HIPCHK(h, tmp.take(&brk, n)); HIPCHK(h, tmp.take(&bscan, n + 1)); HIPCHK(h, tmp.take(&run, n + 1));
	HIPCHK(h, tmp.take(&sec, n)); HIPCHK(h, tmp.take(&unp, n)); HIPCHK(h, tmp.take(&sscan, n + 1)); HIPCHK(h, tmp.take(&uscan, n + 1));
	LAUNCH(h, pairs_link_kernel, grid, block, 0, P, N, link, brk);
	int rc = exclusive_scan(h, brk, n, bscan); if (rc) return rc;
	LAUNCH(h, pairs_runstart_kernel, grid, block, 0, (const uint8_t *)link, (const uint64_t *)bscan, n, run);
	LAUNCH(h, pairs_seq_kernel, grid, block, 0, (const uint8_t *)link, (const uint64_t *)bscan, (const uint32_t *)run, n, sec, unp, mate);
	rc = exclusive_scan(h, sec, n, sscan); if (rc) return rc;
	rc = exclusive_scan(h, unp, n, uscan); if (rc) return rc;
	/* the first of the call's two fixed-size copies: phase 1's totals size phase 2 (an interleaved file leaves it nothing) */
	HIPCHK(h, fetch_queue(h, &totals[PAIRS_T_SEQ], sscan + n));
	HIPCHK(h, fetch_queue(h, &totals[PAIRS_T_UNPAIRED], uscan + n));
	HIPCHK(h, fetch_queue(h, &totals[PAIRS_T_ERR], tot + PAIRS_T_ERR));
	HIPCHK(h, stream_wait(h));
	if (totals[PAIRS_T_ERR] & PAIRS_ERR_NAME) return fail(h, KMR_ERR_INVALID_ARG, NAME_SPAN_ERROR);
	const uint64_t n_seq = totals[PAIRS_T_SEQ], m = totals[PAIRS_T_UNPAIRED];
	/* phase 2 */
	unsigned long long *kin, *kout; uint32_t *vin, *vout, *push = nullptr; uint8_t *side = nullptr; uint64_t *pscan = nullptr;
	timer.mark(2, h->stream); timer.mark(3, h->stream);
	if (m) {
		HIPCHK(h, tmp.take(&kin, m)); HIPCHK(h, tmp.take(&kout, m)); HIPCHK(h, tmp.take(&vin, m)); HIPCHK(h, tmp.take(&vout, m));
		HIPCHK(h, tmp.take(&push, n)); HIPCHK(h, tmp.take(&side, n)); HIPCHK(h, tmp.take(&pscan, n + 1));
		const uint32_t bits = h->tune.pair_hash_bits;
		LAUNCH(h, pairs_keys_kernel, grid, block, 0, (const uint32_t *)unp, (const uint64_t *)uscan, (const uint64_t *)hash, bits >= 64 ? ~0ull : (1ull << bits) - 1, n, kin, vin);
		HIPCHK(h, hipMemsetAsync(push, 0, 4 * n, h->stream)); HIPCHK(h, hipMemsetAsync(side, 0, n, h->stream));
		rc = sort_reserve(h, tmp.sort, m, "kmr_identify_pairs"); if (rc) return rc;
		timer.mark(2, h->stream);
		rc = sort_pairs(h, tmp.sort, kin, kout, vin, vout, m, "kmr_identify_pairs"); if (rc) return rc;
		timer.mark(3, h->stream);
		LAUNCH(h, pairs_group_kernel, dim3(grid_for(m)), block, 0, P, N, (const unsigned long long *)kout, (const uint32_t *)vout, m, mate, push, side, tot);
		rc = exclusive_scan(h, push, n, pscan); if (rc) return rc;
		/* the second: what phase 2 made */
		HIPCHK(h, fetch_queue(h, &totals[PAIRS_T_PUSHED], pscan + n));
		HIPCHK(h, fetch_queue(h, &totals[PAIRS_T_FULL2], tot + PAIRS_T_FULL2, PAIRS_T_WORDS - PAIRS_T_FULL2));
		HIPCHK(h, stream_wait(h));
	}
	pr->n_seq = n_seq; pr->n_pairs = n_seq + totals[PAIRS_T_PUSHED]; pr->n_full = n_seq + totals[PAIRS_T_FULL2];
	pr->n_conflicts = totals[PAIRS_T_CONFLICT1] + totals[PAIRS_T_CONFLICT2];
	h->last_pair_hash_collisions = totals[PAIRS_T_COLLISIONS];
	int64_t *r1, *r2;
	HIPCHK(h, alloc_n(pr->read1, &r1, pr->n_pairs)); HIPCHK(h, alloc_n(pr->read2, &r2, pr->n_pairs));
	LAUNCH(h, pairs_scatter_kernel, grid, block, 0, (const uint32_t *)sec, (const uint64_t *)sscan, (const uint32_t *)push, (const uint64_t *)pscan, (const uint8_t *)side, (const int64_t *)mate,
	       n, n_seq, r1, r2);
	timer.mark(4, h->stream);
	HIPCHK(h, hipStreamSynchronize(h->stream));
	tmp.done();
	h->last_pairs_ms = timer.ms(0, 4); h->last_pairs_parse_ms = timer.ms(0, 1); h->last_pairs_sort_ms = m ? timer.ms(2, 3) : 0.0;
	return KMR_OK;
}

static int identify_pairs_any(kmr_handle *h, const kmr_reads *r, const void *text, uint64_t text_len, bool text_on_device, int store_comment, kmr_pairs **out) {
	if (!h || !r || !out || (text_len && !text)) return KMR_ERR_INVALID_ARG;
	*out = nullptr;
	if (r->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "read batch lives on another device");
	if (r->n >= 0xffffffffull) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_identify_pairs: a batch holds fewer than 2^32 - 1 reads (read indices of the sort are 32-bit)");
	hipSetDevice(h->device);
	auto pr = make_result<kmr_pairs>(h);
	Scratch tmp(h);
	const uint8_t *dtext;
	int rc = to_device(h, tmp, (const uint8_t *)text, r->n ? text_len : 0, &dtext, text_on_device); if (rc) return rc;
	rc = pairs_core(h, tmp, r, dtext, text_len, store_comment, pr.get());
	if (!rc) *out = pr.release();
	return rc;
}
int kmr_identify_pairs(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, int store_comment, kmr_pairs **out) {
	return identify_pairs_any(h, reads, text, text_len, false, store_comment, out);
}
int kmr_identify_pairs_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, int store_comment, kmr_pairs **out) {
	return identify_pairs_any(h, reads, dev_text, text_len, true, store_comment, out);
}
int kmr_pairs_info(const kmr_pairs *p, uint64_t *n_reads, uint64_t *n_pairs, uint64_t *n_full, uint64_t *n_sequential, uint64_t *n_conflicts, int *has_pairs) {
	if (!p) return KMR_ERR_INVALID_ARG;
	if (n_reads) *n_reads = p->n; if (n_pairs) *n_pairs = p->n_pairs; if (n_full) *n_full = p->n_full;
	if (n_sequential) *n_sequential = p->n_seq; if (n_conflicts) *n_conflicts = p->n_conflicts;
	if (has_pairs) *has_pairs = p->n_pairs > 0 && p->n_pairs < p->n;      /* ReadSet::hasPairs, src/ReadSet.h:526-529 */
	return KMR_OK;
}
int kmr_pairs_copy(const kmr_pairs *p, int64_t *mate, int64_t *read1, int64_t *read2) {
	if (!p) return KMR_ERR_INVALID_ARG;
	hipSetDevice(p->device);
	hipError_t e = hipSuccess;
	copy_out(e, mate, p->mate, p->n); copy_out(e, read1, p->read1, p->n_pairs); copy_out(e, read2, p->read2, p->n_pairs);
	return e == hipSuccess ? KMR_OK : KMR_ERR_HIP;
}
int kmr_pairs_device_ptrs(const kmr_pairs *p, void **dev_mate, void **dev_read1, void **dev_read2) {
	if (!p) return KMR_ERR_INVALID_ARG;
	if (dev_mate) *dev_mate = p->mate.get<int64_t>(); if (dev_read1) *dev_read1 = p->read1.get<int64_t>(); if (dev_read2) *dev_read2 = p->read2.get<int64_t>();
	return KMR_OK;
}
void kmr_pairs_free(kmr_pairs *p) { free_on_device(p); }

/* ---- DuplicateFragmentFilter on the device (kmr_dedup.hpp) ---------------- */
/* probToQual (src/Sequence.cpp:807-809) steps from i to i + 1 at dedup_qual_steps()[i]: the smallest double p with
 * (char)(-10. * log10(1.0 - p)) >= i + 1, found by bisection over the bit pattern (the expression is monotone below 0.9999) */
static char dedup_prob_to_qual(double prob) { return (char)(-10. * std::log10(1.0 - prob)); }
static const double *dedup_qual_steps() {
	static double step[DEDUP_QUALS];
	static std::once_flag once;
	std::call_once(once, [] {
		for (int i = 0; i < DEDUP_QUALS; i++) {
			uint64_t lo = 0, hi; const double top = 0.9999;
			memcpy(&hi, &top, 8);
			if (dedup_prob_to_qual(top) < i + 1) { step[i] = top; continue; }      /* never reached: getQualChar answers 40 from there */
			while (hi - lo > 1) {
				const uint64_t mid = lo + (hi - lo) / 2; double p; memcpy(&p, &mid, 8);
				if (dedup_prob_to_qual(p) >= i + 1) hi = mid; else lo = mid;
			}
			memcpy(&step[i], &hi, 8);
		}
	});
	return step;
}
char kmr_consensus_qual(double prob) {
	if (prob >= 0.9999) return 40;
	const double *step = dedup_qual_steps();
	char q = 0;
	while (q < DEDUP_QUALS && step[(int)q] <= prob) q++;
	return q;
}

int kmr_dedup_config_init(kmr_dedup_config *c) {
	if (!c) return KMR_ERR_INVALID_ARG;
	memset(c, 0, sizeof(*c));
	c->struct_size = (uint32_t)sizeof(kmr_dedup_config);
	c->dedup_mode = 0; c->paired = 1; c->dedup_length = 24; c->start_offset = 0; c->edit_distance = 0; c->consensus = 1;      /* src/DuplicateFragmentFilter.h:60-61 */
	return KMR_OK;
}
static int dedup_check_config(kmr_handle *h, const kmr_dedup_config *c) {
	if (!c) return fail(h, KMR_ERR_INVALID_ARG, "kmr_dedup_config: NULL");
	if (c->struct_size != sizeof(kmr_dedup_config)) return fail(h, KMR_ERR_INVALID_ARG, "kmr_dedup_config: struct_size " + std::to_string(c->struct_size) + " is not " + std::to_string(sizeof(kmr_dedup_config)));
	if (c->dedup_mode > 2) return fail(h, KMR_ERR_INVALID_ARG, "kmr_dedup_config: dedup_mode must be 0 (off), 1 or 2");
	if (c->paired > 1) return fail(h, KMR_ERR_INVALID_ARG, "kmr_dedup_config: paired must be 0 or 1");
	if (c->dedup_length == 0 || c->dedup_length % 4 != 0 || c->start_offset % 4 != 0) return fail(h, KMR_ERR_INVALID_ARG, "kmr_dedup_config: dedup_length and start_offset must be multiples of 4, dedup_length not 0");
	if (c->edit_distance != 0) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_dedup_config: only dedup-edit-distance 0 is built");
	if (c->consensus == 0) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_dedup_config: only dedup-consensus 1 is built");
	if (2 * (uint64_t)c->dedup_length > 128) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_dedup_config: a key holds at most 128 bases (2 * dedup_length)");
	if ((uint64_t)c->start_offset + 2 * (uint64_t)c->dedup_length > 0x7fffffffull) return fail(h, KMR_ERR_INVALID_ARG, "kmr_dedup_config: start_offset is too large");
	return 0;
}

/* the handle's DedupTables, made by the first call */
static int dedup_tables(kmr_handle *h, const DedupTables **out) {
	if (!h->dedup_tab) {
		std::unique_ptr<DedupTables> t(new DedupTables);
		double P[256]; quality_table(P, h->cfg.min_quality_score, h->cfg.fastq_start_char);
		for (int q = 0; q < 256; q++) {      /* Read::getProbabilityBases (src/Sequence.cpp:573-576), ProbabilityBase::observe (:871) */
			double prob = P[q];
			/* the table is indexed by the byte a read holds, and from PRINT_REF_QUAL (103) on a byte means "no quality data" at either
			 * quality base (src/Sequence.cpp:535-536); quality_table counts from the Phred value, which is the same thing at base 33 only */
			if (q >= 103) prob = 1.0;
			if (prob < 0.2501) prob = 0.2501;
			t->prob[q] = prob; t->other[q] = (1.0 - prob) / 3.0;
		}
		memcpy(t->step, dedup_qual_steps(), sizeof(t->step));
		HIPCHK(h, h->dedup_tab.alloc(sizeof(DedupTables)));
		HIPCHK(h, hipMemcpy(h->dedup_tab.get(), t.get(), sizeof(DedupTables), hipMemcpyHostToDevice));
	}
	*out = h->dedup_tab.get<DedupTables>();
	return 0;
}

/* dtext and ddisc (may be null): device memory */
static int dedup_core(kmr_handle *h, Scratch &tmp, const kmr_reads *r, const uint8_t *dtext, uint64_t text_len, const kmr_pairs *pairs, const uint8_t *ddisc, const kmr_dedup_config *cfg, kmr_dedup *dd) {
	const uint64_t n = r->n, np = pairs->n_pairs;
	dd->n = n;
	h->last_dedup_ms = h->last_dedup_key_ms = h->last_dedup_sort_ms = h->last_dedup_consensus_ms = 0;
	const DedupTables *tables; int rc = dedup_tables(h, &tables); if (rc) return rc;
	uint8_t *disc;
	HIPCHK(h, alloc_n(dd->disc, &disc, n));
	EventTimer<7> timer(h->tune.dedup_timing);
	timer.mark(0, h->stream);
	if (n) { if (ddisc) HIPCHK(h, hipMemcpyAsync(disc, ddisc, n, hipMemcpyDeviceToDevice, h->stream)); else HIPCHK(h, hipMemsetAsync(disc, 0, n, h->stream)); }
	DedupParams P;
	P.bases = r->bases.get<uint8_t>(); P.quals = r->quals.get<uint8_t>(); P.offsets = r->offsets.get<uint64_t>(); P.name_off = r->name_off.get<uint64_t>(); P.name_len = r->name_len.get<uint32_t>();
	P.text = dtext; P.text_len = text_len; P.n = n; P.total = r->total; P.read1 = pairs->read1.get<int64_t>(); P.read2 = pairs->read2.get<int64_t>(); P.np = np; P.discarded = ddisc;
	P.paired = cfg->paired ? 1u : 0u; P.mode2 = cfg->dedup_mode == 2 ? 1u : 0u; P.L = cfg->paired ? cfg->dedup_length : 2 * cfg->dedup_length; P.so = cfg->start_offset;
	P.W = (cfg->dedup_length / 2 + 7) / 8; P.sides = cfg->paired ? 2u : 1u;
	P.min_q = h->cfg.fastq_start_char + h->cfg.min_quality_score; P.start_char = h->cfg.fastq_start_char;
	const dim3 block(256);
	uint64_t totals[DEDUP_T_WORDS] = {0}, c = 0, K = 0;
	unsigned long long *keys, *first, *first2; uint32_t *cand, *order, *head, *keep = nullptr, *grp, *grp2; const uint32_t *perm = nullptr; uint8_t *flip = nullptr; uint64_t *cscan, *tot, *hscan = nullptr, *start = nullptr, *kscan;
	HIPCHK(h, tmp.take(&tot, (size_t)DEDUP_T_WORDS));
	HIPCHK(h, hipMemsetAsync(tot, 0, 8 * DEDUP_T_WORDS, h->stream));
	if (n && np && cfg->dedup_mode) {
		/* candidates and their keys */
		HIPCHK(h, tmp.take(&keys, (size_t)P.W * np)); HIPCHK(h, tmp.take(&cand, np)); HIPCHK(h, tmp.take(&flip, np)); HIPCHK(h, tmp.take(&cscan, np + 1));
		LAUNCH(h, dedup_key_kernel, dim3(grid_for(np)), block, 0, P, keys, cand, flip, tot);
		timer.mark(1, h->stream);
		rc = exclusive_scan(h, cand, np, cscan); if (rc) return rc;
		/* the first of the call's three fixed-size copies: the number of candidates sizes the sorts */
		HIPCHK(h, fetch_queue(h, &c, cscan + np));
		HIPCHK(h, fetch_queue(h, totals, tot, DEDUP_T_AFFECTED));
		HIPCHK(h, stream_wait(h));
	} else timer.mark(1, h->stream);
	for (int i = 0; i < 4; i++) dd->skipped[i] = totals[i];
	timer.mark(2, h->stream);
	if (c >= 2) {
		const dim3 cgrid(grid_for(c));
		HIPCHK(h, tmp.take(&order, c));
		LAUNCH(h, dedup_compact_kernel, dim3(grid_for(np)), block, 0, (const uint32_t *)cand, (const uint64_t *)cscan, np, order);
		/* least significant word first; the sort is stable, so equal keys keep ascending pair position */
		SortColumn cols[4];      /* a key holds at most 128 bases (kmr_dedup_config_check) */
		if (P.W > 4) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_dedup_fragments: a key of more than 4 words");
		for (uint32_t w = 0; w < P.W; w++) cols[w] = SortColumn{(const uint64_t *)keys + (size_t)(P.W - 1 - w) * np, 1, nullptr, nullptr};
		rc = sort_by_columns(h, tmp.sort, cols, (int)P.W, order, c, "kmr_dedup_fragments", &perm, nullptr); if (rc) return rc;
		timer.mark(3, h->stream);
		/* groups, and those of two members and more */
		HIPCHK(h, tmp.take(&head, c)); HIPCHK(h, tmp.take(&hscan, c + 1)); HIPCHK(h, tmp.take(&start, c + 1));
		HIPCHK(h, tmp.take(&keep, c)); HIPCHK(h, tmp.take(&kscan, c + 1)); HIPCHK(h, tmp.take(&first, c)); HIPCHK(h, tmp.take(&grp, c));
		LAUNCH(h, dedup_heads_kernel, cgrid, block, 0, (const unsigned long long *)keys, np, P.W, (const uint32_t *)perm, c, head);
		rc = exclusive_scan(h, head, c, hscan); if (rc) return rc;
		rc = group_starts(h, head, hscan, c, start); if (rc) return rc;
		LAUNCH(h, dedup_keep_kernel, cgrid, block, 0, (const uint64_t *)hscan, (const uint64_t *)start, c, keep);
		rc = exclusive_scan(h, keep, c, kscan); if (rc) return rc;
		LAUNCH(h, dedup_kept_kernel, cgrid, block, 0, (const uint32_t *)keep, (const uint64_t *)kscan, (const uint64_t *)start, (const uint32_t *)perm, c, first, grp);
		/* the second: the number of groups sizes everything behind */
		HIPCHK(h, fetch(h, &K, kscan + c));
	} else timer.mark(3, h->stream);
	/* the consensus batch (empty if nothing was collapsed) */
	const uint64_t n_new = K * P.sides;
	if (n_new >= 0xffffffffull) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_dedup_fragments: more than 2^32 - 2 consensus reads");
	dd->cons = new kmr_reads;
	kmr_reads *cr = dd->cons;
	cr->device = h->device; cr->n = n_new; cr->input_base = h->cfg.fastq_start_char;
	uint64_t *coff, *cno, *gfirst; uint32_t *cnl, *gsize;
	HIPCHK(h, alloc_n(cr->offsets, &coff, n_new + 1)); HIPCHK(h, alloc_n(cr->name_off, &cno, std::max<uint64_t>(n_new, 1))); HIPCHK(h, alloc_n(cr->name_len, &cnl, std::max<uint64_t>(n_new, 1)));
	HIPCHK(h, alloc_n(dd->group_first, &gfirst, std::max<uint64_t>(K, 1))); HIPCHK(h, alloc_n(dd->group_size, &gsize, std::max<uint64_t>(K, 1)));
	uint64_t name_total = 0;
	timer.mark(4, h->stream);
	if (K) {
		/* output order: ascending position of the first member */
		HIPCHK(h, tmp.take(&first2, K)); HIPCHK(h, tmp.take(&grp2, K));
		rc = sort_reserve(h, tmp.sort, K, "kmr_dedup_fragments"); if (rc) return rc;
		rc = sort_pairs(h, tmp.sort, first, first2, grp, grp2, K, "kmr_dedup_fragments"); if (rc) return rc;
		DedupGroups G; G.perm = perm; G.flip = flip; G.start = start; G.ogroup = grp2; G.K = K;
		uint32_t *len, *nb; uint64_t *nscan; DedupMember *members;
		HIPCHK(h, tmp.take(&len, n_new)); HIPCHK(h, tmp.take(&nb, n_new)); HIPCHK(h, tmp.take(&nscan, n_new + 1)); HIPCHK(h, tmp.take(&members, (size_t)c * P.sides));
		LAUNCH(h, dedup_size_kernel, dim3(grid_for(n_new)), block, 0, P, G, len, nb, gfirst, gsize, tot);
		rc = exclusive_scan(h, len, n_new, coff); if (rc) return rc;
		rc = exclusive_scan(h, nb, n_new, nscan); if (rc) return rc;
		/* the third: the bases and name bytes of the batch, what was collapsed, the error word */
		HIPCHK(h, fetch_queue(h, &cr->total, coff + n_new));
		HIPCHK(h, fetch_queue(h, &name_total, nscan + n_new));
		HIPCHK(h, fetch_queue(h, &totals[DEDUP_T_AFFECTED], tot + DEDUP_T_AFFECTED, 2));
		HIPCHK(h, stream_wait(h));
		if (totals[DEDUP_T_ERR] & DEDUP_ERR_NAME) return fail(h, KMR_ERR_INVALID_ARG, NAME_SPAN_ERROR);
		uint8_t *cb, *cq, *names;
		HIPCHK(h, alloc_n(cr->bases, &cb, cr->total + 64)); HIPCHK(h, alloc_n(cr->quals, &cq, cr->total + 64)); HIPCHK(h, alloc_n(dd->names, &names, name_total));
		HIPCHK(h, hipMemsetAsync(cb + cr->total, 0, 64, h->stream)); HIPCHK(h, hipMemsetAsync(cq + cr->total, 0, 64, h->stream));
		timer.mark(4, h->stream);
		LAUNCH(h, dedup_consensus_kernel, dim3((unsigned)std::min<uint64_t>((n_new + DEDUP_WAVES - 1) / DEDUP_WAVES, (uint64_t)num_cus(h) * 8)), dim3(DEDUP_THREADS), 0,
		       P, G, tables, (const uint64_t *)coff, (const uint64_t *)nscan, members, cb, cq, names, cno, cnl);
		timer.mark(5, h->stream);
		LAUNCH(h, dedup_discard_kernel, dim3(grid_for(c)), block, 0, P, (const uint32_t *)perm, (const uint64_t *)hscan, (const uint32_t *)keep, c, disc);
		timer.mark(6, h->stream);
		HIPCHK(h, hipStreamSynchronize(h->stream));      /* the temporaries above go */
	} else {
		uint8_t *cb, *cq;
		HIPCHK(h, alloc_n(cr->bases, &cb, (size_t)64)); HIPCHK(h, alloc_n(cr->quals, &cq, (size_t)64));
		HIPCHK(h, hipMemsetAsync(cb, 0, 64, h->stream)); HIPCHK(h, hipMemsetAsync(cq, 0, 64, h->stream)); HIPCHK(h, hipMemsetAsync(coff, 0, 8, h->stream));
		timer.mark(5, h->stream); timer.mark(6, h->stream);
		HIPCHK(h, hipStreamSynchronize(h->stream));
	}
	dd->n_groups = K; dd->affected = totals[DEDUP_T_AFFECTED]; dd->name_bytes = name_total;
	h->last_dedup_ms = timer.ms(0, 6); h->last_dedup_key_ms = timer.ms(0, 1); h->last_dedup_sort_ms = c >= 2 ? timer.ms(2, 3) : 0.0; h->last_dedup_consensus_ms = K ? timer.ms(4, 5) : 0.0;
	tmp.done();      /* (waited for above) */
	return KMR_OK;
}

static int dedup_any(kmr_handle *h, const kmr_reads *r, const void *text, uint64_t text_len, bool text_on_device, const kmr_pairs *pairs, const uint8_t *discarded, const kmr_dedup_config *cfg, kmr_dedup **out) {
	if (out) *out = nullptr;
	int rc = dedup_check_config(h, cfg); if (rc) return rc;
	if (!h || !r || !pairs || !out || (text_len && !text)) return fail(h, KMR_ERR_INVALID_ARG, "kmr_dedup_fragments: NULL argument");
	if (r->device != h->device || pairs->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "read batch or pair list lives on another device");
	if (pairs->n != r->n) return fail(h, KMR_ERR_INVALID_ARG, "kmr_dedup_fragments: the pair list belongs to a batch of " + std::to_string(pairs->n) + " reads, not " + std::to_string(r->n));
	if (r->n >= 0xffffffffull) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_dedup_fragments: a batch holds fewer than 2^32 - 1 reads (pair positions of the sort are 32-bit)");
	hipSetDevice(h->device);
	auto dd = make_result<kmr_dedup>(h);
	Scratch tmp(h);
	const uint8_t *dtext, *ddisc;
	rc = to_device(h, tmp, (const uint8_t *)text, r->n ? text_len : 0, &dtext, text_on_device); if (rc) return rc;
	rc = to_device(h, tmp, discarded, r->n, &ddisc); if (rc) return rc;
	rc = dedup_core(h, tmp, r, dtext, text_len, pairs, ddisc, cfg, dd.get());
	if (!rc) *out = dd.release();
	return rc;
}
int kmr_dedup_fragments(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, const kmr_pairs *pairs, const uint8_t *discarded, const kmr_dedup_config *cfg, kmr_dedup **out) {
	return dedup_any(h, reads, text, text_len, false, pairs, discarded, cfg, out);
}
int kmr_dedup_fragments_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, const kmr_pairs *pairs, const uint8_t *discarded, const kmr_dedup_config *cfg, kmr_dedup **out) {
	return dedup_any(h, reads, dev_text, text_len, true, pairs, discarded, cfg, out);
}
int kmr_dedup_info(const kmr_dedup *d, uint64_t *n_groups, uint64_t *n_new_reads, uint64_t *affected, uint64_t skipped[4]) {
	if (!d) return KMR_ERR_INVALID_ARG;
	if (n_groups) *n_groups = d->n_groups; if (n_new_reads) *n_new_reads = d->cons ? d->cons->n : 0; if (affected) *affected = d->affected;
	if (skipped) for (int i = 0; i < 4; i++) skipped[i] = d->skipped[i];
	return KMR_OK;
}
int kmr_dedup_copy(const kmr_dedup *d, uint8_t *discarded_out, uint64_t *group_first, uint32_t *group_size) {
	if (!d) return KMR_ERR_INVALID_ARG;
	hipSetDevice(d->device);
	hipError_t e = hipSuccess;
	copy_out(e, discarded_out, d->disc, d->n); copy_out(e, group_first, d->group_first, d->n_groups); copy_out(e, group_size, d->group_size, d->n_groups);
	return e == hipSuccess ? KMR_OK : KMR_ERR_HIP;
}
int kmr_dedup_device_ptrs(const kmr_dedup *d, void **dev_discarded, void **dev_group_first, void **dev_group_size) {
	if (!d) return KMR_ERR_INVALID_ARG;
	if (dev_discarded) *dev_discarded = d->disc.get<uint8_t>(); if (dev_group_first) *dev_group_first = d->group_first.get<uint64_t>(); if (dev_group_size) *dev_group_size = d->group_size.get<uint32_t>();
	return KMR_OK;
}
int kmr_dedup_reads(const kmr_dedup *d, const kmr_reads **consensus, const void **dev_name_text, uint64_t *name_text_len) {
	if (!d) return KMR_ERR_INVALID_ARG;
	if (consensus) *consensus = d->cons; if (dev_name_text) *dev_name_text = d->names.get<uint8_t>(); if (name_text_len) *name_text_len = d->name_bytes;
	return KMR_OK;
}
int kmr_dedup_names_copy(const kmr_dedup *d, char *dst, uint64_t capacity) {
	if (!d || (d->name_bytes && !dst)) return KMR_ERR_INVALID_ARG;
	if (capacity < d->name_bytes) return KMR_ERR_CAPACITY;
	hipSetDevice(d->device);
	if (d->name_bytes && hipMemcpy(dst, d->names.get<uint8_t>(), d->name_bytes, hipMemcpyDeviceToHost) != hipSuccess) return KMR_ERR_HIP;
	return KMR_OK;
}
void kmr_dedup_free(kmr_dedup *d) { free_on_device(d); }

/* ---- a14: the mercount / mergraph text on the device (kmr_dump.hpp) ---------- */
/* The common part of kmr_dump_text_size and kmr_dump_text: argument checks, the size pass over weak entries [lo, hi) and, when `out`
 * is given, the writer. */
static int dump_core(kmr_handle *h, int kind, uint32_t min_depth, uint64_t lo, uint64_t hi, uint64_t *kept, uint64_t *bytes, kmr_text **out) {
	if (out) *out = nullptr;
	if (!h) return KMR_ERR_INVALID_ARG;
	if (kind != KMR_DUMP_MERCOUNT && kind != KMR_DUMP_MERGRAPH) return fail(h, KMR_ERR_INVALID_ARG, "unknown kmr_dump_kind");
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "dump before kmr_finalize");
	const bool graph = kind == KMR_DUMP_MERGRAPH;
	if (graph && !h->ext) return fail(h, KMR_ERR_STATE, "mergraph needs value_kind = KMR_VALUE_EXT");
	const uint64_t n_map = h->weak.present ? h->weak.n : 0;
	if (hi > n_map) hi = n_map;
	if (lo > hi) return fail(h, KMR_ERR_INVALID_ARG, "dump: entry_lo lies behind entry_hi (entry_hi is clamped to the weak map's entries)");
	hipSetDevice(h->device);
	auto tx = make_result<kmr_text>(h);
	h->last_dump_size_ms = h->last_dump_write_ms = 0;
	const uint64_t n = hi - lo;
	if (n) {
		DumpParams P;
		P.keys = h->weak.keys.get<uint64_t>(); P.vals = h->weak.vals.get<uint32_t>(); P.vw = h->ext ? 15u : 3u; P.k = h->k; P.graph = graph ? 1u : 0u;
		P.min_depth = (int32_t)min_depth; P.lo = lo; P.n = n;
		Scratch tmp(h); uint32_t *len; uint64_t *off;      /* off[n] = bytes, off[n + 1] = kept entries */
		HIPCHK(h, tmp.take(&len, n)); HIPCHK(h, tmp.take(&off, n + 2));
		SelectTimer timer(h->tune.dump_timing);
		timer.mark(0, h->stream);
		HIPCHK(h, hipMemsetAsync(off + n + 1, 0, 8, h->stream));
		LAUNCH(h, dump_size_kernel, dim3(grid_for(n)), dim3(256), 0, P, len, (unsigned long long *)(off + n + 1));
		int rc = exclusive_scan(h, len, n, off); if (rc) return rc;
		uint64_t totals[2] = {0, 0};
		HIPCHK(h, fetch(h, totals, off + n, 2));      /* the one copy that brings sizes back */
		tx->bytes = totals[0]; tx->kept = totals[1];
		if (out && tx->bytes) HIPCHK(h, tx->text.alloc((tx->bytes + 15) & ~(uint64_t)15));
		timer.mark(1, h->stream);      /* (behind the allocation: the events then bracket the writer alone) */
		if (out && tx->bytes) {
			const uint64_t tiles = (tx->bytes + DUMP_TILE - 1) / DUMP_TILE;
			const uint64_t per_block = h->tune.dump_tiles_per_block ? h->tune.dump_tiles_per_block : (tiles + (uint64_t)num_cus(h) * 16 - 1) / ((uint64_t)num_cus(h) * 16);
			const unsigned blocks = (unsigned)((tiles + per_block - 1) / per_block);
			h->last_dump_tiles_per_block = per_block; h->last_dump_blocks = blocks;
			uint8_t *dout = tx->text.get<uint8_t>();
			{ int rc = with_w(h, [&](auto W) -> int { LAUNCH(h, dump_write_kernel<W()>, dim3(blocks), dim3(DUMP_THREADS), 0, P, (const uint64_t *)off, tx->bytes, per_block, dout); return 0; }); if (rc) return rc; }
		}
		timer.mark(2, h->stream);
		HIPCHK(h, hipStreamSynchronize(h->stream));
		tmp.done();
		h->last_dump_size_ms = timer.ms(0, 1); h->last_dump_write_ms = timer.ms(1, 2);
	}
	if (kept) *kept = tx->kept;
	if (bytes) *bytes = tx->bytes;
	if (out) *out = tx.release();
	return KMR_OK;
}

int kmr_dump_text_size(kmr_handle *h, int kind, uint32_t min_depth, uint64_t entry_lo, uint64_t entry_hi, uint64_t *kept, uint64_t *bytes) {
	if (!h || !kept || !bytes) return KMR_ERR_INVALID_ARG;
	return dump_core(h, kind, min_depth, entry_lo, entry_hi, kept, bytes, nullptr);
}
int kmr_dump_text(kmr_handle *h, int kind, uint32_t min_depth, uint64_t entry_lo, uint64_t entry_hi, kmr_text **out) {
	if (!h || !out) { if (out) *out = nullptr; return KMR_ERR_INVALID_ARG; }
	return dump_core(h, kind, min_depth, entry_lo, entry_hi, nullptr, nullptr, out);
}
int kmr_text_info(const kmr_text *t, uint64_t *kept, uint64_t *bytes) {
	if (!t) return KMR_ERR_INVALID_ARG;
	if (kept) *kept = t->kept; if (bytes) *bytes = t->bytes;
	return KMR_OK;
}
int kmr_text_copy(const kmr_text *t, char *dst, uint64_t capacity) {
	if (!t || (t->bytes && !dst)) return KMR_ERR_INVALID_ARG;
	if (capacity < t->bytes) return KMR_ERR_CAPACITY;
	hipSetDevice(t->device);
	return !t->bytes || hipMemcpy(dst, t->text.get<uint8_t>(), t->bytes, hipMemcpyDeviceToHost) == hipSuccess ? KMR_OK : KMR_ERR_HIP;
}
int kmr_text_device_ptr(const kmr_text *t, void **dev_text) {
	if (!t || !dev_text) return KMR_ERR_INVALID_ARG;
	*dev_text = t->text.get<uint8_t>();
	return KMR_OK;
}
void kmr_text_free(kmr_text *t) { free_on_device(t); }

/* The file-appending forms: the text in pieces of entries whose text stays under the staging bound whatever their numbers are (a
 * count has at most 5 digits, a tally at most 10), each copied to the host and appended. */
static int dump_file(kmr_handle *h, const char *path, uint32_t min_depth, bool graph) {
	if (!h || !path) return KMR_ERR_INVALID_ARG;
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "dump before kmr_finalize");
	if (graph && !h->ext) return fail(h, KMR_ERR_STATE, "mergraph needs value_kind = KMR_VALUE_EXT");
	const uint64_t n = h->weak.present ? h->weak.n : 0;
	const uint64_t bound = h->tune.dump_piece_bytes ? h->tune.dump_piece_bytes : (uint64_t)KMR_DUMP_PIECE_BYTES;
	const uint64_t entry_max = graph ? 2ull * (h->k + 15 + 12 * 10) : 2ull * (h->k + 2 + 5);
	const uint64_t step = std::max<uint64_t>(1, bound / entry_max);
	std::unique_ptr<FILE, int (*)(FILE *)> f(fopen(path, "a"), fclose);
	if (!f) return fail(h, KMR_ERR_INVALID_ARG, std::string("cannot open ") + path);
	std::vector<char> stage;
	for (uint64_t lo = 0; lo < n; lo += step) {
		kmr_text *t = nullptr;
		int rc = dump_core(h, graph ? KMR_DUMP_MERGRAPH : KMR_DUMP_MERCOUNT, min_depth, lo, std::min(n, lo + step), nullptr, nullptr, &t); if (rc) return rc;
		std::unique_ptr<kmr_text, void (*)(kmr_text *)> tx(t, kmr_text_free);
		if (!tx->bytes) continue;
		if (stage.size() < tx->bytes) stage.resize(tx->bytes);
		HIPCHK(h, hipMemcpy(stage.data(), tx->text.get<uint8_t>(), tx->bytes, hipMemcpyDeviceToHost));
		if (fwrite(stage.data(), 1, tx->bytes, f.get()) != tx->bytes) return fail(h, KMR_ERR_INVALID_ARG, std::string("cannot write ") + path);
	}
	return KMR_OK;
}
int kmr_dump_mercount(kmr_handle *h, const char *path, uint32_t min_depth) { return dump_file(h, path, min_depth, false); }
int kmr_dump_mergraph(kmr_handle *h, const char *path, uint32_t min_depth) { return dump_file(h, path, min_depth, true); }

/* ---- f2: the batch as 2-bit packed reads + markups -------------------------- */
int kmr_reads_twobit(kmr_handle *h, const kmr_reads *r, uint8_t *twobit, uint64_t twobit_capacity, uint64_t *twobit_offsets,
                     uint32_t *markup_pos, char *markup_char, uint64_t markup_capacity, uint64_t *markup_offsets,
                     uint64_t *twobit_bytes, uint64_t *n_markups) {
	if (!h || !r) return KMR_ERR_INVALID_ARG;
	if (r->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "read batch lives on another device");
	hipSetDevice(h->device);
	const uint64_t n = r->n;
	Scratch tmp(h); uint32_t *dlen, *dcnt; uint64_t *dtb, *dmk;
	HIPCHK(h, tmp.take(&dlen, n + 1)); HIPCHK(h, tmp.take(&dcnt, n + 1)); HIPCHK(h, tmp.take(&dtb, n + 1)); HIPCHK(h, tmp.take(&dmk, n + 1));
	uint64_t tb_total = 0, mk_total = 0;
	if (n) {
		LAUNCH(h, twobit_count_kernel, dim3(grid_for(n)), dim3(256), 0, r->bases.get<uint8_t>(), r->offsets.get<uint64_t>(), n, dlen, dcnt);
		int rc = exclusive_scan(h, dlen, n, dtb); if (rc) return rc;
		rc = exclusive_scan(h, dcnt, n, dmk); if (rc) return rc;
		HIPCHK(h, hipMemcpy(&tb_total, dtb + n, 8, hipMemcpyDeviceToHost)); HIPCHK(h, hipMemcpy(&mk_total, dmk + n, 8, hipMemcpyDeviceToHost));
	} else { HIPCHK(h, hipMemset(dtb, 0, 8)); HIPCHK(h, hipMemset(dmk, 0, 8)); }
	if (twobit_bytes) *twobit_bytes = tb_total; if (n_markups) *n_markups = mk_total;
	if (!twobit && !markup_pos && !markup_char && !twobit_offsets && !markup_offsets) return KMR_OK;      /* sizes only */
	if ((twobit && twobit_capacity < tb_total) || ((markup_pos || markup_char) && markup_capacity < mk_total)) return KMR_ERR_CAPACITY;
	uint8_t *dtw, *dmc; uint32_t *dmp;
	HIPCHK(h, tmp.take(&dtw, tb_total)); HIPCHK(h, tmp.take(&dmp, mk_total)); HIPCHK(h, tmp.take(&dmc, mk_total));
	if (n) {
		LAUNCH(h, twobit_pack_kernel, dim3(grid_for(n)), dim3(256), 0, r->bases.get<uint8_t>(), r->offsets.get<uint64_t>(), n, dtb, dmk, dtw, dmp, dmc);
	}
	HIPCHK(h, hipStreamSynchronize(h->stream));
	tmp.done();
	hipError_t e = hipSuccess;
	if (twobit && tb_total) e = hipMemcpy(twobit, dtw, tb_total, hipMemcpyDeviceToHost);
	if (e == hipSuccess && twobit_offsets) e = hipMemcpy(twobit_offsets, dtb, 8 * (n + 1), hipMemcpyDeviceToHost);
	if (e == hipSuccess && markup_pos && mk_total) e = hipMemcpy(markup_pos, dmp, 4 * mk_total, hipMemcpyDeviceToHost);
	if (e == hipSuccess && markup_char && mk_total) e = hipMemcpy(markup_char, dmc, mk_total, hipMemcpyDeviceToHost);
	if (e == hipSuccess && markup_offsets) e = hipMemcpy(markup_offsets, dmk, 8 * (n + 1), hipMemcpyDeviceToHost);
	HIPCHK(h, e);
	return KMR_OK;
}

int kmr_reads_from_twobit(kmr_handle *h, const uint8_t *twobit, const uint64_t *twobit_offsets, const uint64_t *offsets,
                          const uint64_t *markup_offsets, const uint32_t *markup_pos, const char *markup_char,
                          const char *quals, int uniform_quality, uint64_t n_reads, kmr_reads **out) {
	if (!h || !out || !offsets || !twobit_offsets || (n_reads && !twobit)) return KMR_ERR_INVALID_ARG;
	if (uniform_quality < 0 || uniform_quality > 255 || (quals && uniform_quality)) return fail(h, KMR_ERR_INVALID_ARG, "uniform_quality: 0, or the one quality character of a batch without a quality array");
	*out = nullptr;
	hipSetDevice(h->device);
	const uint64_t first = offsets[0], total = offsets[n_reads] - first, tbytes = twobit_offsets[n_reads] - twobit_offsets[0];
	const uint64_t nm = markup_offsets ? markup_offsets[n_reads] - markup_offsets[0] : 0;
	auto r = make_result<kmr_reads>(h);
	r->n = n_reads; r->total = total; r->input_base = h->cfg.fastq_start_char;
	HIPCHK(h, r->bases.alloc(total + 64)); HIPCHK(h, r->quals.alloc(total + 64));
	HIPCHK(h, r->offsets.alloc(8 * (n_reads + 1)));
	HIPCHK(h, r->name_off.alloc(8 * std::max<uint64_t>(n_reads, 1))); HIPCHK(h, r->name_len.alloc(4 * std::max<uint64_t>(n_reads, 1)));
	HIPCHK(h, hipMemset(r->bases.get<uint8_t>() + total, 0, 64)); HIPCHK(h, hipMemset(r->quals.get<uint8_t>() + total, 0, 64));
	HIPCHK(h, hipMemset(r->name_off.get<uint64_t>(), 0, 8 * std::max<uint64_t>(n_reads, 1))); HIPCHK(h, hipMemset(r->name_len.get<uint32_t>(), 0, 4 * std::max<uint64_t>(n_reads, 1)));
	/* qualities: the array, the one character, or Read::REF_QUAL (a batch always has a quality array; REF_QUAL reads weigh 1) */
	if (quals) { if (total) HIPCHK(h, hipMemcpy(r->quals.get<uint8_t>(), quals + first, total, hipMemcpyHostToDevice)); }
	else HIPCHK(h, hipMemset(r->quals.get<uint8_t>(), uniform_quality ? uniform_quality : 127, total));
	if (!n_reads) { HIPCHK(h, hipMemset(r->offsets.get<uint64_t>(), 0, 8)); *out = r.release(); return KMR_OK; }
	Scratch tmp(h); uint8_t *dtb, *dmc = nullptr; uint64_t *dto, *doff, *dmo = nullptr; uint32_t *dmp = nullptr;
	HIPCHK(h, tmp.take(&dtb, tbytes + 64)); HIPCHK(h, tmp.take(&dto, n_reads + 1)); HIPCHK(h, tmp.take(&doff, n_reads + 1));
	std::vector<uint64_t> rel(n_reads + 1), trel(n_reads + 1), mrel(markup_offsets ? n_reads + 1 : 0);
	for (uint64_t i = 0; i <= n_reads; i++) { rel[i] = offsets[i] - first; trel[i] = twobit_offsets[i] - twobit_offsets[0]; if (markup_offsets) mrel[i] = markup_offsets[i] - markup_offsets[0]; }
	if (tbytes) HIPCHK(h, hipMemcpy(dtb, twobit + twobit_offsets[0], tbytes, hipMemcpyHostToDevice));
	HIPCHK(h, hipMemcpy(dto, trel.data(), 8 * (n_reads + 1), hipMemcpyHostToDevice)); HIPCHK(h, hipMemcpy(doff, rel.data(), 8 * (n_reads + 1), hipMemcpyHostToDevice));
	LAUNCH(h, twobit_unpack_kernel, dim3((unsigned)std::min<uint64_t>((n_reads + 255) / 256, (uint64_t)num_cus(h) * 32)), dim3(256), 0, (const uint8_t *)dtb, (const uint64_t *)dto, (const uint64_t *)doff, n_reads, r->bases.get<uint8_t>(), r->offsets.get<uint64_t>());
	if (nm) {
		HIPCHK(h, tmp.take(&dmo, n_reads + 1)); HIPCHK(h, tmp.take(&dmp, nm)); HIPCHK(h, tmp.take(&dmc, nm));
		HIPCHK(h, hipMemcpy(dmo, mrel.data(), 8 * (n_reads + 1), hipMemcpyHostToDevice));
		HIPCHK(h, hipMemcpy(dmp, markup_pos + markup_offsets[0], 4 * nm, hipMemcpyHostToDevice)); HIPCHK(h, hipMemcpy(dmc, markup_char + markup_offsets[0], nm, hipMemcpyHostToDevice));
		LAUNCH(h, twobit_markup_kernel, dim3(grid_for(n_reads)), dim3(256), 0, (const uint64_t *)dmo, (const uint32_t *)dmp, (const uint8_t *)dmc, (const uint64_t *)r->offsets.get<uint64_t>(), n_reads, r->bases.get<uint8_t>());
	}
	HIPCHK(h, hipStreamSynchronize(h->stream));
	tmp.done();
	*out = r.release();
	return KMR_OK;
}


}  // extern "C"
