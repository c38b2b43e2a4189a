/*
 * kmr_host.hpp -- what the host side of the library shares between its translation units (kmr_api.hip: the spectrum; kmr_stages.hip:
 * the read stages): device memory (dev_malloc, DevBuf, the live-block counter), the handle and the result objects, error reporting
 * (HIPCHK, fail), the checked launch (LAUNCH, launch_status), read-backs (fetch_queue, stream_wait, fetch), dispatch helpers, the few
 * spectrum-side functions the stages call, and the sorts of kmr_sort.hip.
 * Internal: nothing here is an exported symbol of the library (namespace kmr_host and the structs are of hidden visibility), and no
 * kernel is defined here.
 */
#ifndef KMR_HOST_HPP_
#define KMR_HOST_HPP_

#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/kmernator_amd.h"

#define KMR_HIDDEN __attribute__((visibility("hidden")))

namespace kmr { struct SkPacked; }      /* kmr_superkmer.hpp */

namespace kmr_host KMR_HIDDEN {

/* (the variables below exist once in the library: C++17 inline variables) */
inline std::string g_create_error;

/* Every device allocation of the library goes through dev_malloc.  An allocation that fails for lack of memory although the card
 * as a whole could hold it is tried again for a bounded time (memory another handle or torch has just freed is handed back by the
 * driver with a delay, and work still running on other streams may hold what it is about to free); what was asked for and what the
 * device had is kept for the error text (oom_note), so that a KMR_ERR_OOM says how far off it was. */
inline thread_local char g_oom_note[160] = "";
inline std::atomic<long long> g_blocks_live{0};      /* blocks dev_malloc has handed out and DevBuf has not freed (kmr_build_info "device_blocks_live") */
inline hipError_t dev_malloc(void **p, size_t bytes) {
	hipError_t e = hipMalloc(p, bytes);
	if (e == hipSuccess) { if (*p) g_blocks_live++; return e; }      /* (a 0-byte request may succeed with no block) */
	if (e != hipErrorOutOfMemory) return e;
	size_t fr = 0, tot = 0;
	for (int attempt = 0; attempt < 6; attempt++) {
		(void)hipGetLastError();
		hipDeviceSynchronize();
		if (hipMemGetInfo(&fr, &tot) != hipSuccess || bytes > tot) break;
		usleep(20000u << attempt);      /* 20 ms ... 640 ms: 1.3 s at most */
		e = hipMalloc(p, bytes);
		if (e == hipSuccess && *p) g_blocks_live++;
		if (e != hipErrorOutOfMemory) return e;
	}
	(void)hipGetLastError();
	hipMemGetInfo(&fr, &tot);
	snprintf(g_oom_note, sizeof(g_oom_note), " [requested %.3f GB; device has %.3f GB free of %.3f GB]", bytes / 1e9, fr / 1e9, tot / 1e9);
	*p = nullptr;
	return hipErrorOutOfMemory;
}

/* One block of device memory and its size in bytes, freed when the owner goes: every device allocation of the library is one.
 * Kernels take get<T>(); alloc() replaces the block by one of exactly `bytes`, reserve() (below kmr_handle) grows it only. */
class DevBuf {
public:
	DevBuf() = default;
	DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
	DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); std::swap(p_, o.p_); std::swap(cap_, o.cap_); } return *this; }
	~DevBuf() { reset(); }
	void reset() { if (p_) { hipFree(p_); g_blocks_live--; } p_ = nullptr; cap_ = 0; }
	hipError_t alloc(size_t bytes) {      /* empty on failure */
		reset();
		void *p = nullptr;
		const hipError_t e = dev_malloc(&p, bytes);
		if (e == hipSuccess) { p_ = p; cap_ = bytes; }
		return e;
	}
	/* grow-only: a block of `bytes` (default: need) unless the one held has `need`; drains the handle's stream before freeing it.
	 * A failure sets the handle's error text, naming the buffer (`what`). */
	int reserve(kmr_handle *h, const char *what, size_t need, size_t bytes = 0);
	template <class T = void> T *get() const { return (T *)p_; }
	size_t cap() const { return cap_; }
	explicit operator bool() const { return p_ != nullptr; }
private:
	void *p_ = nullptr;
	size_t cap_ = 0;
};

/* scratch of kmr_sort.hip's sorts (declared below), grow-only: a pass's keys before and after, the second order array, rocPRIM's storage */
struct SortBufs { DevBuf kin, kout, perm2, tmp; };

struct DevMap {                      /* a finalized map resident in HBM */
	uint64_t nb = 0, n = 0;
	DevBuf start;                    /* [nb+1] */
	DevBuf keys;                     /* [n][W] */
	DevBuf vals;                     /* weak: [n][vw] */
	DevBuf sweight;                  /* singleton */
	DevBuf spkt;                     /* singleton, EXT */
	DevBuf image;                    /* reference layout, built lazily */
	bool present = false;
};

struct HostPool {                    /* owner of one chunk pool */
	DevBuf base, chunk_list, chunk_count, head;
	uint32_t cap = 0; size_t chunk_bytes = 0;
	uint64_t used_ub = 0;            /* host-side upper bound of chunks handed out */
	uint64_t presize = 0;            /* chunks the next allocation takes beyond what is asked for (a job fed in many calls, see sk_add_reads) */
};

/* The handle's device memory, grouped by when it is given back: */
struct HandleMem {                   /* ... by kmr_destroy */
	DevBuf slots, extslots;          /* device table */
	DevBuf dP, dstats, derr;
	DevMap weak, sing;
	/* streaming lookups (sk_index_* / sk_lookup_kernel): the weak map's entries grouped by minimizer list, of map generation ix_gen */
	DevBuf ix_start, ix_keys, ix_counts;
	DevBuf scratch_stats;
	DevBuf adopt_buf;                /* kmr_sk_exchange_adopt_dev's scan */
	DevBuf trk;                      /* size tracker: one record per read of the last call */
	DevBuf scan_sums;
	DevBuf score_buf;                /* temporaries of kmr_score_reads*, grow-only */
	DevBuf bimodal_buf;              /* one word per read of the last scoring call that ran with kmr_set_bimodal_sigmas >= 0 (bimodal_trim_kernel), grow-only; never allocated while the option is off */
	DevBuf fasta_buf[2][3];          /* scratch of kmr_ingest_fasta* (FASTA text, QUAL text; per block, per line, per record), grow-only */
	DevBuf lut;                      /* lookup accelerator over the weak map (LutView) */
	DevBuf dPk;                      /* build_mode 3: table of k-fold quality products */
	DevBuf d_uni;                    /* uniform-weight flags of adopted records */
	DevBuf qrange;                   /* sk_qual_range_kernel's answer */
	DevBuf sk_fine_state;            /* fine list state of an exchange (2^(sk_bits + sk_fine_shift) words) */
	/* an exchange in steps over the list space (kmr_sk_exchange_range) and the lists below `hi` counted early (kmr_count_lists_prefix):
	 * their entries wait in buffers of their own until kmr_finalize has counted the rest */
	struct Early { bool active = false; uint64_t hi = 0; uint32_t min_depth = 0; DevBuf ue, cursor, fc, err; } early;      /* err: the early pass's own error word, read by kmr_finalize alone */
	DevBuf dedup_tab;                /* kmr_dedup_fragments*: the probability and quality-step tables (DedupTables), made by the first call */
	DevBuf xo_dev;                   /* kmr_extract_by_owner_host: owner segments of one batch kept on the device between the sizing call and the copy-out */
	DevBuf cmp_buf[11];              /* temporaries of kmr_compare_spectrums / kmr_compare_reads* (compare_reads_core's CMP_* indices), grow-only */
	SortBufs cmp_sort;               /* ... and of the sorted path's sort */
};
struct BuildMem {                    /* ... by kmr_release_table too: the streaming build's state */
	DevBuf sk_state;                 /* build_mode 3 (kmr_superkmer.hpp): list words */
	HostPool l1;                     /* the record pool of every partition level */
	DevBuf work_counter;
	DevBuf l1_state; bool l1_state_dirty = false;      /* see PartSource::state */
	/* temporaries of kmr_finalize (chunk CSRs, work items, counters): one grow-only block handed out by bumping a
	 * cursor, so a finalize neither allocates nor frees device memory once the handle has seen one build */
	DevBuf arena; size_t arena_used = 0, arena_want = 0; std::vector<DevBuf> arena_overflow;
	DevBuf linear;                   /* records */
	DevBuf tile_count, kcap, koff;
	/* work units of batches that contain reads longer than one tile */
	DevBuf ucnt, ufirst, u_start, u_end, u_read, umax;
	/* kmr_add_reads_twobit*: the unpacked batch (ASCII bases, one quality character throughout, offsets counted from the call's first read) */
	DevBuf tb_bases, tb_quals, tb_rel, tb_off, tb_len;
	uint64_t tb_quals_filled = 0; int tb_quals_char = -1;
	DevBuf tb_stage[2][8];           /* kmr_add_reads_twobit: two sets of staging buffers for the pieces on the bus */
	DevBuf uw_keys, uw_vals, us_keys, us_b8, us_pkt;
	/* build_mode 3: the count pass's weak entries packed (kmr_buckets.hpp: W key words + one value word), and the radix partition's scratch of the same layout */
	DevBuf ue, ue2;
};
struct ExchangeMem {                 /* ... after the communicator that uses it (kmr_exchange_rccl.hpp): gather scratch, grow-only send / receive buffers */
	DevBuf xc_small, xc_dcounts;
	DevBuf xc_send, xc_send2, xc_recv, xc_recv2;
};

}  // namespace kmr_host
using namespace kmr_host;

/* per-handle knobs of kmr_tune(): sizes the tests shrink to reach the multi-level / retry / sub-batch code with small inputs, and
 * switches the measurement tools flip.  None of them changes a result. */
struct KMR_HIDDEN Tuning {
	uint64_t target_list = 2048;      /* records per final list the partition bits aim for */
	uint64_t sub_batch_bases = 0;     /* 0 = SUB_BATCH_BASES */
	int recycle = -1;                 /* -1 auto, 0 fresh chunks, 1 recycle the chunks a pass has just read */
	int part_blocks = 0;              /* 0 = one partition block per CU */
	double entry_share = -1.0;        /* >= 0: initial size of the count pass's entry buffers as a share of the records */
	double early_entry_share = -1.0;  /* >= 0: size of kmr_count_lists_prefix's entry buffers as a share of the good k-mers (no CU slack) */
	uint64_t saturated_batch_bytes = 0;      /* scratch budget of one batch of the saturated-key pass (0: SAT_BATCH_BYTES) */
	bool no_lut = false, no_narrow = false, no_l1_state = false, no_stream_lookups = false;
	uint64_t long_list_chunks = 0;     /* lists of more chunks are counted in pieces (0: 1024) */
	uint64_t binned_min = 1ull << 18;  /* weak maps of at least this many entries are bucketed by the radix partition of kmr_buckets.hpp (build_mode 3) */
	bool bb_fixed_bins = true;         /* the radix partition gives every bin of a level one capacity instead of measuring the bins (0: histogram, pad and scan before every level; A/B runs, and the way a build takes when a bin overflows) */
	double bb_slack_bins = 1.0, bb_slack_groups = 1.0;      /* scale of the room above the mean in a first-level bin / in a group (bb_fixed_limit); tests: 0 leaves less than the mean, so that the level overflows */
	bool bb_reload = false;            /* bb_scatter_fixed_kernel reads a tile's entries a second time instead of keeping them in registers (A/B runs) */
	uint64_t twobit_piece_bases = 0;   /* kmr_add_reads_twobit: bases per piece of the host-to-device pipeline (0 = 2^26) */
	uint64_t list_aim = 0;             /* k-mers per list the list count of a single GPU's build aims for (0: the defaults of sk_size_lists) */
	bool pow2_lists = false;           /* the list count of build_mode 3 always a power of two (A/B runs, tests of both list functions) */
	bool no_packed_direct = false;     /* kmr_add_reads_twobit* always unpack to text first (A/B runs, tests of the unpack path) */
	bool no_uniform_count = false;     /* never take sk_count_kernel<.., UNI> (A/B runs, tests of the general count pass on one-weight builds) */
	int count_six = 0;                 /* the six-block instance of that pass (20-byte slots, sk_count_blocks): 0 = where the build's ordinals allow it and the lists are enough to feed six blocks per CU, 1 = wherever the ordinals allow it, 2 = never (kmr_tune "count_six"; A/B runs, tests) */
	int count_blocks = 0;              /* blocks per CU of the one-weight, one-word count pass over lists: 4, 5, or 0 = the default choice (sk_count_blocks; A/B runs, tests of both instances) */
	bool no_lean_extract = false;      /* never take sk_extract_lean_kernel (A/B runs, tests of the general kernel on uniform qualities) */
	bool exchange_fail_once = false;   /* tests: the next kmr_exchange_add_reads_dev of this rank fails locally (the other ranks must come back with an error, not hang) */
	uint64_t dump_piece_bytes = 0;     /* kmr_dump_mercount / kmr_dump_mergraph: staging bound of one piece of the file (0 = KMR_DUMP_PIECE_BYTES) */
	uint64_t dump_tiles_per_block = 0; /* kmr_dump_text*: output tiles one block of dump_write_kernel walks (0 = enough for 16 blocks per CU; tests: small values, so that a small text reaches the tile-to-tile hand-off) */
	bool dump_timing = false;          /* kmr_dump_text*: time the size pass and the writer with HIP events (kmr_build_info; measurement tools) */
	bool select_timing = false;        /* kmr_select_* / kmr_filter_*: time scoring, selection and writer with HIP events (kmr_build_info; measurement tools) */
	bool pairs_timing = false;         /* kmr_identify_pairs*: time the name parse, the sort and the whole call with HIP events (kmr_build_info; measurement tools) */
	bool dedup_timing = false;         /* kmr_dedup_fragments*: time the key kernel, the sorts, the consensus kernel and the whole call with HIP events (kmr_build_info; measurement tools) */
	uint32_t partition_units = 0;      /* kmr_partition_*: most units (wavefronts over contiguous reads) of the partition, 0 = the default of 8192 (tests: a few, so that a unit walks many tiles) */
	int artifact_report_lds = -1;      /* kmr_artifact_filter_report*: where the per-sequence counters are summed (-1: in LDS while they fit ART_REPORT_LDS_CAP; tests: 0 = global atomics, 1 = LDS up to ART_REPORT_LDS_MOST) */
	uint32_t pair_hash_bits = 64;      /* kmr_identify_pairs*: bits of the common name's hash the phase-2 sort keys keep (tests: a few bits, so that distinct names share a key) */
	int bimodal_window = -1;           /* bimodal_trim_kernel: the longest run it stages in LDS (-1: BM_CAP; tests: 0, so that every run is walked in global memory) */
	bool csr_partition = true;         /* build_csr: the chunk CSR by the radix partition of csr_bin_*_kernel (default) or, 0, by chunk_hist_kernel / chunk_scatter_kernel's atomic per chunk (A/B runs, tests of both, and what more than 2^24 lists take) */
	int compare_lds_kmers = -1;        /* kmr_compare_reads*: the most k-mers of a read that compare_reads_lds_kernel takes (-1: CMP_CAP; 0: every read goes through the sorted path; tests: a few) */
	uint64_t compare_stage_kmers = 0;  /* kmr_compare_reads*: staging slots of one run of whole reads (0: CMP_STAGE_SLOTS; tests: a few, so that a batch takes several runs and a read alone exceeds one) */
	uint32_t tnf_piece_bases = 0;      /* kmr_tnf_reads / kmr_tnf_windows: bases of one piece of a sequence (0: TNF_PIECE_BASES; tests: a few, so that short inputs cross piece edges) */
	uint64_t match_hit_capacity = 0;   /* kmr_match_add_read_batch: hit records the buffers hold before they first grow (0: MATCH_HIT_CAP; tests: a few, so that the batch is streamed again) */
	uint64_t extend_stage_kmers = 0;   /* kmr_extend_contigs*: staging slots of one run of whole contigs (0: EXT_STAGE_SLOTS; tests: a few, so that a call takes several runs and a contig alone exceeds one) */
	bool extend_timing = false;        /* kmr_extend_contigs*: time gather, extraction, sort, reduce and the walk with HIP events (kmr_build_info; measurement tools) */
	bool no_coarse_lists = true;     /* exchange: scatter into the job's fine lists (default) or, kmr_tune("coarse_lists", 1), into coarse ones that the owner splits before the count pass (sk_refine_kernel: not yet fast enough to pay) */
};

/* What the caller of one feed call knows about it, handed down from the entry point to the extraction (add_reads_dev_call,
 * add_reads_superkmer_t, sk_uniform_weight); it ends with the call */
struct KMR_HIDDEN FeedHints {
	const kmr::SkPacked *packed = nullptr;      /* the batch is two-bit packed and sk_extract_lean_kernel<.., PACKED> takes it as it is (sk_packed_direct_ok) */
	int uniform_q = -1;                         /* >= 0: the qualities of the batch are this one character */
	uint64_t call_bases = 0;                    /* a host batch goes to the device in pieces: the bases of the WHOLE call, for what the first piece sizes (lists, chunk pool) */
	uint64_t piece_origin = 0;                  /* ... and a piece that keeps the call's offsets: its first one, which stream_base has counted already (stream ordinals) */
};

struct KMR_HIDDEN kmr_handle : HandleMem, BuildMem, ExchangeMem {
	kmr_config cfg;
	Tuning tune;
	uint32_t k = 0, kb = 0, hkb = 0, W = 0;
	bool ext = false;
	int device = 0, ncu = 0;
	hipStream_t stream = nullptr;
	std::string err;
	/* device table */
	uint32_t log2cap = 0;
	uint64_t occupied = 0;           /* exact as of the last sync */
	uint64_t pending_kmers = 0;      /* upper bound of keys added since */
	uint64_t stream_base = 0, reads = 0;
	/* build_mode 3: lowest and highest stream ordinal a feed call of this build may have stamped (DevStats' pair as the last sync_state
	 * read it; ord_seen: there was such a call), and whether records came in that this handle did not stamp (adopted from an
	 * exchange): sk_count_blocks */
	uint64_t ord_lo = 0, ord_hi = 0; bool ord_seen = false, ord_foreign = false;
	uint64_t nb_weak = 0, nb_sing = 0;
	bool finalized = false, has_singletons = true;
	kmr_handle *subtract = nullptr;    /* finalized spectrum whose k-mers are skipped (kmr_subtract_reference) */
	uint64_t subtracted = 0;
	kmr_stats stats;
	/* streaming (partition) build path */
	bool partition_mode = false;
	bool superkmer_mode = false;       /* build_mode 3: super-k-mer lists (kmr_superkmer.hpp); implies partition_mode */
	uint64_t ix_lists = 0, ix_gen = ~0ull;      /* the streaming lookups' index (ix_*): its list count and map generation */
	/* size tracker (kmr_config.size_tracker): records of the reads fed by the last call (trk), and the elements made of them at kmr_finalize */
	uint64_t trk_n = 0; std::vector<uint64_t> trk_elems;
	/* the thresholds passed so far (SizeTracker::nextToTrack and the elements' first two counters), found call by call while the
	 * reads are still at hand: the stream ordinal behind the k-mer at which rawKmers reached the threshold, rawKmers, rawGoodKmers */
	long trk_next = 128; uint64_t trk_raw = 0, trk_good = 0; std::vector<unsigned long long> trk_bounds; std::vector<uint64_t> trk_snap_raw, trk_snap_good;
	bool sk_fast_div = false;          /* see kmr_create: the chain's divide as multiply-and-correct */
	bool sk_exchange = false;          /* kmr_sk_exchange_begin: the lists are the whole job's, every owner's k-mers are kept until the exchange */
	bool auto_mode = false;            /* build_mode 0: a handle that is fed k-mer records (the owner exchange) before any reads falls back to mode 2 */
	int bits1 = 0;
	uint64_t inserted_records = 0;     /* records fed through kmr_insert_records_dev (counted on the host) */
	uint32_t lut_log2 = 0;
	uint64_t lut_gen = ~0ull, map_gen = 0;                           /* the lookup table belongs to the maps of generation lut_gen */
	hipStream_t tb_copy_stream = nullptr; hipEvent_t tb_ready[2] = {nullptr, nullptr}, tb_consumed[2] = {nullptr, nullptr}; bool tb_set_used[2] = {false, false};
	/* build_mode 3 (kmr_superkmer.hpp): list count and minimizer geometry */
	uint32_t sk_bits = 0, sk_m = 0, sk_off = 0, sk_win = 0;
	double hP[256], hPk[256];              /* host copies of the probability table and of its k-fold products */
	/* does every record of the lists carry ONE weight (all calls went through the lean extraction with the same quality character)?  The
	 * host knows for its own calls (sk_uni_w: SK_UNI_NONE before the first; sk_uni_mixed), a device pair collects it for adopted records (d_uni) */
	uint32_t sk_uni_w = 0xffffffffu; bool sk_uni_mixed = false; bool last_count_uniform = false;
	/* ... or the senders say so themselves (kmr_sk_exchange_peer_uniform): then nothing is looked at on arrival */
	uint32_t peer_uni_w = 0xffffffffu; bool peer_uni_mixed = false, peers_declare = false;
	uint64_t xr_lo = 0, xr_hi = ~0ull;      /* kmr_sk_exchange_range */
	uint64_t last_early_hi = 0, last_early_entries = 0;      /* what the last kmr_finalize took over from an early count (kmr_build_info) */
	/* the radix partition of the last kmr_finalize (kmr_build_info "bb_path": 0 none, 1 measured bins, 2 bins of one capacity; "bb_fallback": a bin
	 * overflowed and the build was made again with measured bins) */
	int last_bb_path = 0; bool last_bb_fallback = false;
	/* --bimodal-sigmas (kmr_set_bimodal_sigmas; ReadSelector::_bimodalSigmas, -1 = off) and what the last scoring call left: the number of its reads
	 * (~0: there was none) and whether bimodal_buf holds their words (kmr_bimodal_copy).  sel_bimodal: the words kmr_select_bimodal handed in for the
	 * next selecting call over host arrays */
	double bimodal_sigmas = -1.0; uint64_t bimodal_n = ~0ull; bool bimodal_on = false;
	std::vector<uint64_t> sel_bimodal; bool sel_bimodal_set = false;
	int last_score_path = 0;      /* kmr_build_info "score_path": where the last kmr_score_reads / _read_batch / kmr_filter_read_batch got its counts */
	bool last_early_overflowed = false;                       /* ... or that it voided one because its buffers overflowed */
	double last_score_ms = 0, last_select_ms = 0, last_write_ms = 0;      /* the last kmr_filter_read_batch* / kmr_select_reads*: scoring, selection + writer, writer alone (HIP events, taken with kmr_tune "select_timing" only; kmr_build_info) */
	int last_artifact_report_lds = 0;      /* the last kmr_artifact_filter_report* / _apply_report*: 1 = its counters were summed in LDS, 0 = by global atomics (kmr_build_info) */
	double last_dump_size_ms = 0, last_dump_write_ms = 0;      /* the last kmr_dump_text_size / kmr_dump_text: size pass with its scan, writer (HIP events, taken with kmr_tune "dump_timing" only; kmr_build_info) */
	uint64_t last_dump_tiles_per_block = 0, last_dump_blocks = 0;      /* the last kmr_dump_text that wrote a text: tiles per block and blocks of dump_write_kernel (kmr_build_info) */
	double last_pairs_ms = 0, last_pairs_parse_ms = 0, last_pairs_sort_ms = 0;      /* the last kmr_identify_pairs*: the whole call, its name parse, its radix sort (HIP events, taken with kmr_tune "pairs_timing" only; kmr_build_info) */
	double last_dedup_ms = 0, last_dedup_key_ms = 0, last_dedup_sort_ms = 0, last_dedup_consensus_ms = 0;      /* the last kmr_dedup_fragments*: the whole call, its key kernel, its radix sorts, its consensus kernel (HIP events, taken with kmr_tune "dedup_timing" only; kmr_build_info) */
	uint64_t last_pair_hash_collisions = 0;      /* ... and how many of its runs of equal hash keys held more than one distinct common name */
	uint64_t last_saturated_keys = 0, last_saturated_batches = 0;      /* what the last kmr_finalize's saturated-key pass redid, in how many batches */
	int last_csr_path = -1; uint32_t last_csr_chunks = 0;      /* the last build_csr: 1 = radix partition, 0 = an atomic per chunk, and the chunks it looked at (kmr_build_info "csr_path", "csr_chunks") */
	unsigned int l1_head_seen = 0;     /* the record pool's head as of the last sync_state(h, true) */
	uint64_t unit_batches = 0;         /* batches that held a read longer than a tile and were cut into work units (kmr_build_info "unit_batches") */
	int last_match_attempts = 0;       /* how often the last kmr_match_add_read_batch streamed its batch before the hit records fit (kmr_build_info "match_add_attempts") */
	int last_extend_runs = 0; double last_extend_ms[5] = {0, 0, 0, 0, 0};      /* the last kmr_extend_contigs*: its runs of whole contigs (kmr_build_info "extend_runs") and, with kmr_tune "extend_timing", the HIP-event times of gather, extraction, sort, reduce and walk */
	int last_count_blocks = 0;      /* blocks per CU the last launch of the count pass over super-k-mer lists was compiled and sized for (kmr_build_info "count_blocks") */
	int last_count_attempts = 0;    /* how often the last count pass of a kmr_finalize ran before its entries fit (kmr_build_info "count_attempts") */
	bool qual_mixed = false;           /* a build that has seen two different quality characters stops asking (qrange) */
	/* exchange with world_size > 1: sk_bits are the COARSE lists reads are scattered into and that travel; each holds 2^sk_fine_shift
	 * fine lists, made by sk_refine_kernel before the count pass (fine state: sk_fine_state) */
	uint32_t sk_fine_shift = 0;
	uint64_t xo_segcap = 0; std::vector<uint64_t> xo_counts; const void *xo_batch = nullptr; uint64_t xo_first = 0;      /* xo_dev's segments */
	/* kmr_exchange_* (kmr_exchange_rccl.hpp): communicator, transport, what the job was fed so far */
	void *xc_comm = nullptr; kmr_transport xc_tr = {nullptr, nullptr, nullptr};
	uint64_t xc_job_bases = 0, xc_bytes_to_peers = 0;
	/* timing */
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	double ms[KMR_TIME_GROUPS] = {0};
	uint64_t launches[KMR_TIME_GROUPS] = {0};
	std::vector<std::pair<hipEvent_t, hipEvent_t> > pending_events[KMR_TIME_GROUPS];
};

/* what kmr_select_reads* / kmr_filter_read_batch* leave on the device: the output text and the per-read pick flags */
/* a result object lives on one device; its buffers are freed there (free_on_device) */
struct OnDevice { int device = 0; };

struct KMR_HIDDEN kmr_picks : OnDevice {
	DevBuf text, picked;
	uint64_t n = 0, n_picked = 0, bytes = 0;
	/* segment = round * n_inputs + input.  Picks of the plain entry points are one round and one input, and hold no read_seg (it
	 * follows from picked) */
	DevBuf read_seg;                        /* int32 per read, -1 = not picked */
	std::vector<uint64_t> seg_table;        /* per segment {first pick, picks, first byte, bytes} */
	uint32_t n_rounds = 1, n_inputs = 1;
	float round_depth[33] = {};
	uint8_t round_is_remainder[33] = {};
	/* kmr_normalize_*: picks (pairs), chooseRead calls, draws (kmr_normalize_info) */
	bool normalized = false;
	uint64_t norm_info[3] = {};
};

/* what kmr_identify_pairs* leaves on the device: the mate of every read and the pair list */
struct KMR_HIDDEN kmr_pairs : OnDevice {
	DevBuf mate, read1, read2;
	uint64_t n = 0, n_pairs = 0, n_full = 0, n_seq = 0, n_conflicts = 0;
};

/* what kmr_dump_text leaves on the device: the mercount / mergraph text of a range of weak entries */
struct KMR_HIDDEN kmr_text : OnDevice {
	DevBuf text;
	uint64_t kept = 0, bytes = 0;
};

/* device-resident read batch produced by kmr_ingest_fastq* */
struct KMR_HIDDEN kmr_reads : OnDevice {
	DevBuf bases, quals;                          /* 64 bytes of padding behind the data: extract_kernel stages 16-byte blocks */
	DevBuf offsets;                               /* [n + 1] */
	DevBuf name_off, name_len;
	uint64_t n = 0, total = 0, filtered = 0;
	uint32_t input_base = 0;
};

/* what kmr_dedup_fragments* leaves on the device: the discard flags, the collapsed groups, the consensus batch and its names */
struct KMR_HIDDEN kmr_dedup : OnDevice {
	DevBuf disc, group_first, group_size, names;
	kmr_reads *cons = nullptr;                    /* owned */
	~kmr_dedup() { delete cons; }
	uint64_t n = 0, n_groups = 0, affected = 0, name_bytes = 0;
	uint64_t skipped[4] = {0, 0, 0, 0};
};

/* what kmr_tnf_reads / kmr_tnf_windows / kmr_tnf_group_sums leave on the device: n vectors of D counts in column order, their origin and
 * float lengths, and -- made by the first distance call that needs them, kept since -- the per-vector part of either distance */
struct KMR_HIDDEN kmr_tnf : OnDevice {
	DevBuf counts;                                /* [n][D] u32; u64 for group sums (wide) */
	DevBuf origin;                                /* [n][3] u64: sequence, first base, bases */
	DevBuf len;                                   /* [n] f32 */
	DevBuf group;                                 /* [n] u32: the group of every vector */
	mutable DevBuf qt;                            /* Euclidean: [D][n] f64 value / length */
	mutable DevBuf xt, x2;                        /* Spearman: [D][n] f32 rank - mean, [n] f32 sum_x2 */
	std::vector<uint64_t> bounds;                 /* groups + 1 */
	uint64_t n = 0, inexact = 0;
	uint32_t D = 0, k = 0, hash_kind = 0;
	bool wide = false;
};

/* KmerMatch (kmr_match.hpp): the table of the contigs' edge keys, the hit records of the batches streamed so far, and after
 * kmr_match_finish the result.  Refers to the handle it was made from */
struct KMR_HIDDEN kmr_match : OnDevice {
	kmr_handle *h = nullptr;
	kmr_match_config cfg;
	uint64_t n_contigs = 0, n_edge_kmers = 0, n_distinct_keys = 0, n_keys_in_spectrum = 0;
	DevBuf slots, tcontig; uint32_t log2cap = 6;      /* the table: 2^log2cap slots of W + 1 words; the contigs of every key */
	DevBuf hit_key, hit_mate, hit_count;              /* packed (contig, global read), global mate or MATCH_NO_MATE; one u64 counter */
	uint64_t hit_cap = 0, n_hits = 0;
	struct Batch { uint64_t first = 0, n = 0; DevBuf discarded; };      /* the discard flags live until the finish drops the reads */
	std::vector<Batch> batches;
	bool finished = false;
	DevBuf offsets, read_ids, size_before, size_after;
	uint64_t n_reads_total = 0, n_sampled = 0;
};

/* what kmr_extend_contigs* leaves on the device: per contig the new length and the bases added on either side, per contig and side the
 * stop record (reason; edge, A, C, G, T, total), and the new sequences as a read batch */
struct KMR_HIDDEN kmr_extend : OnDevice {
	DevBuf newlen, left, right, reason, vals;
	kmr_reads *result = nullptr;                  /* owned */
	~kmr_extend() { delete result; }
	uint64_t n = 0, n_extended = 0, bases_added = 0;
};

namespace kmr_host KMR_HIDDEN {

inline std::string oom_note() { std::string s(g_oom_note); g_oom_note[0] = 0; return s; }

inline std::string hip_err_text(hipError_t e) { return std::string(hipGetErrorString(e)) + (e == hipErrorOutOfMemory ? oom_note() : std::string()); }

#define HIPCHK(h, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
	(h)->err = std::string(#call) + ": " + hip_err_text(e_); \
	return e_ == hipErrorOutOfMemory ? KMR_ERR_OOM : KMR_ERR_HIP; } } while (0)

/* The one kernel launch of the library: the arguments converted to the kernel's parameter types as in an ordinary call (a kernel's
 * default arguments are spelled out), and what hipGetLastError() says of it.  launch_status hands that back and touches nothing
 * else (the sites that go on without the kernel or report in their own way, and the one entry point without a handle: its result
 * is never dropped, tests/test_host_launch_sites.py); LAUNCH is the launch on the handle's stream as a statement: a failure names
 * the kernel in h->err and leaves the enclosing function with HIPCHK's code.  A grid of no blocks is an error: `if (n) LAUNCH(...)`
 * keeps its condition. */
template <class... P, class... A> hipError_t launch_status(hipStream_t stream, void (*kern)(P...), dim3 grid, dim3 block, size_t lds, A... args) {
	hipLaunchKernelGGL(kern, grid, block, lds, stream, args...);
	return hipGetLastError();
}
#define LAUNCH(h, kern, grid, block, lds, ...) do { hipError_t e_ = launch_status((h)->stream, kern, grid, block, lds, ##__VA_ARGS__); if (e_ != hipSuccess) { \
	(h)->err = std::string(#kern) + ": " + hip_err_text(e_); \
	return e_ == hipErrorOutOfMemory ? KMR_ERR_OOM : KMR_ERR_HIP; } } while (0)

/* Small results back to the host over the handle's stream, each under HIPCHK: fetch_queue queues the copy of n elements of T,
 * stream_wait waits for what is queued (several copies, one wait), fetch is both for a single value or array */
template <class T> hipError_t fetch_queue(kmr_handle *h, T *dst, const void *src, size_t n = 1) { return hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, h->stream); }
inline hipError_t stream_wait(kmr_handle *h) { return hipStreamSynchronize(h->stream); }
template <class T> hipError_t fetch(kmr_handle *h, T *dst, const void *src, size_t n = 1) { const hipError_t e = fetch_queue(h, dst, src, n); return e != hipSuccess ? e : stream_wait(h); }

inline int DevBuf::reserve(kmr_handle *h, const char *what, size_t need, size_t bytes) {
	if (p_ && cap_ >= need) return 0;
	if (!bytes) bytes = need;
	hipError_t e = p_ ? hipStreamSynchronize(h->stream) : hipSuccess;      /* kernels in flight may still read it */
	if (e == hipSuccess) e = alloc(bytes);
	if (e == hipSuccess) return 0;
	h->err = std::string("device buffer ") + what + " (" + std::to_string(bytes) + " bytes): " + hip_err_text(e);
	return e == hipErrorOutOfMemory ? KMR_ERR_OOM : KMR_ERR_HIP;
}

inline int fail(kmr_handle *h, int code, const std::string &msg) { const std::string m = code == KMR_ERR_OOM ? msg + oom_note() : msg; if (h) h->err = m; else g_create_error = m; return code; }

/* The one place where the key width (h->W: 1-4 words, anything else behaves as 4) and, where wanted, the value kind (h->ext) turn into
 * compile-time constants: with_w(h, [&](auto W) { return finalize_superkmer_t<W()>(h, min_depth); }), with_w_ext(h, [&](auto W, auto EXT) { ... }) */
template <int N> using int_c = std::integral_constant<int, N>;
template <class F> auto with_w(const kmr_handle *h, F &&f) {
	switch (h->W) { case 1: return f(int_c<1>()); case 2: return f(int_c<2>()); case 3: return f(int_c<3>()); default: return f(int_c<4>()); }
}
template <class F> auto with_w_ext(const kmr_handle *h, F &&f) {
	return with_w(h, [&](auto W) { return h->ext ? f(W, std::true_type()) : f(W, std::false_type()); });
}

inline int grid_for(uint64_t n, int block = 256, int maxBlocks = 256 * 16) {
	uint64_t g = (n + block - 1) / block;
	if (g < 1) g = 1;
	if (g > (uint64_t)maxBlocks) g = maxBlocks;
	return (int)g;
}

/* a scratch block of n elements of T (256 bytes at least) */
template <class T> hipError_t alloc_n(DevBuf &b, T **p, size_t n) { const hipError_t e = b.alloc(std::max<size_t>(sizeof(T) * n, 256)); *p = b.get<T>(); return e; }

/* up to N HIP events on the handle's stream, created and recorded only while the call's timing knob (kmr_tune "select_timing", "pairs_timing", ...) is set */
template <int N> struct EventTimer {
	hipEvent_t ev[N] = {}; bool on;
	explicit EventTimer(bool enabled) : on(enabled) { if (on) for (auto &e : ev) if (hipEventCreate(&e) != hipSuccess) { e = nullptr; on = false; } }
	~EventTimer() { for (auto e : ev) if (e) hipEventDestroy(e); }
	void mark(int i, hipStream_t s) { if (on) hipEventRecord(ev[i], s); }
	double ms(int a, int b) const { float t = 0; return on && hipEventElapsedTime(&t, ev[a], ev[b]) == hipSuccess ? t : 0.0; }      /* after the stream has been waited for */
};

/* One timed span of work on the handle's stream for group `which` of kmr_kernel_time: the first event is recorded here, the second by
 * end() -- or by the destructor, so that a return in between leaks no event --, and the pair waits in h->pending_events for sync_state. */
struct TimeSpan {
	kmr_handle *h; int which; hipEvent_t a = nullptr, b = nullptr; bool open = true;
	TimeSpan(kmr_handle *h_, int which_) : h(h_), which(which_) { hipEventCreate(&a); hipEventCreate(&b); hipEventRecord(a, h->stream); }
	TimeSpan(const TimeSpan &) = delete;
	TimeSpan &operator=(const TimeSpan &) = delete;
	~TimeSpan() { end(); }
	void end() { if (!open) return; open = false; hipEventRecord(b, h->stream); h->pending_events[which].push_back(std::make_pair(a, b)); }
};

/* ---- defined in kmr_api.hip: what the read stages use of the spectrum ---- */
uint64_t resize_buckets(uint64_t n);
void quality_table(double P[256], unsigned minQ, unsigned startChar);
int exclusive_scan(kmr_handle *h, const uint32_t *in, uint64_t n, uint64_t *out /* n+1 */);
int exclusive_scan_queue(kmr_handle *h, const uint32_t *in, uint64_t n, uint64_t *out /* n+1 */);      /* the same left on the handle's stream: the host does not wait */
int num_cus(kmr_handle *h);
struct ScoreDev { uint32_t *trim_offset, *trim_length; float *score; uint8_t *was_trimmed; const uint64_t *bimodal; };      /* the results in score_buf (bimodal: the words in bimodal_buf, null while --bimodal-sigmas is off), good until the handle's next scoring call */
int score_reads_core(kmr_handle *h, const uint8_t *s_b, const uint64_t *s_o, uint64_t n_reads, double minimum_kmer_score, int scoring_type,
                     uint32_t *trim_offset, uint32_t *trim_length, float *score, uint8_t *was_trimmed, ScoreDev *keep = nullptr);

/* CompareSpectrums (kmr_compare.hpp).  compare_spectrums_core: map 1 of h1 against map 2 of h2, the eight figures to host memory (waits).
 * compare_reads_core: one record per read of the device batch to dev_out (device memory, n_reads records), queued on h2's stream */
int compare_spectrums_core(kmr_handle *h1, kmr_handle *h2, kmr_compare_counts *out);
int compare_reads_core(kmr_handle *h2, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t n_reads, void *dev_out);
/* TnfDistance (kmr_tnf.hpp) takes a batch's k-mers from the same extraction: for a handle of one key word, slot koff[r] + i of *stage holds the
 * canonical key word of k-mer i of read r where it passes the weight test and all ones where it does not (CompareOp).  *koff (n_reads + 1) and
 * *stage live in h->cmp_buf until the handle's next kmr_compare_reads* or tnf_stage_core; the work is queued on h's stream, and the call waits
 * for the sizes.  The handle's world_size, num_parts and kmer_subsample are not applied. */
int tnf_stage_core(kmr_handle *h, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t n_reads, const uint64_t **koff, const uint64_t **stage, uint64_t *slots);

/* KmerMatch (kmr_match.hpp): the parts that need the spectrum and the extraction.  match_create_core fills m's table from the contigs
 * (device batch) and waits; match_add_core streams one device batch through MatchOp, appending to m's hit records (grown and the batch
 * streamed again where they did not fit), and waits for the count.  mate / discarded: device arrays of the batch, or NULL */
int match_create_core(kmr_handle *h, kmr_match *m, const uint8_t *bases, const uint64_t *offsets, uint64_t n_contigs);
int match_add_core(kmr_handle *h, kmr_match *m, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t n_reads, uint64_t first_global,
                   const int64_t *mate, const uint8_t *discarded);

/* ContigExtender (kmr_extend.hpp): gathers the pools, builds their spectra and walks the contigs; fills `out` and waits.  The batches are
 * of h's device, cfg is checked; pool_offsets (n_contigs + 1), pool_reads and active (or NULL) are device memory */
int extend_core(kmr_handle *h, const kmr_reads *contigs, const kmr_reads *reads, const uint64_t *pool_offsets, const uint64_t *pool_reads, const uint8_t *active,
                const kmr_extend_config *cfg, kmr_extend *out);

/* ---- defined in kmr_stages.hip (its kmr_ingest.hpp holds the two-bit kernels): what the spectrum's packed feed path launches.  All
 * pointers are device memory; the work is queued on the handle's stream. */
/* byte offsets of reads packed back to back, ceil(L / 4) bytes each: len[n + 1] scratch, off[n + 1] */
int twobit_byte_offsets(kmr_handle *h, const uint64_t *offsets, uint64_t n, uint32_t *len, uint64_t *off);
/* rel[i] = offsets[i] - offsets[0], i <= n */
int twobit_rel_offsets(kmr_handle *h, const uint64_t *offsets, uint64_t n, uint64_t *rel);
/* packed reads to ASCII bases (and rel as above), then the markups, if any, over them */
int twobit_unpack(kmr_handle *h, const uint8_t *twobit, const uint64_t *twobit_off, const uint64_t *offsets, const uint64_t *mk_off, const uint32_t *mk_pos, const uint8_t *mk_char,
                  uint64_t n, uint8_t *bases, uint64_t *rel);

/* ---- defined in kmr_sort.hip: the stable sort of (u64 key, u32 value) pairs on the handle's stream; `who` names the entry point in the
 * error text.  sort_reserve: the size query; bufs.tmp is grown to it, so one reservation serves every sort_pairs of no more pairs */
int sort_reserve(kmr_handle *h, SortBufs &bufs, size_t n, const char *who);
int sort_pairs(kmr_handle *h, SortBufs &bufs, const unsigned long long *kin, unsigned long long *kout, const uint32_t *vin, uint32_t *vout, size_t n, const char *who);
/* the sort key of element p in one pass of sort_by_columns: tags[p] if tags is set, else words[(row ? row[p] : p) * stride] */
struct SortColumn { const uint64_t *words; uint64_t stride; const uint32_t *row; const uint32_t *tags; };
/* n elements by ncols columns, cols[0] the least significant: one stable pass per column.  order: the element indices in their starting
 * order (overwritten).  *sorted: the sorted order, in `order` or in bufs.perm2, whichever the pass count leaves it in; *last_keys (unless
 * null): the last column in sorted order, the caller's to overwrite.  All queued; the host waits only where a buffer of bufs has to grow */
int sort_by_columns(kmr_handle *h, SortBufs &bufs, const SortColumn *cols, int ncols, uint32_t *order, uint64_t n, const char *who, const uint32_t **sorted, unsigned long long **last_keys);
/* head[j] = 1 where sorted element j opens a group, hscan its exclusive scan (n + 1): start[g] = the opener of group g, start[groups] = n */
int group_starts(kmr_handle *h, const uint32_t *head, const uint64_t *hscan, uint64_t n, uint64_t *start);

}  // namespace kmr_host

namespace kmr {      /* kmr_sort.hip: rocPRIM's radix sort as it is (saturated_fix_t) */
int sort_pairs_u64_u32(void *tmp, size_t *tmp_bytes, const unsigned long long *keys_in, unsigned long long *keys_out, const unsigned int *vals_in, unsigned int *vals_out, size_t n, hipStream_t stream);
}

#endif
