/*
 * kmr_api.hip -- C-ABI of include/kmernator_amd.h on top of the HIP kernels: the spectrum (the read stages -- ingest, artifact
 * filter, selection, pairs, duplicate fragments, dump text -- are kmr_stages.hip; kmr_host.hpp is what the two share).
 *
 * Host logic only: handle life cycle, device memory, launches on the handle's
 * stream, growth of the device table, finalize (bucket histogram -> scan ->
 * scatter -> sort -> image) and the stateless helpers.  There is no CPU
 * fallback: every compute entry point needs a HIP device and fails with
 * KMR_ERR_NO_DEVICE otherwise.
 * Shared decisions have one place each: the checked launch and the read-backs of small results (kmr_host.hpp: LAUNCH, launch_status,
 * fetch_queue / stream_wait / fetch), key width / value kind / minimizer window as template arguments (with_w, with_w_ext,
 * with_win), the sizes of a value and the set-up of a finalized map (value_words, image_value_bytes, alloc_map_arrays,
 * sort_map_buckets), kernel-argument structs (reads_view, finalize_params, count_out, sk_own_lists), the plan of the count pass over
 * super-k-mer lists (sk_count_uniform, sk_count_select), the entry buffers' policy and the attempt loop of a count pass (count_entry_buffers,
 * count_attempts), the end of a finalize (publish_maps), the host-to-device piece pipeline (tb_feed_pieces), what a feed call hands down
 * (FeedHints) and its one way into the build (add_reads_dev_call, the sk_* parts of add_reads_superkmer_t), and what the stages at the
 * end of the file share (CompareSpectrums per read, TnfDistance, KmerMatch, ContigExtender: kmer_slot_plan, stage_run, own_reads_params, kmr_runs.hpp).  The heavy kernel
 * templates are compiled elsewhere (kmr_instances.hpp, kmr_inst.hip); the headers' plain kernels here.
 */
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <unistd.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cctype>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "kmr_host.hpp"
#include "kmr_runs.hpp"
#include "kmr_image_layout.hpp"
#include "kmr_kernels.hpp"
#include "kmr_partition.hpp"
#include "kmr_superkmer.hpp"
#include "kmr_buckets.hpp"
#include "kmr_synth.hpp"
#define KMR_INSTANCES_EXTERN
#include "kmr_instances.hpp"      /* the heavy kernels are compiled in the objects made of kmr_inst.hip */

using namespace kmr;

namespace {


/* diagnostics on stderr and the measurement-only hooks exist in a -DKMR_DEBUG_HOOKS build alone: the shipped library reads no
 * environment variable */
#ifdef KMR_DEBUG_HOOKS
bool dbg() { static const bool d = getenv("KMR_DEBUG") != nullptr; return d; }
#else
constexpr bool dbg() { return false; }
#endif


}  // namespace

namespace kmr_host {

static uint64_t min_pow2(uint64_t n) {   /* BucketExposedMapLogic::getMinPowerOf2, src/Kmer.h:2199-2212 */
	uint64_t p = n;
	if (p == 0) p = 1;
	else if ((p & (p - 1)) != 0) { p--; for (size_t i = 1; i < 64; i <<= 1) p |= p >> i; p++; }
	return p;
}
uint64_t resize_buckets(uint64_t n) { if (n > 67108864ull) n = 67108864ull; return min_pow2(n); }   /* :2224-2229 */

/* Read::initializeQualityToProbability (src/Sequence.cpp:522-540) as a function of the Phred value;
 * the reference rescales reads to base 33 first (ReadSet.cpp:324-337) */
void quality_table(double P[256], unsigned minQ, unsigned startChar) {
	for (int raw = 0; raw < 256; raw++) {
		int i = raw - (int)startChar + 33;
		if (i < 33 + (int)minQ) P[raw] = 0.0;
		else if (i < 103) P[raw] = 1.0 - pow(10.0, ((33 - i) / 10.0));
		else P[raw] = 1.0;
	}
}

}  // namespace kmr_host

namespace {

/* ... and the minimizer window of build_mode 3 (h->sk_win: 32 for keys of two words and more only -- no window-32 instance exists for
 * one-word keys --, 16, 8, anything else behaves as 4) */
template <int W, class F> auto with_win(uint32_t win, F &&f) {
	if (W > 1 && win == 32) return f(int_c<(W > 1 ? 32 : 16)>());
	return win == 16 ? f(int_c<16>()) : (win == 8 ? f(int_c<8>()) : f(int_c<4>()));
}

size_t slot_bytes(kmr_handle *h) { return with_w(h, [](auto W) { return sizeof(Slot<W()>); }); }
/* words of a weak entry's value (count, weight, forward count; with extension values twelve tallies more), and the bytes an entry's value
 * takes in a stored map's image */
uint32_t value_words(const kmr_handle *h) { return h->ext ? 15 : 3; }
uint32_t image_value_bytes(const kmr_handle *h, bool weakMap) { return weakMap ? (h->ext ? 60 : 12) : (h->ext ? 5 : 1); }

/* Kernel-argument structs leave their makers with every field set, a site states only what differs.  reads_view: a batch of reads on
 * the device (no work units: prepare_units cuts them where a read is longer than a tile) */
ReadsView reads_view(const void *bases, const void *quals, const void *offsets, uint64_t n_reads, const void *discarded = nullptr, uint64_t stream_base = 0, uint64_t first_read_idx = 0) {
	ReadsView rv{};
	rv.bases = (const uint8_t *)bases; rv.quals = (const uint8_t *)quals; rv.offsets = (const uint64_t *)offsets; rv.discarded = (const uint8_t *)discarded;
	rv.n_reads = n_reads; rv.stream_base = stream_base; rv.first_read_idx = first_read_idx;
	return rv;
}
/* reads [r, r + m) of a batch (bases and qualities stay: the offsets address them) */
ReadsView reads_slice(const ReadsView &all, uint64_t r, uint64_t m) {
	ReadsView rv = all;
	rv.offsets = all.offsets + r; rv.n_reads = m; rv.discarded = all.discarded ? all.discarded + r : nullptr; rv.first_read_idx = all.first_read_idx + r;
	return rv;
}
FinalizeParams finalize_params(kmr_handle *h, uint32_t min_depth) {
	FinalizeParams f{};      /* (uni_wbits: sk_count_uniform) */
	f.kb = h->hkb; f.ext_min_q = h->cfg.ext_min_quality; f.min_depth = min_depth; f.has_singletons = h->cfg.separate_singletons ? 1 : 0; f.nb_weak = h->nb_weak; f.nb_sing = h->nb_sing;
	return f;
}

DevParams dev_params(kmr_handle *h) {
	DevParams p;
	p.k = h->k; p.kb = h->hkb; p.min_weight = h->cfg.min_weight; p.fastq_start = h->cfg.fastq_start_char; p.ext_min_q = h->cfg.ext_min_quality;
	p.qzero = h->cfg.fastq_start_char + std::max<uint32_t>(1u, h->cfg.min_quality_score);   /* Q0 has probability 0 too */
	p.subsample = h->cfg.kmer_subsample; p.rank = h->cfg.rank; p.world = h->cfg.world_size; p.num_parts = h->cfg.num_parts; p.part_idx = h->cfg.part_idx;
	p.count_sender_bad = 0u;      /* (extract_by_owner_t's build-mode launch sets it) */
	p.P = h->dP.get<double>(); p.stats = h->dstats.get<DevStats>(); p.err = h->derr.get<uint32_t>();
	p.sub_wstart = p.sub_wkeys = p.sub_sstart = p.sub_skeys = nullptr; p.sub_wvals = nullptr; p.sub_sweight = nullptr; p.sub_wnb = p.sub_snb = 0; p.sub_vw = 0;
	if (h->subtract) {
		const kmr_handle *o = h->subtract;
		if (o->weak.present && o->weak.n) { p.sub_wstart = o->weak.start.get<uint64_t>(); p.sub_wkeys = o->weak.keys.get<uint64_t>(); p.sub_wvals = o->weak.vals.get<uint32_t>(); p.sub_wnb = o->weak.nb; p.sub_vw = value_words(o); }
		if (o->sing.present && o->sing.n) { p.sub_sstart = o->sing.start.get<uint64_t>(); p.sub_skeys = o->sing.keys.get<uint64_t>(); p.sub_sweight = o->sing.sweight.get<uint8_t>(); p.sub_snb = o->sing.nb; }
	}
	return p;
}


template <int W> Table<W> table_of(kmr_handle *h) { Table<W> t; t.slots = h->slots.get<Slot<W>>(); t.ext = h->extslots.get<ExtSlot>(); t.log2cap = h->log2cap; return t; }

template <int W> int clear_table(kmr_handle *h, void *slots, ExtSlot *ext, uint32_t log2cap) {
	LAUNCH(h, table_clear_kernel<W>, dim3(grid_for(1ull << log2cap)), dim3(256), 0, (Slot<W> *)slots, ext, 1ull << log2cap);
	return 0;
}
int clear_table_any(kmr_handle *h, void *slots, ExtSlot *ext, uint32_t log2cap) { return with_w(h, [&](auto W) { return clear_table<W()>(h, slots, ext, log2cap); }); }

/* slots (and extension slots) of a cleared table; `slots` and `ext` are replaced only when all of it succeeded */
int alloc_table(kmr_handle *h, uint32_t log2cap, DevBuf &slots, DevBuf &ext) {
	DevBuf s, x;
	HIPCHK(h, s.alloc(slot_bytes(h) << log2cap));
	if (h->ext) HIPCHK(h, x.alloc(sizeof(ExtSlot) << log2cap));
	const int rc = clear_table_any(h, s.get(), x.get<ExtSlot>(), log2cap);
	if (rc) return rc;
	slots = std::move(s); ext = std::move(x);
	return 0;
}

/* read the device error word and counters; synchronises the stream.  with_pool_head: the record pool's head comes back with the same
 * wait (h->l1_head_seen, for a build_csr that follows with no launch in between that takes chunks) */
int sync_state(kmr_handle *h, bool with_pool_head = false) {
	h->l1_head_seen = 0;
	if (with_pool_head && h->l1.head) HIPCHK(h, fetch_queue(h, &h->l1_head_seen, h->l1.head.get<unsigned int>()));
	HIPCHK(h, hipStreamSynchronize(h->stream));
	for (int which = 0; which < KMR_TIME_GROUPS; which++) {
		for (auto &pr : h->pending_events[which]) {
			float ms = 0; hipEventElapsedTime(&ms, pr.first, pr.second);
			h->ms[which] += ms; h->launches[which]++;
			hipEventDestroy(pr.first); hipEventDestroy(pr.second);
		}
		h->pending_events[which].clear();
	}
	uint32_t e = 0; DevStats s;
	HIPCHK(h, hipMemcpy(&e, h->derr.get<uint32_t>(), sizeof(e), hipMemcpyDeviceToHost));
	HIPCHK(h, hipMemcpy(&s, h->dstats.get<DevStats>(), sizeof(s), hipMemcpyDeviceToHost));
#ifdef KMR_DEBUG_HOOKS
	if (h->superkmer_mode) { if (dbg()) fprintf(stderr, "sk_extract windows: %llu general, %llu fast\n", s.claimed, s.inserted); s.claimed = 0; s.inserted = 0; }
#endif
	/* (through the k-mer record exchange: good k-mers are counted where they arrive, bad ones where they were read) */
	h->stats.raw_kmers = s.raw + s.inserted + s.sender_bad; h->stats.raw_good_kmers = s.good + s.inserted; h->stats.discarded = s.raw - s.good + s.sender_bad;
	h->occupied = s.claimed; h->pending_kmers = 0; h->subtracted = s.subtracted;
	h->ord_seen = s.ord_nlo != 0; h->ord_lo = ~s.ord_nlo; h->ord_hi = s.ord_hi;
	if (e & ERR_READ_TOO_LONG) return fail(h, KMR_ERR_UNSUPPORTED, "a read is longer than the per-wavefront LDS tile (" + std::to_string(TILE_SPAN) + " bases)");
	if (e & ERR_TABLE_FULL) return fail(h, KMR_ERR_CAPACITY, "device k-mer table is full; raise kmr_config.max_table_entries / estimated_raw_kmers");
	if (e & ERR_SEGMENT_OVERFLOW) return fail(h, KMR_ERR_CAPACITY, "an owner segment overflowed seg_capacity");
	if (e & ERR_POOL_FULL) return fail(h, KMR_ERR_CAPACITY, "record pool overflow (internal sizing error)");
	if (e & ERR_ENTRIES_FULL) return fail(h, KMR_ERR_CAPACITY, "entry buffer overflow (internal sizing error)");
	return 0;
}

template <int W, bool EXT> int grow_table_t(kmr_handle *h, uint32_t newlog) {
	DevBuf ns, ne;
	int rc = alloc_table(h, newlog, ns, ne);
	if (rc) return rc;
	Table<W> src = table_of<W>(h), dst; dst.slots = ns.get<Slot<W>>(); dst.ext = ne.get<ExtSlot>(); dst.log2cap = newlog;
	LAUNCH(h, (rehash_kernel<W, EXT>), dim3(grid_for(1ull << h->log2cap)), dim3(256), 0, src, dst, h->hkb, h->derr.get<uint32_t>());
	HIPCHK(h, hipStreamSynchronize(h->stream));
	h->slots = std::move(ns); h->extslots = std::move(ne); h->log2cap = newlog;
	return 0;
}
int grow_table(kmr_handle *h, uint32_t newlog) { return with_w_ext(h, [&](auto W, auto EXT) { return grow_table_t<W(), EXT()>(h, newlog); }); }

/* make room for up to 'incoming' new keys: keep the load factor below 0.85 even if all are new */
int ensure_capacity(kmr_handle *h, uint64_t incoming) {
	const uint64_t cap = 1ull << h->log2cap;
	if ((double)(h->occupied + h->pending_kmers + incoming) <= 0.85 * (double)cap) { h->pending_kmers += incoming; return 0; }
	int rc = sync_state(h);          /* learn the true occupancy */
	if (rc) return rc;
	if ((double)(h->occupied + incoming) > 0.85 * (double)cap) {
		uint32_t nl = h->log2cap;
		while ((double)(h->occupied + incoming) > 0.6 * (double)(1ull << nl)) nl++;
		rc = grow_table(h, nl);
		if (rc) return rc;
	}
	h->pending_kmers = incoming;
	return 0;
}

const size_t EXTRACT_SMEM = (size_t)WAVES_PER_BLOCK * 2 * TILE_BUF;

/* If the batch holds reads longer than one LDS tile, cut them into work units (see ReadsView) and point rv at them. */
/* longest: the batch's longest read where the caller has it already (sk_uniform_weight's pass over the qualities takes it along);
 * otherwise it is learned here first, and only a batch that holds a read longer than `span` has its units counted and cut. */
int prepare_units(kmr_handle *h, ReadsView &rv, uint32_t span = (uint32_t)TILE_SPAN, const unsigned int *longest = nullptr) {
	rv.u_start = rv.u_end = rv.u_read = nullptr; rv.n_units = 0;
	const uint64_t n = rv.n_reads;
	if (n == 0) return 0;
	int rc = 0;
	unsigned int mx = 0;
	if (longest) mx = *longest;
	else {
		rc = h->umax.reserve(h, "umax", 4); if (rc) return rc;
		HIPCHK(h, hipMemsetAsync(h->umax.get<unsigned int>(), 0, 4, h->stream));
		LAUNCH(h, unit_max_kernel, dim3(grid_for(n)), dim3(256), 0, rv.offsets, n, h->umax.get<unsigned int>());
		HIPCHK(h, fetch(h, &mx, h->umax.get<unsigned int>()));
	}
	if (mx <= span) return 0;                   /* the usual case: every read is one unit */
	h->unit_batches++;
	rc = h->ucnt.reserve(h, "ucnt", 4 * (n + 1)); if (rc) return rc;
	LAUNCH(h, unit_count_kernel, dim3(grid_for(n)), dim3(256), 0, rv.offsets, n, h->k, span, h->ucnt.get<uint32_t>());
	rc = h->ufirst.reserve(h, "ufirst", 8 * (n + 1)); if (rc) return rc;
	rc = exclusive_scan_queue(h, h->ucnt.get<uint32_t>(), n, h->ufirst.get<uint64_t>()); if (rc) return rc;
	uint64_t U = 0;
	HIPCHK(h, fetch(h, &U, h->ufirst.get<uint64_t>() + n));
	if (h->u_read.cap() < 8 * U) {      /* (u_read is allocated last) */
		h->u_start.reset(); h->u_end.reset(); h->u_read.reset();
		HIPCHK(h, h->u_start.alloc(8 * U)); HIPCHK(h, h->u_end.alloc(8 * U)); HIPCHK(h, h->u_read.alloc(8 * U));
	}
	LAUNCH(h, unit_fill_kernel, dim3(grid_for(n)), dim3(256), 0, rv.offsets, n, h->k, span, h->ufirst.get<uint64_t>(), h->u_start.get<uint64_t>(), h->u_end.get<uint64_t>(), h->u_read.get<uint64_t>());
	rv.u_start = h->u_start.get<uint64_t>(); rv.u_end = h->u_end.get<uint64_t>(); rv.u_read = h->u_read.get<uint64_t>(); rv.n_units = U;
	return 0;
}

template <int W, bool EXT, class Op> int launch_extract(kmr_handle *h, const ReadsView &rv, const DevParams &dp, const Op &op, uint64_t max_blocks = 0) {
	const bool sub = Op::NEEDS_WEIGHT && (dp.sub_wnb | dp.sub_snb) != 0;      /* lookups ignore the subtracting reference */
	auto kern = sub ? extract_kernel<W, EXT, Op, true> : extract_kernel<W, EXT, Op, false>;
	HIPCHK(h, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)EXTRACT_SMEM));
	if (dbg()) { int nb = 0; hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)kern, WAVES_PER_BLOCK * 64, EXTRACT_SMEM); fprintf(stderr, "extract: %d blocks of %d waves per CU (dynamic LDS %zu)\n", nb, WAVES_PER_BLOCK, EXTRACT_SMEM);
		for (size_t tr : {(size_t)79872, (size_t)65536, (size_t)52000, (size_t)38000}) { hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)kern, WAVES_PER_BLOCK * 64, tr); fprintf(stderr, "   with %zu bytes: %d blocks\n", tr, nb); } }
	const uint64_t tiles = ((rv.u_start ? rv.n_units : rv.n_reads) + 63) / 64;
	uint64_t blocks = (tiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
	if (blocks == 0) return 0;
	if (max_blocks && blocks > max_blocks) blocks = max_blocks;      /* wavefronts then walk several tiles */
	if (blocks > 0x7fffffffull) return fail(h, KMR_ERR_INVALID_ARG, "too many reads in one batch");
	LAUNCH(h, kern, dim3((unsigned)blocks), dim3(WAVES_PER_BLOCK * 64), EXTRACT_SMEM, rv, dp, op);
	return 0;
}

template <int W, bool EXT> int add_reads_dev_t(kmr_handle *h, const ReadsView &rvAll, uint64_t total_bases) {
	/* chunks of reads bounded so that a chunk cannot add more than ~2^27 keys between capacity checks */
	const uint64_t n = rvAll.n_reads;
	const uint64_t avg = n ? std::max<uint64_t>(1, total_bases / n) : 1;
	uint64_t chunk = std::max<uint64_t>(64, ((1ull << 27) / avg) & ~63ull);
	std::vector<uint64_t> off2(2);
	for (uint64_t r = 0; r < n; r += chunk) {
		const uint64_t m = std::min(chunk, n - r);
		/* bases in this chunk: read the two boundary offsets */
		HIPCHK(h, fetch_queue(h, &off2[0], rvAll.offsets + r));
		HIPCHK(h, fetch_queue(h, &off2[1], rvAll.offsets + r + m));
		HIPCHK(h, stream_wait(h));
		const uint64_t bases = off2[1] - off2[0];
		int rc = ensure_capacity(h, bases);     /* #k-mers <= #bases */
		if (rc) return rc;
		ReadsView rv = reads_slice(rvAll, r, m);
		rc = prepare_units(h, rv); if (rc) return rc;
		InsertOp<W, EXT> op; op.table = table_of<W>(h);
		TimeSpan t(h, 0);
		rc = launch_extract<W, EXT>(h, rv, dev_params(h), op);
		t.end();
		if (rc) return rc;
	}
	return 0;
}

int add_reads_dev_any(kmr_handle *h, const ReadsView &rv, uint64_t total_bases) { return with_w_ext(h, [&](auto W, auto EXT) { return add_reads_dev_t<W(), EXT()>(h, rv, total_bases); }); }

}  // namespace
namespace kmr_host {
int exclusive_scan_queue(kmr_handle *h, const uint32_t *in, uint64_t n, uint64_t *out /* n+1 */) {
	const uint64_t nblocks = (n + SCAN_ITEMS - 1) / SCAN_ITEMS;
	const size_t eb = sizeof(unsigned long long);
	int rc = h->scan_sums.reserve(h, "scan_sums", eb * (nblocks + 1), eb * std::max<uint64_t>(nblocks + 1, 4096)); if (rc) return rc;
	unsigned long long *sums = h->scan_sums.get<unsigned long long>(), *total = sums + nblocks;
	LAUNCH(h, scan_block_sums_kernel, dim3((unsigned)nblocks), dim3(256), 0, in, n, sums);
	LAUNCH(h, scan_sums_kernel, dim3(1), dim3(256), 0, sums, nblocks, total);
	LAUNCH(h, scan_apply_kernel, dim3((unsigned)nblocks), dim3(256), 0, in, n, sums, out);
	return 0;
}
int exclusive_scan(kmr_handle *h, const uint32_t *in, uint64_t n, uint64_t *out /* n+1 */) {
	const int rc = exclusive_scan_queue(h, in, n, out); if (rc) return rc;
	HIPCHK(h, hipStreamSynchronize(h->stream));
	return 0;
}
}  // namespace kmr_host
namespace {

/* bump allocation out of the finalize arena (256-byte aligned); what does not fit is allocated on the side, freed by
 * arena_reset() and added to the size the arena gets next time */
int arena_alloc(kmr_handle *h, void **out, size_t bytes) {
	const size_t need = (bytes + 255) & ~(size_t)255;
	if (h->arena && h->arena_used + need <= h->arena.cap()) { *out = h->arena.get<uint8_t>() + h->arena_used; h->arena_used += need; h->arena_want += need; return 0; }
	h->arena_want += need;
	DevBuf b;
	HIPCHK(h, b.alloc(std::max<size_t>(need, 256)));
	*out = b.get();
	h->arena_overflow.push_back(std::move(b));
	return 0;
}
/* start of a finalize: everything handed out before is dead (the stream is idle) */
int arena_reset(kmr_handle *h) {
	HIPCHK(h, hipStreamSynchronize(h->stream));
	h->arena_overflow.clear();
	if (h->arena_want > h->arena.cap()) {
		if (h->arena.alloc(h->arena_want + h->arena_want / 8 + (1 << 20)) != hipSuccess) (void)hipGetLastError();
	}
	h->arena_used = 0; h->arena_want = 0;
	return 0;
}
template <class T> int arena_get(kmr_handle *h, T **out, size_t count) { return arena_alloc(h, (void **)out, count * sizeof(T)); }
/* What every kmr_finalize ends with: the maps are the handle's state (has_singletons, entry counts, a new map generation) and the
 * device's error word and counters are read.  The finalize arena's temporaries are dead: if some of them had to be allocated on
 * the side, the arena is brought to size now, so that it is this build (a handle's first) that pays for it and not the next one */
int publish_maps(kmr_handle *h, bool keepSing) {
	h->has_singletons = keepSing;
	h->stats.weak_entries = h->weak.n; h->stats.singleton_entries = keepSing ? h->sing.n : 0;
	h->finalized = true; h->map_gen++;
	int rc = sync_state(h);
	if (!rc && !h->arena_overflow.empty()) rc = arena_reset(h);
	return rc;
}

/* empty the map but keep its buffers */
void clear_map(DevMap &m) { m.image.reset(); m.n = 0; m.present = false; }


template <int W> MapView<W> view_of(const DevMap &m, uint32_t vw) {
	MapView<W> v; v.start = m.start.get<uint64_t>(); v.keys = m.keys.get<uint64_t>(); v.vals = m.vals.get<uint32_t>(); v.sweight = m.sweight.get<uint8_t>(); v.nb = m.present ? m.nb : 0; v.vw = vw;
	return v;
}

/* The arrays of a finalized map of m.n entries, 8 bytes at least each: keys and values of a weak map; keys, weights and, with extension
 * values, packets of a singleton map */
template <int W> int alloc_map_arrays(kmr_handle *h, DevMap &m, bool weakMap) {
	HIPCHK(h, m.keys.alloc(std::max<uint64_t>(8, 8ull * W * m.n)));
	if (weakMap) HIPCHK(h, m.vals.alloc(std::max<uint64_t>(8, 4ull * value_words(h) * m.n)));
	else {
		HIPCHK(h, m.sweight.alloc(std::max<uint64_t>(8, m.n)));
		if (h->ext) HIPCHK(h, m.spkt.alloc(std::max<uint64_t>(8, 4 * m.n)));
	}
	return 0;
}
/* Sort every bucket of a map by key.  The view names the arrays of the map's kind only (a weak map owns no weights or packets, a
 * singleton map no values, and none but a build with extension values packets: their buffers are empty) */
template <int W> int sort_map_buckets(kmr_handle *h, DevMap &m, bool weakMap) {
	SortView<W> sv; sv.keys = m.keys.get<uint64_t>(); sv.vw = weakMap ? value_words(h) : 0;
	sv.vals = weakMap ? m.vals.get<uint32_t>() : nullptr; sv.b8 = weakMap ? nullptr : m.sweight.get<uint8_t>(); sv.pkt = weakMap ? nullptr : m.spkt.get<uint32_t>();
	const dim3 grid(grid_for(m.nb, 4, 1 << 20));
	if (!weakMap) LAUNCH(h, (sort_buckets_kernel<W, 0>), grid, dim3(256), 0, sv, m.start.get<uint64_t>(), m.nb);
	else if (h->ext) LAUNCH(h, (sort_buckets_kernel<W, 15>), grid, dim3(256), 0, sv, m.start.get<uint64_t>(), m.nb);
	else LAUNCH(h, (sort_buckets_kernel<W, 3>), grid, dim3(256), 0, sv, m.start.get<uint64_t>(), m.nb);
	return 0;
}

template <int W, bool EXT> int finalize_t(kmr_handle *h, uint32_t min_depth) {
	int rc = sync_state(h);
	if (rc) return rc;
	TimeSpan whole(h, KMR_TIME_FINALIZE);
	const FinalizeParams f = finalize_params(h, min_depth);
	const bool keepSing = f.has_singletons && min_depth <= 1;
	DevBuf wcb, scb, fcb;
	HIPCHK(h, wcb.alloc(4 * h->nb_weak)); HIPCHK(h, scb.alloc(4 * h->nb_sing)); HIPCHK(h, fcb.alloc(sizeof(FinalizeCounters)));
	uint32_t *wc = wcb.get<uint32_t>(), *sc = scb.get<uint32_t>(); FinalizeCounters *fc = fcb.get<FinalizeCounters>();
	HIPCHK(h, hipMemsetAsync(wc, 0, 4 * h->nb_weak, h->stream)); HIPCHK(h, hipMemsetAsync(sc, 0, 4 * h->nb_sing, h->stream)); HIPCHK(h, hipMemsetAsync(fc, 0, sizeof(FinalizeCounters), h->stream));
	Table<W> t = table_of<W>(h);
	const int g = grid_for(1ull << h->log2cap);
	LAUNCH(h, classify_kernel<W>, dim3(g), dim3(256), 0, t, f, wc, sc, fc);
	FinalizeCounters c;
	HIPCHK(h, fetch(h, &c, fc));
	h->stats.unique_kmers = c.unique;
	/* singletonKmers only moves inside the hasSingletons branches of append() (src/KmerSpectrum.h:1625,1649) */
	h->stats.singleton_kmers = f.has_singletons ? c.singletons : 0;
	DevMap &wm = h->weak, &sm = h->sing;
	wm = DevMap(); sm = DevMap();
	wm.nb = h->nb_weak; wm.n = c.weak_kept; wm.present = true;
	sm.nb = h->nb_sing; sm.n = c.sing_kept; sm.present = keepSing;
	HIPCHK(h, wm.start.alloc(8 * (wm.nb + 1))); HIPCHK(h, sm.start.alloc(8 * (sm.nb + 1)));
	rc = exclusive_scan(h, wc, wm.nb, wm.start.get<uint64_t>()); if (rc) return rc;
	rc = exclusive_scan(h, sc, sm.nb, sm.start.get<uint64_t>()); if (rc) return rc;
	rc = alloc_map_arrays<W>(h, wm, true); if (rc) return rc;
	rc = alloc_map_arrays<W>(h, sm, false); if (rc) return rc;
	HIPCHK(h, hipMemsetAsync(wc, 0, 4 * h->nb_weak, h->stream)); HIPCHK(h, hipMemsetAsync(sc, 0, 4 * h->nb_sing, h->stream));
	LAUNCH(h, (scatter_kernel<W, EXT>), dim3(g), dim3(256), 0, t, f, wm.start.get<uint64_t>(), wc, wm.keys.get<uint64_t>(), wm.vals.get<uint32_t>(), sm.start.get<uint64_t>(), sc, sm.keys.get<uint64_t>(), sm.sweight.get<uint8_t>(), sm.spkt.get<uint32_t>());
	rc = sort_map_buckets<W>(h, wm, true); if (rc) return rc;
	if (sm.n) { rc = sort_map_buckets<W>(h, sm, false); if (rc) return rc; }
	whole.end();
	HIPCHK(h, hipStreamSynchronize(h->stream));
	/* the table allocation is kept for kmr_reset(); kmr_release_table() frees it */
	if (!keepSing) { sm.n = 0; }
	return publish_maps(h, keepSing);
}

template <int W> int build_image_t(kmr_handle *h, DevMap &m, bool weakMap) {
	if (m.image) return 0;
	const uint32_t vw = value_words(h), vbytes = image_value_bytes(h, weakMap);
	HIPCHK(h, m.image.alloc(8 * (2 + m.nb) + 4 * m.nb + m.n * (h->kb + vbytes)));
	LAUNCH(h, image_header_kernel, dim3(grid_for(m.nb)), dim3(256), 0, m.image.get<uint8_t>(), m.start.get<uint64_t>(), m.nb, h->kb, vbytes);
	if (m.n) LAUNCH(h, image_entries_kernel<W>, dim3(grid_for(m.n)), dim3(256), 0, m.image.get<uint8_t>(), m.start.get<uint64_t>(), m.nb, h->kb, vbytes,
	               m.keys.get<uint64_t>(), weakMap ? m.vals.get<uint32_t>() : nullptr, vw, m.sweight.get<uint8_t>(), m.spkt.get<uint32_t>(), m.n);
	HIPCHK(h, hipStreamSynchronize(h->stream));
	return 0;
}
int build_image(kmr_handle *h, DevMap &m, bool weakMap) { return with_w(h, [&](auto W) { return build_image_t<W()>(h, m, weakMap); }); }

/* A stored map becomes the map `out`.  The layout is checked on the host first (kmr_image_layout.hpp), before any kernel follows an
 * offset or a count of it, and the map is built on the side: `out` changes only once the check, every allocation and every launch
 * have succeeded, so a refused or failed load leaves the map it was to replace as it was. */
template <int W> int load_image_t(kmr_handle *h, DevMap &out, bool weakMap, const uint8_t *src, uint64_t len) {
	const uint32_t vw = value_words(h), vbytes = image_value_bytes(h, weakMap);
	const kmr_host::ImageLayout lay = kmr_host::check_image_layout(src, len, h->kb, vbytes);
	if (lay.reason) return fail(h, KMR_ERR_INVALID_ARG, lay.reason);
	const uint64_t nb = lay.nb;
	DevMap m;
	m.nb = nb; m.n = lay.n; m.present = true;
	HIPCHK(h, m.image.alloc(len));
	HIPCHK(h, hipMemcpy(m.image.get<uint8_t>(), src, len, hipMemcpyHostToDevice));
	{
		DevBuf counts; HIPCHK(h, counts.alloc(4 * nb));
		LAUNCH(h, image_counts_kernel, dim3(grid_for(nb)), dim3(256), 0, m.image.get<uint8_t>(), nb, counts.get<uint32_t>());
		HIPCHK(h, m.start.alloc(8 * (nb + 1)));
		int rc = exclusive_scan(h, counts.get<uint32_t>(), nb, m.start.get<uint64_t>()); if (rc) return rc;
	}
	int rc = alloc_map_arrays<W>(h, m, weakMap); if (rc) return rc;
	if (m.n) LAUNCH(h, image_unpack_kernel<W>, dim3(grid_for(m.n)), dim3(256), 0, m.image.get<uint8_t>(), m.start.get<uint64_t>(), nb, h->kb, vbytes, m.keys.get<uint64_t>(), m.vals.get<uint32_t>(), vw, m.sweight.get<uint8_t>(), m.spkt.get<uint32_t>(), m.n);
	/* restore() accepts unsorted buckets (setLastSorted); lookups here need them sorted */
	rc = sort_map_buckets<W>(h, m, weakMap); if (rc) return rc;
	HIPCHK(h, hipStreamSynchronize(h->stream));
	m.image.reset();    /* rebuilt (sorted) on demand */
	out = std::move(m);
	return 0;
}

/* union of the handle's map with a stored map of the same shape (see merge_copy_kernel) */
template <int W> int merge_image_t(kmr_handle *h, DevMap &m, bool weakMap, const uint8_t *src, uint64_t len) {
	DevMap t;
	int rc = load_image_t<W>(h, t, weakMap, src, len);
	if (rc) return rc;
	if (t.nb != m.nb) return fail(h, KMR_ERR_INVALID_ARG, "Can not merge two maps of differing sizes (src/Kmer.h:3210)");
	const uint32_t vw = value_words(h);
	DevMap d; d.nb = m.nb; d.n = m.n + t.n; d.present = true;
	DevBuf countsb, dupb;
	HIPCHK(h, countsb.alloc(4 * m.nb)); HIPCHK(h, dupb.alloc(4));
	uint32_t *counts = countsb.get<uint32_t>(), *dup = dupb.get<uint32_t>();
	HIPCHK(h, hipMemsetAsync(dup, 0, 4, h->stream));
	HIPCHK(h, d.start.alloc(8 * (m.nb + 1)));
	LAUNCH(h, merge_counts_kernel, dim3(grid_for(m.nb)), dim3(256), 0, m.start.get<uint64_t>(), t.start.get<uint64_t>(), m.nb, counts);
	rc = exclusive_scan(h, counts, m.nb, d.start.get<uint64_t>()); if (rc) return rc;
	rc = alloc_map_arrays<W>(h, d, weakMap); if (rc) return rc;
	if (m.n) LAUNCH(h, merge_copy_kernel<W>, dim3(grid_for(m.n)), dim3(256), 0, m.start.get<uint64_t>(), t.start.get<uint64_t>(), false, m.nb, m.n, m.keys.get<uint64_t>(), weakMap ? m.vals.get<uint32_t>() : nullptr, vw, m.sweight.get<uint8_t>(), m.spkt.get<uint32_t>(), d.start.get<uint64_t>(), d.keys.get<uint64_t>(), d.vals.get<uint32_t>(), d.sweight.get<uint8_t>(), d.spkt.get<uint32_t>());
	if (t.n) LAUNCH(h, merge_copy_kernel<W>, dim3(grid_for(t.n)), dim3(256), 0, t.start.get<uint64_t>(), m.start.get<uint64_t>(), true, m.nb, t.n, t.keys.get<uint64_t>(), weakMap ? t.vals.get<uint32_t>() : nullptr, vw, t.sweight.get<uint8_t>(), t.spkt.get<uint32_t>(), d.start.get<uint64_t>(), d.keys.get<uint64_t>(), d.vals.get<uint32_t>(), d.sweight.get<uint8_t>(), d.spkt.get<uint32_t>());
	rc = sort_map_buckets<W>(h, d, weakMap); if (rc) return rc;
	LAUNCH(h, duplicate_keys_kernel<W>, dim3(grid_for(d.nb)), dim3(256), 0, d.start.get<uint64_t>(), d.nb, d.keys.get<uint64_t>(), dup);
	uint32_t hdup = 0;
	HIPCHK(h, fetch(h, &hdup, dup));
	/* (a k-mer in both singleton maps would have to be promoted into the weak map: KmerMap::mergePromote, which the reference
	 * itself refuses -- "This method is broken", src/Kmer.h:2675-2677) */
	if (hdup && !weakMap) return fail(h, KMR_ERR_UNSUPPORTED, "the two singleton maps share k-mers: merging them means promoting those into the weak map (mergePromote, which the reference refuses too)");
	if (hdup) {      /* mergeAdd proper: the k-mers both maps hold add their values */
		DevMap d2; d2.nb = d.nb; d2.present = true;
		LAUNCH(h, merge_distinct_kernel<W>, dim3(grid_for(d.nb)), dim3(256), 0, d.start.get<uint64_t>(), d.nb, d.keys.get<uint64_t>(), counts);
		HIPCHK(h, d2.start.alloc(8 * (d.nb + 1)));
		rc = exclusive_scan(h, counts, d.nb, d2.start.get<uint64_t>()); if (rc) return rc;
		HIPCHK(h, fetch(h, &d2.n, d2.start.get<uint64_t>() + d.nb));
		rc = alloc_map_arrays<W>(h, d2, true); if (rc) return rc;
		LAUNCH(h, merge_add_kernel<W>, dim3(grid_for(d.nb)), dim3(256), 0, d.start.get<uint64_t>(), d.nb, d.keys.get<uint64_t>(), d.vals.get<uint32_t>(), vw, d2.start.get<uint64_t>(), d2.keys.get<uint64_t>(), d2.vals.get<uint32_t>());
		HIPCHK(h, hipStreamSynchronize(h->stream));
		d = std::move(d2);
	}
	m = std::move(d);
	return 0;
}

/* packed host keys -> counts (u32) or weights (f64, getCount(kmer, true)); exactly one of the two outputs is given */
template <int W> int lookup_t(kmr_handle *h, const uint8_t *packed, uint64_t n, uint32_t *counts, double *weights = nullptr) {
	const uint64_t ob = counts ? 4 : 8;
	DevBuf dk, dc;
	HIPCHK(h, dk.alloc(std::max<uint64_t>(8, n * h->kb))); HIPCHK(h, dc.alloc(std::max<uint64_t>(8, ob * n)));
	HIPCHK(h, hipMemcpyAsync(dk.get(), packed, n * h->kb, hipMemcpyHostToDevice, h->stream));
	const uint32_t vw = value_words(h);
	LAUNCH(h, lookup_keys_kernel<W>, dim3(grid_for(n)), dim3(256), 0, view_of<W>(h->weak, vw), view_of<W>(h->sing, vw), dk.get<uint8_t>(), n, h->hkb,
	       counts ? dc.get<uint32_t>() : nullptr, counts ? nullptr : dc.get<double>());
	HIPCHK(h, hipMemcpyAsync(counts ? (void *)counts : (void *)weights, dc.get(), ob * n, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, hipStreamSynchronize(h->stream));
	return 0;
}

/* the lookup accelerator of the current weak map (built on first use after the map changed); slots == nullptr when it cannot
 * be had (no memory): the callers then search the buckets */
template <int W> LutView<W> lut_of(kmr_handle *h) {
	LutView<W> v; v.slots = nullptr; v.mask = 0; v.shift = 0;
	if (h->tune.no_lut || !h->weak.present || h->weak.n == 0) return v;
	if (!(h->lut && h->lut_gen == h->map_gen)) {
		uint32_t l2 = 10; while ((1ull << l2) < 2 * h->weak.n) l2++;
		const size_t bytes = (size_t)(W + 1) * 8 << l2;
		if (h->lut.cap() < bytes) {
			if (h->lut) { hipStreamSynchronize(h->stream); h->lut.reset(); }
			size_t fr = 0, tot = 0;
			if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < bytes + (1ull << 30) || h->lut.alloc(bytes) != hipSuccess) { (void)hipGetLastError(); return v; }
		}

		const uint32_t vw = value_words(h);
		if (launch_status(h->stream, lut_clear_kernel, dim3(4096), dim3(256), 0, h->lut.get<uint64_t>(), 1ull << l2, (uint32_t)(W + 1)) != hipSuccess) return v;
		if (launch_status(h->stream, lut_build_kernel<W>, dim3(grid_for(h->weak.n)), dim3(256), 0, view_of<W>(h->weak, vw), h->weak.n, h->lut.get<uint64_t>(), (1ull << l2) - 1, 64 - l2, h->hkb) != hipSuccess) return v;
		h->lut_log2 = l2; h->lut_gen = h->map_gen;
	}
	v.slots = h->lut.get<uint64_t>(); v.mask = (1ull << h->lut_log2) - 1; v.shift = 64 - h->lut_log2;
	return v;
}

template <int W> int lookup_reads_t(kmr_handle *h, const ReadsView &rv, uint32_t *dout, const uint64_t *dout_off, bool weak_only = false) {
	LookupOp<W> op; const uint32_t vw = value_words(h); op.weak_only = weak_only;
	op.lut = weak_only ? lut_of<W>(h) : LutView<W>{nullptr, 0, 0};
	op.weak = view_of<W>(h->weak, vw); op.sing = view_of<W>(h->sing, vw); op.out = dout; op.out_offsets = dout_off; op.first_read_idx = rv.first_read_idx;
	return launch_extract<W, false>(h, rv, dev_params(h), op);
}
template <int W> int lookup_reads_weighted_t(kmr_handle *h, const ReadsView &rv, double *dout, const uint64_t *dout_off) {
	LookupWeightOp<W> op; const uint32_t vw = value_words(h);
	op.weak = view_of<W>(h->weak, vw); op.sing = view_of<W>(h->sing, vw); op.out = dout; op.out_offsets = dout_off; op.first_read_idx = rv.first_read_idx;
	return launch_extract<W, false>(h, rv, dev_params(h), op);
}

/* stage host read arrays on the device (padded so 16-byte tile loads stay inside the allocation) */
int stage_reads(kmr_handle *h, const char *bases, const uint64_t *offsets, uint64_t n, DevBuf &b, DevBuf &o) {
	const uint64_t total = n ? offsets[n] - offsets[0] : 0;
	HIPCHK(h, b.alloc(total + 64)); HIPCHK(h, o.alloc(8 * (n + 1)));
	HIPCHK(h, hipMemcpyAsync(b.get(), bases + (n ? offsets[0] : 0), total, hipMemcpyHostToDevice, h->stream));
	std::vector<uint64_t> rel(n + 1);
	for (uint64_t i = 0; i <= n; i++) rel[i] = n ? offsets[i] - offsets[0] : 0;
	HIPCHK(h, hipMemcpyAsync(o.get(), rel.data(), 8 * (n + 1), hipMemcpyHostToDevice, h->stream));
	HIPCHK(h, hipStreamSynchronize(h->stream));   /* rel[] goes out of scope */
	return 0;
}


/* ---------------------------------------------------------------------- */
/* streaming build path (kmr_partition.hpp)                                  */
#define TARGET_LIST_RECORDS (h->tune.target_list)      /* records per final list the partition bits aim for (kmr_tune "target_list_records") */
const double MAX_LIST_DISTINCT = 600.0;       /* distinct keys per final list the 1024-slot table takes comfortably (limit 819) */
const uint64_t L2_ITEM_CHUNKS = 16384;       /* level-2 work item = up to 1M records of one level-1 list */
const uint64_t SUB_BATCH_BASES = 1ull << 30;      /* linear records of one sub-batch: <= 17 GB at 16 bytes; 2^28 cost 2 ms per C2 step in launch tails */

size_t rec_bytes(kmr_handle *h) { return h->superkmer_mode ? 16 : 8 * h->W + (h->ext ? 16 : 8); }      /* Record<W> / RecordX<W>; a 16-byte granule of a super-k-mer record */
/* entries an entry buffer of the count pass holds: keys apart from their values (uw_* / us_*), or packed with a value word (ue, ue2, early.ue) */
uint64_t key_entries(kmr_handle *h, const DevBuf &keys) { return keys.cap() / (8ull * h->W); }
uint64_t packed_entries(kmr_handle *h, const DevBuf &ue) { return ue.cap() / (8ull * (h->W + 1)); }
/* partition kernel shape: one 1024-thread block per compute unit, 8 records per thread per batch, a
 * 4-record write-combining line per list in LDS (see partition_direct_kernel) */
/* (PD_THREADS, PD_RPT, PD_LINE and COUNT_LOG2S: kmr_instances.hpp) */
/* partition bits per level that keep the per-list book-keeping and lines inside the 160 KB of LDS */
int max_part_bits(kmr_handle *h) { return rec_bytes(h) <= 24 ? 10 : 9; }
PoolView pool_view(kmr_handle *h, HostPool &p) { PoolView v; v.base = p.base.get<uint8_t>(); v.chunk_list = p.chunk_list.get<uint32_t>(); v.chunk_count = p.chunk_count.get<uint32_t>(); v.head = p.head.get<unsigned int>(); v.cap = p.cap; v.err = h->derr.get<uint32_t>(); return v; }
/* log2 of the weak map's bucket count: the partition is cut along the bucket index (part_order) */
uint32_t part_rot(kmr_handle *h) { uint32_t r = 0; while ((1ull << (r + 1)) <= h->nb_weak) r++; return r; }
template <int W, bool EXT, int LEVEL> int launch_partition(kmr_handle *h, const PartSource<W> &S, HostPool &pool, int grid, int bits, int shift) {
	auto kern = partition_direct_kernel<W, EXT, LEVEL, PD_THREADS, PD_RPT, PD_LINE>;
	const size_t smem = partition_direct_smem_bytes<W, EXT, PD_THREADS, PD_RPT, PD_LINE>(bits);
	if (dbg()) fprintf(stderr, "partition level %d W=%d bits=%d shift=%d smem=%zu grid=%d\n", LEVEL, W, bits, shift, smem, grid);
	HIPCHK(h, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
	                              (int)partition_direct_smem_bytes<W, EXT, PD_THREADS, PD_RPT, PD_LINE>(max_part_bits(h))));
	LAUNCH(h, kern, dim3(grid), dim3(PD_THREADS), smem, S, pool_view(h, pool), h->work_counter.get<unsigned int>(), bits, shift);
	return 0;
}

/* make sure the pool can take 'extra' more chunks (keeps the used prefix when it has to move) */
int pool_reserve(kmr_handle *h, HostPool &p, uint64_t extra, bool keep) {
	unsigned int used = 0;
	if (!keep) p.used_ub = 0;
	if (p.head && keep) {
		/* the host keeps an upper bound of the chunks handed out so far (every launch adds what it reserved); only
		 * when that bound no longer fits is the stream drained and the real allocator head read back */
		if (p.base && p.used_ub + extra + 64 <= p.cap) { p.used_ub += extra; return 0; }
		HIPCHK(h, hipStreamSynchronize(h->stream)); HIPCHK(h, hipMemcpy(&used, p.head.get<unsigned int>(), 4, hipMemcpyDeviceToHost)); if (used > p.cap) used = p.cap;
	}
	p.used_ub = (uint64_t)used + extra;
	const uint64_t need = (uint64_t)used + extra + 64;
	if (need >= 0xffffffffull) return fail(h, KMR_ERR_CAPACITY, "record pool would exceed 2^32 chunks");
	if (!p.head) { HIPCHK(h, p.head.alloc(4)); HIPCHK(h, hipMemset(p.head.get(), 0, 4)); }
	if (!keep) HIPCHK(h, hipMemsetAsync(p.head.get<unsigned int>(), 0, 4, h->stream));
	if (need <= p.cap) return 0;
	uint64_t ncap = keep && used ? need + need / 4 : need;
	if (p.presize && need + p.presize < 0xffffffffull) ncap = std::max(ncap, need + p.presize);
	p.presize = 0;
	p.chunk_bytes = (size_t)CH * rec_bytes(h);
	DevBuf nb, nl, nc;
	HIPCHK(h, nb.alloc(ncap * p.chunk_bytes));
	HIPCHK(h, nl.alloc(4 * ncap)); HIPCHK(h, nc.alloc(4 * ncap));
	if (used) {
		HIPCHK(h, hipMemcpy(nb.get(), p.base.get(), (size_t)used * p.chunk_bytes, hipMemcpyDeviceToDevice));
		HIPCHK(h, hipMemcpy(nl.get(), p.chunk_list.get(), 4ull * used, hipMemcpyDeviceToDevice));
		HIPCHK(h, hipMemcpy(nc.get(), p.chunk_count.get(), 4ull * used, hipMemcpyDeviceToDevice));
		/* device-to-device copies may return before they have run: the sources are freed next */
		HIPCHK(h, hipDeviceSynchronize());
	}
	p.base = std::move(nb); p.chunk_list = std::move(nl); p.chunk_count = std::move(nc); p.cap = (uint32_t)ncap;
	return 0;
}


int zero_work_counter(kmr_handle *h) {
	int rc = h->work_counter.reserve(h, "work_counter", 4); if (rc) return rc;
	HIPCHK(h, hipMemsetAsync(h->work_counter.get<unsigned int>(), 0, 4, h->stream));
	return 0;
}

}  // namespace
namespace kmr_host {
int num_cus(kmr_handle *h) {
	if (h->ncu <= 0) {
		hipDeviceProp_t pr; h->ncu = 256;
		if (hipGetDeviceProperties(&pr, h->device) == hipSuccess) h->ncu = pr.multiProcessorCount;
	}
	return h->ncu;
}
}  // namespace kmr_host
namespace {
int part_grid(kmr_handle *h) { return num_cus(h) * 2; }
/* the partition kernel wants a compute unit to itself: every (block, list) pair is a write stream, and the fewer of
 * those there are the longer the runs each batch appends */
int partition_blocks(kmr_handle *h) { return h->tune.part_blocks > 0 ? h->tune.part_blocks : num_cus(h); }

/* per-block level-1 state, allocated (and emptied) on first use */
template <int W, bool EXT> int ensure_l1_state(kmr_handle *h) {
	const size_t stride = partition_state_bytes<W, EXT, PD_LINE>(h->bits1), need = stride * (size_t)partition_blocks(h);
	if (h->l1_state.cap() == need) return 0;
	if (h->l1_state) HIPCHK(h, hipStreamSynchronize(h->stream));
	HIPCHK(h, h->l1_state.alloc(need));
	LAUNCH(h, partition_state_init_kernel, dim3(partition_blocks(h)), dim3(256), 0, h->l1_state.get<uint8_t>(), stride, h->bits1, (uint32_t)partition_blocks(h));
	h->l1_state_dirty = false;
	return 0;
}
/* last level-1 launch of a build: no input, every block flushes what it kept back */
template <int W, bool EXT> int flush_l1_state(kmr_handle *h) {
	if (!h->l1_state || !h->l1_state_dirty) return 0;
	int rc = pool_reserve(h, h->l1, (uint64_t)partition_blocks(h) * ((1ull << h->bits1) + 512) + 64, true); if (rc) return rc;
	rc = zero_work_counter(h); if (rc) return rc;
	PartSource<W> S; memset(&S, 0, sizeof(S));
	S.kb = h->hkb; S.rot = part_rot(h); S.state = h->l1_state.get<uint8_t>(); S.state_final = 1;
	rc = launch_partition<W, EXT, 1>(h, S, h->l1, partition_blocks(h), h->bits1, 0);
	h->l1_state_dirty = false;
	return rc;
}

/* level-1 partition of a linear record buffer into h->l1 */
template <int W, bool EXT> int partition_level1(kmr_handle *h, const void *linear, const uint64_t *ext_start, const uint32_t *ext_count,
                                      uint64_t n_ext, uint32_t ext_stride, uint64_t ext_len, uint64_t total, uint64_t max_records,
                                      unsigned long long *valid_counter = nullptr, uint32_t packed_words = 0, uint64_t ordinal_base = 0) {
	if (n_ext == 0) return 0;
	const int grid = (int)std::min<uint64_t>(partition_blocks(h), n_ext);
	if (!h->l1.base) {
		const uint64_t est = std::max<uint64_t>(max_records, h->cfg.estimated_raw_kmers / std::max<uint32_t>(1, h->cfg.world_size));
		const uint64_t launches = est / std::max<uint64_t>(1, max_records) + 2;
		/* level 2 writes into the same pool (it recycles the chunks it reads): room for its partly filled chunks */
		const uint64_t l2_allowance = (est / CH / L2_ITEM_CHUNKS + (1ull << h->bits1) + 1) * (1ull << max_part_bits(h)) + (uint64_t)part_grid(h) * 512;
		{	/* what only kmr_finalize uses (entry buffers) is dead during a build: released if the pool would not fit beside it */
			const uint64_t chunks = est / CH + launches * (uint64_t)grid * ((1ull << h->bits1) + 512) + 64 + l2_allowance;
			size_t mfree = 0, mtotal = 0;
			if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess && (double)mfree < (double)chunks * CH * rec_bytes(h) * 1.02 + (double)(2ull << 30)) {
				HIPCHK(h, hipStreamSynchronize(h->stream));
				h->uw_keys.reset(); h->uw_vals.reset(); h->us_keys.reset(); h->us_b8.reset(); h->us_pkt.reset(); h->ue.reset(); h->ue2.reset();
			}
		}
		uint64_t want = est / CH + launches * (uint64_t)grid * ((1ull << h->bits1) + 512) + 64 + l2_allowance;
		{	/* with room to spare the pool takes a second copy of the records, so that level 2 can append fresh chunks */
			size_t mfree = 0, mtotal = 0;
			const double twice = (double)(want + est / CH) * CH * rec_bytes(h) * 1.02;
			if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess && twice + (double)(8ull << 30) < (double)mfree * 0.5) want += est / CH;
		}
		int rc0 = pool_reserve(h, h->l1, want, true);
		if (rc0) return rc0;
	}
	int rc = pool_reserve(h, h->l1, max_records / CH + (uint64_t)grid * ((1ull << h->bits1) + 512) + 64, true);
	if (rc) return rc;
	rc = zero_work_counter(h); if (rc) return rc;
	PartSource<W> S; memset(&S, 0, sizeof(S));
	S.linear = linear; S.ext_start = ext_start; S.ext_count = ext_count; S.n_ext = n_ext; S.ext_stride = ext_stride; S.ext_len = ext_len; S.total = total;
	S.valid_counter = valid_counter; S.kb = h->hkb; S.rot = part_rot(h); S.packed_words = packed_words; S.ordinal_base = ordinal_base;
	if (!h->tune.no_l1_state) {
		rc = ensure_l1_state<W, EXT>(h); if (rc) return rc;
		S.state = h->l1_state.get<uint8_t>(); S.state_final = 0; h->l1_state_dirty = true;
	}
	TimeSpan t(h, KMR_TIME_PARTITION1);
	return launch_partition<W, EXT, 1>(h, S, h->l1, grid, h->bits1, 0);
}

void choose_bits1(kmr_handle *h, uint64_t records_hint) {
	/* total bits aim at TARGET_LIST_RECORDS per final list; level 2 takes up to max_part_bits(h) of them.  Two of
	 * those are held back: if most k-mers turn out to be distinct the lists have to be up to 4x smaller (see the
	 * distinct probe, probe_distinct_share). */
	uint64_t est = std::max<uint64_t>(records_hint, h->cfg.estimated_raw_kmers / std::max<uint32_t>(1, h->cfg.world_size));
	const int mb = max_part_bits(h);
	int T = 0; while (T < 2 * mb && (est >> T) > TARGET_LIST_RECORDS) T++;
	h->bits1 = std::max(0, std::min(mb, T + 2 - mb));
}

/* k-mer capacity of every work unit of rv (cut here: prepare_units) -> region of each 64-unit tile in the linear buffer of rec_size-byte
 * records: h->koff, h->linear and h->tile_count are ready for a LinearOp launch, which may write total_cap records in `tiles` tiles */
int linear_regions(kmr_handle *h, ReadsView &rv, size_t rec_size, uint64_t &tiles, uint64_t &total_cap) {
	int rc = prepare_units(h, rv); if (rc) return rc;
	const uint64_t nu = rv.u_start ? rv.n_units : rv.n_reads;
	rc = h->kcap.reserve(h, "kcap", 4 * std::max<uint64_t>(nu + 1, 16)); if (rc) return rc;
	rc = h->koff.reserve(h, "koff", 8 * std::max<uint64_t>(nu + 1, 16)); if (rc) return rc;
	LAUNCH(h, kmer_capacity_kernel, dim3(grid_for(nu)), dim3(256), 0, rv, h->k, h->kcap.get<uint32_t>());
	rc = exclusive_scan(h, h->kcap.get<uint32_t>(), nu, h->koff.get<uint64_t>()); if (rc) return rc;
	HIPCHK(h, hipMemcpy(&total_cap, h->koff.get<uint64_t>() + nu, 8, hipMemcpyDeviceToHost));
	tiles = (nu + 63) / 64;
	rc = h->linear.reserve(h, "linear", rec_size * std::max<uint64_t>(total_cap, 16)); if (rc) return rc;
	return h->tile_count.reserve(h, "tile_count", 4 * std::max<uint64_t>(tiles, 16));
}
/* sender side of the exchange: reads -> linear records (every owner's) -> owner segments */
template <int W, bool EXT> int extract_by_owner_t(kmr_handle *h, const ReadsView &rvAll, uint64_t total_bases, void *dev_records, uint64_t seg_capacity, void *dev_seg_counts, uint32_t *dev_pos = nullptr) {
	const uint64_t n = rvAll.n_reads;
	const uint64_t avg = n ? std::max<uint64_t>(1, total_bases / n) : 1;
	const uint64_t chunk = std::max<uint64_t>(64, (SUB_BATCH_BASES / avg) & ~63ull);
	DevParams dp = dev_params(h);
	dp.count_sender_bad = dev_pos == nullptr ? 1u : 0u;      /* build (not request) mode: the kernel counts what it does not send */
	for (uint64_t r = 0; r < n; r += chunk) {
		const uint64_t m = std::min(chunk, n - r);
		ReadsView rv = reads_slice(rvAll, r, m);
		uint64_t tiles = 0, total_cap = 0;
		int rc = linear_regions(h, rv, sizeof(typename PoolRec<W, EXT>::type), tiles, total_cap); if (rc) return rc;      /* (rec_bytes() is the granule size on a super-k-mer handle) */
		LinearOp<W, EXT, false> op; op.records = (typename PoolRec<W, EXT>::type *)h->linear.get(); op.koff = h->koff.get<uint64_t>(); op.tile_count = h->tile_count.get<uint32_t>(); op.first_read_idx = rv.first_read_idx;
		rc = launch_extract<W, EXT>(h, rv, dp, op); if (rc) return rc;
		rc = zero_work_counter(h); if (rc) return rc;
		const int grid = (int)std::min<uint64_t>((uint64_t)num_cus(h) * 8, tiles);
		/* who owns a k-mer: getDistributedThreadId, or -- a spectrum that was built through the list exchange -- the list of its minimizer */
		OwnerFn of; of.m = 0; of.off = of.win = of.list_bits = 0;
		if (h->superkmer_mode && h->sk_exchange) { of.m = h->sk_m; of.off = h->sk_off; of.win = h->sk_win; of.list_bits = h->sk_bits; }
		auto scatter = dev_pos ? owner_scatter_kernel<W, EXT, true> : owner_scatter_kernel<W, EXT>;      /* (request mode writes positions too) */
		LAUNCH(h, scatter, dim3(grid), dim3(OWNER_THREADS), 0, (const typename PoolRec<W, EXT>::type *)h->linear.get(), h->koff.get<uint64_t>(), h->tile_count.get<uint32_t>(), tiles, h->hkb,
		       h->cfg.world_size, (uint32_t *)dev_records, seg_capacity, (unsigned long long *)dev_seg_counts, h->work_counter.get<unsigned int>(), h->derr.get<uint32_t>(), dev_pos, of);
	}
	return 0;
}

template <int W, bool EXT> int add_reads_partition_t(kmr_handle *h, const ReadsView &rvAll, uint64_t total_bases) {
	const uint64_t n = rvAll.n_reads;
	if (!h->l1.head) choose_bits1(h, total_bases);
	const uint64_t avg = n ? std::max<uint64_t>(1, total_bases / n) : 1;
	const uint64_t sub_bases = h->tune.sub_batch_bases ? h->tune.sub_batch_bases : SUB_BATCH_BASES;
	const uint64_t chunk = std::max<uint64_t>(64, (sub_bases / avg) & ~63ull);
	for (uint64_t r = 0; r < n; r += chunk) {
		const uint64_t m = std::min(chunk, n - r);
		ReadsView rv = reads_slice(rvAll, r, m);
		uint64_t tiles = 0, total_cap = 0;
		int rc = linear_regions(h, rv, rec_bytes(h), tiles, total_cap); if (rc) return rc;
		LinearOp<W, EXT> op; op.records = (typename PoolRec<W, EXT>::type *)h->linear.get(); op.koff = h->koff.get<uint64_t>(); op.tile_count = h->tile_count.get<uint32_t>(); op.first_read_idx = rv.first_read_idx;
		TimeSpan tb(h, KMR_TIME_BUILD), te(h, KMR_TIME_EXTRACT);
		rc = launch_extract<W, EXT>(h, rv, dev_params(h), op);
		te.end();
#ifdef KMR_DEBUG_HOOKS
		if (!rc && getenv("KMR_DEBUG_SAME_TILE")) {
			/* measurement aid (tools/l1_write_side.py): every tile of the level-1 pass reads the records of one of the first N tiles again, i.e. its
			 * input comes out of L2 and only the scatter writes go to HBM -- what the pass would cost if extract fed it from
			 * registers.  The result is not a spectrum. */
			const uint64_t distinct = std::max<uint64_t>(1, strtoull(getenv("KMR_DEBUG_SAME_TILE"), nullptr, 10));
			LAUNCH(h, same_tile_kernel, dim3(grid_for(tiles)), dim3(256), 0, h->koff.get<uint64_t>(), tiles, distinct, total_cap / std::max<uint64_t>(tiles, 1));
		}
#endif
		if (!rc) rc = partition_level1<W, EXT>(h, h->linear.get(), h->koff.get<uint64_t>(), h->tile_count.get<uint32_t>(), tiles, 64, 0, 0, total_cap);
		tb.end();
		if (rc) return rc;
	}
	return 0;
}
int add_reads_partition(kmr_handle *h, const ReadsView &rv, uint64_t total_bases) { return with_w_ext(h, [&](auto W, auto EXT) { return add_reads_partition_t<W(), EXT()>(h, rv, total_bases); }); }

/* chunk CSR of a pool: list_start[nl+1] (device) and list_chunks[n_chunks] (device) */
/* ... by the radix partition of the (list, chunk) pairs (csr_bin_*_kernel in kmr_partition.hpp): four launches, no device atomic per chunk */
int build_csr_partition(kmr_handle *h, HostPool &p, uint64_t nl, uint32_t first, unsigned int used, uint64_t *list_start, uint64_t *list_chunks) {
	const uint32_t width = (uint32_t)((nl + CSRP_BINS - 1) / CSRP_BINS), nbins = (uint32_t)((nl + width - 1) / width);
	uint32_t *bins, *pair_list; uint64_t *pair_val;      /* bins: counts, cursors, starts (+ 1) */
	{ int arc = arena_get(h, &bins, 3 * (size_t)CSRP_BINS + 1); if (arc) return arc; arc = arena_get(h, &pair_list, std::max<unsigned>(used, 1)); if (arc) return arc;
	  arc = arena_get(h, &pair_val, std::max<unsigned>(used, 1)); if (arc) return arc; }
	uint32_t *bin_count = bins, *bin_cursor = bins + CSRP_BINS, *bin_start = bins + 2 * CSRP_BINS;
	const uint32_t *cl = p.chunk_list.get<uint32_t>() + first, *cc = p.chunk_count.get<uint32_t>() + first;
	const unsigned grid = (unsigned)(((uint64_t)used + CSRP_TILE - 1) / CSRP_TILE);
	const uint64_t magic = csrp_magic(width);
	HIPCHK(h, hipMemsetAsync(bin_count, 0, 4 * CSRP_BINS, h->stream));
	if (used) LAUNCH(h, csr_bin_hist_kernel, dim3(grid), dim3(CSRP_THREADS), 0, cl, used, (uint32_t)nl, magic, nbins, bin_count);
	LAUNCH(h, csr_bin_scan_kernel, dim3(1), dim3(CSRP_BINS), 0, bin_count, nbins, bin_start, bin_cursor);
	if (used) LAUNCH(h, csr_bin_scatter_kernel, dim3(grid), dim3(CSRP_THREADS), 0, cl, cc, used, first, (uint32_t)nl, magic, nbins, bin_cursor, pair_list, pair_val);
	HIPCHK(h, hipFuncSetAttribute((const void *)csr_bin_place_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4 * width)));
	LAUNCH(h, csr_bin_place_kernel, dim3(nbins), dim3(CSRP_PLACE_THREADS), 4 * (size_t)width, bin_start, pair_list, pair_val, (uint32_t)nl, width, nbins, list_start, list_chunks);
	return 0;
}
/* head_seen: the pool's head where the caller has it from a wait of its own (sync_state) and nothing has taken a chunk since; without
 * it the head is fetched here, which is this function's only wait. */
int build_csr(kmr_handle *h, HostPool &p, uint64_t nl, uint32_t first, uint64_t **list_start, uint64_t **list_chunks, uint32_t *n_chunks_out, const unsigned int *head_seen = nullptr) {
	unsigned int used = 0;
	if (head_seen) used = *head_seen;
	else HIPCHK(h, fetch(h, &used, p.head.get<unsigned int>()));
	if (used > p.cap) used = p.cap;
	used = used > first ? used - first : 0;            /* only chunks [first, head) are looked at */
	const bool by_partition = h->tune.csr_partition && nl >= 1 && nl <= CSRP_MAX_LISTS;
	h->last_csr_path = by_partition ? 1 : 0; h->last_csr_chunks = used;
	{ int arc = arena_get(h, list_start, nl + 1); if (arc) return arc; arc = arena_get(h, list_chunks, std::max<unsigned>(used, 1)); if (arc) return arc; }
	if (by_partition) { int rc = build_csr_partition(h, p, nl, first, used, *list_start, *list_chunks); if (rc) return rc; }
	else {
		uint32_t *cnt;
		{ int arc = arena_get(h, &cnt, nl); if (arc) return arc; }
		HIPCHK(h, hipMemsetAsync(cnt, 0, 4 * nl, h->stream));
		const unsigned csr_grid = (unsigned)(((uint64_t)used + CSR_THREADS * CSR_ITEMS - 1) / (CSR_THREADS * CSR_ITEMS));
		if (used) LAUNCH(h, chunk_hist_kernel, dim3(csr_grid), dim3(CSR_THREADS), 0, p.chunk_list.get<uint32_t>() + first, used, cnt, (uint32_t)nl);
		int rc = exclusive_scan_queue(h, cnt, nl, *list_start); if (rc) return rc;
		HIPCHK(h, hipMemsetAsync(cnt, 0, 4 * nl, h->stream));
		if (used) LAUNCH(h, chunk_scatter_kernel, dim3(csr_grid), dim3(CSR_THREADS), 0, p.chunk_list.get<uint32_t>() + first, p.chunk_count.get<uint32_t>() + first, used, first, *list_start, cnt, *list_chunks, (uint32_t)nl);
	}
	*n_chunks_out = used;
	if (dbg()) {
		unsigned long long hv[2] = {0, 0};
		DevBuf db; HIPCHK(h, db.alloc(16)); HIPCHK(h, hipMemset(db.get(), 0, 16));
		unsigned long long *d = db.get<unsigned long long>();
		if (used) LAUNCH(h, pool_records_kernel, dim3(grid_for(used)), dim3(256), 0, p.chunk_list.get<uint32_t>(), p.chunk_count.get<uint32_t>(), used, d, d + 1);
		HIPCHK(h, hipStreamSynchronize(h->stream));
		HIPCHK(h, hipMemcpy(hv, d, 16, hipMemcpyDeviceToHost));
		fprintf(stderr, "build_csr: lists %llu chunks %u valid %llu records %llu (expected %llu)\n", (unsigned long long)nl, used, hv[1], hv[0], (unsigned long long)h->stats.raw_good_kmers);
		unsigned long long vv[3] = {0, 0, 0};
		int bits = 0; while ((1ull << bits) < nl) bits++;
		DevBuf vb; HIPCHK(h, vb.alloc(24)); HIPCHK(h, hipMemset(vb.get(), 0, 24));
		unsigned long long *v = vb.get<unsigned long long>();
		PoolView pvw = pool_view(h, p);
		{ int vrc = with_w_ext(h, [&](auto W, auto EXT) -> int { LAUNCH(h, (verify_lists_kernel<W(), EXT()>), dim3(4096), dim3(256), 0, pvw, *list_start, *list_chunks, nl, bits, h->hkb, part_rot(h), v, v + 1, v + 2); return 0; }); if (vrc) return vrc; }
		HIPCHK(h, hipStreamSynchronize(h->stream));
		HIPCHK(h, hipMemcpy(vv, v, 24, hipMemcpyDeviceToHost));
		fprintf(stderr, "verify_lists: records via CSR %llu misfiled %llu zero-weight %llu\n", vv[0], vv[1], vv[2]);
	}
	return 0;
}

int finish_maps_from_entries(kmr_handle *h, uint32_t *wc, uint32_t *sc, uint64_t wslots, uint64_t sslots, uint64_t wn, uint64_t sn, bool keepSing, uint32_t *&overflow, bool weak_uncounted = false, bool fixed_bins = false);
CountOut count_out(kmr_handle *h, bool packed, unsigned long long *cursors, uint32_t *wc, uint32_t *sc, FinalizeCounters *fc);

/* one launch of the count pass over k-mer records: the kernel for (W, EXT, table size, NARROW) with the dynamic LDS it wants;
 * list_filter: 0 every list, 1 / 2 those the narrow tallies can / cannot take */
template <int W, bool EXT, int LOG2S, bool NARROW = false> int launch_count(kmr_handle *h, int grid, const uint64_t *ls, const uint64_t *lc, uint64_t nl, const CountOut &out, const FinalizeParams &f, int list_filter) {
	auto kern = count_kernel<W, EXT, LOG2S, NARROW>;
	const size_t smem = count_smem_bytes<W, EXT, LOG2S, NARROW>();
	HIPCHK(h, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
	LAUNCH(h, kern, dim3(grid), dim3(COUNT_THREADS), smem, pool_view(h, h->l1), ls, lc, nl, out, f, h->work_counter.get<unsigned int>(), list_filter);
	return 0;
}

/* ---- what the counting finalizers (build_mode 2 and 3) share: the entry buffers' policy and the attempt loop (the tail: publish_maps) ---- */

/* what a counting finalize carries from the sizing of its entry buffers to the maps */
struct CountPass {
	FinalizeParams f{}; bool keepSing = false, ext = false;
	bool packed = false;      /* the weak entries packed in h->ue (build_mode 3 without extension values) or keys and values apart in h->uw_*, see count_out */
	uint64_t wcap = 0, scap = 0, wmax = 0, smax = 0;                             /* entry buffers: entries now, upper bounds */
	uint32_t *wc = nullptr, *sc = nullptr; FinalizeCounters *fc = nullptr; unsigned long long *cursors = nullptr;
	FinalizeCounters c{}; unsigned long long cur[2] = {0, 0};                    /* what the count pass reported */
};

/* room the blocks of a count pass leave unused: one partly used output slab of 8192 slots each (the pass over super-k-mer lists: a slab
 * of SK_OSLAB entries per wavefront, four wavefronts a block; blocks_per_cu: what its launch is sized for, sk_count_blocks) */
uint64_t entry_slack(uint64_t slabs) { return slabs * 8192 + 16; }
uint64_t sk_entry_slack(kmr_handle *h, int blocks_per_cu) { return entry_slack((uint64_t)num_cus(h) * (uint64_t)blocks_per_cu); }

/* Entry buffers of the pass over G good k-mers: how many entries to start with (wfirst / sfirst and the slack) and their upper bounds;
 * the per-bucket counts, counters and cursors.  The worst case (every second record a weak entry, or every record a singleton) is
 * 5-10 x what sequencing data produces, and at C4 size it is 70 GB: the buffers start from an estimate and the count pass is simply
 * run again with larger ones if that was not enough (count_attempts).  The pass retires an output slab that cannot take a list's
 * entries whole, so up to (entries of one list - 1) of every slab stay unused: an eighth on top of the bounds.  adopted: after an
 * owner exchange the lists this rank counts hold other ranks' k-mers too -- G only knows this rank's own reads: no upper bound then */
int count_entry_buffers(kmr_handle *h, CountPass &p, uint64_t G, uint64_t slack, uint64_t wfirst, uint64_t sfirst, bool adopted) {
	const uint64_t wbound = p.f.has_singletons ? G / 2 : G, sbound = p.keepSing ? G : 0;
	p.wmax = adopted ? (1ull << 40) : wbound + wbound / 8 + slack; p.smax = p.keepSing ? (adopted ? (1ull << 40) : sbound + sbound / 8 + slack) : 16;
	p.wcap = std::min<uint64_t>(p.wmax, wfirst + slack); p.scap = p.keepSing ? std::min<uint64_t>(p.smax, sfirst + slack) : 16;
	if (h->tune.entry_share >= 0) {       /* kmr_tune "entry_share": start from a given (e.g. hopeless) estimate so that the pass has to run again */
		const uint64_t n = (uint64_t)((double)G * h->tune.entry_share) + 16384;
		p.wcap = std::min<uint64_t>(p.wmax, n); if (p.keepSing) p.scap = std::min<uint64_t>(p.smax, n);
		if (p.packed) h->ue.reset(); else { h->uw_keys.reset(); h->uw_vals.reset(); }
		h->us_keys.reset(); h->us_b8.reset(); h->us_pkt.reset();
	}
	p.wcap = std::max(p.wcap, p.packed ? packed_entries(h, h->ue) : key_entries(h, h->uw_keys)); p.scap = std::max(p.scap, key_entries(h, h->us_keys));
	int rc = arena_get(h, &p.wc, h->nb_weak); if (rc) return rc; rc = arena_get(h, &p.sc, h->nb_sing); if (rc) return rc;
	rc = arena_get(h, &p.fc, 1); if (rc) return rc; rc = arena_get(h, &p.cursors, 2); if (rc) return rc;
	return 0;
}
/* h->uw_keys / h->uw_vals hold n weak entries of vw value words, keys and values apart */
int ensure_weak_apart(kmr_handle *h, uint64_t n, uint32_t vw) {
	if (key_entries(h, h->uw_keys) >= n && h->uw_vals) return 0;
	h->uw_keys.reset(); h->uw_vals.reset();
	HIPCHK(h, h->uw_keys.alloc(8ull * h->W * n)); HIPCHK(h, h->uw_vals.alloc(4ull * vw * n));
	return 0;
}
/* ... and the buffers of a count pass hold p.wcap weak entries in its form and p.scap singletons */
int ensure_entry_buffers(kmr_handle *h, const CountPass &p) {
	if (!p.packed) { const int rc = ensure_weak_apart(h, p.wcap, p.ext ? 15 : 3); if (rc) return rc; }
	else if (packed_entries(h, h->ue) < p.wcap) { h->ue.reset(); HIPCHK(h, h->ue.alloc(8ull * (h->W + 1) * p.wcap)); }
	if (key_entries(h, h->us_keys) < p.scap || !h->us_b8 || (p.ext && !h->us_pkt)) {
		h->us_keys.reset(); h->us_b8.reset(); h->us_pkt.reset();
		HIPCHK(h, h->us_keys.alloc(8ull * h->W * p.scap)); HIPCHK(h, h->us_b8.alloc(p.scap)); if (p.ext) HIPCHK(h, h->us_pkt.alloc(4 * p.scap));
	}
	return 0;
}
/* per-bucket counts, counters and cursors start at zero */
int count_clear(kmr_handle *h, const CountPass &p) {
	HIPCHK(h, hipMemsetAsync(p.wc, 0, 4 * h->nb_weak, h->stream)); HIPCHK(h, hipMemsetAsync(p.sc, 0, 4 * h->nb_sing, h->stream));
	HIPCHK(h, hipMemsetAsync(p.fc, 0, sizeof(FinalizeCounters), h->stream)); HIPCHK(h, hipMemsetAsync(p.cursors, 0, 16, h->stream));
	return 0;
}
/* the counters, the cursors and the device error word with one wait */
int count_read_back(kmr_handle *h, CountPass &p, uint32_t &err) {
	HIPCHK(h, fetch_queue(h, &p.c, p.fc)); HIPCHK(h, fetch_queue(h, p.cur, p.cursors, 2));
	HIPCHK(h, fetch_queue(h, &err, h->derr.get<uint32_t>()));
	HIPCHK(h, stream_wait(h));
	return 0;
}
/* The count pass, run again with doubled entry buffers while they overflow (ERR_ENTRIES_FULL), up to their bounds and eight times at
 * most.  queue(out, repeated, repeat_on) puts one attempt's launches on the stream; it may name error flags in repeat_on that ask for
 * the same attempt again with buffers as they are (both they and the overflow flag are cleared; `repeated` tells it so).
 * make_room() runs before an attempt allocates: what the caller can give back.  h->last_count_attempts: how many attempts it took. */
template <class MakeRoom, class Queue> int count_attempts(kmr_handle *h, CountPass &p, MakeRoom make_room, Queue queue) {
	TimeSpan t(h, KMR_TIME_COUNT);
	bool repeated = false;
	for (int attempt = 0; ; attempt++) {
		h->last_count_attempts = attempt + 1;
		int rc = make_room(); if (rc) return rc;
		rc = ensure_entry_buffers(h, p); if (rc) return rc;
		rc = count_clear(h, p); if (rc) return rc;
		const CountOut out = count_out(h, p.packed, p.cursors, p.wc, p.sc, p.fc);
		rc = zero_work_counter(h); if (rc) return rc;
		uint32_t repeat_on = 0, err = 0;
		rc = queue(out, repeated, repeat_on); if (rc) return rc;
		rc = count_read_back(h, p, err); if (rc) return rc;
		repeated = (err & repeat_on) != 0;
		if (repeated) err &= ~(repeat_on | (uint32_t)ERR_ENTRIES_FULL);
		else if (!(err & ERR_ENTRIES_FULL)) return 0;
		/* still full with the buffers at their bounds (or after the last attempt): the cursors point past the buffers, nothing downstream may use them */
		else if ((p.wcap >= p.wmax && p.scap >= p.smax) || attempt >= 8) return fail(h, KMR_ERR_CAPACITY, "entry buffers of the count pass overflowed at their upper bound (internal sizing error)");
		else {      /* more kept entries than the estimate promised: larger buffers, same pass again */
			err &= ~(uint32_t)ERR_ENTRIES_FULL;
			p.wcap = std::min<uint64_t>(p.wmax, p.wcap * 2); if (p.keepSing) p.scap = std::min<uint64_t>(p.smax, p.scap * 2);
			if (dbg()) fprintf(stderr, "count pass: entry buffers too small, retrying with %llu / %llu\n", (unsigned long long)p.wcap, (unsigned long long)p.scap);
		}
		HIPCHK(h, hipMemcpy(h->derr.get<uint32_t>(), &err, 4, hipMemcpyHostToDevice));
	}
}
/* ---- build_mode 2: the phases of finalize_partition_t ---- */

/* the share of distinct keys, and of distinct keys seen more than once, per record: measured on a sample of level-1 lists */
template <int W, bool EXT> int probe_distinct_share(kmr_handle *h, const uint64_t *ls1, const uint64_t *lc1, uint64_t nl1, uint64_t G, double &distinct_share, double &repeated_share) {
	distinct_share = 1.0; repeated_share = 0.5;
	if (!G) return 0;
	unsigned long long *dpr, hpr[4] = {0, 0, 0, 0};
	const uint32_t n_probes = (uint32_t)std::min<uint64_t>(PROBE_LISTS, nl1);
	const size_t tbytes = 8 * ((size_t)n_probes * PROBE_SLOTS + 4);
	int rc = arena_alloc(h, (void **)&dpr, tbytes); if (rc) return rc;
	HIPCHK(h, hipMemsetAsync(dpr, 0, tbytes, h->stream));
	LAUNCH(h, (distinct_probe_kernel<W, EXT>), dim3(n_probes * PROBE_SPLIT), dim3(256), 0, pool_view(h, h->l1), ls1, lc1, nl1, h->hkb, part_rot(h),
	       (int)h->bits1, n_probes, dpr + 4, dpr);
	HIPCHK(h, fetch(h, hpr, dpr, 4));
	if (hpr[0] >= 256) { distinct_share = std::min(1.0, std::max(0.01, (double)hpr[1] / (double)hpr[0])); repeated_share = std::min(0.5, (double)hpr[2] / (double)hpr[0]); }
	if (dbg()) fprintf(stderr, "distinct probe: %llu records, %llu distinct (%llu repeated) -> shares %.3f %.3f\n", hpr[0], hpr[1], hpr[2], distinct_share, repeated_share);
	return 0;
}
/* partition levels 2, 3, ... until the lists are cut by T bits, max_part_bits a pass; ls / lc: the chunk CSR of the current (finally:
 * the last) level, cur_bits: its bits */
template <int W, bool EXT> int partition_further_levels(kmr_handle *h, uint64_t G, int T, uint64_t *&ls, uint64_t *&lc, int &cur_bits) {
	const int mb = max_part_bits(h);
	uint32_t nch = 0, valid_from = 0;                 /* chunks below valid_from belong to levels that were left behind by a fresh-chunk pass */
	for (int level = 2; cur_bits < T; level++) {
		const int nbits = std::min(mb, T - cur_bits);
		const uint64_t nl_prev = 1ull << cur_bits;
		/* work items: the lists of the previous level, long ones cut into equal items (every item ends with a flush of
		 * partly filled chunks, and a short leftover item would cost as many of those as a full one) */
		std::vector<uint64_t> hs(nl_prev + 1);
		HIPCHK(h, hipMemcpy(hs.data(), ls, 8 * (nl_prev + 1), hipMemcpyDeviceToHost));
		std::vector<uint64_t> ib, ie; std::vector<uint32_t> il;
		for (uint64_t l = 0; l < nl_prev; l++) {
			const uint64_t nc = hs[l + 1] - hs[l];
			if (!nc) continue;
			const uint64_t nit = (nc + L2_ITEM_CHUNKS - 1) / L2_ITEM_CHUNKS, per = (nc + nit - 1) / nit;
			for (uint64_t c = hs[l]; c < hs[l + 1]; c += per) { ib.push_back(c); ie.push_back(std::min(hs[l + 1], c + per)); il.push_back((uint32_t)l); }
		}
		int rc = 0;
		if (ib.empty()) { cur_bits += nbits; rc = build_csr(h, h->l1, 1ull << cur_bits, valid_from, &ls, &lc, &nch); if (rc) return rc; continue; }
		/* The pass writes into the pool it reads.  With room for a second copy of the records it appends fresh chunks
		 * (compact, slab by slab: the faster writes); without, a block recycles the chunks it has just read. */
		const uint64_t partials = ib.size() * (1ull << nbits) + (uint64_t)part_grid(h) * 512 + 64;
		unsigned int head_before = 0;
		HIPCHK(h, hipMemcpy(&head_before, h->l1.head.get<unsigned int>(), 4, hipMemcpyDeviceToHost));
		const bool recycle = h->tune.recycle >= 0 ? h->tune.recycle != 0 : (uint64_t)head_before + G / CH + partials + 64 > h->l1.cap;
		h->l1.used_ub = head_before;
		rc = pool_reserve(h, h->l1, (recycle ? 0 : G / CH) + partials, true); if (rc) return rc;
		uint64_t *dib, *die; uint32_t *dil;
		rc = arena_get(h, &dib, ib.size()); if (rc) return rc; rc = arena_get(h, &die, ie.size()); if (rc) return rc; rc = arena_get(h, &dil, il.size()); if (rc) return rc;
		HIPCHK(h, hipMemcpyAsync(dib, ib.data(), 8 * ib.size(), hipMemcpyHostToDevice, h->stream)); HIPCHK(h, hipMemcpyAsync(die, ie.data(), 8 * ie.size(), hipMemcpyHostToDevice, h->stream));
		HIPCHK(h, hipMemcpyAsync(dil, il.data(), 4 * il.size(), hipMemcpyHostToDevice, h->stream));
		rc = zero_work_counter(h); if (rc) return rc;
		PartSource<W> S; memset(&S, 0, sizeof(S));
		S.src = pool_view(h, h->l1); S.list_chunks = lc; S.item_begin = dib; S.item_end = die; S.item_list = dil; S.n_items = ib.size(); S.kb = h->hkb; S.rot = part_rot(h);
		S.recycle = recycle ? 1 : 0;
		const int grid = (int)std::min<uint64_t>(partition_blocks(h), ib.size());
		if (dbg()) fprintf(stderr, "level %d: %d bits after %d, %zu items, %s\n", level, nbits, cur_bits, ib.size(), recycle ? "recycling chunks" : "fresh chunks");
		{ TimeSpan t(h, KMR_TIME_PARTITION2); rc = launch_partition<W, EXT, 2>(h, S, h->l1, grid, nbits, cur_bits); }
		if (rc) return rc;
		HIPCHK(h, hipStreamSynchronize(h->stream));      /* the host vectors behind the item copies go out of scope */
		cur_bits += nbits;
		/* CSR of the new level: fresh chunks lie behind the old head (what is below keeps the list ids of the level
		 * left behind and is never looked at again); recycled ones anywhere in the range that was valid before */
		if (!recycle) valid_from = head_before;
		rc = build_csr(h, h->l1, 1ull << cur_bits, valid_from, &ls, &lc, &nch); if (rc) return rc;
	}
	return 0;
}
/* the count pass over the nl final lists of G records (count_attempts), with a table of 2^count_log2s slots */
template <int W, bool EXT> int partition_count_pass(kmr_handle *h, CountPass &p, uint64_t G, const uint64_t *ls, const uint64_t *lc, uint64_t nl, int count_log2s) {
	const uint32_t vw = EXT ? 15 : 3;
	/* the linear record buffer is dead during finalize: given back when the entry buffers would not fit beside it */
	auto make_room = [&]() -> int {
		const double need = (key_entries(h, h->uw_keys) < p.wcap ? (8.0 * W + 4.0 * vw) * (double)p.wcap : 0.0) + (key_entries(h, h->us_keys) < p.scap ? (8.0 * W + 1.0) * (double)p.scap : 0.0);
		size_t mfree = 0, mtotal = 0;
		if (need > 0 && h->linear && hipMemGetInfo(&mfree, &mtotal) == hipSuccess && (double)mfree < need + (double)G * 0.3 * (8.0 * W + 12.0) + (double)(2ull << 30)) {
			HIPCHK(h, hipStreamSynchronize(h->stream));
			h->linear.reset();
		}
		return 0;
	};
	auto launches = [&](const CountOut &out) -> int {
		int rc = 0;
		const int grid = (int)std::min<uint64_t>((uint64_t)part_grid(h) * 2, nl);
		if (count_log2s == 11) {
			rc = launch_count<W, EXT, 11>(h, grid, ls, lc, nl, out, p.f, 0); if (rc) return rc;
		} else if (EXT && W == 1 && !h->tune.no_narrow) {
			/* extension values at k <= 32: 16-bit tallies for every list of at most 65 535 records (two blocks per CU), then
			 * the wide table for whatever is longer */
			rc = launch_count<W, EXT, COUNT_LOG2S, true>(h, grid, ls, lc, nl, out, p.f, 1); if (rc) return rc;
			/* is any list longer than the narrow tallies can take?  (the work counter word doubles as the maximum) */
			rc = zero_work_counter(h); if (rc) return rc;
			LAUNCH(h, max_list_chunks_kernel, dim3(grid_for(nl)), dim3(256), 0, ls, nl, h->work_counter.get<unsigned int>());
			unsigned int longest = 0;
			HIPCHK(h, fetch(h, &longest, h->work_counter.get<unsigned int>()));
			rc = zero_work_counter(h); if (rc) return rc;
			if (longest > COUNT_NARROW_CHUNKS) { rc = launch_count<W, EXT, COUNT_LOG2S>(h, std::min(grid, part_grid(h)), ls, lc, nl, out, p.f, 2); if (rc) return rc; }
		} else {
			rc = launch_count<W, EXT, COUNT_LOG2S>(h, grid, ls, lc, nl, out, p.f, 0); if (rc) return rc;
		}
		return 0;
	};
	return count_attempts(h, p, make_room, [&](const CountOut &out, bool, uint32_t &) -> int {
		int rc = launches(out);
#ifdef KMR_DEBUG_HOOKS
		/* debugging aid: the count pass is repeated on the same input and must report the same numbers */
		for (int cr = 0, reps = getenv("KMR_COUNT_CHECK") ? atoi(getenv("KMR_COUNT_CHECK")) : 0; cr < reps && !rc; cr++) {
			uint32_t e = 0;
			rc = count_read_back(h, p, e); if (rc) return rc;
			fprintf(stderr, "count pass %d: unique %llu singletons %llu weak_kept %llu sing_kept %llu slots %llu/%llu\n", cr, (unsigned long long)p.c.unique,
			        (unsigned long long)p.c.singletons, (unsigned long long)p.c.weak_kept, (unsigned long long)p.c.sing_kept, p.cur[0], p.cur[1]);
			rc = count_clear(h, p); if (rc) return rc;
			rc = zero_work_counter(h); if (rc) return rc;
			rc = launches(out);
		}
#endif
		return rc;
	});
}

template <int W, bool EXT> int finalize_partition_t(kmr_handle *h, uint32_t min_depth) {
	int rc = sync_state(h);
	if (rc) return rc;
	TimeSpan whole(h, KMR_TIME_FINALIZE);
	const uint64_t G = h->stats.raw_good_kmers;     /* records in the level-1 pool */
	CountPass p;
	p.f = finalize_params(h, min_depth);
	p.keepSing = p.f.has_singletons && min_depth <= 1;
	p.ext = EXT;
	if (!h->l1.head) { rc = pool_reserve(h, h->l1, 0, false); if (rc) return rc; }
	rc = arena_reset(h); if (rc) return rc;
	rc = flush_l1_state<W, EXT>(h); if (rc) return rc;
	/* level-1 CSR; then that of the current (finally: the last) level */
	uint64_t *ls = nullptr, *lc = nullptr; uint32_t nch = 0;
	rc = build_csr(h, h->l1, 1ull << h->bits1, 0, &ls, &lc, &nch); if (rc) return rc;
	/* Final lists are sized by what the count pass can hold in its LDS table: measure the share of distinct keys
	 * on a sample of level-1 lists, then take enough further bits for ~MAX_LIST_DISTINCT distinct keys per list (and
	 * at most TARGET_LIST_RECORDS records), up to max_part_bits per pass and as many passes as that takes (C2: one,
	 * 10 + 10 bits; C4 with 5 x 10^9 two-word records: 10 + 10 + 2). */
	double distinct_share, repeated_share;
	rc = probe_distinct_share<W, EXT>(h, ls, lc, 1ull << h->bits1, G, distinct_share, repeated_share); if (rc) return rc;
	int T = 0; while (T < 40 && ((G >> T) > TARGET_LIST_RECORDS || (double)(G >> T) * distinct_share > MAX_LIST_DISTINCT)) T++;
	T = std::min(T, 28);                              /* list ids are 32-bit with room to spare */
	int cur_bits = h->bits1;
	rc = partition_further_levels<W, EXT>(h, G, T, ls, lc, cur_bits); if (rc) return rc;
	const uint64_t nl = 1ull << cur_bits;
	const int count_log2s = (!EXT && (double)(G >> cur_bits) * distinct_share > MAX_LIST_DISTINCT) ? 11 : COUNT_LOG2S;      /* with extension tallies 2048 slots do not fit LDS */
	if (dbg()) fprintf(stderr, "count pass: %llu lists of ~%llu records, table 2^%d\n", (unsigned long long)nl, (unsigned long long)(G >> cur_bits), count_log2s);
	/* entry buffers: sized from the probe's shares with 50 % headroom */
	rc = count_entry_buffers(h, p, G, entry_slack((uint64_t)part_grid(h) * 8), (uint64_t)((double)G * (p.f.has_singletons ? repeated_share : distinct_share) * 1.5) + G / 64,
	                         (uint64_t)((double)G * std::max(0.0, distinct_share - repeated_share) * 1.5) + G / 64, false); if (rc) return rc;
	rc = partition_count_pass<W, EXT>(h, p, G, ls, lc, nl, count_log2s); if (rc) return rc;
	h->stats.unique_kmers = p.c.unique;
	h->stats.singleton_kmers = p.f.has_singletons ? p.c.singletons : 0;
	{ TimeSpan t(h, KMR_TIME_BUCKETS); uint32_t *none = nullptr; rc = finish_maps_from_entries(h, p.wc, p.sc, p.cur[0], p.cur[1], p.c.weak_kept, p.c.sing_kept, p.keepSing, none); }      /* (measured bins: nothing is left on the stream) */
	if (rc) return rc;
	whole.end();
	return publish_maps(h, p.keepSing);
}

/* Entries that one of `bins` equal shares of n hashed keys may hold (bins of one capacity, kmr_buckets.hpp): the largest count
 * below the mean, and above it `scale` times six standard deviations of the binomial share (2^-30 a bin), 1/64 of the mean
 * for what the hash is short of uniform, and 16.  scale = 0 leaves the bins less than n together: one of them overflows. */
uint64_t bb_fixed_limit(uint64_t n, uint64_t bins, double scale) {
	const double mean = (double)n / (double)bins;
	return (n - 1) / bins + (uint64_t)(std::max(scale, 0.0) * (6.0 * std::sqrt(mean) + mean / 64.0 + 16.0));
}

/* The weak map out of the count pass's packed entries (h->ue) by the radix partition of kmr_buckets.hpp (COUNT_DIR values).
 * done = false and nothing changed when the geometry does not fit: the caller takes the scatter + per-bucket sort.
 * fixed_bins: bins of one capacity -- everything is left on the stream, `overflow` is the device word the caller reads once the
 * stream is drained (set: the map is void, h->ue overwritten); else, or where the buffers do not fit them, measured bins and
 * overflow = null: nothing is left on the stream. */
template <int W> int binned_buckets_t(kmr_handle *h, uint64_t wslots, uint64_t wn, bool fixed_bins, bool &done, uint32_t *&overflow) {
	done = false; overflow = nullptr;
	DevMap &wm = h->weak;
	const uint64_t nb = wm.nb;
	uint32_t B = 0; while ((1ull << (B + 1)) <= nb) B++;
	if (h->ext || wn < h->tune.binned_min || wn == 0 || (1ull << B) != nb || wslots >= (1ull << 40)) return 0;
	uint32_t g = 0; while (g < std::min<uint32_t>(B, BB_MAX_GROUP_BITS) && (wn >> (B - g)) < 512) g++;
	const uint32_t R = B - g;
	if (R < 1 || R > 2 * BB_MAX_BITS || (wn >> R) > 1024) return 0;
	const uint32_t bits1 = R <= (uint32_t)BB_MAX_BITS ? R : (R + 1) / 2, bits2 = R - bits1;
	const uint64_t bins1 = 1ull << bits1, groups = 1ull << R;
	uint32_t *hist1 = nullptr, *hist2 = nullptr, *pad1 = nullptr; uint64_t *start1 = nullptr, *gstart = nullptr; unsigned long long *cursor = nullptr; unsigned int *dmax = nullptr;
	int rc = 0;
	BbInput in1; in1.entries = h->ue.get<uint64_t>(); in1.seg_start = nullptr; in1.seg_count = nullptr; in1.n_seg = 1; in1.n_slots = wslots; in1.holes = 1; in1.seg_stride = 0;
	auto scatter_grid = [&](uint64_t n_slots) { const uint64_t tiles = (n_slots + BB_TILE - 1) / BB_TILE; return (unsigned)std::min<uint64_t>(tiles, (uint64_t)num_cus(h) * 8); };
	auto scratch = [&](uint64_t entries) { return h->ue2.reserve(h, "ue2", 8ull * (W + 1) * entries); };      /* h->ue2: the other side of the partition's ping-pong */
	auto map_arrays = [&]() -> int {
		int rc2 = wm.keys.reserve(h, "weak map keys", std::max<uint64_t>(8ull * W * wn, 8)); if (rc2) return rc2;
		return wm.vals.reserve(h, "weak map vals", std::max<uint64_t>(12ull * wn, 8));
	};
	/* in_stride, overflow: bins of one capacity (bb_group_kernel) */
	auto group_launch = [&](const uint64_t *entries, const uint64_t *gs, const uint32_t *gc, uint64_t in_stride, const uint32_t *overflow) -> int {
		auto gk = bb_group_kernel<W>;
		HIPCHK(h, hipFuncSetAttribute((const void *)gk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bb_group_smem_bytes<W>()));
		/* the blocks stride over the groups: as many of them as fit the chip at once, so that they all get the same number of groups */
		int per_cu = 0;
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)gk, BB_GROUP_THREADS, bb_group_smem_bytes<W>()) != hipSuccess || per_cu < 1) per_cu = 4;
		if (dbg()) fprintf(stderr, "bb_group<W=%d>: %d blocks per CU, %llu groups\n", W, per_cu, (unsigned long long)groups);
		LAUNCH(h, gk, dim3((unsigned)std::min<uint64_t>(groups, (uint64_t)num_cus(h) * per_cu)), dim3(BB_GROUP_THREADS), bb_group_smem_bytes<W>(), entries, wm.keys.get<uint64_t>(), wm.vals.get<uint32_t>(), gs, gc, groups, g, h->hkb, nb, wm.start.get<uint64_t>(), wn, h->derr.get<uint32_t>(), in_stride, overflow);
		return 0;
	};
	const uint32_t shift1 = B - bits1, shift2 = g;
	/* bins of one capacity: lim1 entries in a first-level bin of stride1 slots (whole tiles: the second level reads it tile by tile),
	 * lim2 entries in a group of stride2 slots; the first level writes h->ue2, a second one back into h->ue */
	const uint64_t lim2 = std::min<uint64_t>(bb_fixed_limit(wn, groups, h->tune.bb_slack_groups), bb_group_cap<W>()), stride2 = std::max<uint64_t>(lim2, 1);
	const uint64_t lim1 = bits2 ? bb_fixed_limit(wn, bins1, h->tune.bb_slack_bins) : 0, stride1 = std::max<uint64_t>((lim1 + BB_TILE - 1) / BB_TILE, 1) * BB_TILE;
	if (fixed_bins && lim1 < (1ull << 32) && (!bits2 || groups * stride2 <= packed_entries(h, h->ue))) {
		uint32_t *fill = nullptr, *ovf = nullptr;      /* fill: [bins1] of the first level, then [groups] of the second when there are two */
		rc = scratch(bits2 ? bins1 * stride1 : groups * stride2); if (rc) return rc;
		rc = map_arrays(); if (rc) return rc;
		rc = arena_get(h, &fill, bits2 ? bins1 + groups : groups); if (rc) return rc;
		rc = arena_get(h, &gstart, groups + 1); if (rc) return rc;
		rc = arena_get(h, &ovf, 1); if (rc) return rc;
		HIPCHK(h, hipMemsetAsync(fill, 0, 4 * (bits2 ? bins1 + groups : groups), h->stream)); HIPCHK(h, hipMemsetAsync(ovf, 0, 4, h->stream));
		auto scatter = [&](const BbInput &in, uint32_t shift, uint32_t bits, uint32_t *f, uint64_t limit, uint64_t stride, uint64_t *out) -> int {
			const unsigned grid = scatter_grid(in.n_slots);
			if (W == 1 && !h->tune.bb_reload) LAUNCH(h, (bb_scatter_fixed_kernel<W, W == 1>), dim3(grid), dim3(BB_THREADS), 0, in, shift, bits, h->hkb, nb, f, (uint32_t)limit, stride, out, ovf);
			else LAUNCH(h, (bb_scatter_fixed_kernel<W, false>), dim3(grid), dim3(BB_THREADS), 0, in, shift, bits, h->hkb, nb, f, (uint32_t)limit, stride, out, ovf);
			return 0;
		};
		uint32_t *gfill = fill;
		if (!bits2) { rc = scatter(in1, shift1, bits1, fill, lim2, stride2, h->ue2.get<uint64_t>()); if (rc) return rc; }
		else {
			rc = scatter(in1, shift1, bits1, fill, lim1, stride1, h->ue2.get<uint64_t>()); if (rc) return rc;
			BbInput in2; in2.entries = h->ue2.get<uint64_t>(); in2.seg_start = nullptr; in2.seg_count = fill; in2.n_seg = (uint32_t)bins1; in2.n_slots = bins1 * stride1; in2.holes = 0; in2.seg_stride = stride1;
			gfill = fill + bins1;
			rc = scatter(in2, shift2, bits2, gfill, lim2, stride2, h->ue.get<uint64_t>()); if (rc) return rc;
		}
		/* the map is dense: a group's entries go where the groups before it end */
		rc = exclusive_scan_queue(h, gfill, groups, gstart); if (rc) return rc;
		rc = group_launch(bits2 ? h->ue.get<uint64_t>() : h->ue2.get<uint64_t>(), gstart, gfill, stride2, ovf); if (rc) return rc;
		overflow = ovf; h->last_bb_path = 2;
		done = true;
		return 0;
	}
	rc = arena_get(h, &hist1, bins1); if (rc) return rc;
	rc = arena_get(h, &start1, bins1 + 1); if (rc) return rc;
	rc = arena_get(h, &cursor, groups); if (rc) return rc;
	rc = arena_get(h, &dmax, 1); if (rc) return rc;
	if (bits2) { rc = arena_get(h, &hist2, groups); if (rc) return rc; rc = arena_get(h, &pad1, bins1); if (rc) return rc; rc = arena_get(h, &gstart, groups + 1); if (rc) return rc; }
	HIPCHK(h, hipMemsetAsync(hist1, 0, 4 * bins1, h->stream)); HIPCHK(h, hipMemsetAsync(dmax, 0, 4, h->stream));
	auto hist_grid = [&](uint64_t n_slots, uint32_t &tpb) { const uint64_t tiles = (n_slots + BB_TILE - 1) / BB_TILE; tpb = (uint32_t)std::max<uint64_t>(1, (tiles + 2047) / 2048); return (unsigned)((tiles + tpb - 1) / tpb); };
	uint32_t tpb = 1; unsigned grid = hist_grid(wslots, tpb);
	LAUNCH(h, bb_hist_kernel<W>, dim3(grid), dim3(BB_THREADS), 0, in1, shift1, bits1, h->hkb, nb, tpb, hist1);
	unsigned int mx = 0;
	if (!bits2) {
		/* one level: its bins are the groups, their scan is where the groups lie in the map */
		LAUNCH(h, bb_pad_kernel, dim3(grid_for(bins1)), dim3(256), 0, (const uint32_t *)hist1, bins1, (uint32_t *)nullptr, dmax);
		HIPCHK(h, fetch_queue(h, &mx, dmax));
		rc = exclusive_scan(h, hist1, bins1, start1); if (rc) return rc;      /* (synchronises) */
		if (mx > bb_group_cap<W>()) return 0;
		rc = scratch(wn); if (rc) return rc;
		LAUNCH(h, bb_cursor_init_kernel, dim3(grid_for(bins1)), dim3(256), 0, (const uint64_t *)start1, bins1, cursor);
		LAUNCH(h, bb_scatter_kernel<W>, dim3(scatter_grid(wslots)), dim3(BB_THREADS), 0, in1, shift1, bits1, h->hkb, nb, cursor, h->ue2.get<uint64_t>());
		rc = map_arrays(); if (rc) return rc;
		rc = group_launch(h->ue2.get<uint64_t>(), start1, hist1, 0, nullptr); if (rc) return rc;
		h->last_bb_path = 1;
		done = true;
		return 0;
	}
	/* two levels: the first one's bins start at tile boundaries (the second level reads them tile by tile) */
	LAUNCH(h, bb_pad_kernel, dim3(grid_for(bins1)), dim3(256), 0, (const uint32_t *)hist1, bins1, pad1, dmax);
	rc = exclusive_scan(h, pad1, bins1, start1); if (rc) return rc;
	uint64_t padded_total = 0;
	HIPCHK(h, hipMemcpy(&padded_total, start1 + bins1, 8, hipMemcpyDeviceToHost));
	rc = scratch(std::max(padded_total, wn)); if (rc) return rc;
	LAUNCH(h, bb_cursor_init_kernel, dim3(grid_for(bins1)), dim3(256), 0, (const uint64_t *)start1, bins1, cursor);
	LAUNCH(h, bb_scatter_kernel<W>, dim3(scatter_grid(wslots)), dim3(BB_THREADS), 0, in1, shift1, bits1, h->hkb, nb, cursor, h->ue2.get<uint64_t>());
	BbInput in2; in2.entries = h->ue2.get<uint64_t>(); in2.seg_start = start1; in2.seg_count = hist1; in2.n_seg = (uint32_t)bins1; in2.n_slots = padded_total; in2.holes = 0; in2.seg_stride = 0;
	HIPCHK(h, hipMemsetAsync(hist2, 0, 4 * groups, h->stream)); HIPCHK(h, hipMemsetAsync(dmax, 0, 4, h->stream));
	grid = hist_grid(padded_total, tpb);
	LAUNCH(h, bb_hist_kernel<W>, dim3(grid), dim3(BB_THREADS), 0, in2, shift2, bits2, h->hkb, nb, tpb, hist2);
	LAUNCH(h, bb_pad_kernel, dim3(grid_for(groups)), dim3(256), 0, (const uint32_t *)hist2, groups, (uint32_t *)nullptr, dmax);
	HIPCHK(h, fetch_queue(h, &mx, dmax));
	rc = exclusive_scan(h, hist2, groups, gstart); if (rc) return rc;
	/* the packed entries the count pass wrote are about to be overwritten (the second level writes where the first one read): a
	 * group too large for the LDS arrays sends the build down the other path BEFORE that */
	if (mx > bb_group_cap<W>() || packed_entries(h, h->ue) < wn) return 0;
	LAUNCH(h, bb_cursor_init_kernel, dim3(grid_for(groups)), dim3(256), 0, (const uint64_t *)gstart, groups, cursor);
	LAUNCH(h, bb_scatter_kernel<W>, dim3(scatter_grid(padded_total)), dim3(BB_THREADS), 0, in2, shift2, bits2, h->hkb, nb, cursor, h->ue.get<uint64_t>());
	rc = map_arrays(); if (rc) return rc;
	rc = group_launch(h->ue.get<uint64_t>(), gstart, hist2, 0, nullptr); if (rc) return rc;
	h->last_bb_path = 1;
	done = true;
	return 0;
}

/* weak_uncounted: the count pass kept no per-bucket counts of the weak entries (wc is scratch): the radix partition of
 * kmr_buckets.hpp needs none, and if it declines they are counted here.  overflow: null when the maps are complete and the stream
 * drained; else (bins of one capacity, binned_buckets_t) everything is on the stream and the caller waits once, for this word */
template <int W> int finish_maps_t(kmr_handle *h, uint32_t *wc, uint32_t *sc, uint64_t wslots, uint64_t sslots, uint64_t wn, uint64_t sn, bool keepSing, uint32_t *&overflow, bool weak_uncounted, bool fixed_bins) {
	const uint32_t vw = value_words(h);
	DevMap &wm = h->weak, &sm = h->sing;
	clear_map(wm); clear_map(sm);          /* the buffers of the previous build are reused when they are large enough */
	wm.nb = h->nb_weak; wm.n = wn; wm.present = true;
	sm.nb = h->nb_sing; sm.n = keepSing ? sn : 0; sm.present = keepSing;
	int rc = wm.start.reserve(h, "weak map start", 8 * (wm.nb + 1)); if (rc) return rc;
	rc = sm.start.reserve(h, "singleton map start", 8 * (sm.nb + 1)); if (rc) return rc;
	bool weakDone = false;
	h->last_bb_path = 0; overflow = nullptr;
	if (weak_uncounted) {
		rc = binned_buckets_t<W>(h, wslots, wn, fixed_bins, weakDone, overflow); if (rc) return rc;
		if (!weakDone) {      /* the other path wants keys and values apart and a count per bucket */
			rc = ensure_weak_apart(h, std::max<uint64_t>(wslots, 16), vw); if (rc) return rc;
			HIPCHK(h, hipMemsetAsync(wc, 0, 4 * wm.nb, h->stream));
			if (wslots) LAUNCH(h, bb_unpack_kernel<W>, dim3(grid_for(wslots)), dim3(256), 0, (const uint64_t *)h->ue.get<uint64_t>(), wslots, h->hkb, wm.nb, (uint64_t *)h->uw_keys.get(), (uint32_t *)h->uw_vals.get(), wc);
		}
	}
	if (!weakDone) { rc = exclusive_scan(h, wc, wm.nb, wm.start.get<uint64_t>()); if (rc) return rc; }
	if (keepSing) { rc = overflow ? exclusive_scan_queue(h, sc, sm.nb, sm.start.get<uint64_t>()) : exclusive_scan(h, sc, sm.nb, sm.start.get<uint64_t>()); if (rc) return rc; }      /* (bins of one capacity: nothing waits here either) */
	else HIPCHK(h, hipMemsetAsync(sm.start.get<uint64_t>(), 0, 8 * (sm.nb + 1), h->stream));      /* no singleton map is kept: every bucket starts (and ends) at 0 */
	if (!weakDone) {
		rc = wm.keys.reserve(h, "weak map keys", std::max<uint64_t>(8ull * W * wm.n, 8)); if (rc) return rc;
		rc = wm.vals.reserve(h, "weak map vals", std::max<uint64_t>(4ull * vw * wm.n, 8)); if (rc) return rc;
	}
	rc = sm.keys.reserve(h, "singleton map keys", std::max<uint64_t>(8ull * W * sm.n, 8)); if (rc) return rc;
	rc = sm.sweight.reserve(h, "singleton map sweight", std::max<uint64_t>(sm.n, 8)); if (rc) return rc;
	if (h->ext) { rc = sm.spkt.reserve(h, "singleton map spkt", std::max<uint64_t>(4 * sm.n, 8)); if (rc) return rc; }
	HIPCHK(h, hipMemsetAsync(wc, 0, 4 * wm.nb, h->stream)); HIPCHK(h, hipMemsetAsync(sc, 0, 4 * sm.nb, h->stream));
	if (weakDone) { /* keys, values and bucket starts are in place */ }
	else if (wm.n && vw > 4) LAUNCH(h, (entry_scatter_kernel<W, true>), dim3(grid_for(wslots)), dim3(256), 0, (const uint64_t *)h->uw_keys.get(), (const uint32_t *)h->uw_vals.get(),
	                (const uint8_t *)nullptr, (const uint32_t *)nullptr, wslots, vw, h->hkb, wm.nb, wm.start.get<uint64_t>(), wc, wm.keys.get<uint64_t>(), wm.vals.get<uint32_t>(), (uint8_t *)nullptr, (uint32_t *)nullptr, nullptr, 6);
	else if (wm.n) {
		/* lists cut by minimizer (build_mode 3) scatter their entries over unrelated buckets: 64-bit cursors that start at the buckets'
		 * first entries, one returning add per entry */
		unsigned long long *cur64 = nullptr;
		if (h->superkmer_mode && arena_get(h, &cur64, wm.nb) == 0) HIPCHK(h, hipMemcpyAsync(cur64, wm.start.get<uint64_t>(), 8 * wm.nb, hipMemcpyDeviceToDevice, h->stream));
		else cur64 = nullptr;
		LAUNCH(h, entry_scatter_kernel<W>, dim3(grid_for(wslots)), dim3(256), 0, (const uint64_t *)h->uw_keys.get(), (const uint32_t *)h->uw_vals.get(),
		                (const uint8_t *)nullptr, (const uint32_t *)nullptr, wslots, vw, h->hkb, wm.nb, wm.start.get<uint64_t>(), wc, wm.keys.get<uint64_t>(), wm.vals.get<uint32_t>(), (uint8_t *)nullptr, (uint32_t *)nullptr, cur64, 6);
	}
	if (sm.n) LAUNCH(h, entry_scatter_kernel<W>, dim3(grid_for(sslots)), dim3(256), 0, (const uint64_t *)h->us_keys.get(), (const uint32_t *)nullptr,
	                (const uint8_t *)h->us_b8.get(), (const uint32_t *)h->us_pkt.get(), sslots, 0u, h->hkb, sm.nb, sm.start.get<uint64_t>(), sc, sm.keys.get<uint64_t>(), (uint32_t *)nullptr, sm.sweight.get<uint8_t>(), h->ext ? sm.spkt.get<uint32_t>() : (uint32_t *)nullptr, nullptr, 6);
	if (!weakDone) { rc = sort_map_buckets<W>(h, wm, true); if (rc) return rc; }      /* (else sorted by bb_group_kernel) */
	if (sm.n) { rc = sort_map_buckets<W>(h, sm, false); if (rc) return rc; }
	if (!overflow) HIPCHK(h, hipStreamSynchronize(h->stream));      /* (bins of one capacity: the caller waits once, for the overflow word) */
	return 0;
}
int finish_maps_from_entries(kmr_handle *h, uint32_t *wc, uint32_t *sc, uint64_t wslots, uint64_t sslots, uint64_t wn, uint64_t sn, bool keepSing, uint32_t *&overflow, bool weak_uncounted, bool fixed_bins) {
	return with_w(h, [&](auto W) { return finish_maps_t<W()>(h, wc, sc, wslots, sslots, wn, sn, keepSing, overflow, weak_uncounted, fixed_bins); });
}
int finalize_partition(kmr_handle *h, uint32_t min_depth) { return with_w_ext(h, [&](auto W, auto EXT) { return finalize_partition_t<W(), EXT()>(h, min_depth); }); }
template <int W, bool EXT> int insert_records_partition_t(kmr_handle *h, const void *recs, uint64_t n) {
	if (!h->l1.head) choose_bits1(h, n);
	TimeSpan t(h, 0);
	/* received segments contain holes (weight 0): the device counts the real records into stats.raw/good */
	return partition_level1<W, EXT>(h, recs, nullptr, nullptr, (n + 8191) / 8192, 0, 8192, n, n, &h->dstats.get<DevStats>()->inserted,
	                             2 * W + (h->ext ? 2 : 1), h->stream_base);
}
int insert_records_partition(kmr_handle *h, const void *recs, uint64_t n) { return with_w_ext(h, [&](auto W, auto EXT) { return insert_records_partition_t<W(), EXT()>(h, recs, n); }); }
/* ---------------------------------------------------------------------- */
/* build_mode 3: super-k-mer lists (kmr_superkmer.hpp)                        */
/* Minimizer geometry for k: the window of WIN m-mer offsets sits in the middle of the k-mer (2 * off + WIN = k - m + 1), m is
 * the largest length <= 16 (one 32-bit word) of the right parity, WIN the largest of 16 / 8 / 4 that leaves m >= 10. */
bool sk_geometry(uint32_t k, uint32_t m_wish, uint32_t &win, uint32_t &m, uint32_t &off, uint32_t win_max = 16) {
	/* (a window of 32 offsets -- runs of 16.5 k-mers, half the records and list appends of a window of 16 -- exists where it leaves
	 * m >= 14 (k >= 45, keys of two words and more) but is NOT the default: on C4 it takes the extraction from 40.7 to 28.4 ms and the count
	 * pass from 115 to 257 ms -- one place of the genome then puts 33 x coverage k-mers into ONE list, lists of 700 k-mers hold one or
	 * three such places, and the long ones overflow the LDS table into sub-passes; kmr_tune "superkmer_window" = 32 asks for it) */
	/* (a window of 18 offsets at k = 31 -- minimizers of 14 bases, 10 % fewer records -- was built and measured too: extraction 7.57 -> 6.98 ms,
	 * count pass 9.56 -> 10.92 ms on C2; its instances are no longer compiled, the kernels still take any window 16 + {1, 2, 4, 8, 16}) */
	for (uint32_t w : {32u, 16u, 8u, 4u}) {
		if (w > win_max) continue;
		if (w == 32u && (k < 45u || (m_wish && m_wish < 14u))) continue;
		if (k < w + 9) continue;
		uint32_t mm = std::min<uint32_t>(m_wish ? m_wish : 16u, k - w + 1);
		if (mm > 16) mm = 16;
		if (((k - mm + 1 - w) & 1u) != 0) mm--;                 /* k - m + 1 - WIN must be even */
		if (mm < 10 && !m_wish) continue;
		if (mm < 4) continue;
		win = w; m = mm; off = (k - mm + 1 - w) / 2;
		return true;
	}
	return false;
}
const uint64_t SK_EXTRACT_WAVES_PER_CU = std::max(2 * SK_WAVES, SKL_MIN_BLOCKS * SKL_WAVES);      /* wavefronts an extraction launch keeps per CU (each holds two slabs of 64 chunks) */
/* One extraction launch: a wavefront per tile of 64 reads (or units), `waves` of them a block, and no more blocks than are resident
 * at per_cu a CU -- a wavefront walks tiles tile0, tile0 + stride, ...; args: what the kernel takes behind the reads */
template <typename... P, typename... A> int launch_sk_tiles(kmr_handle *h, void (*kern)(ReadsView, P...), const char *name, int w, int win, int waves, int per_cu, size_t smem, const ReadsView &rv, const SkParams &sp, A... args) {
	HIPCHK(h, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
	const uint64_t tiles = ((rv.u_start ? rv.n_units : rv.n_reads) + 63) / 64;
	uint64_t blocks = (tiles + waves - 1) / waves;
	if (blocks == 0) return 0;
	blocks = std::min<uint64_t>(blocks, (uint64_t)num_cus(h) * per_cu);
	if (dbg()) { int nb = 0; hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)kern, waves * 64, smem); fprintf(stderr, "%s<W=%d,WIN=%d>: %d blocks of %d waves per CU (LDS %zu), grid %llu, m=%u off=%u bits=%u\n", name, w, win, nb, waves, smem, (unsigned long long)blocks, sp.m, sp.off, sp.list_bits); }
	LAUNCH(h, kern, dim3((unsigned)blocks), dim3(waves * 64), smem, rv, args...);
	return 0;
}
template <int W, int WIN, bool FILT, bool EXT = false> int launch_sk_extract(kmr_handle *h, const ReadsView &rv, const SkParams &sp, const DevParams &dp) {
	return launch_sk_tiles(h, sk_extract_kernel<W, WIN, FILT, EXT>, "sk_extract", W, WIN, SK_WAVES, 2, SK_EXTRACT_SMEM, rv, sp, dp, sp, pool_view(h, h->l1));
}
uint32_t sk_dbg_flags(const char *name) {
#ifdef KMR_DEBUG_HOOKS
	const char *e = getenv(name); return e ? (uint32_t)atoi(e) : 0u;
#else
	(void)name; return 0u;
#endif
}
bool sp_debug_extract(kmr_handle *h) { (void)h; return sk_dbg_flags("KMR_SK_EXTRACT_DBG") != 0; }      /* the ablation switches live in the general kernel */
template <int W, int WIN, bool PACKED = false> int launch_sk_extract_lean(kmr_handle *h, const ReadsView &rv, const SkParams &sp, const DevParams &dp, float wK, const SkPacked &packed = SkPacked{}) {
	return launch_sk_tiles(h, sk_extract_lean_kernel<W, WIN, PACKED>, "sk_extract_lean", W, WIN, SKL_WAVES, SKL_MIN_BLOCKS, SKL_EXTRACT_SMEM, rv, sp, dp, sp, pool_view(h, h->l1), wK, packed);
}
/* Does the extraction of this build drop k-mers?  Then the general kernel's filtering form takes every launch.  world_size > 1: without
 * the exchange a rank keeps the k-mers the reference's owner function gives it (getDistributedThreadId, as the other build modes do);
 * inside an exchange (kmr_sk_exchange_begin) every k-mer is kept, the lists decide the owner */
bool sk_build_filters(const kmr_handle *h, const DevParams &dp) { return dp.subsample > 1 || dp.num_parts > 1 || (dp.sub_wnb | dp.sub_snb) != 0 || (dp.world > 1 && !h->sk_exchange); }
/* What a k-mer without an N weighs when all its bases have quality character q, as the general kernel would form it: (float) of the k-fold
 * product of the character's probability, 1 for Read::REF_QUAL.  lean = false below the floor: the general kernel's zero handling */
void sk_weight_of_quality(const kmr_handle *h, unsigned int q, bool &lean, float &wK) {
	lean = false; wK = 1.0f;
	if (q == 127) lean = true;
	else if (h->hP[q] > 0.0) { lean = true; wK = (float)h->hPk[q]; }
}
/* Do all k-mers without an N of these reads weigh the same (no qualities, or one quality character throughout)?  Then wK is that
 * weight and sk_extract_lean_kernel may take the launch.
 * longest (may be NULL): where the answer takes a pass over the quality bytes, the pass also finds the longest read and its one wait
 * serves both; *have_longest says whether it did (prepare_units then has nothing to ask the device). */
int sk_uniform_weight(kmr_handle *h, const ReadsView &rv, const FeedHints &hints, bool &lean, float &wK, unsigned int *longest = nullptr, bool *have_longest = nullptr) {
	lean = false; wK = 1.0f;
	if (have_longest) *have_longest = false;
	if (h->tune.no_lean_extract) return 0;
	if (!rv.quals && hints.uniform_q < 0) { lean = true; return 0; }
	if (h->qual_mixed || rv.n_reads == 0) return 0;
	if (hints.uniform_q >= 0) { sk_weight_of_quality(h, (unsigned int)hints.uniform_q, lean, wK); return 0; }      /* the caller said so (kmr_add_reads_twobit*): no pass over the quality bytes, no round trip */
	const int QR_MAX = 32;      /* word of the longest read: 128 bytes behind the characters' pair, away from their atomics */
	{ int rc = h->qrange.reserve(h, "qrange", 4 * (QR_MAX + 1)); if (rc) return rc; }
	unsigned int got[QR_MAX + 1] = {255u, 0u};      /* lowest, highest character; ...; longest read */
	HIPCHK(h, hipMemcpyAsync(h->qrange.get<unsigned int>(), got, sizeof(got), hipMemcpyHostToDevice, h->stream));
	/* half a block per CU of the launch's eight walks the offsets (a C2 batch: 80 MB of them beside 1.5 GB of qualities) */
	const unsigned qr_blocks = (unsigned)num_cus(h) * 8, len_blocks = longest ? (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(qr_blocks / 16, (rv.n_reads + 4095) / 4096)) : 0u;
	LAUNCH(h, sk_qual_range_kernel, dim3(qr_blocks), dim3(256), 0, rv.quals, rv.offsets, rv.n_reads, h->qrange.get<unsigned int>(), h->qrange.get<unsigned int>() + QR_MAX, len_blocks);
	HIPCHK(h, fetch(h, got, h->qrange.get<unsigned int>(), QR_MAX + 1));
	if (longest) { *longest = got[QR_MAX]; *have_longest = true; }
	if (got[0] != got[1]) { h->qual_mixed = got[0] < got[1]; return 0; }      /* (255 > 0: no quality byte at all) */
	sk_weight_of_quality(h, got[0], lean, wK);
	return 0;
}
SkParams sk_params(kmr_handle *h) { SkParams sp; sp.dbg = sk_dbg_flags("KMR_SK_EXTRACT_DBG"); sp.keep_all_owners = h->sk_exchange ? 1u : 0u; sp.track = nullptr; sp.m = h->sk_m; sp.off = h->sk_off; sp.list_bits = h->sk_bits; sp.state = h->sk_state.get<unsigned long long>(); sp.Pk = h->dPk.get<double>(); sp.Rp = h->dPk.get<double>() + 256; sp.fast_div = h->sk_fast_div ? 1u : 0u; return sp; }
/* one weight for the whole build so far? (the count pass's UNI form): a call that had reads went lean with weight wK, or did not */
void sk_note_call_weight(kmr_handle *h, bool lean, float wK) {
	uint32_t wb; memcpy(&wb, &wK, 4);
	if (!lean) h->sk_uni_mixed = true;
	else if (h->sk_uni_w == SK_UNI_NONE) h->sk_uni_w = wb;
	else if (h->sk_uni_w != wb) h->sk_uni_mixed = true;
}
/* The list space of a build, before its first extraction: h->sk_bits (and sk_fine_shift), the list words allocated and set.  job_bases:
 * the bases of the first call, or of the whole host call it is a piece of; lean: the first call's qualities decide.
 * - est: the list space is the whole job's (with world_size > 1 a rank owns every world_size-th list), sized from the caller's estimate of
 *   all the k-mers (estimateRawKmers), else from job_bases times the ranks.
 * - per_list, k-mers per list (about 1100, as the final lists of the two-level partition): the list's distinct keys have to fit the 1024-slot
 *   table of the count pass (80 %), or the list is redone in sub-passes.  At k <= 32 a list of ~1200 k-mers holds ~350 distinct ones in
 *   sequencing data; longer k-mers are hit by read errors more often (k = 51, 1 % errors: 40 % of the k-mers hold one and are nearly all
 *   distinct), so their lists are cut half as long (C4: count pass 133 -> 93 ms; another halving costs more in per-list work than it
 *   saves).  Extension values: a 512-slot table, COUNT_LOG2S_EXT.  One-word keys: the count pass costs 8.8 ms per 10^9 k-mers of C2-like
 *   reads with lists of 1300-1600 k-mers, 9.25 at 1144 and at 1830, 10.2 at 2000 -- overflowing tables --, 11.2 at 715 and ~13 at 570 --
 *   twice the per-list work: between two powers of two the longer lists win up to ~1900 k-mers; 1536 leaves the table room for inputs
 *   with more distinct k-mers than C2's 30 % (the bound was 1224 once: HISTORY.md).
 * - Inside an exchange with coarse lists the bits are those of the wire: as many lists and as full as one GPU's.
 * - aim, one GPU: the list count the count pass likes best instead of a power of two (the code of such a count is the count, sk_list_of).
 *   One-word keys: lists of ~1450 k-mers (8.8 ms per 10^9 k-mers; C2's 2^20 lists of 1144: 9.25).  Two-word keys: lists just below their
 *   bound instead of anywhere between half of it and the bound -- C4 at 665 / 850 / 1100 k-mers per list: 195.7 / 201 / 275 ms.  Extension
 *   values, 10 M reads at k = 21: 2^22 lists of 310 69.4 ms; 570 / 800 / 1000 / 1300 per list: 58.6 / 55.8 / 55.2 / 62.4 ms.  est counts
 *   raw k-mers: reads with qualities of their own lose some of them to the weight floor -- the noisy C2 batch at 1300 / 1450 / 1600 / 1750
 *   raw k-mers per list: count pass 12.7 / 11.4 / 11.1 / 11.0 ms; flat qualities at 1450 / 1550 / 1650: 10.6 / 10.8 / 10.8. */
template <int W> int sk_size_lists(kmr_handle *h, uint64_t job_bases, bool lean) {
	const uint64_t est = h->cfg.estimated_raw_kmers ? h->cfg.estimated_raw_kmers : job_bases * std::max<uint32_t>(1, h->cfg.world_size);
	const uint64_t per_list = h->ext ? (W > 1 ? 400 : 600) : ((h->tune.target_list == 2048 && W > 1) ? 700 : h->tune.target_list * 3 / 4);
	uint32_t bits = 6; while (bits < 24 && (est >> bits) > per_list) bits++;
	h->sk_fine_shift = 0;
	if (h->sk_exchange && h->cfg.world_size > 1 && !h->tune.no_coarse_lists) {
		uint32_t sh = 0; while ((1u << sh) < h->cfg.world_size) sh++;
		if (bits >= 6 + sh) { h->sk_fine_shift = sh; bits -= sh; }
	}
	h->sk_bits = bits;
	if (h->cfg.world_size <= 1 && !h->sk_exchange && h->tune.target_list == 2048 && !h->tune.pow2_lists) {
		const uint64_t aim = h->tune.list_aim ? h->tune.list_aim : (W == 1 ? (h->ext ? 800 : (lean ? 1450 : 1700)) : per_list * 19 / 20);
		const uint64_t nlists = (est / aim + 63) & ~63ull;
		if (nlists > 64 && (nlists < (1ull << bits) || h->tune.list_aim) && nlists < (1ull << 31)) h->sk_bits = (uint32_t)nlists;
	}
	const uint64_t nl0 = sk_list_count(h->sk_bits);
	HIPCHK(h, h->sk_state.alloc(8 * nl0));
	LAUNCH(h, sk_state_init_kernel, dim3(grid_for(nl0)), dim3(256), 0, h->sk_state.get<unsigned long long>(), nl0);
	return 0;
}
/* A job fed in many calls (estimated_raw_kmers says how much is to come) or in the pieces of one host call (call_bases) gets its pool in ONE
 * allocation: before the pool exists, h->l1.presize is what the rest of the job typically takes beyond this call's worst case (flat qualities
 * ~0.25 granules per base, a weight per k-mer ~0.55), a quarter of the free memory at most -- an estimate, and kmr_finalize needs room of its
 * own.  Growing call by call frees the old pool every time, and an allocation right after tens of GB were freed waits seconds for the driver to
 * clear them (config 3's whole input in eight calls: 5.1 s for the first build, HISTORY.md section 6); denser input still grows the pool as before */
void sk_presize_pool(kmr_handle *h, uint64_t call_bases, uint64_t total_bases, uint64_t avg, bool lean) {
	if (h->l1.base || h->cfg.world_size > 1 || h->sk_exchange || !(h->cfg.estimated_raw_kmers || call_bases > total_bases)) return;
	const double job_bases = h->cfg.estimated_raw_kmers ? (double)h->cfg.estimated_raw_kmers * (double)avg / (double)(avg > h->k ? avg - h->k + 1 : 1) : (double)call_bases;
	const double rest = job_bases - (double)total_bases;
	size_t fr = 0, tot = 0;
	if (rest > 0 && hipMemGetInfo(&fr, &tot) == hipSuccess) {
		const uint64_t want = (uint64_t)(rest * (h->ext ? 2.0 : 1.0) * (lean ? 0.3 : 0.65) / SK_CHUNK_G);
		h->l1.presize = std::min<uint64_t>(want, (uint64_t)(fr / 4) / ((size_t)CH * rec_bytes(h)));
	}
}
/* room in the pool for one launch over `bases` bases: a granule per k-mer is more than any input takes (flat qualities: a quarter of that), one open
 * chunk per list -- inside an exchange the lists of other owners start afresh after every pack: for every call --, two slabs of 64 chunks per wavefront */
uint64_t sk_launch_chunks(kmr_handle *h, uint64_t bases) { return (h->ext ? 2 : 1) * bases / SK_CHUNK_G + ((h->l1.base && !h->sk_exchange) ? 0 : sk_list_count(h->sk_bits)) + (uint64_t)num_cus(h) * SK_EXTRACT_WAVES_PER_CU * 130 + 64; }
/* One extraction launch over reads [r, r + rv.n_reads) of a call, in the form the call chose: the packed batch as it is (lean), the
 * general kernel where values carry extensions or the build filters k-mers, else the lean kernel for one weight wK or the general one */
template <int W> int sk_launch_extraction(kmr_handle *h, const ReadsView &rv, const SkParams &sp, const DevParams &dp, bool filt, bool lean, float wK, const SkPacked *packed, uint64_t r) {
	if (packed) {
		SkPacked pkd = *packed; pkd.off += r; if (pkd.mk_off) pkd.mk_off += r;
		return with_win<W>(h->sk_win, [&](auto WIN) { return launch_sk_extract_lean<W, WIN(), true>(h, rv, sp, dp, wK, pkd); });
	}
	return with_win<W>(h->sk_win, [&](auto WIN) {
		if (h->ext) return filt ? launch_sk_extract<W, WIN(), true, true>(h, rv, sp, dp) : launch_sk_extract<W, WIN(), false, true>(h, rv, sp, dp);
		if (filt) return launch_sk_extract<W, WIN(), true>(h, rv, sp, dp);
		return lean ? launch_sk_extract_lean<W, WIN()>(h, rv, sp, dp, wK) : launch_sk_extract<W, WIN(), false>(h, rv, sp, dp);
	});
}
/* size tracker, behind a call's launches, which filled h->trk with per-read records (raw and good k-mers, end ordinal).  SizeTracker::track
 * (src/KmerSpectrum.h:879-894) is called before every k-mer: the thresholds this call's reads pass, each at the t-th raw k-mer of some
 * read; the walk of those reads (sk_track_boundary_kernel) gives the ordinal and the good k-mers */
template <int W> int sk_track_call(kmr_handle *h, const ReadsView &rvAll, const DevParams &dp) {
	const uint64_t n = rvAll.n_reads;
	std::vector<SkTrackRec> recs(n);
	HIPCHK(h, fetch(h, recs.data(), h->trk.get<SkTrackRec>(), n));
	std::vector<SkBoundary> bd; std::vector<uint64_t> good_before;
	const bool walkable = (dp.sub_wnb | dp.sub_snb) == 0;      /* (a subtracting reference decides per k-mer what is raw: read ends there) */
	for (uint64_t r = 0; r < n; r++) {
		while ((uint64_t)h->trk_next <= h->trk_raw + recs[r].raw) {
			SkBoundary b; b.read = r; b.t = (uint32_t)((uint64_t)h->trk_next - h->trk_raw); b.good = 0; b.ordinal = 0;
			if (!walkable) { b.t = recs[r].raw; b.good = recs[r].good; b.ordinal = recs[r].end_ordinal; }
			bd.push_back(b); good_before.push_back(h->trk_good);
			h->trk_snap_raw.push_back(walkable ? (uint64_t)h->trk_next : h->trk_raw + recs[r].raw);
			h->trk_next = (long)((double)h->trk_next * 1.05);
			if (!walkable) break;      /* one element per read end */
		}
		if (!walkable) while ((uint64_t)h->trk_next <= h->trk_raw + recs[r].raw) h->trk_next = (long)((double)h->trk_next * 1.05);
		h->trk_raw += recs[r].raw; h->trk_good += recs[r].good;
	}
	if (h->trk_bounds.size() + bd.size() > SK_TRACK_MAX) return fail(h, KMR_ERR_UNSUPPORTED, "size tracker: more than 512 elements");
	if (!bd.empty() && walkable) {
		DevBuf dbdb; HIPCHK(h, dbdb.alloc(bd.size() * sizeof(SkBoundary)));
		SkBoundary *dbd = dbdb.get<SkBoundary>();
		auto chk = [&](hipError_t e) { return e == hipSuccess ? 0 : fail(h, KMR_ERR_HIP, std::string("size tracker boundaries: ") + hipGetErrorString(e)); };
		int rc = chk(hipMemcpyAsync(dbd, bd.data(), bd.size() * sizeof(SkBoundary), hipMemcpyHostToDevice, h->stream)); if (rc) return rc;
		ReadsView rv = rvAll; rv.u_start = rv.u_end = rv.u_read = nullptr; rv.n_units = 0;      /* (whole reads: the caller's work units do not apply) */
		rc = chk(launch_status(h->stream, sk_track_boundary_kernel<W>, dim3((unsigned)((bd.size() + 63) / 64)), dim3(64), 0, rv, dp, dbd, (uint32_t)bd.size())); if (rc) return rc;
		rc = chk(fetch_queue(h, bd.data(), dbd, bd.size())); if (rc) return rc;
		rc = chk(hipStreamSynchronize(h->stream)); if (rc) return rc;
	}
	for (size_t i = 0; i < bd.size(); i++) { h->trk_bounds.push_back(bd[i].ordinal); h->trk_snap_good.push_back(good_before[i] + bd[i].good); }
	return 0;
}
/* One call's reads into the lists: the form of its extraction, the build's one-weight state, before the first launch of a build the
 * list space, then a launch per sub-batch, and the size tracker's thresholds where it is on */
template <int W> int add_reads_superkmer_t(kmr_handle *h, const ReadsView &rvAll, uint64_t total_bases, const FeedHints &hints) {
	const uint64_t n = rvAll.n_reads;
	const DevParams dp = dev_params(h);
	const bool filt = sk_build_filters(h, dp), tracking = h->cfg.size_tracker && n;
	bool lean = false; float wK = 1.0f; int rc = 0;
	const uint64_t avg = n ? std::max<uint64_t>(1, total_bases / n) : 1;
	const uint64_t sub_bases = h->tune.sub_batch_bases ? h->tune.sub_batch_bases : (1ull << 31);
	const uint64_t chunk = std::max<uint64_t>(64, (sub_bases / avg) & ~63ull);
	/* one sub-batch: the call's longest read is the batch's, and the pass over the qualities (where one runs) brings it along */
	unsigned int longest = 0; bool have_longest = false;
	if (!filt && !h->ext && !sp_debug_extract(h)) { rc = sk_uniform_weight(h, rvAll, hints, lean, wK, n <= chunk ? &longest : nullptr, &have_longest); if (rc) return rc; }      /* (extension values want every neighbour's quality: the general kernel) */
	if (hints.packed && (!lean || h->cfg.size_tracker)) return fail(h, KMR_ERR_STATE, "internal: a packed batch handed to an extraction that wants text");      /* (sk_packed_direct_ok said otherwise) */
	if (n) sk_note_call_weight(h, lean, wK);
	if (n) {      /* the ordinals this call stamps, for sk_count_blocks: rv.stream_base (kmr_set_stream_origin, what earlier calls added, less FeedHints' piece origin) + a base's offset */
		LAUNCH(h, sk_ord_span_kernel, dim3(1), dim3(64), 0, rvAll.offsets, n, rvAll.stream_base, h->dstats.get<DevStats>());
	}
	if (!h->sk_state) { rc = sk_size_lists<W>(h, std::max<uint64_t>(total_bases, hints.call_bases), lean); if (rc) return rc; }
	if (tracking) { h->trk_n = 0; rc = h->trk.reserve(h, "trk", n * sizeof(SkTrackRec)); if (rc) return rc; HIPCHK(h, hipMemsetAsync(h->trk.get<SkTrackRec>(), 0, n * sizeof(SkTrackRec), h->stream)); }      /* (sk_track_call) */
	for (uint64_t r = 0; r < n; r += chunk) {
		const uint64_t m = std::min(chunk, n - r);
		ReadsView rv = reads_slice(rvAll, r, m);
		rc = prepare_units(h, rv, hints.packed ? SK_PACKED_SPAN : (uint32_t)TILE_SPAN, have_longest ? &longest : nullptr); if (rc) return rc;
		if (r == 0) sk_presize_pool(h, hints.call_bases, total_bases, avg, lean);
		rc = pool_reserve(h, h->l1, sk_launch_chunks(h, m * avg + avg), true); if (rc) return rc;
		TimeSpan tb(h, KMR_TIME_BUILD), te(h, KMR_TIME_EXTRACT);
		SkParams sp = sk_params(h);
		if (h->cfg.size_tracker) sp.track = h->trk.get<SkTrackRec>() + r;
		rc = sk_launch_extraction<W>(h, rv, sp, dp, filt, lean, wK, hints.packed, r);
		te.end(); tb.end();
		if (rc) return rc;
	}
	return tracking ? sk_track_call<W>(h, rvAll, dp) : 0;
}
int add_reads_superkmer(kmr_handle *h, const ReadsView &rv, uint64_t total_bases, const FeedHints &hints) { return with_w(h, [&](auto W) { return add_reads_superkmer_t<W()>(h, rv, total_bases, hints); }); }
/* k-mers seen SK_ORDERED_FROM times or more (sat_*_kernel in kmr_superkmer.hpp): weightedCount and directionBias of their entries in the
 * finished weak map from their first 65 535 sightings in input order, added into a float one after the other as the serial reference
 * does.  n_clamped: how many such keys the count pass kept, n_sightings: their sightings.
 * On high-coverage input (a small genome, an amplicon, a dominant species) nearly every key qualifies, and every sighting costs the
 * pass 24 bytes of scratch (two key and two value arrays of the sort) -- more than the record pool the sightings came from.  So the
 * keys are redone in batches of whole keys, taken in (list, entry) order: a batch is a run of lists (or of one list's keys) whose
 * sightings, estimated from their chunks at the density of the whole pass, fit SAT_BATCH_BYTES, and holds fewer than 2^23 keys (the
 * key's index in a batch has bits 41-63 of the sort key, sat_collect_kernel).  One list whose sightings alone exceed the budget (a
 * homopolymer: 10^6 sightings and more) is a batch of its own.  A batch's scratch lives while that batch runs. */
/* 1 GiB: ~4.5 x 10^7 sightings per batch, enough for the radix sort to run at full rate, and small against the 288 GB of a GPU and the
 * record pool of any build that has that many sightings of hot keys (the pool holds them and all their neighbours) */
static const uint64_t SAT_BATCH_BYTES = 1ull << 30;
static const uint64_t SAT_BATCH_KEYS = (1ull << 23) - 1;
static const uint64_t SAT_PAIR_BYTES = 24;
template <int W> int saturated_fix_t(kmr_handle *h, const uint64_t *ls, const uint64_t *lc, uint64_t nl, unsigned long long n_clamped, unsigned long long n_sightings, uint32_t has_singletons) {
	DevMap &wm = h->weak;
	h->last_saturated_keys = 0; h->last_saturated_batches = 0;
	if (!n_clamped || !wm.n) return 0;
	uint32_t list_bits = 0; while ((1ull << list_bits) < nl) list_bits++;
	if ((1ull << list_bits) != nl) list_bits = (uint32_t)nl;      /* a list count that is not a power of two is its own code (sk_list_of) */
	auto no_mem = [&](const char *what, size_t bytes) { return fail(h, KMR_ERR_OOM, std::string("saturated-key pass (weights of k-mers seen 256 times or more): no device memory for ") + what + " (" + std::to_string(bytes) + " bytes)"); };
	auto dalloc = [](DevBuf &b, size_t bytes) { return b.alloc(std::max<size_t>(bytes, 256)); };
	DevBuf bfound, bentry, blist;
	if (dalloc(bfound, 8) != hipSuccess) return no_mem("a counter", 8);
	unsigned long long *dfound = bfound.get<unsigned long long>(); uint64_t *d_entry = nullptr; uint32_t *d_list = nullptr;
	uint64_t cap = std::min<uint64_t>(wm.n, 4 * n_clamped + 1024);
	unsigned long long found = 0;
	for (;;) {
		if (dalloc(bentry, 8 * cap) != hipSuccess || dalloc(blist, 4 * cap) != hipSuccess) return no_mem("the key list", 12 * cap);
		d_entry = bentry.get<uint64_t>(); d_list = blist.get<uint32_t>();
		HIPCHK(h, hipMemsetAsync(dfound, 0, 8, h->stream));
		LAUNCH(h, sat_find_kernel<W>, dim3(grid_for(wm.n)), dim3(256), 0, (const uint64_t *)wm.keys.get<uint64_t>(), (const uint32_t *)wm.vals.get<uint32_t>(), wm.n, h->sk_m, h->sk_off, h->sk_win, list_bits, dfound, cap, d_entry, d_list, value_words(h));
		HIPCHK(h, fetch(h, &found, dfound));
		if (found <= cap) break;
		cap = found;      /* more entries at 256 or more than expected: again with room for all */
	}
	if (!found) return 0;
	std::vector<uint64_t> entry(found); std::vector<uint32_t> lst(found);
	HIPCHK(h, hipMemcpy(entry.data(), d_entry, 8 * found, hipMemcpyDeviceToHost)); HIPCHK(h, hipMemcpy(lst.data(), d_list, 4 * found, hipMemcpyDeviceToHost));
	std::vector<uint64_t> order(found);
	for (uint64_t i = 0; i < found; i++) order[i] = i;
	std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return lst[a] != lst[b] ? lst[a] < lst[b] : entry[a] < entry[b]; });
	std::vector<uint64_t> sentry(found); std::vector<uint32_t> dl; std::vector<uint64_t> le0, le1;
	for (uint64_t i = 0; i < found; i++) {
		sentry[i] = entry[order[i]];
		const uint32_t l = lst[order[i]];
		if (dl.empty() || dl.back() != l) { dl.push_back(l); le0.push_back(i); le1.push_back(i + 1); } else le1.back() = i + 1;
	}
	std::vector<uint64_t>().swap(entry); std::vector<uint32_t>().swap(lst); std::vector<uint64_t>().swap(order);
	HIPCHK(h, hipMemcpy(d_entry, sentry.data(), 8 * found, hipMemcpyHostToDevice));
	HIPCHK(h, hipMemcpy(d_list, dl.data(), 4 * dl.size(), hipMemcpyHostToDevice));
	std::vector<uint64_t> c0(dl.size()), c1(dl.size());
	{
		DevBuf bc0, bc1;
		if (dalloc(bc0, 8 * dl.size()) != hipSuccess || dalloc(bc1, 8 * dl.size()) != hipSuccess) return no_mem("the chunk ranges", 16 * dl.size());
		LAUNCH(h, sat_gather_kernel, dim3(grid_for(dl.size())), dim3(256), 0, ls, (const uint32_t *)d_list, (uint64_t)dl.size(), bc0.get<uint64_t>(), bc1.get<uint64_t>());
		HIPCHK(h, hipMemcpy(c0.data(), bc0.get<uint64_t>(), 8 * dl.size(), hipMemcpyDeviceToHost)); HIPCHK(h, hipMemcpy(c1.data(), bc1.get<uint64_t>(), 8 * dl.size(), hipMemcpyDeviceToHost));
	}
	blist = DevBuf();
	/* segments: a list's keys, cut into runs of at most SAT_BATCH_KEYS (a run re-reads its list's chunks); their sightings estimated at
	 * the pass's density (the count pass's sightings of such keys over the chunks of the lists that hold them) */
	struct Seg { uint32_t li; uint64_t e0, e1, est; };
	std::vector<Seg> segs;
	uint64_t all_chunks = 0;
	for (size_t i = 0; i < dl.size(); i++) all_chunks += c1[i] - c0[i];
	const double per_chunk = all_chunks ? (double)n_sightings / (double)all_chunks : 0.0;
	for (size_t i = 0; i < dl.size(); i++)
		for (uint64_t a = le0[i]; a < le1[i]; a += SAT_BATCH_KEYS) {
			const uint64_t b = std::min<uint64_t>(le1[i], a + SAT_BATCH_KEYS);
			const double share = (double)(b - a) / (double)(le1[i] - le0[i]);
			segs.push_back(Seg{(uint32_t)i, a, b, (uint64_t)(per_chunk * (double)(c1[i] - c0[i]) * share) + 1});
		}
	const uint64_t budget = h->tune.saturated_batch_bytes ? h->tune.saturated_batch_bytes : SAT_BATCH_BYTES;
	uint64_t batches = 0;
	for (size_t s0 = 0; s0 < segs.size(); ) {
		/* the batch: segments s0 .. s1 - 1 (at least one) */
		size_t s1 = s0 + 1; uint64_t est = segs[s0].est;
		while (s1 < segs.size() && segs[s1].e1 - segs[s0].e0 <= SAT_BATCH_KEYS && (est + segs[s1].est) * SAT_PAIR_BYTES <= budget) est += segs[s1++].est;
		const uint64_t k0 = segs[s0].e0, nk = segs[s1 - 1].e1 - k0;
		/* work items: pieces of 256 chunks of the batch's lists, key indices relative to the batch */
		std::vector<uint64_t> items;
		for (size_t g = s0; g < s1; g++)
			for (uint64_t a = c0[segs[g].li]; a < c1[segs[g].li]; a += 256) { items.push_back(a); items.push_back(std::min(c1[segs[g].li], a + 256)); items.push_back(segs[g].e0 - k0); items.push_back(segs[g].e1 - k0); }
		const size_t ni = items.size() / 4;
		std::vector<uint64_t> soa(4 * ni);
		for (size_t i = 0; i < ni; i++) for (int q = 0; q < 4; q++) soa[q * ni + i] = items[4 * i + q];
		uint64_t pcap = est + est / 4 + 1024;
		for (int attempt = 0; ni; attempt++) {
			DevBuf bitems, bk_in, bk_out, bv_in, bv_out, btmp;      /* the batch's scratch */
			if (dalloc(bitems, 32 * ni) != hipSuccess) return no_mem("its work items", 32 * ni);
			uint64_t *d_items = bitems.get<uint64_t>();
			HIPCHK(h, hipMemcpy(d_items, soa.data(), 32 * ni, hipMemcpyHostToDevice));
			if (dalloc(bk_in, 8 * pcap) != hipSuccess || dalloc(bk_out, 8 * pcap) != hipSuccess || dalloc(bv_in, 4 * pcap) != hipSuccess || dalloc(bv_out, 4 * pcap) != hipSuccess)
				return no_mem("the sightings of one batch", SAT_PAIR_BYTES * pcap);
			unsigned long long *pk_in = bk_in.get<unsigned long long>(), *pk_out = bk_out.get<unsigned long long>(); uint32_t *pv_in = bv_in.get<uint32_t>(), *pv_out = bv_out.get<uint32_t>();
			HIPCHK(h, hipMemsetAsync(dfound, 0, 8, h->stream));
			int rc = zero_work_counter(h); if (rc) return rc;
			LAUNCH(h, sat_collect_kernel<W>, dim3((unsigned)std::min<uint64_t>(ni, (uint64_t)num_cus(h) * 4)), dim3(256), 0, pool_view(h, h->l1), lc, h->k, (const uint64_t *)wm.keys.get<uint64_t>(), (const uint64_t *)(d_entry + k0),
			       (const uint64_t *)d_items, (const uint64_t *)(d_items + ni), (const uint64_t *)(d_items + 2 * ni), (const uint64_t *)(d_items + 3 * ni), (uint64_t)ni, dfound, pcap, pk_in, pv_in, h->work_counter.get<unsigned int>());
			unsigned long long n_pairs = 0;
			HIPCHK(h, fetch(h, &n_pairs, dfound));
			if (n_pairs > pcap) {      /* denser than the estimate: the batch again with room for exactly what it holds */
				if (attempt) return fail(h, KMR_ERR_CAPACITY, "saturated-key pass: sightings of a batch changed between two passes (internal error)");
				pcap = n_pairs;
				continue;
			}
			size_t tmp_bytes = 0;
			if (kmr::sort_pairs_u64_u32(nullptr, &tmp_bytes, pk_in, pk_out, pv_in, pv_out, n_pairs, h->stream) != 0) return fail(h, KMR_ERR_HIP, "saturated-key pass: radix sort (size query)");
			if (dalloc(btmp, tmp_bytes) != hipSuccess) return no_mem("the sort's temporary storage", tmp_bytes);
			if (kmr::sort_pairs_u64_u32(btmp.get(), &tmp_bytes, pk_in, pk_out, pv_in, pv_out, n_pairs, h->stream) != 0) return fail(h, KMR_ERR_HIP, "saturated-key pass: radix sort");
			LAUNCH(h, sat_reduce_kernel, dim3((unsigned)std::min<uint64_t>(nk, 4096)), dim3(256), 0, (const unsigned long long *)pk_out, (const uint32_t *)pv_out, (uint64_t)n_pairs, (const uint64_t *)(d_entry + k0), (uint64_t)nk, has_singletons, wm.vals.get<uint32_t>(), value_words(h));
			HIPCHK(h, hipStreamSynchronize(h->stream));
			break;
		}
		batches++;
		s0 = s1;
	}
	h->last_saturated_keys = found; h->last_saturated_batches = batches;
	return 0;
}

/* ---- The count pass over super-k-mer lists as kmr_finalize (finalize_superkmer_t) and kmr_count_lists_prefix (count_prefix_superkmer_t)
 * plan it.  The two must agree: kmr_finalize takes the early count's entries over as they are, so an early pass that decides "one
 * weight" while the final pass decides otherwise would mix two roundings in one map. */

/* One weight for every record of the lists (own calls: host state; adopted records: what the senders declared, else the device
 * pair)?  Then the count pass's UNI form, with that weight in uni_wbits. */
template <int W> int sk_count_uniform(kmr_handle *h, bool tracking, bool &uni, uint32_t &uni_wbits) {
	uni = false; uni_wbits = 0;
	if (tracking || h->ext || h->sk_uni_mixed || h->tune.no_uniform_count) return 0;
	if (W > 1 && (h->k & 31u) == 0) return 0;      /* (multi-word keys: the one-weight pass has no state words, it needs pad bits in the last key word) */
	uint32_t w = h->sk_uni_w; bool mixed = false;
	if (h->peer_uni_mixed) mixed = true;
	else if (h->peer_uni_w != SK_UNI_NONE) { if (w == SK_UNI_NONE) w = h->peer_uni_w; else if (w != h->peer_uni_w) mixed = true; }
	if (h->d_uni) {
		uint32_t dv[2] = {SK_UNI_NONE, 0u};
		HIPCHK(h, hipMemcpy(dv, h->d_uni.get<uint32_t>(), 8, hipMemcpyDeviceToHost));
		if (dv[1]) mixed = true;
		else if (dv[0] != SK_UNI_NONE) { if (w == SK_UNI_NONE) w = dv[0]; else if (w != dv[0]) mixed = true; }
	}
	if (!mixed && w != SK_UNI_NONE) { uni = true; uni_wbits = w; }
	return 0;
}
/* the lists this rank's pass looks at (SkLong, list mode): all of them, or -- inside an owner exchange whose lists were not refined --
 * rank, rank + world_size, ...: the other lists went to their owners.  No long-list threshold, no work items, no merge table. */
template <int W> SkLong<W> sk_own_lists(kmr_handle *h, bool refined) {
	SkLong<W> lg{};
	lg.list_first = 0; lg.list_stride = 1;
	if (h->sk_exchange && h->cfg.world_size > 1 && !refined) { lg.list_first = h->cfg.rank; lg.list_stride = h->cfg.world_size; }
	return lg;
}
/* sk_count_kernel's form for (W, ext, tracking, uni) together with the dynamic LDS it wants, the attribute set */
template <int W> struct SkCountLaunch {
	void (*kern)(const uint4 *, const uint64_t *, const uint64_t *, uint64_t, uint32_t, SkCountHot, unsigned int *, uint32_t, const SkCountArgs<W> *);
	size_t smem;
	int blocks;      /* blocks per CU the grid is sized for */
};
/* Blocks per CU a launch of the count pass is sized for: four (every form's grid has been num_cus x 4 all along, whatever its instance is
 * compiled for), or five or six for the one form that exists as such instances -- one-weight, one-word keys, lists (not work items).
 * The entry buffers' slack follows it (a slab tail per wavefront launched).  n_lists: the lists the launch goes over.
 * Six (slots of 20 bytes: a first-sighting word of 32 bits, the ordinal relative to the build's lowest) wants
 *   - kmr_tune "count_blocks" 0 (an explicit 4 or 5 means that instance) and "count_six" below 2,
 *   - every record stamped by this handle's own feed calls, so that their lowest and highest ordinal are known (ord_lo, ord_hi: what
 *     sk_ord_span_kernel collected, as the sync_state at the head of kmr_finalize and of kmr_count_lists_prefix read it; records adopted
 *     from an exchange carry their senders' ordinals), and highest - lowest < 2^31,
 *   - enough lists that a sixth block per CU gets a batch of SK_LBATCH of them from the work counter at all ("count_six" 1 waives this). */
static const int SK_COUNT_BLOCKS_DEFAULT = 5;      /* what "count_blocks" 0 means for that form where six does not apply: C2's count pass 8.72 -> 7.7 ms (profiles/count_blocks_ab.jsonl) */
static const bool SK_COUNT_SIX_DEFAULT = true;     /* "count_six" 0 takes the six-block instance where the rule allows it (profiles/count_six_ab.jsonl) */
template <int W> int sk_count_blocks(kmr_handle *h, bool ext, bool tracking, bool uni, bool item, uint64_t n_lists) {
	if (W != 1 || ext || tracking || !uni || item) return 4;
	if (h->tune.count_blocks) return h->tune.count_blocks;
	const bool ordinals = h->ord_seen && !h->ord_foreign && h->ord_hi >= h->ord_lo && h->ord_hi - h->ord_lo < (1ull << 31);
	const bool fed = n_lists >= (uint64_t)num_cus(h) * 6 * SK_LBATCH;
	if (ordinals && (h->tune.count_six == 1 || (h->tune.count_six == 0 && SK_COUNT_SIX_DEFAULT && fed))) return 6;
	return SK_COUNT_BLOCKS_DEFAULT;
}
template <int W, int LOG2S, bool TRACK, bool EXT, bool UNI, bool ITEM, int BLOCKS = 0> SkCountLaunch<W> sk_count_form() { return {sk_count_kernel<W, LOG2S, TRACK, EXT, UNI, ITEM, BLOCKS>, sk_count_smem_bytes<W, LOG2S, TRACK, EXT, UNI, BLOCKS == 6>(), BLOCKS ? BLOCKS : 4}; }
template <int W, bool ITEM> SkCountLaunch<W> sk_count_forms(bool ext, bool tracking, bool uni, int blocks) {
	if constexpr (!ITEM) { if (tracking && !ext) return sk_count_form<W, COUNT_LOG2S, true, false, false, false>(); }
	if constexpr (W == 1 && !ITEM) {
		if (blocks == 5) return sk_count_form<1, COUNT_LOG2S, false, false, true, false, 5>();
		if (blocks == 6) return sk_count_form<1, COUNT_LOG2S, false, false, true, false, 6>();
	}
	return ext ? sk_count_form<W, COUNT_LOG2S_EXT, false, true, false, ITEM>() :
	    (uni ? sk_count_form<W, COUNT_LOG2S, false, false, true, ITEM>() : sk_count_form<W, COUNT_LOG2S, false, false, false, ITEM>());
}
/* The kernel fixes at compile time what a launch used to tell it through null pointers: `item` (the pass over work items of long lists,
 * lg.item_c0 and the merge table) and the form of the weak entries (packed without per-bucket counts unless ext).  An `out` or `lg` of
 * the other form is an internal error here, not a null pointer on the device. */
template <int W> int sk_count_select(kmr_handle *h, bool ext, bool tracking, bool uni, bool item, uint64_t n_lists, const CountOut &out, const SkLong<W> &lg, SkCountLaunch<W> &k) {
	if (item && tracking) return fail(h, KMR_ERR_STATE, "internal: the size tracker's count pass has no long-list items");
	if (item != (lg.item_c0 != nullptr) || (item && (!lg.item_c1 || !lg.merge.slots || !lg.merge_used))) return fail(h, KMR_ERR_STATE, "internal: count pass and its work items disagree");
	if (ext ? (!out.wkeys || !out.wvals || !out.weakCount) : !out.wentries) return fail(h, KMR_ERR_STATE, "internal: count pass and its entry buffers disagree");
	const int blocks = sk_count_blocks<W>(h, ext, tracking, uni, item, n_lists);
	k = item ? sk_count_forms<W, true>(ext, tracking, uni, blocks) : sk_count_forms<W, false>(ext, tracking, uni, blocks);
	if (k.blocks != blocks) return fail(h, KMR_ERR_STATE, "internal: count pass and its blocks per CU disagree");
	if (!item) h->last_count_blocks = k.blocks;
	const auto kern = k.kern; const size_t smem = k.smem;
	HIPCHK(h, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
	return 0;
}
/* One launch of the count pass: its rarely read arguments go into an SkCountArgs of the finalize arena first (a one-thread kernel on the
 * same stream writes it: no host buffer that would have to outlive the call), the rest goes by value */
template <int W> int sk_count_launch(kmr_handle *h, const SkCountLaunch<W> &k, int grid, const uint64_t *ls, const uint64_t *lc, uint64_t nl, const CountOut &out, const FinalizeParams &f, const SkTrackView &tv, const SkLong<W> &lg) {
	SkCountArgs<W> a{out, f, tv, lg};
	SkCountArgs<W> *d = nullptr;
	int rc = arena_get(h, &d, 1); if (rc) return rc;
	LAUNCH(h, sk_count_args_kernel<W>, dim3(1), dim3(64), 0, a, d);
	SkCountHot hot = sk_count_hot<W>(a);
	if (k.blocks == 6) hot.ord_base = (uint32_t)h->ord_lo;      /* (that instance has no extension values: the word is free) */
	LAUNCH(h, k.kern, dim3(grid), dim3(SKC_THREADS), k.smem, (const uint4 *)pool_view(h, h->l1).base, ls, lc, nl, h->k, hot, h->work_counter.get<unsigned int>(), sk_dbg_flags("KMR_SK_COUNT_DBG"), (const SkCountArgs<W> *)d);
	return 0;
}

/* what the phases of finalize_superkmer_t hand to one another: the count pass's state (CountPass) and what the lists add */
template <int W> struct SkFinalize : CountPass {
	bool tracking = false, refined = false, uni = false;
	uint64_t nl = 1; uint64_t *ls = nullptr, *lc = nullptr; uint32_t nch = 0;      /* the lists and their chunk CSR */
	SkTrackView tv{};
	SkLong<W> lgMain{}, lgItems{}; uint64_t n_items = 0;                         /* the pass over lists, the pass over work items of long lists */
	uint64_t early_slots = 0; FinalizeCounters early_c{};                        /* an early count that is taken over */
};

/* the coarse lists this rank owns (its own share and what it adopted) -> fine lists (sk_refine_kernel); nl: how many */
int sk_refine_lists(kmr_handle *h, uint64_t &nl) {
	const uint32_t fine_bits = h->sk_bits + h->sk_fine_shift;
	const uint64_t nlf = 1ull << fine_bits;
	unsigned int head = 0;
	HIPCHK(h, hipStreamSynchronize(h->stream));
	HIPCHK(h, hipMemcpy(&head, h->l1.head.get<unsigned int>(), 4, hipMemcpyDeviceToHost));
	if (head > h->l1.cap) head = h->l1.cap;
	int rc = h->sk_fine_state.reserve(h, "sk_fine_state", 8 * nlf); if (rc) return rc;
	LAUNCH(h, sk_state_init_kernel, dim3(grid_for(nlf)), dim3(256), 0, h->sk_fine_state.get<unsigned long long>(), nlf);
	const int rgrid = (int)std::min<uint64_t>(((uint64_t)head + SK_REFINE_WAVES - 1) / SK_REFINE_WAVES + 1, (uint64_t)num_cus(h) * 8);
	/* every old chunk's records again, cut into at most 2^shift pieces per chunk (a piece may open a chunk), an open chunk per owned fine list */
	rc = pool_reserve(h, h->l1, (uint64_t)head * 2 + nlf / h->cfg.world_size + (uint64_t)rgrid * SK_REFINE_WAVES * 130 + 64, true); if (rc) return rc;
	if (head) LAUNCH(h, sk_refine_kernel, dim3(rgrid), dim3(SK_REFINE_WAVES * 64), 0, pool_view(h, h->l1), head, fine_bits, h->sk_fine_state.get<unsigned long long>());
	LAUNCH(h, sk_close_kernel, dim3(grid_for(nlf)), dim3(256), 0, h->sk_fine_state.get<unsigned long long>(), nlf, h->l1.chunk_count.get<uint32_t>(), h->l1.cap);
	nl = nlf;
	return 0;
}
/* size tracker: SizeTracker::track (src/KmerSpectrum.h:879-894) applied after every read, in stream order; what it pushes is known
 * from the per-read records alone except the unique / singleton counters, which the count pass fills in per boundary (tv) */
int sk_track_view(kmr_handle *h, SkTrackView &tv) {
	const std::vector<unsigned long long> &bounds = h->trk_bounds;
	if (bounds.size() > SK_TRACK_MAX) return fail(h, KMR_ERR_UNSUPPORTED, "size tracker: more than 512 elements");
	unsigned long long *db = nullptr; unsigned int *dd = nullptr;
	int rc = arena_get(h, &db, bounds.size() + 1); if (rc) return rc;
	rc = arena_get(h, &dd, 2 * (bounds.size() + 1)); if (rc) return rc;
	if (!bounds.empty()) HIPCHK(h, hipMemcpyAsync(db, bounds.data(), 8 * bounds.size(), hipMemcpyHostToDevice, h->stream));
	tv.bounds = db; tv.n = (uint32_t)bounds.size(); tv.d_unique = dd; tv.d_single = dd + bounds.size() + 1;
	return 0;
}
/* ... and after the pass: the tracker's elements out of the per-boundary counters */
int sk_track_elements(kmr_handle *h, const SkTrackView &tv, uint32_t has_singletons) {
	std::vector<unsigned int> dd(2 * (tv.n + 1), 0);
	HIPCHK(h, hipMemcpy(dd.data(), tv.d_unique, 8 * (tv.n + 1), hipMemcpyDeviceToHost));
	h->trk_elems.clear();
	uint64_t uniq = 0; int64_t single = 0;
	const uint64_t sub = h->cfg.kmer_subsample > 1 ? h->cfg.kmer_subsample : 1;      /* track() scales what it stores, :882-887 */
	for (uint32_t i = 0; i < tv.n; i++) {
		uniq += dd[i]; single += (int32_t)dd[tv.n + 1 + i];
		h->trk_elems.push_back(h->trk_snap_raw[i] * sub); h->trk_elems.push_back(h->trk_snap_good[i] * sub);
		h->trk_elems.push_back(uniq * sub); h->trk_elems.push_back(has_singletons ? (uint64_t)single * sub : 0);
	}
	return 0;
}
/* Lists below early.hi were counted by kmr_count_lists_prefix: the pass starts behind them (p.lgMain.list_first) and their entries are
 * taken over afterwards (sk_append_early).  An early count that overflowed its buffers, or was made for another min-depth or map
 * layout, is void: everything is counted here.  device_error: the early pass left an error other than an overflow in the build's
 * error word; the caller ends its timing and reports it through sync_state. */
template <int W> int sk_early_takeover(kmr_handle *h, SkFinalize<W> &p, uint32_t min_depth, bool &device_error) {
	device_error = false;
	FinalizeCounters &early_c = p.early_c;
	h->last_early_hi = 0; h->last_early_entries = 0; h->last_early_overflowed = false;
	if (!h->early.active) return 0;
	uint32_t eerr = 0;      /* (the early pass's own word: its overflow never reaches h->derr, sync_state or another call) */
	HIPCHK(h, hipMemcpy(&eerr, h->early.err.get<uint32_t>(), 4, hipMemcpyDeviceToHost));
	unsigned long long ecur = 0;
	HIPCHK(h, hipMemcpy(&ecur, h->early.cursor.get<unsigned long long>(), 8, hipMemcpyDeviceToHost)); HIPCHK(h, hipMemcpy(&early_c, h->early.fc.get(), sizeof(early_c), hipMemcpyDeviceToHost));
	if (eerr & ~(uint32_t)ERR_ENTRIES_FULL) {      /* anything but an overflow is the build's error as ever */
		uint32_t e = 0; HIPCHK(h, hipMemcpy(&e, h->derr.get<uint32_t>(), 4, hipMemcpyDeviceToHost)); e |= eerr & ~(uint32_t)ERR_ENTRIES_FULL;
		HIPCHK(h, hipMemcpy(h->derr.get<uint32_t>(), &e, 4, hipMemcpyHostToDevice)); h->early.active = false;
		device_error = true;
		return 0;
	}
	const bool overflowed = (eerr & ERR_ENTRIES_FULL) || ecur > packed_entries(h, h->early.ue);
	const bool ok = !overflowed && h->early.min_depth == min_depth && !p.tracking && !p.ext && !p.keepSing && !p.refined;
	h->last_early_overflowed = overflowed;
	if (ok) {
		p.early_slots = ecur;
		h->last_early_hi = h->early.hi; h->last_early_entries = early_c.weak_kept;
		const uint64_t stride0 = p.lgMain.list_stride, first0 = p.lgMain.list_first;
		uint64_t first = h->early.hi;
		if (stride0 > 1) first += (first0 + stride0 - first % stride0) % stride0;      /* the first list at or behind hi that is this rank's */
		p.lgMain.list_first = first;
	} else { h->early.active = false; memset(&early_c, 0, sizeof(early_c)); }
	return 0;
}
/* long lists (SkLong in kmr_superkmer.hpp): found from the CSR, cut into work items (p.lgItems), counted by a second launch into a merge table */
template <int W> int sk_long_items(kmr_handle *h, SkFinalize<W> &p) {
	p.lgItems = p.lgMain; p.n_items = 0;
	/* (extension values: the 16-bit tallies of a block's table are exact below 65 536 k-mers, SK_EXT_LONG_CHUNKS) */
	const uint64_t LONG_CHUNKS = p.ext ? std::min<uint64_t>(h->tune.long_list_chunks ? h->tune.long_list_chunks : SK_EXT_LONG_CHUNKS, SK_EXT_LONG_CHUNKS) : (h->tune.long_list_chunks ? h->tune.long_list_chunks : 1024), PIECE = std::max<uint64_t>(1, LONG_CHUNKS / 2);
	if (p.tracking || p.nch <= LONG_CHUNKS) return 0;
	const uint64_t cap = (uint64_t)p.nch / PIECE + 2 * 1024 + 16;
	uint64_t *ic0 = nullptr, *ic1 = nullptr; unsigned long long *dn = nullptr;
	int rc = arena_get(h, &ic0, cap); if (rc) return rc; rc = arena_get(h, &ic1, cap); if (rc) return rc; rc = arena_get(h, &dn, 1); if (rc) return rc;
	HIPCHK(h, hipMemsetAsync(dn, 0, 8, h->stream));
	LAUNCH(h, sk_long_items_kernel, dim3(grid_for(p.nl)), dim3(256), 0, p.ls, p.nl, LONG_CHUNKS, PIECE, ic0, ic1, cap, dn, nullptr);
	unsigned long long hn = 0;
	HIPCHK(h, fetch(h, &hn, dn));
	if (hn > cap) return fail(h, KMR_ERR_CAPACITY, "long-list work items (internal sizing error)");
	p.n_items = hn;
	if (p.n_items) {
		p.lgMain.long_threshold = LONG_CHUNKS;
		p.lgItems.item_c0 = ic0; p.lgItems.item_c1 = ic1; p.lgItems.n_items = p.n_items; p.lgItems.merge_used = dn;
	}
	return 0;
}
/* where a count pass puts its entries: the weak ones packed (h->ue: build_mode 3 without extension values, bucketed without a per-bucket
 * histogram, kmr_buckets.hpp) or keys and values apart with their per-bucket counts (h->uw_*), singletons in h->us_* */
CountOut count_out(kmr_handle *h, bool packed, unsigned long long *cursors, uint32_t *wc, uint32_t *sc, FinalizeCounters *fc) {
	CountOut out{};
	if (packed) { out.wentries = h->ue.get<uint64_t>(); out.wcap = packed_entries(h, h->ue); }
	else { out.wkeys = h->uw_keys.get<uint64_t>(); out.wvals = h->uw_vals.get<uint32_t>(); out.wcap = key_entries(h, h->uw_keys); out.spkt = h->us_pkt.get<uint32_t>(); out.weakCount = wc; }
	out.wcursor = cursors; out.scursor = cursors + 1;
	out.skeys = h->us_keys.get<uint64_t>(); out.sweight = h->us_b8.get<uint8_t>(); out.scap = key_entries(h, h->us_keys);
	out.singCount = sc; out.fc = fc; out.err = h->derr.get<uint32_t>();
	return out;
}
/* The count pass over the lists and, where some are long, over their work items into a merge table (count_attempts: again with doubled
 * entry buffers while they overflow; this pass asks for a repeat with a larger merge table while that fills) */
template <int W> int sk_count_pass(kmr_handle *h, SkFinalize<W> &p) {
	const uint64_t nl = p.nl, n_items = p.n_items; const SkTrackView &tv = p.tv;
	uint32_t merge_log2 = 16;
	DevBuf mslots, mext;      /* an attempt's merge table, given back before the next one allocates */
	return count_attempts(h, p, [&]() -> int { mslots.reset(); mext.reset(); return 0; }, [&](const CountOut &out, bool repeated, uint32_t &repeat_on) -> int {
		if (repeated) merge_log2 += 3;
		int rc = 0;
		SkCountLaunch<W> k;
		rc = sk_count_select<W>(h, p.ext, p.tracking, p.uni, false, nl, out, p.lgMain, k); if (rc) return rc;
		const int grid = (int)std::min<uint64_t>((uint64_t)num_cus(h) * k.blocks, (nl / p.lgMain.list_stride + SK_LBATCH) / SK_LBATCH);
		if (p.tracking) HIPCHK(h, hipMemsetAsync(tv.d_unique, 0, 8 * (tv.n + 1), h->stream));
		if (dbg()) { int nb = 0; hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)k.kern, SKC_THREADS, k.smem); fprintf(stderr, "sk_count<W=%d>: %d blocks per CU (LDS %zu), %llu lists, %u chunks\n", W, nb, k.smem, (unsigned long long)nl, p.nch); }
		rc = sk_count_launch<W>(h, k, grid, p.ls, p.lc, nl, out, p.f, tv, p.lgMain); if (rc) return rc;
		if (!n_items) return 0;
		/* the merge table holds the distinct keys of the long lists: few when a list is long because a k-mer repeats, at most the
		 * k-mers of those lists; it starts small and the attempt is repeated with a larger one if it fills */
		SkLong<W> &lgItems = p.lgItems;
		if (mslots.alloc(sizeof(Slot<W>) << merge_log2) != hipSuccess) return fail(h, KMR_ERR_OOM, "merge table of the long lists");
		if (p.ext && mext.alloc(sizeof(ExtSlot) << merge_log2) != hipSuccess) return fail(h, KMR_ERR_OOM, "merge table of the long lists");
		LAUNCH(h, table_clear_kernel<W>, dim3(grid_for(1ull << merge_log2)), dim3(256), 0, mslots.get<Slot<W>>(), mext.get<ExtSlot>(), 1ull << merge_log2);
		lgItems.merge.slots = mslots.get<Slot<W>>(); lgItems.merge.ext = mext.get<ExtSlot>(); lgItems.merge.log2cap = merge_log2;
		HIPCHK(h, hipMemsetAsync(lgItems.merge_used, 0, 8, h->stream));
		rc = zero_work_counter(h); if (rc) return rc;
		rc = sk_count_select<W>(h, p.ext, p.tracking, p.uni, true, n_items, out, lgItems, k); if (rc) return rc;
		const int grid2 = (int)std::min<uint64_t>((uint64_t)num_cus(h) * k.blocks, n_items);
		rc = sk_count_launch<W>(h, k, grid2, p.ls, p.lc, nl, out, p.f, tv, lgItems); if (rc) return rc;
		LAUNCH(h, sk_merge_emit_kernel<W>, dim3(grid_for(1ull << merge_log2)), dim3(256), 0, lgItems.merge, out, p.f);
		if (merge_log2 < 30) repeat_on = ERR_TABLE_FULL;
		return 0;
	});
}
/* the early count's entries behind this pass's (the slabs' unused tails are holes in both), its counters added */
template <int W> int sk_append_early(kmr_handle *h, SkFinalize<W> &p) {
	FinalizeCounters &c = p.c; const FinalizeCounters &early_c = p.early_c; unsigned long long *cur = p.cur; const uint64_t early_slots = p.early_slots;
	const size_t eb = 8ull * (W + 1);
	if (cur[0] + early_slots > packed_entries(h, h->ue)) {
		DevBuf bigger;
		HIPCHK(h, bigger.alloc(eb * (cur[0] + early_slots + 4096)));
		HIPCHK(h, hipMemcpyAsync(bigger.get(), h->ue.get(), eb * cur[0], hipMemcpyDeviceToDevice, h->stream)); HIPCHK(h, hipStreamSynchronize(h->stream));
		h->ue = std::move(bigger);
	}
	HIPCHK(h, hipMemcpyAsync((uint8_t *)h->ue.get<uint64_t>() + eb * cur[0], h->early.ue.get<uint64_t>(), eb * early_slots, hipMemcpyDeviceToDevice, h->stream));
	cur[0] += early_slots;
	c.unique += early_c.unique; c.singletons += early_c.singletons; c.weak_kept += early_c.weak_kept; c.sing_kept += early_c.sing_kept;
	c.saturated += early_c.saturated; c.sat_sightings += early_c.sat_sightings;
	h->stats.unique_kmers = c.unique; h->stats.singleton_kmers = p.f.has_singletons ? c.singletons : 0;
	return 0;
}

template <int W> int finalize_superkmer_t(kmr_handle *h, uint32_t min_depth) {
	int rc = sync_state(h, true);
	if (rc) return rc;
	TimeSpan whole(h, KMR_TIME_FINALIZE);
	const uint64_t G = h->stats.raw_good_kmers;
	SkFinalize<W> p;
	p.f = finalize_params(h, min_depth);
	p.keepSing = p.f.has_singletons && min_depth <= 1;
	p.ext = h->ext; p.packed = !p.ext;      /* extension values: entries of 15 value words, keys and values apart, bucketed by the scatter + per-bucket sort */
	p.tracking = h->cfg.size_tracker != 0;
	if (!h->l1.head) { rc = pool_reserve(h, h->l1, 0, false); if (rc) return rc; }
	rc = arena_reset(h); if (rc) return rc;
	p.nl = h->sk_state ? sk_list_count(h->sk_bits) : 1;
	if (h->sk_state) {
		LAUNCH(h, sk_close_kernel, dim3(grid_for(p.nl)), dim3(256), 0, h->sk_state.get<unsigned long long>(), p.nl, h->l1.chunk_count.get<uint32_t>(), h->l1.cap);
	}
	p.refined = h->sk_state && h->sk_fine_shift > 0;
	if (p.refined) { rc = sk_refine_lists(h, p.nl); if (rc) return rc; }
	rc = build_csr(h, h->l1, p.nl, 0, &p.ls, &p.lc, &p.nch, p.refined ? nullptr : &h->l1_head_seen); if (rc) return rc;      /* (refining takes chunks) */
	/* entry buffers: sequencing data keeps a few per cent of its k-mers as weak entries */
	rc = sk_count_uniform<W>(h, p.tracking, p.uni, p.f.uni_wbits); if (rc) return rc;
	h->last_count_uniform = p.uni;
	rc = count_entry_buffers(h, p, G, sk_entry_slack(h, sk_count_blocks<W>(h, p.ext, p.tracking, p.uni, false, p.nl)), G / (p.f.has_singletons ? 8 : 3), G / 3, h->sk_exchange && h->cfg.world_size > 1); if (rc) return rc;
	if (p.tracking) { rc = sk_track_view(h, p.tv); if (rc) return rc; }
	p.lgMain = sk_own_lists<W>(h, p.refined);
	bool device_error = false;
	rc = sk_early_takeover<W>(h, p, min_depth, device_error); if (rc) return rc;
	if (device_error) { whole.end(); return sync_state(h); }
	rc = sk_long_items<W>(h, p); if (rc) return rc;
	/* the lists counted, the early count's entries behind them, the maps out of the entries; overflow as finish_maps_t leaves it */
	uint32_t *overflow = nullptr;
	auto count_and_bucket = [&](bool fixed_bins) -> int {
		int rc2 = sk_count_pass<W>(h, p); if (rc2) return rc2;
		h->stats.unique_kmers = p.c.unique; h->stats.singleton_kmers = p.f.has_singletons ? p.c.singletons : 0;
		if (p.tracking && !h->last_bb_fallback) { rc2 = sk_track_elements(h, p.tv, p.f.has_singletons); if (rc2) return rc2; }      /* (a second pass counts the same elements) */
		if (p.early_slots) { rc2 = sk_append_early<W>(h, p); if (rc2) return rc2; }
		h->early.active = false;
		TimeSpan t(h, KMR_TIME_BUCKETS);
		return finish_maps_from_entries(h, p.wc, p.sc, p.cur[0], p.cur[1], p.c.weak_kept, p.c.sing_kept, p.keepSing, overflow, p.packed, fixed_bins);
	};
	h->last_bb_fallback = false;
	rc = count_and_bucket(h->tune.bb_fixed_bins); if (rc) return rc;
	if (overflow) {
		/* bins of one capacity: the partition and the group kernel are on the stream, this is where the host waits for them.  A bin or
		 * group that was fuller than its capacity voids the map, and the packed entries may be overwritten: the lists are counted
		 * again and bucketed with measured bins */
		uint32_t ovf = 0;
		HIPCHK(h, fetch(h, &ovf, overflow));
		if (ovf) {
			if (dbg()) fprintf(stderr, "bucket build: a bin of the radix partition overflowed its capacity, again with measured bins\n");
			h->last_bb_fallback = true;
			rc = count_and_bucket(false); if (rc) return rc;
		}
	}
	h->last_saturated_keys = 0; h->last_saturated_batches = 0;
	if (p.c.saturated) { rc = saturated_fix_t<W>(h, p.ls, p.lc, p.nl, p.c.saturated, p.c.sat_sightings, p.f.has_singletons); if (rc) return rc; }
	whole.end();
	return publish_maps(h, p.keepSing);
}
/* kmr_count_lists_prefix: the count pass over this handle's lists below `hi`, now, into entry buffers of their own -- the lower part of
 * the list space is counted while the upper part is still on the wire; kmr_finalize counts what is left and takes these entries
 * over.  Direction-counting values without a singleton map in the result (min_depth >= 2 or no separate singletons), fine lists only;
 * anything else, or buffers that turn out too small, leaves the lists to kmr_finalize. */
template <int W> int count_prefix_superkmer_t(kmr_handle *h, uint32_t min_depth, uint64_t hi) {
	int rc = sync_state(h, true); if (rc) return rc;
	FinalizeParams f = finalize_params(h, min_depth);
	const bool keepSing = f.has_singletons && min_depth <= 1;
	h->early.active = false;      /* an earlier early count is replaced */
	if (h->ext || h->cfg.size_tracker || keepSing || (h->sk_state && h->sk_fine_shift > 0) || !h->sk_state) return KMR_OK;      /* nothing counted early: kmr_finalize does it all */
	const uint64_t nl = sk_list_count(h->sk_bits);
	if (hi > nl) hi = nl;
	if (hi == 0) return KMR_OK;
	rc = arena_reset(h); if (rc) return rc;
	LAUNCH(h, sk_close_kernel, dim3(grid_for(nl)), dim3(256), 0, h->sk_state.get<unsigned long long>(), nl, h->l1.chunk_count.get<uint32_t>(), h->l1.cap);
	uint64_t *ls = nullptr, *lc = nullptr; uint32_t nch = 0;
	rc = build_csr(h, h->l1, nl, 0, &ls, &lc, &nch, &h->l1_head_seen); if (rc) return rc;
	/* room: the share of the good k-mers that lies below hi, at the rate kmr_finalize starts with.  Too little (low coverage, or an
	 * owner whose lists hold more than its own reads' share) sets ERR_ENTRIES_FULL in the early pass's own error word, which only
	 * kmr_finalize reads: it voids the early count and counts every list itself (kmr_build_info "early_overflowed") */
	const uint64_t G = h->stats.raw_good_kmers;      /* (an owner's lists hold about as many k-mers as its own reads gave: the job's share of one rank) */
	bool uni = false;
	if (!h->peer_uni_mixed) { rc = sk_count_uniform<W>(h, false, uni, f.uni_wbits); if (rc) return rc; }      /* (senders that declared mixed weights settle it here without a look at the device pair) */
	uint64_t want = (uint64_t)((double)G * ((double)hi / (double)nl) / (f.has_singletons ? 6.0 : 2.5)) + sk_entry_slack(h, sk_count_blocks<W>(h, false, false, uni, false, hi));
	if (h->tune.early_entry_share >= 0) { want = (uint64_t)((double)G * h->tune.early_entry_share) + 16384; h->early.ue.reset(); }      /* kmr_tune "early_entry_share" */
	rc = h->early.ue.reserve(h, "early count ue", 8ull * (W + 1) * want); if (rc) return rc;
	rc = h->early.cursor.reserve(h, "early count cursor", 16); if (rc) return rc;
	rc = h->early.fc.reserve(h, "early count fc", sizeof(FinalizeCounters)); if (rc) return rc;
	rc = h->early.err.reserve(h, "early count error word", 4); if (rc) return rc;
	HIPCHK(h, hipMemsetAsync(h->early.cursor.get<unsigned long long>(), 0, 16, h->stream)); HIPCHK(h, hipMemsetAsync(h->early.fc.get(), 0, sizeof(FinalizeCounters), h->stream));
	HIPCHK(h, hipMemsetAsync(h->early.err.get<uint32_t>(), 0, 4, h->stream));      /* (a replaced early count leaves no flag behind) */
	const SkTrackView tv{};
	SkLong<W> lg = sk_own_lists<W>(h, false);
	/* (lists too long for one block are left to kmr_finalize's pass over work items, which covers the whole list space) */
	lg.long_threshold = h->tune.long_list_chunks ? h->tune.long_list_chunks : 1024;
	uint32_t *sc = nullptr;
	rc = arena_get(h, &sc, h->nb_sing); if (rc) return rc;
	HIPCHK(h, hipMemsetAsync(sc, 0, 4 * h->nb_sing, h->stream));
	CountOut out{};      /* packed weak entries only, everything in the early pass's own buffers */
	out.wentries = h->early.ue.get<uint64_t>(); out.wcursor = h->early.cursor.get<unsigned long long>(); out.wcap = packed_entries(h, h->early.ue);
	out.scursor = h->early.cursor.get<unsigned long long>() + 1;
	out.singCount = sc; out.fc = (FinalizeCounters *)h->early.fc.get(); out.err = h->early.err.get<uint32_t>();
	rc = zero_work_counter(h); if (rc) return rc;
	const uint64_t n_work = hi > lg.list_first ? (hi - lg.list_first + lg.list_stride - 1) / lg.list_stride : 0;
	if (n_work) {
		SkCountLaunch<W> k;
		rc = sk_count_select<W>(h, false, false, uni, false, hi, out, lg, k); if (rc) return rc;
		const int grid = (int)std::min<uint64_t>((uint64_t)num_cus(h) * k.blocks, (n_work + SK_LBATCH) / SK_LBATCH);
		TimeSpan t(h, KMR_TIME_COUNT);
		rc = sk_count_launch<W>(h, k, grid, ls, lc, hi, out, f, tv, lg);
		t.end();
		if (rc) return rc;
	}
	h->early.active = true; h->early.hi = hi; h->early.min_depth = min_depth;
	return KMR_OK;      /* asynchronous: the handle's stream carries the pass; kmr_finalize (or kmr_sync) waits for it */
}
int count_prefix_superkmer(kmr_handle *h, uint32_t min_depth, uint64_t hi) { return with_w(h, [&](auto W) { return count_prefix_superkmer_t<W()>(h, min_depth, hi); }); }
int finalize_superkmer(kmr_handle *h, uint32_t min_depth) { return with_w(h, [&](auto W) { return finalize_superkmer_t<W()>(h, min_depth); }); }

/* the device memory of group M of the handle goes back (kmr_handle's bases) */
template <class M> void release(kmr_handle *h) { static_cast<M &>(*h) = M(); }

void free_partition_state(kmr_handle *h) {
	release<BuildMem>(h);
	if (h->tb_copy_stream) { hipStreamDestroy(h->tb_copy_stream); h->tb_copy_stream = nullptr; for (int a = 0; a < 2; a++) { hipEventDestroy(h->tb_ready[a]); hipEventDestroy(h->tb_consumed[a]); h->tb_set_used[a] = false; } }
}

}  // namespace

/* ====================================================================== */
extern "C" {

uint32_t kmr_abi_version(void) { return KMR_ABI_VERSION; }

int kmr_config_init(kmr_config *c) {
	if (!c) return KMR_ERR_INVALID_ARG;
	memset(c, 0, sizeof(*c));
	c->struct_size = sizeof(*c);
	c->value_kind = KMR_VALUE_COUNT_DIR; c->min_weight = 0.10f; c->min_quality_score = 3; c->fastq_start_char = 33;
	c->ext_min_quality = 20; c->separate_singletons = 1; c->kmer_subsample = 1; c->device = -1; c->rank = 0; c->world_size = 1;
	c->estimated_depth = 20.0; c->estimated_error_rate = 0.35; c->kmers_per_bucket = 32; c->num_parts = 1; c->part_idx = 0;
	return KMR_OK;
}

const char *kmr_last_error(const kmr_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int kmr_create(const kmr_config *cfg, kmr_handle **out) {
	if (!cfg || !out) return fail(nullptr, KMR_ERR_INVALID_ARG, "null argument");
	*out = nullptr;
	if (cfg->struct_size != sizeof(kmr_config)) return fail(nullptr, KMR_ERR_INVALID_ARG, "kmr_config.struct_size mismatch (ABI)");
	if (cfg->k < 1 || cfg->k > 128) return fail(nullptr, KMR_ERR_INVALID_ARG, "k must be in 1..128");
	if (cfg->world_size < 1 || cfg->rank >= cfg->world_size) return fail(nullptr, KMR_ERR_INVALID_ARG, "bad rank/world_size");
	if (cfg->value_kind > KMR_VALUE_EXT) return fail(nullptr, KMR_ERR_INVALID_ARG, "bad value_kind");
	if (cfg->hash_kind > KMR_HASH_LOOKUP8) return fail(nullptr, KMR_ERR_INVALID_ARG, "bad hash_kind");
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, KMR_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
	kmr_handle *h = new kmr_handle();
	h->cfg = *cfg;
	if (h->cfg.kmer_subsample == 0) h->cfg.kmer_subsample = 1;
	if (h->cfg.num_parts == 0) h->cfg.num_parts = 1;
	h->k = cfg->k; h->kb = (cfg->k + 3) / 4; h->W = (h->kb + 7) / 8; h->ext = cfg->value_kind == KMR_VALUE_EXT;
	h->hkb = h->kb | (cfg->hash_kind << 16);      /* what the kernels' hash sees: key bytes and the hash kind (kmr_key.hpp, key_hash) */
	memset(&h->stats, 0, sizeof(h->stats));
	int rc = 0;
	do {
		if (cfg->device >= 0) { if (hipSetDevice(cfg->device) != hipSuccess) { rc = fail(nullptr, KMR_ERR_NO_DEVICE, "hipSetDevice failed"); break; } }
		if (hipGetDevice(&h->device) != hipSuccess) { rc = fail(nullptr, KMR_ERR_NO_DEVICE, "hipGetDevice failed"); break; }
		if (hipStreamCreate(&h->stream) != hipSuccess) { rc = fail(nullptr, KMR_ERR_HIP, "hipStreamCreate failed"); break; }
		/* bucket sizing of the KmerSpectrum ctor (src/KmerSpectrum.h:414-416, src/Kmer.h:2837) */
		uint64_t w = cfg->num_buckets_weak, s = cfg->num_buckets_singleton;
		const double depth = cfg->estimated_depth > 0 ? cfg->estimated_depth : 20.0;
		const uint32_t kpb = cfg->kmers_per_bucket ? cfg->kmers_per_bucket : 32;
		/* estimated_raw_kmers is the whole job's; a rank's maps are built for its share, the figure
		 * DistributedKmerSpectrum::estimateRawKmers (src/DistributedFunctions.h:144-162) hands the constructor */
		const uint64_t raw = cfg->estimated_raw_kmers / (cfg->world_size > 1 ? cfg->world_size : 1);
		if (w == 0) { unsigned long est = (unsigned long)(int)(raw / depth); w = est / kpb + 1; }
		if (s == 0) { unsigned long est = cfg->separate_singletons ? (unsigned long)(raw * cfg->estimated_error_rate) : 1; s = est / kpb + 1; }
		h->nb_weak = resize_buckets(w); h->nb_sing = resize_buckets(s);
		h->has_singletons = cfg->separate_singletons != 0;
		/* table capacity */
		uint64_t want = cfg->max_table_entries ? (uint64_t)(cfg->max_table_entries / 0.7) : (uint64_t)(cfg->estimated_raw_kmers * 0.45 / 0.6);
		if (cfg->world_size > 1 && !cfg->max_table_entries) want /= cfg->world_size;
		uint32_t lg = 16; while ((1ull << lg) < want && lg < 40) lg++;
		h->log2cap = lg;
		double P[256]; quality_table(P, cfg->min_quality_score, cfg->fastq_start_char);
		if (h->dP.alloc(sizeof(P)) != hipSuccess || h->dstats.alloc(sizeof(DevStats)) != hipSuccess || h->derr.alloc(4) != hipSuccess) { rc = fail(nullptr, KMR_ERR_OOM, "hipMalloc failed"); break; }
		hipMemcpy(h->dP.get<double>(), P, sizeof(P), hipMemcpyHostToDevice); hipMemset(h->dstats.get<DevStats>(), 0, sizeof(DevStats)); hipMemset(h->derr.get<uint32_t>(), 0, 4);
		/* build_mode: 0 auto (streaming partition path unless EXT values), 1 table, 2 partition */
		if (cfg->build_mode > 3) { rc = fail(nullptr, KMR_ERR_INVALID_ARG, "bad build_mode"); break; }
		h->partition_mode = cfg->build_mode != 1;
		/* auto: super-k-mer lists where they apply (count / direction values, one partition, k >= 13), else the two-level k-mer partition */
		uint32_t wish_w = 0, wish_m = 0, wish_o = 0;
		const bool sk_auto = cfg->build_mode == 0 && cfg->world_size <= 1 && sk_geometry(h->k, 0, wish_w, wish_m, wish_o);
		h->auto_mode = cfg->build_mode == 0;
		/* (an auto handle of a multi-rank job starts on the k-mer partition -- plain kmr_add_reads* there means the getDistributedThreadId
		 * filter -- but is made ready for the lists: kmr_exchange_init moves it over) */
		/* (and any handle whose k has a minimizer geometry can answer lookups as a streaming pass over the same lists) */
		const bool sk_ready = sk_geometry(h->k, 0, wish_w, wish_m, wish_o);
		if (cfg->build_mode == 3 || sk_auto || sk_ready) {
			if (!sk_geometry(h->k, 0, h->sk_win, h->sk_m, h->sk_off)) { rc = fail(nullptr, KMR_ERR_UNSUPPORTED, "build_mode 3 (super-k-mer lists) needs k >= 13"); break; }
			h->superkmer_mode = cfg->build_mode == 3 || sk_auto;
			double Pk[256];
			for (int cidx = 0; cidx < 256; cidx++) { double wv = 1.0; for (uint32_t jj = 0; jj < h->k; jj++) wv *= P[cidx]; Pk[cidx] = wv; }      /* the loop of buildWeightedKmers, src/KmerReadUtils.h:205-208 */
			memcpy(h->hPk, Pk, sizeof(Pk)); memcpy(h->hP, P, sizeof(h->hP));
			if (h->dPk.alloc(2 * sizeof(Pk)) != hipSuccess) { rc = fail(nullptr, KMR_ERR_OOM, "hipMalloc failed"); break; }
			hipMemcpy(h->dPk.get<double>(), Pk, sizeof(Pk), hipMemcpyHostToDevice);
			/* reciprocals for the chain's divide, usable only if multiply-and-correct reproduces the correctly rounded quotient of every
			 * pair of table entries (all 256 x 256 are tried; the kernel divides otherwise) */
			double Rp[256]; bool fast = true;
			for (int cidx = 0; cidx < 256; cidx++) Rp[cidx] = P[cidx] != 0.0 ? 1.0 / P[cidx] : 0.0;
			for (int a = 0; a < 256 && fast; a++) for (int b = 0; b < 256; b++) {
				if (P[a] == 0.0 || P[b] == 0.0) continue;
				const double q0 = P[a] * Rp[b];
				if (std::fma(std::fma(-q0, P[b], P[a]), Rp[b], q0) != P[a] / P[b]) { fast = false; break; }
			}
			h->sk_fast_div = fast;
			hipMemcpy(h->dPk.get<double>() + 256, Rp, sizeof(Rp), hipMemcpyHostToDevice);
		}
		if (cfg->size_tracker && (!h->superkmer_mode || h->ext || cfg->world_size > 1)) { rc = fail(nullptr, KMR_ERR_UNSUPPORTED, "size_tracker: kept by the super-k-mer build (build_mode 0 / 3, direction-counting values, k >= 13) of a single partition"); break; }
		if (!h->partition_mode) {
			rc = alloc_table(h, h->log2cap, h->slots, h->extslots);
			if (rc) { g_create_error = h->err; break; }
		}
		if (hipStreamSynchronize(h->stream) != hipSuccess) { rc = fail(nullptr, KMR_ERR_HIP, std::string("table clear failed: ") + hipGetErrorString(hipGetLastError())); break; }
	} while (0);
	if (rc) { kmr_destroy(h); return rc; }
	*out = h;
	return KMR_OK;
}

static void exchange_destroy_comm(kmr_handle *h);
void kmr_destroy(kmr_handle *h) {
	if (!h) return;
	if (h->stream) hipStreamSynchronize(h->stream);
	for (int which = 0; which < KMR_TIME_GROUPS; which++) for (auto &pr : h->pending_events[which]) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
	release<HandleMem>(h);
	free_partition_state(h);
	exchange_destroy_comm(h);
	release<ExchangeMem>(h);      /* what the communicator used */
	if (h->stream) hipStreamDestroy(h->stream);
	delete h;
}

int kmr_num_buckets(const kmr_handle *h, int which, uint64_t *out) {
	if (!h || !out) return KMR_ERR_INVALID_ARG;
	if (which == KMR_MAP_WEAK) *out = h->finalized && h->weak.present ? h->weak.nb : h->nb_weak;
	else if (which == KMR_MAP_SINGLETON) *out = h->finalized && h->sing.present ? h->sing.nb : h->nb_sing;
	else return KMR_ERR_UNSUPPORTED;
	return KMR_OK;
}

/* KmerSpectrum::buildKmerSpectrum starts with weak.reset(false); singleton.reset(false)
 * (src/KmerSpectrum.h:2091-2096): empty maps, allocations kept. */
int kmr_reset(kmr_handle *h) {
	if (!h) return KMR_ERR_INVALID_ARG;
	hipSetDevice(h->device);
	HIPCHK(h, hipStreamSynchronize(h->stream));
	clear_map(h->weak); clear_map(h->sing);      /* empty maps, allocations kept (reset(false)) */
	int rc = 0;
	if (h->partition_mode) {
		if (h->l1.head) HIPCHK(h, hipMemsetAsync(h->l1.head.get<unsigned int>(), 0, 4, h->stream));
		h->l1.used_ub = 0;
		h->inserted_records = 0;
		h->qual_mixed = false;
		h->sk_uni_w = SK_UNI_NONE; h->sk_uni_mixed = false; h->peer_uni_w = SK_UNI_NONE; h->peer_uni_mixed = false; h->peers_declare = false;
		h->xr_lo = 0; h->xr_hi = ~0ull; h->early.active = false;
		if (h->d_uni) { const uint32_t init[2] = {SK_UNI_NONE, 0u}; HIPCHK(h, hipMemcpyAsync(h->d_uni.get<uint32_t>(), init, 8, hipMemcpyHostToDevice, h->stream)); HIPCHK(h, hipStreamSynchronize(h->stream)); }
		if (h->sk_state) LAUNCH(h, sk_state_init_kernel, dim3(grid_for(sk_list_count(h->sk_bits))), dim3(256), 0, h->sk_state.get<unsigned long long>(), sk_list_count(h->sk_bits));
		if (h->l1_state) {      /* what an unfinished build kept back is dropped with its pool */
			LAUNCH(h, partition_state_init_kernel, dim3(partition_blocks(h)), dim3(256), 0, h->l1_state.get<uint8_t>(),
			       h->l1_state.cap() / (size_t)partition_blocks(h), h->bits1, (uint32_t)partition_blocks(h));
			h->l1_state_dirty = false;
		}
	} else {
		if (!h->slots) rc = alloc_table(h, h->log2cap, h->slots, h->extslots);
		else rc = clear_table_any(h, h->slots.get(), h->extslots.get<ExtSlot>(), h->log2cap);
		if (rc) return rc;
	}
	HIPCHK(h, hipMemsetAsync(h->dstats.get<DevStats>(), 0, sizeof(DevStats), h->stream));
	HIPCHK(h, hipMemsetAsync(h->derr.get<uint32_t>(), 0, 4, h->stream));
	memset(&h->stats, 0, sizeof(h->stats));
	h->occupied = h->pending_kmers = 0; h->stream_base = 0; h->reads = 0; h->ord_lo = h->ord_hi = 0; h->ord_seen = h->ord_foreign = false; h->subtracted = 0; h->xc_job_bases = 0; h->xc_bytes_to_peers = 0;
	h->trk_n = 0; h->trk_elems.clear();
	h->trk_next = 128; h->trk_raw = h->trk_good = 0; h->trk_bounds.clear(); h->trk_snap_raw.clear(); h->trk_snap_good.clear();
	h->finalized = false; h->map_gen++; h->has_singletons = h->cfg.separate_singletons != 0;
	return KMR_OK;
}
int kmr_release_table(kmr_handle *h) {
	if (!h) return KMR_ERR_INVALID_ARG;
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_release_table before kmr_finalize");
	hipSetDevice(h->device);
	h->slots.reset(); h->extslots.reset();
	if (h->partition_mode) free_partition_state(h);
	return KMR_OK;
}

void *kmr_stream(kmr_handle *h) { return h ? (void *)h->stream : nullptr; }

/* the stream ordinal the next kmr_add_reads* starts from (see the header) */
int kmr_set_stream_origin(kmr_handle *h, uint64_t ordinal) {
	if (!h) return KMR_ERR_INVALID_ARG;
	if (h->finalized) return fail(h, KMR_ERR_STATE, "kmr_set_stream_origin after kmr_finalize");
	if (ordinal > MAX_STREAM_ORDINAL) return fail(h, KMR_ERR_CAPACITY, "stream ordinals have 40 bits");
	h->stream_base = ordinal;
	return KMR_OK;
}

/* knobs of one handle (see struct Tuning); set before the first kmr_add_reads* of a build */
int kmr_tune(kmr_handle *h, const char *knob, double value) {
	if (!h || !knob) return KMR_ERR_INVALID_ARG;
	const std::string k(knob);
	if (k == "target_list_records") h->tune.target_list = value >= 1 ? (uint64_t)value : 2048;
	else if (k == "sub_batch_bases") h->tune.sub_batch_bases = value >= 1 ? (uint64_t)value : 0;
	else if (k == "recycle_chunks") h->tune.recycle = value < 0 ? -1 : (value != 0 ? 1 : 0);
	else if (k == "partition_blocks") h->tune.part_blocks = value >= 1 ? (int)value : 0;
	else if (k == "entry_share") h->tune.entry_share = value;
	else if (k == "early_entry_share") h->tune.early_entry_share = value;
	else if (k == "saturated_batch_bytes") h->tune.saturated_batch_bytes = value >= 1 ? (uint64_t)value : 0;
	else if (k == "lookup_table") h->tune.no_lut = value == 0;
	else if (k == "stream_lookups") h->tune.no_stream_lookups = value == 0;
	else if (k == "long_list_chunks") h->tune.long_list_chunks = value < 2 ? 2 : (uint64_t)value;
	else if (k == "lean_extract") h->tune.no_lean_extract = value == 0;
	else if (k == "uniform_count") h->tune.no_uniform_count = value == 0;
	else if (k == "count_blocks") { if (value != 0 && value != 4 && value != 5) return fail(h, KMR_ERR_INVALID_ARG, "count_blocks is 0 (default), 4 or 5"); h->tune.count_blocks = (int)value; }
	else if (k == "count_six") { if (value != 0 && value != 1 && value != 2) return fail(h, KMR_ERR_INVALID_ARG, "count_six is 0 (default), 1 (wherever the ordinals allow) or 2 (never)"); h->tune.count_six = (int)value; }
	else if (k == "packed_direct") h->tune.no_packed_direct = value == 0;
	else if (k == "pow2_lists") h->tune.pow2_lists = value != 0;
	else if (k == "list_aim") h->tune.list_aim = value >= 1 ? (uint64_t)value : 0;
	else if (k == "twobit_piece_bases") h->tune.twobit_piece_bases = (uint64_t)value;
	else if (k == "exchange_fail_once") h->tune.exchange_fail_once = value != 0;
	else if (k == "binned_buckets_min") h->tune.binned_min = value >= 0 ? (uint64_t)value : ~0ull;        /* < 0: never */
	else if (k == "bb_fixed_bins") h->tune.bb_fixed_bins = value != 0;
	else if (k == "bb_slack_bins") h->tune.bb_slack_bins = value;
	else if (k == "bb_slack_groups") h->tune.bb_slack_groups = value;
	else if (k == "bb_reload") h->tune.bb_reload = value != 0;
	else if (k == "coarse_lists") h->tune.no_coarse_lists = value == 0;
	else if (k == "select_timing") h->tune.select_timing = value != 0;
	else if (k == "dump_timing") h->tune.dump_timing = value != 0;
	else if (k == "pairs_timing") h->tune.pairs_timing = value != 0;
	else if (k == "dedup_timing") h->tune.dedup_timing = value != 0;
	else if (k == "bimodal_window") h->tune.bimodal_window = value >= 0 && value <= BM_CAP ? (int)value : -1;
	else if (k == "partition_units") h->tune.partition_units = value >= 1 && value <= 8192 ? (uint32_t)value : 0;
	else if (k == "artifact_report_lds") h->tune.artifact_report_lds = value == 0 ? 0 : value == 1 ? 1 : -1;
	else if (k == "pair_hash_bits") h->tune.pair_hash_bits = value >= 1 && value < 64 ? (uint32_t)value : 64;
	else if (k == "dump_piece_bytes") h->tune.dump_piece_bytes = value >= 1 ? (uint64_t)value : 0;
	else if (k == "dump_tiles_per_block") h->tune.dump_tiles_per_block = value >= 1 ? (uint64_t)std::min(value, 4294967296.0) : 0;
	else if (k == "narrow_tallies") h->tune.no_narrow = value == 0;
	else if (k == "keep_level1_state") h->tune.no_l1_state = value == 0;
	else if (k == "csr_partition") h->tune.csr_partition = value != 0;
	else if (k == "compare_lds_kmers") h->tune.compare_lds_kmers = value >= 0 && value <= CMP_CAP_MOST ? (int)value : -1;
	else if (k == "compare_stage_kmers") h->tune.compare_stage_kmers = value >= 1 ? std::min<uint64_t>((uint64_t)value, 1ull << 31) : 0;
	else if (k == "tnf_piece_bases") h->tune.tnf_piece_bases = value >= 1 ? (uint32_t)std::min<double>(value, 1u << 30) : 0;
	else if (k == "match_hit_capacity") h->tune.match_hit_capacity = value >= 1 ? (uint64_t)std::min<double>(value, 4294967294.0) : 0;
	else if (k == "extend_stage_kmers") h->tune.extend_stage_kmers = value >= 1 ? std::min<uint64_t>((uint64_t)value, 1ull << 31) : 0;
	else if (k == "extend_timing") h->tune.extend_timing = value != 0;
	else if (k == "superkmer_window") {      /* largest minimizer window the geometry may take (32 / 16 / 8 / 4): A/B runs, tests of the narrower windows at large k */
		if (h->superkmer_mode && !h->sk_state) { uint32_t w, m, o; if (!sk_geometry(h->k, 0, w, m, o, (uint32_t)value)) return fail(h, KMR_ERR_INVALID_ARG, "no minimizer geometry under that window"); h->sk_win = w; h->sk_m = m; h->sk_off = o; }
	}
	else if (k == "superkmer_minimizer") {
		if (h->superkmer_mode && !h->sk_state) { uint32_t w, m, o; if (!sk_geometry(h->k, (uint32_t)value, w, m, o)) return fail(h, KMR_ERR_INVALID_ARG, "no minimizer geometry for that length"); h->sk_win = w; h->sk_m = m; h->sk_off = o; }
	}
	else return fail(h, KMR_ERR_INVALID_ARG, "unknown tuning knob '" + k + "'");
	return KMR_OK;
}

int kmr_build_info(kmr_handle *h, const char *what, double *value) {
	if (!h || !what || !value) return KMR_ERR_INVALID_ARG;
	const std::string k(what);
	if (k == "lists") *value = h->sk_state ? (double)sk_list_count(h->sk_bits) : 0.0;
	else if (k == "uniform_count") *value = h->last_count_uniform ? 1.0 : 0.0;
	else if (k == "count_blocks") *value = (double)h->last_count_blocks;
	else if (k == "chunk_pool_chunks") *value = (double)h->l1.cap;
	else if (k == "superkmer_window") *value = (double)h->sk_win;
	else if (k == "early_lists") *value = (double)h->last_early_hi;
	else if (k == "early_entries") *value = (double)h->last_early_entries;
	else if (k == "early_overflowed") *value = h->last_early_overflowed ? 1.0 : 0.0;
	else if (k == "bb_path") *value = (double)h->last_bb_path;
	else if (k == "bb_fallback") *value = h->last_bb_fallback ? 1.0 : 0.0;
	else if (k == "score_path") *value = (double)h->last_score_path;
	else if (k == "saturated_keys") *value = (double)h->last_saturated_keys;
	else if (k == "saturated_batches") *value = (double)h->last_saturated_batches;
	else if (k == "count_attempts") *value = (double)h->last_count_attempts;
	else if (k == "csr_path") *value = (double)h->last_csr_path;
	else if (k == "csr_chunks") *value = (double)h->last_csr_chunks;
	else if (k == "unit_batches") *value = (double)h->unit_batches;
	else if (k == "match_add_attempts") *value = (double)h->last_match_attempts;
	else if (k == "extend_runs") *value = (double)h->last_extend_runs;
	else if (k == "extend_gather_ms") *value = h->last_extend_ms[0];
	else if (k == "extend_extract_ms") *value = h->last_extend_ms[1];
	else if (k == "extend_sort_ms") *value = h->last_extend_ms[2];
	else if (k == "extend_reduce_ms") *value = h->last_extend_ms[3];
	else if (k == "extend_walk_ms") *value = h->last_extend_ms[4];
	else if (k == "device_blocks_live") *value = (double)g_blocks_live.load();
	else if (k == "filter_score_ms") *value = h->last_score_ms;
	else if (k == "select_ms") *value = h->last_select_ms;
	else if (k == "select_write_ms") *value = h->last_write_ms;
	else if (k == "artifact_report_lds") *value = h->last_artifact_report_lds;
	else if (k == "pairs_ms") *value = h->last_pairs_ms;
	else if (k == "pairs_parse_ms") *value = h->last_pairs_parse_ms;
	else if (k == "pairs_sort_ms") *value = h->last_pairs_sort_ms;
	else if (k == "pair_hash_collisions") *value = (double)h->last_pair_hash_collisions;
	else if (k == "dedup_ms") *value = h->last_dedup_ms;
	else if (k == "dedup_key_ms") *value = h->last_dedup_key_ms;
	else if (k == "dedup_sort_ms") *value = h->last_dedup_sort_ms;
	else if (k == "dedup_consensus_ms") *value = h->last_dedup_consensus_ms;
	else if (k == "dump_size_ms") *value = h->last_dump_size_ms;
	else if (k == "dump_write_ms") *value = h->last_dump_write_ms;
	else if (k == "dump_tiles_per_block") *value = (double)h->last_dump_tiles_per_block;
	else if (k == "dump_blocks") *value = (double)h->last_dump_blocks;
	else return fail(h, KMR_ERR_INVALID_ARG, "unknown build figure '" + k + "'");
	return KMR_OK;
}

int kmr_sync(kmr_handle *h) { if (!h) return KMR_ERR_INVALID_ARG; hipSetDevice(h->device); return sync_state(h); }

/* Reads on the device go into the build: the one form the feed entry points end in, behind their own argument checks (dev_bases
 * is null where hints.packed holds the batch).  hints: what the caller knows of this call, FeedHints */
static int add_reads_dev_call(kmr_handle *h, const void *dev_bases, const void *dev_quals, const void *dev_offsets, uint64_t n_reads, uint64_t total_bases, uint64_t first_global_read_idx, const void *dev_discarded, const FeedHints &hints) {
	const ReadsView rv = reads_view(dev_bases, dev_quals, dev_offsets, n_reads, dev_discarded, h->stream_base - hints.piece_origin, first_global_read_idx);
	/* the stream ordinal of an occurrence decides which sighting of a k-mer was its first (directionBias, the quantised first
	 * weight): 40 bits in the table slots, and the 16-byte records of build_mode 2 without extension values carry 32 of them */
	if (h->stream_base + total_bases > MAX_STREAM_ORDINAL) return fail(h, KMR_ERR_CAPACITY, "more than 2^40 input bases on one handle");
	if (h->partition_mode && !h->superkmer_mode && !h->ext && h->stream_base + total_bases > (1ull << 32))
		return fail(h, KMR_ERR_CAPACITY, "build_mode 2 orders occurrences by a 32-bit stream ordinal: at most 2^32 input bases per handle without extension values (use build_mode 0 / 3 or 1)");
	int rc = h->superkmer_mode ? add_reads_superkmer(h, rv, total_bases, hints) : (h->partition_mode ? add_reads_partition(h, rv, total_bases) : add_reads_dev_any(h, rv, total_bases));
	h->stream_base += total_bases; h->reads += n_reads; h->stats.reads = h->reads;
	return rc;
}
int kmr_add_reads_dev(kmr_handle *h, const void *dev_bases, const void *dev_quals, const void *dev_offsets, uint64_t n_reads,
                      uint64_t total_bases, uint64_t first_global_read_idx, const void *dev_discarded) {
	if (!h) return KMR_ERR_INVALID_ARG;
	if (h->finalized) return fail(h, KMR_ERR_STATE, "kmr_add_reads after kmr_finalize");
	if (n_reads == 0) return KMR_OK;
	if (!dev_bases || !dev_offsets) return fail(h, KMR_ERR_INVALID_ARG, "null device buffer");
	hipSetDevice(h->device);
	return add_reads_dev_call(h, dev_bases, dev_quals, dev_offsets, n_reads, total_bases, first_global_read_idx, dev_discarded, FeedHints());
}

/* one piece of a host batch onto the device: staging set `set` of the handle (grow-only), the copy on the handle's copy stream */
static hipError_t tb_stage_copy(kmr_handle *h, int set, int which, const void *src, size_t bytes, void **dst) {
	DevBuf &buf = h->tb_stage[set][which];
	if (buf.cap() < bytes + 128) {      /* the piece, 64 bytes of padding behind it and 64 to spare */
		if (buf) { hipError_t e0 = hipStreamSynchronize(h->stream); if (e0 != hipSuccess) return e0; }
		hipError_t e = buf.alloc(bytes + bytes / 8 + 4096); if (e != hipSuccess) return e;
	}
	*dst = buf.get();
	return bytes ? hipMemcpyAsync(buf.get(), src, bytes, hipMemcpyHostToDevice, h->tb_copy_stream) : hipSuccess;
}
static int tb_pipeline_ready(kmr_handle *h) {
	if (h->tb_copy_stream) return 0;
	HIPCHK(h, hipStreamCreateWithFlags(&h->tb_copy_stream, hipStreamNonBlocking));
	for (int i = 0; i < 2; i++) { HIPCHK(h, hipEventCreateWithFlags(&h->tb_ready[i], hipEventDisableTiming)); HIPCHK(h, hipEventCreateWithFlags(&h->tb_consumed[i], hipEventDisableTiming)); }
	return 0;
}

/* a failed HIP call of the piece pipeline: both streams drained before the error goes back */
#define TBCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { hipStreamSynchronize(h->tb_copy_stream); hipStreamSynchronize(h->stream); h->err = std::string(#call) + ": " + hip_err_text(e_); return e_ == hipErrorOutOfMemory ? KMR_ERR_OOM : KMR_ERR_HIP; } } while (0)
/* A host batch goes over in pieces of about 2^28 bases (kmr_tune "twobit_piece_bases") through two sets of staging buffers and a copy
 * stream of the handle's own: while the device extracts piece i, piece i + 1 is on the bus (the host's pageable memory: the calling
 * thread feeds the copies, the device does not wait for it).  stage(set, r0, r1) puts the copies of reads [r0, r1) on the copy stream
 * (tb_stage_copy into staging set `set`), feed(r0, r1, call_bases) hands the staged piece to the device entry; both return a KMR code.  Per piece:
 * wait for the set's last piece to be consumed, stage, record ready, the handle's stream waits for it, feed, record consumed. */
}  // extern "C"
template <class Stage, class Feed> static int tb_feed_pieces(kmr_handle *h, const uint64_t *offsets, uint64_t n_reads, Stage &&stage, Feed &&feed) {
	{ int rcp = tb_pipeline_ready(h); if (rcp) return rcp; }
	const uint64_t piece_bases = h->tune.twobit_piece_bases ? h->tune.twobit_piece_bases : (1ull << 28);
	int rc = KMR_OK; int set = 0;
	const uint64_t call_bases = n_reads ? offsets[n_reads] - offsets[0] : 0;      /* what the first piece sizes is the whole call's (FeedHints) */
	for (uint64_t r0 = 0; r0 < n_reads && rc == KMR_OK; set ^= 1) {
		uint64_t r1 = r0 + 1;
		while (r1 < n_reads && offsets[r1 + 1] - offsets[r0] <= piece_bases) r1++;
		if (h->tb_set_used[set]) TBCHK(hipStreamWaitEvent(h->tb_copy_stream, h->tb_consumed[set], 0));      /* the piece that used this set last has been extracted */
		{ int rcs = stage(set, r0, r1); if (rcs) return rcs; }
		TBCHK(hipEventRecord(h->tb_ready[set], h->tb_copy_stream));
		TBCHK(hipStreamWaitEvent(h->stream, h->tb_ready[set], 0));
		rc = feed(r0, r1, call_bases);
		TBCHK(hipEventRecord(h->tb_consumed[set], h->stream)); h->tb_set_used[set] = true;
		r0 = r1;
	}
	hipStreamSynchronize(h->tb_copy_stream);
	if (!rc) rc = sync_state(h);
	else hipStreamSynchronize(h->stream);
	return rc;
}
extern "C" {

int kmr_add_reads(kmr_handle *h, const char *bases, const char *quals, const uint64_t *offsets, uint64_t n_reads,
                  uint64_t first_global_read_idx, const uint8_t *discarded) {
	if (!h) return KMR_ERR_INVALID_ARG;
	if (h->finalized) return fail(h, KMR_ERR_STATE, "kmr_add_reads after kmr_finalize");
	if (n_reads == 0) return KMR_OK;
	if (!bases || !offsets) return fail(h, KMR_ERR_INVALID_ARG, "null buffer");
	hipSetDevice(h->device);
	/* the offsets go over as they are (the device arrays are addressed through pointers moved back by the piece's first offset) */
	void *db = nullptr, *dq = nullptr, *doff = nullptr, *dd = nullptr;
	auto stage = [&](int set, uint64_t r0, uint64_t r1) -> int {
		const uint64_t m = r1 - r0, total = offsets[r1] - offsets[r0];
		dq = nullptr; dd = nullptr;
		TBCHK(tb_stage_copy(h, set, 0, bases + offsets[r0], total, &db)); TBCHK(tb_stage_copy(h, set, 2, offsets + r0, 8 * (m + 1), &doff));
		if (quals) TBCHK(tb_stage_copy(h, set, 6, quals + offsets[r0], total, &dq));
		if (discarded) TBCHK(tb_stage_copy(h, set, 7, discarded + r0, m, &dd));
		TBCHK(hipMemsetAsync((uint8_t *)db + total, 0, 64, h->tb_copy_stream)); if (dq) TBCHK(hipMemsetAsync((uint8_t *)dq + total, 0, 64, h->tb_copy_stream));
		return KMR_OK;
	};
	auto feed = [&](uint64_t r0, uint64_t r1, uint64_t call_bases) {
		return add_reads_dev_call(h, (uint8_t *)db - offsets[r0], dq ? (uint8_t *)dq - offsets[r0] : nullptr, doff, r1 - r0, offsets[r1] - offsets[r0], first_global_read_idx + r0, dd, FeedHints{nullptr, -1, call_bases, offsets[r0]});
	};
	return tb_feed_pieces(h, offsets, n_reads, stage, feed);
}

/* May sk_extract_lean_kernel<.., PACKED> take a packed batch as it is?  Whenever add_reads_superkmer_t would hand the unpacked
 * batch to the lean extraction: lists, direction-counting values, nothing that filters k-mers, and one weight for every k-mer. */
static bool sk_packed_direct_ok(kmr_handle *h, bool has_quals, int uniform_quality) {
	if (!h->superkmer_mode || h->ext || h->cfg.size_tracker || h->tune.no_lean_extract || h->tune.no_packed_direct || sp_debug_extract(h) || has_quals || h->qual_mixed) return false;
	if (sk_build_filters(h, dev_params(h))) return false;
	bool lean = true; float wK = 1.0f;
	if (uniform_quality) sk_weight_of_quality(h, (unsigned int)uniform_quality, lean, wK);
	return lean;
}
/* kmr_add_reads_twobit_dev, and a piece of kmr_add_reads_twobit (call_bases: the bases of that whole call, FeedHints) */
static int add_reads_twobit_dev_call(kmr_handle *h, const void *dev_twobit, const void *dev_twobit_offsets, const void *dev_offsets, const void *dev_markup_offsets, const void *dev_markup_pos, const void *dev_markup_char,
                                     const void *dev_quals, int uniform_quality, uint64_t n_reads, uint64_t total_bases, uint64_t first_global_read_idx, const void *dev_discarded, uint64_t call_bases) {
	if (h->finalized) return fail(h, KMR_ERR_STATE, "kmr_add_reads after kmr_finalize");
	if (n_reads == 0) return KMR_OK;
	if (!dev_twobit || !dev_offsets) return fail(h, KMR_ERR_INVALID_ARG, "null device buffer");
	if (dev_markup_offsets && (!dev_markup_pos || !dev_markup_char)) return fail(h, KMR_ERR_INVALID_ARG, "markup offsets without markups");
	if (uniform_quality < 0 || uniform_quality > 255 || (dev_quals && uniform_quality)) return fail(h, KMR_ERR_INVALID_ARG, "uniform_quality: 0, or the one quality character of a batch without a quality array");
	hipSetDevice(h->device);
	/* grow-only scratch of the handle; everything below is ordered on the handle's stream, so the next call's unpack waits for
	 * this call's extraction */
	const bool direct = sk_packed_direct_ok(h, dev_quals != nullptr, uniform_quality);
	FeedHints hints; hints.call_bases = call_bases; hints.uniform_q = (!dev_quals && uniform_quality) ? uniform_quality : -1;
	if (!direct && h->tb_bases.cap() < total_bases + 64) {
		if (h->tb_bases) HIPCHK(h, hipStreamSynchronize(h->stream));
		HIPCHK(h, h->tb_bases.alloc(total_bases + 64));
		HIPCHK(h, hipMemsetAsync(h->tb_bases.get<uint8_t>(), 0, total_bases + 64, h->stream));
	}
	if (h->tb_len.cap() < 4 * (n_reads + 1)) {      /* (tb_len is allocated last) */
		if (h->tb_len) HIPCHK(h, hipStreamSynchronize(h->stream));
		h->tb_rel.reset(); h->tb_off.reset(); h->tb_len.reset();
		HIPCHK(h, h->tb_rel.alloc(8 * (n_reads + 1))); HIPCHK(h, h->tb_off.alloc(8 * (n_reads + 1))); HIPCHK(h, h->tb_len.alloc(4 * (n_reads + 1)));
	}
	const uint64_t *tboff = (const uint64_t *)dev_twobit_offsets;
	if (!tboff) {      /* every read on the byte behind the one before it: ceil(L / 4) bytes each */
		int rc = twobit_byte_offsets(h, (const uint64_t *)dev_offsets, n_reads, h->tb_len.get<uint32_t>(), h->tb_off.get<uint64_t>()); if (rc) return rc;
		tboff = h->tb_off.get<uint64_t>();
	}
	if (direct) {
		/* the lean extraction stages the packed bytes as they are: no unpacked copy of the batch, no quality bytes */
		{ int rc = twobit_rel_offsets(h, (const uint64_t *)dev_offsets, n_reads, h->tb_rel.get<uint64_t>()); if (rc) return rc; }
		SkPacked pkd; pkd.bytes = (const uint8_t *)dev_twobit; pkd.off = tboff; pkd.mk_off = (const uint64_t *)dev_markup_offsets; pkd.mk_pos = (const uint32_t *)dev_markup_pos; pkd.mk_char = (const uint8_t *)dev_markup_char;
		hints.packed = &pkd;
		return add_reads_dev_call(h, nullptr, nullptr, h->tb_rel.get<uint64_t>(), n_reads, total_bases, first_global_read_idx, dev_discarded, hints);
	}
	{ int rc = twobit_unpack(h, (const uint8_t *)dev_twobit, tboff, (const uint64_t *)dev_offsets, (const uint64_t *)dev_markup_offsets, (const uint32_t *)dev_markup_pos,
	                         (const uint8_t *)dev_markup_char, n_reads, h->tb_bases.get<uint8_t>(), h->tb_rel.get<uint64_t>()); if (rc) return rc; }
	const void *q = dev_quals;
	if (!dev_quals && uniform_quality) {
		if (h->tb_quals.cap() < total_bases + 64) {
			if (h->tb_quals) HIPCHK(h, hipStreamSynchronize(h->stream));
			HIPCHK(h, h->tb_quals.alloc(total_bases + 64)); h->tb_quals_filled = 0; h->tb_quals_char = -1;
		}
		if (h->tb_quals_char != uniform_quality || h->tb_quals_filled < total_bases) {      /* (a buffer the last call filled with the same character stands) */
			HIPCHK(h, hipMemsetAsync(h->tb_quals.get(), uniform_quality, h->tb_quals.cap(), h->stream));
			h->tb_quals_char = uniform_quality; h->tb_quals_filled = h->tb_quals.cap();
		}
		q = h->tb_quals.get<uint8_t>();
	}
	/* (dev_quals[0] is the quality of the call's first base: the unpacked batch and its offsets start there too) */
	return add_reads_dev_call(h, h->tb_bases.get<uint8_t>(), q, h->tb_rel.get<uint64_t>(), n_reads, total_bases, first_global_read_idx, dev_discarded, hints);
}
int kmr_add_reads_twobit_dev(kmr_handle *h, const void *dev_twobit, const void *dev_twobit_offsets, const void *dev_offsets, const void *dev_markup_offsets, const void *dev_markup_pos, const void *dev_markup_char,
                             const void *dev_quals, int uniform_quality, uint64_t n_reads, uint64_t total_bases, uint64_t first_global_read_idx, const void *dev_discarded) {
	if (!h) return KMR_ERR_INVALID_ARG;
	return add_reads_twobit_dev_call(h, dev_twobit, dev_twobit_offsets, dev_offsets, dev_markup_offsets, dev_markup_pos, dev_markup_char, dev_quals, uniform_quality, n_reads, total_bases, first_global_read_idx, dev_discarded, 0);
}

int kmr_add_reads_twobit(kmr_handle *h, const uint8_t *twobit, const uint64_t *twobit_offsets, const uint64_t *offsets,
                         const uint64_t *markup_offsets, const uint32_t *markup_pos, const char *markup_char,
                         const char *quals, int uniform_quality, uint64_t n_reads, uint64_t first_global_read_idx, const uint8_t *discarded) {
	if (!h) return KMR_ERR_INVALID_ARG;
	if (h->finalized) return fail(h, KMR_ERR_STATE, "kmr_add_reads after kmr_finalize");
	if (n_reads == 0) return KMR_OK;
	if (!twobit || !twobit_offsets || !offsets) return fail(h, KMR_ERR_INVALID_ARG, "null buffer");
	hipSetDevice(h->device);
	void *dtb = nullptr, *dto = nullptr, *doff = nullptr, *dmo = nullptr, *dmp = nullptr, *dmc = nullptr, *dq = nullptr, *dd = nullptr;
	/* (the offset arrays go over as they are: the unpack kernel counts base offsets from the piece's first one itself, and the packed
	 * bytes / markups are addressed through pointers moved back by the piece's first offset -- no pass over the reads on the host) */
	auto stage = [&](int set, uint64_t r0, uint64_t r1) -> int {
		const uint64_t m = r1 - r0, total = offsets[r1] - offsets[r0], tbytes = twobit_offsets[r1] - twobit_offsets[r0];
		const uint64_t nm = markup_offsets ? markup_offsets[r1] - markup_offsets[r0] : 0;
		dmo = dmp = dmc = dq = dd = nullptr;
		TBCHK(tb_stage_copy(h, set, 0, twobit + twobit_offsets[r0], tbytes, &dtb)); TBCHK(tb_stage_copy(h, set, 1, twobit_offsets + r0, 8 * (m + 1), &dto)); TBCHK(tb_stage_copy(h, set, 2, offsets + r0, 8 * (m + 1), &doff));
		dtb = (uint8_t *)dtb - twobit_offsets[r0];
		if (nm) {
			TBCHK(tb_stage_copy(h, set, 3, markup_offsets + r0, 8 * (m + 1), &dmo)); TBCHK(tb_stage_copy(h, set, 4, markup_pos + markup_offsets[r0], 4 * nm, &dmp)); TBCHK(tb_stage_copy(h, set, 5, markup_char + markup_offsets[r0], nm, &dmc));
			dmp = (uint32_t *)dmp - markup_offsets[r0]; dmc = (uint8_t *)dmc - markup_offsets[r0];
		}
		if (quals) TBCHK(tb_stage_copy(h, set, 6, quals + offsets[r0], total, &dq));
		if (discarded) TBCHK(tb_stage_copy(h, set, 7, discarded + r0, m, &dd));
		return KMR_OK;
	};
	auto feed = [&](uint64_t r0, uint64_t r1, uint64_t call_bases) {
		return add_reads_twobit_dev_call(h, dtb, dto, doff, dmo, dmp, dmc, dq, quals ? 0 : uniform_quality, r1 - r0, offsets[r1] - offsets[r0], first_global_read_idx + r0, dd, call_bases);
	};
	return tb_feed_pieces(h, offsets, n_reads, stage, feed);
}

int kmr_finalize(kmr_handle *h, uint32_t min_depth) {
	if (!h) return KMR_ERR_INVALID_ARG;
	if (h->finalized) return fail(h, KMR_ERR_STATE, "already finalized");
	hipSetDevice(h->device);
	{ int src_ = sync_state(h); if (src_) return src_; }
	h->subtract = nullptr;                             /* optimize(): subtractingReference.reset() */
	if (h->superkmer_mode) return finalize_superkmer(h, min_depth);
	if (h->partition_mode) return finalize_partition(h, min_depth);
	return with_w_ext(h, [&](auto W, auto EXT) { return finalize_t<W(), EXT()>(h, min_depth); });
}

int kmr_get_stats(kmr_handle *h, kmr_stats *out) {
	if (!h || !out) return KMR_ERR_INVALID_ARG;
	hipSetDevice(h->device);
	if (!h->finalized) { int rc = sync_state(h); if (rc) return rc; h->stats.unique_kmers = h->partition_mode ? 0 : h->occupied; }
	h->stats.reads = h->reads;
	*out = h->stats;
	return KMR_OK;
}

int kmr_lookup(kmr_handle *h, const uint8_t *packed, uint64_t n, uint32_t *counts) {
	if (!h || (n && (!packed || !counts))) return KMR_ERR_INVALID_ARG;
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_lookup before kmr_finalize");
	if (n == 0) return KMR_OK;
	hipSetDevice(h->device);
	return with_w(h, [&](auto W) { return lookup_t<W()>(h, packed, n, counts); });
}

/* kmr_lookup_reads and kmr_lookup_reads_weighted: one output element (u32 count or f64 weight) per k-mer position */
static int lookup_reads_host(kmr_handle *h, const char *bases, const uint64_t *offsets, uint64_t n_reads, void *out, const uint64_t *out_offsets, bool weighted) {
	hipSetDevice(h->device);
	DevBuf sb, so;
	int rc = stage_reads(h, bases, offsets, n_reads, sb, so); if (rc) return rc;
	/* size of the output = last offset + k-mers of the last read */
	uint64_t outN = 0;
	for (uint64_t r = 0; r < n_reads; r++) { uint64_t L = offsets[r + 1] - offsets[r]; uint64_t nk = L >= h->k ? L - h->k + 1 : 0; outN = std::max(outN, out_offsets[r] + nk); }
	const uint64_t eb = weighted ? 8 : 4;
	DevBuf doutb, doffb;
	HIPCHK(h, doutb.alloc(std::max<uint64_t>(8, eb * outN))); HIPCHK(h, doffb.alloc(8 * n_reads));
	void *dout = doutb.get(); uint64_t *doff = doffb.get<uint64_t>();
	HIPCHK(h, hipMemsetAsync(dout, 0, eb * outN, h->stream));
	HIPCHK(h, hipMemcpyAsync(doff, out_offsets, 8 * n_reads, hipMemcpyHostToDevice, h->stream));
	ReadsView rv = reads_view(sb.get(), nullptr, so.get(), n_reads);
	rc = prepare_units(h, rv); if (rc) return rc;
	rc = with_w(h, [&](auto W) { return weighted ? lookup_reads_weighted_t<W()>(h, rv, (double *)dout, doff) : lookup_reads_t<W()>(h, rv, (uint32_t *)dout, doff); });
	if (!rc) { HIPCHK(h, hipMemcpyAsync(out, dout, eb * outN, hipMemcpyDeviceToHost, h->stream)); rc = sync_state(h); }
	else hipStreamSynchronize(h->stream);
	return rc;
}
int kmr_lookup_reads(kmr_handle *h, const char *bases, const uint64_t *offsets, uint64_t n_reads, uint32_t *counts_out, const uint64_t *out_offsets) {
	if (!h || !bases || !offsets || !counts_out || !out_offsets) return KMR_ERR_INVALID_ARG;
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_lookup_reads before kmr_finalize");
	if (n_reads == 0) return KMR_OK;
	return lookup_reads_host(h, bases, offsets, n_reads, counts_out, out_offsets, false);
}

int kmr_lookup_weighted(kmr_handle *h, const uint8_t *packed, uint64_t n, double *weights) {
	if (!h || (n && (!packed || !weights))) return KMR_ERR_INVALID_ARG;
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_lookup_weighted before kmr_finalize");
	if (n == 0) return KMR_OK;
	hipSetDevice(h->device);
	return with_w(h, [&](auto W) { return lookup_t<W()>(h, packed, n, nullptr, weights); });
}

int kmr_lookup_reads_weighted(kmr_handle *h, const char *bases, const uint64_t *offsets, uint64_t n_reads, double *weights_out, const uint64_t *out_offsets) {
	if (!h || !bases || !offsets || !weights_out || !out_offsets) return KMR_ERR_INVALID_ARG;
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_lookup_reads_weighted before kmr_finalize");
	if (n_reads == 0) return KMR_OK;
	return lookup_reads_host(h, bases, offsets, n_reads, weights_out, out_offsets, true);
}

}  // extern "C"
/* ---- lookups as a streaming pass (kmr_superkmer.hpp, "lookups as a streaming pass"): position_counts[offsets[r] + i] = weak-map
 * count of k-mer i of read r, zero where the k-mer is absent or holds an N.  The handle's list pool and list state are reused
 * (after kmr_finalize the build's lists are dead). */
bool stream_lookups_possible(kmr_handle *h) {
	return h->dPk && !h->tune.no_stream_lookups && h->weak.present && h->weak.n > 0 && h->cfg.size_tracker == 0 && !h->sk_exchange;
}
template <int W> int sk_index_t(kmr_handle *h) {
	if (h->ix_gen == h->map_gen && h->ix_start) return 0;
	const uint64_t nl = sk_list_count(h->sk_bits), n = h->weak.n;
	const uint32_t vw = value_words(h);
	if (h->ix_lists != nl) { h->ix_lists = 0; HIPCHK(h, h->ix_start.alloc(8 * (nl + 1))); h->ix_lists = nl; }
	if (h->ix_counts.cap() < 4 * n) {      /* (ix_counts is allocated last) */
		h->ix_keys.reset(); h->ix_counts.reset();
		HIPCHK(h, h->ix_keys.alloc(8ull * W * n)); HIPCHK(h, h->ix_counts.alloc(4 * n));
	}
	uint32_t *elist = nullptr, *hist = nullptr;
	int rc = arena_get(h, &elist, n); if (rc) return rc;
	rc = arena_get(h, &hist, nl); if (rc) return rc;
	HIPCHK(h, hipMemsetAsync(hist, 0, 4 * nl, h->stream));
	LAUNCH(h, sk_index_hist_kernel<W>, dim3(grid_for(n)), dim3(256), 0, (const uint64_t *)h->weak.keys.get<uint64_t>(), n, h->sk_m, h->sk_off, h->sk_win, h->sk_bits, elist, hist);
	rc = exclusive_scan(h, hist, nl, h->ix_start.get<uint64_t>()); if (rc) return rc;
	HIPCHK(h, hipMemsetAsync(hist, 0, 4 * nl, h->stream));
	LAUNCH(h, sk_index_scatter_kernel<W>, dim3(grid_for(n)), dim3(256), 0, (const uint64_t *)h->weak.keys.get<uint64_t>(), (const uint32_t *)h->weak.vals.get<uint32_t>(), vw, n, elist, h->ix_start.get<uint64_t>(), hist, h->ix_keys.get<uint64_t>(), h->ix_counts.get<uint32_t>());
	h->ix_gen = h->map_gen;
	return 0;
}
template <int W> int lookup_stream_t(kmr_handle *h, const ReadsView &rvAll, uint64_t total_bases, uint32_t *position_counts, uint64_t out_n) {
	int rc = arena_reset(h); if (rc) return rc;
	if (!h->sk_state) {      /* a handle that was not built on the lists (loaded image, other build mode): lists sized for this batch */
		uint32_t bits = 6; while (bits < 24 && (total_bases >> bits) > h->tune.target_list / 2 + 200) bits++;
		h->sk_bits = bits;
		HIPCHK(h, h->sk_state.alloc(8ull << bits));
	}
	rc = h->scratch_stats.reserve(h, "scratch_stats", sizeof(DevStats)); if (rc) return rc;
	rc = sk_index_t<W>(h); if (rc) return rc;
	const uint64_t nl = sk_list_count(h->sk_bits);
	LAUNCH(h, sk_state_init_kernel, dim3(grid_for(nl)), dim3(256), 0, h->sk_state.get<unsigned long long>(), nl);
	if (h->l1.head) HIPCHK(h, hipMemsetAsync(h->l1.head.get<unsigned int>(), 0, 4, h->stream));
	h->l1.used_ub = 0;
	ReadsView rv = rvAll;
	rc = prepare_units(h, rv); if (rc) return rc;
	rc = pool_reserve(h, h->l1, total_bases / SK_CHUNK_G + nl + (uint64_t)num_cus(h) * SK_EXTRACT_WAVES_PER_CU * 130 + 64, true); if (rc) return rc;
	/* every k-mer without an N is asked for: no qualities (weight 1, or 0 with an N), no filters, nothing added to the handle's counters */
	DevParams dp = dev_params(h);
	dp.min_weight = 0.5f; dp.subsample = 1; dp.world = 1; dp.num_parts = 1; dp.sub_wnb = 0; dp.sub_snb = 0; dp.stats = h->scratch_stats.get<DevStats>();
	SkParams sp = sk_params(h); sp.keep_all_owners = 1; sp.track = nullptr;
	rc = with_win<W>(h->sk_win, [&](auto WIN) { return (!rv.quals && !h->tune.no_lean_extract) ? launch_sk_extract_lean<W, WIN()>(h, rv, sp, dp, 1.0f) : launch_sk_extract<W, WIN(), false>(h, rv, sp, dp); });
	if (rc) return rc;
	LAUNCH(h, sk_close_kernel, dim3(grid_for(nl)), dim3(256), 0, h->sk_state.get<unsigned long long>(), nl, h->l1.chunk_count.get<uint32_t>(), h->l1.cap);
	uint64_t *ls = nullptr, *lc = nullptr; uint32_t nch = 0;
	rc = build_csr(h, h->l1, nl, 0, &ls, &lc, &nch); if (rc) return rc;
	rc = zero_work_counter(h); if (rc) return rc;
	const int grid = (int)std::min<uint64_t>((uint64_t)num_cus(h) * 4, (nl + SK_LBATCH - 1) / SK_LBATCH);
	auto kern = sk_lookup_kernel<W>;
	const size_t smem = sk_lookup_smem_bytes<W>();
	HIPCHK(h, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
	/* long lists in pieces (as in the count pass; here the pieces need no merge) */
	const uint64_t LONG_CHUNKS = h->tune.long_list_chunks ? h->tune.long_list_chunks : 1024, PIECE = std::max<uint64_t>(1, LONG_CHUNKS / 2);
	uint64_t n_items = 0; uint64_t *ic0 = nullptr, *ic1 = nullptr; uint32_t *il = nullptr;
	if (nch > LONG_CHUNKS) {
		const uint64_t cap = (uint64_t)nch / PIECE + 2 * 1024 + 16;
		unsigned long long *dn = nullptr;
		rc = arena_get(h, &ic0, cap); if (rc) return rc; rc = arena_get(h, &ic1, cap); if (rc) return rc; rc = arena_get(h, &il, cap); if (rc) return rc; rc = arena_get(h, &dn, 1); if (rc) return rc;
		HIPCHK(h, hipMemsetAsync(dn, 0, 8, h->stream));
		LAUNCH(h, sk_long_items_kernel, dim3(grid_for(nl)), dim3(256), 0, ls, nl, LONG_CHUNKS, PIECE, ic0, ic1, cap, dn, il);
		unsigned long long hn = 0;
		HIPCHK(h, fetch(h, &hn, dn));
		if (hn > cap) return fail(h, KMR_ERR_CAPACITY, "long-list work items (internal sizing error)");
		n_items = hn;
	}
	LAUNCH(h, kern, dim3(grid), dim3(COUNT_THREADS), smem, pool_view(h, h->l1), ls, lc, nl, h->k, h->ix_start.get<uint64_t>(), h->ix_keys.get<uint64_t>(), h->ix_counts.get<uint32_t>(), position_counts, out_n, h->work_counter.get<unsigned int>(),
	       (const uint64_t *)nullptr, (const uint64_t *)nullptr, (const uint32_t *)nullptr, (uint64_t)0, n_items ? LONG_CHUNKS : (uint64_t)0);
	if (n_items) {
		rc = zero_work_counter(h); if (rc) return rc;
		LAUNCH(h, kern, dim3((unsigned)std::min<uint64_t>((uint64_t)num_cus(h) * 4, n_items)), dim3(COUNT_THREADS), smem, pool_view(h, h->l1), ls, lc, nl, h->k, h->ix_start.get<uint64_t>(), h->ix_keys.get<uint64_t>(), h->ix_counts.get<uint32_t>(),
		       position_counts, out_n, h->work_counter.get<unsigned int>(), (const uint64_t *)ic0, (const uint64_t *)ic1, (const uint32_t *)il, n_items, (uint64_t)0);
	}
	return 0;
}
int lookup_stream(kmr_handle *h, const ReadsView &rv, uint64_t total_bases, uint32_t *position_counts, uint64_t out_n) {
	return with_w(h, [&](auto W) { return lookup_stream_t<W()>(h, rv, total_bases, position_counts, out_n); });
}

namespace kmr_host {
/* The scoring of a batch whose counts are at hand, queued on the handle's stream: score_reads_kernel and, with
 * kmr_set_bimodal_sigmas >= 0 only, bimodal_trim_kernel behind it.  *words: that pass's word per read (in bimodal_buf), null
 * while the option is off -- then nothing but the first kernel is launched and nothing is allocated. */
static int launch_scoring(kmr_handle *h, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, const uint32_t *counts, const uint64_t *count_off,
                          double minimum_kmer_score, int scoring_type, uint32_t *dto, uint32_t *dtl, float *dsc, uint8_t *dwt, const uint64_t **words) {
	*words = nullptr;
	h->bimodal_n = n_reads; h->bimodal_on = false;
	LAUNCH(h, score_reads_kernel, dim3((unsigned)std::min<uint64_t>(((n_reads + 63) / 64 + SC_WAVES - 1) / SC_WAVES, 1u << 16)), dim3(SC_WAVES * 64), 0, bases, offsets, n_reads, h->k, counts, count_off,
	       (float)minimum_kmer_score, scoring_type, dto, dtl, dsc, dwt);
	if (!(h->bimodal_sigmas >= 0.0)) return 0;
	int rc = h->bimodal_buf.reserve(h, "bimodal_buf", 8 * n_reads, 8 * n_reads + n_reads); if (rc) return rc;
	uint64_t *w = h->bimodal_buf.get<uint64_t>();
	const uint32_t window = h->tune.bimodal_window < 0 ? (uint32_t)BM_CAP : (uint32_t)h->tune.bimodal_window;
	LAUNCH(h, bimodal_trim_kernel, dim3((unsigned)std::min<uint64_t>((n_reads + BM_WAVES - 1) / BM_WAVES, 1u << 16)), dim3(BM_WAVES * 64), 0, n_reads, h->k, counts, count_off,
	       h->bimodal_sigmas, scoring_type, window, dto, dtl, dsc, dwt, w);
	h->bimodal_on = true; *words = w;
	return 0;
}

/* ReadSelector::scoreAndTrimReads (src/ReadSelector.h:1182-1207) on the weak map; s_b / s_o: device bases and offsets,
 * offsets: the same offsets on the host */
int score_reads_core(kmr_handle *h, const uint8_t *s_b, const uint64_t *s_o, uint64_t n_reads, double minimum_kmer_score, int scoring_type,
                     uint32_t *trim_offset, uint32_t *trim_length, float *score, uint8_t *was_trimmed, ScoreDev *keep) {
	int rc = 0;
	ReadsView rv = reads_view(s_b, nullptr, s_o, n_reads);
	/* per-read k-mer counts and their exclusive scan on the device (no host pass over the reads); one grow-only block for
	 * every temporary (freeing the ~GB count array costs more than the scoring) */
	auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
	const size_t fixed = al(4 * (n_reads + 1)) + al(8 * (n_reads + 1)) + 3 * al(4 * n_reads) + al(n_reads);
	rc = h->score_buf.reserve(h, "score_buf", fixed, fixed + fixed / 4); if (rc) return rc;
	uint8_t *p = h->score_buf.get<uint8_t>();
	uint32_t *dkc = (uint32_t *)p; p += al(4 * (n_reads + 1));
	uint64_t *dcoff = (uint64_t *)p;
	/* counts per k-mer: as a streaming pass over minimizer lists (indexed by the k-mer's base position: the reads' own offsets are the
	 * count offsets), or -- where the handle has no list geometry, or on request -- by probing the lookup table k-mer by k-mer */
	bool stream = stream_lookups_possible(h);
	h->last_score_path = stream ? 1 : 2;
	uint64_t outN = 0, first_off = 0;
	if (stream) {
		HIPCHK(h, hipMemcpy(&outN, s_o + n_reads, 8, hipMemcpyDeviceToHost)); HIPCHK(h, hipMemcpy(&first_off, s_o, 8, hipMemcpyDeviceToHost));
		/* the streaming pass answers zero for a k-mer that holds any markup; that is what the reference scores only behind an
		 * N, X or '.', so a batch with another markup (an IUPAC code, a lower-case n) is probed k-mer by k-mer: the whole
		 * batch, for one such base.  Every streaming call pays one pass over its bases and a host wait for the answer. */
		if (outN > first_off) {
			uint32_t other = 0;
			HIPCHK(h, hipMemsetAsync(dkc, 0, 4, h->stream));
			LAUNCH(h, other_markup_kernel, dim3(grid_for((outN - first_off) / 16 + 2)), dim3(256), 0, s_b, first_off, outN, dkc);
			HIPCHK(h, fetch(h, &other, dkc));
			if (other) { stream = false; h->last_score_path = 3; }
		}
	}
	if (!stream) {
		LAUNCH(h, kmer_capacity_kernel, dim3(grid_for(n_reads)), dim3(256), 0, rv, h->k, dkc);
		rc = exclusive_scan(h, dkc, n_reads, dcoff); if (rc) return rc;
		HIPCHK(h, hipMemcpy(&outN, dcoff + n_reads, 8, hipMemcpyDeviceToHost));
	}
	const size_t need = fixed + al(std::max<uint64_t>(8, 4 * outN));
	if (h->score_buf.cap() < need) {         /* grow, keeping the scan */
		DevBuf nbuf; HIPCHK(h, nbuf.alloc(need + need / 8));
		HIPCHK(h, hipMemcpy(nbuf.get(), h->score_buf.get(), al(4 * (n_reads + 1)) + al(8 * (n_reads + 1)), hipMemcpyDeviceToDevice));
		HIPCHK(h, hipDeviceSynchronize());
		h->score_buf = std::move(nbuf);
	}
	p = h->score_buf.get<uint8_t>() + al(4 * (n_reads + 1));
	dcoff = (uint64_t *)p; p += al(8 * (n_reads + 1));
	uint32_t *dto = (uint32_t *)p; p += al(4 * n_reads);
	uint32_t *dtl = (uint32_t *)p; p += al(4 * n_reads);
	float *dsc = (float *)p; p += al(4 * n_reads);
	uint8_t *dwt = p; p += al(n_reads);
	uint32_t *dcounts = (uint32_t *)p;
	HIPCHK(h, hipMemsetAsync(dcounts, 0, 4 * outN, h->stream));
	if (stream) {
		rc = lookup_stream(h, rv, outN - first_off, dcounts, outN);
		dcoff = (uint64_t *)s_o;
	} else {
		{ int urc = prepare_units(h, rv); if (urc) return urc; }
		rc = with_w(h, [&](auto W) { return lookup_reads_t<W()>(h, rv, dcounts, dcoff, true); });
	}
	if (!rc) {
		const uint64_t *dwords;
		rc = launch_scoring(h, s_b, s_o, n_reads, dcounts, dcoff, minimum_kmer_score, scoring_type, dto, dtl, dsc, dwt, &dwords); if (rc) return rc;
		if (keep) { keep->trim_offset = dto; keep->trim_length = dtl; keep->score = dsc; keep->was_trimmed = dwt; keep->bimodal = dwords; }      /* the results stay on the device */
		else {
			HIPCHK(h, hipMemcpyAsync(trim_offset, dto, 4 * n_reads, hipMemcpyDeviceToHost, h->stream)); HIPCHK(h, hipMemcpyAsync(trim_length, dtl, 4 * n_reads, hipMemcpyDeviceToHost, h->stream));
			HIPCHK(h, hipMemcpyAsync(score, dsc, 4 * n_reads, hipMemcpyDeviceToHost, h->stream)); HIPCHK(h, hipMemcpyAsync(was_trimmed, dwt, n_reads, hipMemcpyDeviceToHost, h->stream));
		}
		rc = sync_state(h);
	} else hipStreamSynchronize(h->stream);
	return rc;
}
}  // namespace kmr_host

extern "C" {
int kmr_score_reads(kmr_handle *h, const char *bases, const uint64_t *offsets, uint64_t n_reads, double minimum_kmer_score, int scoring_type,
                    uint32_t *trim_offset, uint32_t *trim_length, float *score, uint8_t *was_trimmed) {
	if (!h || !bases || !offsets || !trim_offset || !trim_length || !score || !was_trimmed) return KMR_ERR_INVALID_ARG;
	if (scoring_type < 0 || scoring_type > 4) return fail(h, KMR_ERR_INVALID_ARG, "bad scoring_type");
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_score_reads before kmr_finalize");
	if (n_reads == 0) return KMR_OK;
	hipSetDevice(h->device);
	DevBuf sb, so;
	int rc = stage_reads(h, bases, offsets, n_reads, sb, so); if (rc) return rc;
	return score_reads_core(h, sb.get<uint8_t>(), so.get<uint64_t>(), n_reads, minimum_kmer_score, scoring_type, trim_offset, trim_length, score, was_trimmed);
}
/* the same on a device-resident read batch (kmr_ingest_fastq): FASTQ text -> reads -> spectrum -> trim/score without the
 * reads ever being staged by the host */
int kmr_score_read_batch(kmr_handle *h, const kmr_reads *r, double minimum_kmer_score, int scoring_type,
                         uint32_t *trim_offset, uint32_t *trim_length, float *score, uint8_t *was_trimmed) {
	if (!h || !r || !trim_offset || !trim_length || !score || !was_trimmed) return KMR_ERR_INVALID_ARG;
	if (scoring_type < 0 || scoring_type > 4) return fail(h, KMR_ERR_INVALID_ARG, "bad scoring_type");
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_score_read_batch before kmr_finalize");
	if (r->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "read batch lives on another device");
	if (r->n == 0) return KMR_OK;
	hipSetDevice(h->device);
	return score_reads_core(h, r->bases.get<uint8_t>(), r->offsets.get<uint64_t>(), r->n, minimum_kmer_score, scoring_type, trim_offset, trim_length, score, was_trimmed);
}

/* --bimodal-sigmas of the handle's scoring calls (ReadSelector::_bimodalSigmas; negative = off, the default) */
int kmr_set_bimodal_sigmas(kmr_handle *h, double sigmas) {
	if (!h) return KMR_ERR_INVALID_ARG;
	if (sigmas != sigmas) return fail(h, KMR_ERR_INVALID_ARG, "kmr_set_bimodal_sigmas: NaN");
	h->bimodal_sigmas = sigmas;
	return KMR_OK;
}
int kmr_bimodal_copy(kmr_handle *h, uint64_t *words, uint64_t n_reads) {
	if (!h || (n_reads && !words)) return KMR_ERR_INVALID_ARG;
	if (h->bimodal_n == ~0ull) return fail(h, KMR_ERR_STATE, "kmr_bimodal_copy before any scoring call");
	if (n_reads != h->bimodal_n) return fail(h, KMR_ERR_INVALID_ARG, "kmr_bimodal_copy: the last scoring call held " + std::to_string(h->bimodal_n) + " reads, not " + std::to_string(n_reads));
	if (!n_reads) return KMR_OK;
	if (!h->bimodal_on) { memset(words, 0, 8 * n_reads); return KMR_OK; }
	hipSetDevice(h->device);
	HIPCHK(h, hipMemcpyAsync(words, h->bimodal_buf.get(), 8 * n_reads, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, hipStreamSynchronize(h->stream));
	return KMR_OK;
}

static DevMap *map_of(kmr_handle *h, int which) {
	if (which == KMR_MAP_WEAK) return &h->weak;
	if (which == KMR_MAP_SINGLETON) return &h->sing;
	return nullptr;
}

int kmr_image_size(kmr_handle *h, int which, uint64_t *bytes) {
	if (!h || !bytes) return KMR_ERR_INVALID_ARG;
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_image_size before kmr_finalize");
	DevMap *m = map_of(h, which);
	if (!m) return fail(h, KMR_ERR_UNSUPPORTED, "solid map is not built on this path");
	const uint32_t vbytes = which == KMR_MAP_WEAK ? (h->ext ? 60 : 12) : (h->ext ? 5 : 1);
	const uint64_t n = m->present ? m->n : 0;
	*bytes = 8 * (2 + m->nb) + 4 * m->nb + n * (h->kb + vbytes);
	return KMR_OK;
}

int kmr_write_image(kmr_handle *h, int which, void *dst, uint64_t capacity) {
	if (!h || !dst) return KMR_ERR_INVALID_ARG;
	uint64_t need; int rc = kmr_image_size(h, which, &need); if (rc) return rc;
	if (capacity < need) return fail(h, KMR_ERR_CAPACITY, "image buffer too small");
	hipSetDevice(h->device);
	DevMap *m = map_of(h, which);
	if (!m->present) {   /* a cleared singleton map, or the weak map of a handle that only loaded a singleton image: numBuckets empty buckets */
		uint8_t *p = (uint8_t *)dst; uint64_t nb = m->nb, mask = nb - 1; memcpy(p, &nb, 8); memcpy(p + 8, &mask, 8);
		for (uint64_t b = 0; b < nb; b++) { uint64_t off = 8 * (2 + nb) + 4 * b; memcpy(p + 16 + 8 * b, &off, 8); uint32_t z = 0; memcpy(p + off, &z, 4); }
		return KMR_OK;
	}
	rc = build_image(h, *m, which == KMR_MAP_WEAK); if (rc) return rc;
	HIPCHK(h, hipMemcpy(dst, m->image.get(), need, hipMemcpyDeviceToHost));
	return KMR_OK;
}

int kmr_load_image(kmr_handle *h, int which, const void *src, uint64_t len) {
	if (!h || !src) return KMR_ERR_INVALID_ARG;
	if (h->reads != 0) return fail(h, KMR_ERR_STATE, "kmr_load_image needs a fresh handle");
	DevMap *m = map_of(h, which);
	if (!m) return fail(h, KMR_ERR_UNSUPPORTED, "solid map is not built on this path");
	hipSetDevice(h->device);
	const int rc = with_w(h, [&](auto W) { return load_image_t<W()>(h, *m, which == KMR_MAP_WEAK, (const uint8_t *)src, len); });
	if (rc) return rc;
	h->slots.reset(); h->extslots.reset();
	if (which == KMR_MAP_WEAK) { h->nb_weak = m->nb; h->stats.weak_entries = m->n; if (!h->sing.present) { h->has_singletons = false; h->sing.nb = h->nb_sing; } }
	else { h->nb_sing = m->nb; h->stats.singleton_entries = m->n; h->has_singletons = true; if (!h->weak.present) h->weak.nb = h->nb_weak; }
	h->finalized = true; h->map_gen++;
	return KMR_OK;
}

int kmr_count_histogram(kmr_handle *h, uint64_t *counts, double *weights, uint32_t n_bins) {
	if (!h || !counts || n_bins < 2) return KMR_ERR_INVALID_ARG;
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_count_histogram before kmr_finalize");
	hipSetDevice(h->device);
	DevBuf dcb, dwb;
	HIPCHK(h, dcb.alloc(8 * n_bins)); HIPCHK(h, hipMemsetAsync(dcb.get(), 0, 8 * n_bins, h->stream));
	if (weights) { HIPCHK(h, dwb.alloc(8 * n_bins)); HIPCHK(h, hipMemsetAsync(dwb.get(), 0, 8 * n_bins, h->stream)); }
	unsigned long long *dc = dcb.get<unsigned long long>(); double *dw = dwb.get<double>();
	if (h->weak.present && h->weak.n)
		LAUNCH(h, histogram_kernel, dim3(grid_for(h->weak.n)), dim3(256), 0, h->weak.vals.get<uint32_t>(), value_words(h), h->weak.n, n_bins, dc, dw);
	HIPCHK(h, hipMemcpyAsync(counts, dc, 8 * n_bins, hipMemcpyDeviceToHost, h->stream));
	if (weights) HIPCHK(h, hipMemcpyAsync(weights, dw, 8 * n_bins, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, hipStreamSynchronize(h->stream));
	return KMR_OK;
}

/* Order-independent digest of a finalized map (see kmr_synth.hpp): what a full-size build is compared by, and what the ranks or
 * parts of a partitioned build add up to. */
int kmr_map_digest(kmr_handle *h, int which_map, kmr_digest *out) {
	if (!h || !out) return KMR_ERR_INVALID_ARG;
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_map_digest before kmr_finalize");
	if (which_map != KMR_MAP_WEAK && which_map != KMR_MAP_SINGLETON) return fail(h, KMR_ERR_UNSUPPORTED, "no such map");
	static_assert(sizeof(kmr_digest) == sizeof(synth::Digest), "kmr_digest layout");
	hipSetDevice(h->device);
	memset(out, 0, sizeof(*out));
	const DevMap &m = which_map == KMR_MAP_WEAK ? h->weak : h->sing;
	if (which_map == KMR_MAP_SINGLETON && !h->has_singletons) return KMR_OK;
	if (!m.present || !m.n) return KMR_OK;
	DevBuf db; HIPCHK(h, db.alloc(sizeof(synth::Digest)));
	synth::Digest *d = db.get<synth::Digest>();
	HIPCHK(h, hipMemsetAsync(d, 0, sizeof(synth::Digest), h->stream));
	if (which_map == KMR_MAP_WEAK)
		LAUNCH(h, synth::map_digest_kernel, dim3(grid_for(m.n, 256, 4096)), dim3(256), 0, m.keys.get<uint64_t>(), (uint32_t)h->W, m.vals.get<uint32_t>(), value_words(h), (const uint8_t *)nullptr, (const uint32_t *)nullptr, m.n, d);
	else
		LAUNCH(h, synth::map_digest_kernel, dim3(grid_for(m.n, 256, 4096)), dim3(256), 0, m.keys.get<uint64_t>(), (uint32_t)h->W, (const uint32_t *)nullptr, 0u, m.sweight.get<uint8_t>(), h->ext ? m.spkt.get<uint32_t>() : (const uint32_t *)nullptr, m.n, d);
	HIPCHK(h, hipMemcpyAsync(out, d, sizeof(synth::Digest), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, hipStreamSynchronize(h->stream));
	out->entries = m.n;
	return KMR_OK;
}

/* SURVEY.md section 8(d)'s synthetic reads, written into caller-owned device memory on the current device (kmr_synth.hpp holds
 * the definition of the generator): reads first_read .. first_read + n_reads of the job `seed`, read_len bases each. */
int kmr_synth_reads_dev(uint64_t seed, uint64_t first_read, uint64_t n_reads, uint32_t read_len, uint64_t genome_len, uint32_t noisy_quals,
                        void *dev_bases, void *dev_quals, uint64_t *dev_offsets) {
	if (!dev_bases || read_len == 0 || genome_len < read_len) return KMR_ERR_INVALID_ARG;
	if (n_reads == 0 && !dev_offsets) return KMR_OK;
	const uint64_t blocks = (n_reads + 1 + 255) / 256;
	if (blocks > 0x7fffffffull) return KMR_ERR_CAPACITY;
	if (launch_status(nullptr, synth::synth_reads_kernel, dim3((uint32_t)blocks), dim3(256), 0, seed, first_read, n_reads, read_len, genome_len, noisy_quals,
	                  (uint8_t *)dev_bases, (uint8_t *)dev_quals, dev_offsets) != hipSuccess) return KMR_ERR_HIP;
	return hipStreamSynchronize(0) == hipSuccess ? KMR_OK : KMR_ERR_HIP;
}

/* KmerSpectrum::subtractReference (src/KmerSpectrum.h:472-474; apps/FilterReads-P.cpp:117): k-mers that exist in the finalized
 * spectrum `reference` are skipped by every later kmr_add_reads* of h (append(), :1582-1588).  kmr_finalize(h) drops the link,
 * as optimize() does (:463-464); reference == NULL drops it at once.  `reference` must stay alive and unchanged meanwhile. */
int kmr_subtract_reference(kmr_handle *h, kmr_handle *reference) {
	if (!h) return KMR_ERR_INVALID_ARG;
	if (reference) {
		if (reference == h) return fail(h, KMR_ERR_INVALID_ARG, "a spectrum cannot subtract itself");
		if (!reference->finalized) return fail(h, KMR_ERR_STATE, "the subtracting spectrum must be finalized");
		if (reference->k != h->k || reference->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "the subtracting spectrum must have the same k and live on the same device");
		if (h->finalized) return fail(h, KMR_ERR_STATE, "kmr_subtract_reference after kmr_finalize");
	}
	hipSetDevice(h->device);
	int rc = sync_state(h); if (rc) return rc;         /* launches in flight carry the old link */
	h->subtract = reference;
	return KMR_OK;
}
int kmr_subtracted(kmr_handle *h, uint64_t *out) {
	if (!h || !out) return KMR_ERR_INVALID_ARG;
	hipSetDevice(h->device);
	if (!h->finalized) { int rc = sync_state(h); if (rc) return rc; }
	*out = h->subtracted;
	return KMR_OK;
}

/* merge a stored part into the finalized maps (buildKmerSpectrumInParts' restore-and-merge loop, src/KmerSpectrum.h:1871-1884) */
int kmr_merge_image(kmr_handle *h, int which, const void *src, uint64_t len) {
	if (!h || !src) return KMR_ERR_INVALID_ARG;
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_merge_image before kmr_finalize / kmr_load_image");
	DevMap *m = map_of(h, which);
	if (!m) return fail(h, KMR_ERR_UNSUPPORTED, "solid map is not built on this path");
	if (!m->present) return fail(h, KMR_ERR_STATE, "this map is not present in the handle (singletons purged?)");
	hipSetDevice(h->device);
	const bool weakMap = which == KMR_MAP_WEAK;
	const int rc = with_w(h, [&](auto W) { return merge_image_t<W()>(h, *m, weakMap, (const uint8_t *)src, len); });
	h->map_gen++;
	if (rc) return rc;
	if (weakMap) h->stats.weak_entries = m->n; else h->stats.singleton_entries = m->n;
	return KMR_OK;
}

/* KmerSpectrum::Histogram (src/KmerSpectrum.h:909-1057) of the finalized spectrum: Histogram(zoom_max, log_base).set(ks) */
uint32_t kmr_histogram_bins(uint32_t zoom_max) { return (1u << 16) + 1u + zoom_max + 1u; }       /* ctor :948-950 */
int kmr_histogram(kmr_handle *h, uint32_t zoom_max, double log_base, uint64_t *visits, uint64_t *visited_count, double *visited_weight, uint32_t n_bins) {
	if (!h || !visits || !visited_count || !visited_weight) return KMR_ERR_INVALID_ARG;
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_histogram before kmr_finalize");
	if (zoom_max > 65535 || !(log_base > 1.0)) return fail(h, KMR_ERR_INVALID_ARG, "bad zoom_max / log_base");
	const uint32_t nb = kmr_histogram_bins(zoom_max);
	if (n_bins < nb) return fail(h, KMR_ERR_CAPACITY, "histogram arrays need kmr_histogram_bins(zoom_max) entries");
	hipSetDevice(h->device);
	/* getIdx (:936-938) for every 16-bit count, with the host's libm */
	std::vector<uint32_t> lut(65536, 0);
	const double logFactor = log(log_base);
	const unsigned int zoomLogSkip = (unsigned int)(log((double)zoom_max + 1.0) / logFactor - 1.0);
	for (uint32_t c = 1; c < 65536; c++) lut[c] = c <= zoom_max ? c : (unsigned int)(log((double)c) / logFactor - zoomLogSkip + zoom_max);
	DevBuf dlb, dvb, dcb, dwb;
	HIPCHK(h, dlb.alloc(4 * 65536)); HIPCHK(h, dvb.alloc(8ull * nb)); HIPCHK(h, dcb.alloc(8ull * nb)); HIPCHK(h, dwb.alloc(8ull * nb));
	uint32_t *dl = dlb.get<uint32_t>(); unsigned long long *dv = dvb.get<unsigned long long>(), *dc = dcb.get<unsigned long long>(); double *dw = dwb.get<double>();
	HIPCHK(h, hipMemcpyAsync(dl, lut.data(), 4 * 65536, hipMemcpyHostToDevice, h->stream));
	HIPCHK(h, hipMemsetAsync(dv, 0, 8ull * nb, h->stream)); HIPCHK(h, hipMemsetAsync(dc, 0, 8ull * nb, h->stream)); HIPCHK(h, hipMemsetAsync(dw, 0, 8ull * nb, h->stream));
	if (h->weak.present && h->weak.n)
		LAUNCH(h, ref_histogram_kernel, dim3(grid_for(h->weak.n, 256, 2048)), dim3(256), 0, h->weak.vals.get<uint32_t>(), value_words(h), (const uint8_t *)nullptr, h->weak.n, dl, dv, dc, dw);
	if (h->has_singletons && h->sing.present && h->sing.n)
		LAUNCH(h, ref_histogram_kernel, dim3(grid_for(h->sing.n, 256, 2048)), dim3(256), 0, (const uint32_t *)nullptr, 0u, h->sing.sweight.get<uint8_t>(), h->sing.n, dl, dv, dc, dw);
	HIPCHK(h, hipMemcpyAsync(visits, dv, 8ull * nb, hipMemcpyDeviceToHost, h->stream)); HIPCHK(h, hipMemcpyAsync(visited_count, dc, 8ull * nb, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, hipMemcpyAsync(visited_weight, dw, 8ull * nb, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, hipStreamSynchronize(h->stream));
	return KMR_OK;
}

int kmr_add_read_batch(kmr_handle *h, const kmr_reads *r, uint64_t first_global_read_idx) {
	if (!h || !r) return KMR_ERR_INVALID_ARG;
	if (r->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "read batch lives on another device");
	int rc = kmr_add_reads_dev(h, r->bases.get<uint8_t>(), r->quals.get<uint8_t>(), r->offsets.get<uint64_t>(), r->n, r->total, first_global_read_idx, nullptr);
	if (!rc) rc = kmr_sync(h);
	return rc;
}
/* ---- stateless helpers ------------------------------------------------- */
uint64_t kmr_hash(const uint8_t *key, uint32_t len) {
	if (!key || len == 0 || len > 32) return 0;
	Key<4> k; key_from_bytes<4>(k, key, len);
	return key_hash<4>(k, len);
}
uint64_t kmr_hash_of_kind(const uint8_t *key, uint32_t len, uint32_t hash_kind) {
	if (!key || len == 0 || len > 32 || hash_kind > KMR_HASH_LOOKUP8) return 0;
	Key<4> k; key_from_bytes<4>(k, key, len);
	return key_hash<4>(k, len | (hash_kind << 16));
}
uint64_t kmr_bucket_idx(uint64_t hash, uint64_t nb) { return hash & (nb - 1); }
uint32_t kmr_local_thread_id(uint64_t hash, uint64_t nb, uint32_t t) { return (nb > 1 && t > 1) ? (uint32_t)((hash & (nb - 1)) % t) : 0; }
uint32_t kmr_distributed_thread_id(uint64_t hash, uint32_t n) { return distributed_thread_id(hash, n); }

int64_t kmr_compress_sequence(const char *bases, uint64_t len, uint8_t *out, uint32_t *mpos, char *mchar, uint64_t mcap) {
	if (!bases) return KMR_ERR_INVALID_ARG;
	int64_t nm = 0;
	uint64_t offset = 0;
	while (offset < len) {
		uint8_t c = 0;
		for (int i = 6; i >= 0 && offset < len; i -= 2) {
			char b = bases[offset]; uint8_t code;
			switch (b) { case 'A': case 'a': code = 0; break; case 'C': case 'c': code = 1; break; case 'G': case 'g': code = 2; break; case 'T': case 't': code = 3; break;
			case '\0': len = offset; code = 255; break;
			default: if (b == '.') b = 'N'; if ((uint64_t)nm < mcap) { if (mpos) mpos[nm] = (uint32_t)offset; if (mchar) mchar[nm] = b; } nm++; code = 0; }
			if (code == 255) break;
			offset++;
			c |= code << i;
		}
		if (out) *out++ = c;
	}
	return nm;
}

int kmr_least_complement(const uint8_t *packed, uint32_t k, uint8_t *out) {
	if (!packed || !out || k < 1 || k > 128) return KMR_ERR_INVALID_ARG;
	const uint32_t kb = (k + 3) / 4;
	Roller<4> r; r.init(k);
	for (uint32_t p = 0; p < k; p++) r.push((packed[p >> 2] >> (6 - 2 * (p & 3))) & 3);
	const bool least = key_le<4>(r.fwd, r.rc);
	const Key<4> &c = least ? r.fwd : r.rc;
	for (uint32_t j = 0; j < kb; j++) out[j] = key_byte<4>(c, j);
	return least ? 1 : 0;
}

int kmr_extract_by_owner_dev(kmr_handle *h, const void *dev_bases, const void *dev_quals, const void *dev_offsets, uint64_t n_reads,
                             uint64_t total_bases, uint64_t first_global_read_idx, const void *dev_discarded,
                             void *dev_records, uint64_t seg_capacity, void *dev_seg_counts) {
	if (!h || !dev_bases || !dev_offsets || !dev_records || !dev_seg_counts) return KMR_ERR_INVALID_ARG;
	if (h->cfg.world_size > (uint32_t)OWNER_MAX) return fail(h, KMR_ERR_UNSUPPORTED, "owner exchange supports up to 8 ranks per node");
	if (h->superkmer_mode && h->auto_mode && !h->sk_state) h->superkmer_mode = false;      /* auto: the k-mer record exchange runs on the two-level partition */
	if (h->superkmer_mode) return fail(h, KMR_ERR_UNSUPPORTED, "k-mer records by owner are a build_mode 1 / 2 path");
	hipSetDevice(h->device);
	const ReadsView rv = reads_view(dev_bases, dev_quals, dev_offsets, n_reads, dev_discarded, h->stream_base, first_global_read_idx);
	HIPCHK(h, hipMemsetAsync(dev_seg_counts, 0, 8 * h->cfg.world_size, h->stream));
	const int rc = with_w_ext(h, [&](auto W, auto EXT) { return extract_by_owner_t<W(), EXT()>(h, rv, total_bases, dev_records, seg_capacity, dev_seg_counts); });
	h->stream_base += total_bases; h->reads += n_reads;
	return rc;
}

/* ---- f1, distributed form: lookups of k-mers other ranks own (DistributedReadSelector, src/DistributedFunctions.h:809-1045) */
int kmr_lookup_requests_dev(kmr_handle *h, const void *dev_bases, const void *dev_offsets, uint64_t n_reads, uint64_t total_bases,
                            void *dev_keys, void *dev_pos, uint64_t seg_capacity, void *dev_seg_counts) {
	if (!h || !dev_bases || !dev_offsets || !dev_keys || !dev_pos || !dev_seg_counts) return KMR_ERR_INVALID_ARG;
	if (h->cfg.world_size > (uint32_t)OWNER_MAX) return fail(h, KMR_ERR_UNSUPPORTED, "owner exchange supports up to 8 ranks per node");
	if (total_bases >= (1ull << 32)) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_lookup_requests_dev: positions are 32-bit, pass at most 2^32 - 1 bases per call");
	hipSetDevice(h->device);
	const ReadsView rv = reads_view(dev_bases, nullptr, dev_offsets, n_reads);
	HIPCHK(h, hipMemsetAsync(dev_seg_counts, 0, 8 * h->cfg.world_size, h->stream));
	if (n_reads == 0) return KMR_OK;
	return with_w_ext(h, [&](auto W, auto EXT) { return extract_by_owner_t<W(), EXT()>(h, rv, total_bases, dev_keys, seg_capacity, dev_seg_counts, (uint32_t *)dev_pos); });
}
int kmr_lookup_keys_dev(kmr_handle *h, const void *dev_keys, uint64_t n, void *dev_counts) {
	if (!h || (n && (!dev_keys || !dev_counts))) return KMR_ERR_INVALID_ARG;
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_lookup_keys_dev before kmr_finalize");
	if (n == 0) return KMR_OK;
	hipSetDevice(h->device);
	const uint32_t vw = value_words(h);
	return with_w(h, [&](auto W) -> int { LAUNCH(h, lookup_words_kernel<W()>, dim3(grid_for(n)), dim3(256), 0, view_of<W()>(h->weak, vw), lut_of<W()>(h), (const uint64_t *)dev_keys, n, h->hkb, (uint32_t *)dev_counts); return KMR_OK; });
}
int kmr_lookup_keys_weighted_dev(kmr_handle *h, const void *dev_keys, uint64_t n, void *dev_weights) {
	if (!h || (n && (!dev_keys || !dev_weights))) return KMR_ERR_INVALID_ARG;
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_lookup_keys_weighted_dev before kmr_finalize");
	if (n == 0) return KMR_OK;
	hipSetDevice(h->device);
	const uint32_t vw = value_words(h);
	return with_w(h, [&](auto W) -> int { LAUNCH(h, lookup_words_weight_kernel<W()>, dim3(grid_for(n)), dim3(256), 0, view_of<W()>(h->weak, vw), view_of<W()>(h->sing, vw), lut_of<W()>(h),
	                                      (const uint64_t *)dev_keys, n, h->hkb, (double *)dev_weights); return KMR_OK; });
}
int kmr_scatter_counts_dev(kmr_handle *h, const void *dev_counts, const void *dev_pos, uint64_t n, void *dev_position_counts) {
	if (!h || (n && (!dev_counts || !dev_pos || !dev_position_counts))) return KMR_ERR_INVALID_ARG;
	if (n == 0) return KMR_OK;
	hipSetDevice(h->device);
	LAUNCH(h, scatter_counts_kernel, dim3(grid_for(n)), dim3(256), 0, (const uint32_t *)dev_counts, (const uint32_t *)dev_pos, n, (uint32_t *)dev_position_counts);
	return KMR_OK;
}
int kmr_score_counts_dev(kmr_handle *h, const void *dev_bases, const void *dev_offsets, uint64_t n_reads, const void *dev_position_counts,
                         double minimum_kmer_score, int scoring_type, uint32_t *trim_offset, uint32_t *trim_length, float *score, uint8_t *was_trimmed) {
	if (!h || !dev_bases || !dev_offsets || !dev_position_counts || !trim_offset || !trim_length || !score || !was_trimmed) return KMR_ERR_INVALID_ARG;
	if (scoring_type < 0 || scoring_type > 4) return fail(h, KMR_ERR_INVALID_ARG, "bad scoring_type");
	if (n_reads == 0) return KMR_OK;
	hipSetDevice(h->device);
	DevBuf b_dto, b_dtl, b_dsc, b_dwt;
	HIPCHK(h, b_dto.alloc(4 * n_reads)); HIPCHK(h, b_dtl.alloc(4 * n_reads)); HIPCHK(h, b_dsc.alloc(4 * n_reads)); HIPCHK(h, b_dwt.alloc(n_reads));
	uint32_t *dto = b_dto.get<uint32_t>(), *dtl = b_dtl.get<uint32_t>(); float *dsc = b_dsc.get<float>(); uint8_t *dwt = b_dwt.get<uint8_t>();
	/* k-mer i of read r sits at position offsets[r] + i: the offsets are their own count offsets */
	const uint64_t *dwords;
	int rc = launch_scoring(h, (const uint8_t *)dev_bases, (const uint64_t *)dev_offsets, n_reads, (const uint32_t *)dev_position_counts, (const uint64_t *)dev_offsets, minimum_kmer_score, scoring_type, dto, dtl, dsc, dwt, &dwords);
	if (rc) { hipStreamSynchronize(h->stream); return rc; }
	hipError_t e = hipSuccess;
	if (e == hipSuccess) e = hipMemcpyAsync(trim_offset, dto, 4 * n_reads, hipMemcpyDeviceToHost, h->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(trim_length, dtl, 4 * n_reads, hipMemcpyDeviceToHost, h->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(score, dsc, 4 * n_reads, hipMemcpyDeviceToHost, h->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(was_trimmed, dwt, n_reads, hipMemcpyDeviceToHost, h->stream);
	hipStreamSynchronize(h->stream);
	HIPCHK(h, e);
	return KMR_OK;
}

int kmr_insert_records_dev(kmr_handle *h, const void *dev_records, uint64_t n) {
	if (!h || (n && !dev_records)) return KMR_ERR_INVALID_ARG;
	if (h->finalized) return fail(h, KMR_ERR_STATE, "kmr_insert_records_dev after kmr_finalize");
	if (n == 0) return KMR_OK;
	hipSetDevice(h->device);
	if (h->superkmer_mode && h->auto_mode && !h->sk_state) h->superkmer_mode = false;
	if (h->superkmer_mode) return fail(h, KMR_ERR_UNSUPPORTED, "k-mer records are inserted by build_mode 1 / 2");
	if (h->partition_mode) { int prc = insert_records_partition(h, dev_records, n); h->stream_base += n; return prc; }
	int rc = ensure_capacity(h, n); if (rc) return rc;
	TimeSpan t(h, 0);
	rc = with_w_ext(h, [&](auto W, auto EXT) -> int { LAUNCH(h, (insert_records_kernel<W(), EXT()>), dim3(grid_for(n)), dim3(256), 0, table_of<W()>(h), (const uint32_t *)dev_records, n, dev_params(h), h->stream_base); return 0; });
	t.end();
	if (rc) return rc;
	h->stream_base += n;
	return KMR_OK;
}

/* Host-buffer forms of the two halves, for a host whose exchange is MPI_Alltoallv over host memory (the shim's
 * GpuDistributedKmerSpectrum): records of a device-resident batch binned by owner and copied out owner after owner, and records
 * received from the other ranks staged in and inserted. */
int kmr_extract_by_owner_host(kmr_handle *h, const kmr_reads *batch, uint64_t first_global_read_idx, uint64_t *seg_counts, void *records, uint64_t capacity_bytes) {
	if (!h || !batch || !seg_counts) return KMR_ERR_INVALID_ARG;
	if (batch->device != h->device) return fail(h, KMR_ERR_INVALID_ARG, "read batch lives on another device");
	hipSetDevice(h->device);
	const uint32_t world = h->cfg.world_size, rb = KMR_RECORD_BYTES(h->k, h->cfg.value_kind);
	if (!(h->xo_dev && h->xo_batch == (const void *)batch && h->xo_first == first_global_read_idx)) {
		h->xo_dev.reset();
		h->xo_counts.assign(world, 0); h->xo_batch = nullptr;
		DevBuf dcounts;
		HIPCHK(h, dcounts.alloc(8 * world));
		const uint64_t upper = batch->total + 64;          /* k-mers <= bases */
		uint64_t segcap = std::min<uint64_t>(upper, upper / world + upper / (4 * world) + 4096);
		const uint64_t sb = h->stream_base, rd = h->reads;
		unsigned long long bad0 = 0; hipMemcpy(&bad0, &h->dstats.get<DevStats>()->sender_bad, 8, hipMemcpyDeviceToHost);      /* a repeated attempt must not count the dropped k-mers twice */
		for (;;) {
			if (h->xo_dev.alloc((size_t)world * segcap * rb) != hipSuccess) return fail(h, KMR_ERR_OOM, "owner segments");
			h->stream_base = sb; h->reads = rd;             /* a repeated attempt stamps the same ordinals */
			int rc = kmr_extract_by_owner_dev(h, batch->bases.get<uint8_t>(), batch->quals.get<uint8_t>(), batch->offsets.get<uint64_t>(), batch->n, batch->total, first_global_read_idx, nullptr, h->xo_dev.get(), segcap, dcounts.get());
			if (!rc) rc = sync_state(h);
			if (rc == KMR_ERR_CAPACITY && segcap < upper) {      /* a skewed batch: one owner takes more than its share */
				uint32_t e = 0; hipMemcpy(&e, h->derr.get<uint32_t>(), 4, hipMemcpyDeviceToHost); e &= ~(uint32_t)ERR_SEGMENT_OVERFLOW; hipMemcpy(h->derr.get<uint32_t>(), &e, 4, hipMemcpyHostToDevice); hipMemcpy(&h->dstats.get<DevStats>()->sender_bad, &bad0, 8, hipMemcpyHostToDevice);
				h->xo_dev.reset();
				segcap = std::min<uint64_t>(upper, segcap * 2);
				continue;
			}
			if (rc) { h->xo_dev.reset(); return rc; }
			break;
		}
		HIPCHK(h, hipMemcpy(h->xo_counts.data(), dcounts.get(), 8 * world, hipMemcpyDeviceToHost));
		h->xo_segcap = segcap; h->xo_batch = batch; h->xo_first = first_global_read_idx;
	}
	uint64_t total = 0;
	for (uint32_t r = 0; r < world; r++) { seg_counts[r] = h->xo_counts[r]; total += h->xo_counts[r]; }
	if (!records) return KMR_OK;                           /* sizing call: the segments wait on the device */
	if (capacity_bytes < total * rb) return fail(h, KMR_ERR_CAPACITY, "record buffer too small");
	uint8_t *dst = (uint8_t *)records;
	for (uint32_t r = 0; r < world; r++) {
		if (h->xo_counts[r]) HIPCHK(h, hipMemcpy(dst, (const uint8_t *)h->xo_dev.get() + (size_t)r * h->xo_segcap * rb, (size_t)h->xo_counts[r] * rb, hipMemcpyDeviceToHost));
		dst += (size_t)h->xo_counts[r] * rb;
	}
	h->xo_dev.reset(); h->xo_batch = nullptr;
	return KMR_OK;
}
int kmr_insert_records(kmr_handle *h, const void *host_records, uint64_t n) {
	if (!h || (n && !host_records)) return KMR_ERR_INVALID_ARG;
	if (n == 0) return KMR_OK;
	hipSetDevice(h->device);
	const size_t bytes = (size_t)n * KMR_RECORD_BYTES(h->k, h->cfg.value_kind);
	DevBuf d;
	HIPCHK(h, d.alloc(bytes));
	hipError_t e = hipMemcpy(d.get(), host_records, bytes, hipMemcpyHostToDevice);
	int rc = e == hipSuccess ? kmr_insert_records_dev(h, d.get(), n) : KMR_ERR_HIP;
	if (!rc) rc = sync_state(h); else hipStreamSynchronize(h->stream);
	return rc;
}

/* ---- owner exchange of super-k-mer lists (build_mode 3, world_size > 1): see kmr_superkmer.hpp */
static int sk_exchange_ready(kmr_handle *h, const char *who) {
	if (!h->superkmer_mode) return fail(h, KMR_ERR_STATE, std::string(who) + ": the handle does not build super-k-mer lists (build_mode 3)");
	if (h->finalized) return fail(h, KMR_ERR_STATE, std::string(who) + " after kmr_finalize");
	if (h->cfg.world_size > SK_OWNER_MAX) return fail(h, KMR_ERR_UNSUPPORTED, "at most 64 ranks");
	if (!h->sk_exchange) return fail(h, KMR_ERR_STATE, std::string(who) + " without kmr_sk_exchange_begin (the reads of this handle were filtered by getDistributedThreadId)");
	return 0;
}
int kmr_sk_exchange_begin(kmr_handle *h) {
	if (!h) return KMR_ERR_INVALID_ARG;
	if (!h->superkmer_mode) return fail(h, KMR_ERR_STATE, "kmr_sk_exchange_begin: the handle does not build super-k-mer lists (build_mode 3)");
	if (h->cfg.world_size > SK_OWNER_MAX) return fail(h, KMR_ERR_UNSUPPORTED, "at most 64 ranks");
	if (h->sk_state && !h->sk_exchange && h->reads) return fail(h, KMR_ERR_STATE, "kmr_sk_exchange_begin after reads were added");
	h->sk_exchange = true;
	return KMR_OK;
}
static int sk_ensure_state(kmr_handle *h) {      /* a rank without reads still owns lists */
	if (h->sk_state) return 0;
	return add_reads_superkmer(h, reads_view(nullptr, nullptr, nullptr, 0), 0, FeedHints());
}
int kmr_sk_exchange_counts(kmr_handle *h, uint64_t *chunks, uint64_t *granules) {
	if (!h || !chunks || !granules) return KMR_ERR_INVALID_ARG;
	int rc = sk_exchange_ready(h, "kmr_sk_exchange_counts"); if (rc) return rc;
	hipSetDevice(h->device);
	rc = sk_ensure_state(h); if (rc) return rc;
	rc = sync_state(h); if (rc) return rc;
	const uint32_t world = h->cfg.world_size;
	const uint64_t nl = sk_list_count(h->sk_bits);
	unsigned int head = 0;
	HIPCHK(h, hipMemcpy(&head, h->l1.head.get<unsigned int>(), 4, hipMemcpyDeviceToHost));
	if (head > h->l1.cap) head = h->l1.cap;
	DevBuf db; HIPCHK(h, db.alloc(16 * SK_OWNER_MAX));
	unsigned long long *d = db.get<unsigned long long>();
	HIPCHK(h, hipMemsetAsync(d, 0, 16 * SK_OWNER_MAX, h->stream));
	LAUNCH(h, sk_close_kernel, dim3(grid_for(nl)), dim3(256), 0, h->sk_state.get<unsigned long long>(), nl, h->l1.chunk_count.get<uint32_t>(), h->l1.cap);
	if (head) LAUNCH(h, sk_owner_count_kernel, dim3(grid_for(head)), dim3(256), 0, h->l1.chunk_list.get<uint32_t>(), h->l1.chunk_count.get<uint32_t>(), head, world, d, d + SK_OWNER_MAX, h->xr_lo, h->xr_hi);
	std::vector<unsigned long long> hv(2 * SK_OWNER_MAX, 0);
	HIPCHK(h, fetch(h, hv.data(), d, 2 * SK_OWNER_MAX));
	for (uint32_t r = 0; r < world; r++) { chunks[r] = hv[r]; granules[r] = hv[SK_OWNER_MAX + r]; }
	return KMR_OK;
}
int kmr_sk_exchange_pack_dev(kmr_handle *h, void *dev_data, void *dev_meta, const uint64_t *granule_offset, const uint64_t *chunk_offset) {
	if (!h || !dev_data || !dev_meta || !granule_offset || !chunk_offset) return KMR_ERR_INVALID_ARG;
	int rc = sk_exchange_ready(h, "kmr_sk_exchange_pack_dev"); if (rc) return rc;
	hipSetDevice(h->device);
	const uint32_t world = h->cfg.world_size;
	unsigned int head = 0;
	HIPCHK(h, hipMemcpy(&head, h->l1.head.get<unsigned int>(), 4, hipMemcpyDeviceToHost));
	if (head > h->l1.cap) head = h->l1.cap;
	DevBuf db; HIPCHK(h, db.alloc(32 * SK_OWNER_MAX));
	unsigned long long *d = db.get<unsigned long long>();
	std::vector<unsigned long long> hv(4 * SK_OWNER_MAX, 0);
	for (uint32_t r = 0; r < world; r++) { hv[r] = granule_offset[r]; hv[SK_OWNER_MAX + r] = chunk_offset[r]; }
	HIPCHK(h, hipMemcpyAsync(d, hv.data(), 32 * SK_OWNER_MAX, hipMemcpyHostToDevice, h->stream));
	if (head) {
		LAUNCH(h, sk_pack_kernel, dim3(grid_for((uint64_t)head * 64, 256, num_cus(h) * 8)), dim3(256), 0, pool_view(h, h->l1), head, world, h->cfg.rank,
		       d, d + SK_OWNER_MAX, d + 2 * SK_OWNER_MAX, d + 3 * SK_OWNER_MAX, (uint4 *)dev_data, (uint2 *)dev_meta, h->xr_lo, h->xr_hi);
		LAUNCH(h, sk_state_drop_kernel, dim3(grid_for(sk_list_count(h->sk_bits))), dim3(256), 0, h->sk_state.get<unsigned long long>(), sk_list_count(h->sk_bits), world, h->cfg.rank, h->xr_lo, h->xr_hi);
	}
	HIPCHK(h, stream_wait(h));      /* hv and d go out of scope */
	return KMR_OK;
}
/* the part of the list space the next kmr_sk_exchange_counts / kmr_sk_exchange_pack_dev are about ([0, ~0) = all of it) */
int kmr_sk_exchange_range(kmr_handle *h, uint64_t list_lo, uint64_t list_hi) {
	if (!h || list_lo > list_hi) return KMR_ERR_INVALID_ARG;
	h->xr_lo = list_lo; h->xr_hi = list_hi;
	return KMR_OK;
}
int kmr_count_lists_prefix(kmr_handle *h, uint32_t min_depth, uint64_t list_hi) {
	if (!h) return KMR_ERR_INVALID_ARG;
	if (h->finalized) return fail(h, KMR_ERR_STATE, "kmr_count_lists_prefix after kmr_finalize");
	if (!h->superkmer_mode) return KMR_OK;      /* the other build modes have no lists: kmr_finalize counts */
	hipSetDevice(h->device);
	return count_prefix_superkmer(h, min_depth, list_hi);
}
/* One weight for every record of this rank's lists so far?  state = kind << 32 | weight bits, kind 0: no record yet, 1: one weight, 2: several
 * (records with weights of their own).  A sender's state travels with its chunk counts; the owner folds it in with
 * kmr_sk_exchange_peer_uniform and then takes the count pass's one-weight form when all agree, without looking at the records. */
int kmr_sk_exchange_uniform(kmr_handle *h, uint64_t *state) {
	if (!h || !state) return KMR_ERR_INVALID_ARG;
	*state = h->sk_uni_mixed ? (2ull << 32) : (h->sk_uni_w == SK_UNI_NONE ? 0ull : ((1ull << 32) | h->sk_uni_w));
	return KMR_OK;
}
int kmr_sk_exchange_peer_uniform(kmr_handle *h, uint64_t state) {
	if (!h) return KMR_ERR_INVALID_ARG;
	const uint32_t kind = (uint32_t)(state >> 32), w = (uint32_t)state;
	if (kind > 2) return fail(h, KMR_ERR_INVALID_ARG, "bad uniform-weight state");
	h->peers_declare = true;      /* arms the next kmr_sk_exchange_adopt_dev only */
	if (kind == 2) h->peer_uni_mixed = true;
	else if (kind == 1) { if (h->peer_uni_w == SK_UNI_NONE) h->peer_uni_w = w; else if (h->peer_uni_w != w) h->peer_uni_mixed = true; }
	return KMR_OK;
}
int kmr_sk_exchange_adopt_dev(kmr_handle *h, const void *dev_data, const void *dev_meta, uint64_t n_chunks, uint64_t n_granules) {
	if (!h || (n_chunks && (!dev_data || !dev_meta))) return KMR_ERR_INVALID_ARG;
	int rc = sk_exchange_ready(h, "kmr_sk_exchange_adopt_dev"); if (rc) return rc;
	/* the senders' declarations (kmr_sk_exchange_peer_uniform) cover this adopt and no other: one that nobody armed looks at the records */
	const bool declared = h->peers_declare;
	h->peers_declare = false;
	if (n_chunks == 0) return KMR_OK;
	hipSetDevice(h->device);
	rc = sk_ensure_state(h); if (rc) return rc;
	h->ord_foreign = true;      /* records with their senders' ordinals: the build's span is no longer this handle's to know (sk_count_blocks) */
	const int grid = (int)std::min<uint64_t>((n_chunks + SK_ADOPT_WAVES * SK_ADOPT_GROUP - 1) / (SK_ADOPT_WAVES * SK_ADOPT_GROUP), (uint64_t)num_cus(h) * 8);
	/* (a received chunk is appended as one piece: at worst every one of them opens a chunk of its own) */
	rc = pool_reserve(h, h->l1, n_chunks + n_granules / SK_CHUNK_G + (sk_list_count(h->sk_bits) / h->cfg.world_size) + (uint64_t)grid * SK_ADOPT_WAVES * 130 + 64, true); if (rc) return rc;
	/* per-chunk counts and their scan: a grow-only buffer of the handle (a job adopts once per piece and batch) */
	const size_t need = 8 * (n_chunks + 1) + 4 * (n_chunks + 1) + 256;
	rc = h->adopt_buf.reserve(h, "adopt_buf", need, need + need / 4); if (rc) return rc;
	uint64_t *start = (uint64_t *)h->adopt_buf.get<uint8_t>(); uint32_t *cnt = (uint32_t *)(h->adopt_buf.get<uint8_t>() + 8 * (n_chunks + 1));
	/* (from here on a failure is carried to the wait at the end) */
	rc = [&]() -> int { LAUNCH(h, sk_meta_counts_kernel, dim3(grid_for(n_chunks)), dim3(256), 0, (const uint2 *)dev_meta, n_chunks, cnt); return 0; }();
	if (!rc) rc = exclusive_scan(h, cnt, n_chunks, start);
	if (!rc && !h->d_uni && !declared) {
		if (h->d_uni.alloc(8) != hipSuccess) rc = fail(h, KMR_ERR_OOM, "uniform-weight flags");
		else { const uint32_t init[2] = {SK_UNI_NONE, 0u}; if (hipMemcpyAsync(h->d_uni.get<uint32_t>(), init, 8, hipMemcpyHostToDevice, h->stream) != hipSuccess) rc = fail(h, KMR_ERR_HIP, "uniform-weight flags"); else hipStreamSynchronize(h->stream); }
	}
	/* (senders that declare their weights -- kmr_sk_exchange_peer_uniform, what both drivers do -- spare the owner this look at every
	 * received header: 3.5 ms for 4.2 GB at 8 ranks) */
	if (!rc && !declared && launch_status(h->stream, sk_uniform_check_kernel, dim3(grid_for(n_chunks)), dim3(256), 0, (const uint4 *)dev_data, start, cnt, n_chunks, h->d_uni.get<uint32_t>()) != hipSuccess) rc = fail(h, KMR_ERR_HIP, "sk_uniform_check_kernel launch");
	if (!rc && launch_status(h->stream, sk_adopt_kernel, dim3(grid), dim3(SK_ADOPT_WAVES * 64), 0, (const uint4 *)dev_data, (const uint2 *)dev_meta, start, n_chunks, sk_params(h), pool_view(h, h->l1)) != hipSuccess) rc = fail(h, KMR_ERR_HIP, "sk_adopt_kernel launch");
	hipStreamSynchronize(h->stream);
	return rc ? rc : sync_state(h);
}

/* ---- f3: KmerSpectrum::SizeTracker (src/KmerSpectrum.h:812-900) */
int kmr_size_tracker(kmr_handle *h, int force_last, uint64_t *elements, uint64_t capacity, uint64_t *n_elements) {
	if (!h || !n_elements) return KMR_ERR_INVALID_ARG;
	if (!h->cfg.size_tracker) return fail(h, KMR_ERR_STATE, "kmr_size_tracker: kmr_config.size_tracker was not set");
	if (!h->finalized) return fail(h, KMR_ERR_STATE, "kmr_size_tracker before kmr_finalize");
	const uint64_t n = h->trk_elems.size() / 4 + (force_last ? 1 : 0);
	*n_elements = n;
	if (!elements) return KMR_OK;
	if (capacity < n) return fail(h, KMR_ERR_CAPACITY, "kmr_size_tracker: element buffer too small");
	if (!h->trk_elems.empty()) memcpy(elements, h->trk_elems.data(), 8 * h->trk_elems.size());
	if (force_last) {      /* trackSpectrum(true), as the apps call it after the build (apps/FilterReads.cpp:141) */
		const uint64_t sub = h->cfg.kmer_subsample > 1 ? h->cfg.kmer_subsample : 1;
		uint64_t *e = elements + h->trk_elems.size();
		e[0] = h->stats.raw_kmers * sub; e[1] = h->stats.raw_good_kmers * sub; e[2] = h->stats.unique_kmers * sub; e[3] = h->stats.singleton_kmers * sub;
	}
	return KMR_OK;
}

#include "kmr_exchange_rccl.hpp"

int kmr_kernel_time(kmr_handle *h, int which, double *ms, uint64_t *launches) {
	if (!h || which < 0 || which >= KMR_TIME_GROUPS) return KMR_ERR_INVALID_ARG;
	hipSetDevice(h->device);
	int rc = sync_state(h); if (rc) return rc;
	if (ms) *ms = h->ms[which];
	if (launches) *launches = h->launches[which];
	return KMR_OK;
}
int kmr_kernel_time_reset(kmr_handle *h) {
	if (!h) return KMR_ERR_INVALID_ARG;
	int rc = sync_state(h); if (rc) return rc;
	for (int i = 0; i < KMR_TIME_GROUPS; i++) { h->ms[i] = 0; h->launches[i] = 0; }
	return KMR_OK;
}

}  // extern "C"

/* ---- CompareSpectrums (kmr_compare.hpp): the spectrum side of kmr_compare_spectrums / kmr_compare_reads* (kmr_stages.hip) ---- */
namespace {

/* h->cmp_buf: what compare_reads_core keeps between calls (the sorted path's sort: h->cmp_sort) */
enum { CMP_B_ACC = 0, CMP_B_NK, CMP_B_KOFF, CMP_B_STAGE, CMP_B_CNT, CMP_B_LOFF, CMP_B_SRC, CMP_B_RID, CMP_B_PERM, CMP_B_HSCAN, CMP_B_START, CMP_B_COUNT };
static_assert(CMP_B_COUNT == sizeof(HandleMem::cmp_buf) / sizeof(DevBuf), "kmr_host.hpp's cmp_buf holds one block per CMP_B_ index");

/* dev_params for an extraction whose reads are the call's own: nothing is subtracted.  whole: every k-mer of the batch is this
 * call's too, whatever the handle's kmer_subsample, world_size and num_parts */
DevParams own_reads_params(kmr_handle *h, bool whole) {
	DevParams dp = dev_params(h);
	dp.sub_wstart = dp.sub_wkeys = dp.sub_sstart = dp.sub_skeys = nullptr; dp.sub_wvals = nullptr; dp.sub_sweight = nullptr; dp.sub_wnb = dp.sub_snb = 0;
	if (whole) { dp.subsample = 1; dp.world = 1; dp.rank = 0; dp.num_parts = 1; dp.part_idx = 0; }
	return dp;
}

/* k-mers per read into nk (n) and their exclusive scan into koff (n + 1), queued: k-mer i of read r has slot koff[r] + i.  most_err:
 * two device words, zero before: the most k-mers of a read, and 1 if a read holds 2^32 or more */
int kmer_slots_queue(kmr_handle *h, const uint64_t *offsets, uint64_t n, uint32_t *nk, uint64_t *koff, unsigned int *most_err) {
	LAUNCH(h, compare_nk_kernel, dim3(grid_for(n)), dim3(256), 0, offsets, n, h->k, nk, most_err, most_err + 1);
	return exclusive_scan_queue(h, nk, n, koff);
}
/* ... in h->cmp_buf (*koff), with the call's one fixed-size copy behind: all slots, the most of a read, the error word (waits).  A read
 * of 2^32 k-mers or more is refused with the caller's text */
int kmer_slot_plan(kmr_handle *h, const uint64_t *offsets, uint64_t n, uint64_t **koff, uint64_t *total, unsigned int *most, const char *refusal) {
	DevBuf *B = h->cmp_buf;
	int rc = B[CMP_B_ACC].reserve(h, "compare counters", 256); if (rc) return rc;
	rc = B[CMP_B_NK].reserve(h, "compare k-mer counts", 4 * std::max<uint64_t>(n, 1)); if (rc) return rc;
	rc = B[CMP_B_KOFF].reserve(h, "compare k-mer offsets", 8 * (n + 1)); if (rc) return rc;
	unsigned int *most_err = (unsigned int *)((unsigned long long *)(B[CMP_B_ACC].get<CompareRec>() + 1) + CMP_T_WORDS), hm[2] = {0, 0};
	*koff = B[CMP_B_KOFF].get<uint64_t>(); *total = 0;
	HIPCHK(h, hipMemsetAsync(most_err, 0, 8, h->stream));
	rc = kmer_slots_queue(h, offsets, n, B[CMP_B_NK].get<uint32_t>(), *koff, most_err); if (rc) return rc;
	HIPCHK(h, fetch_queue(h, total, *koff + n));
	HIPCHK(h, fetch_queue(h, hm, most_err, 2));
	HIPCHK(h, stream_wait(h));
	*most = hm[0];
	return hm[1] ? fail(h, KMR_ERR_UNSUPPORTED, refusal) : 0;
}

/* Stages one run: `slots` slots of `words` words in buf, all ones, then reads [first, first + count) of the batch through
 * extract_kernel with op, whose stage this sets */
template <int W, class Op> int stage_run(kmr_handle *h, DevBuf &buf, const char *what, const ReadsView &all, uint64_t first, uint64_t count, uint64_t slots, uint32_t words,
                                         const DevParams &dp, Op op) {
	int rc = buf.reserve(h, what, 8ull * words * slots); if (rc) return rc;
	op.stage = buf.get<uint64_t>();
	HIPCHK(h, hipMemsetAsync(op.stage, 0xff, 8ull * words * slots, h->stream));
	ReadsView rv = reads_slice(all, first, count);
	rc = prepare_units(h, rv); if (rc) return rc;
	return launch_extract<W, false>(h, rv, dp, op);
}

uint64_t map_entries(const DevMap &m) { return m.present ? m.n : 0; }

/* size, count sum and saturated entries of h's map into tot (CMP_T_WORDS words, zeroed here), on stream s */
int compare_totals(kmr_handle *h, kmr_handle *on, unsigned long long *tot) {
	HIPCHK(on, hipMemsetAsync(tot, 0, 8 * CMP_T_WORDS, on->stream));
	const uint64_t nw = map_entries(h->weak), ns = map_entries(h->sing);
	if (nw + ns == 0) return 0;
	LAUNCH(on, compare_totals_kernel, dim3(grid_for(nw + ns)), dim3(256), 0, h->weak.vals.get<uint32_t>(), value_words(h), nw, h->sing.sweight.get<uint8_t>(), ns, tot);
	return 0;
}

template <int W> int compare_spectrums_t(kmr_handle *h1, kmr_handle *h2, kmr_compare_counts *out) {
	int rc = h2->cmp_buf[CMP_B_ACC].reserve(h2, "compare counters", 256); if (rc) return rc;
	CompareRec *acc = h2->cmp_buf[CMP_B_ACC].get<CompareRec>();
	unsigned long long *tot2 = (unsigned long long *)(acc + 1);
	if (h1 != h2) HIPCHK(h2, hipStreamSynchronize(h1->stream));      /* h1's maps are complete before h2's stream reads them */
	HIPCHK(h2, hipMemsetAsync(acc, 0, sizeof(CompareRec), h2->stream));
	rc = compare_totals(h2, h2, tot2); if (rc) return rc;
	const uint64_t nw1 = map_entries(h1->weak), ns1 = map_entries(h1->sing);
	if (nw1 + ns1) {
		LAUNCH(h2, compare_maps_kernel<W>, dim3(grid_for(nw1 + ns1)), dim3(256), 0, view_of<W>(h1->weak, value_words(h1)), nw1, view_of<W>(h1->sing, 0), ns1,
		       view_of<W>(h2->weak, value_words(h2)), view_of<W>(h2->sing, 0), h2->hkb, acc);
	}
	unsigned long long host[8 + CMP_T_WORDS];
	HIPCHK(h2, fetch(h2, host, acc, 8 + CMP_T_WORDS));
	const CompareRec *a = (const CompareRec *)host; const unsigned long long *t = host + 8;
	out->size1 = a->size1; out->size2 = t[CMP_T_SIZE]; out->common = a->common; out->common_count1 = a->common_count1; out->common_count2 = a->common_count2;
	out->total_count1 = a->total_count1; out->total_count2 = t[CMP_T_TOTAL]; out->saturated = a->saturated + t[CMP_T_SATURATED];
	return KMR_OK;
}

/* the sorted path over the run's reads of more than cap k-mers (all of them at cap 0): see kmr_compare.hpp */
template <int W> int compare_long_run(kmr_handle *h, const uint64_t *stage, const uint64_t *koff, uint64_t r0, uint64_t m, uint32_t cap, const unsigned long long *tot2, CompareRec *out) {
	DevBuf *B = h->cmp_buf;
	const dim3 block(256);
	int rc = B[CMP_B_CNT].reserve(h, "compare long counts", 4 * m); if (rc) return rc;
	rc = B[CMP_B_LOFF].reserve(h, "compare long offsets", 8 * (m + 1)); if (rc) return rc;
	uint32_t *cnt = B[CMP_B_CNT].get<uint32_t>(); uint64_t *loff = B[CMP_B_LOFF].get<uint64_t>();
	LAUNCH(h, compare_long_count_kernel, dim3(grid_for(m)), block, 0, koff, r0, m, cap, tot2, cnt, out);
	rc = exclusive_scan_queue(h, cnt, m, loff); if (rc) return rc;
	uint64_t c = 0;
	HIPCHK(h, fetch(h, &c, loff + m));
	if (c == 0) return 0;
	if (c >= 0xffffffffull) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_compare_reads: a run of the sorted path holds 2^32 - 1 k-mers or more (lower kmr_tune \"compare_stage_kmers\")");
	rc = B[CMP_B_SRC].reserve(h, "compare sort slots", 4 * c); if (rc) return rc;
	rc = B[CMP_B_RID].reserve(h, "compare sort reads", 4 * c); if (rc) return rc;
	rc = B[CMP_B_PERM].reserve(h, "compare sort order", 4 * c); if (rc) return rc;
	rc = B[CMP_B_HSCAN].reserve(h, "compare heads", 8 * (c + 1)); if (rc) return rc;
	rc = B[CMP_B_START].reserve(h, "compare head starts", 8 * (c + 1)); if (rc) return rc;
	uint32_t *src = B[CMP_B_SRC].get<uint32_t>(), *rid = B[CMP_B_RID].get<uint32_t>();
	uint64_t *hscan = B[CMP_B_HSCAN].get<uint64_t>(), *start = B[CMP_B_START].get<uint64_t>();
	const dim3 cgrid(grid_for(c));
	LAUNCH(h, compare_long_fill_kernel, cgrid, block, 0, koff, r0, m, (const uint64_t *)loff, c, src, rid, B[CMP_B_PERM].get<uint32_t>());
	/* least significant first: the key words, then the read; the sort is stable */
	SortColumn cols[W + 1];
	for (int w = 0; w < W; w++) cols[w] = SortColumn{stage + w, (uint64_t)W, src, nullptr};
	cols[W] = SortColumn{nullptr, 0, nullptr, rid};
	const uint32_t *perm; unsigned long long *kout;
	rc = sort_by_columns(h, h->cmp_sort, cols, W + 1, B[CMP_B_PERM].get<uint32_t>(), c, "kmr_compare_reads", &perm, &kout); if (rc) return rc;
	uint32_t *head = (uint32_t *)kout;      /* the sort keys are dead once the order stands */
	LAUNCH(h, compare_long_heads_kernel, cgrid, block, 0, stage, (uint32_t)W, (const uint32_t *)src, (const uint32_t *)rid, perm, c, head);
	rc = exclusive_scan_queue(h, head, c, hscan); if (rc) return rc;
	rc = group_starts(h, head, hscan, c, start); if (rc) return rc;
	LAUNCH(h, compare_long_add_kernel<W>, cgrid, block, 0, stage, (const uint32_t *)src, (const uint32_t *)rid, perm, (const uint32_t *)head, (const uint64_t *)hscan,
	       (const uint64_t *)start, c, r0, view_of<W>(h->weak, value_words(h)), view_of<W>(h->sing, 0), h->hkb, out);
	return 0;
}

template <int W> int compare_reads_t(kmr_handle *h, const ReadsView &all, CompareRec *out) {
	DevBuf *B = h->cmp_buf;
	const uint64_t n = all.n_reads;
	int rc = B[CMP_B_ACC].reserve(h, "compare counters", 256); if (rc) return rc;
	unsigned long long *tot2 = (unsigned long long *)(B[CMP_B_ACC].get<CompareRec>() + 1);
	rc = compare_totals(h, h, tot2); if (rc) return rc;
	uint64_t *koff, total; unsigned int most;
	rc = kmer_slot_plan(h, all.offsets, n, &koff, &total, &most, "kmr_compare_reads: a read of 2^32 k-mers or more"); if (rc) return rc;
	const uint32_t cap = h->tune.compare_lds_kmers < 0 ? CMP_CAP : (uint32_t)h->tune.compare_lds_kmers;
	const uint64_t budget = h->tune.compare_stage_kmers ? h->tune.compare_stage_kmers : CMP_STAGE_SLOTS;
	/* runs of whole reads (cut_runs).  Only a batch of more k-mers than one run holds has its offsets looked at by the host */
	std::vector<uint64_t> hk, cut = {0, n};
	if (total > budget) {
		hk.resize(n + 1);
		HIPCHK(h, hipMemcpy(hk.data(), koff, 8 * (n + 1), hipMemcpyDeviceToHost));
		cut = cut_runs(n, budget, [&](uint64_t r) { return hk[r]; });
	}
	const DevParams dp = own_reads_params(h, false);      /* a read's own map subtracts nothing */
	const MapView<W> weak = view_of<W>(h->weak, value_words(h)), sing = view_of<W>(h->sing, 0);
	for (size_t i = 0; i + 1 < cut.size(); i++) {
		const uint64_t r0 = cut[i], m = cut[i + 1] - r0;
		const uint64_t slots = hk.empty() ? total : hk[r0 + m] - hk[r0];
		if (slots) {
			CompareOp<W> op; op.koff = koff; op.slot_base = hk.empty() ? 0 : hk[r0];
			rc = stage_run<W>(h, B[CMP_B_STAGE], "compare staging", all, r0, m, slots, W, dp, op); if (rc) return rc;
		}
		const uint64_t *stage = B[CMP_B_STAGE].get<uint64_t>();
		if (cap) {
			const size_t smem = (size_t)CMP_WAVES * cap * W * 8;
			HIPCHK(h, hipFuncSetAttribute((const void *)compare_reads_lds_kernel<W>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)CMP_WAVES * CMP_CAP_MOST * W * 8)));
			const uint64_t blocks = std::min<uint64_t>((m + CMP_WAVES - 1) / CMP_WAVES, (uint64_t)num_cus(h) * 16);
			LAUNCH(h, compare_reads_lds_kernel<W>, dim3((unsigned)blocks), dim3(CMP_WAVES * 64), smem, stage, (const uint64_t *)koff, r0, m, cap, weak, sing, h->hkb,
			       (const unsigned long long *)tot2, out);
		}
		if (cap == 0 || most > cap) { rc = compare_long_run<W>(h, stage, koff, r0, m, cap, tot2, out); if (rc) return rc; }
	}
	return KMR_OK;
}

/* the staging of compare_reads_t for the whole batch in one run, for a handle of one key word (see kmr_host.hpp) */
int tnf_stage(kmr_handle *h, const ReadsView &all, const uint64_t **koff_out, const uint64_t **stage_out, uint64_t *slots) {
	uint64_t *koff, total; unsigned int most;
	int rc = kmer_slot_plan(h, all.offsets, all.n_reads, &koff, &total, &most, "a sequence of 2^32 k-mers or more"); if (rc) return rc;
	*koff_out = koff; *slots = total; *stage_out = nullptr;
	if (total == 0) return KMR_OK;
	CompareOp<1> op; op.koff = koff; op.slot_base = 0;
	rc = stage_run<1>(h, h->cmp_buf[CMP_B_STAGE], "compare staging", all, 0, all.n_reads, total, 1, own_reads_params(h, true), op); if (rc) return rc;
	*stage_out = h->cmp_buf[CMP_B_STAGE].get<uint64_t>();
	return KMR_OK;
}

/* ---- KmerMatch (kmr_match.hpp): the table of kmr_match_create and the streaming pass of kmr_match_add_read_batch (kmr_stages.hip) ---- */
template <int W> int match_create_t(kmr_handle *h, kmr_match *m, const uint8_t *bases, const uint64_t *offsets, uint64_t nc) {
	const dim3 block(256);
	const int64_t M64 = (int64_t)m->cfg.max_positions_from_edge - (int64_t)h->k + 1;
	const int32_t M = (int32_t)std::max<int64_t>(M64, -1);      /* every negative value means the same: all k-mers */
	DevBuf b_cnt, b_eoff, b_err;
	uint32_t *cnt, *err; uint64_t *eoff;
	HIPCHK(h, alloc_n(b_cnt, &cnt, nc + 1)); HIPCHK(h, alloc_n(b_eoff, &eoff, nc + 1)); HIPCHK(h, alloc_n(b_err, &err, (size_t)1));
	HIPCHK(h, hipMemsetAsync(err, 0, 4, h->stream)); HIPCHK(h, hipMemsetAsync(eoff, 0, 8, h->stream));
	uint64_t E = 0; uint32_t herr = 0;
	if (nc) {
		LAUNCH(h, match_edge_count_kernel, dim3(grid_for(nc)), block, 0, offsets, nc, h->k, M, cnt, err);
		int rc = exclusive_scan_queue(h, cnt, nc, eoff); if (rc) return rc;
		HIPCHK(h, fetch_queue(h, &E, eoff + nc));
		HIPCHK(h, fetch_queue(h, &herr, err));
		HIPCHK(h, stream_wait(h));
	}
	if (herr) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_match_create: a contig of 2^31 - 1 bases or more");
	if (E >= 0xffffffffull) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_match_create: 2^32 - 1 edge k-mers or more");
	m->n_contigs = nc; m->n_edge_kmers = E; m->n_distinct_keys = m->n_keys_in_spectrum = 0;
	uint64_t n_lists = 0;      /* (key, contig) pairs of the kept keys */
	DevBuf b_keys, b_contig, b_order, b_flags, b_scans; SortBufs sort;
	uint64_t *keys = nullptr, *scans = nullptr; uint32_t *contig = nullptr, *order = nullptr, *flags = nullptr; const uint32_t *perm = nullptr;
	if (E) {
		HIPCHK(h, alloc_n(b_keys, &keys, E * W)); HIPCHK(h, alloc_n(b_contig, &contig, E)); HIPCHK(h, alloc_n(b_order, &order, E));
		HIPCHK(h, alloc_n(b_flags, &flags, 3 * E)); HIPCHK(h, alloc_n(b_scans, &scans, 3 * (E + 1)));
		const dim3 egrid(grid_for(E));
		LAUNCH(h, match_edge_keys_kernel<W>, egrid, block, 0, bases, offsets, nc, h->k, M, (const uint64_t *)eoff, E, keys, contig, order);
		/* least significant first: the contig, then the key words from the last to the first; the sort is stable */
		SortColumn cols[W + 1];
		cols[0] = SortColumn{nullptr, 0, nullptr, contig};
		for (int w = 0; w < W; w++) cols[1 + w] = SortColumn{keys + (W - 1 - w), (uint64_t)W, nullptr, nullptr};
		int rc = sort_by_columns(h, sort, cols, W + 1, order, E, "kmr_match_create", &perm, nullptr); if (rc) return rc;
		MapView<W> weak = view_of<W>(h->weak, value_words(h)), sing = view_of<W>(h->sing, 0);
		if (!h->has_singletons) sing.nb = 0;
		uint32_t *khead = flags, *kkept = flags + E, *phead = flags + 2 * E;
		uint64_t *hscan = scans, *kscan = scans + (E + 1), *pscan = scans + 2 * (E + 1);
		LAUNCH(h, match_flags_kernel<W>, egrid, block, 0, (const uint64_t *)keys, (const uint32_t *)contig, (const uint32_t *)perm, E, weak, sing, h->hkb, khead, kkept, phead);
		rc = exclusive_scan_queue(h, khead, E, hscan); if (rc) return rc;
		rc = exclusive_scan_queue(h, kkept, E, kscan); if (rc) return rc;
		rc = exclusive_scan_queue(h, phead, E, pscan); if (rc) return rc;
		HIPCHK(h, fetch_queue(h, &m->n_distinct_keys, hscan + E));
		HIPCHK(h, fetch_queue(h, &m->n_keys_in_spectrum, kscan + E));
		HIPCHK(h, fetch_queue(h, &n_lists, pscan + E));
		HIPCHK(h, stream_wait(h));
	}
	m->log2cap = 6;
	while ((1ull << m->log2cap) < 2 * m->n_keys_in_spectrum) m->log2cap++;      /* at most half full */
	const size_t slot_bytes_ = (size_t)(W + 1) * 8 << m->log2cap;
	HIPCHK(h, m->slots.alloc(slot_bytes_));
	HIPCHK(h, m->tcontig.alloc(std::max<size_t>(4 * n_lists, 256)));
	HIPCHK(h, hipMemsetAsync(m->slots.get(), 0xff, slot_bytes_, h->stream));
	if (m->n_keys_in_spectrum) {
		LAUNCH(h, match_table_fill_kernel<W>, dim3(grid_for(E)), block, 0, (const uint64_t *)keys, (const uint32_t *)contig, (const uint32_t *)perm, E,
		       (const uint32_t *)flags, (const uint32_t *)(flags + E), (const uint32_t *)(flags + 2 * E), (const uint64_t *)(scans + 2 * (E + 1)),
		       m->slots.get<uint64_t>(), 64u - m->log2cap, m->tcontig.get<uint32_t>());
	}
	HIPCHK(h, hipStreamSynchronize(h->stream));      /* the temporaries go */
	return KMR_OK;
}

template <int W> int match_add_t(kmr_handle *h, kmr_match *m, const ReadsView &all, uint64_t first_global, const int64_t *mate) {
	if (!m->hit_count) { HIPCHK(h, m->hit_count.alloc(256)); HIPCHK(h, hipMemsetAsync(m->hit_count.get(), 0, 8, h->stream)); }
	if (m->hit_cap == 0) {
		const uint64_t cap = h->tune.match_hit_capacity ? h->tune.match_hit_capacity : MATCH_HIT_CAP;
		HIPCHK(h, m->hit_key.alloc(std::max<size_t>(8 * cap, 256))); HIPCHK(h, m->hit_mate.alloc(std::max<size_t>(8 * cap, 256)));
		m->hit_cap = cap;
	}
	const DevParams dp = own_reads_params(h, false);      /* the spectrum's own reads: nothing is subtracted */
	ReadsView rv = all;
	int rc = prepare_units(h, rv); if (rc) return rc;
	for (int attempt = 1;; attempt++) {
		MatchOp<W> op;
		op.table.slots = m->slots.get<uint64_t>(); op.table.contigs = m->tcontig.get<uint32_t>(); op.table.shift = 64u - m->log2cap;
		op.hit_key = m->hit_key.get<unsigned long long>(); op.hit_mate = m->hit_mate.get<unsigned long long>(); op.count = m->hit_count.get<unsigned long long>();
		op.cap = m->hit_cap; op.mate = mate; op.first_global = first_global;
		rc = launch_extract<W, false>(h, rv, dp, op); if (rc) return rc;
		uint64_t count = 0;
		HIPCHK(h, fetch(h, &count, m->hit_count.get()));
		h->last_match_attempts = attempt;
		if (count <= m->hit_cap) { m->n_hits = count; return KMR_OK; }
		/* the records did not fit: room for all of them (the count of a batch repeats), the earlier batches' records kept, and once more */
		if (count >= 0xffffffffull) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_match_add_read_batch: 2^32 - 1 hit records or more");
		if (attempt >= 3) return fail(h, KMR_ERR_CAPACITY, "kmr_match_add_read_batch: the hit records did not fit after their buffers grew (internal sizing error)");
		const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(count, 2 * m->hit_cap), 0xfffffffeull);
		DevBuf nk, nm;
		HIPCHK(h, nk.alloc(8 * cap)); HIPCHK(h, nm.alloc(8 * cap));
		if (m->n_hits) {
			HIPCHK(h, hipMemcpyAsync(nk.get(), m->hit_key.get(), 8 * m->n_hits, hipMemcpyDeviceToDevice, h->stream));
			HIPCHK(h, hipMemcpyAsync(nm.get(), m->hit_mate.get(), 8 * m->n_hits, hipMemcpyDeviceToDevice, h->stream));
		}
		HIPCHK(h, hipMemcpyAsync(m->hit_count.get(), &m->n_hits, 8, hipMemcpyHostToDevice, h->stream));
		HIPCHK(h, hipStreamSynchronize(h->stream));
		m->hit_key = std::move(nk); m->hit_mate = std::move(nm); m->hit_cap = cap;
	}
}

/* ---- ContigExtender (kmr_extend.hpp): everything of kmr_extend_contigs* behind the argument checks (kmr_stages.hip) ---- */
struct ExtendBufs { DevBuf stage, sgrp, order, flags, scans, cnt, val, wkeys, wcnt, wval, skeys, bounds, rec; SortBufs sort; };      /* what extend_t keeps across the runs of a call, grow-only */

/* The pool spectra of one run: items [i0, i0 + ni) of the gathered batch, S > 0 slots from slot0, contigs [A.c0, A.c0 + A.m).  Stage,
 * sort, reduce: A's tables set, A.bounds (zero before) filled.  Waits once, for the sizes of the tables */
template <int W> int extend_run_spectra(kmr_handle *h, ExtendBufs &B, const ReadsView &all, const DevParams &dp, const uint64_t *koff, const uint32_t *grp, uint64_t i0, uint64_t ni,
                                        uint64_t slot0, uint64_t S, EventTimer<5> &tr, ExtendArgs &A) {
	const dim3 block(256), sgrid(grid_for(S));
	ExtendOp<W> op; op.koff = koff; op.slot_base = slot0;
	int rc = stage_run<W>(h, B.stage, "extend staging", all, i0, ni, S, W + 1, dp, op); if (rc) return rc;
	const uint64_t *stage = B.stage.get<uint64_t>();
	tr.mark(1, h->stream);
	rc = B.sgrp.reserve(h, "extend groups", 4 * S); if (rc) return rc;
	rc = B.order.reserve(h, "extend sort order", 4 * S); if (rc) return rc;
	rc = B.flags.reserve(h, "extend flags", 8 * S); if (rc) return rc;
	rc = B.scans.reserve(h, "extend scans", 16 * (S + 1)); if (rc) return rc;
	rc = B.cnt.reserve(h, "extend counts", 4 * S); if (rc) return rc;
	rc = B.val.reserve(h, "extend weights", 4 * S); if (rc) return rc;
	uint32_t *sgrp = B.sgrp.get<uint32_t>(), *wflag = B.flags.get<uint32_t>(), *sflag = wflag + S, *cnt = B.cnt.get<uint32_t>(); float *val = B.val.get<float>();
	uint64_t *wscan = B.scans.get<uint64_t>(), *sscan = wscan + (S + 1);
	LAUNCH(h, extend_fill_kernel, sgrid, block, 0, koff, i0, ni, grp, S, sgrp, B.order.get<uint32_t>());
	/* least significant first: the key words from the last to the first, then (contig, source); the sort is stable */
	SortColumn cols[W + 1];
	for (int w = 0; w < W; w++) cols[w] = SortColumn{stage + (W - 1 - w), (uint64_t)W + 1, nullptr, nullptr};
	cols[W] = SortColumn{nullptr, 0, nullptr, sgrp};
	const uint32_t *perm; unsigned long long *sorted_grp;      /* the last pass's keys */
	rc = sort_by_columns(h, B.sort, cols, W + 1, B.order.get<uint32_t>(), S, "kmr_extend_contigs", &perm, &sorted_grp); if (rc) return rc;
	tr.mark(2, h->stream);
	LAUNCH(h, extend_reduce_kernel, sgrid, block, 0, stage, (uint32_t)W, (const uint32_t *)sgrp, perm, S, h->cfg.separate_singletons ? 1u : 0u, wflag, sflag, cnt, val);
	rc = exclusive_scan_queue(h, wflag, S, wscan); if (rc) return rc;
	rc = exclusive_scan_queue(h, sflag, S, sscan); if (rc) return rc;
	uint64_t nw = 0, ns = 0;
	HIPCHK(h, fetch_queue(h, &nw, wscan + S));
	HIPCHK(h, fetch_queue(h, &ns, sscan + S));
	HIPCHK(h, stream_wait(h));
	rc = B.wkeys.reserve(h, "extend weak keys", std::max<size_t>(8ull * W * nw, 256)); if (rc) return rc;
	rc = B.wcnt.reserve(h, "extend weak counts", std::max<size_t>(4 * nw, 256)); if (rc) return rc;
	rc = B.wval.reserve(h, "extend weak weights", std::max<size_t>(4 * nw, 256)); if (rc) return rc;
	rc = B.skeys.reserve(h, "extend solid keys", std::max<size_t>(8ull * W * ns, 256)); if (rc) return rc;
	A.wkeys = B.wkeys.get<uint64_t>(); A.wcnt = B.wcnt.get<uint32_t>(); A.wval = B.wval.get<float>(); A.skeys = B.skeys.get<uint64_t>();
	LAUNCH(h, extend_compact_kernel, sgrid, block, 0, stage, (uint32_t)W, perm, S, (const uint32_t *)wflag, (const uint32_t *)sflag, (const uint64_t *)wscan,
	       (const uint64_t *)sscan, (const uint32_t *)cnt, (const float *)val, B.wkeys.get<uint64_t>(), B.wcnt.get<uint32_t>(), B.wval.get<float>(), B.skeys.get<uint64_t>());
	LAUNCH(h, extend_bounds_kernel, dim3(grid_for(A.m)), block, 0, (const unsigned long long *)sorted_grp, S, (const uint64_t *)wscan, (const uint64_t *)sscan, A.c0, A.m, (uint64_t *)A.bounds);
	return 0;
}

template <int W> int extend_t(kmr_handle *h, const kmr_reads *contigs, const kmr_reads *reads, const uint64_t *po, const uint64_t *pr, const uint8_t *active,
                              const kmr_extend_config *cfg, kmr_extend *out) {
	const dim3 block(256);
	const uint64_t nc = contigs->n;
	const uint32_t maxx = cfg->max_extend;
	const uint8_t *cbases = contigs->bases.get<uint8_t>(); const uint64_t *coff = contigs->offsets.get<uint64_t>();
	out->n = nc; out->n_extended = out->bases_added = 0;
	h->last_extend_runs = 0;
	for (double &t : h->last_extend_ms) t = 0;
	auto result = std::unique_ptr<kmr_reads>(new kmr_reads);
	result->device = h->device; result->n = nc; result->input_base = h->cfg.fastq_start_char;
	uint64_t *noff;
	HIPCHK(h, alloc_n(result->offsets, &noff, nc + 1));
	HIPCHK(h, hipMemsetAsync(noff, 0, 8 * (nc + 1), h->stream));
	HIPCHK(h, result->name_off.alloc(8 * std::max<uint64_t>(nc, 1))); HIPCHK(h, result->name_len.alloc(4 * std::max<uint64_t>(nc, 1)));
	HIPCHK(h, hipMemsetAsync(result->name_off.get(), 0, 8 * std::max<uint64_t>(nc, 1), h->stream)); HIPCHK(h, hipMemsetAsync(result->name_len.get(), 0, 4 * std::max<uint64_t>(nc, 1), h->stream));
	uint32_t *newlen, *left, *right, *reason; double *vals;
	HIPCHK(h, alloc_n(out->newlen, &newlen, nc)); HIPCHK(h, alloc_n(out->left, &left, nc)); HIPCHK(h, alloc_n(out->right, &right, nc));
	HIPCHK(h, alloc_n(out->reason, &reason, 2 * nc)); HIPCHK(h, alloc_n(out->vals, &vals, 2 * nc * EXT_VALS));
	if (nc == 0) {
		HIPCHK(h, result->bases.alloc(64)); HIPCHK(h, result->quals.alloc(64));
		HIPCHK(h, hipStreamSynchronize(h->stream));
		out->result = result.release();
		return KMR_OK;
	}
	/* 1: the offsets, then the items */
	DevBuf b_small, b_len, b_grp, b_goff, b_nk, b_koff;
	uint32_t *err; HIPCHK(h, alloc_n(b_small, &err, (size_t)64));
	unsigned long long *info = (unsigned long long *)(err + 8);      /* (err + 2: kmer_slots_queue's two words) */
	HIPCHK(h, hipMemsetAsync(err, 0, 256, h->stream));
	LAUNCH(h, extend_check_offsets_kernel, dim3(grid_for(nc + 1)), block, 0, po, nc, err);
	std::vector<uint64_t> hpo(nc + 1);
	uint32_t herr = 0;
	HIPCHK(h, fetch_queue(h, hpo.data(), po, nc + 1));
	HIPCHK(h, fetch_queue(h, &herr, err));
	HIPCHK(h, stream_wait(h));
	if (herr) return fail(h, KMR_ERR_INVALID_ARG, "kmr_extend_contigs: pool_offsets does not start at 0 or does not ascend");
	const uint64_t P = hpo[nc], n_items = P + nc;
	if (n_items >= 0xffffffffull) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_extend_contigs: 2^32 - 1 pooled reads and contigs or more");
	EventTimer<2> tg(h->tune.extend_timing);
	tg.mark(0, h->stream);
	uint32_t *len, *grp, *nk; uint64_t *goff, *koff;
	HIPCHK(h, alloc_n(b_len, &len, n_items)); HIPCHK(h, alloc_n(b_grp, &grp, n_items)); HIPCHK(h, alloc_n(b_goff, &goff, n_items + 1));
	HIPCHK(h, alloc_n(b_nk, &nk, n_items)); HIPCHK(h, alloc_n(b_koff, &koff, n_items + 1));
	LAUNCH(h, extend_item_kernel, dim3(grid_for(n_items)), block, 0, po, pr, active, reads->offsets.get<uint64_t>(), reads->n, coff, nc, n_items, len, grp, err);
	int rc = exclusive_scan_queue(h, len, n_items, goff); if (rc) return rc;
	uint64_t G = 0;
	HIPCHK(h, fetch_queue(h, &G, goff + n_items));
	HIPCHK(h, fetch_queue(h, &herr, err));
	HIPCHK(h, stream_wait(h));
	if (herr & 2u) return fail(h, KMR_ERR_INVALID_ARG, "kmr_extend_contigs: a pool index lies outside the read batch");
	if (herr & 4u) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_extend_contigs: a sequence of 2^31 - 1 bases or more");
	/* 2: the gathered batch and its k-mer slots */
	DevBuf b_gb, b_gq;
	HIPCHK(h, b_gb.alloc(G + 64)); HIPCHK(h, b_gq.alloc(G + 64));
	uint8_t *gb = b_gb.get<uint8_t>(), *gq = b_gq.get<uint8_t>();
	HIPCHK(h, hipMemsetAsync(gb + G, 0, 64, h->stream)); HIPCHK(h, hipMemsetAsync(gq + G, 0, 64, h->stream));
	if (G) {
		LAUNCH(h, extend_gather_kernel, dim3(grid_for((G + 63) / 64)), block, 0, (const uint64_t *)goff, n_items, G, po, pr, (const uint32_t *)grp, reads->bases.get<uint8_t>(),
		       reads->quals.get<uint8_t>(), reads->offsets.get<uint64_t>(), cbases, coff, gb, gq);
	}
	rc = kmer_slots_queue(h, goff, n_items, nk, koff, err + 2); if (rc) return rc;      /* (an item of 2^32 k-mers was refused above) */
	tg.mark(1, h->stream);
	std::vector<uint64_t> hk(n_items + 1);
	HIPCHK(h, fetch(h, hk.data(), koff, n_items + 1));
	h->last_extend_ms[0] = tg.ms(0, 1);
	/* 3: runs of whole contigs, each with its pool (cut_runs); contig c's items begin at hpo[c] + c */
	const uint64_t budget = h->tune.extend_stage_kmers ? h->tune.extend_stage_kmers : EXT_STAGE_SLOTS;
	const std::vector<uint64_t> cut = cut_runs(nc, budget, [&](uint64_t c) { return hk[hpo[c] + c]; });
	/* the sequences with max_extend free bases on either side, the recorded keys */
	DevBuf b_seq;
	HIPCHK(h, b_seq.alloc(std::max<uint64_t>(contigs->total + 2ull * maxx * nc, 256)));
	const size_t rec_wave = (size_t)2 * maxx * W * 8;
	const bool rec_lds = rec_wave <= EXT_LDS_WAVE_BYTES;
	const DevParams dp = own_reads_params(h, true);      /* a pool's spectrum is whole */
	const ReadsView all = reads_view(gb, gq, goff, n_items);
	ExtendBufs B;
	for (size_t ri = 0; ri + 1 < cut.size(); ri++) {
		const uint64_t c0 = cut[ri], m = cut[ri + 1] - c0;
		const uint64_t i0 = hpo[c0] + c0, i1 = hpo[c0 + m] + c0 + m, S = hk[i1] - hk[i0];
		if (S >= 0xffffffffull) return fail(h, KMR_ERR_UNSUPPORTED, "kmr_extend_contigs: a run of 2^32 - 1 k-mers or more (lower kmr_tune \"extend_stage_kmers\")");
		EventTimer<5> tr(h->tune.extend_timing);
		tr.mark(0, h->stream);
		uint64_t *bounds;
		HIPCHK(h, alloc_n(B.bounds, &bounds, 4 * m));
		HIPCHK(h, hipMemsetAsync(bounds, 0, 32 * m, h->stream));
		ExtendArgs A;
		A.cbases = cbases; A.coff = coff; A.active = active; A.c0 = c0; A.m = m;
		A.wkeys = A.skeys = nullptr; A.wcnt = nullptr; A.wval = nullptr; A.bounds = bounds;
		if (S) { rc = extend_run_spectra<W>(h, B, all, dp, koff, grp, i0, i1 - i0, hk[i0], S, tr, A); if (rc) return rc; }
		else { tr.mark(1, h->stream); tr.mark(2, h->stream); }
		tr.mark(3, h->stream);
		A.k = h->k; A.max_extend = maxx; A.use_weights = cfg->use_weights ? 1u : 0u;
		A.min_consensus = cfg->minimum_consensus / 100; A.min_coverage = cfg->minimum_coverage; A.max_delta = cfg->maximum_delta_ratio;
		A.seq = b_seq.get<uint8_t>(); A.left = left; A.right = right; A.reason = reason; A.vals = vals;
		const uint64_t blocks = std::min<uint64_t>((m + EXT_WAVES - 1) / EXT_WAVES, (uint64_t)num_cus(h) * 8);
		A.rec_global = nullptr;
		if (!rec_lds) { rc = B.rec.reserve(h, "extend recorded keys", std::max<size_t>(rec_wave * EXT_WAVES * blocks, 256)); if (rc) return rc; A.rec_global = B.rec.get<uint64_t>(); }
		LAUNCH(h, extend_contigs_kernel<W>, dim3((unsigned)blocks), dim3(EXT_WAVES * 64), rec_lds ? rec_wave * EXT_WAVES : 0, A);
		tr.mark(4, h->stream);
		h->last_extend_runs++;
		if (tr.on) {
			HIPCHK(h, hipStreamSynchronize(h->stream));
			for (int i = 0; i < 4; i++) h->last_extend_ms[1 + i] += tr.ms(i, i + 1);
		}
	}
	/* 4: the result batch */
	LAUNCH(h, extend_newlen_kernel, dim3(grid_for(nc)), block, 0, coff, nc, (const uint32_t *)left, (const uint32_t *)right, newlen, info);
	rc = exclusive_scan_queue(h, newlen, nc, noff); if (rc) return rc;
	unsigned long long hinfo[2] = {0, 0};
	HIPCHK(h, fetch_queue(h, &result->total, noff + nc));
	HIPCHK(h, fetch_queue(h, hinfo, info, 2));
	HIPCHK(h, stream_wait(h));
	out->n_extended = hinfo[0]; out->bases_added = hinfo[1];
	const uint64_t T = result->total;
	HIPCHK(h, result->bases.alloc(T + 64)); HIPCHK(h, result->quals.alloc(T + 64));
	HIPCHK(h, hipMemsetAsync(result->bases.get<uint8_t>() + T, 0, 64, h->stream)); HIPCHK(h, hipMemsetAsync(result->quals.get<uint8_t>() + T, 0, 64, h->stream));
	if (T) {
		LAUNCH(h, extend_result_kernel, dim3(grid_for((T + 63) / 64)), block, 0, (const uint64_t *)noff, nc, T, b_seq.get<uint8_t>(), coff, (const uint32_t *)left, maxx,
		       result->bases.get<uint8_t>(), result->quals.get<uint8_t>());
	}
	HIPCHK(h, hipStreamSynchronize(h->stream));      /* the temporaries go */
	out->result = result.release();
	return KMR_OK;
}

}  // namespace

namespace kmr_host {
int extend_core(kmr_handle *h, const kmr_reads *contigs, const kmr_reads *reads, const uint64_t *pool_offsets, const uint64_t *pool_reads, const uint8_t *active,
                const kmr_extend_config *cfg, kmr_extend *out) {
	const int rc = with_w(h, [&](auto W) { return extend_t<W()>(h, contigs, reads, pool_offsets, pool_reads, active, cfg, out); });
	if (rc) hipStreamSynchronize(h->stream);
	return rc;
}
int tnf_stage_core(kmr_handle *h, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t n_reads, const uint64_t **koff, const uint64_t **stage, uint64_t *slots) {
	if (h->W != 1) return fail(h, KMR_ERR_UNSUPPORTED, "tnf_stage_core: a key of more than one word");
	const int rc = tnf_stage(h, reads_view(bases, quals, offsets, n_reads), koff, stage, slots);
	if (rc) hipStreamSynchronize(h->stream);
	return rc;
}
int match_create_core(kmr_handle *h, kmr_match *m, const uint8_t *bases, const uint64_t *offsets, uint64_t n_contigs) {
	const int rc = with_w(h, [&](auto W) { return match_create_t<W()>(h, m, bases, offsets, n_contigs); });
	if (rc) hipStreamSynchronize(h->stream);
	return rc;
}
int match_add_core(kmr_handle *h, kmr_match *m, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t n_reads, uint64_t first_global,
                   const int64_t *mate, const uint8_t *discarded) {
	const ReadsView rv = reads_view(bases, quals, offsets, n_reads, discarded);      /* first_read_idx 0: the Op adds first_global itself */
	const int rc = with_w(h, [&](auto W) { return match_add_t<W()>(h, m, rv, first_global, mate); });
	if (rc) hipStreamSynchronize(h->stream);
	return rc;
}
int compare_spectrums_core(kmr_handle *h1, kmr_handle *h2, kmr_compare_counts *out) { return with_w(h2, [&](auto W) { return compare_spectrums_t<W()>(h1, h2, out); }); }
int compare_reads_core(kmr_handle *h2, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t n_reads, void *dev_out) {
	const ReadsView rv = reads_view(bases, quals, offsets, n_reads);
	const int rc = with_w(h2, [&](auto W) { return compare_reads_t<W()>(h2, rv, (CompareRec *)dev_out); });
	if (rc) hipStreamSynchronize(h2->stream);
	return rc;
}
}  // namespace kmr_host
