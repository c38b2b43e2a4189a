/*
 * kmernator_amd.h -- C-ABI of the MI355X-native k-mer spectrum builder.
 *
 * This is the drop-in boundary for ONE path of JGI-Bioinformatics/Kmernator:
 * the FilterReads / KmerSpectrum k-mer-spectrum build and lookup.  Every entry
 * point below names the reference interface it replaces (path:line under the
 * reference checkout).  The reference has no FFI of its own -- the boundary is
 * a compile-time C++ template API -- so the C++ shim a maintainer adds on the
 * Kmernator side (a KmerSpectrum<> subclass that calls these functions and
 * restore()s the returned images into the reference's own map types) is shown
 * in INTEGRATION.md and shipped as include/kmernator_amd_shim.hpp.
 *
 * Conventions
 *   - plain C types only; no exceptions cross the boundary.
 *   - every function returns 0 on success or a negative kmr_status; the text
 *     of the last error of a handle is kmr_last_error(h) (thread-unsafe, like
 *     the reference's maps, src/Kmer.h:2269 "bucket ownership" model).
 *   - all in/out buffers are caller owned.  "host" pointers are ordinary
 *     memory; "dev" pointers are HIP device memory of the handle's device.
 *   - k is per handle (the reference keeps it in the process-global KmerSizer,
 *     src/Kmer.h:83-127).
 *   - packed k-mers use the reference byte layout (TwoBitSequence,
 *     src/TwoBitSequence.cpp:242-269): 4 bases per byte, first base in bits
 *     7..6, A=0 C=1 G=2 T=3, kb = ceil(k/4) bytes, pad bits zero.
 *   - there is NO CPU fallback: if the HIP device or the code object is
 *     missing every compute entry point fails with KMR_ERR_NO_DEVICE.
 */
#ifndef KMERNATOR_AMD_H_
#define KMERNATOR_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMR_ABI_VERSION 1

typedef enum kmr_status {
	KMR_OK = 0,
	KMR_ERR_INVALID_ARG = -1,
	KMR_ERR_NO_DEVICE = -2,   /* no HIP device / kernel image not loadable */
	KMR_ERR_HIP = -3,         /* a HIP runtime call failed                  */
	KMR_ERR_OOM = -4,         /* device or host allocation failed           */
	KMR_ERR_STATE = -5,       /* call not valid in the handle's state       */
	KMR_ERR_CAPACITY = -6,    /* a caller supplied buffer is too small      */
	KMR_ERR_UNSUPPORTED = -7  /* option not built (e.g. solid map)          */
} kmr_status;

/* Value type families of the reference's maps (src/KmerTrackingData.h).
 * COUNT_DIR: weak = TrackingDataWithDirection (12 B: u16 count @0, f32
 *            weightedCount @4, u16 directionBias @8; :491-551), singleton =
 *            TrackingDataSingleton (1 B; :613-686).   [FilterReads(-P)]
 * EXT:       weak = ExtensionTrackingData (60 B = the 12 B above + u32
 *            [Left,Right][A,C,G,T,N,X]; :1027-1074), singleton =
 *            ExtensionTrackingDataSingleton (5 B; :1078-1126). [MeraculousCounter] */
typedef enum kmr_value_kind { KMR_VALUE_COUNT_DIR = 0, KMR_VALUE_EXT = 1 } kmr_value_kind;

/* Which of the spectrum's maps (src/KmerSpectrum.h:396-403). */
typedef enum kmr_map { KMR_MAP_WEAK = 0, KMR_MAP_SINGLETON = 1, KMR_MAP_SOLID = 2 } kmr_map;

/* Replaces the option singletons read on this path:
 * KmerSizer::set (src/Kmer.h:107), KmerSpectrumOptions (src/KmerSpectrum.h:92-139),
 * GeneralOptions min-quality-score / fastq-base-quality (src/Options.h:327-331),
 * ExtensionTracking::setMinQuality (src/KmerTrackingData.h:157-163) and the bucket
 * sizing of the KmerSpectrum constructor (src/KmerSpectrum.h:414-421, src/Kmer.h:2837,2224). */
/* Two fields SURVEY section 8(b) sketches are deliberately absent.  num_devices: one handle drives ONE device, as one MPI rank
 * drives one share of the spectrum in the reference (DistributedKmerSpectrum, src/DistributedFunctions.h:126); a node's N GPUs are
 * N handles with rank / world_size set (one process or thread each) joined by kmr_exchange_*.  deterministic: results do not
 * depend on scheduling -- counts, direction biases (global stream ordinals decide the first sighting), singleton bytes and
 * extension tallies are exact and repeatable; only weightedCount's low bits depend on the order of an f64 atomic sum, inside the
 * 1e-5 * count the reference's own OpenMP / MPI builds vary by. */
typedef struct kmr_config {
	uint32_t struct_size;            /* = sizeof(kmr_config), ABI guard                       */
	uint32_t k;                      /* k-mer length in bases, 1..128                          */
	uint64_t num_buckets_weak;       /* 0 => derive from estimated_raw_kmers like the ctor     */
	uint64_t num_buckets_singleton;  /* 0 => derive; both rounded up to a power of two <= 2^26 */
	uint64_t estimated_raw_kmers;    /* KmerSpectrum::estimateRawKmers() of the whole job; with world_size > 1 a
	                                  * rank sizes its maps for estimated_raw_kmers / world_size, as
	                                  * DistributedKmerSpectrum::estimateRawKmers does (src/DistributedFunctions.h:144-162) */
	uint32_t value_kind;             /* kmr_value_kind                                         */
	float    min_weight;             /* --min-kmer-quality (TrackingData::minimumWeight), 0.10 */
	uint32_t min_quality_score;      /* --min-quality-score, 3 (MeraculousCounter: 2)          */
	uint32_t fastq_start_char;       /* Phred base of the quals handed in: 33 or 64            */
	uint32_t ext_min_quality;        /* ExtensionTracking min quality, 20                      */
	uint32_t separate_singletons;    /* 1 = reference default (hasSingletons)                  */
	uint32_t kmer_subsample;         /* --kmer-subsample; keep k-mer iff hash % n == 0; 1=all  */
	int32_t  device;                 /* HIP device ordinal; -1 = current                       */
	uint32_t rank;                   /* owner partition of this handle ...                     */
	uint32_t world_size;             /* ... out of world_size (1 = single partition)           */
	double   estimated_depth;        /* --estimated-depth, 20 (used only to derive buckets)    */
	double   estimated_error_rate;   /* --estimated-error-rate, 0.35 (ditto)                   */
	uint32_t kmers_per_bucket;       /* --kmers-per-bucket, 32 (ditto)                         */
	uint32_t num_parts;              /* --build-partitions: keep k-mers whose                  */
	uint32_t part_idx;               /*   getDMPThread(kmer,num_parts)==part_idx; 0/1 = all    */
	uint32_t build_mode;             /* 0 = auto (3 where it applies, else 2), 1 = open-addressed device table, 2 = two-level
	                                    k-mer partition + LDS counting, 3 = super-k-mer lists: one scatter pass by minimizer,
	                                    expansion + counting in LDS (k >= 13; both value kinds in all three modes) */
	uint64_t max_table_entries;      /* 0 = size from estimated_raw_kmers; else distinct-key
	                                    capacity of the device table                           */
	uint32_t hash_kind;              /* kmr_hash_kind: which hash places a k-mer in its bucket / owner / part / subsample.
	                                    0 = KmerHasher::getHash as it is today: lookup3 hashlittle2 (src/Kmer.h:207-230);
	                                    1 = lookup8 hash() with level 0xDEADBEEF (src/lookup8.h:90-160; what getHash used
	                                    before, src/Kmer.h:210-212 -- the reference no longer calls it).  Images written with
	                                    one kind cannot be loaded into a handle of the other (the bucket of a key differs) */
	uint32_t size_tracker;           /* 1 = keep KmerSpectrum::SizeTracker snapshots (src/KmerSpectrum.h:812-900), see
	                                    kmr_size_tracker below                                                          */
} kmr_config;
enum kmr_hash_kind { KMR_HASH_LOOKUP3 = 0, KMR_HASH_LOOKUP8 = 1 };

typedef struct kmr_handle kmr_handle;

/* Counters of KmerSpectrum (src/KmerSpectrum.h:405-409,455-459) and of
 * TrackingData::discarded (src/KmerTrackingData.h:354-364). */
typedef struct kmr_stats {
	uint64_t raw_kmers;        /* every k-mer occurrence offered to append()                  */
	uint64_t raw_good_kmers;   /* occurrences that passed the weight test                     */
	uint64_t unique_kmers;     /* distinct k-mers ever seen (weak + singleton)                */
	uint64_t singleton_kmers;  /* distinct k-mers seen exactly once                           */
	uint64_t discarded;        /* occurrences with weight <= min_weight                       */
	uint64_t weak_entries;     /* entries now in the weak map (after finalize: after purge)   */
	uint64_t singleton_entries;/* entries now in the singleton map                            */
	uint64_t reads;            /* reads consumed (discarded reads included)                   */
} kmr_stats;

/* Fill *cfg with the reference defaults listed above (k must still be set). */
int kmr_config_init(kmr_config *cfg);

/* Create / destroy.  Replaces KmerSpectrum(estimatedRawKmers, separateSingletons)
 * (src/KmerSpectrum.h:414-421) and DistributedKmerSpectrum(world, ...)
 * (src/DistributedFunctions.h:126-131); the handle owns all device memory. */
int  kmr_create(const kmr_config *cfg, kmr_handle **out);
void kmr_destroy(kmr_handle *h);
const char *kmr_last_error(const kmr_handle *h);   /* h may be NULL: creation errors */

/* Effective bucket counts after power-of-two rounding (BucketExposedMapLogic::
 * resizeBuckets, src/Kmer.h:2224-2236). */
int kmr_num_buckets(const kmr_handle *h, int which_map, uint64_t *out);

/* Feed one batch of reads.  Replaces the per-read body of
 * KmerSpectrum::_buildKmerSpectrumSerial/_Parallel (src/KmerSpectrum.h:1914-2074)
 * = KmerReadUtils::buildWeightedKmers (src/KmerReadUtils.h:176-248) + append()
 * (src/KmerSpectrum.h:1578-1668).  Host buffers:
 *   bases  : ASCII sequence characters of all reads back to back
 *   quals  : ASCII qualities, same layout; NULL = reads without quals
 *            (reference reads, weight 1.0; src/KmerReadUtils.h:195-199)
 *   offsets: n_reads+1 byte offsets into bases/quals (read r = [off[r],off[r+1]))
 *   discarded: optional, 1 = Read::isDiscarded() (skipped)
 * May be called any number of times before kmr_finalize. */
int kmr_add_reads(kmr_handle *h, const char *bases, const char *quals,
                  const uint64_t *offsets, uint64_t n_reads,
                  uint64_t first_global_read_idx, const uint8_t *discarded);

/* Same, but the buffers are already in the handle's device memory (this is
 * the form bench.py times: inputs resident in HBM).  Asynchronous on the
 * handle's stream; kmr_sync() waits. */
int kmr_add_reads_dev(kmr_handle *h, const void *dev_bases, const void *dev_quals,
                      const void *dev_offsets, uint64_t n_reads, uint64_t total_bases,
                      uint64_t first_global_read_idx, const void *dev_discarded);
int kmr_sync(kmr_handle *h);

/* Post-build steps of buildKmerSpectrumInParts / DistributedKmerSpectrum::
 * buildKmerSpectrum: purgeMinDepth(min_depth) (src/KmerSpectrum.h:1805-1815,
 * 1825; src/DistributedFunctions.h:560-569) and optimize() (sorted buckets,
 * src/Kmer.h:3079-3088).  After this call the maps are immutable and
 * queryable / exportable. */
int kmr_finalize(kmr_handle *h, uint32_t min_depth);

/* Position in the whole input of the next base handed to kmr_add_reads* (default: 0 after kmr_create / kmr_reset, then the bases
 * added so far).  The order of occurrences in the input decides which sighting of a k-mer was its first -- the one
 * TrackingDataSingleton keeps without a direction and with a quantised weight (src/KmerTrackingData.h:641-658).  Ranks that each
 * read a slice of one input set their slice's offset here, and the owner-partitioned spectra (kmr_sk_exchange_*) come out as the
 * serial build of the whole input would have them, whatever the ranks' timing. */
int kmr_set_stream_origin(kmr_handle *h, uint64_t ordinal);

/* Empty the maps and counters but keep the device allocations, as
 * KmerSpectrum::buildKmerSpectrum does on entry (weak.reset(false);
 * singleton.reset(false), src/KmerSpectrum.h:2091-2096).  Asynchronous. */
int kmr_reset(kmr_handle *h);
/* Give the build-time hash table back to the device once finalized (the
 * finalized maps stay queryable); kmr_reset() re-allocates it. */
int kmr_release_table(kmr_handle *h);

int kmr_get_stats(kmr_handle *h, kmr_stats *out);

/* KmerSpectrum::subtractReference (src/KmerSpectrum.h:472-474; apps/FilterReads-P.cpp:117): k-mers present in the
 * finalized spectrum `reference` (same k, same device) are skipped by later kmr_add_reads* calls on h before they
 * count as raw k-mers (append(), :1582-1588).  kmr_finalize(h) drops the link as optimize() does; NULL drops it now.
 * kmr_subtracted = the `subtracted` counter. */
int kmr_subtract_reference(kmr_handle *h, kmr_handle *reference);
int kmr_subtracted(kmr_handle *h, uint64_t *out);

/* Lookup.  Replaces KmerMap::getElementIfExists(kmer).value().getCount()
 * (src/Kmer.h:2617-2624; consumer src/ReadSelector.h:924-931) and
 * KmerSpectrum::getCount(kmer,false) (src/KmerSpectrum.h:701-725): weak count
 * if present, else 1 if in the singleton map, else 0.  Keys are packed
 * canonical k-mers, kb bytes each. */
int kmr_lookup(kmr_handle *h, const uint8_t *packed_kmers, uint64_t n, uint32_t *counts);

/* Fused extract + canonicalise + lookup for whole reads: counts_out gets one
 * u32 per k-mer position of each read (read r writes out_offsets[r]..+L-k+1).
 * This is ReadSelector::scoreReadByKmers' inner loop (src/ReadSelector.h:1048-1076). */
int kmr_lookup_reads(kmr_handle *h, const char *bases, const uint64_t *offsets,
                     uint64_t n_reads, uint32_t *counts_out, const uint64_t *out_offsets);

/* KmerSpectrum::getCount(kmer, true) / getCounts(KmerWeights&, true) (src/KmerSpectrum.h:670-680, 701-716; the reference's
 * default, TrackingData::useWeightedByDefault, src/Kmer.cpp:77): weightedCount of the weak entry, else the singleton's
 * (_weight - 1) / 254 (TrackingDataSingleton::getWeightedCount, src/KmerTrackingData.h:657-659), else 0.0.  One f64 per key;
 * the weak value's f32 converts exactly.  Same keys, state rules and error codes as kmr_lookup. */
int kmr_lookup_weighted(kmr_handle *h, const uint8_t *packed_kmers, uint64_t n, double *weights);
/* The same per k-mer position of whole reads: weights_out[out_offsets[r] + i] as kmr_lookup_reads lays out its counts. */
int kmr_lookup_reads_weighted(kmr_handle *h, const char *bases, const uint64_t *offsets, uint64_t n_reads,
                              double *weights_out, const uint64_t *out_offsets);

/* Trim and score whole reads against the weak map: ReadSelector::scoreAndTrimReads
 * (src/ReadSelector.h:1182-1207) = per-position counts (getValue :924-931, weak map only), cut at the first
 * N/X markup (_setNumKmers :1037-1047), first longest run of k-mers with count >= minimum_kmer_score
 * (trimReadByMinimumKmerScore :949-1014; its bimodal cut: kmr_set_bimodal_sigmas below), score of that run (scoreReadByScoringType
 * :1094-1180) and setTrimHeaders (:1015-1036).  Per read: trim_offset (bases), trim_length (bases, run + k - 1,
 * 0 = nothing left), score (-1 if nothing left; KS_SUM leaves 0 as the reference does), was_trimmed.
 * A markup other than N, X and '.' (an IUPAC code, a lower-case n) does not cut: the reference looks the k-mers that hold it up
 * with the 'A' compressSequence stores in its place (src/TwoBitSequence.cpp:253-260, getKmersForRead src/ReadSelector.h:413-415).
 * The per-k-mer probes do that; the streaming pass answers zero for such a k-mer, so kmr_score_reads, kmr_score_read_batch and
 * kmr_filter_read_batch* first scan the batch's bases (one pass and one host wait per call) and probe the WHOLE batch if a single
 * such base is in it: slower by the difference of the two lookup paths, which has not been measured for such batches.
 * kmr_build_info "score_path" tells which path the last call took.  kmr_lookup_requests_dev leaves such k-mers unasked (zero). */
typedef enum kmr_scoring { KMR_SCORE_SUM = 0, KMR_SCORE_MEDIAN = 1, KMR_SCORE_MIN = 2, KMR_SCORE_MAX = 3, KMR_SCORE_AVG = 4 } kmr_scoring;
int kmr_score_reads(kmr_handle *h, const char *bases, const uint64_t *offsets, uint64_t n_reads,
                    double minimum_kmer_score, int scoring_type,
                    uint32_t *trim_offset, uint32_t *trim_length, float *score, uint8_t *was_trimmed);
/* --bimodal-sigmas (ReadSelector::_bimodalSigmas; the default of kmr_create is -1, off), for every scoring call of the handle:
 * kmr_score_reads, kmr_score_read_batch, kmr_score_counts_dev and the fused kmr_filter_ / kmr_partition_ / kmr_normalize_read_batch*.
 * With sigmas >= 0 a run of n >= 3 k-mers is searched for the split p in 1 .. n-1 whose halves first = v[0..p), second = v[p..n)
 * differ most in mean depth (src/ReadSelector.h:981-1008, Statistics::findBimodalPartition src/Utils.h:1031-1056):
 *   mean     the f64 sum in index order, divided by the count where the count is above 1
 *   stdDev   the VARIANCE (the reference never takes its root): f64 sum of (x - mean) * (x - mean) in index order over count - 1,
 *            0 for one value; raised to sqrt(mean) where mean > 0 and it is below that (the Poisson floor)
 *   diff     abs(first.mean - second.mean), where abs is C's int abs(int): the unqualified call on a double resolves to it with
 *            the reference's includes (<cstdlib>, <cmath>, no using-directive), so the difference is TRUNCATED toward zero to an
 *            int first (2.9 - 0.2 gives 2).  That reading is this library's contract
 *   a split qualifies if diff > sigmas * max(first.stdDev, second.stdDev); the qualifying split of the strictly largest diff wins,
 *   so of equal diffs the earliest p.
 * first.mean > second.mean drops the tail (run length p), otherwise the head (offset + p, length n - p); was_trimmed is set and
 * the score is that of the reduced run.  The record's label gains "Bimodal@<p + k>:<(int)first.mean>/<(int)second.mean>", with
 * "Inv" in front where the head was dropped, between AFTrim and Trim.  With sigmas < 0 nothing is added to a scoring call: no
 * kernel, no allocation, no wait.  NaN: KMR_ERR_INVALID_ARG. */
int kmr_set_bimodal_sigmas(kmr_handle *h, double sigmas);
/* One word per read of the handle's last scoring call: 0 = not cut, else p + k in bits 0-31, (int)first.mean in bits 32-47,
 * (int)second.mean in bits 48-63 (Inv where the first is the smaller).  All zero if that call ran with the option off.
 * KMR_ERR_STATE: no scoring call yet; KMR_ERR_INVALID_ARG: n_reads is not that call's. */
int kmr_bimodal_copy(kmr_handle *h, uint64_t *words, uint64_t n_reads);

/* Export in the reference's on-disk / mmap format so the caller can
 * WeakMapType::restore(dst) it.  Replaces KmerMapByKmerArrayPair::getSizeToStore /
 * store(void*) (src/Kmer.h:3143-3159,3181-3191) and KmerSpectrum::storeMmap
 * (src/KmerSpectrum.h:476-488).  Layout: u64 numBuckets; u64 bucketMask;
 * u64 offset[numBuckets]; then per bucket {u32 n; u8 keys[n][kb]; V values[n]}
 * with keys sorted by memcmp. */
int kmr_image_size(kmr_handle *h, int which_map, uint64_t *bytes);
int kmr_write_image(kmr_handle *h, int which_map, void *dst, uint64_t capacity);

/* Restore: replaces KmerSpectrum::restoreMmap / KmerMapByKmerArrayPair(const void*)
 * (src/KmerSpectrum.h:489-518, src/Kmer.h:3124-3135).  The handle must be fresh
 * (no reads added); it becomes finalized. */
int kmr_load_image(kmr_handle *h, int which_map, const void *src, uint64_t len);
/* KmerMapByKmerArrayPair::mergeAdd (src/Kmer.h:3209-3261) of a stored map into the handle's finalized map of the same kind and
 * bucket count: the restore-and-merge loop of KmerSpectrum::buildKmerSpectrumInParts (src/KmerSpectrum.h:1871-1884; parts built
 * with kmr_config.num_parts / part_idx hold disjoint k-mers) and the weak-map step of KmerSpectrum::mergeVector (:2572-2584): a
 * k-mer both weak maps hold gets a.add(b) -- += on the u16 count and directionBias (as in the reference they wrap, nothing
 * saturates), on the float weightedCount and on the u32 extension tallies (src/KmerTrackingData.h:489-493,538-542,1059-1064).
 * Singleton maps that share a k-mer are refused with KMR_ERR_UNSUPPORTED: that k-mer would have to be promoted into the weak map,
 * KmerMap::mergePromote, which the reference itself throws on (src/Kmer.h:2675-2677). */
int kmr_merge_image(kmr_handle *h, int which_map, const void *src, uint64_t len);

/* Order-independent digest of a finalized map: a spectrum of 10^9 entries is compared, and the rank / part maps of a partitioned
 * build are added up, without moving the maps (the reference compares maps entry by entry on the host, e.g. the store / restore
 * check of test/KmerTest.cpp:545-594; nothing of the kind exists there for a whole spectrum).  Per entry
 *   e = mix(..mix(mix(v0 ^ w[0]) ^ w[1])..)  over the key's 8-byte big-endian words (the packed canonical k-mer, zero padded),
 *   mix(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31
 *   weak map:      v0 = count | directionBias << 16; extension values then fold their 12 u32 tallies in pairs (lo | hi << 32)
 *   singleton map: v0 = 1 << 32 | _weight | packet << 40
 * hash_sum / hash_xor are the sum (mod 2^64) and the xor of e over all entries, count_sum / dir_sum the plain sums;
 * weighted_sum adds weightedCount (singleton map: (_weight - 1) / 254) in double -- its last bits depend on the order of addition,
 * as the reference's own float accumulation does (src/KmerTrackingData.h:427-448). */
typedef struct kmr_digest {
	uint64_t entries, count_sum, dir_sum, hash_sum, hash_xor;
	double weighted_sum;
} kmr_digest;
int kmr_map_digest(kmr_handle *h, int which_map, kmr_digest *out);

/* The synthetic reads of SURVEY.md section 8(d) (what bench.py times and the full-size parity tests build), generated on the
 * current device into caller-owned device buffers: reads first_read .. first_read + n_reads (global indices: a rank's share of a
 * job is a range) of read_len bases over a uniform random genome of genome_len bases, random strand, 1 % substitutions, no N;
 * Phred-33 qualities, all 'I' or (noisy_quals) Q 40/30/20/10/2 with probabilities .80/.10/.05/.04/.01 and Q10 on errors.
 * Integer arithmetic only (xorshift64*, defined in kmernator_amd/csrc/kmr_synth.hpp), so the CPU restatement of the tests gives
 * the same bytes.  dev_bases / dev_quals: n_reads * read_len bytes (dev_quals may be NULL); dev_offsets: n_reads + 1 entries or
 * NULL.  Runs on the null stream and returns when the bytes are there.  The reference has no generator; its inputs are files. */
int kmr_synth_reads_dev(uint64_t seed, uint64_t first_read, uint64_t n_reads, uint32_t read_len, uint64_t genome_len, uint32_t noisy_quals,
                        void *dev_bases, void *dev_quals, uint64_t *dev_offsets);

/* Histogram of weak counts (KmerSpectrum::Histogram, src/KmerSpectrum.h:909-1057):
 * counts[c] = number of weak entries with count == c for c < n_bins-1, last bin
 * collects the rest; weights[c] = sum of weightedCount (may be NULL). */
int kmr_count_histogram(kmr_handle *h, uint64_t *counts, double *weights, uint32_t n_bins);
/* KmerSpectrum::Histogram(zoom_max, log_base).set(spectrum) (src/KmerSpectrum.h:909-1057; getHistogram uses
 * Histogram(256), :1066-1071): per bucket visits, visitedCount and visitedWeight over the weak map and, when it
 * is kept, the singleton map.  Bucket of a count: count <= zoom_max ? count : log(count)/log(log_base) -
 * zoomLogSkip + zoom_max (:936-938).  The arrays need kmr_histogram_bins(zoom_max) = 65538 + zoom_max entries. */
uint32_t kmr_histogram_bins(uint32_t zoom_max);
int kmr_histogram(kmr_handle *h, uint32_t zoom_max, double log_base, uint64_t *visits,
                  uint64_t *visited_count, double *visited_weight, uint32_t n_bins);

/* MeraculousDistributedKmerSpectrum::dumpCounts / dumpGraphs
 * (src/Meraculous.h:107-134): text lines for every weak entry with
 * count >= min_depth, both orientations.  Appends to the file at 'path'. */
int kmr_dump_mercount(kmr_handle *h, const char *path, uint32_t min_depth);
int kmr_dump_mergraph(kmr_handle *h, const char *path, uint32_t min_depth);
/* The two write their file in pieces: the text of a run of entries is made on the device (kmr_dump_text), copied to the host
 * and appended.  A piece's run is sized so that its text stays under this staging bound whatever its numbers are (kmr_tune
 * "dump_piece_bytes" overrides it). */
#define KMR_DUMP_PIECE_BYTES (256ull << 20)

/* The same text in device memory (src/Meraculous.h:107-134: dumpCounts :107-120 writes "<k-mer>\t<count>\n" for the k-mer and
 * for its reverse complement, dumpGraphs :121-133 "<k-mer>\t<ExtensionTracking::toTextValues>\n" = twelve tallies with a blank
 * behind each, then "0", the reverse line with ExtensionTracking::getReverseComplement, src/KmerTrackingData.h:219-226) for
 * the weak entries [entry_lo, entry_hi) in map order (bucket by bucket, sorted inside a bucket: the reference's iteration
 * order) whose count passes (int)count >= (int)min_depth.  entry_hi is clamped to the weak map's entry count (UINT64_MAX = to
 * the end); entry_lo > entry_hi after that is KMR_ERR_INVALID_ARG.  The texts of consecutive ranges that partition [0, n)
 * concatenate to the text of the whole map: a caller streams a file larger than it wants to stage that way, and every rank of
 * a distributed build dumps its own entries (each rank of the reference writes its own part, DistributedOfstreamMap :108, :122).
 * KMR_ERR_STATE before kmr_finalize and for KMR_DUMP_MERGRAPH without KMR_VALUE_EXT; KMR_ERR_INVALID_ARG for a NULL handle or
 * output pointer and for an unknown kind.  An empty map, an empty range and a range without a kept entry are valid and give
 * 0 bytes.  Byte offsets are 64-bit: the size of a text is bounded by device memory alone. */
enum kmr_dump_kind { KMR_DUMP_MERCOUNT = 0, KMR_DUMP_MERGRAPH = 1 };
typedef struct kmr_text kmr_text;
/* size only: kept entries and bytes of the text */
int kmr_dump_text_size(kmr_handle *h, int kind, uint32_t min_depth, uint64_t entry_lo, uint64_t entry_hi,
                       uint64_t *kept, uint64_t *bytes);
/* the text itself, in device memory */
int kmr_dump_text(kmr_handle *h, int kind, uint32_t min_depth, uint64_t entry_lo, uint64_t entry_hi, kmr_text **out);
int kmr_text_info(const kmr_text *t, uint64_t *kept, uint64_t *bytes);      /* either may be NULL */
/* the text to host memory (KMR_ERR_CAPACITY if capacity < bytes) */
int kmr_text_copy(const kmr_text *t, char *dst, uint64_t capacity);
/* the text where it lies (for a compressor or a device-aware MPI-IO); valid until kmr_text_free */
int kmr_text_device_ptr(const kmr_text *t, void **dev_text);
void kmr_text_free(kmr_text *t);

/* ---- stateless helpers (bit-identical to the reference functions) -------- */

/* KmerHasher::getHash (src/Kmer.h:207-230) = Lookup3::hashlittle2
 * (src/lookup3.h:470-641) with pc=0xDEADBEEF, pb=0, result c | b<<32. */
uint64_t kmr_hash(const uint8_t *key, uint32_t len);
uint64_t kmr_hash_of_kind(const uint8_t *key, uint32_t len, uint32_t hash_kind);      /* the same for either hash kind, len <= 32 */
/* BucketExposedMapLogic::getBucketIdx / getLocalThreadId / getDistributedThreadId
 * (src/Kmer.h:2329-2333, 2269-2280, 2284-2295). */
uint64_t kmr_bucket_idx(uint64_t hash, uint64_t num_buckets_pow2);
uint32_t kmr_local_thread_id(uint64_t hash, uint64_t num_buckets_pow2, uint32_t num_threads);
uint32_t kmr_distributed_thread_id(uint64_t hash, uint32_t world_size);
/* TwoBitSequence::compressSequence (src/TwoBitSequence.cpp:242-269); returns
 * the number of markups (non-ACGT bases), written to markup_pos/markup_char
 * up to markup_cap. */
int64_t kmr_compress_sequence(const char *bases, uint64_t len, uint8_t *out,
                              uint32_t *markup_pos, char *markup_char, uint64_t markup_cap);
/* Kmer::buildLeastComplement (src/Kmer.h:356-364): writes the canonical form
 * of a packed k-mer, returns 1 if the input was already the least. */
int kmr_least_complement(const uint8_t *packed, uint32_t k, uint8_t *out);

/* ---- device-level pieces for one-process-per-GPU owner partitioning ------
 * These replace the body of DistributedKmerSpectrum::_buildKmerSpectrumMPI
 * (src/DistributedFunctions.h:340-458): sender side = buildWeightedKmers +
 * isDiscard + getThreadIds (:418-433) + bufferMessage (:438); the
 * MPI_Alltoallv (src/MPIBuffer.h:588-600) is done by the caller (RCCL
 * all-to-all over xGMI via torch.distributed); receiver side =
 * StoreKmerMessageHeaderProcessor::process -> append (:323-328).
 *
 * A record is KMR_RECORD_BYTES(k, value_kind) bytes, 4-byte aligned: the u64 key words (big-endian packed
 * k-mer, zero padded; each word as two little-endian u32, low half first), an f32 signed weight (negative =
 * observed strand was the reverse complement, as StoreKmerMessageHeader::weight :279) and, for
 * KMR_VALUE_EXT only, the u32 extension packet (leftBase,rightBase chars, leftQ,rightQ;
 * ExtensionMessagePacket, src/KmerTrackingData.h:232-288).  12 bytes per k-mer at k <= 32 against the
 * reference's 24 + kb byte message (src/DistributedFunctions.h:274-303). */
#define KMR_KEY_WORDS(k) ((((k) + 3u) / 4u + 7u) / 8u)
#define KMR_RECORD_BYTES(k, value_kind) (8u * KMR_KEY_WORDS(k) + ((value_kind) == KMR_VALUE_EXT ? 8u : 4u))

/* Extract all good k-mers of a device-resident read batch and bin them by
 * owner = kmr_distributed_thread_id(hash, world_size) into world_size
 * contiguous segments of dev_records; segment s starts at record seg_capacity * s.
 * dev_seg_counts[world_size] (u64, device) receives the number of records per owner.
 * Returns KMR_ERR_CAPACITY (after sync) if a segment overflowed.  Asynchronous on the
 * handle's stream otherwise. */
int kmr_extract_by_owner_dev(kmr_handle *h, const void *dev_bases, const void *dev_quals,
                             const void *dev_offsets, uint64_t n_reads, uint64_t total_bases,
                             uint64_t first_global_read_idx, const void *dev_discarded,
                             void *dev_records, uint64_t seg_capacity, void *dev_seg_counts);
/* Insert n records (any owner mix that belongs to this handle) into the table. */
int kmr_insert_records_dev(kmr_handle *h, const void *dev_records, uint64_t n_records);

/* The same exchange for build_mode 3 (super-k-mer lists), whose unit is not the k-mer but the list: every rank scatters the
 * super-k-mers of ITS reads (kmr_add_reads* after kmr_sk_exchange_begin: nothing is filtered by owner; without that call a
 * handle with world_size > 1 keeps what getDistributedThreadId gives its rank, as in the other build modes, and has nothing to
 * exchange) into the job's 2^list_bits lists, list l belongs to
 * rank l % world_size, and what a rank holds of other ranks' lists travels as it lies: ~4 bytes per k-mer on the wire instead of
 * the reference's 24 + kb (src/DistributedFunctions.h:274-303).  The owner of a k-mer is decided by its minimizer (private to
 * the build), not by getDistributedThreadId: per-rank spectra are a different partition of the same k-mers, their union is
 * the same spectrum.
 *   kmr_sk_exchange_begin     the handle's reads are meant for the exchange (sticky; before the first kmr_add_reads*)
 *   kmr_sk_exchange_counts    closes the lists; chunks[r], granules[r] (host, [world_size]) = what this rank holds for owner r
 *                             (16-byte granules; r == rank: what stays)
 *   kmr_sk_exchange_pack_dev  the chunks of the other owners -> dev_data (owner r's granules from granule_offset[r] on, 16 bytes
 *                             each) and dev_meta (its (list, granules) pairs, u32 x 2, from chunk_offset[r] on); they leave the pool
 *   (the caller moves data and meta to their owners: all-to-all over RCCL / MPI)
 *   kmr_sk_exchange_adopt_dev the received chunks (any order) are appended to this rank's own lists
 * then kmr_finalize as usual.  All three synchronise. */
int kmr_sk_exchange_begin(kmr_handle *h);      /* before the first reads of the handle */
int kmr_sk_exchange_counts(kmr_handle *h, uint64_t *chunks, uint64_t *granules);
int kmr_sk_exchange_pack_dev(kmr_handle *h, void *dev_data, void *dev_meta, const uint64_t *granule_offset, const uint64_t *chunk_offset);
int kmr_sk_exchange_adopt_dev(kmr_handle *h, const void *dev_data, const void *dev_meta, uint64_t n_chunks, uint64_t n_granules);
/* Do all records of this rank's lists carry ONE weight (every call so far took the bases-only extraction with the same quality
 * character)?  *state = kind << 32 | weight bits; kind 0: no record yet, 1: one weight, 2: several.  A sender hands its state to the
 * owners along with its chunk counts, an owner folds it in with kmr_sk_exchange_peer_uniform BEFORE adopting that sender's chunks: if all
 * agree, kmr_finalize counts with the one-weight form of the count pass.  A declaration covers the NEXT kmr_sk_exchange_adopt_dev only
 * (that call clears it, and so does kmr_reset): declare, before each adopt, for every sender whose chunks it carries.  An adopt that
 * nobody declared for checks the received records itself (a pass over every received header).  Nothing in the reference corresponds (its wire records carry a weight per k-mer,
 * src/DistributedFunctions.h:274-303). */
int kmr_sk_exchange_uniform(kmr_handle *h, uint64_t *state);
int kmr_sk_exchange_peer_uniform(kmr_handle *h, uint64_t state);
/* An exchange in steps over the list space, so that an owner can count what has arrived while the rest is on the wire:
 * kmr_sk_exchange_range restricts the next kmr_sk_exchange_counts / kmr_sk_exchange_pack_dev to the lists in [list_lo, list_hi)
 * (0, ~0: all of them, the default; kmr_reset restores it); kmr_count_lists_prefix runs the count pass over this handle's lists below
 * list_hi NOW -- asynchronously on the handle's stream, into entry buffers of their own -- once everything those lists will ever get
 * has been adopted; kmr_finalize (same min_depth) then counts the lists from list_hi on and takes the early entries over.  The
 * result is that of kmr_finalize alone.  What cannot be counted early (extension values, a kept singleton map, the size tracker,
 * coarse lists, early buffers that turn out too small) is quietly left to kmr_finalize.  The early pass has an error word of its
 * own: an overflow of its buffers fails no call (not the next adopt, not a second kmr_count_lists_prefix, which replaces the early
 * count and its flag, not kmr_finalize); kmr_finalize voids that early count and counts every list itself (kmr_build_info
 * "early_overflowed"; kmr_tune "early_entry_share" sizes the buffers).  The reference's MPI build has no such
 * phase: its owners insert k-mers as messages arrive (src/DistributedFunctions.h:323-328) and purge at the end. */
int kmr_sk_exchange_range(kmr_handle *h, uint64_t list_lo, uint64_t list_hi);
int kmr_count_lists_prefix(kmr_handle *h, uint32_t min_depth, uint64_t list_hi);

/* KmerSpectrum::SizeTracker (src/KmerSpectrum.h:812-900): the history of (rawKmers, rawGoodKmers, uniqueKmers, singletonKmers) the
 * apps write as --size-history-file (apps/FilterReads.cpp:141-147) and EstimateSize fits.  The reference calls track() before every
 * k-mer it appends (trackSpectrum, :1574-1581: thread 0 only, so its parallel builds record an arbitrary subset); here the same
 * rule -- an element whenever rawKmers has reached nextToTrack (128, then x 1.05 truncated to long) -- is applied after every READ,
 * in input order: element i holds the four counters as they stand after the first read that brings rawKmers to the i-th threshold
 * (counters of a serial build of exactly the reads up to there; what differs from the reference's serial history is only where
 * inside a read the sample is taken).  Needs kmr_config.size_tracker = 1 (kept by the super-k-mer build of a single partition;
 * kmr_create refuses other combinations) and a finalized handle.  elements: [capacity][4] u64, may be NULL to ask for the count;
 * force_last = 1 appends the element trackSpectrum(true) adds after the build.  With kmer_subsample > 1 the stored values are
 * scaled as track() does (:882-887). */
int kmr_size_tracker(kmr_handle *h, int force_last, uint64_t *elements, uint64_t capacity, uint64_t *n_elements);

/* The whole exchange inside the library, RCCL called directly (librccl is dlopen'ed on first use: no link-time dependency): what a
 * C / C++ host -- one process or thread per GPU of a node, no MPI, no Python -- calls instead of
 * DistributedKmerSpectrum::_buildKmerSpectrumMPI (src/DistributedFunctions.h:340-458; the MPI_Alltoallv of src/MPIBuffer.h:588-600
 * becomes grouped ncclSend / ncclRecv over xGMI, one message of <= 1 GiB per peer and slice; the local share never moves).
 *   kmr_exchange_unique_id      rank 0 makes the job's id; the host hands the KMR_EXCHANGE_ID_BYTES to every rank (file, pipe, socket)
 *   kmr_exchange_init           collective: ncclCommInitRank(cfg.world_size, id, cfg.rank) on the handle's device (or
 *                               kmr_exchange_init_transport below: the host's own collectives).  A build_mode 0
 *                               handle that can build super-k-mer lists moves to them here (build_mode 3 semantics, see above)
 *   kmr_exchange_add_reads_dev  collective, one batch of THIS rank's reads (device pointers as kmr_add_reads_dev; n_reads may be 0):
 *                               build_mode 3: global stream ordinals (an all-gather of the batch sizes), extract into the job's
 *                               lists, counts, chunks of other owners out, received chunks appended; other modes: the batch's
 *                               k-mer records binned by getDistributedThreadId (segments grown and re-extracted if one owner takes
 *                               more than its share), counts, records out, kmr_insert_records_dev of what arrived
 *   kmr_exchange_stats          bytes sent to other ranks and the time of the all-to-alls (HIP events on the handle's stream)
 * then kmr_finalize on every rank.  kmr_destroy frees the communicator.  Every rank must make the same sequence of calls. */
#define KMR_EXCHANGE_ID_BYTES 128
struct kmr_reads;      /* a device-resident read batch, see "FASTQ ingest" below */
int kmr_exchange_unique_id(void *id);
int kmr_exchange_init(kmr_handle *h, const void *id);
/* The same driver over the host's own collectives instead of RCCL (an MPI job: MPI_Allgather and a device-aware MPI_Alltoallv, or one
 * staged through host memory; the tests plug in gloo).  Both are collective and return 0 or a KMR_ERR_* code.
 *   allgather_u64   every rank contributes n values (host memory); all[r * n + j] = value j of rank r
 *   alltoallv_dev   DEVICE buffers: send_bytes[r] bytes at send + send_off[r] go to rank r, recv_bytes[r] bytes from rank r land at
 *                   recv + recv_off[r]; the entries of the calling rank are 0; hip_stream = the handle's stream (the buffers were
 *                   written on it; the call returns when the received bytes are visible to it).  No message exceeds 1 GiB. */
typedef struct kmr_transport {
	void *user;
	int (*allgather_u64)(void *user, const uint64_t *mine, uint64_t n, uint64_t *all);
	int (*alltoallv_dev)(void *user, const void *send, const uint64_t *send_off, const uint64_t *send_bytes,
	                     void *recv, const uint64_t *recv_off, const uint64_t *recv_bytes, void *hip_stream);
} kmr_transport;
int kmr_exchange_init_transport(kmr_handle *h, const kmr_transport *t);
int kmr_exchange_add_reads_dev(kmr_handle *h, const void *dev_bases, const void *dev_quals, const void *dev_offsets, uint64_t n_reads,
                               uint64_t total_bases, uint64_t first_global_read_idx, const void *dev_discarded);
int kmr_exchange_add_read_batch(kmr_handle *h, const struct kmr_reads *batch, uint64_t first_global_read_idx);      /* the same for a device-resident read batch ("FASTQ ingest" below); NULL = no reads this round */
int kmr_exchange_stats(kmr_handle *h, uint64_t *bytes_to_peers, double *alltoall_ms);

/* For a kmr_transport that stages the device segments through host memory (an MPI without device pointers; the -P shim's
 * TRANSPORT_MPI): copies between host memory and the device buffers alltoallv_dev is handed, ordered behind the handle's stream. */
int kmr_copy_to_host(kmr_handle *h, void *host_dst, const void *dev_src, uint64_t bytes);
int kmr_copy_to_device(kmr_handle *h, void *dev_dst, const void *host_src, uint64_t bytes);

/* Host-buffer forms of the two halves for a host whose exchange is MPI_Alltoallv over host memory (the reference's own,
 * src/MPIBuffer.h:588-600; include/kmernator_amd_shim.hpp, GpuDistributedKmerSpectrum).  kmr_extract_by_owner_host: the records
 * of a device-resident batch, owner after owner without gaps; seg_counts[world_size] always receives the counts, and with
 * records == NULL that is all the call does (the segments wait on the device for the call that fetches them). */
struct kmr_reads;      /* a device-resident read batch, see "FASTQ ingest" below */
int kmr_extract_by_owner_host(kmr_handle *h, const struct kmr_reads *batch, uint64_t first_global_read_idx,
                              uint64_t *seg_counts, void *records, uint64_t capacity_bytes);
int kmr_insert_records(kmr_handle *h, const void *host_records, uint64_t n_records);

/* ---- f1, distributed form: scoreAndTrimReads when the spectrum is partitioned by owner --------
 * DistributedReadSelector::scoreAndTrimReads / _batchKmerLookup (src/DistributedFunctions.h:876-1045): every k-mer of a
 * rank's reads is looked up at its owner (request = requestId + k-mer, response = requestId + score over
 * MPI_Alltoallv).  Here a request is the key alone (8 * KMR_KEY_WORDS(k) bytes: the u64 key words, most significant
 * first) and a response a u32 count: the answers come back in request order, so the requester keeps the position of
 * each request instead of sending an id.
 *
 * kmr_lookup_requests_dev: every k-mer without markup of a device-resident read batch, binned by owner into world_size
 * segments of dev_keys (segment s starts at key seg_capacity * s); dev_pos[seg_capacity * s + j] (u32) = position of
 * request j's first base in dev_bases (offsets[r] + i; < 2^32), dev_seg_counts[world_size] (u64) the exact counts.
 * kmr_lookup_keys_dev: owner side, weak-map count of n received keys (ReadSelector::getValue, src/ReadSelector.h:924-931).
 * kmr_scatter_counts_dev: position_counts[pos[j]] = counts[j] for the answers of one owner segment.
 * kmr_score_counts_dev: trimReadByMinimumKmerScore + scoring + setTrimHeaders (as kmr_score_reads) from counts indexed
 * by base position (u32 position_counts[total_bases], zero where no answer was written); dev_bases 16-byte aligned and
 * padded by 64 bytes as for kmr_add_reads_dev.  Every count must be <= 65535, as every answer of kmr_lookup_keys_dev is (the
 * count saturates there): where a group of reads fits, the kernel keeps its counts as 16-bit values.
 * All asynchronous on the handle's stream except kmr_score_counts_dev, which returns host arrays. */
int kmr_lookup_requests_dev(kmr_handle *h, const void *dev_bases, const void *dev_offsets, uint64_t n_reads, uint64_t total_bases,
                            void *dev_keys, void *dev_pos, uint64_t seg_capacity, void *dev_seg_counts);
int kmr_lookup_keys_dev(kmr_handle *h, const void *dev_keys, uint64_t n, void *dev_counts);
/* kmr_lookup_keys_weighted_dev: n keys in the form of kmr_lookup_keys_dev answered as KmerSpectrum::getCount(kmer, true)
 * (src/KmerSpectrum.h:670-680, as kmr_lookup_weighted): f64 dev_weights[n].  Unlike kmr_lookup_keys_dev, which reads the weak map
 * only (ReadSelector::getValue), it consults the weak map AND the singleton map.  Asynchronous on the handle's stream. */
int kmr_lookup_keys_weighted_dev(kmr_handle *h, const void *dev_keys, uint64_t n, void *dev_weights);
int kmr_scatter_counts_dev(kmr_handle *h, const void *dev_counts, const void *dev_pos, uint64_t n, void *dev_position_counts);
int kmr_score_counts_dev(kmr_handle *h, const void *dev_bases, const void *dev_offsets, uint64_t n_reads, const void *dev_position_counts,
                         double minimum_kmer_score, int scoring_type, uint32_t *trim_offset, uint32_t *trim_length,
                         float *score, uint8_t *was_trimmed);

/* ---- f2: FASTQ ingest on the device -------------------------------------
 * Parses a whole in-memory FASTQ block into a device-resident read batch:
 * FastqStreamParser::readRecord (src/ReadFileReader.h:768-835) + ReadFileReader::nextRead
 * (:296-329: Casava-1.8 failed-filter reads are dropped, bases upper-cased, #bases == #quals)
 * + ReadSet::appendFasta/addRead/validateFastqStart (src/ReadSet.cpp:136-141,311-345,
 * src/ReadSet.h:171-209): qualities are rescaled from input_quality_base (33, 64, or 0 = the
 * handle's fastq_start_char; --fastq-base-quality) to the handle's fastq_start_char, and a read
 * among the first 19 999 whose minimum quality lies outside [start, start+40] flips the input base
 * once for the whole batch, as __setFastqStart does.  store_comment = GlobalOptions::isCommentStored()
 * (the reference's default is 1).  Malformed input (what makes the reference throw, plus non-'@' junk
 * between records, which the reference skips) returns KMR_ERR_INVALID_ARG. */
typedef struct kmr_reads kmr_reads;
int kmr_ingest_fastq(kmr_handle *h, const char *text, uint64_t len, uint32_t input_quality_base,
                     int store_comment, kmr_reads **out);
int kmr_ingest_fastq_dev(kmr_handle *h, const void *dev_text, uint64_t len, uint32_t input_quality_base,
                         int store_comment, kmr_reads **out);
/* ---- FASTA and FASTA+QUAL ingest on the device --------------------------
 * The '>' side of ReadSet::appendAnyFile (src/ReadFileReader.h:205-231): FastaStreamParser and, with a qual text, FastaQualStreamParser
 * (:844-1006) over a whole in-memory text, into the same kind of batch as kmr_ingest_fastq gives -- FASTA reads, the 454 pair of
 * reads.fasta + reads.qual, genomes and contigs for kmr_subtract_reference.  qual_text == NULL: every base gets Read::REF_QUAL (127),
 * which kmr_add_read_batch weighs as 1.0.  Otherwise record i of the qual text belongs to record i of the FASTA (same trimmed name), a
 * number v becomes the character min(v, 127 - start - 1) + start (convertQualIntsToChars, src/Utils.h:652-667; start = the handle's
 * fastq_start_char), and validateFastqStart runs as for FASTQ: kmr_reads_info reports the other base if the batch was shifted.
 *
 * A record is a '>' line followed directly by one or more non-empty lines; its bases are those lines concatenated and upper-cased.
 * Lines end at '\n' (the last may lack it; '\r' is content); empty lines may stand between a record and the next header and at the
 * end.  Name, comment and the Casava-1.8 filter apply to the header as to the '@' line of FASTQ; name_off/name_len of kmr_reads_copy
 * span the header behind '>' in `text`.  Everything accepted is parsed as the reference parses it; what its stream and mmap forms
 * disagree on or mangle returns KMR_ERR_INVALID_ARG with the cause in kmr_last_error: text or an empty line before the first
 * header, a header followed by a header or at the end of the text, an empty line before or between sequence lines, an empty name;
 * in the qual text also a byte other than digit, blank and tab, more than 3 digits, a line ending in a digit where the next of the
 * record starts with one (the reference joins them into one number), and a different record count, name or number of qualities.
 * A record of more than 2^32 - 2 bases returns KMR_ERR_UNSUPPORTED.  An empty text is an empty batch.
 *
 * The host form copies the texts to the device; the _dev form reads the caller's device memory in place, at any alignment, and
 * touches no byte outside [text, text + len) and [qual_text, qual_text + qual_len).  A record is spread over the whole device
 * whether it is one line of 100 Mbp or 60-column lines.  The call's scratch (about 36 bytes per line and 20 per record, 44 and 8 for the
 * qual text) stays with the handle, grow-only, until kmr_destroy.
 *
 * Not covered: an input quality base that differs from the start character (the reference then rescales REF_QUAL itself,
 * src/ReadSet.cpp:324,336: there is no quality-base argument); gz / bgzf input; multi-line FASTQ; the reference's skip of up to
 * 100 000 junk lines between records.  kmr_reads_twobit stays one thread per read (slow for a genome), and
 * kmr_artifact_filter_create keeps its own host-side FASTA parse. */
int kmr_ingest_fasta(kmr_handle *h, const char *text, uint64_t len, const char *qual_text, uint64_t qual_len,
                     int store_comment, kmr_reads **out);
int kmr_ingest_fasta_dev(kmr_handle *h, const void *dev_text, uint64_t len, const void *dev_qual_text, uint64_t qual_len,
                         int store_comment, kmr_reads **out);
/* n_filtered = records dropped by the Casava filter; input_quality_base = the base after detection */
int kmr_reads_info(const kmr_reads *r, uint64_t *n_reads, uint64_t *total_bases,
                   uint32_t *input_quality_base, uint64_t *n_filtered);
/* the same kind of batch from reads the host has already parsed (arrays as for kmr_add_reads, qualities scaled to the
 * handle's fastq_start_char); names are empty */
int kmr_reads_from_host(kmr_handle *h, const char *bases, const char *quals, const uint64_t *offsets, uint64_t n_reads,
                        kmr_reads **out);
/* ... and from reads the host keeps as the reference's Read does (arrays as for kmr_add_reads_twobit below: 2-bit packed bases, markups,
 * qualities as characters / one character for all / none = Read::REF_QUAL): a quarter of the base bytes on the bus */
int kmr_reads_from_twobit(kmr_handle *h, const uint8_t *twobit, const uint64_t *twobit_offsets, const uint64_t *offsets,
                          const uint64_t *markup_offsets, const uint32_t *markup_pos, const char *markup_char,
                          const char *quals, int uniform_quality, uint64_t n_reads, kmr_reads **out);
/* device arrays in the layout kmr_add_reads_dev takes: bases[total], quals[total], u64 offsets[n+1] */
int kmr_reads_device_ptrs(const kmr_reads *r, void **dev_bases, void **dev_quals, void **dev_offsets);
/* copies to host; any pointer may be NULL.  name_off/name_len: span of each read's name line
 * (after '@') in the input text, for the host-side Read names */
int kmr_reads_copy(const kmr_reads *r, char *bases, char *quals, uint64_t *offsets,
                   uint64_t *name_off, uint32_t *name_len);
/* The batch in the form the reference's Read keeps its bases (src/Sequence.h: 2-bit packed + markups):
 * TwoBitSequence::compressSequence (src/TwoBitSequence.cpp:242-269) over every read on the device.  Read i's packed bases are
 * twobit[twobit_offsets[i] .. twobit_offsets[i+1]) (ceil(L/4) bytes, first base in bits 7-6, last byte zero padded), its markups
 * (any character but ACGTacgt; '.' recorded as 'N') are entries markup_offsets[i] .. markup_offsets[i+1] of markup_pos /
 * markup_char, in ascending offset.  *twobit_bytes and *n_markups always receive the sizes; with every array NULL that is all
 * the call does, and KMR_ERR_CAPACITY means an array was too small for them.  All arrays are host memory. */
int kmr_reads_twobit(kmr_handle *h, const kmr_reads *r, uint8_t *twobit, uint64_t twobit_capacity, uint64_t *twobit_offsets,
                     uint32_t *markup_pos, char *markup_char, uint64_t markup_capacity, uint64_t *markup_offsets,
                     uint64_t *twobit_bytes, uint64_t *n_markups);
/* Feed a batch in the form the reference's Read keeps it (src/Sequence.h:166-171,287-289: bases as a TwoBitSequence -- 2 bits per base, every
 * read on bytes of its own, first base in bits 7-6 -- plus markups for everything that is not ACGT, qualities as characters or
 * none): what a ReadSet hands over without a string per read, and a quarter of the bytes of kmr_add_reads on the way to the
 * device.  Replaces Read::getFasta / getQuals in front of KmerReadUtils::buildWeightedKmers (src/KmerReadUtils.h:176-190) and
 * TwoBitSequence::uncompressSequence + applyMarkup (src/TwoBitSequence.cpp:286-340), which run on the device.
 *   twobit / twobit_offsets   packed bases, read i = bytes [twobit_offsets[i], twobit_offsets[i+1]) (>= ceil(L_i / 4) of them; the layout
 *                             kmr_reads_twobit writes); the device form takes NULL offsets when every read starts on the byte
 *                             behind the one before it
 *   offsets                   n_reads + 1 base offsets (read i has offsets[i+1] - offsets[i] bases), as for kmr_add_reads
 *   markup_offsets / _pos / _char   optional: read i's markups are entries [markup_offsets[i], markup_offsets[i+1]), position and character
 *   quals                     qualities indexed by offsets (host form; the device form: dev_quals[0] is the quality of the call's first
 *                             base), or NULL and uniform_quality = the ONE quality character every base of the batch has (0: reads
 *                             without qualities, weight 1.0 as kmr_add_reads with quals == NULL)
 * Results are those of kmr_add_reads on the same reads.  The device form is asynchronous on the handle's stream like kmr_add_reads_dev.
 * A batch without a quality array (one character, or none) that is built on the super-k-mer lists with direction-counting values is
 * extracted from the packed bytes as they are; every other batch is unpacked to text in a scratch of the handle first.  kmr_tune
 * "packed_direct" = 0 forces the unpack (tests, A/B runs).
 * Device form: the packed bytes are fetched 16 bytes at a time from 16-byte aligned addresses, so up to 15 bytes in front of the
 * first read's first byte and behind the last read's last byte are READ (never used): dev_twobit must lie in an allocation that
 * holds them -- as hipMalloc'ed buffers do in front (256-byte aligned), and give the buffer 64 spare bytes behind the last read, as
 * for kmr_add_reads_dev. */
int kmr_add_reads_twobit(kmr_handle *h, const uint8_t *twobit, const uint64_t *twobit_offsets, const uint64_t *offsets,
                         const uint64_t *markup_offsets, const uint32_t *markup_pos, const char *markup_char,
                         const char *quals, int uniform_quality, uint64_t n_reads, uint64_t first_global_read_idx, const uint8_t *discarded);
int kmr_add_reads_twobit_dev(kmr_handle *h, const void *dev_twobit, const void *dev_twobit_offsets, const void *dev_offsets,
                             const void *dev_markup_offsets, const void *dev_markup_pos, const void *dev_markup_char,
                             const void *dev_quals, int uniform_quality, uint64_t n_reads, uint64_t total_bases,
                             uint64_t first_global_read_idx, const void *dev_discarded);
/* kmr_add_reads_dev on the batch, then kmr_sync */
int kmr_add_read_batch(kmr_handle *h, const kmr_reads *r, uint64_t first_global_read_idx);
void kmr_reads_free(kmr_reads *r);
/* kmr_score_reads on a device-resident read batch: FASTQ text -> reads -> spectrum -> trim / score without the host
 * staging the reads (outputs are host arrays of kmr_reads_info's n_reads entries) */
int kmr_score_read_batch(kmr_handle *h, const kmr_reads *r, double minimum_kmer_score, int scoring_type,
                         uint32_t *trim_offset, uint32_t *trim_length, float *score, uint8_t *was_trimmed);

/* ---- f4: artifact filter (FilterKnownOddities, src/FilterKnownOddities.h) ------------------
 * The screen FilterReads runs over every read before the spectrum build (apps/FilterReads.cpp:107-118):
 * (1) the longest run of bases with quality >= start + min_quality ("best"; the runner-up may be rescued as a
 * remnant read), (2) every 4th match_length-mer inside it looked up (canonical form) in a set made of all
 * match_length-mers of the artifact sequences, circularised, plus their substitution neighbours, (3) keep the
 * longer side of the read next to the hits, then discard or trim (recordAffectedRead :551-640).
 *
 * The artifact sequences are handed in as FASTA text (multi-line records allowed; the reference's are
 * FilterKnownOddities::getArtifactFasta/getSimpleRepeatFasta/getPhiX and --artifact-reference-file). Sequence
 * indices are 1-based in file order (0 is the reference's empty "no match" read); value n_sequences marks a
 * read that only lost bases to the quality screen ("MinQualityTrim"). */
typedef struct kmr_artifact_config {
	uint32_t match_length;          /* --artifact-match-length (24): multiple of 4, <= 28                             */
	uint32_t edit_distance;         /* --artifact-edit-distance (2)                                                   */
	uint32_t build_edits;           /* --build-artifact-edits-in-filter (2): 0 never, 1 always, 2 while < 750 000 keys */
	uint32_t simple_repeat_begin;   /* [begin, end) = the simple-repeat sequences (--mask-simple-repeats); 0,0 = none */
	uint32_t simple_repeat_end;
	uint32_t phix_idx;              /* the PhiX sequence (--phix-output); 0 = none                                    */
	uint32_t reference_begin;       /* first --artifact-reference-file sequence (not circularised); 0 = none          */
	uint32_t min_quality;           /* --min-quality-score                                                            */
	uint32_t fastq_start_char;      /* Read::FASTQ_START_CHAR the reads are scaled to                                 */
	float    min_read_length;       /* --min-read-length (fraction of the read if <= 1, bases otherwise)              */
} kmr_artifact_config;
void kmr_artifact_config_init(kmr_artifact_config *c);      /* the reference's defaults, start char 33, min quality 3, min length 0.40 */

typedef struct kmr_artifact_filter kmr_artifact_filter;
/* constructor + prepareMaps (:205-287); the key set lives in device memory */
int kmr_artifact_filter_create(kmr_handle *h, const kmr_artifact_config *cfg, const char *fasta, uint64_t len,
                               kmr_artifact_filter **out);
/* sequences.getSize(), filter.size(), and the edits left for query time (numErrors after prepareMaps) */
int kmr_artifact_filter_info(const kmr_artifact_filter *f, uint64_t *n_sequences, uint64_t *n_filter_kmers,
                             uint32_t *remaining_edits);
/* copies the (key, sequence index) pairs out in ascending key order (key = 2-bit packed match_length-mer,
 * first base most significant); returns KMR_ERR_CAPACITY if cap is too small */
int kmr_artifact_filter_entries(const kmr_artifact_filter *f, uint64_t *keys, uint32_t *values, uint64_t cap);
void kmr_artifact_filter_free(kmr_artifact_filter *f);
/* applyFilter (:663-733) over a device-resident read batch.  mate (host, n entries, may be NULL) = index of the
 * paired read or -1 (applyFilterToPair :355-386).  Per read (host arrays, each may be NULL):
 * value (matched sequence, n_sequences = quality trim only, 0 = clean), [min_pass, max_pass) the part to keep,
 * action 0 = untouched / 1 = trimmed ("AFTrim:<min_pass>+<max_pass-min_pass>") / 2 = discarded, and
 * [remnant_off, +remnant_len) the second-best quality run rescued as an extra read (len 0 = none).
 * *out (may be NULL) receives a new batch: read i trimmed or emptied in place, the remnants appended in read
 * order (the reference appends them per OpenMP thread). */
int kmr_artifact_filter_apply(kmr_handle *h, const kmr_artifact_filter *f, const kmr_reads *in, const int64_t *mate,
                              uint32_t *value, uint32_t *min_pass, uint32_t *max_pass, uint8_t *action,
                              uint32_t *remnant_off, uint32_t *remnant_len, kmr_reads **out);

/* ---- selectReads / writePicks: pick the passing reads and write FilterReads' output on the device ----------
 * selectReads (apps/FilterReads.h:159-279): its plain branch first (one threshold, one output), --partition-by-depth,
 * --remainder-trim and the per-input-file outputs behind it (kmr_partition_*), --max-kmer-output-depth last (kmr_normalize_*):
 * ReadSelector::pickAllPassingReads / pickAllPassingPairs (src/ReadSelector.h:547-596) and writePicks (:1242-1262).
 * Per read i of a device-resident batch -- the reads as the artifact filter left them (kmr_artifact_filter_apply's *out)
 * or an unfiltered batch -- and its results of the earlier stages:
 *   passing[i]  isPassingRead (:550-557): not discarded (af_action[i] != 2), score[i] >= minimum_score and
 *               passesLength(trim_length[i], length of read i in the batch, min_read_length) (:209-228, in float as there:
 *               a length <= 1 fails; a minimum <= 1 is a fraction of the read, above 1 a number of bases)
 *   pairs       mate[i] = index of the paired read or -1, the convention of kmr_artifact_filter_apply; NULL = every read
 *               is single (pickAllPassingReads).  isPassingPair (:558-568): both reads must pass if both_pass is set
 *               (--min-passing-in-pair 2), else either.  Every read of a passing pair is picked, also a mate that failed or
 *               was discarded (pickIfNew only asks for availability, :513-542)
 *   order       optimizePickOrder sorts the picks (:1212-1221): records appear in ascending read index
 *   record      Read::toFastq / toFasta (src/Sequence.cpp:761-779): "@name[ label]\n" bases "\n+\n" quals "\n", or
 *               ">name[ label]\n" bases "\n"; bases and quals are [trim_offset, trim_offset + trim_length) of the read.  A
 *               discarded read, or a trim of at most one base, prints as the base N with the quality output_quality_base + 1
 *               (src/Sequence.cpp:305-311, 729-733).  Qualities move from the handle's fastq_start_char to
 *               output_quality_base (--fastq-output-base-quality).  Read::REF_QUAL (127) is not a quality: a read whose first
 *               quality in the batch is 127 has none (Read::setRead, src/Sequence.cpp:652-655: what kmr_ingest_fasta without a
 *               qual text and kmr_extend_contigs give), and every base of such a read, and of a slice that starts on a 127,
 *               prints as PRINT_REF_QUAL (103, 'g') at either output base (Read::getQuals :744-746).  A 127 elsewhere moves
 *               like any byte.  Where the two quality bases differ this is the library's own rule: the reference's serial readers
 *               rescale a 127 with every other byte on the way in (src/ReadSet.cpp:324-337), after which it is no REF_QUAL.
 *               A trim_offset equal to the read's length leaves no base and prints the masked N, as in the reference; past the
 *               end, where the reference asserts, the same
 *   name        the read's name span (name_off / name_len of kmr_reads_copy) in `text`, the FASTQ text the batch was
 *               ingested from, up to the first blank or tab.  The caller hands that text in again (the library keeps no copy)
 *   label       parts joined by single blanks (Read::LABEL_SEP): "AFTrim:<min_pass>+<max_pass - min_pass>" if af_action[i]
 *               is 1, "Trim:<offset>+<length>" if was_trimmed[i], "<Label>:<(int)(score + 0.5)>" with Label = Score /
 *               MedianScore / MinScore / MaxScore / AvgScore (getKmerScoringTypeLabel, :248-257, in kmr_scoring's order).
 *               A discarded read was never scored (:1195-1197) and has no label.  Where the reference leaves the number open
 *               the rule is this library's: (int)(score + 0.5) is taken in double and truncates toward zero; a NaN score, for
 *               which the cast is undefined in C++, prints 0, and a sum outside int prints the nearest of -2147483648 and
 *               2147483647 (a NaN never passes the score test).  max_pass < min_pass, which the reference asserts against,
 *               prints the signed difference
 * Not covered: stored comments are not printed and a Casava "name 1:Y" is not rewritten to "name/1"; the unmasked formats.
 * Bimodal trimming: "Bimodal@..." / "InvBimodal@..." stands between AFTrim and Trim (kmr_set_bimodal_sigmas; the fused forms tag
 * what they score, the host-array forms take the words through kmr_select_bimodal).  Markup characters other than N, X and '.' are outside the parity claim: the reference applies a read's
 * markup positions to the already trimmed string (src/Sequence.cpp:322-325, src/TwoBitSequence.cpp:317-327), so such a
 * character lands on the wrong base when the trim offset is not 0, while the device prints the batch's own characters where
 * they are (N and X never lie inside a k-mer trim: it ends before the first of them).
 * Bounds: a batch holds fewer than 2^32 - 1 reads (KMR_ERR_UNSUPPORTED beyond); byte offsets of the output are 64-bit, its
 * size is bounded by device memory alone.
 * Every per-read array is host memory of kmr_reads_info's n_reads entries (the remnants the artifact filter appended
 * included: mate -1, af_action 0 for them); mate may be NULL, the three af_* arrays may be NULL together.  An empty batch
 * and zero picks are valid and give 0 bytes. */
typedef struct kmr_select_config {
	uint32_t struct_size;            /* = sizeof(kmr_select_config), ABI guard                                  */
	uint32_t both_pass;              /* --min-passing-in-pair 2                                                 */
	double   minimum_score;          /* --min-depth: the read's score must reach it (2)                         */
	float    min_read_length;        /* --min-read-length (0.40): fraction of the read if <= 1, bases otherwise */
	uint32_t output_quality_base;    /* --fastq-output-base-quality: 33 or 64 (33)                              */
	uint32_t format;                 /* 0 = FASTQ, 1 = FASTA                                                    */
	uint32_t scoring_type;           /* kmr_scoring: the score of the fused form, and the label (MEDIAN)        */
} kmr_select_config;
int kmr_select_config_init(kmr_select_config *cfg);      /* the reference's defaults */
typedef struct kmr_picks kmr_picks;
/* The words of kmr_bimodal_copy that belong to the trims of the NEXT kmr_select_reads*, kmr_partition_reads* or kmr_normalize_reads*
 * on the handle: that call prints their tags and consumes them (a count other than its batch's: KMR_ERR_INVALID_ARG there).
 * NULL takes them back. */
int kmr_select_bimodal(kmr_handle *h, const uint64_t *words, uint64_t n_reads);
/* selection and output from host arrays as kmr_score_read_batch / kmr_score_counts_dev and kmr_artifact_filter_apply return them */
int kmr_select_reads(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, const int64_t *mate,
                     const uint8_t *af_action, const uint32_t *af_min_pass, const uint32_t *af_max_pass,
                     const uint32_t *trim_offset, const uint32_t *trim_length, const float *score, const uint8_t *was_trimmed,
                     const kmr_select_config *cfg, kmr_picks **out);
/* The fused form: scoreAndTrimReads as kmr_score_read_batch (needs a finalized handle, KMR_ERR_STATE otherwise), then the
 * selection, with the trims kept on the device.  cfg->minimum_score is both the k-mer threshold of the trim and the read
 * threshold of the selection, as FilterReads hands minDepth to both (apps/FilterReads.cpp:197-199). */
int kmr_filter_read_batch(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, const int64_t *mate,
                          const uint8_t *af_action, const uint32_t *af_min_pass, const uint32_t *af_max_pass,
                          const kmr_select_config *cfg, kmr_picks **out);
/* the same two with the FASTQ text already in device memory */
int kmr_select_reads_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, const int64_t *mate,
                         const uint8_t *af_action, const uint32_t *af_min_pass, const uint32_t *af_max_pass,
                         const uint32_t *trim_offset, const uint32_t *trim_length, const float *score, const uint8_t *was_trimmed,
                         const kmr_select_config *cfg, kmr_picks **out);
int kmr_filter_read_batch_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, const int64_t *mate,
                              const uint8_t *af_action, const uint32_t *af_min_pass, const uint32_t *af_max_pass,
                              const kmr_select_config *cfg, kmr_picks **out);
/* picks (ReadSelector::getNumPicks) and the size of the output text */
int kmr_picks_info(const kmr_picks *p, uint64_t *n_picked, uint64_t *bytes);
/* the text to host memory (KMR_ERR_CAPACITY if capacity < bytes) and, unless NULL, one flag per read of the batch: 1 = picked */
int kmr_picks_copy(const kmr_picks *p, char *dst, uint64_t capacity, uint8_t *picked_flags);
/* the text where it lies (for a compressor or a device-aware MPI-IO); valid until kmr_picks_free */
int kmr_picks_device_ptr(const kmr_picks *p, void **dev_text);
void kmr_picks_free(kmr_picks *p);

/* ---- selectReads, the partitioned branch (apps/FilterReads.h:209-278): --partition-by-depth, --remainder-trim and one
 * output per input file.  Everything above holds per read -- passing, pairs, record, name, label are those of
 * scoreAndTrimReads(min depth) and do not change between rounds; what is new is that the selection runs in rounds:
 *   rounds      maxDepth = partition_by_depth if it is > 0, else minDepth (= minimum_score, an unsigned int there, :159);
 *               for (unsigned depth = maxDepth; depth >= minDepth; depth /= 2) selects at tmpMinDepth = max(minDepth, depth)
 *               (:221-223), a float compared with the read's float score, with the current min_read_length and both_pass.
 *               The sequence is not "every power of two": 16 over 2 gives 16 8 4 2, 20 over 3 gives 20 10 5 and ends without
 *               reaching minDepth, partition_by_depth < minDepth runs no round and picks nothing
 *   available   a picked read is no longer available (pickIfNew, src/ReadSelector.h:513-542; isPassingRead :550-557), so a
 *               read lands in the FIRST round whose decision picks it; every read of a passing pair is picked in that round,
 *               also a mate that failed or was discarded
 *   remainder   if the output is partitioned, the loop reached depth == minDepth, remainder_trim > 0 and
 *               (both_pass is set || (int) min_read_length != remainder_trim) (:256-262), one more round runs at minDepth with
 *               --min-passing-in-pair 1 and min_read_length = remainder_trim: the mates and shorter trims the strict rounds left
 *   order       optimizePickOrder sorts the picks of the current round only (:1212-1221): the output is round-major, ascending
 *               read index inside a round; with --separate-outputs 0 that concatenation is the one output file
 *   files       with --separate-outputs 1 every name gets "-MinDepth<minDepth>" (:173), a partitioned round
 *               "-PartitionDepth<tmpMinDepth>" (:232; a float through lexical_cast: 16, not 16.0), the remainder round
 *               "-Remainder" (:230), and writePick adds "-" + getReadFileNamePrefix(read) (src/ReadSelector.h:1252-1262), so the
 *               reads of a round split by input file.  input_starts = n_inputs + 1 ascending read indices, the first 0, the
 *               last n_reads: input j holds the reads [input_starts[j], input_starts[j + 1]) (it may be empty).  NULL / 0 =
 *               one input
 *   segment     = round * n_inputs + input.  The text of kmr_picks_copy / kmr_picks_device_ptr is the segments in that order,
 *               each a contiguous slice; the segment table gives per segment {first pick, picks, first byte, bytes}, and
 *               read_segment the segment of every read of the batch (-1 = not picked)
 * partition_by_depth 0 is one round at minimum_score as kmr_select_reads runs it (any minimum_score, no remainder): with one
 * input the same bytes and flags.  With partition_by_depth set, minimum_score must be a whole number in [0, 2^32)
 * (KMR_ERR_INVALID_ARG otherwise), and partition_by_depth is taken as the unsigned depth of the loop (the reference reads an int;
 * values above 2^31 - 1 cannot be given to it).
 * Bounds: at most 33 rounds (32 halvings of a 32-bit depth and the remainder; minimum_score 0 under a depth of 2^31 or more
 * would need 34: KMR_ERR_UNSUPPORTED); rounds x inputs <= 256 segments (KMR_ERR_UNSUPPORTED beyond): the counting pass keeps 12
 * bytes of LDS per segment and wavefront, 3 KiB at 256, which lets 32 wavefronts share a CU's 160 KiB.
 * Not covered: --kmer-size 0 (the tmpMinDepth = 0 special case, :224-227).  Bimodal trimming is the handle's (kmr_set_bimodal_sigmas).
 * KMR_ERR_INVALID_ARG: a wrong struct_size; input_starts that does not start at 0, descends or does not end at n_reads. */
typedef struct kmr_partition_config {
	uint32_t struct_size;            /* = sizeof(kmr_partition_config), ABI guard                                           */
	kmr_select_config select;        /* minimum_score = --min-depth, min_read_length, both_pass, format, ...                */
	uint32_t partition_by_depth;     /* --partition-by-depth; 0 = off: one round at minimum_score, no remainder             */
	float    remainder_trim;         /* --remainder-trim; <= 0 = off (-1, the reference's default)                          */
} kmr_partition_config;
int kmr_partition_config_init(kmr_partition_config *cfg);      /* the reference's defaults: both off */
/* The table of rounds of a configuration, without a device: n_rounds and, per round in the order they run (arrays of 33, any
 * may be NULL), the depth (tmpMinDepth), min_read_length, both_pass and whether it is the remainder round. */
int kmr_partition_rounds(const kmr_partition_config *cfg, uint32_t *n_rounds, float *round_depth, float *round_min_read_length,
                         uint32_t *round_both_pass, uint8_t *round_is_remainder);
/* as kmr_select_reads / kmr_select_reads_dev / kmr_filter_read_batch / kmr_filter_read_batch_dev */
int kmr_partition_reads(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, const int64_t *mate,
                        const uint8_t *af_action, const uint32_t *af_min_pass, const uint32_t *af_max_pass,
                        const uint32_t *trim_offset, const uint32_t *trim_length, const float *score, const uint8_t *was_trimmed,
                        const uint64_t *input_starts, uint32_t n_inputs, const kmr_partition_config *cfg, kmr_picks **out);
int kmr_partition_reads_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, const int64_t *mate,
                            const uint8_t *af_action, const uint32_t *af_min_pass, const uint32_t *af_max_pass,
                            const uint32_t *trim_offset, const uint32_t *trim_length, const float *score, const uint8_t *was_trimmed,
                            const uint64_t *input_starts, uint32_t n_inputs, const kmr_partition_config *cfg, kmr_picks **out);
int kmr_partition_read_batch(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, const int64_t *mate,
                             const uint8_t *af_action, const uint32_t *af_min_pass, const uint32_t *af_max_pass,
                             const uint64_t *input_starts, uint32_t n_inputs, const kmr_partition_config *cfg, kmr_picks **out);
int kmr_partition_read_batch_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, const int64_t *mate,
                                 const uint8_t *af_action, const uint32_t *af_min_pass, const uint32_t *af_max_pass,
                                 const uint64_t *input_starts, uint32_t n_inputs, const kmr_partition_config *cfg, kmr_picks **out);
/* rounds and inputs of the picks: 1 and 1 from the plain entry points */
int kmr_picks_segments_info(const kmr_picks *p, uint32_t *n_rounds, uint32_t *n_inputs);
/* to host memory, any may be NULL: per round its depth and whether it is the remainder round; per segment (n_rounds x n_inputs,
 * round-major) its first pick, picks, first byte and bytes; per read of the batch its segment, -1 = not picked */
int kmr_picks_segments_copy(const kmr_picks *p, float *round_depth, uint8_t *round_is_remainder, uint64_t *seg_first_pick,
                            uint64_t *seg_picks, uint64_t *seg_first_byte, uint64_t *seg_bytes, int32_t *read_segment);

/* ---- selectReads, the normalizing branch (apps/FilterReads.h:178-206): --max-kmer-output-depth, "targeted read normalization
 * depth", with --normalization-method RANDOM: ReadSelector::pickCoverageNormalizedSubset and chooseRead
 * (src/ReadSelector.h:661-749).  Reads of high coverage are thinned so that a k-mer is written about target_depth times.
 * passing, record, name and label are those above at (minimum_score, min_read_length); what is new, with T = target_depth:
 *   score       s(i) = passing(i) ? (long) score[i] : -1 (:685-686); the cast truncates, 0.7 becomes 0 (beyond the range of a
 *               long, where the reference's cast is undefined, it saturates).  A missing side of a half pair has s = -1
 *   choose      chooseRead (:661-672) of a score s > 0: true if s <= T, else (draw(g) % s) <= T -- inclusive, so T + 1 of s
 *               residues keep the read
 *   draw        the reference draws from one mt19937 per OpenMP thread seeded with time(NULL): no two of its runs agree.  The
 *               rule is kept and the stream replaced: draw(g) = word 0 of Philox4x32-10 with the counter (g & 0xffffffff,
 *               g >> 32, 0, 0) and the key (seed & 0xffffffff, seed >> 32), g = first_global_read_idx + read index.  A result
 *               depends on (seed, g) alone: not on scheduling, not on how a job is cut into batches or ranks
 *   pairs       the pair list (read1, read2, n_pairs) as kmr_pairs_copy returns it, -1 = no read on that side; NULL = every
 *               read is a half pair; a read no pair names is a half pair (read, -1) of its own
 *   by_pair 1   (the reference passes reads.hasPairs()) per pair: skipped unless isPassingPair (:558-568: both reads must pass
 *               if both exist and both_pass is set, else either); skipped under both_pass if s1 <= 0 or s2 <= 0 (:697-702);
 *               skipped if s1 <= 0 and s2 <= 0; else choose(max(s1, s2), g of the pair's lower read index).  A chosen pair is
 *               one pick that holds every read of the pair, also a mate that failed or was discarded (it prints as N)
 *   by_pair 0   read1 is kept if s1 > 0 and choose(s1, g(read1)), read2 likewise; if either is kept they form one pick (:716-733)
 *   order       optimizePickOrder (:1212-1221) sorts picks by the lower read index of the pair (Pair::operator<,
 *               src/ReadSet.h:118-123); a pick is written read1 then read2 (:1245-1250), and read1 may be the higher index
 *               (phase 2 of kmr_identify_pairs).  The output therefore interleaves mates whatever their indices
 *   files       one round at depth minimum_score and n_inputs segments; every record goes to the file of its own read's input
 *               (:1252-1262), so the mates of an R1 file and an R2 file part again.  The reference names the files
 *               output + "-MinDepth<d>" + "-MaxDepth<T>" + "-" + prefix + suffix (apps/FilterReads.h:173,180)
 * Two things the reference does and this keeps: under both_pass the s <= 0 test drops EVERY half pair, although isPassingPair
 * and pickAllPassingPairs let a passing half pair through; and a passing read whose score truncates to 0 is never chosen.
 * Refused with KMR_ERR_UNSUPPORTED: method != 0 -- OPTIMAL is a serial greedy heap over a shared count map (:751-922) --
 * and use_logscale (--use-logscale-above-max): its log((float) score / (float) targetDepth) binds to the float or the double
 * overload depending on the include order and is rounded under the reference's -ffast-math, so nothing pins its value.
 * Not covered: --max-kmer-output-depth together with --partition-by-depth (the reference refuses it, src/ReadSelector.h:137).
 * KMR_ERR_INVALID_ARG: target_depth 0, a wrong struct_size, read1 without read2, a pair index outside [-1, n_reads), a pair
 * without a read, a read that two pairs name, input_starts as above.  n_picked of kmr_picks_info counts records.  An empty
 * batch and zero picks are valid.  The number of launches does not depend on the batch, nothing per read comes back to the
 * host, and the call waits once for the totals. */
typedef struct kmr_normalize_config {
	uint32_t struct_size;            /* = sizeof(kmr_normalize_config), ABI guard                                          */
	kmr_select_config select;        /* minimum_score = --min-depth, min_read_length, both_pass, format, ...               */
	uint64_t target_depth;           /* --max-kmer-output-depth, > 0                                                       */
	uint64_t seed;                   /* key of the draws                                                                   */
	uint64_t first_global_read_idx;  /* global index of the batch's first read: a job cut into batches draws as one        */
	uint32_t by_pair;                /* decide per pair (ReadSet::hasPairs of the job) or per read                         */
	uint32_t method;                 /* 0 = RANDOM; anything else KMR_ERR_UNSUPPORTED                                      */
	uint32_t use_logscale;           /* --use-logscale-above-max: KMR_ERR_UNSUPPORTED if set                               */
} kmr_normalize_config;
int kmr_normalize_config_init(kmr_normalize_config *cfg);      /* the select defaults, RANDOM, seed 0; target_depth is the caller's */
/* as kmr_partition_reads / _reads_dev / _read_batch / _read_batch_dev with the pair list in place of mate */
int kmr_normalize_reads(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, const int64_t *read1,
                        const int64_t *read2, uint64_t n_pairs, const uint8_t *af_action, const uint32_t *af_min_pass,
                        const uint32_t *af_max_pass, const uint32_t *trim_offset, const uint32_t *trim_length, const float *score,
                        const uint8_t *was_trimmed, const uint64_t *input_starts, uint32_t n_inputs, const kmr_normalize_config *cfg,
                        kmr_picks **out);
int kmr_normalize_reads_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, const int64_t *read1,
                            const int64_t *read2, uint64_t n_pairs, const uint8_t *af_action, const uint32_t *af_min_pass,
                            const uint32_t *af_max_pass, const uint32_t *trim_offset, const uint32_t *trim_length, const float *score,
                            const uint8_t *was_trimmed, const uint64_t *input_starts, uint32_t n_inputs,
                            const kmr_normalize_config *cfg, kmr_picks **out);
int kmr_normalize_read_batch(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, const int64_t *read1,
                             const int64_t *read2, uint64_t n_pairs, const uint8_t *af_action, const uint32_t *af_min_pass,
                             const uint32_t *af_max_pass, const uint64_t *input_starts, uint32_t n_inputs,
                             const kmr_normalize_config *cfg, kmr_picks **out);
int kmr_normalize_read_batch_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, const int64_t *read1,
                                 const int64_t *read2, uint64_t n_pairs, const uint8_t *af_action, const uint32_t *af_min_pass,
                                 const uint32_t *af_max_pass, const uint64_t *input_starts, uint32_t n_inputs,
                                 const kmr_normalize_config *cfg, kmr_picks **out);
/* of picks the four above made (KMR_ERR_INVALID_ARG for others), any may be NULL: the picks as the reference counts them (pairs,
 * the return value of pickCoverageNormalizedSubset), the chooseRead calls, and those among them that drew (s > T) */
int kmr_normalize_info(const kmr_picks *p, uint64_t *n_picks, uint64_t *n_candidates, uint64_t *n_draws);

/* ---- the artifact filter's report: its -Artifact.fastq and -PhiX.fastq files and its per-sequence counters, on the device ----------
 * What FilterKnownOddities' Recorder (src/FilterKnownOddities.h:296-353) makes of the decisions kmr_artifact_filter_apply returns,
 * in the order one thread of the reference takes (under OpenMP the reference's own order is arbitrary):
 *   unit        with a pair list one entry of it, read1 then read2, either may be absent (applyFilterToPair :355-386); without,
 *               one read (applyFilterToRead with recordEffects :389, :695).  v1, v2 = the reads' own value, 0 for an absent side;
 *               nothing happens unless v1 != 0 || v2 != 0 (:555-560)
 *   PhiX unit   isPhiX(v1) || isPhiX(v2) (:556): every present read, a clean mate included, is discarded and counted under phix_idx:
 *               discarded[phix]++, bases[phix] += length (:569-587, recordDiscard :310-320); with phix_output each is written
 *               without a label to the PhiX file of the input read1 belongs to (:574), read2's if read1 is absent
 *   other unit  for each present read with v != 0 (:613, :623): action 2: discarded[v]++, bases[v] += length, and with artifact_output
 *               a record labelled getFilterName(v) in the Artifact file of read1's input (:603-609, :618); action 1: trimmed[v]++,
 *               bases[v] += length - (max_pass - min_pass), no record (recordTrim :321-334).  The action is the one
 *               kmr_artifact_filter_apply returned; a clean mate is neither counted nor written
 *   record      _writeFilterRead (:734-736) = FormatOutput::FastqUnmasked() after read.discard() (:311): getFastaNoMarkup of a
 *               discarded read answers N (src/Sequence.cpp:290-296) while getQuals(unmasked) skips its discarded shortcut
 *               (:729-759): "@name[ label]\nN\n+\n" all `length` qualities "\n", length = the read's before the filter; for a length
 *               <= 1 the quality line is the one character output_quality_base + 1 (:752-758).  print_bases = 1 prints the read's own
 *               `length` characters, as the unfiltered batch holds them, in place of N (reads of length <= 1 as before)
 *   name        as the selection's writer cuts it: up to the first blank or tab; qualities move from the handle's fastq_start_char
 *               to output_quality_base; stored comments stay uncovered, as in the selection
 *   label       getFilterName (:543-550): the FASTA header of sequence v after '>' up to the first blank or tab; for
 *               v == n_sequences "MinQualityTrim<min_quality>"; an empty name prints no label (src/Sequence.cpp:767)
 *   files       OfstreamMap(out, "-PhiX.fastq") / (out, "-Artifact.fastq") with key "-" + prefix (:670-677): the picks' segment table
 *               has two rows times n_inputs, row 0 Artifact, row 1 PhiX; a segment without a record is a file the reference never opens
 *   table       applyFilter :714-725: the counters of every index with bases > 0, ascending
 * `in` is the batch the filter was applied to (lengths and qualities are the original ones), `text` its name text.  value, action,
 * min_pass and max_pass are the host arrays kmr_artifact_filter_apply returned (n_reads entries).  read1 / read2 (n_pairs entries, -1 =
 * no read on that side) have the convention of kmr_pairs_copy and kmr_normalize_reads; NULL = every read is a unit of its own.
 * input_starts / n_inputs as kmr_partition_reads takes them (at most 128 inputs).
 * KMR_ERR_INVALID_ARG, with the cause in kmr_last_error: a wrong struct_size, a quality base other than 33 or 64, read1 without
 * read2, an index outside [-1, n), a pair without a read, a read two pairs name or, under a pair list, a read no pair names
 * (identifyPairs never leaves one), phix_output with a filter whose phix_idx is 0, a value above n_sequences.
 * An empty batch and a batch without records are valid and give 0 bytes. */
typedef struct kmr_artifact_report_config {
	uint32_t struct_size;            /* = sizeof(kmr_artifact_report_config), ABI guard                 */
	uint32_t artifact_output;        /* --filter-output: write the Artifact records (1)                  */
	uint32_t phix_output;            /* --phix-output: write the PhiX records (1)                        */
	uint32_t output_quality_base;    /* --fastq-output-base-quality: 33 or 64 (33)                       */
	uint32_t print_bases;            /* 0 = the base line N, as the reference writes it; 1 = the bases   */
} kmr_artifact_report_config;
int kmr_artifact_report_config_init(kmr_artifact_report_config *cfg);
typedef struct kmr_artifact_report kmr_artifact_report;
int kmr_artifact_filter_report(kmr_handle *h, const kmr_artifact_filter *f, const kmr_reads *in, const char *text, uint64_t text_len,
                               const int64_t *read1, const int64_t *read2, uint64_t n_pairs, const uint32_t *value, const uint8_t *action,
                               const uint32_t *min_pass, const uint32_t *max_pass, const uint64_t *input_starts, uint32_t n_inputs,
                               const kmr_artifact_report_config *cfg, kmr_artifact_report **report);
/* the same with the name text in device memory */
int kmr_artifact_filter_report_dev(kmr_handle *h, const kmr_artifact_filter *f, const kmr_reads *in, const void *dev_text, uint64_t text_len,
                                   const int64_t *read1, const int64_t *read2, uint64_t n_pairs, const uint32_t *value, const uint8_t *action,
                                   const uint32_t *min_pass, const uint32_t *max_pass, const uint64_t *input_starts, uint32_t n_inputs,
                                   const kmr_artifact_report_config *cfg, kmr_artifact_report **report);
/* The fused form: everything kmr_artifact_filter_apply does, with the same optional host outputs and the same *out batch, and the
 * report from the decisions while they are on the device (no per-read array crosses the bus unless the caller asked for one).  It
 * takes the pair list; the mate of the apply step is derived from it on the device. */
int kmr_artifact_filter_apply_report(kmr_handle *h, const kmr_artifact_filter *f, const kmr_reads *in, const char *text, uint64_t text_len,
                                     const int64_t *read1, const int64_t *read2, uint64_t n_pairs, uint32_t *value, uint32_t *min_pass,
                                     uint32_t *max_pass, uint8_t *action, uint32_t *remnant_off, uint32_t *remnant_len, kmr_reads **out,
                                     const uint64_t *input_starts, uint32_t n_inputs, const kmr_artifact_report_config *cfg,
                                     kmr_artifact_report **report);
int kmr_artifact_filter_apply_report_dev(kmr_handle *h, const kmr_artifact_filter *f, const kmr_reads *in, const void *dev_text, uint64_t text_len,
                                         const int64_t *read1, const int64_t *read2, uint64_t n_pairs, uint32_t *value, uint32_t *min_pass,
                                         uint32_t *max_pass, uint8_t *action, uint32_t *remnant_off, uint32_t *remnant_len, kmr_reads **out,
                                         const uint64_t *input_starts, uint32_t n_inputs, const kmr_artifact_report_config *cfg,
                                         kmr_artifact_report **report);
/* discarded (discardedCounts), trimmed (readCounts) and bases (baseCounts) per sequence index, n_sequences + 1 entries each (each may
 * be NULL); KMR_ERR_CAPACITY below that */
int kmr_artifact_report_counts(const kmr_artifact_report *report, uint64_t *discarded, uint64_t *trimmed, uint64_t *bases, uint64_t capacity);
/* the records: a kmr_picks borrowed from the report (do not free it; it lives as long as the report).  kmr_picks_info, _copy,
 * _device_ptr, _segments_info and _segments_copy work on it: n_rounds is 2 (row 0 Artifact, row 1 PhiX), a read's segment is
 * row * n_inputs + input or -1.  The text stays in device memory until it is copied. */
int kmr_artifact_report_picks(const kmr_artifact_report *report, const kmr_picks **picks);
void kmr_artifact_report_free(kmr_artifact_report *report);
/* getFilterName(idx) for idx in [1, n_sequences]: the NUL-terminated label; KMR_ERR_CAPACITY if it does not fit dst */
int kmr_artifact_filter_name(const kmr_artifact_filter *f, uint32_t idx, char *dst, uint64_t capacity);

/* ---- ReadSet::identifyPairs: which reads of a batch are the two ends of one fragment, on the device ----------
 * One call equals one ReadSet::identifyPairs() (src/ReadSet.cpp:446-570) on a fresh ReadSet that holds the batch's reads in
 * batch order: no earlier pairs, previousReadName empty.  apps/FilterReads.cpp:103 and importAndProcessReadset of FilterReads-P
 * call it after the input is read; the artifact filter, isPassingPair and ReadSet::hasPairs (which chooses between
 * pickAllPassingPairs and pickAllPassingReads) use what it finds.
 *   name        a read's name and comment are what trimName (src/Utils.h:561-598) makes of its name span (name_off / name_len of
 *               kmr_reads_copy) in `text`, the FASTQ text the batch was ingested from: the name runs to the first blank, tab, CR
 *               or LF, the comment is the rest if at least one character follows the separator.  With store_comment == 0 a
 *               Casava-1.8 comment (isCommentCasava18, :678-685) on a name that does not already end in "/x" rewrites the name
 *               to name/1 or name/2 and the read keeps no comment; with store_comment != 0 the comment is kept and the name is
 *               not rewritten.  Pass the value the batch was ingested with
 *   readNum     (:689-713) 1 or 2 from a Casava comment if there is one, else from a trailing /1 /A /F -> 1 or /2 /B /R -> 2, else 0
 *   commonName  (:669-676) the name without its last character if it is longer than 2 and its second-to-last character is '/'
 *   phase 1     sequential pairs (:467-478 over _isSequentialPair, :94-118): the reads in order with one pending read; a read
 *               with readNum 0 clears it, a read that isPair()s with it (:719-733: same common name, different non-zero read
 *               numbers) forms Pair(i - 1, i) and clears it, any other read becomes the pending one.  The earlier index is read1
 *   phase 2     by name (:500-565) over the reads phase 1 left unpaired, in index order, with a map from common name to pair:
 *               without an entry the read pushes a half pair (read2 if readNum == 2, else read1) and enters the map if
 *               readNum > 0; with an entry it fills the free side (readNum == 2 -> read2, anything else, 0 included, -> read1)
 *               and the entry is erased, or, if that side is taken, the entry is erased and the read pushes a half pair of its
 *               own that is not entered (the two warning branches, :522-543: n_conflicts)
 *   result      mate[i] = the read paired with i or -1 (the convention of kmr_artifact_filter_apply and kmr_select_reads);
 *               the pair list (read1, read2) with -1 for MAX_READ_IDX in the reference's order: phase-1 pairs ascending, then
 *               the phase-2 records in the order of the reads that pushed them.  n_pairs = getPairSize(), n_full = pairs with
 *               both reads, n_sequential = phase-1 pairs, has_pairs = hasPairs(): 0 < n_pairs < n_reads (src/ReadSet.h:526-529)
 * Names are matched through a 64-bit hash of the common name and then byte for byte, so a hash collision does not change the
 * result (kmr_tune "pair_hash_bits", kmr_build_info "pair_hash_collisions").  Nothing per read crosses the bus inside the call.
 * A batch without names (kmr_reads_from_host, kmr_reads_from_twobit: text_len 0) is valid: every read is a half pair of its
 * own and has_pairs is 0.  An empty batch is valid.  A name span outside the text is KMR_ERR_INVALID_ARG.
 * Not covered: a second identifyPairs() on a set that already has pairs (the reference stores a read index where a pair
 * index is read back, :492-495 against :520, which coincides only by accident); the per-file identifyPairs and re-ordering
 * of appendAllFiles (:216-239) -- one call over the concatenated batch gives the same pairs for an R1 file followed by an R2
 * file; printing name/1 for rewritten Casava names in writePicks (see above).
 * Bounds: a batch holds fewer than 2^32 - 1 reads (KMR_ERR_UNSUPPORTED beyond). */
typedef struct kmr_pairs kmr_pairs;
int kmr_identify_pairs(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, int store_comment, kmr_pairs **out);
/* the same with the FASTQ text already in device memory */
int kmr_identify_pairs_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, int store_comment, kmr_pairs **out);
/* any pointer may be NULL */
int kmr_pairs_info(const kmr_pairs *p, uint64_t *n_reads, uint64_t *n_pairs, uint64_t *n_full, uint64_t *n_sequential, uint64_t *n_conflicts, int *has_pairs);
/* to host memory: mate[n_reads], read1[n_pairs], read2[n_pairs]; any may be NULL */
int kmr_pairs_copy(const kmr_pairs *p, int64_t *mate, int64_t *read1, int64_t *read2);
/* the three arrays (int64) where they lie; any may be NULL; valid until kmr_pairs_free */
int kmr_pairs_device_ptrs(const kmr_pairs *p, void **dev_mate, void **dev_read1, void **dev_read2);
void kmr_pairs_free(kmr_pairs *p);

/* ---- DuplicateFragmentFilter: fragments with the same first bases collapse to consensus reads, on the device ----------
 * One call equals one DuplicateFragmentFilter::_filterDuplicateFragments (src/DuplicateFragmentFilter.h:505-559) over the
 * batch, with cutoff 2, edit distance 0 and consensus on, in the order a single-threaded reference visits the pair list:
 * the paired pass (paired = 1) or the pass --dedup-single adds (paired = 0).  apps/FilterReads.cpp:120-141 runs the stage
 * between the artifact filter and the spectrum build when --dedup-mode is 1 or 2.  `pairs` is what kmr_identify_pairs* left
 * for this batch, `text` the FASTQ text the batch was ingested from (names), `discarded` one byte per read, non-zero =
 * Read::isDiscarded (the artifact filter's action == 2), NULL = none.
 *   candidates  (:194-279) the pair list in its own order.  Paired pass: a record with both ends takes part, one with a
 *               single end counts as skipped[2] (unpaired); single pass: a record with exactly one end takes part, one with
 *               two counts as unpaired.  A member with a discarded read counts as skipped[0]; one with a read shorter than
 *               start_offset + L up to its first X or x (getFirstMarkupXLength, src/Sequence.cpp:432-439) as skipped[1],
 *               read 1 tested before read 2, one count per record; a read index outside the batch as skipped[3].  L is
 *               dedup_length in the paired pass and 2 * dedup_length in the single pass (:188-190)
 *   key         (:217-241) the 2-bit code (anything but ACGT packs as A) of read 1's bases [start_offset, start_offset + L)
 *               followed by the reverse complement of read 2's, or of the one read's window in the single pass.  With
 *               dedup_mode 2 the paired pass takes the smaller, in memcmp order, of the key and its reverse complement
 *               (buildLeastComplement, src/Kmer.h:356-364: a tie keeps the key) and a member whose key was replaced is
 *               flipped: its read2 counts as side 1
 *   groups      members with equal keys, in ascending position in the pair list (the instance order of a serial build,
 *               src/KmerTrackingData.h:810-841); those of two members and more are collapsed
 *   consensus   (:420-503, :361-418) per collapsed group one read per side -- two in the paired pass, side 1 then side 2, one
 *               in the single pass --: ReadSet::getConsensusRead(min_quality_score) of the side's reads in member order
 *               (src/ReadSet.cpp:572-629; Read::getProbabilityBases and ProbabilityBase, src/Sequence.cpp:563-582, 807-967,
 *               src/Sequence.h:304-338, the copy constructor's setTop included), named "C" + the member count + "-" + the
 *               name of the side's first member up to its first blank or tab (what kmr_select_reads prints of a name)
 *   discards    every read of every member of a collapsed group (:475-491); affected = reads so discarded
 * The consensus reads are a batch of their own, owned by the kmr_dedup: bases and qualities at the handle's
 * fastq_start_char, name spans pointing into a name text of its own (the names back to back, each followed by a newline).
 * kmr_artifact_filter_apply, kmr_add_read_batch, kmr_identify_pairs* and kmr_filter_read_batch* take it as any other batch;
 * the reference appends it behind the last read (:552), so its output text follows the main batch's.  In the paired pass read
 * 2g and read 2g + 1 are the two sides of group g.
 * dedup_mode 0 is the reference's default and means the stage is off (:563-566): a valid call that collapses nothing.
 * An empty batch, a batch without pairs and a batch without duplicates are valid: no groups, an empty consensus batch.
 * Nothing per read crosses the bus inside the call but `discarded`; three fixed-size copies bring sizes back.
 * Not covered: the order of the consensus reads among themselves -- the reference's follows the bucket iteration of its map
 * and, under OpenMP, the thread that met the group; here groups come out in ascending position of their first member, and the
 * parity claim is on the set of consensus reads, each byte for byte, the discard flags and the counters; dedup-edit-distance 1
 * (its consolidation order depends on a sort of equal counts and on thread timing) and dedup-consensus 0 (it draws from
 * LongRand): KMR_ERR_UNSUPPORTED; keys of more than 128 bases (2 * dedup_length > 128): KMR_ERR_UNSUPPORTED; the artifact
 * filter's run over the new reads (:534-550) and reads.append stay with the caller; the Casava rewrite of a first member's
 * name, as in kmr_select_reads.  dedup_length or start_offset not a multiple of 4 is KMR_ERR_INVALID_ARG (the option check, :137).
 * Bounds: a batch holds fewer than 2^32 - 1 reads; a group's member count enters getA .. getT as a short, as in the reference. */
typedef struct kmr_dedup_config {
	uint32_t struct_size;
	uint32_t dedup_mode;        /* 0 off, 1 one orientation, 2 both orientations */
	uint32_t paired;            /* 1: the pass over pairs, 0: the --dedup-single pass over single reads */
	uint32_t dedup_length;      /* 24 */
	uint32_t start_offset;      /* 0 */
	uint32_t edit_distance;     /* 0 */
	uint32_t consensus;         /* 1 */
} kmr_dedup_config;
int kmr_dedup_config_init(kmr_dedup_config *cfg);      /* the reference's defaults (:60-61), paired = 1 */
typedef struct kmr_dedup kmr_dedup;
int kmr_dedup_fragments(kmr_handle *h, const kmr_reads *reads, const char *text, uint64_t text_len, const kmr_pairs *pairs,
                        const uint8_t *discarded, const kmr_dedup_config *cfg, kmr_dedup **out);
/* the same with the FASTQ text already in device memory (`discarded` is host memory in both) */
int kmr_dedup_fragments_dev(kmr_handle *h, const kmr_reads *reads, const void *dev_text, uint64_t text_len, const kmr_pairs *pairs,
                            const uint8_t *discarded, const kmr_dedup_config *cfg, kmr_dedup **out);
/* any pointer may be NULL; skipped = discarded, too short, unpaired, invalid */
int kmr_dedup_info(const kmr_dedup *d, uint64_t *n_groups, uint64_t *n_new_reads, uint64_t *affected, uint64_t skipped[4]);
/* to host memory: discarded_out[n_reads] = the flags handed in OR the new discards; per collapsed group, in output order, the
 * pair-list position of its first member and its member count; any may be NULL */
int kmr_dedup_copy(const kmr_dedup *d, uint8_t *discarded_out, uint64_t *group_first, uint32_t *group_size);
/* the same three arrays where they lie; valid until kmr_dedup_free */
int kmr_dedup_device_ptrs(const kmr_dedup *d, void **dev_discarded, void **dev_group_first, void **dev_group_size);
/* the consensus batch (owned by d: do not kmr_reads_free it), its name text on the device and that text's length */
int kmr_dedup_reads(const kmr_dedup *d, const kmr_reads **consensus, const void **dev_name_text, uint64_t *name_text_len);
/* the name text to host memory (KMR_ERR_CAPACITY if capacity < name_text_len) */
int kmr_dedup_names_copy(const kmr_dedup *d, char *dst, uint64_t capacity);
void kmr_dedup_free(kmr_dedup *d);
/* BaseQual::getQualChar (src/Sequence.cpp:807-819) without FASTQ_START_CHAR: 40 from 0.9999, else (char)(-10. * log10(1.0 - prob)),
 * answered from the 39 doubles at which that expression steps -- the table the device compares against.  prob >= 0.  Needs no device. */
char kmr_consensus_qual(double prob);

/* ---- CompareSpectrums (apps/CompareSpectrums.cpp): the distinct k-mers and the k-mer occurrences two read sets share ----
 *
 * The reference builds both spectra solid-only with TrackingDataMinimal4 (src/KmerTrackingData.h:1132-1212: every occurrence that
 * passes TrackingData::isDiscard, f32 |weight| > min-kmer-quality, adds 1 to a u32; a k-mer over a markup weighs 0 and never passes;
 * no singleton split, no saturation) and reports, for maps m1 and m2 (countCommonKmers :146-162, evaluate :225-242):
 *   size1, size2                   m1.size(), m2.size()
 *   common                         keys of m1 that m2 holds
 *   common_count1, common_count2   sum over those keys of m1's count, and of m2's count
 *   total_count1, total_count2     sum of all counts of m1, and of m2
 *
 * The map a handle stands for is what KmerSpectrum::getCount(kmer, false) answers from (src/KmerSpectrum.h:642-695): the weak entries
 * with their u16 count, plus the singleton entries with count 1 where the handle keeps that map.  A handle built with
 * separate_singletons 0 or 1 and finalized with min_depth <= 1 equals the reference's solid map key for key; one finalized with
 * min_depth 2 compares what it still holds.
 *
 * Saturation: a stored count stops at 65535, the reference's u32 does not.  `saturated` counts the entries read, on either side, whose
 * stored count is 65535: the figures are the reference's whenever it is 0 and lower bounds otherwise.  In the per-read form a read's
 * own counts are exact sums; only map 2's counts can saturate, and `saturated` is the number of map 2's entries at 65535. */
typedef struct kmr_compare_counts {
	uint64_t size1, size2, common, common_count1, common_count2, total_count1, total_count2;
	uint64_t saturated;
} kmr_compare_counts;

/* Set against set (evaluate :225-242): h1's map against h2's.  Both handles must be finalized (KMR_ERR_STATE), on the same device, with
 * the same k and the same hash_kind (KMR_ERR_INVALID_ARG); either value kind is accepted, h1 == h2 is allowed, and the two maps may
 * have different bucket counts.  Runs on h2's stream after h1's work has finished, and waits for the result. */
int kmr_compare_spectrums(kmr_handle *h1, kmr_handle *h2, kmr_compare_counts *out);

/* Every read of a batch on its own against the whole of h2's map (--per-read, evaluatePerRead :243-257, which builds a KmerSpectrum
 * per read): read r is map 1 all by itself -- its keys the canonical k-mers of the read whose occurrences pass the weight test, a
 * key's count the number of such occurrences --, found by the build's own extraction.  k, min_weight, min_quality_score, the quality
 * base and the hash kind are h2's; the batch was ingested through h2 (or a handle of the same configuration), so that its qualities
 * are on the handle's scale.  size2 and total_count2 are the same in every record; a read shorter than k gives a record of zeros apart
 * from those two (and `saturated`).  Records are in read order.  Reads of up to 256 k-mers are answered by one wavefront each out of LDS,
 * longer ones (contigs, genomes) through a radix sort of their (read, k-mer) pairs; the batch is walked in runs of whole reads whose
 * k-mers fit a staging buffer (kmr_tune "compare_lds_kmers", "compare_stage_kmers"); neither changes a result.
 * KMR_ERR_STATE before kmr_finalize; KMR_ERR_UNSUPPORTED for a handle with world_size > 1, num_parts > 1 or kmer_subsample > 1 (the
 * owner-partitioned form adds up over ranks: not built yet), and for a read of 2^32 k-mers or more.
 * kmr_compare_reads: per_read is host memory of n_reads records.  kmr_compare_reads_dev: dev_per_read is device memory of n_reads
 * records, written by work queued on h2's stream (the call itself waits only for the sizes it needs: the batch's k-mers to cut the
 * runs and, where reads take the sorted path, their number per run). */
int kmr_compare_reads(kmr_handle *h2, const kmr_reads *set1, kmr_compare_counts *per_read);
int kmr_compare_reads_dev(kmr_handle *h2, const kmr_reads *set1, void *dev_per_read);

/* The header of CompareSpectrums' table (:211-212) is "\nSet 1\tSet 2\tCommon\t%Uniq1\t%Tot1\t%Uniq2\t%Tot2\n"; this writes one line of it
 * (:234-241, :250-256): size1 \t size2 \t common \t P(common * 100.0 / size1) \t P(common_count1 * 100.0 / total_count1) \t
 * P(common * 100.0 / size2) \t P(common_count2 * 100.0 / total_count2) \t label \n, P being setprecision(4) in the default float
 * format ("%.4g").  A zero denominator is 0.0 / 0.0 at run time in the reference, which an x86-64 glibc build prints as "-nan": that
 * is written here, whatever the host.  The label is empty in the whole form and the read's name in the per-read form.  Host only, needs
 * no device; *bytes is the length of the line (no terminating 0 is written); KMR_ERR_CAPACITY if cap is smaller, with *bytes set. */
int kmr_compare_line(const kmr_compare_counts *c, const char *label, uint64_t label_len, char *dst, uint64_t cap, uint64_t *bytes);

/* ReadSet::circularize (src/ReadSet.cpp:120-130; CompareSpectrums --circular-reference passes extra_length = k, not k - 1, so that the
 * first k-mer of a circular sequence is counted twice): a new batch in which every read is bases + bases[0 : min(extra_length, L)], its
 * qualities extended the same way.  Offsets are rebuilt, the 64 bytes of padding kept, the name spans carried over; an empty read stays
 * empty and extra_length 0 is a copy.  Free the result with kmr_reads_free. */
int kmr_reads_circularize(kmr_handle *h, const kmr_reads *in, uint32_t extra_length, kmr_reads **out);

/* ---- TnfDistance (apps/TnfDistance.cpp): tetranucleotide-frequency vectors of sequences and windows, and the distances between them ----
 *
 * The reference counts the canonical k-mers of a very small k (--kmer-size, default 4) per sequence by building a whole KmerSpectrum for
 * it (buildTnfs :462-484), reads the counts out in the order of a fixed map (TNF::stdMap) and compares the vectors by a Euclidean or a
 * Spearman distance.  The k of every call below is the handle's k, as KmerSizer is global in the reference: a handle created with k = 4 and
 * never fed is enough, none of the calls needs a finalized spectrum, and world_size, num_parts and kmer_subsample do not matter to any of
 * them.  k > 6 is KMR_ERR_UNSUPPORTED (4^6 u32 bins are the 16 KiB of LDS a wavefront counts in; the reference sizes its map "for hexamers").
 *
 * Columns.  D(k) canonical k-mers: 2, 10, 32, 136, 512, 2080 for k = 1 .. 6.  Their order is the iteration order of TNF::stdMap, a KmerMap
 * asked for 2112 buckets, which makes 4096 (getMinPowerOf2, src/Kmer.h:2199-2212): ascending bucket = hash & 4095 of the hash kind over the
 * packed key bytes, and ascending key within a bucket (the map appends and re-sorts a bucket on every insert, src/Kmer.h:3095-3106 with
 * getNumUnsorted :1701-1704).  The order matters to the bits of a distance, because the sums run in it.
 *   kmr_tnf_dims      D(k); KMR_ERR_UNSUPPORTED for k = 0 or k > 6
 *   kmr_tnf_columns   codes[D]: column -> the 2k-bit code of the canonical k-mer, first base in the high bits, A C G T = 0 1 2 3
 *   kmr_tnf_header    "Count\tLength" and "\t<k-mer>" per column (toHeader :295-303), no line end; *bytes is its length,
 *                     KMR_ERR_CAPACITY if cap is smaller (with *bytes set)
 * These three need no device.
 *
 * Vectors.  A kmr_tnf holds n vectors of D counts on the device, for each the sequence it came from, its first base and its number of
 * bases (the origin), its float length, and the bounds of the groups (input files) the vectors fall into.
 *   kmr_tnf_reads       one vector per sequence of the batch (buildTnfs): column c is the number of occurrences of that canonical k-mer
 *                       that pass the build's weight test (TrackingDataMinimal4, as above kmr_compare_counts): a sequence with real
 *                       qualities loses its low-weight k-mers, a FASTA sequence (quality 127) only the k-mers over a markup.  A sequence
 *                       shorter than k is a vector of zeros.  The batch was ingested through h or a handle of its configuration.
 *   kmr_tnf_windows     shredReadByWindow (:486-494) and purgeShortTNFS (:506-518): of a sequence of L bases a window of `window` bases at
 *                       every i = 0, step, 2 step, ... with i < L - window (strictly: L <= window gives none).  Windows carry reference
 *                       quality: every k-mer without a markup counts, whatever the sequence's own qualities.  A window whose counts sum to
 *                       less than min_count is dropped (the tool passes window * 3 / 4); the survivors keep the input order (the
 *                       reference's swap-with-last order shows only in its per-thread .data files).  step >= 1.
 *   input_starts / n_inputs   as for kmr_partition_reads: n_inputs + 1 ascending sequence indices from 0 to n; NULL / 0 = one input.  The
 *                       groups of the result are the inputs.
 *   kmr_tnf_group_sums  one vector per group, the group's vectors added (wholeTnfs :717), each a group of its own.  The reference adds floats
 *                       in read order; here the counts add as u64 and are converted once, which is the same while every sum stays <= 2^24.
 *   kmr_tnf_info        n, D, the number of groups, and `inexact`: the columns (of all vectors) above 2^24, where a float no longer holds
 *                       the count -- the figures are the reference's while it is 0, in the manner of `saturated` above.
 *   kmr_tnf_copy        to host memory, each where the pointer is not NULL: counts[n * D] (vector-major, column order), lengths[n]
 *                       (calcLength / buildLength :396-416: double l += (double)(v * v) with the product in float, (float)sqrt(l), 0
 *                       becomes 1), origin[3 n] (sequence, first base, bases; a group sum: group, 0, 0), group_bounds[groups + 1].
 * Sequences are cut into pieces of bases (kmr_tune "tnf_piece_bases", default 4096) that the wavefronts of the device count separately; it
 * changes no result.  A sequence of 2^32 k-mers or more is KMR_ERR_UNSUPPORTED.
 *
 * Distances, to the bit of an x86-64 build of the reference without -ffast-math (the Release build's -ffast-math is not followed, as for
 * the oracle): no multiply-add is contracted, every sum runs in column order.
 *   KMR_TNF_EUCLIDEAN (getDistance :434-441)   float d = (float)((double)a[i] / (double)la - (double)b[i] / (double)lb);
 *                                              dist = dist + d * d in float; then sqrtf(dist)
 *   KMR_TNF_SPEARMAN (RankVector, src/Utils.h:2090-2160)   ranks 1 .. D, ties (float)tieRankSum / (float)tieSize; mean = (D + 1) / 2 in
 *                                              integer division; three float sums of float products; (1 - sum_xy / sqrtf(sum_x2 * sum_y2)) / 2
 *   kmr_tnf_distances / _dev   with b: rows [first_row, first_row + n_rows) of a against all of b, row-major n_rows x n_b floats (b = one vector
 *                       is the --reference-file form).  With b == NULL: the strict lower triangle of a, row i holding j < i, the rows
 *                       packed: row i begins at i (i - 1) / 2 - first_row (first_row - 1) / 2 (--inter-distance-file, :649-662).
 *                       first_row / n_rows let a caller stream a matrix that does not fit.  out is host memory (_dev: device memory, written
 *                       by work queued on h's stream).  The first distance call of a formula on a vector set makes its per-vector part
 *                       (quotients, or ranks) and keeps it with the set.  a, b and h on one device, same D and hash kind.
 *   kmr_tnf_likelihoods   the whole --intra-inter-file computation (:664-902) over a batch: windows of (window, step) and, where window2 >
 *                       window, of (window2, step2) (window2 < window takes window's values, as the option parser does), each purged at
 *                       3/4; out = four histograms of bins + 2 u64 (GenericHistogram, src/Utils.h:2163-2254: _step = (float)(end - 0) / bins,
 *                       idx = (int)(v / _step) + 1, v > end in the last, end = (float)sqrt(2.0) Euclidean / 1 Spearman): intra, inter,
 *                       intra-vs-whole, inter-vs-whole.  The loops are the reference's: a file with fewer than two surviving windows adds
 *                       nothing to the two intra histograms; equal window sizes take the lower triangle within a file and file pairs j < i,
 *                       different sizes every window against every window2 of the same file and of every other file; every window against
 *                       the group sum of every other file.  No distance is stored.  A distance that is not a number (undefined in the
 *                       reference) is counted in bin 0.  A block the reference would subsample (numSamples >= its share of max_samples, :689-691
 *                       and :827-832; the default, INT64_MAX, never) is refused with KMR_ERR_UNSUPPORTED, naming the block: the reference
 *                       draws from a time-seeded generator there.  1 <= bins <= 4094.
 * Not built: --cluster-file (a serial greedy merge), --include-intra-inter-data-file, the five-part labels of reads within 0.20 of the
 * reference (:560-574), subsampling, k > 6. */
typedef struct kmr_tnf kmr_tnf;
enum kmr_tnf_formula { KMR_TNF_EUCLIDEAN = 0, KMR_TNF_SPEARMAN = 1 };
typedef struct kmr_tnf_likelihood_config {
	uint32_t struct_size;
	uint32_t formula;          /* kmr_tnf_formula */
	uint64_t window, step;     /* --window-size, --window-step */
	uint64_t window2, step2;   /* --window2-size, --window2-step */
	uint32_t bins;             /* --likelihood-bins */
	uint32_t reserved;
	int64_t max_samples;       /* --max-samples */
} kmr_tnf_likelihood_config;
int kmr_tnf_dims(uint32_t k, uint32_t *dims);
int kmr_tnf_columns(uint32_t k, uint32_t hash_kind, uint16_t *codes);
int kmr_tnf_header(uint32_t k, uint32_t hash_kind, char *dst, uint64_t cap, uint64_t *bytes);
int kmr_tnf_reads(kmr_handle *h, const kmr_reads *reads, const uint64_t *input_starts, uint32_t n_inputs, kmr_tnf **out);
int kmr_tnf_windows(kmr_handle *h, const kmr_reads *reads, const uint64_t *input_starts, uint32_t n_inputs, uint64_t window, uint64_t step, int64_t min_count, kmr_tnf **out);
int kmr_tnf_group_sums(kmr_handle *h, const kmr_tnf *tnf, kmr_tnf **out);
int kmr_tnf_info(const kmr_tnf *tnf, uint64_t *n, uint32_t *dims, uint32_t *n_groups, uint64_t *inexact);
int kmr_tnf_copy(const kmr_tnf *tnf, uint64_t *counts, float *lengths, uint64_t *origin, uint64_t *group_bounds);
void kmr_tnf_free(kmr_tnf *tnf);
int kmr_tnf_distances(kmr_handle *h, const kmr_tnf *a, const kmr_tnf *b, int formula, uint64_t first_row, uint64_t n_rows, float *out);
int kmr_tnf_distances_dev(kmr_handle *h, const kmr_tnf *a, const kmr_tnf *b, int formula, uint64_t first_row, uint64_t n_rows, void *dev_out);
/* window 10000, step 1000, window2 10000, step2 1000, 100 bins, Euclidean, max_samples INT64_MAX */
int kmr_tnf_likelihood_config_init(kmr_tnf_likelihood_config *cfg);
int kmr_tnf_likelihoods(kmr_handle *h, const kmr_reads *reads, const uint64_t *input_starts, uint32_t n_inputs, const kmr_tnf_likelihood_config *cfg, uint64_t *out);

/* ---- KmerMatch (src/KmerMatch.h, src/MatcherInterface.h): the reads that share a k-mer with the ends of contigs ----
 *
 * DistributedNucleatingAssembler's matching step: for every contig the reads of the target set that share a k-mer with the first or
 * last match-max-positions-from-edge bases of the contig, sampled where there are too many, with their mates, in ascending order of
 * their global read index.  The reference looks every edge k-mer of a contig up in a spectrum whose values hold every (read, position)
 * instance of the k-mer (TrackingDataWithAllReads, src/KmerTrackingData.h:779-887).  Here the join is turned around: the contigs' edge
 * k-mers are a small table on the device and the reads stream through the build's extraction once per call, probing it.
 *
 * A read r matches contig c exactly when some k-mer occurrence of r passes the build's weight test (TrackingData::isDiscard: f32
 * |weight| > min_weight; a reference-quality read weighs 1, a k-mer over a markup 0; a discarded read gives no k-mers), its canonical
 * key is an edge key of c, and the handle's finalized spectrum holds the key -- which stands for purgeMinDepth(minDepth) of KmerMatch's
 * constructor (KmerMatch.h:100-107, src/KmerSpectrum.h:1805-1815): with min_depth <= 1 the singleton map counts (KmerMatch.h:155-161),
 * with 2 it is gone, above 2 the weak entries below the depth are gone too.  The caller's contract: the handle was built from exactly
 * the reads that are streamed, and finalized with the depth KmerMatch would get.
 *
 * Contig k-mers (KmerMatch.h:136, src/Kmer.h:885, KmerWeights(twoBit, len, true)): every window of the packed sequence, canonical, no
 * weights, qualities or markups -- a non-ACGT base is the 2-bit code 0 ('A'), and a window over an N is still looked up.  A contig
 * shorter than k has no k-mers and an empty result.
 * Edge windows (KmerMatch.h:124-149): with M = max_positions_from_edge - k + 1 as an int and n k-mers, k-mer j is considered if
 * j <= (unsigned)M || j >= upperMinKmer, upperMinKmer = n - M if (int)n > M and 0 otherwise.  So the left side takes M + 1 k-mers and
 * the right side M (the reference's asymmetry), M = 0 takes the first k-mer only, and M < 0 (an edge setting below k - 1, 0 included)
 * takes every k-mer, (unsigned)M being huge.
 * Hit set (:114-120): a contig's hits are a set of global read indices (first_global_read_idx + index in the batch); a key that lies
 * in several contigs gives the read to each.
 * Sampling (KmerMatch.h:127,168-171, MatcherInterface.h:280-287): a set of size > maxHits reads, maxHits = 2.0f * max_read_matches,
 * keeps a read when u <= maxHits / (float)size, in f32.  The reference draws u from a time-seeded uniform_01<float>; here
 * u = (float)(draw >> 8) * 2^-24, draw = word 0 of Philox4x32-10 over the counter (read & 0xffffffff, read >> 32, contig index, 1)
 * and the key (seed & 0xffffffff, seed >> 32), so that a result repeats and does not depend on how the reads are cut into batches.
 * size is the set's size over all batches: the sampling happens in kmr_match_finish.  max_read_matches = 0 means no sampling, as the
 * option's help says (the reference's code would keep almost nothing then: the fraction is 0).
 * Mates (MatcherInterface.h:772-792): with include_mate and a pairing given, the mate of every read that survived the sampling joins
 * the set (the mates of sampled-away reads do not).
 * Result (MatcherInterface.h:311-321): every set in ascending global read index without the reads whose discard flag is set -- a
 * discarded read never hits, but it can come in as a mate.
 * Not built: the second cut to exactly 20 * max_read_matches reads (Random::sample, :304), --max-read-depth-matches, the overhang screen
 * through KmerAlign (return-overlap-only, :599-662) and the Vmatch back-end.  The sizes before and after sampling are reported per
 * contig, so that a caller can apply a cut of its own.
 * Bounds: at most 2^24 contigs, each shorter than 2^31 - 1 bases, fewer than 2^32 - 1 edge k-mers in all, global read indices below 2^40,
 * fewer than 2^32 - 1 hit records: KMR_ERR_UNSUPPORTED beyond. */
typedef struct kmr_match_config {
	uint32_t struct_size;
	int32_t max_positions_from_edge;      /* --match-max-positions-from-edge, 500 */
	uint32_t max_read_matches;            /* --max-read-matches, 450; 0 = no sampling */
	uint32_t include_mate;                /* --include-mate, 1 */
	uint64_t seed;                        /* of the sampling's random numbers, 0 */
} kmr_match_config;
typedef struct kmr_match kmr_match;
int kmr_match_config_init(kmr_match_config *cfg);
/* The table of the contigs' edge keys (KmerMatch.h:124-149), filtered against h's spectrum once.  KMR_ERR_STATE before kmr_finalize;
 * KMR_ERR_UNSUPPORTED for a handle that holds part of a spectrum (world_size > 1, num_parts > 1, kmer_subsample > 1);
 * KMR_ERR_INVALID_ARG for contigs of another device.  The object refers to h, which must outlive it; free it with kmr_match_free. */
int kmr_match_create(kmr_handle *h, const kmr_reads *contigs, const kmr_match_config *cfg, kmr_match **out);
/* contigs, considered k-mers (with repeats), distinct keys among them, and those of them the spectrum holds; any may be NULL */
int kmr_match_edge_info(const kmr_match *m, uint64_t *n_contigs, uint64_t *n_edge_kmers, uint64_t *n_distinct_keys, uint64_t *n_keys_in_spectrum);
/* Stream one batch of the target reads (_matchLocal's lookups :151-161 from the reads' side); may be called repeatedly.  pairs: the
 * batch's own pairing (kmr_identify_pairs), NULL = no mates; discarded: host array of one flag per read, NULL = none.  Waits for the
 * batch's hit count; if the hit buffers were too small they grow and the batch is streamed again (kmr_tune "match_hit_capacity").
 * KMR_ERR_STATE after kmr_match_finish; KMR_ERR_INVALID_ARG for a batch or pairing of another device or another number of reads. */
int kmr_match_add_read_batch(kmr_match *m, const kmr_reads *reads, uint64_t first_global_read_idx, const kmr_pairs *pairs, const uint8_t *discarded);
/* sets made unique, sampled, mates added, sorted, discarded reads dropped (KmerMatch.h:163-171, MatcherInterface.h:772-792, :311-321) */
int kmr_match_finish(kmr_match *m);
/* after kmr_match_finish (KMR_ERR_STATE before): contigs, reads of all sets, contigs whose set was sampled; any may be NULL */
int kmr_match_info(const kmr_match *m, uint64_t *n_contigs, uint64_t *n_reads_total, uint64_t *n_sampled_contigs);
/* offsets (n_contigs + 1), read_ids (n_reads_total: contig i's reads are read_ids[offsets[i] .. offsets[i + 1]), ascending), and per
 * contig the set's size before sampling and after it (before the mates join); any may be NULL.  KMR_ERR_STATE before kmr_match_finish */
int kmr_match_copy(const kmr_match *m, uint64_t *offsets, uint64_t *read_ids, uint64_t *size_before_sampling, uint64_t *size_after_sampling);
/* the same four arrays (uint64) where they lie; any may be NULL; valid until kmr_match_free */
int kmr_match_device_ptrs(const kmr_match *m, void **dev_offsets, void **dev_read_ids, void **dev_size_before_sampling, void **dev_size_after_sampling);
void kmr_match_free(kmr_match *m);

/* ---- ContigExtender (src/ContigExtender.h:157-247, src/KmerSpectrum.h:2311-2373): the other half of a round of
 * DistributedNucleatingAssembler (apps/DistributedNucleatingAssembler.cpp:230-275) -- every contig walks outwards base by base while the
 * k-mer spectrum of its own pool of reads agrees.  All (contig, pool) pairs of a call are worked on at once (kmr_extend.hpp).
 *
 * Pool spectrum: buildKmerSpectrum(pool, false) under h's config -- min_weight, the quality settings, separate_singletons; h supplies k
 * and that config only and need not have been fed.  world_size, num_parts and kmer_subsample are not applied.  A key's value is
 * getWeightedCount() (use_weights) or getCount(); the weighted count is an f32 that takes one f32 addition per sighting in the serial
 * order (pool order, then position), the first sighting quantised through the singleton map's byte where that map is on; with it on a
 * key seen once is invisible, since extendContig reads the weak map only.  No purgeMinDepth.
 * One step (extendContig): the contig must be longer than k; the edge k-mer is the first or last k bases as compressSequence packs
 * them (a non-ACGT base is the code 0, 'A'; lower case is upper case); its canonical key's value, as a double, must not be 0.0; the
 * four one-base extensions in the order A, C, G, T, canonical, are summed in that order into total; the step goes on if
 * total >= minimum_coverage && total / edge > maximum_delta_ratio; the first i with value[i] / total >= minimum_consensus / 100 is
 * taken, and the step ends without a base if that candidate key is in the contig's solid spectrum: the contig's own k-mers that pass
 * the weight test at quality Read::REF_QUAL, plus the new edge k-mer of every step of this call on either side (recordKmer).
 * One contig (extendContigs with minKmerSize == maxKmerSize == k): while (iteration++ < max_extend && (left | right)), left before
 * right, a side that failed is not tried again, a contig shorter than k ends the loop.  The multi-k form of extendContigs (spectra
 * built with kmerStep but walked with += 2, freed by a shifted index) is not built: the assembler never takes it.
 * Stop records: per contig and side why the side stopped and the f64 values of the last step it tried (zero where the step did not
 * get that far) -- the reference's debug lines.
 * Result: the sequences as Read::getFasta gives them (ACGT in upper case, '.' as 'N', other markups as they are) with the new bases,
 * all of quality Read::REF_QUAL, as a read batch without names that kmr_match_create and a further kmr_extend_contigs take.
 * Bounds: k <= 128 as everywhere; max_extend <= KMR_EXTEND_MAX_EXTEND, fewer than 2^31 contigs, fewer than 2^32 - 1 pooled reads and
 * contigs, sequences shorter than 2^31 - 1 bases: KMR_ERR_UNSUPPORTED beyond. */
#define KMR_EXTEND_MAX_EXTEND 65536u
enum kmr_extend_stop_reason {
	KMR_EXTEND_STOP_LIMIT = 0,        /* the iteration limit: the side was still growing */
	KMR_EXTEND_STOP_SHORT = 1,        /* the contig is not longer than k */
	KMR_EXTEND_STOP_NO_EDGE = 2,      /* the edge k-mer has no value in the pool's weak map */
	KMR_EXTEND_STOP_COVERAGE = 3,     /* total < minimum_coverage or total / edge <= maximum_delta_ratio */
	KMR_EXTEND_STOP_AMBIGUOUS = 4,    /* no extension reaches minimum_consensus */
	KMR_EXTEND_STOP_REPEAT = 5,       /* the chosen k-mer is in the contig's solid spectrum */
	KMR_EXTEND_STOP_INACTIVE = 6      /* the contig's `active` flag is 0: it was not looked at */
};
typedef struct kmr_extend_config {
	uint32_t struct_size;
	uint32_t max_extend;              /* maxExtend, 50 */
	double minimum_consensus;         /* --minimum-consensus in percent, 85 */
	double minimum_coverage;          /* --minimum-coverage, 4.8 */
	double maximum_delta_ratio;       /* --maximum-delta-ratio, 0.33 */
	uint32_t use_weights;             /* TrackingData::useWeighted(), 1 */
	uint32_t reserved;
} kmr_extend_config;
typedef struct kmr_extend_stop {
	uint32_t reason, reserved;        /* kmr_extend_stop_reason */
	double edge, ext[4], total;       /* of the last step the side tried */
} kmr_extend_stop;
typedef struct kmr_extend kmr_extend;
int kmr_extend_config_init(kmr_extend_config *cfg);
/* contigs and reads: batches of h's device (KMR_ERR_INVALID_ARG otherwise).  Contig i's pool: reads pool_reads[pool_offsets[i] ..
 * pool_offsets[i + 1]) of `reads`, in that order; a read may sit in many pools.  pool_offsets must start at 0 and ascend, every pool
 * index must lie in the batch (KMR_ERR_INVALID_ARG).  active: one byte per contig, 0 = leave the contig as it is; NULL = all.  The
 * three arrays are host memory here and device memory in the _dev form (e.g. kmr_match_device_ptrs' offsets, and its read ids once
 * the caller has made them local to `reads`).  Free the result with kmr_extend_free. */
int kmr_extend_contigs(kmr_handle *h, const kmr_reads *contigs, const kmr_reads *reads, const uint64_t *pool_offsets, const uint64_t *pool_reads, const uint8_t *active,
                       const kmr_extend_config *cfg, kmr_extend **out);
int kmr_extend_contigs_dev(kmr_handle *h, const kmr_reads *contigs, const kmr_reads *reads, const void *dev_pool_offsets, const void *dev_pool_reads, const void *dev_active,
                           const kmr_extend_config *cfg, kmr_extend **out);
/* contigs, contigs that grew, bases added in all; any may be NULL */
int kmr_extend_info(const kmr_extend *e, uint64_t *n_contigs, uint64_t *n_extended, uint64_t *bases_added);
/* per contig the new length and the bases added on the left and on the right; stops: two records per contig, left then right; any may
 * be NULL.  All arrays are host memory */
int kmr_extend_copy(const kmr_extend *e, uint32_t *new_len, uint32_t *left, uint32_t *right, kmr_extend_stop *stops);
/* the new sequences (owned by e: do not kmr_reads_free them) */
int kmr_extend_reads(const kmr_extend *e, const kmr_reads **reads);
void kmr_extend_free(kmr_extend *e);
/* ContigExtender::getNewName (src/ContigExtender.h:249-268), byte for byte: find_last_of("-l") finds the last '-' OR 'l'; host work, no
 * device.  Writes the NUL-terminated name to buf; KMR_ERR_CAPACITY if it does not fit cap bytes */
int kmr_extend_new_name(const char *old_name, uint64_t left, uint64_t right, char *buf, uint64_t cap);
/* ContigExtender::getMinMaxKmerSize (:269-279) from the option's k-mer size, the longest read, the bases and the number of reads */
int kmr_extend_min_max_kmer_size(uint32_t kmer_size, uint32_t max_sequence_length, uint64_t base_count, uint64_t n_reads, uint32_t max_steps,
                                 uint32_t *min_kmer_size, uint32_t *max_kmer_size, uint32_t *kmer_step);

/* Raw HIP stream of the handle (hipStream_t) so callers can order their own
 * work (torch.cuda.ExternalStream) against it. */
void *kmr_stream(kmr_handle *h);

/* Implementation knobs of one handle; none of them changes a result.  They exist so that tests reach the multi-level,
 * retry and sub-batch code with small inputs and measurement tools can sweep a parameter; the library reads no
 * environment variable.  Knobs (value): "target_list_records" (records per final list the partition bits aim for, 2048),
 * "sub_batch_bases" (bases per extract launch, 0 = default), "recycle_chunks" (-1 auto, 0, 1), "partition_blocks"
 * (0 = one per CU), "entry_share" (initial entry-buffer share of the count pass, < 0 = from the probe), "lookup_table",
 * "narrow_tallies", "keep_level1_state" (1 / 0), "superkmer_minimizer" (minimizer length of build_mode 3, 0 = default),
 * "stream_lookups" (1: kmr_score_* gets its k-mer counts from a streaming pass over minimizer lists where k allows it; 0: per-k-mer
 * probes of the lookup table; a batch that holds a base which is neither ACGT nor N, X or '.' is probed whatever this says, see kmr_score_reads), "long_list_chunks" (super-k-mer lists of more 1 KB chunks are counted / looked up in pieces, 1024), "coarse_lists" (owner exchange:
 * 1 = scatter into and exchange coarse lists that the owner splits before the count pass, 0 = the job's fine lists; default 0).
 *   "pow2_lists" (1: the list count of build_mode 3 is always a power of two; default 0: a single GPU's build takes est / list_aim lists),
 *   "list_aim" (k-mers per list that count aims for; default 1450 when every k-mer weighs the same, 1700 raw k-mers otherwise, 800 with
 *   extension values, just below the table's bound for keys of more than one word), "packed_direct" (0: kmr_add_reads_twobit* always
 *   unpack to text first).
 *   "uniform_count" (0: never the one-weight form of the count pass), "lean_extract" (0: never the bases-only extraction),
 *   "count_blocks" (blocks per compute unit of the one-weight count pass over lists of one-word keys: 4, 5 -- its instance compiled for
 *   96 registers -- or 0, the default choice; every other form of the count pass runs as before whatever this says; anything else is
 *   KMR_ERR_INVALID_ARG; see kmr_build_info "count_blocks"; may be set at any time),
 *   "count_six" (the six-block instance of that pass -- table slots of 20 bytes, whose first-sighting word holds a 32-bit ordinal relative
 *   to the build's lowest -- where "count_blocks" is 0: 0 = the default: taken when every record was stamped by this handle's own
 *   kmr_add_reads* calls, their stream ordinals span less than 2^31 and the build has at least compute units x 6 x 24 lists; 1 = taken
 *   wherever the ordinals allow it, whatever the list count; 2 = never; anything else is KMR_ERR_INVALID_ARG; may be set at any time),
 *   "superkmer_window" (the widest minimizer window build_mode 3 may take: 32 (k >= 45) / 16 / 8 / 4).
 *   "early_entry_share" (>= 0: kmr_count_lists_prefix's entry buffers hold that share of the good k-mers + 16 384 entries; < 0 = from the
 *   list share, the default), "saturated_batch_bytes" (scratch budget of one batch of kmr_finalize's ordered pass over k-mers seen 256
 *   times or more, 0 = 1 GiB; a key whose sightings alone exceed it is a batch of its own).
 *   "select_timing" (1: kmr_select_reads* / kmr_filter_read_batch* / kmr_partition_* / kmr_normalize_* time their phases with HIP events, see kmr_build_info; default 0).
 *   "partition_units" (most wavefronts, each over a contiguous range of reads, that kmr_select_reads* / kmr_filter_read_batch* / kmr_partition_* deal the batch to
 *   (kmr_normalize_*: its 2 n slots), 1 - 8192; 0 = the default, 4096 (kmr_normalize_*: 8192) unless there are many segments; tests set a few so that one wavefront walks many tiles of 64 reads; may be set at any time).
 *   "dump_timing" (1: kmr_dump_text_size / kmr_dump_text time their size pass and writer with HIP events, see kmr_build_info; default 0),
 *   "dump_piece_bytes" (staging bound of one piece of kmr_dump_mercount / kmr_dump_mergraph's file, 0 = KMR_DUMP_PIECE_BYTES; may be set at any time).
 *   "dump_tiles_per_block" (32 KiB tiles of the text that one block of kmr_dump_text's writer walks, 0 = the default, as many as leave 16 blocks
 *   a compute unit; tests set 1, 2, 3 or more than the text has so that a small text takes the writer's tile-to-tile hand-off; changes no
 *   byte of the text; see kmr_build_info; may be set at any time).
 *   "pair_hash_bits" (bits of the common name's hash that kmr_identify_pairs* sorts by, 1 - 64, default 64: with a few bits distinct names
 *   share a key, which tests use to reach the byte-for-byte grouping), "pairs_timing" (1: kmr_identify_pairs* times its phases with HIP
 *   events, see kmr_build_info; default 0); both may be set at any time.
 *   "dedup_timing" (1: kmr_dedup_fragments* times its phases with HIP events, see kmr_build_info; default 0; may be set at any time).
 *   "artifact_report_lds" (where kmr_artifact_filter_report* / kmr_artifact_filter_apply_report* sum the per-sequence counters: 1 = per unit in LDS
 *   first, while 24 bytes a sequence index fit 48 KiB, 0 = global 64-bit atomics, anything else = the default, LDS while they fit 6 KiB; tests force
 *   either; see kmr_build_info; may be set at any time).
 *   "csr_partition" (how kmr_finalize, kmr_count_lists_prefix and the streaming lookups find every list's chunks: 1, the default, by a radix
 *   partition of the (list, chunk) pairs, 0 by one device atomic per chunk, which builds of more than 2^24 lists take anyway; see
 *   kmr_build_info "csr_path"; may be set at any time).
 *   "compare_lds_kmers" (kmr_compare_reads*: the most k-mers of a read that one wavefront answers out of LDS, 1 - 512; 0 sends every read
 *   through the sorted path; anything else = the default, 256), "compare_stage_kmers" (k-mers of one run of whole reads of
 *   kmr_compare_reads*, 0 = 2^26; a read that alone exceeds it is a run of its own); both may be set at any time.
 *   "tnf_piece_bases" (kmr_tnf_reads / kmr_tnf_windows / kmr_tnf_likelihoods: bases of one piece of a sequence, the unit the wavefronts share
 *   out, 0 = 4096; tests set 64 or 65 so that a short input crosses piece edges; may be set at any time).
 *   "match_hit_capacity" (hit records the buffers of a kmr_match hold before they first grow, 0 = 2^20; tests set a few so that a handful
 *   of reads overflows them and the batch is streamed again; read by kmr_match_add_read_batch; may be set at any time).
 *   "extend_stage_kmers" (k-mers of one run of whole contigs with their pools of kmr_extend_contigs*, 0 = 2^24; a contig whose pool alone
 *   exceeds it is a run of its own; tests set a few hundred so that a call takes several runs), "extend_timing" (1: kmr_extend_contigs*
 *   times its phases with HIP events and waits after every run, see kmr_build_info; default 0); both may be set at any time.
 * Call before the first kmr_add_reads* of a build.  KMR_ERR_INVALID_ARG for an unknown knob. */
int kmr_tune(kmr_handle *h, const char *knob, double value);
/* What the current build decided, for tests and measurement tools (the reference logs such figures, LOG_VERBOSE): "lists" = super-k-mer
 * lists of the build (0 before the first reads, or in another build mode), "uniform_count" = 1 if the last kmr_finalize ran the
 * count pass's one-weight form, "count_blocks" = blocks per compute unit the last launch of the count pass over lists (kmr_finalize or
 * kmr_count_lists_prefix) was sized for: 5 or 6 where kmr_tune "count_blocks" / "count_six" or the default chose the five- or the six-block instance, else 4, "chunk_pool_chunks" = 1 KB chunks the pool holds, "superkmer_window" = the minimizer window in use, "early_lists" / "early_entries" = the bound below which the last
 * kmr_finalize took its lists' entries from kmr_count_lists_prefix (0: it counted everything itself) and how many entries those were,
 * "early_overflowed" = 1 if the last kmr_finalize voided an early count because its buffers had overflowed, "saturated_keys" /
 * "saturated_batches" = the weak entries of count 256 or more the last kmr_finalize of build_mode 3 redid in input order (all of them,
 * every time) and in how many batches, "count_attempts" = how often the last kmr_finalize of build_mode 2 or 3 ran its count pass before
 * the entries fit their buffers (1 unless the first sizes were too small; kmr_tune "entry_share" forces that in tests), "bb_path" = how the last kmr_finalize bucketed the weak map (0: per-bucket scatter and sort, 1: radix
 * partition with measured bins, 2: with bins of one capacity), "bb_fallback" = 1 if a bin overflowed its capacity and the map was made again
 * with measured bins, "score_path" = where the last kmr_score_reads / kmr_score_read_batch / kmr_filter_read_batch* on this handle got its
 * k-mer counts (0: none yet, 1: the streaming pass, 2: per-k-mer probes because the handle or kmr_tune "stream_lookups" says so, 3: probes
 * because the batch holds a markup other than N, X and '.'),
 * "device_blocks_live" = blocks of device memory the library holds at this moment in the whole process (every handle, read batch
 * and artifact filter; not only h's), "filter_score_ms" / "select_ms" / "select_write_ms" = HIP-event times of the last kmr_filter_read_batch* /
 * kmr_select_reads* on this handle: its scoring, its selection with the writer, the writer alone (0 unless kmr_tune "select_timing" is set),
 * "dump_size_ms" / "dump_write_ms" = HIP-event times of the last kmr_dump_text_size / kmr_dump_text on this handle: its size pass with
 * the scan, its writer (0 unless kmr_tune "dump_timing" is set), "dump_tiles_per_block" / "dump_blocks" = tiles per block and blocks of the
 * writer of the last kmr_dump_text on this handle that made a text (a block of more than one tile took the hand-off), "pairs_ms" / "pairs_parse_ms" / "pairs_sort_ms" = HIP-event times of the
 * last kmr_identify_pairs* on this handle: the whole call, its name parse, its radix sort (0 unless kmr_tune "pairs_timing" is set),
 * "pair_hash_collisions" = runs of equal sort keys of that call that held more than one distinct common name,
 * "dedup_ms" / "dedup_key_ms" / "dedup_sort_ms" / "dedup_consensus_ms" = HIP-event times of the last kmr_dedup_fragments* on this
 * handle: the whole call, its key kernel, its radix sorts, its consensus kernel (0 unless kmr_tune "dedup_timing" is set),
 * "artifact_report_lds" = 1 if the last kmr_artifact_filter_report* / kmr_artifact_filter_apply_report* on this handle summed its counters in LDS, 0 if by
 * global atomics,
 * "csr_path" / "csr_chunks" = how the last chunk index of this handle was made (1: radix partition, 0: an atomic per chunk, -1: none yet) and
 * how many chunks of the pool it looked at, "unit_batches" = batches fed to this handle so far that held a read longer than an extraction
 * tile and were cut into work units, "match_add_attempts" = how often the last kmr_match_add_read_batch on this handle streamed its
 * batch before the hit records fit their buffers (1 unless they had to grow), "extend_runs" = the runs of whole contigs the last
 * kmr_extend_contigs* on this handle took, "extend_gather_ms" / "extend_extract_ms" / "extend_sort_ms" / "extend_reduce_ms" /
 * "extend_walk_ms" = HIP-event times of that call: the gathered batch with its slot scan, the extraction into the staging array, the
 * radix sort passes, the reduce with its scans and tables, extend_contigs_kernel (0 unless kmr_tune "extend_timing" is set).
 * KMR_ERR_INVALID_ARG for an unknown name. */
int kmr_build_info(kmr_handle *h, const char *what, double *value);

/* Timing of the hot path measured with HIP events on the handle's stream
 * (used by bench.py for the roofline object).  Returns the accumulated
 * milliseconds and the number of timed launch groups since the last reset.
 * Groups 0 and 1 span whole phases, the others single kernels of the
 * streaming build path (they nest inside 0 and 1). */
enum kmr_time_group {
	KMR_TIME_BUILD = 0,       /* kmr_add_reads*: extract + insert / level-1 partition, per sub-batch */
	KMR_TIME_FINALIZE = 1,    /* kmr_finalize: everything                                           */
	KMR_TIME_EXTRACT = 2,     /* extract_kernel launches                                             */
	KMR_TIME_PARTITION1 = 3,  /* level-1 partition launches                                          */
	KMR_TIME_PARTITION2 = 4,  /* level-2 partition launch                                            */
	KMR_TIME_COUNT = 5,       /* count pass                                                          */
	KMR_TIME_BUCKETS = 6,     /* bucket scan + entry scatter + bucket sort                           */
	KMR_TIME_EXCHANGE = 7,    /* kmr_exchange_add_reads_dev: the all-to-all of list chunks / k-mer records (RCCL)   */
	KMR_TIME_GROUPS = 8
};
int kmr_kernel_time(kmr_handle *h, int which, double *ms, uint64_t *launches);
int kmr_kernel_time_reset(kmr_handle *h);

uint32_t kmr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* KMERNATOR_AMD_H_ */
