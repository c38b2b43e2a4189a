/*
 * kmernator_amd.hpp -- C++ host side above the C-ABI (include/kmernator_amd.h), for callers that do not
 * pull in Kmernator's own headers (those need Boost; the binding for a Kmernator checkout is
 * kmernator_amd_shim.hpp).  Method names, argument meaning and error behaviour follow the reference:
 *
 *   kmernator::KmerSpectrum   KmerSpectrum<So,We,Si>                       src/KmerSpectrum.h
 *     buildKmerSpectrum       buildKmerSpectrum(const ReadSet&)           :2081-2115 (flat arrays or a device ReadSet)
 *     purgeMinDepth           purgeMinDepth + optimize                     :1805-1815, :460-466
 *     getCount                getCount(kmer, false)                        :701-725
 *     getCount(.., useWeights) getCount(kmer, useWeights) as double         :670-691, :701-716
 *     getRawKmers ...         :455-459
 *     subtractReference       :472-474
 *     getHistogram            Histogram(256).set(*this) + toString         :909-1071
 *     storeMmap / restoreMmap :476-518 (file naming: <name>, <name>-singleton)
 *     dumpCounts / dumpGraphs MeraculousDistributedKmerSpectrum            src/Meraculous.h:107-134
 *     scoreAndTrimReads       ReadSelector::scoreAndTrimReads              src/ReadSelector.h:1182-1207
 *     setBimodalSigmas        ReadSelector::_bimodalSigmas (--bimodal-sigmas) src/ReadSelector.h:981-1008
 *     countCommonKmers        countCommonKmers + evaluate                  apps/CompareSpectrums.cpp:146-162, :225-242
 *     compareReads            evaluatePerRead                              apps/CompareSpectrums.cpp:243-257
 *   kmernator::ReadSet        ReadSet::appendFastq... on the device        src/ReadSet.cpp:311-345
 *
 * Errors surface as kmernator::KmerSpectrumError (the reference throws LoggedException, src/Log.h:442-484).
 * Header only; link with -lkmernator_amd.
 */
#ifndef KMERNATOR_AMD_HPP_
#define KMERNATOR_AMD_HPP_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <memory>
#include <string>
#include <vector>

#include "kmernator_amd.h"

namespace kmernator {

struct KmerSpectrumError : std::runtime_error {
	int code;
	KmerSpectrumError(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};

class KmerSpectrum;

/* KmerSpectrum::Histogram: buckets filled on the device, finish()/toString() as :986-1035 */
class Histogram {
public:
	unsigned int zoomMax; double logBase;
	std::vector<uint64_t> visits, visitedCount, cumulativeVisits; std::vector<double> visitedWeight;
	uint64_t count = 0; double totalCount = 0, totalWeightedCount = 0; unsigned int lastBucket = 0;
	Histogram(unsigned int z, double b) : zoomMax(z), logBase(b) {}
	unsigned int getBucketValue(unsigned int idx) const {
		const unsigned int skip = (unsigned int)(std::log((double)zoomMax + 1.0) / std::log(logBase) - 1.0);
		return idx <= zoomMax ? idx : (unsigned int)std::pow(logBase, (double)(idx + skip - zoomMax));
	}
	void finish() {
		count = 0; totalCount = totalWeightedCount = 0; lastBucket = 0;
		cumulativeVisits.assign(visits.size(), 0);
		for (size_t i = visits.size(); i-- > 0;) {
			cumulativeVisits[i] = count += visits[i];
			if (visits[i]) { totalCount += (double)visitedCount[i]; totalWeightedCount += visitedWeight[i]; if (i > lastBucket) lastBucket = (unsigned int)i; }
		}
	}
	std::string toString() {
		finish();
		std::ostringstream ss; ss.setf(std::ios::fixed); ss.precision(3);
		ss << "Counts, Weights and Directions\n";
		ss << "Counts:\t" << count << "\t" << totalCount << "\t" << (totalCount / count) << "\t\n";
		ss << "Weights:\t" << count << "\t" << totalWeightedCount << "\t" << (totalWeightedCount / count) << "\t" << (totalWeightedCount / totalCount) << "\n\n";
		ss << "Bucket\tCumulative\tUnique\t%Unique\tCount\t%Count\tWeight\tQualProb\t%Weight\n";
		for (unsigned int i = 1; i < lastBucket + 1; i++)
			ss << getBucketValue(i) << "\t" << cumulativeVisits[i] << "\t" << visits[i] << "\t" << 100.0 * visits[i] / count << "\t" << visitedCount[i] << "\t"
			   << 100.0 * visitedCount[i] / totalCount << "\t\t" << visitedWeight[i] << "\t" << visitedWeight[i] / visitedCount[i] << "\t" << 100.0 * visitedWeight[i] / totalWeightedCount << "\t\n";
		return ss.str();
	}
};

/* reads parsed from FASTQ text on the device, bound to the device of the spectrum that parsed them */
class ReadSet {
public:
	ReadSet(KmerSpectrum &sp, const std::string &fastqText, uint32_t inputQualityBase = 0, bool storeComment = true);
	/* FASTA text, or a FASTA + QUAL pair (qualText != nullptr), parsed on the device: kmr_ingest_fasta */
	static std::unique_ptr<ReadSet> fromFasta(KmerSpectrum &sp, const std::string &fastaText, const std::string *qualText = nullptr, bool storeComment = true);
	~ReadSet() { kmr_reads_free(_r); }
	ReadSet(const ReadSet &) = delete; ReadSet &operator=(const ReadSet &) = delete;
	uint64_t getSize() const { return _n; }
	uint64_t getBaseCount() const { return _bases; }
	uint32_t getInputQualityBase() const { return _qbase; }
	uint64_t getFiltered() const { return _filtered; }
	std::string getName(uint64_t i) const { return _text.substr(_nameOff[i], _nameLen[i]); }
	const kmr_reads *raw() const { return _r; }
private:
	friend class FilterKnownOddities;
	friend class ReadSelector;
	friend class ContigExtender;
	ReadSet(const std::string &text, kmr_reads *r) : _text(text), _r(r) { load(); }      /* a batch the library derived from another one */
	void load();
	std::string _text; kmr_reads *_r = nullptr; uint64_t _n = 0, _bases = 0, _filtered = 0; uint32_t _qbase = 0;
	std::vector<uint64_t> _nameOff; std::vector<uint32_t> _nameLen;
};

class KmerSpectrum {
public:
	enum ScoringType { KS_SUM = 0, KS_MEDIAN = 1, KS_MIN = 2, KS_MAX = 3, KS_AVG = 4 };
	static kmr_config defaults(uint32_t k, uint64_t estimatedRawKmers) { kmr_config c; kmr_config_init(&c); c.k = k; c.estimated_raw_kmers = estimatedRawKmers; return c; }
	explicit KmerSpectrum(const kmr_config &cfg) : _cfg(cfg) {
		const int rc = kmr_create(&cfg, &_h);
		if (rc != KMR_OK) throw KmerSpectrumError(rc, std::string("kmr_create: ") + kmr_last_error(nullptr));
	}
	~KmerSpectrum() { kmr_destroy(_h); }
	KmerSpectrum(const KmerSpectrum &) = delete; KmerSpectrum &operator=(const KmerSpectrum &) = delete;

	uint32_t k() const { return _cfg.k; }
	uint32_t keyBytes() const { return (_cfg.k + 3) / 4; }
	kmr_handle *raw() { return _h; }
	const kmr_config &config() const { return _cfg; }

	void reset() { check(kmr_reset(_h), "kmr_reset"); }
	void buildKmerSpectrum(const char *bases, const char *quals, const uint64_t *offsets, uint64_t nReads, uint64_t firstReadIdx = 0, const uint8_t *discarded = nullptr) {
		check(kmr_add_reads(_h, bases, quals, offsets, nReads, firstReadIdx, discarded), "kmr_add_reads");
	}
	void buildKmerSpectrum(const ReadSet &reads, uint64_t firstReadIdx = 0) { check(kmr_add_read_batch(_h, reads.raw(), firstReadIdx), "kmr_add_read_batch"); }
	/* N GPUs, one process (or thread) per GPU, no MPI: DistributedKmerSpectrum::buildKmerSpectrum (src/DistributedFunctions.h:340-458)
	 * over RCCL inside the library.  Rank 0 makes the id and the host hands it to the others; config.rank / world_size say who is who;
	 * every rank calls buildKmerSpectrumExchange the same number of times (nullptr: no reads this round), then purgeMinDepth. */
	static std::vector<uint8_t> exchangeUniqueId() {
		std::vector<uint8_t> id(KMR_EXCHANGE_ID_BYTES);
		const int rc = kmr_exchange_unique_id(id.data());
		if (rc != KMR_OK) throw KmerSpectrumError(rc, std::string("kmr_exchange_unique_id: ") + kmr_last_error(nullptr));
		return id;
	}
	void exchangeInit(const std::vector<uint8_t> &id) {
		if (id.size() != KMR_EXCHANGE_ID_BYTES) throw KmerSpectrumError(KMR_ERR_INVALID_ARG, "exchangeInit: the id has KMR_EXCHANGE_ID_BYTES bytes");
		check(kmr_exchange_init(_h, id.data()), "kmr_exchange_init");
	}
	void buildKmerSpectrumExchange(const ReadSet *reads, uint64_t firstReadIdx = 0) { check(kmr_exchange_add_read_batch(_h, reads ? reads->raw() : nullptr, firstReadIdx), "kmr_exchange_add_read_batch"); }
	void subtractReference(KmerSpectrum *other) { check(kmr_subtract_reference(_h, other ? other->_h : nullptr), "kmr_subtract_reference"); }
	void purgeMinDepth(uint32_t minDepth) { check(kmr_finalize(_h, minDepth), "kmr_finalize"); }

	kmr_stats stats() { kmr_stats s; check(kmr_get_stats(_h, &s), "kmr_get_stats"); return s; }
	uint64_t getRawKmers() { return stats().raw_kmers; }
	uint64_t getRawGoodKmers() { return stats().raw_good_kmers; }
	uint64_t getUniqueKmers() { return stats().unique_kmers; }
	uint64_t getSingletonKmers() { return stats().singleton_kmers; }

	/* packed canonical k-mers, keyBytes() each */
	std::vector<uint32_t> getCount(const std::vector<uint8_t> &packedKmers) {
		std::vector<uint32_t> out(packedKmers.size() / keyBytes());
		if (!out.empty()) check(kmr_lookup(_h, packedKmers.data(), out.size(), out.data()), "kmr_lookup");
		return out;
	}
	/* getCount(kmer, useWeights): with useWeights the weak entry's weightedCount, else the singleton's (_weight - 1) / 254,
	 * else 0 (the reference's default, TrackingData::useWeightedByDefault); without, the counts above as double */
	std::vector<double> getCount(const std::vector<uint8_t> &packedKmers, bool useWeights) {
		if (!useWeights) { const std::vector<uint32_t> c = getCount(packedKmers); return std::vector<double>(c.begin(), c.end()); }
		std::vector<double> out(packedKmers.size() / keyBytes());
		if (!out.empty()) check(kmr_lookup_weighted(_h, packedKmers.data(), out.size(), out.data()), "kmr_lookup_weighted");
		return out;
	}
	Histogram getHistogram(unsigned int zoomMax = 256, double logBase = 2.0) {
		Histogram h(zoomMax, logBase);
		const uint32_t nb = kmr_histogram_bins(zoomMax);
		h.visits.resize(nb); h.visitedCount.resize(nb); h.visitedWeight.resize(nb);
		check(kmr_histogram(_h, zoomMax, logBase, h.visits.data(), h.visitedCount.data(), h.visitedWeight.data(), nb), "kmr_histogram");
		h.finish();
		return h;
	}
	/* --bimodal-sigmas (ReadSelector::_bimodalSigmas; negative = off, the default) of every scoring call of this spectrum from now on */
	/* CompareSpectrums: this spectrum as map 1 against `other` as map 2; `saturated` counts the entries read whose stored count is
	 * 65535 (the figures are the reference's while it is 0, lower bounds otherwise) */
	kmr_compare_counts countCommonKmers(KmerSpectrum &other) { kmr_compare_counts c; other.check(kmr_compare_spectrums(_h, other._h, &c), "kmr_compare_spectrums"); return c; }
	/* ... and every read of a device ReadSet on its own against this spectrum as map 2, one record per read */
	std::vector<kmr_compare_counts> compareReads(const ReadSet &reads) {
		std::vector<kmr_compare_counts> out(reads.getSize());
		check(kmr_compare_reads(_h, reads.raw(), out.empty() ? nullptr : out.data()), "kmr_compare_reads");
		return out;
	}
	void setBimodalSigmas(double sigmas) { check(kmr_set_bimodal_sigmas(_h, sigmas), "kmr_set_bimodal_sigmas"); _bimodalSigmas = sigmas; }
	/* bimodal: one word per read where setBimodalSigmas is on (0 = not cut; kmr_bimodal_copy), else empty; the selections that
	 * take a TrimResult print its tags */
	struct TrimResult { std::vector<uint32_t> trimOffset, trimLength; std::vector<float> score; std::vector<uint8_t> wasTrimmed; std::vector<uint64_t> bimodal; };
	TrimResult scoreAndTrimReads(const ReadSet &reads, double minimumKmerScore, ScoringType t = KS_MEDIAN) {
		TrimResult r; const uint64_t n = reads.getSize();
		r.trimOffset.resize(n); r.trimLength.resize(n); r.score.resize(n); r.wasTrimmed.resize(n);
		if (n) {
			check(kmr_score_read_batch(_h, reads.raw(), minimumKmerScore, (int)t, r.trimOffset.data(), r.trimLength.data(), r.score.data(), r.wasTrimmed.data()), "kmr_score_read_batch");
			if (_bimodalSigmas >= 0.0) { r.bimodal.resize(n); check(kmr_bimodal_copy(_h, r.bimodal.data(), n), "kmr_bimodal_copy"); }
		}
		return r;
	}
	/* hands a TrimResult's tags to the next selection over host arrays (kmr_select_bimodal); none: takes back what is left */
	void selectBimodal(const TrimResult &t) { check(kmr_select_bimodal(_h, t.bimodal.empty() ? nullptr : t.bimodal.data(), t.bimodal.size()), "kmr_select_bimodal"); }

	std::vector<uint8_t> image(int whichMap) {
		uint64_t n = 0; check(kmr_image_size(_h, whichMap, &n), "kmr_image_size");
		std::vector<uint8_t> buf(n);
		check(kmr_write_image(_h, whichMap, buf.data(), n), "kmr_write_image");
		return buf;
	}
	void storeMmap(const std::string &filename, uint32_t minDepth) {
		write(filename, image(KMR_MAP_WEAK));
		if (minDepth <= 1) write(filename + "-singleton", image(KMR_MAP_SINGLETON));
	}
	void restoreMmap(const std::string &filename) {
		bool loaded = false;
		std::vector<uint8_t> b;
		if (read(filename, b)) { check(kmr_load_image(_h, KMR_MAP_WEAK, b.data(), b.size()), "kmr_load_image"); loaded = true; }
		if (read(filename + "-singleton", b)) { check(kmr_load_image(_h, KMR_MAP_SINGLETON, b.data(), b.size()), "kmr_load_image"); loaded = true; }
		if (!loaded) throw KmerSpectrumError(KMR_ERR_INVALID_ARG, "Terribly sorry but there were no kmer spectrum mmap files at: " + filename + "*");
	}
	void dumpCounts(const std::string &filename, uint32_t minDepth) { check(kmr_dump_mercount(_h, filename.c_str(), minDepth), "kmr_dump_mercount"); }
	void dumpGraphs(const std::string &filename, uint32_t minDepth) { check(kmr_dump_mergraph(_h, filename.c_str(), minDepth), "kmr_dump_mergraph"); }
	/* the same text, made on the device, for the weak entries [lo, hi) in map order (kmr_dump_text) */
	std::string dumpCountsText(uint32_t minDepth, uint64_t lo = 0, uint64_t hi = UINT64_MAX) { return dumpText(KMR_DUMP_MERCOUNT, minDepth, lo, hi); }
	std::string dumpGraphsText(uint32_t minDepth, uint64_t lo = 0, uint64_t hi = UINT64_MAX) { return dumpText(KMR_DUMP_MERGRAPH, minDepth, lo, hi); }

	std::string dumpText(int kind, uint32_t minDepth, uint64_t lo, uint64_t hi) {
		kmr_text *t = nullptr;
		check(kmr_dump_text(_h, kind, minDepth, lo, hi, &t), "kmr_dump_text");
		std::unique_ptr<kmr_text, void (*)(kmr_text *)> tx(t, kmr_text_free);
		uint64_t bytes = 0;
		kmr_text_info(t, nullptr, &bytes);
		std::string out(bytes, '\0');
		const int rc = kmr_text_copy(t, bytes ? &out[0] : nullptr, bytes);
		if (rc != KMR_OK) throw KmerSpectrumError(rc, "kmr_text_copy");
		return out;
	}
	void check(int rc, const char *what) const { if (rc != KMR_OK) throw KmerSpectrumError(rc, std::string(what) + ": " + kmr_last_error(_h)); }
private:
	static void write(const std::string &f, const std::vector<uint8_t> &b) { std::ofstream o(f, std::ios::binary); o.write((const char *)b.data(), (std::streamsize)b.size()); if (!o) throw KmerSpectrumError(KMR_ERR_INVALID_ARG, "cannot write " + f); }
	static bool read(const std::string &f, std::vector<uint8_t> &b) {
		std::ifstream i(f, std::ios::binary | std::ios::ate); if (!i) return false;
		const std::streamsize n = i.tellg(); if (n <= 0) return false;
		b.resize((size_t)n); i.seekg(0); i.read((char *)b.data(), n); return (bool)i;
	}
	kmr_config _cfg; kmr_handle *_h = nullptr; double _bimodalSigmas = -1.0;
	friend class ReadSet;
	friend class FilterKnownOddities;
};

inline ReadSet::ReadSet(KmerSpectrum &sp, const std::string &fastqText, uint32_t inputQualityBase, bool storeComment) : _text(fastqText) {
	sp.check(kmr_ingest_fastq(sp._h, _text.data(), _text.size(), inputQualityBase, storeComment ? 1 : 0, &_r), "kmr_ingest_fastq");
	load();
}
inline std::unique_ptr<ReadSet> ReadSet::fromFasta(KmerSpectrum &sp, const std::string &fastaText, const std::string *qualText, bool storeComment) {
	kmr_reads *r = nullptr;
	sp.check(kmr_ingest_fasta(sp._h, fastaText.data(), fastaText.size(), qualText ? qualText->c_str() : nullptr, qualText ? qualText->size() : 0, storeComment ? 1 : 0, &r), "kmr_ingest_fasta");
	return std::unique_ptr<ReadSet>(new ReadSet(fastaText, r));
}
inline void ReadSet::load() {
	kmr_reads_info(_r, &_n, &_bases, &_qbase, &_filtered);
	_nameOff.resize(_n ? _n : 1); _nameLen.resize(_n ? _n : 1);
	if (kmr_reads_copy(_r, nullptr, nullptr, nullptr, _nameOff.data(), _nameLen.data()) != KMR_OK) throw KmerSpectrumError(KMR_ERR_HIP, "kmr_reads_copy");
}

/* TnfDistance (apps/TnfDistance.cpp): vectors of canonical k-mer counts on the device (kmr_tnf), k the spectrum's (1 - 6); see the
 * TnfDistance block of kmernator_amd.h.  tnfDims / tnfColumns / tnfHeader need no device. */
inline uint32_t tnfDims(uint32_t k) { uint32_t d = 0; const int rc = kmr_tnf_dims(k, &d); if (rc != KMR_OK) throw KmerSpectrumError(rc, "kmr_tnf_dims"); return d; }
inline std::vector<uint16_t> tnfColumns(uint32_t k, uint32_t hashKind = 0) {
	std::vector<uint16_t> codes(tnfDims(k));
	const int rc = kmr_tnf_columns(k, hashKind, codes.data()); if (rc != KMR_OK) throw KmerSpectrumError(rc, "kmr_tnf_columns");
	return codes;
}
inline std::string tnfHeader(uint32_t k, uint32_t hashKind = 0) {
	uint64_t bytes = 0;
	std::string s((size_t)16 + (k + 1) * tnfDims(k), '\0');
	const int rc = kmr_tnf_header(k, hashKind, &s[0], s.size(), &bytes); if (rc != KMR_OK) throw KmerSpectrumError(rc, "kmr_tnf_header");
	s.resize(bytes);
	return s;
}
class TnfVectors {
public:
	/* buildTnfs (:462-484): one vector per sequence; inputStarts = n_inputs + 1 sequence indices, empty = one input */
	static std::unique_ptr<TnfVectors> ofReads(KmerSpectrum &sp, const ReadSet &reads, const std::vector<uint64_t> &inputStarts = std::vector<uint64_t>()) {
		kmr_tnf *t = nullptr;
		sp.check(kmr_tnf_reads(sp.raw(), reads.raw(), inputStarts.empty() ? nullptr : inputStarts.data(), inputStarts.empty() ? 0 : (uint32_t)inputStarts.size() - 1, &t), "kmr_tnf_reads");
		return std::unique_ptr<TnfVectors>(new TnfVectors(sp, t));
	}
	/* shredReadByWindow + purgeShortTNFS (:486-518); the tool's minCount is window * 3 / 4 */
	static std::unique_ptr<TnfVectors> ofWindows(KmerSpectrum &sp, const ReadSet &reads, uint64_t window, uint64_t step, int64_t minCount, const std::vector<uint64_t> &inputStarts = std::vector<uint64_t>()) {
		kmr_tnf *t = nullptr;
		sp.check(kmr_tnf_windows(sp.raw(), reads.raw(), inputStarts.empty() ? nullptr : inputStarts.data(), inputStarts.empty() ? 0 : (uint32_t)inputStarts.size() - 1, window, step, minCount, &t), "kmr_tnf_windows");
		return std::unique_ptr<TnfVectors>(new TnfVectors(sp, t));
	}
	~TnfVectors() { kmr_tnf_free(_t); }
	TnfVectors(const TnfVectors &) = delete; TnfVectors &operator=(const TnfVectors &) = delete;
	uint64_t size() const { return _n; }
	uint32_t dims() const { return _d; }
	uint32_t numGroups() const { return _g; }
	uint64_t inexact() const { return _inexact; }      /* columns above 2^24: the reference's floats are followed while this is 0 */
	std::vector<uint64_t> counts() const { std::vector<uint64_t> a(_n * _d); copy(a.data(), nullptr, nullptr, nullptr); return a; }
	std::vector<float> lengths() const { std::vector<float> a(_n); copy(nullptr, a.data(), nullptr, nullptr); return a; }
	std::vector<uint64_t> origin() const { std::vector<uint64_t> a(3 * _n); copy(nullptr, nullptr, a.data(), nullptr); return a; }
	std::vector<uint64_t> groups() const { std::vector<uint64_t> a((size_t)_g + 1); copy(nullptr, nullptr, nullptr, a.data()); return a; }
	/* wholeTnfs (:717): one vector per group */
	std::unique_ptr<TnfVectors> groupSums() const {
		kmr_tnf *t = nullptr;
		_sp.check(kmr_tnf_group_sums(_sp.raw(), _t, &t), "kmr_tnf_group_sums");
		return std::unique_ptr<TnfVectors>(new TnfVectors(_sp, t));
	}
	/* getDistance (:434-446) of rows [firstRow, firstRow + nRows) against every vector of `other` (row-major), or with other == nullptr the
	 * packed strict lower triangle; formula: KMR_TNF_EUCLIDEAN / KMR_TNF_SPEARMAN */
	std::vector<float> distances(const TnfVectors *other, int formula, uint64_t firstRow = 0, uint64_t nRows = UINT64_MAX) const {
		if (nRows == UINT64_MAX) nRows = _n - firstRow;
		const uint64_t e = firstRow + nRows;
		std::vector<float> out(other ? nRows * other->_n : (e ? e * (e - 1) / 2 : 0) - (firstRow ? firstRow * (firstRow - 1) / 2 : 0));
		_sp.check(kmr_tnf_distances(_sp.raw(), _t, other ? other->_t : nullptr, formula, firstRow, nRows, out.empty() ? nullptr : out.data()), "kmr_tnf_distances");
		return out;
	}
	/* the four histograms of --intra-inter-file (:664-902), bins + 2 counters each */
	static std::vector<uint64_t> likelihoods(KmerSpectrum &sp, const ReadSet &reads, const kmr_tnf_likelihood_config &cfg, const std::vector<uint64_t> &inputStarts = std::vector<uint64_t>()) {
		std::vector<uint64_t> out((size_t)4 * (cfg.bins + 2));
		sp.check(kmr_tnf_likelihoods(sp.raw(), reads.raw(), inputStarts.empty() ? nullptr : inputStarts.data(), inputStarts.empty() ? 0 : (uint32_t)inputStarts.size() - 1, &cfg, out.data()), "kmr_tnf_likelihoods");
		return out;
	}
	const kmr_tnf *raw() const { return _t; }
private:
	TnfVectors(KmerSpectrum &sp, kmr_tnf *t) : _sp(sp), _t(t) { kmr_tnf_info(t, &_n, &_d, &_g, &_inexact); }
	void copy(uint64_t *c, float *l, uint64_t *o, uint64_t *g) const { const int rc = kmr_tnf_copy(_t, c, l, o, g); if (rc != KMR_OK) throw KmerSpectrumError(rc, "kmr_tnf_copy"); }
	KmerSpectrum &_sp; kmr_tnf *_t; uint64_t _n = 0, _inexact = 0; uint32_t _d = 0, _g = 0;
};

/* KmerMatch (src/KmerMatch.h:93-185, src/MatcherInterface.h): for every contig the reads that share a k-mer with one of its edge windows,
 * sampled, with their mates, sorted (kmr_match_*).  `sp` is the finalized spectrum of exactly the reads that are streamed, and outlives
 * the object */
struct MatchResults {
	std::vector<uint64_t> offsets, reads, sizeBeforeSampling, sizeAfterSampling;      /* contig i: reads[offsets[i] .. offsets[i + 1]), ascending */
	uint64_t sampledContigs = 0;
	size_t size() const { return offsets.empty() ? 0 : offsets.size() - 1; }
	std::vector<uint64_t> operator[](size_t i) const { return std::vector<uint64_t>(reads.begin() + (ptrdiff_t)offsets[i], reads.begin() + (ptrdiff_t)offsets[i + 1]); }
};
class KmerMatch {
public:
	static kmr_match_config defaults() { kmr_match_config c; kmr_match_config_init(&c); return c; }
	KmerMatch(KmerSpectrum &sp, const ReadSet &contigs, const kmr_match_config &cfg = defaults()) : _sp(sp) { sp.check(kmr_match_create(sp.raw(), contigs.raw(), &cfg, &_m), "kmr_match_create"); }
	~KmerMatch() { kmr_match_free(_m); }
	KmerMatch(const KmerMatch &) = delete; KmerMatch &operator=(const KmerMatch &) = delete;
	/* one batch of the target reads; pairs: the batch's own pairing (kmr_identify_pairs) or nullptr, discarded: one flag per read or empty */
	void addReads(const ReadSet &reads, uint64_t firstGlobalReadIdx = 0, const kmr_pairs *pairs = nullptr, const std::vector<uint8_t> &discarded = std::vector<uint8_t>()) {
		if (!discarded.empty() && discarded.size() != reads.getSize()) throw KmerSpectrumError(KMR_ERR_INVALID_ARG, "KmerMatch::addReads: one discard flag per read");
		_sp.check(kmr_match_add_read_batch(_m, reads.raw(), firstGlobalReadIdx, pairs, discarded.empty() ? nullptr : discarded.data()), "kmr_match_add_read_batch");
	}
	MatchResults finish() {
		_sp.check(kmr_match_finish(_m), "kmr_match_finish");
		uint64_t nc = 0, nr = 0;
		MatchResults r;
		_sp.check(kmr_match_info(_m, &nc, &nr, &r.sampledContigs), "kmr_match_info");
		r.offsets.resize(nc + 1); r.reads.resize(nr); r.sizeBeforeSampling.resize(nc); r.sizeAfterSampling.resize(nc);
		_sp.check(kmr_match_copy(_m, r.offsets.data(), nr ? r.reads.data() : nullptr, nc ? r.sizeBeforeSampling.data() : nullptr, nc ? r.sizeAfterSampling.data() : nullptr), "kmr_match_copy");
		return r;
	}
	/* contigs, considered k-mers, distinct keys, keys the spectrum holds */
	void edgeInfo(uint64_t &contigs, uint64_t &edgeKmers, uint64_t &distinctKeys, uint64_t &keysInSpectrum) const { kmr_match_edge_info(_m, &contigs, &edgeKmers, &distinctKeys, &keysInSpectrum); }
	const kmr_match *raw() const { return _m; }
private:
	KmerSpectrum &_sp; kmr_match *_m = nullptr;
};

/* ContigExtender (src/ContigExtender.h:157-247 at one k-mer size, over KmerSpectrum::extendContig, src/KmerSpectrum.h:2311-2373): every
 * contig walks outwards while the spectrum of its own pool of reads agrees (kmr_extend_*).  `sp` supplies k and the build's config
 * and need not have been fed.  getNewName / getMinMaxKmerSize need no device. */
struct ExtendResults {
	std::vector<std::string> sequences, names;             /* the new sequences; getNewName of the names handed in (empty without names) */
	std::vector<uint32_t> left, right, newLength;          /* bases added per contig */
	std::vector<kmr_extend_stop> stops;                    /* two per contig: left, right */
	uint64_t extended = 0, basesAdded = 0;
	std::unique_ptr<ReadSet> readSet;                      /* the sequences as a batch of quality Read::REF_QUAL, for the next round's KmerMatch */
};
class ContigExtender {
public:
	static kmr_extend_config defaults() { kmr_extend_config c; kmr_extend_config_init(&c); return c; }
	explicit ContigExtender(KmerSpectrum &sp, const kmr_extend_config &cfg = defaults()) : _sp(sp), _cfg(cfg) {}
	/* contig i's pool: reads poolReads[poolOffsets[i] .. poolOffsets[i + 1]) of `reads`; active: one flag per contig or empty */
	ExtendResults extendContigs(const ReadSet &contigs, const ReadSet &reads, const std::vector<uint64_t> &poolOffsets, const std::vector<uint64_t> &poolReads,
	                            const std::vector<std::string> &names = std::vector<std::string>(), const std::vector<uint8_t> &active = std::vector<uint8_t>()) {
		if (poolOffsets.size() != contigs.getSize() + 1 || (!active.empty() && active.size() != contigs.getSize()) || (!names.empty() && names.size() != contigs.getSize()))
			throw KmerSpectrumError(KMR_ERR_INVALID_ARG, "ContigExtender::extendContigs: one pool, name and flag per contig");
		kmr_extend *e = nullptr;
		_sp.check(kmr_extend_contigs(_sp.raw(), contigs.raw(), reads.raw(), poolOffsets.data(), poolReads.empty() ? nullptr : poolReads.data(), active.empty() ? nullptr : active.data(), &_cfg, &e),
		          "kmr_extend_contigs");
		std::unique_ptr<kmr_extend, void (*)(kmr_extend *)> hold(e, kmr_extend_free);
		ExtendResults r;
		uint64_t n = 0;
		kmr_extend_info(e, &n, &r.extended, &r.basesAdded);
		const uint64_t m = n ? n : 1;
		r.left.assign(m, 0); r.right.assign(m, 0); r.newLength.assign(m, 0); r.stops.resize(2 * m);
		_sp.check(kmr_extend_copy(e, r.newLength.data(), r.left.data(), r.right.data(), r.stops.data()), "kmr_extend_copy");
		r.left.resize(n); r.right.resize(n); r.newLength.resize(n); r.stops.resize(2 * n);
		const kmr_reads *batch = nullptr;
		_sp.check(kmr_extend_reads(e, &batch), "kmr_extend_reads");
		uint64_t total = 0;
		kmr_reads_info(batch, nullptr, &total, nullptr, nullptr);
		std::string bases(total, '\0'), quals(total, '\0');
		std::vector<uint64_t> off(n + 1);
		if (kmr_reads_copy(batch, &bases[0], &quals[0], off.data(), nullptr, nullptr) != KMR_OK) throw KmerSpectrumError(KMR_ERR_HIP, "kmr_reads_copy");
		for (uint64_t i = 0; i < n; i++) {
			r.sequences.push_back(bases.substr(off[i], off[i + 1] - off[i]));
			if (!names.empty()) r.names.push_back(getNewName(names[i], r.left[i], r.right[i]));
		}
		kmr_reads *own = nullptr;      /* a batch of its own: the result object goes with this call */
		_sp.check(kmr_reads_from_host(_sp.raw(), bases.data(), quals.data(), off.data(), n, &own), "kmr_reads_from_host");
		r.readSet.reset(new ReadSet(std::string(), own));
		return r;
	}
	/* ContigExtender::getNewName (:249-268) */
	static std::string getNewName(const std::string &oldName, uint64_t leftTotal, uint64_t rightTotal) {
		std::string buf(oldName.size() + 48, '\0');
		const int rc = kmr_extend_new_name(oldName.c_str(), leftTotal, rightTotal, &buf[0], buf.size()); if (rc != KMR_OK) throw KmerSpectrumError(rc, "kmr_extend_new_name");
		buf.resize(std::strlen(buf.c_str()));
		return buf;
	}
	/* ContigExtender::getMinMaxKmerSize (:269-279) */
	static void getMinMaxKmerSize(uint32_t kmerSize, const ReadSet &reads, uint32_t maxSequenceLength, uint32_t &minKmerSize, uint32_t &maxKmerSize, uint32_t &kmerStep, uint32_t maxSteps = 6) {
		const int rc = kmr_extend_min_max_kmer_size(kmerSize, maxSequenceLength, reads.getBaseCount(), reads.getSize(), maxSteps, &minKmerSize, &maxKmerSize, &kmerStep);
		if (rc != KMR_OK) throw KmerSpectrumError(rc, "kmr_extend_min_max_kmer_size");
	}
private:
	KmerSpectrum &_sp; kmr_extend_config _cfg;
};

/* FilterKnownOddities (src/FilterKnownOddities.h): the artifact screen FilterReads runs before the spectrum build */
class FilterKnownOddities {
public:
	struct Results {                      /* per read, FilterResults (:289-296) + what recordAffectedRead did with it */
		std::vector<uint32_t> value, minPass, maxPass, remnantOffset, remnantLength;
		std::vector<uint8_t> action;      /* 0 untouched, 1 trimmed ("AFTrim:<minPass>+<maxPass-minPass>"), 2 discarded */
	};
	static kmr_artifact_config defaults(const kmr_config &sp) { kmr_artifact_config c; kmr_artifact_config_init(&c); c.fastq_start_char = sp.fastq_start_char; c.min_quality = sp.min_quality_score; return c; }
	FilterKnownOddities(KmerSpectrum &sp, const std::string &artifactFasta, const kmr_artifact_config &cfg) : _sp(sp) {
		sp.check(kmr_artifact_filter_create(sp.raw(), &cfg, artifactFasta.data(), artifactFasta.size(), &_f), "kmr_artifact_filter_create");
	}
	~FilterKnownOddities() { kmr_artifact_filter_free(_f); }
	FilterKnownOddities(const FilterKnownOddities &) = delete; FilterKnownOddities &operator=(const FilterKnownOddities &) = delete;
	uint64_t getFilterSize() const { uint64_t n = 0; kmr_artifact_filter_info(_f, nullptr, &n, nullptr); return n; }
	/* applyFilter(ReadSet&) (:663-733): the reads afterwards (trimmed in place, remnants appended); mate = paired read or -1 */
	std::unique_ptr<ReadSet> applyFilter(const ReadSet &reads, Results &res, const int64_t *mate = nullptr) {
		const uint64_t n = reads.getSize(), m = n ? n : 1;
		res.value.assign(m, 0); res.minPass.assign(m, 0); res.maxPass.assign(m, 0); res.remnantOffset.assign(m, 0); res.remnantLength.assign(m, 0); res.action.assign(m, 0);
		kmr_reads *out = nullptr;
		_sp.check(kmr_artifact_filter_apply(_sp.raw(), _f, reads.raw(), mate, res.value.data(), res.minPass.data(), res.maxPass.data(), res.action.data(),
		                                    res.remnantOffset.data(), res.remnantLength.data(), &out), "kmr_artifact_filter_apply");
		return std::unique_ptr<ReadSet>(new ReadSet(reads._text, out));
	}
	/* what the Recorder (:296-353) makes of applyFilter's results: the counters and the -Artifact.fastq / -PhiX.fastq records */
	struct Report {
		std::vector<uint64_t> discarded, trimmed, bases;      /* per sequence index, n_sequences + 1 entries */
		std::string text;                                     /* all records: segment after segment */
		uint32_t nInputs = 1;
		std::vector<uint64_t> segFirstByte, segBytes, segRecords;      /* [row * nInputs + input], row 0 Artifact, row 1 PhiX */
	};
	static kmr_artifact_report_config reportDefaults() { kmr_artifact_report_config c; kmr_artifact_report_config_init(&c); return c; }
	std::string getFilterName(uint32_t idx) const {
		char buf[4096];
		if (kmr_artifact_filter_name(_f, idx, buf, sizeof buf) != KMR_OK) throw KmerSpectrumError(KMR_ERR_INVALID_ARG, "kmr_artifact_filter_name");
		return buf;
	}
	/* kmr_artifact_filter_report over the batch `res` was computed from; read1 / read2 = the pair list (nullptr: every read on its own),
	 * inputStarts = nInputs + 1 read indices (nullptr: one input) */
	Report report(const ReadSet &reads, const Results &res, const kmr_artifact_report_config &cfg, const int64_t *read1 = nullptr, const int64_t *read2 = nullptr, uint64_t nPairs = 0,
	              const uint64_t *inputStarts = nullptr, uint32_t nInputs = 0) {
		kmr_artifact_report *rep = nullptr;
		_sp.check(kmr_artifact_filter_report(_sp.raw(), _f, reads.raw(), reads._text.data(), reads._text.size(), read1, read2, nPairs, res.value.data(), res.action.data(),
		                                     res.minPass.data(), res.maxPass.data(), inputStarts, nInputs, &cfg, &rep), "kmr_artifact_filter_report");
		std::unique_ptr<kmr_artifact_report, void (*)(kmr_artifact_report *)> hold(rep, kmr_artifact_report_free);
		Report out;
		uint64_t nSeq = 0, bytes = 0; uint32_t nRows = 0;
		kmr_artifact_filter_info(_f, &nSeq, nullptr, nullptr);
		out.discarded.assign(nSeq + 1, 0); out.trimmed.assign(nSeq + 1, 0); out.bases.assign(nSeq + 1, 0);
		_sp.check(kmr_artifact_report_counts(rep, out.discarded.data(), out.trimmed.data(), out.bases.data(), nSeq + 1), "kmr_artifact_report_counts");
		const kmr_picks *pk = nullptr;
		_sp.check(kmr_artifact_report_picks(rep, &pk), "kmr_artifact_report_picks");
		kmr_picks_info(pk, nullptr, &bytes); kmr_picks_segments_info(pk, &nRows, &out.nInputs);
		const size_t segs = (size_t)nRows * out.nInputs;
		out.segFirstByte.assign(segs, 0); out.segBytes.assign(segs, 0); out.segRecords.assign(segs, 0);
		_sp.check(kmr_picks_segments_copy(pk, nullptr, nullptr, nullptr, out.segRecords.data(), out.segFirstByte.data(), out.segBytes.data(), nullptr), "kmr_picks_segments_copy");
		out.text.resize(bytes);
		if (bytes) _sp.check(kmr_picks_copy(pk, &out.text[0], bytes, nullptr), "kmr_picks_copy");
		return out;
	}
private:
	KmerSpectrum &_sp; kmr_artifact_filter *_f = nullptr;
};

/* ReadSelector (src/ReadSelector.h) over a device-resident ReadSet: pickAllPassingReads / pickAllPassingPairs (:576-596) and writePicks
 * (:1242-1262), pickCoverageNormalizedSubset (:673-749), selection and output text made on the device (kmr_select_reads,
 * kmr_filter_read_batch, kmr_partition_*, kmr_normalize_*).  mate = paired read or -1 per
 * read of the batch `reads` was filtered from (nullptr: all single); af = the artifact filter's results for that batch.  Both are copied
 * and extended over the remnants the filter appended to `reads` (single, untouched reads), so the arrays handed on always have
 * reads.getSize() entries */
class ReadSelector {
public:
	static kmr_select_config defaults() { kmr_select_config c; kmr_select_config_init(&c); return c; }
	/* nMate = entries of mate (0: reads.getSize()) */
	ReadSelector(KmerSpectrum &sp, const ReadSet &reads, const int64_t *mate = nullptr, const FilterKnownOddities::Results *af = nullptr, uint64_t nMate = 0) : _sp(sp), _reads(reads) {
		const uint64_t n = reads.getSize(), m = n ? n : 1;
		if (mate) {
			if (!nMate) nMate = n;
			if (nMate > n) throw KmerSpectrumError(KMR_ERR_INVALID_ARG, "ReadSelector: more mates than reads");
			_mate.assign(m, -1); std::copy(mate, mate + nMate, _mate.begin());
		}
		if (af) {
			const uint64_t k = std::min<uint64_t>(af->action.size(), std::min<uint64_t>(af->minPass.size(), af->maxPass.size()));
			if (k > m) throw KmerSpectrumError(KMR_ERR_INVALID_ARG, "ReadSelector: more artifact filter results than reads");
			_action.assign(m, 0); _minPass.assign(m, 0); _maxPass.assign(m, 0);
			std::copy(af->action.begin(), af->action.begin() + k, _action.begin()); std::copy(af->minPass.begin(), af->minPass.begin() + k, _minPass.begin()); std::copy(af->maxPass.begin(), af->maxPass.begin() + k, _maxPass.begin());
		}
	}
	~ReadSelector() { kmr_picks_free(_p); }
	ReadSelector(const ReadSelector &) = delete; ReadSelector &operator=(const ReadSelector &) = delete;
	/* scoreAndTrimReads + the selection in one call that keeps the trims on the device; returns the number of picks */
	uint64_t filterReads(const kmr_select_config &cfg) {
		reset();
		_sp.check(kmr_filter_read_batch(_sp.raw(), _reads.raw(), _reads._text.data(), _reads._text.size(), mate(), action(), minPass(), maxPass(), &cfg, &_p), "kmr_filter_read_batch");
		return getNumPicks();
	}
	/* the selection over trims the caller holds (KmerSpectrum::scoreAndTrimReads) */
	uint64_t pickAllPassingPairs(const KmerSpectrum::TrimResult &t, const kmr_select_config &cfg) {
		reset();
		_sp.selectBimodal(t);
		_sp.check(kmr_select_reads(_sp.raw(), _reads.raw(), _reads._text.data(), _reads._text.size(), mate(), action(), minPass(), maxPass(),
		                           t.trimOffset.data(), t.trimLength.data(), t.score.data(), t.wasTrimmed.data(), &cfg, &_p), "kmr_select_reads");
		return getNumPicks();
	}
	/* selectReads (apps/FilterReads.h:159-279) with --max-kmer-output-depth off: the rounds of cfg.partition_by_depth and
	 * cfg.remainder_trim over the inputs [inputStarts[j], inputStarts[j + 1]) (empty = one input); the fused call when trims is
	 * null, else the selection over the trims the caller holds.  Returns the files the reference writes, in order, as (name, text):
	 * with separateOutputs output + "-MinDepth<d>" + "-PartitionDepth<depth>" or "-Remainder" (when partitioned) + "-" + prefix +
	 * ".fastq" / ".fasta", a file no read went to left out; without, one entry named output with the concatenation.
	 * inputPrefixes default to "transformed-<j + 1>" (src/ReadSet.cpp:376-382). */
	struct Segments { uint32_t nRounds = 0, nInputs = 0; std::vector<float> roundDepth; std::vector<uint8_t> roundIsRemainder; std::vector<uint64_t> firstPick, picks, firstByte, bytes; std::vector<int32_t> readSegment; };
	static kmr_partition_config partitionDefaults() { kmr_partition_config c; kmr_partition_config_init(&c); return c; }
	std::vector<std::pair<std::string, std::string> > selectReads(const kmr_partition_config &cfg, const std::vector<uint64_t> &inputStarts = std::vector<uint64_t>(),
	                                                              const std::vector<std::string> &inputPrefixes = std::vector<std::string>(), const std::string &output = "",
	                                                              bool separateOutputs = true, const KmerSpectrum::TrimResult *trims = nullptr) {
		reset();
		const uint64_t *starts = inputStarts.empty() ? nullptr : inputStarts.data();
		const uint32_t nIn = inputStarts.empty() ? 0 : (uint32_t)(inputStarts.size() - 1);
		if (trims) _sp.selectBimodal(*trims);
		if (trims) _sp.check(kmr_partition_reads(_sp.raw(), _reads.raw(), _reads._text.data(), _reads._text.size(), mate(), action(), minPass(), maxPass(), trims->trimOffset.data(), trims->trimLength.data(),
		                                         trims->score.data(), trims->wasTrimmed.data(), starts, nIn, &cfg, &_p), "kmr_partition_reads");
		else _sp.check(kmr_partition_read_batch(_sp.raw(), _reads.raw(), _reads._text.data(), _reads._text.size(), mate(), action(), minPass(), maxPass(), starts, nIn, &cfg, &_p), "kmr_partition_read_batch");
		const std::string text = writePicks();
		const Segments s = segments();
		std::vector<std::pair<std::string, std::string> > files;
		if (!separateOutputs) { files.push_back(std::make_pair(output, text)); return files; }
		if (!inputPrefixes.empty() && inputPrefixes.size() != s.nInputs) throw KmerSpectrumError(KMR_ERR_INVALID_ARG, "selectReads: one prefix per input");
		for (uint32_t r = 0; r < s.nRounds; r++) {
			std::string name = output + "-MinDepth" + std::to_string((unsigned int)cfg.select.minimum_score);
			if (cfg.partition_by_depth > 0) {
				char depth[32]; std::snprintf(depth, sizeof depth, "%.9g", (double)s.roundDepth[r]);      /* lexical_cast<string>(float): 16, not 16.0 */
				if (s.roundIsRemainder[r]) name += "-Remainder"; else if (s.roundDepth[r] > 0) name += std::string("-PartitionDepth") + depth;
			}
			for (uint32_t j = 0; j < s.nInputs; j++) {
				const size_t g = (size_t)r * s.nInputs + j;
				if (!s.picks[g]) continue;
				const std::string prefix = inputPrefixes.empty() ? "transformed-" + std::to_string(j + 1) : inputPrefixes[j];
				files.push_back(std::make_pair(name + "-" + prefix + (cfg.select.format == 1 ? ".fasta" : ".fastq"), text.substr(s.firstByte[g], s.bytes[g])));
			}
		}
		return files;
	}
	/* The pair list coverage normalization decides over, as kmr_pairs_copy returns it (-1 = no read on that side); without one every
	 * read is a half pair, as is a read no pair names */
	void setPairs(const int64_t *read1, const int64_t *read2, uint64_t nPairs) { _read1.assign(read1, read1 + nPairs); _read2.assign(read2, read2 + nPairs); }
	static kmr_normalize_config normalizeDefaults() { kmr_normalize_config c; kmr_normalize_config_init(&c); return c; }
	struct NormalizeInfo { uint64_t picks = 0, candidates = 0, draws = 0; };
	/* selectReads with --max-kmer-output-depth = cfg.target_depth (apps/FilterReads.h:178-206; pickCoverageNormalizedSubset, RANDOM,
	 * the draws Philox4x32-10 of (cfg.seed, cfg.first_global_read_idx + read index)): the fused call when trims is null.  Returns the
	 * files as selectReads above, one round, named output + "-MinDepth<d>" + "-MaxDepth<T>" + "-" + prefix + suffix (:173,180);
	 * normalizeInfo().picks is the reference's return value (pairs), getNumPicks() counts records */
	std::vector<std::pair<std::string, std::string> > selectReadsNormalized(const kmr_normalize_config &cfg, const std::vector<uint64_t> &inputStarts = std::vector<uint64_t>(),
	                                                                        const std::vector<std::string> &inputPrefixes = std::vector<std::string>(), const std::string &output = "",
	                                                                        bool separateOutputs = true, const KmerSpectrum::TrimResult *trims = nullptr) {
		reset();
		const uint64_t *starts = inputStarts.empty() ? nullptr : inputStarts.data();
		const uint32_t nIn = inputStarts.empty() ? 0 : (uint32_t)(inputStarts.size() - 1);
		const int64_t *r1 = _read1.empty() ? nullptr : _read1.data(), *r2 = _read2.empty() ? nullptr : _read2.data();
		if (trims) _sp.selectBimodal(*trims);
		if (trims) _sp.check(kmr_normalize_reads(_sp.raw(), _reads.raw(), _reads._text.data(), _reads._text.size(), r1, r2, _read1.size(), action(), minPass(), maxPass(), trims->trimOffset.data(),
		                                         trims->trimLength.data(), trims->score.data(), trims->wasTrimmed.data(), starts, nIn, &cfg, &_p), "kmr_normalize_reads");
		else _sp.check(kmr_normalize_read_batch(_sp.raw(), _reads.raw(), _reads._text.data(), _reads._text.size(), r1, r2, _read1.size(), action(), minPass(), maxPass(), starts, nIn, &cfg, &_p), "kmr_normalize_read_batch");
		const std::string text = writePicks();
		const Segments s = segments();
		std::vector<std::pair<std::string, std::string> > files;
		if (!separateOutputs) { files.push_back(std::make_pair(output, text)); return files; }
		if (!inputPrefixes.empty() && inputPrefixes.size() != s.nInputs) throw KmerSpectrumError(KMR_ERR_INVALID_ARG, "selectReadsNormalized: one prefix per input");
		const std::string name = output + "-MinDepth" + std::to_string((unsigned int)cfg.select.minimum_score) + "-MaxDepth" + std::to_string(cfg.target_depth);
		for (uint32_t j = 0; j < s.nInputs; j++) {
			if (!s.picks[j]) continue;
			const std::string prefix = inputPrefixes.empty() ? "transformed-" + std::to_string(j + 1) : inputPrefixes[j];
			files.push_back(std::make_pair(name + "-" + prefix + (cfg.select.format == 1 ? ".fasta" : ".fastq"), text.substr(s.firstByte[j], s.bytes[j])));
		}
		return files;
	}
	NormalizeInfo normalizeInfo() const {
		NormalizeInfo i;
		if (kmr_normalize_info(_p, &i.picks, &i.candidates, &i.draws) != KMR_OK) throw KmerSpectrumError(KMR_ERR_STATE, "normalizeInfo: the picks are not those of a normalization");
		return i;
	}
	/* the segment table of the picks (kmr_picks_segments_copy): segment = round * nInputs + input */
	Segments segments() const {
		Segments s;
		if (kmr_picks_segments_info(_p, &s.nRounds, &s.nInputs) != KMR_OK) throw KmerSpectrumError(KMR_ERR_STATE, "segments: nothing has been picked");
		const size_t g = (size_t)s.nRounds * s.nInputs, n = _reads.getSize();
		s.roundDepth.assign(33, 0); s.roundIsRemainder.assign(33, 0);
		s.firstPick.assign(g + 1, 0); s.picks.assign(g + 1, 0); s.firstByte.assign(g + 1, 0); s.bytes.assign(g + 1, 0); s.readSegment.assign(n + 1, -1);
		const int rc = kmr_picks_segments_copy(_p, s.roundDepth.data(), s.roundIsRemainder.data(), s.firstPick.data(), s.picks.data(), s.firstByte.data(), s.bytes.data(), s.readSegment.data());
		if (rc != KMR_OK) throw KmerSpectrumError(rc, "kmr_picks_segments_copy");
		s.roundDepth.resize(s.nRounds); s.roundIsRemainder.resize(s.nRounds);
		s.firstPick.resize(g); s.picks.resize(g); s.firstByte.resize(g); s.bytes.resize(g); s.readSegment.resize(n);
		return s;
	}
	uint64_t getNumPicks() const { uint64_t n = 0; kmr_picks_info(_p, &n, nullptr); return n; }
	/* the text of the picks; picked (optional) receives one flag per read of the batch */
	std::string writePicks(std::vector<uint8_t> *picked = nullptr) const {
		uint64_t bytes = 0;
		if (kmr_picks_info(_p, nullptr, &bytes) != KMR_OK) throw KmerSpectrumError(KMR_ERR_STATE, "writePicks: nothing has been picked");
		std::string out(bytes, '\0');
		if (picked) picked->assign(_reads.getSize() ? _reads.getSize() : 1, 0);
		const int rc = kmr_picks_copy(_p, &out[0], bytes, picked ? picked->data() : nullptr);
		if (rc != KMR_OK) throw KmerSpectrumError(rc, "kmr_picks_copy");
		if (picked) picked->resize(_reads.getSize());
		return out;
	}
	const kmr_picks *raw() const { return _p; }
private:
	void reset() { kmr_picks_free(_p); _p = nullptr; }
	const int64_t *mate() const { return _mate.empty() ? nullptr : _mate.data(); }
	const uint8_t *action() const { return _action.empty() ? nullptr : _action.data(); }
	const uint32_t *minPass() const { return _minPass.empty() ? nullptr : _minPass.data(); }
	const uint32_t *maxPass() const { return _maxPass.empty() ? nullptr : _maxPass.data(); }
	KmerSpectrum &_sp; const ReadSet &_reads; std::vector<int64_t> _mate; std::vector<uint8_t> _action; std::vector<uint32_t> _minPass, _maxPass; std::vector<int64_t> _read1, _read2; kmr_picks *_p = nullptr;
};

}  // namespace kmernator
#endif
