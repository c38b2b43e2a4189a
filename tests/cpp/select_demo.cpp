// FilterReads to its output file through the C++ host side (include/kmernator_amd.hpp), no reference headers:
//   select_demo <fastq> <artifacts.fa> <out-prefix> <min-read-length> <both-pass 0|1> <output-quality-base>
// artifact filter (--artifact-edit-distance 1), spectrum of the filtered reads, then ReadSelector: <out-prefix>.fused is
// filterReads' text, <out-prefix>.select the text of pickAllPassingPairs over the trims of scoreAndTrimReads.  The reads are
// paired (2i, 2i + 1), as test/runFilterTests.sh runs them.
#include <cstdlib>
#include <fstream>
#include <iterator>
#include "kmernator_amd.hpp"

using namespace kmernator;

static std::string slurp(const char *path) { std::ifstream f(path, std::ios::binary); return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }

int main(int argc, char **argv) {
	if (argc < 7) { std::fprintf(stderr, "usage: select_demo <fastq> <artifacts.fa> <out-prefix> <min-read-length> <both-pass> <output-quality-base>\n"); return 2; }
	const std::string out = argv[3];
	try {
		KmerSpectrum sp(KmerSpectrum::defaults(31, 46000));
		ReadSet input(sp, slurp(argv[1]));
		kmr_artifact_config ac = FilterKnownOddities::defaults(sp.config());
		ac.edit_distance = 1; ac.min_read_length = (float)std::atof(argv[4]);
		FilterKnownOddities filter(sp, slurp(argv[2]), ac);
		FilterKnownOddities::Results fr;
		std::unique_ptr<ReadSet> reads = filter.applyFilter(input, fr);
		sp.buildKmerSpectrum(*reads);
		sp.purgeMinDepth(2);
		std::vector<int64_t> mate(input.getSize());
		for (uint64_t i = 0; i < mate.size(); i++) mate[i] = (int64_t)(i ^ 1);
		kmr_select_config cfg = ReadSelector::defaults();
		cfg.min_read_length = ac.min_read_length; cfg.both_pass = (uint32_t)std::atoi(argv[5]); cfg.output_quality_base = (uint32_t)std::atoi(argv[6]);
		/* the results and the mates cover the input's reads; the selector extends them over the remnants the filter appended */
		ReadSelector sel(sp, *reads, mate.data(), &fr, mate.size());
		const uint64_t nFused = sel.filterReads(cfg);
		std::vector<uint8_t> picked;
		{ std::ofstream o(out + ".fused", std::ios::binary); o << sel.writePicks(&picked); }
		const KmerSpectrum::TrimResult t = sp.scoreAndTrimReads(*reads, cfg.minimum_score, KmerSpectrum::KS_MEDIAN);
		const uint64_t nSelect = sel.pickAllPassingPairs(t, cfg);
		{ std::ofstream o(out + ".select", std::ios::binary); o << sel.writePicks(); }
		uint64_t flagged = 0; for (uint8_t f : picked) flagged += f;
		std::printf("reads %llu picks %llu %llu flagged %llu\n", (unsigned long long)reads->getSize(), (unsigned long long)nFused, (unsigned long long)nSelect, (unsigned long long)flagged);
	} catch (const KmerSpectrumError &e) {
		std::fprintf(stderr, "%s\n", e.what());
		return e.code == KMR_ERR_NO_DEVICE ? 3 : 1;
	}
	return 0;
}
