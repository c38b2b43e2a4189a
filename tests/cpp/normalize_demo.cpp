// FilterReads --max-kmer-output-depth through the C++ host side (include/kmernator_amd.hpp), no reference headers:
//   normalize_demo <fastq> <out-prefix> <target-depth> <seed> <first-read-idx>
// spectrum of the reads (min depth 2), then ReadSelector::selectReadsNormalized in its fused form over the pairs (2i, 2i + 1), as
// test/runFilterTests.sh pairs them: one file under the reference's name, <out-prefix>-MinDepth2-MaxDepth<T>-reads.fastq.
#include <cstdlib>
#include <fstream>
#include <iterator>
#include "kmernator_amd.hpp"

using namespace kmernator;

static std::string slurp(const char *path) { std::ifstream f(path, std::ios::binary); return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }

int main(int argc, char **argv) {
	if (argc < 6) { std::fprintf(stderr, "usage: normalize_demo <fastq> <out-prefix> <target-depth> <seed> <first-read-idx>\n"); return 2; }
	try {
		KmerSpectrum sp(KmerSpectrum::defaults(31, 46000));
		ReadSet reads(sp, slurp(argv[1]));
		sp.buildKmerSpectrum(reads);
		sp.purgeMinDepth(2);
		std::vector<int64_t> read1, read2;
		for (uint64_t i = 0; i + 1 < reads.getSize(); i += 2) { read1.push_back((int64_t)i); read2.push_back((int64_t)i + 1); }
		kmr_normalize_config cfg = ReadSelector::normalizeDefaults();
		cfg.select.min_read_length = 25.0f; cfg.select.output_quality_base = 64;
		cfg.target_depth = std::strtoull(argv[3], nullptr, 10); cfg.seed = std::strtoull(argv[4], nullptr, 10); cfg.first_global_read_idx = std::strtoull(argv[5], nullptr, 10);
		cfg.by_pair = 1;
		ReadSelector sel(sp, reads);
		sel.setPairs(read1.data(), read2.data(), read1.size());
		const auto files = sel.selectReadsNormalized(cfg, std::vector<uint64_t>(), std::vector<std::string>(1, "reads"), argv[2]);
		for (const auto &f : files) { std::ofstream o(f.first, std::ios::binary); o << f.second; std::printf("%s %llu\n", f.first.c_str(), (unsigned long long)f.second.size()); }
		const ReadSelector::NormalizeInfo info = sel.normalizeInfo();
		std::printf("reads %llu records %llu picks %llu candidates %llu draws %llu\n", (unsigned long long)reads.getSize(), (unsigned long long)sel.getNumPicks(),
		            (unsigned long long)info.picks, (unsigned long long)info.candidates, (unsigned long long)info.draws);
	} catch (const KmerSpectrumError &e) {
		std::fprintf(stderr, "%s\n", e.what());
		return e.code == KMR_ERR_NO_DEVICE ? 3 : 1;
	}
	return 0;
}
