// FilterReads --partition-by-depth through the C++ host side (include/kmernator_amd.hpp), no reference headers:
//   partition_demo <fastq> <artifacts.fa> <out-prefix> <min-read-length> <partition-by-depth> <remainder-trim>
// artifact filter (--artifact-edit-distance 1), spectrum of the filtered reads, then ReadSelector::selectReads: one file per round
// under the reference's names, <out-prefix>-MinDepth2-PartitionDepth<d>-reads.fastq and <out-prefix>-MinDepth2-Remainder-reads.fastq.
// The reads are paired (2i, 2i + 1), as test/runFilterTests.sh runs them.
#include <cstdlib>
#include <fstream>
#include <iterator>
#include "kmernator_amd.hpp"

using namespace kmernator;

static std::string slurp(const char *path) { std::ifstream f(path, std::ios::binary); return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }

int main(int argc, char **argv) {
	if (argc < 7) { std::fprintf(stderr, "usage: partition_demo <fastq> <artifacts.fa> <out-prefix> <min-read-length> <partition-by-depth> <remainder-trim>\n"); return 2; }
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
		kmr_partition_config cfg = ReadSelector::partitionDefaults();
		cfg.select.min_read_length = ac.min_read_length; cfg.select.output_quality_base = 64;
		cfg.partition_by_depth = (uint32_t)std::atoi(argv[5]); cfg.remainder_trim = (float)std::atof(argv[6]);
		ReadSelector sel(sp, *reads, mate.data(), &fr, mate.size());
		const auto files = sel.selectReads(cfg, std::vector<uint64_t>(), std::vector<std::string>(1, "reads"), argv[3]);
		const ReadSelector::Segments s = sel.segments();
		for (const auto &f : files) { std::ofstream o(f.first, std::ios::binary); o << f.second; std::printf("%s %llu\n", f.first.c_str(), (unsigned long long)f.second.size()); }
		std::printf("reads %llu picks %llu rounds %u\n", (unsigned long long)reads->getSize(), (unsigned long long)sel.getNumPicks(), s.nRounds);
	} catch (const KmerSpectrumError &e) {
		std::fprintf(stderr, "%s\n", e.what());
		return e.code == KMR_ERR_NO_DEVICE ? 3 : 1;
	}
	return 0;
}
