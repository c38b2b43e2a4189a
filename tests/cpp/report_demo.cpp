// The artifact filter's report through the C++ host side (include/kmernator_amd.hpp), no reference headers:
//   report_demo <fastq> <artifacts.fa> <out-file> <phix-index>
// artifact filter without built-in or query-time edits over reads paired (2i, 2i + 1), then FilterKnownOddities::report: the records
// go to <out-file>, the counters and the segment table to stdout.
#include <cstdlib>
#include <fstream>
#include <iterator>
#include "kmernator_amd.hpp"

using namespace kmernator;

static std::string slurp(const char *path) { std::ifstream f(path, std::ios::binary); return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }

int main(int argc, char **argv) {
	if (argc < 5) { std::fprintf(stderr, "usage: report_demo <fastq> <artifacts.fa> <out-file> <phix-index>\n"); return 2; }
	try {
		KmerSpectrum sp(KmerSpectrum::defaults(31, 46000));
		ReadSet input(sp, slurp(argv[1]));
		kmr_artifact_config ac = FilterKnownOddities::defaults(sp.config());
		ac.edit_distance = 0; ac.phix_idx = (uint32_t)std::atoi(argv[4]);
		FilterKnownOddities filter(sp, slurp(argv[2]), ac);
		const uint64_t n = input.getSize();
		std::vector<int64_t> mate(n), read1, read2;
		for (uint64_t i = 0; i < n; i++) mate[i] = (i ^ 1) < n ? (int64_t)(i ^ 1) : -1;
		for (uint64_t i = 0; i < n; i += 2) { read1.push_back((int64_t)i); read2.push_back(i + 1 < n ? (int64_t)(i + 1) : -1); }
		FilterKnownOddities::Results fr;
		std::unique_ptr<ReadSet> reads = filter.applyFilter(input, fr, mate.data());
		kmr_artifact_report_config rc = FilterKnownOddities::reportDefaults();
		rc.phix_output = ac.phix_idx != 0;
		const FilterKnownOddities::Report rep = filter.report(input, fr, rc, read1.data(), read2.data(), read1.size());
		{ std::ofstream o(argv[3], std::ios::binary); o << rep.text; }
		for (size_t v = 0; v < rep.bases.size(); v++)
			if (rep.bases[v]) std::printf("%llu %llu %llu %s\n", (unsigned long long)rep.discarded[v], (unsigned long long)rep.trimmed[v], (unsigned long long)rep.bases[v], filter.getFilterName((uint32_t)v).c_str());
		for (size_t s = 0; s < rep.segBytes.size(); s++) std::printf("segment %llu %llu %llu\n", (unsigned long long)rep.segRecords[s], (unsigned long long)rep.segFirstByte[s], (unsigned long long)rep.segBytes[s]);
	} catch (const KmerSpectrumError &e) {
		std::fprintf(stderr, "%s\n", e.what());
		return e.code == KMR_ERR_NO_DEVICE ? 3 : 1;
	}
	return 0;
}
