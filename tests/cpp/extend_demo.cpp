// ContigExtender of include/kmernator_amd.hpp from a C++ host.
//   extend_demo names                                          getNewName and getMinMaxKmerSize, no device
//   extend_demo extend K CONTIGS.fa READS.fastq POOLS.txt MAX  one line per contig: name, left, right, the two stop reasons, the twelve
//                                                              stop values as hexadecimal bits, the sequence
// POOLS.txt holds one line per contig: the indices of its pool's reads, blank separated.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "kmernator_amd.hpp"

using namespace kmernator;

static std::string slurp(const char *path) {
	std::ifstream f(path, std::ios::binary);
	std::stringstream s;
	s << f.rdbuf();
	return s.str();
}

int main(int argc, char **argv) {
	if (argc >= 2 && !strcmp(argv[1], "names")) {
		const char *names[] = {"c1", "c1-l3r4", "cell-1", "ctgl", "x-l2", "a-l1r2-l3r4"};
		for (const char *n : names) std::cout << n << " " << ContigExtender::getNewName(n, 0, 0) << " " << ContigExtender::getNewName(n, 2, 5) << "\n";
		uint32_t lo = 0, hi = 0, step = 0;
		if (kmr_extend_min_max_kmer_size(31, 150, 15000, 100, 6, &lo, &hi, &step) != KMR_OK) return 1;
		std::cout << lo << " " << hi << " " << step << "\n";
		return 0;
	}
	if (argc != 7 || strcmp(argv[1], "extend")) { std::cerr << "usage: extend_demo names | extend K CONTIGS.fa READS.fastq POOLS.txt MAX_EXTEND\n"; return 2; }
	try {
		KmerSpectrum sp(KmerSpectrum::defaults((uint32_t)atoi(argv[2]), 4096));
		std::unique_ptr<ReadSet> contigs = ReadSet::fromFasta(sp, slurp(argv[3]));
		ReadSet reads(sp, slurp(argv[4]), 33);
		std::vector<uint64_t> off(1, 0), idx;
		std::ifstream pf(argv[5]);
		std::string line;
		while (std::getline(pf, line)) {
			std::istringstream ls(line);
			uint64_t v;
			while (ls >> v) idx.push_back(v);
			off.push_back(idx.size());
		}
		std::vector<std::string> names;
		for (uint64_t i = 0; i < contigs->getSize(); i++) names.push_back(contigs->getName(i));
		kmr_extend_config cfg = ContigExtender::defaults();
		cfg.max_extend = (uint32_t)atoi(argv[6]);
		ContigExtender ex(sp, cfg);
		const ExtendResults r = ex.extendContigs(*contigs, reads, off, idx, names);
		for (size_t i = 0; i < r.sequences.size(); i++) {
			printf("%s %u %u %u %u", r.names[i].c_str(), r.left[i], r.right[i], r.stops[2 * i].reason, r.stops[2 * i + 1].reason);
			for (int side = 0; side < 2; side++) {
				const kmr_extend_stop &s = r.stops[2 * i + side];
				const double v[6] = {s.edge, s.ext[0], s.ext[1], s.ext[2], s.ext[3], s.total};
				for (double d : v) { uint64_t b; memcpy(&b, &d, 8); printf(" %016" PRIx64, b); }
			}
			printf(" %s\n", r.sequences[i].c_str());
		}
		printf("extended %" PRIu64 " bases %" PRIu64 " batch %" PRIu64 "\n", r.extended, r.basesAdded, r.readSet->getSize());
	} catch (const std::exception &e) { std::cerr << e.what() << "\n"; return 1; }
	return 0;
}
