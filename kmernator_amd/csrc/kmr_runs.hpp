/* kmr_runs.hpp -- how a batch whose k-mer slots exceed a staging budget is cut into runs (kmr_compare_reads*: whole reads;
 * kmr_extend_contigs*: whole contigs with their pools).  Plain C++, no HIP: tests/cpp/cut_runs_test.cpp includes it. */
#ifndef KMR_RUNS_HPP_
#define KMR_RUNS_HPP_
#include <stdint.h>
#include <vector>

namespace kmr_host {
/* Runs of whole groups whose slots fit the budget; a group that alone exceeds it is a run of its own.  slots_upto(g): the slots of
 * the groups before g, g <= n_groups.  Returns the first group of every run, and n_groups: run i is [cut[i], cut[i + 1]) */
template <class F> std::vector<uint64_t> cut_runs(uint64_t n_groups, uint64_t budget, F slots_upto) {
	std::vector<uint64_t> cut(1, 0);
	uint64_t g0 = 0;
	for (uint64_t g = 0; g < n_groups; g++) if (slots_upto(g + 1) - slots_upto(g0) > budget && g > g0) { cut.push_back(g); g0 = g; }
	cut.push_back(n_groups);
	return cut;
}
}  // namespace kmr_host
#endif
