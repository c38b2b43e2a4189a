// cut_runs (kmernator_amd/csrc/kmr_runs.hpp) on its own, so that it can run under the host sanitizers (-fsanitize=address,undefined):
// how kmr_compare_reads* and kmr_extend_contigs* cut a batch into runs of whole groups whose k-mer slots fit a staging budget.  Every
// case names the cut it expects, and every cut is held to the rule as well: a run fits the budget or is one group, and no run could
// have taken the next group too.  Prints one line per case; exit status 0 = every expectation held.
#include <cstdio>
#include <vector>

#include "../../kmernator_amd/csrc/kmr_runs.hpp"

typedef std::vector<uint64_t> Vec;
static int failures = 0;

static void expect_cut(const char *what, const Vec &sizes, uint64_t budget, const Vec &want) {
	const uint64_t n = sizes.size();
	Vec upto(n + 1, 0);
	for (uint64_t g = 0; g < n; g++) upto[g + 1] = upto[g] + sizes[g];
	const Vec cut = kmr_host::cut_runs(n, budget, [&](uint64_t g) { return upto.at(g); });
	bool ok = cut == want && cut.size() >= 2 && cut.front() == 0 && cut.back() == n;
	for (size_t i = 0; ok && i + 1 < cut.size(); i++) {
		const uint64_t a = cut[i], b = cut[i + 1];
		ok = (b > a || n == 0) && (upto[b] - upto[a] <= budget || b - a == 1);      /* fits, or one group alone */
		if (ok && b < n) ok = upto[b + 1] - upto[a] > budget;                       /* the next group did not fit */
	}
	std::printf("%-58s budget %-4llu runs %zu %s\n", what, (unsigned long long)budget, cut.size() - 1, ok ? "ok" : "WRONG");
	if (!ok) failures++;
}

int main() {
	expect_cut("budget above the total: one run", {3, 4, 5}, 100, {0, 3});
	expect_cut("budget equal to the total: one run", {3, 4, 5}, 12, {0, 3});
	expect_cut("one slot less than the total", {3, 4, 5}, 11, {0, 2, 3});
	expect_cut("budget 0: every full group alone", {1, 2, 3}, 0, {0, 1, 2, 3});
	expect_cut("budget 0: empty groups ride along", {0, 0, 2, 0}, 0, {0, 2, 3, 4});
	expect_cut("budget 1", {1, 1, 1}, 1, {0, 1, 2, 3});
	expect_cut("budget 1 across an empty group", {1, 0, 1}, 1, {0, 2, 3});
	expect_cut("oversize group first", {10, 2, 2}, 5, {0, 1, 3});
	expect_cut("oversize group in the middle: neighbours not merged", {2, 2, 10, 2, 2}, 5, {0, 2, 3, 5});
	expect_cut("oversize group last", {2, 2, 10}, 5, {0, 2, 3});
	expect_cut("oversize groups only", {9, 9, 9}, 5, {0, 1, 2, 3});
	expect_cut("oversize behind an empty group", {0, 10}, 5, {0, 1, 2});
	expect_cut("empty groups between full ones, budget of two", {3, 0, 0, 3, 0, 3}, 6, {0, 5, 6});
	expect_cut("empty groups between full ones, budget of one", {3, 0, 0, 3, 0, 3}, 3, {0, 3, 5, 6});
	expect_cut("empty groups only", {0, 0, 0}, 0, {0, 3});
	expect_cut("one group", {7}, 3, {0, 1});
	expect_cut("no group", {}, 5, {0, 0});

	// the extender's addressing: group c is contig c with its pool, items hpo[c] + c up to hpo[c + 1] + c + 1 of the item scan hk
	const Vec hpo = {0, 2, 2, 5}, hk = {0, 4, 8, 9, 10, 13, 16, 19, 20};      // items: 3, 1, 4 -> slots 9, 1, 10
	const Vec cut = kmr_host::cut_runs(3, 10, [&](uint64_t c) { return hk.at(hpo.at(c) + c); });
	const bool ok = cut == Vec({0, 2, 3});
	std::printf("%-58s budget %-4d runs %zu %s\n", "through the extender's item offsets", 10, cut.size() - 1, ok ? "ok" : "WRONG");
	if (!ok) failures++;
	return failures ? 1 : 0;
}
