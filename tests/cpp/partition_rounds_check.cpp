// The host arithmetic of the partitioned selection (kmernator_amd/csrc/kmr_select_rounds.hpp) on its own, so that it can run
// under the host sanitizers (-fsanitize=address,undefined): the table of rounds over the cases of apps/FilterReads.h:211-272 and
// the check of input_starts.  Prints one line per case; exit status 0 = every expectation held.
#include <cstdio>
#include <vector>

#include "../../kmernator_amd/csrc/kmr_select_rounds.hpp"

static int failures = 0;

static void expect_rounds(const char *what, unsigned minDepth, unsigned partition, float remainder, float minLength, bool both, int rc, std::vector<float> depths, int remainderAt) {
	kmr::SelRounds R;
	const int got = kmr::sel_round_table(minDepth, partition, remainder, minLength, both, R);
	bool ok = got == rc;
	if (ok && rc == 0) {
		ok = R.n == depths.size();
		for (uint32_t r = 0; ok && r < R.n; r++) ok = R.min_score[r] == depths[r] && (R.is_remainder[r] != 0) == ((int)r == remainderAt);
		if (ok && remainderAt >= 0) ok = R.min_read_length[remainderAt] == remainder && !R.both_pass[remainderAt];
	}
	std::printf("%-44s rc %d rounds %u %s\n", what, got, got ? 0u : R.n, ok ? "ok" : "WRONG");
	if (!ok) failures++;
}

int main() {
	expect_rounds("16 over 2", 2, 16, -1.0f, 0.40f, false, 0, {16, 8, 4, 2}, -1);
	expect_rounds("16 over 2, remainder 25", 2, 16, 25.0f, 0.40f, false, 0, {16, 8, 4, 2, 2}, 4);
	expect_rounds("20 over 3, remainder 25 (never reaches 3)", 3, 20, 25.0f, 0.40f, false, 0, {20, 10, 5}, -1);
	expect_rounds("2 over 2", 2, 2, -1.0f, 0.40f, false, 0, {2}, -1);
	expect_rounds("1 over 2 (no round)", 2, 1, 25.0f, 0.40f, false, 0, {}, -1);
	expect_rounds("off, remainder set", 2, 0, 25.0f, 0.40f, true, 0, {2}, -1);
	expect_rounds("remainder equal to the length, one passing", 2, 4, 25.0f, 25.9f, false, 0, {4, 2}, -1);
	expect_rounds("remainder equal to the length, both passing", 2, 4, 25.0f, 25.9f, true, 0, {4, 2, 2}, 2);
	expect_rounds("min depth 0", 0, 2, 3.0f, 0.40f, false, 0, {2, 1, 0, 0}, 3);
	expect_rounds("a huge minimum length", 2, 2, 25.0f, 3.0e38f, false, 0, {2, 2}, 1);
	std::vector<float> all;
	for (int b = 31; b >= 0; b--) all.push_back((float)(1u << b));
	expect_rounds("2^31 over 1: 32 rounds", 1, 1u << 31, -1.0f, 0.40f, false, 0, all, -1);
	all.push_back(1.0f);
	expect_rounds("2^31 over 1 and a remainder: 33 rounds", 1, 1u << 31, 25.0f, 0.40f, false, 0, all, 32);
	expect_rounds("2^32 - 1 over 0 and a remainder: 34 rounds", 0, 0xffffffffu, 25.0f, 0.40f, false, -1, {}, -1);
	expect_rounds("2^31 over 2^31: the doubled depth wraps", 1u << 31, 1u << 31, 25.0f, 0.40f, false, 0, {2147483648.0f}, -1);

	struct { const char *what; std::vector<uint64_t> starts; bool ok; uint32_t at; } cases[] = {
		{"one input", {0, 10}, true, 0}, {"an empty input", {0, 4, 4, 10}, true, 0}, {"does not start at 0", {1, 10}, false, 0},
		{"descends", {0, 7, 3, 10}, false, 2}, {"all empty", {0, 0, 0}, true, 0}};
	for (auto &c : cases) {
		bool ok;
		const uint32_t at = kmr::sel_check_input_starts(c.starts.data(), (uint32_t)c.starts.size() - 1, &ok);
		const bool good = ok == c.ok && at == c.at;
		std::printf("input_starts: %-30s %s at %u %s\n", c.what, ok ? "accepted" : "refused", at, good ? "ok" : "WRONG");
		if (!good) failures++;
	}
	return failures ? 1 : 0;
}
