/*
 * kmr_select_rounds.hpp -- the host arithmetic of selectReads' partitioned branch (apps/FilterReads.h:209-278): the table of
 * rounds and the check of the caller's input boundaries.  Plain C++ without HIP, so that it also compiles into a stand-alone
 * program (tests/cpp/partition_rounds_check.cpp, which runs it under the host sanitizers).
 */
#ifndef KMR_SELECT_ROUNDS_HPP_
#define KMR_SELECT_ROUNDS_HPP_

#include <stdint.h>

namespace kmr {

enum { SEL_MAX_ROUNDS = 33 };      /* 32 halvings of a 32-bit depth and the remainder round */

/* one row per round, in the order the rounds run; handed to the kernels by value */
struct SelRounds {
	uint32_t n;
	float min_score[SEL_MAX_ROUNDS];            /* tmpMinDepth, a float as in the reference (:223) */
	float min_read_length[SEL_MAX_ROUNDS];
	uint8_t both_pass[SEL_MAX_ROUNDS];
	uint8_t is_remainder[SEL_MAX_ROUNDS];
};

/* The loop of apps/FilterReads.h:211-272 taken literally, unsigned arithmetic included: depth starts at partitionByDepth
 * (at minDepth when that is 0), is halved while it stays >= minDepth, and only a round that lands ON minDepth may start the
 * remainder round (min-passing-in-pair 1, min-read-length = remainderTrim).  16 over 2 gives 16 8 4 2, 20 over 3 gives
 * 20 10 5 and no remainder, 1 over 2 gives nothing.  Returns 0, or -1 if the table would hold more than SEL_MAX_ROUNDS rows
 * (minDepth 0 under a depth of 2^31 or more). */
inline int sel_round_table(unsigned int minDepth, unsigned int partitionByDepth, float remainderTrim, float minReadLength, bool bothPass, SelRounds &R) {
	R.n = 0;
	unsigned int maxDepth = partitionByDepth;
	const bool isPartitioned = maxDepth > 0;
	if (!isPartitioned) maxDepth = minDepth;
	int minPassingInPair = bothPass ? 2 : 1;
	bool hasRemainderTrim = false;
	for (unsigned int depth = maxDepth; depth >= minDepth; depth /= 2) {
		const float tmpMinDepth = (float)(minDepth > depth ? minDepth : depth);
		if (R.n == SEL_MAX_ROUNDS) return -1;
		R.min_score[R.n] = tmpMinDepth; R.min_read_length[R.n] = minReadLength;
		R.both_pass[R.n] = minPassingInPair == 2; R.is_remainder[R.n] = hasRemainderTrim;
		R.n++;
		if (depth == minDepth) {
			/* (int) getMinReadLength() != getRemainderTrim(), :261: the int goes back to float for the comparison */
			const float asInt = minReadLength < 2147483648.0f ? (float)(int)minReadLength : minReadLength;
			if (!hasRemainderTrim && isPartitioned && remainderTrim > 0.0f && (minPassingInPair != 1 || asInt != remainderTrim)) {
				minPassingInPair = 1;
				minReadLength = remainderTrim;
				hasRemainderTrim = true;
				depth *= 2;
			} else break;
		}
	}
	return 0;
}

/* input_starts: n_inputs + 1 read indices, the first 0, never descending (an input may be empty).  Returns 0 or the index of
 * the first entry that is out of place (0 for a first entry that is not 0). */
inline uint32_t sel_check_input_starts(const uint64_t *starts, uint32_t n_inputs, bool *ok) {
	*ok = false;
	if (starts[0] != 0) return 0;
	for (uint32_t j = 1; j <= n_inputs; j++) if (starts[j] < starts[j - 1]) return j;
	*ok = true;
	return 0;
}

}  // namespace kmr
#endif
