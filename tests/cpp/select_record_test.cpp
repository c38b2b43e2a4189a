/* sel_label, sel_measure / sel_record_bytes and sel_emit / sel_put_record of kmernator_amd/csrc/kmr_select.hpp (plain integer code
 * apart from atomicOr and the wavefront fences) as host functions, the 64 lanes of a wavefront one after the other, against labels and
 * records made with snprintf and std::string: every decimal width in every number of a label, every scoring name, the scores where
 * (int)(score + 0.5) rounds, clamps or has no meaning, the longest label followed by the shortest in the same buffer; names of every
 * length across one and two strides of 64, slices that put every section border on every lane, the clamps of a slice, both formats,
 * both output bases, reads without qualities.  A label is written into a heap block of exactly its measured length and a record into
 * one of exactly `bytes` bytes, so the address sanitizer sees a byte out of range, and again between guard bytes that must stay.
 *   g++ -std=c++17 -fsanitize=address,undefined -Itests/cpp/hipstub -Ikmernator_amd/csrc tests/cpp/select_record_test.cpp */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "kmr_select.hpp"

using namespace kmr;

static const uint32_t EDGE[] = {0u, 9u, 10u, 99u, 100u, 999u, 1000u, 9999u, 10000u, 99999u, 100000u, 999999u, 1000000u, 9999999u, 10000000u,
                                99999999u, 100000000u, 999999999u, 1000000000u, 4294967295u};
static const int N_EDGE = sizeof(EDGE) / sizeof(EDGE[0]);
static const char *NAMES[] = {"Score", "MedianScore", "MinScore", "MaxScore", "AvgScore"};
static const uint8_t GUARD = 0xA5;
static const int N_GUARD = 32;

static long long checks = 0;
static int wrong = 0;

/* one read batch and its per-read arrays */
struct Batch {
	std::vector<uint8_t> bases, quals, text, act, wt;
	std::vector<uint64_t> offsets, name_off, words;
	std::vector<uint32_t> name_len, af_min, af_max, to, tl;
	std::vector<float> score;
	Batch() { offsets.push_back(0); }
	uint64_t add(const std::string &name_line, const std::string &b, const std::string &q) {
		text.push_back('@'); name_off.push_back(text.size()); name_len.push_back((uint32_t)name_line.size());
		text.insert(text.end(), name_line.begin(), name_line.end()); text.push_back('\n');
		bases.insert(bases.end(), b.begin(), b.end()); quals.insert(quals.end(), q.begin(), q.end()); offsets.push_back(bases.size());
		act.push_back(0); wt.push_back(0); words.push_back(0); af_min.push_back(0); af_max.push_back(0); to.push_back(0); tl.push_back((uint32_t)b.size()); score.push_back(5.0f);
		return offsets.size() - 2;
	}
	SelectParams params(uint32_t scoring, bool fasta, uint32_t in_base, uint32_t out_base) const {
		SelectParams P;
		memset(&P, 0, sizeof P);
		P.bases = bases.data(); P.quals = quals.data(); P.offsets = offsets.data(); P.name_off = name_off.data(); P.name_len = name_len.data();
		P.text = text.data(); P.text_len = text.size(); P.af_action = act.data(); P.af_min = af_min.data(); P.af_max = af_max.data();
		P.trim_off = to.data(); P.trim_len = tl.data(); P.score = score.data(); P.was_trimmed = wt.data(); P.bimodal = words.data();
		P.n = offsets.size() - 1; P.scoring = scoring; P.fasta = fasta ? 1u : 0u; P.out_base = out_base; P.qual_shift = (int32_t)out_base - (int32_t)in_base;
		return P;
	}
};

/* the number the label shows for a score: the reference's cast where C++ defines it, this library's rule elsewhere */
static long long shown_score(float score) {
	if (isnan(score)) return 0;
	const double s = (double)score + 0.5;
	if (s >= 2147483648.0) return 2147483647ll;
	if (s <= -2147483649.0) return -2147483648ll;
	return (long long)s;      /* truncates toward zero, and is in range */
}
static std::string label_of(const Batch &B, uint64_t i, uint32_t scoring) {
	char buf[256];
	std::string s;
	if (B.act[i] == 2) return s;
	if (B.act[i] == 1) { snprintf(buf, sizeof buf, " AFTrim:%u+%lld", B.af_min[i], (long long)B.af_max[i] - (long long)B.af_min[i]); s += buf; }
	if (B.words[i]) {
		const unsigned m1 = (unsigned)(B.words[i] >> 32) & 0xffffu, m2 = (unsigned)(B.words[i] >> 48);
		snprintf(buf, sizeof buf, " %sBimodal@%u:%u/%u", m1 < m2 ? "Inv" : "", (unsigned)(B.words[i] & 0xffffffffu), m1, m2); s += buf;
	}
	if (B.wt[i]) { snprintf(buf, sizeof buf, " Trim:%u+%u", B.to[i], B.tl[i]); s += buf; }
	snprintf(buf, sizeof buf, " %s:%lld", NAMES[scoring], shown_score(B.score[i])); s += buf;
	return s;
}
static std::string record_of(const Batch &B, uint64_t i, uint32_t scoring, bool fasta, uint32_t in_base, uint32_t out_base) {
	const uint64_t b0 = B.offsets[i], L = B.offsets[i + 1] - b0;
	std::string name((const char *)B.text.data() + B.name_off[i], B.name_len[i]);
	name = name.substr(0, name.find_first_of(" \t"));
	uint64_t to = B.to[i], tl = B.tl[i];
	if (to >= L) tl = 0; else if (tl > L - to) tl = L - to;
	std::string bases = "N", quals(1, (char)(out_base + 1));
	if (B.act[i] != 2 && tl > 1) {
		bases.assign((const char *)B.bases.data() + b0 + to, tl);
		quals.assign(tl, (char)103);
		if (B.quals[b0] != 127 && B.quals[b0 + to] != 127) for (uint64_t j = 0; j < tl; j++) quals[j] = (char)(B.quals[b0 + to + j] + out_base - in_base);
	}
	const std::string head = name + label_of(B, i, scoring) + "\n" + bases + "\n";
	return fasta ? ">" + head : "@" + head + "+\n" + quals + "\n";
}

/* the label of read i: measured, written into a block of exactly that length, and compared */
static void check_label(const Batch &B, uint64_t i, uint32_t scoring) {
	const SelectParams P = B.params(scoring, false, 33, 33);
	const std::string want = label_of(B, i, scoring);
	const uint32_t n = sel_label(P, i, nullptr, false);
	uint8_t *block = (uint8_t *)malloc(n ? n : 1);
	const uint32_t m = sel_label(P, i, block, true);
	if (n != m || n != want.size() || n > (uint32_t)SEL_LABEL_MOST || memcmp(block, want.data(), n) != 0) {
		if (wrong++ < 10) printf("WRONG label read %llu scoring %u: measured %u written %u, wanted \"%s\"\n", (unsigned long long)i, scoring, n, m, want.c_str());
	}
	free(block);
	checks++;
}

/* read i's record by the 64 lanes in turn: into a block of exactly `bytes` bytes, and between guards */
static void check_record(const Batch &B, uint64_t i, uint32_t scoring, bool fasta, uint32_t in_base, uint32_t out_base, uint8_t *s_label) {
	const SelectParams P = B.params(scoring, fasta, in_base, out_base);
	const std::string want = record_of(B, i, scoring, fasta, in_base, out_base);
	uint32_t nlen = 0, err = 0;
	const uint32_t bytes = sel_measure(P, i, &nlen, &err);
	bool ok = err == 0 && bytes == want.size();
	if (ok) {
		uint8_t *block = (uint8_t *)calloc(bytes, 1);
		for (int lane = 0; lane < 64; lane++) sel_emit(P, i, nlen, bytes, block, lane, s_label);
		ok = memcmp(block, want.data(), bytes) == 0;
		free(block);
		std::vector<uint8_t> guarded((size_t)bytes + 2 * N_GUARD, GUARD);
		for (int lane = 63; lane >= 0; lane--) sel_emit(P, i, nlen, bytes, guarded.data() + N_GUARD, lane, s_label);      /* lane 0 last: the label is still the one of the block above */
		ok = ok && memcmp(guarded.data() + N_GUARD, want.data(), bytes) == 0;
		for (int g = 0; g < N_GUARD; g++) ok = ok && guarded[g] == GUARD && guarded[N_GUARD + bytes + g] == GUARD;
	}
	if (!ok && wrong++ < 10) printf("WRONG record read %llu scoring %u fasta %d base %u -> %u: %u bytes, wanted %zu: %s", (unsigned long long)i, scoring, (int)fasta, in_base, out_base, bytes, want.size(), want.c_str());
	checks++;
}

static std::string acgt(size_t n, unsigned seed) { std::string s(n, 'A'); for (size_t j = 0; j < n; j++) s[j] = "ACGT"[(j * 7 + seed + j / 5) & 3]; return s; }
static std::string quals_of(size_t n, unsigned seed, uint32_t base) { std::string s(n, '!'); for (size_t j = 0; j < n; j++) s[j] = (char)(base + 2 + (j * 11 + seed) % 39); return s; }

static void labels() {
	Batch B;
	/* every width in every number, differences of both signs, every pair of means */
	static const unsigned MEANS[3] = {0, 1, 65535};
	for (int a = 0; a < N_EDGE; a++) for (int b = 0; b < N_EDGE; b++) {
		const uint64_t i = B.add("w", acgt(8, a), quals_of(8, b, 33));
		B.act[i] = 1; B.af_min[i] = EDGE[a]; B.af_max[i] = EDGE[b]; B.to[i] = EDGE[b]; B.tl[i] = EDGE[a]; B.wt[i] = 1;
		B.words[i] = (uint64_t)EDGE[(a + b) % N_EDGE] | ((uint64_t)MEANS[a % 3] << 32) | ((uint64_t)MEANS[b % 3] << 48);
		B.score[i] = (b & 1) ? -(float)EDGE[a] : (float)EDGE[a];
	}
	/* the scores: the halves, just below them, between -1 and 0, the int range's ends and beyond, no number at all */
	static const float SCORES[] = {2.5f, 2.4999998f, 0.49999997f, 0.5f, 1.5f, -0.4f, -0.5f, -0.6f, -1.0f, -1.5f, 0.0f, -0.0f, 2147483520.0f, 2147483648.0f, -2147483648.0f,
	                               -2147483904.0f, 3e38f, -3e38f, INFINITY, -INFINITY, NAN, -NAN};
	for (size_t k = 0; k < sizeof SCORES / sizeof SCORES[0]; k++) {
		const uint64_t i = B.add("s", acgt(8, (unsigned)k), quals_of(8, (unsigned)k, 33));
		B.score[i] = SCORES[k]; B.wt[i] = k & 1; B.act[i] = k % 3 == 2 ? 2 : 0;      /* some discarded: no label at all */
	}
	for (uint32_t scoring = 0; scoring < 5; scoring++) {
		for (uint64_t i = 0; i + 1 < B.offsets.size(); i++) check_label(B, i, scoring);
		printf("labels %s ok\n", NAMES[scoring]);
	}
	/* the longest label there is, then the shortest through the same wavefront buffer: nothing of the first is left in the record */
	Batch Z;
	const uint64_t a = Z.add("a", "ACGTAC", "IIIIII"), b = Z.add("b", "ACGTAC", "555555");
	Z.act[a] = 1; Z.af_min[a] = 4294967295u; Z.af_max[a] = 0; Z.words[a] = 4294967295ull | (10000ull << 32) | (65535ull << 48); Z.to[a] = Z.tl[a] = 4294967295u; Z.wt[a] = 1;
	Z.score[a] = -2147483648.0f;
	const SelectParams P = Z.params(1, false, 33, 33);
	if (sel_label(P, a, nullptr, false) != (uint32_t)SEL_LABEL_MOST) { printf("WRONG: the longest label is %u bytes, SEL_LABEL_MOST %d\n", sel_label(P, a, nullptr, false), SEL_LABEL_MOST); wrong++; }
	check_label(Z, a, 1);
	uint8_t *s_label = (uint8_t *)malloc(SEL_LABEL_CAP);      /* exactly the wavefront's LDS bytes */
	check_record(Z, a, 1, false, 33, 33, s_label);
	check_record(Z, b, 1, false, 33, 33, s_label);
	check_record(Z, a, 0, true, 33, 64, s_label);
	check_record(Z, b, 0, true, 33, 64, s_label);
	free(s_label);
	printf("longest label ok\n");
}

static void geometry() {
	uint8_t *s_label = (uint8_t *)malloc(SEL_LABEL_CAP);
	static const char *TAILS[] = {"", " c x", "\tc x", "\t", " "};
	for (int in64 = 0; in64 < 2; in64++) {
		const uint32_t in_base = in64 ? 64 : 33;
		Batch B;
		/* names 1 .. 200 with a slice that moves along with them, then every slice length 0 .. 200 under four short names */
		for (uint32_t nl = 1; nl <= 200; nl++) {
			const uint32_t L = 3 + nl % 70;
			const uint64_t i = B.add(std::string(nl, (char)('a' + nl % 26)) + TAILS[nl % 5], acgt(L, nl), quals_of(L, nl, in_base));
			B.to[i] = nl % 3; B.tl[i] = L - nl % 3;
		}
		for (uint32_t nl = 1; nl <= 4; nl++) for (uint32_t bl = 0; bl <= 200; bl++) {
			const uint32_t L = bl + 2;
			const uint64_t i = B.add(std::string(nl, 'n') + TAILS[bl % 5], acgt(L, bl), quals_of(L, bl, in_base));
			B.to[i] = 1; B.tl[i] = bl; B.wt[i] = bl & 1;
		}
		/* the clamps of a slice, a discarded read, reads without qualities */
		static const uint32_t CL[][2] = {{29, 5}, {30, 5}, {35, 5}, {10, 21}, {0, 31}, {0, 0}, {0, 1}, {0, 2}, {28, 2}, {28, 3}, {29, 1}, {4294967295u, 2}, {2, 4294967295u}};
		for (size_t k = 0; k < sizeof CL / sizeof CL[0]; k++) for (int kind = 0; kind < 4; kind++) {
			std::string q = quals_of(30, (unsigned)k, in_base);
			if (kind == 1) q[0] = 127;                                 /* no qualities */
			if (kind == 2) q[CL[k][0] < 30 ? CL[k][0] : 5] = 127;        /* the slice starts on a 127 */
			if (kind == 3) q[29] = 127;                                /* a 127 behind real qualities */
			const uint64_t i = B.add("c", acgt(30, (unsigned)k), q);
			B.to[i] = CL[k][0]; B.tl[i] = CL[k][1]; B.wt[i] = 1;
		}
		const uint64_t d = B.add("d", acgt(30, 1), quals_of(30, 1, in_base));
		B.act[d] = 2;
		for (int fasta = 0; fasta < 2; fasta++) for (uint32_t out_base = 33; out_base <= 64; out_base += 31) {
			for (uint64_t i = 0; i + 1 < B.offsets.size(); i++) check_record(B, i, 1, fasta != 0, in_base, out_base, s_label);
			printf("records base %u -> %u %s ok\n", in_base, out_base, fasta ? "fasta" : "fastq");
		}
	}
	free(s_label);
}

int main() {
	labels();
	geometry();
	printf("%lld checks, %d wrong\n", checks, wrong);
	return wrong ? 1 : 0;
}
