/* dump_line and dump_size_kernel of kmernator_amd/csrc/kmr_dump.hpp (plain integer code apart from atomicOr) as host functions,
 * against lines made with snprintf and a base-by-base reverse complement: every k on both sides of a byte, a word and a pad border,
 * numbers of every width with 4294967295 and 0 among them, both lines of both texts, and a line placed at every byte offset across
 * a tile's start and end and at all four phases inside -- what lies outside the tile must be dropped, what lies inside must be the
 * line's bytes and nothing else.  The tile is a heap block of exactly its size, so the address sanitizer sees a word out of range.
 * The walk over tiles (dump_write_kernel) needs a workgroup and is tested on the device (tests/test_gpu_dump_edges.py).
 *   g++ -std=c++17 -fsanitize=address,undefined -Itests/cpp/hipstub -Ikmernator_amd/csrc tests/cpp/dump_line_test.cpp */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "kmr_dump.hpp"

using namespace kmr;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static const uint32_t EDGE[] = {0u, 9u, 10u, 99u, 100u, 999u, 1000u, 9999u, 10000u, 99999u, 100000u, 999999u, 1000000u, 9999999u, 10000000u,
                                99999999u, 100000000u, 999999999u, 1000000000u, 4294967295u};
static const int N_EDGE = sizeof(EDGE) / sizeof(EDGE[0]);

static std::string bases_of(const uint64_t *kw, uint32_t k) {
	std::string s(k, '?');
	for (uint32_t p = 0; p < k; p++) s[p] = "ACGT"[(kw[p >> 5] >> (62 - 2 * (p & 31))) & 3];
	return s;
}
static std::string reverse_complement(const std::string &s) {
	std::string r(s.rbegin(), s.rend());
	for (size_t i = 0; i < r.size(); i++) r[i] = r[i] == 'A' ? 'T' : r[i] == 'C' ? 'G' : r[i] == 'G' ? 'C' : 'A';
	return r;
}
/* ExtensionTracking::getReverseComplement by its loop: A <-> T, C <-> G, N and X stay; left and right change places */
static void tallies_rc(const uint32_t *t, uint32_t *out) {
	static const int rc[6] = {3, 2, 1, 0, 4, 5};
	for (int i = 0; i < 6; i++) { out[rc[i]] = t[6 + i]; out[6 + rc[i]] = t[i]; }
}
static std::string line_of(const std::string &seq, bool graph, uint32_t count, const uint32_t *t) {
	char buf[512];
	if (!graph) snprintf(buf, sizeof buf, "\t%u\n", count);
	else snprintf(buf, sizeof buf, "\t%u %u %u %u %u %u %u %u %u %u %u %u 0\n", t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], t[9], t[10], t[11]);
	return seq + buf;
}

static long long checks = 0;
static int wrong = 0;

template <int W>
static void run_k(uint32_t k, uint32_t *tile) {
	const int n = 12;
	const uint32_t vw = 15;
	std::vector<uint64_t> keys((size_t)n * W, 0);
	std::vector<uint32_t> vals((size_t)n * vw, 0);
	for (int e = 0; e < n; e++) {
		for (uint32_t p = 0; p < k; p++) {
			const uint64_t code = e == 0 ? 0 : e == 1 ? 3 : rnd() & 3;      /* A^k, T^k, then random */
			keys[(size_t)e * W + (p >> 5)] |= code << (62 - 2 * (p & 31));
		}
		vals[e * vw] = (e < 4 ? (uint32_t[]){0u, 9u, 10000u, 65535u}[e] : (uint32_t)(rnd() & 0xffff)) | ((uint32_t)rnd() << 16);      /* the count's word holds padding above */
		for (int j = 0; j < 12; j++) vals[e * vw + 3 + j] = (rnd() & 1) ? EDGE[rnd() % N_EDGE] : (uint32_t)(rnd() >> (rnd() & 31));
		if (e == 2) for (int j = 0; j < 12; j++) vals[e * vw + 3 + j] = 4294967295u;
		if (e == 3) for (int j = 0; j < 12; j++) vals[e * vw + 3 + j] = 0;
	}
	for (int graph = 0; graph < 2; graph++) {
		DumpParams P;
		P.keys = keys.data(); P.vals = vals.data(); P.vw = vw; P.k = k; P.graph = (uint32_t)graph; P.min_depth = -1; P.lo = 0; P.n = n;
		std::vector<uint32_t> len(n);
		unsigned long long kept = 0;
		dump_size_kernel(P, len.data(), &kept);
		for (int e = 0; e < n; e++) {
			const std::string fwd = bases_of(&keys[(size_t)e * W], k);
			uint32_t rt[12];
			tallies_rc(&vals[e * vw + 3], rt);
			const std::string lines[2] = {line_of(fwd, graph, vals[e * vw] & 0xffffu, &vals[e * vw + 3]), line_of(reverse_complement(fwd), graph, vals[e * vw] & 0xffffu, rt)};
			if (len[e] != lines[0].size() + lines[1].size() || lines[0].size() != lines[1].size()) { printf("WRONG size k %u entry %d graph %d: %u\n", k, e, graph, len[e]); wrong++; }
			const int L = (int)lines[0].size();
			std::vector<int> ats;
			for (int at = -L - 4; at <= 8; at++) ats.push_back(at);
			for (int at = DUMP_TILE - L - 8; at <= DUMP_TILE - 1; at++) ats.push_back(at);
			for (int at = 1001; at < 1005; at++) ats.push_back(at);
			for (int rev = 0; rev < 2; rev++) for (int at : ats) {
				dump_line<W>(P, (uint64_t)e, rev != 0, at, tile);
				const uint8_t *b = (const uint8_t *)tile;
				const int w0 = at - 8 < 0 ? 0 : at - 8, w1 = at + L + 8 > DUMP_TILE ? DUMP_TILE : at + L + 8;
				bool ok = true;
				for (int p = w0; p < w1; p++) ok = ok && b[p] == (p >= at && p < at + L ? (uint8_t)lines[rev][p - at] : 0);
				if (!ok && wrong++ < 10) printf("WRONG k %u entry %d graph %d rev %d at %d\n", k, e, graph, rev, at);
				if (w1 > w0) memset(tile + w0 / 4, 0, (size_t)((w1 + 3) / 4 - w0 / 4) * 4);
				checks++;
			}
		}
		if (kept != (unsigned long long)n) { printf("WRONG kept k %u: %llu\n", k, kept); wrong++; }
	}
	for (int w = 0; w < DUMP_TILE_WORDS; w++) if (tile[w]) { printf("WRONG k %u: a byte far from its line, word %d\n", k, w); wrong++; break; }
}

int main() {
	uint32_t *tile = (uint32_t *)calloc(DUMP_TILE_WORDS, 4);
	for (uint32_t k = 1; k <= 128; k++) {
		if (k > 20 && !(k % 32 <= 1 || k % 32 == 31)) continue;
		if (k <= 32) run_k<1>(k, tile); else if (k <= 64) run_k<2>(k, tile); else if (k <= 96) run_k<3>(k, tile); else run_k<4>(k, tile);
		printf("k %u ok\n", k);
	}
	free(tile);
	printf("%lld placements, %d wrong\n", checks, wrong);
	return wrong ? 1 : 0;
}
