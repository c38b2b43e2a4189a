/* dedup_key_kernel of kmernator_amd/csrc/kmr_dedup.hpp (the 256-bit key built by shifts, its reverse complement on the key words, the
 * canonical choice by a multi-word comparison, the skip tests) as a host function over whole pair lists, one "lane" walking them all,
 * against keys this program builds itself, base by base, from strings: window 1 + reverse complement of window 2, four bases a byte,
 * compared with memcmp, the smaller of the forward and the reverse key in mode 2.  All sixteen dedup_length values x start_offset
 * 0, 4, 60, 64 x both modes x both passes; random reads around the needed length with N, lower case and X, every fragment also as
 * (B, A), keys that tie with their reverse complement up to a word border both ways round, palindromic keys, discarded reads, read
 * indices outside the batch, half pairs.  Every array is a heap block of exactly its size, so the address sanitizer sees an index
 * out of range.  The consensus kernel needs 64 lanes and is tested on the device (tests/test_gpu_dedup_edges.py).
 *   g++ -std=c++17 -fsanitize=address,undefined -Itests/cpp/hipstub -Ikmernator_amd/csrc tests/cpp/dedup_key_test.cpp */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "kmr_dedup.hpp"

using namespace kmr;

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static std::string rnd_bases(size_t n) { std::string s(n, 'A'); for (size_t i = 0; i < n; i++) s[i] = "ACGT"[rnd() & 3]; return s; }

/* what a base packs as, as a letter: anything but ACGT (either case) packs as A */
static char packed(char c) {
	switch (c) { case 'C': case 'c': return 'C'; case 'G': case 'g': return 'G'; case 'T': case 't': return 'T'; default: return 'A'; }
}
static std::string packed(const std::string &s) { std::string r(s); for (size_t i = 0; i < r.size(); i++) r[i] = packed(r[i]); return r; }
static std::string revcomp(const std::string &s) {
	std::string r(s.rbegin(), s.rend());
	for (size_t i = 0; i < r.size(); i++) r[i] = r[i] == 'A' ? 'T' : r[i] == 'C' ? 'G' : r[i] == 'G' ? 'C' : 'A';
	return r;
}
/* four bases a byte, the first in the high bits; s.size() is a multiple of 4 */
static std::vector<uint8_t> key_bytes(const std::string &s) {
	std::vector<uint8_t> b(s.size() / 4, 0);
	for (size_t i = 0; i < s.size(); i++) b[i / 4] |= (uint8_t)((s[i] == 'A' ? 0 : s[i] == 'C' ? 1 : s[i] == 'G' ? 2 : 3) << (6 - 2 * (i % 4)));
	return b;
}
/* word w of the key: its bytes 8 w .. 8 w + 7, the first the most significant, zeros behind the key's end */
static uint64_t key_word(const std::vector<uint8_t> &b, uint32_t w) {
	uint64_t v = 0;
	for (size_t i = 0; i < 8; i++) v = (v << 8) | (8 * w + i < b.size() ? b[8 * w + i] : 0);
	return v;
}
static size_t first_x(const std::string &s) { for (size_t i = 0; i < s.size(); i++) if (s[i] == 'X' || s[i] == 'x') return i; return s.size(); }

struct Batch {
	std::vector<std::string> reads;
	std::vector<uint8_t> discarded;
	std::vector<int64_t> read1, read2;
	void pair(const std::string &a, const std::string &b, int d1 = 0, int d2 = 0) {
		read1.push_back((int64_t)reads.size()); reads.push_back(a); discarded.push_back((uint8_t)d1);
		read2.push_back((int64_t)reads.size()); reads.push_back(b); discarded.push_back((uint8_t)d2);
	}
	void single(const std::string &a, bool second_side, int d = 0) {
		(second_side ? read2 : read1).push_back((int64_t)reads.size()); (second_side ? read1 : read2).push_back(-1);
		reads.push_back(a); discarded.push_back((uint8_t)d);
	}
};

/* a read around the needed length: mostly ACGT, now and then N, n, lower case, a dot; an X or x somewhere in one of eight */
static std::string noisy_read(uint32_t need) {
	const size_t len = (rnd() % 8 == 0) ? need - 1 - rnd() % 2 : need + rnd() % 7;
	std::string s = rnd_bases(len);
	for (size_t i = 0; i < len; i++) { const uint64_t r = rnd() % 40; if (r < 5) s[i] = "Nnacgt.R"[rnd() % 8]; }
	if (rnd() % 8 == 0 && len) s[rnd() % len] = (rnd() & 1) ? 'X' : 'x';
	return s;
}
/* a key of n bases that agrees with its reverse complement in bases 0 .. 32 w - 1 and differs at base 32 w */
static std::string tie_key(uint32_t n, uint32_t w, bool forward_less) {
	std::string k = rnd_bases(n);
	for (uint32_t i = 0; i < 32 * w; i++) k[n - 1 - i] = revcomp(std::string(1, k[i]))[0];
	const uint32_t i = 32 * w;
	k[i] = forward_less ? 'A' : 'C'; k[n - 1 - i] = forward_less ? 'G' : 'T';
	return k;
}

static long long records = 0;
static int wrong = 0;
static long long n_flipped = 0, n_forward = 0, n_ties_decided_late = 0, n_palindromes = 0;

static void run(uint32_t L, uint32_t so, bool mode2, bool paired) {
	const uint32_t win = paired ? L : 2 * L, need = so + win, W = (L / 2 + 7) / 8, nkey = 2 * L;
	Batch B;
	const std::string lead = rnd_bases(so);
	for (int i = 0; i < 24; i++) {
		const std::string a = noisy_read(need), b = noisy_read(need);
		B.pair(a, b); B.pair(b, a);
		B.single(a, i & 1);
	}
	/* keys chosen as keys: window 1 = key[0, L), window 2 = reverse complement of key[L, 2 L); in the single pass the key is the window */
	std::vector<std::string> chosen;
	std::vector<int> expect_flip;      /* 1, 0, or -1 for "whatever the comparison says" */
	for (uint32_t w = 0; 32 * w < nkey / 2; w++)
		for (int fl = 0; fl < 2; fl++) { chosen.push_back(tie_key(nkey, w, fl == 0)); expect_flip.push_back(fl); }
	{ const std::string half = rnd_bases(nkey / 2); chosen.push_back(half + revcomp(half)); expect_flip.push_back(0); }
	chosen.push_back(std::string(nkey, 'A')); expect_flip.push_back(0);       /* poly-A against poly-T */
	chosen.push_back(std::string(nkey, 'T')); expect_flip.push_back(1);
	const size_t first_chosen = B.read1.size();
	for (size_t c = 0; c < chosen.size(); c++) {
		const std::string &k = chosen[c];
		if (paired) B.pair(lead + k.substr(0, L) + rnd_bases(c % 3), lead + revcomp(k.substr(L)) + rnd_bases((c + 1) % 3));
		else B.single(lead + k + rnd_bases(c % 3), c & 1);
	}
	/* the skips: discarded (tested before the length), both ends short (one count), exactly long enough, X at the window's last base,
	 * behind it and in front of it, read indices outside the batch */
	const std::string good = lead + rnd_bases(win);
	B.pair(good, good, 1, 0); B.pair(good, good, 0, 1); B.pair(good.substr(0, need - 1), good, 1, 0); B.pair(good.substr(0, need - 1), good.substr(0, need - 1));
	B.pair(good, good + "X"); B.pair(good + "x", good); B.single(good + "x", false); B.single(good.substr(0, need - 1), true); B.single(good, true, 1);
	{ std::string x = good; x[need - 1] = 'X'; B.pair(x, good); B.pair(good, x); B.single(x, false); }
	if (so) { std::string x = good; x[so - 1] = 'x'; B.pair(x, good); B.pair(good, x); B.single(x, true); x = good; x[0] = 'X'; B.single(x, false); }
	const uint64_t n = B.reads.size();
	B.read1.push_back((int64_t)n); B.read2.push_back(0);
	B.read1.push_back(0); B.read2.push_back((int64_t)n + 5);
	B.read1.push_back(-1); B.read2.push_back((int64_t)n);
	B.read1.push_back(-1); B.read2.push_back(-1);
	const uint64_t np = B.read1.size();

	/* the batch as the kernel takes it */
	std::vector<uint64_t> offsets(n + 1, 0);
	for (uint64_t i = 0; i < n; i++) offsets[i + 1] = offsets[i] + B.reads[i].size();
	std::vector<uint8_t> bases(offsets[n]);
	for (uint64_t i = 0; i < n; i++) memcpy(bases.data() + offsets[i], B.reads[i].data(), B.reads[i].size());
	DedupParams P;
	memset(&P, 0, sizeof P);
	P.bases = bases.data(); P.offsets = offsets.data(); P.n = n; P.total = offsets[n];
	P.read1 = B.read1.data(); P.read2 = B.read2.data(); P.np = np; P.discarded = B.discarded.data();
	P.paired = paired; P.mode2 = mode2; P.L = win; P.so = so; P.W = W; P.sides = paired ? 2 : 1;
	std::vector<unsigned long long> keys((size_t)W * np, 0xa5a5a5a5a5a5a5a5ull);
	std::vector<uint32_t> cand(np, 7u);
	std::vector<uint8_t> flip(np, 7);
	std::vector<uint64_t> totals(DEDUP_T_WORDS, 0);
	dedup_key_kernel(P, keys.data(), cand.data(), flip.data(), totals.data());

	/* the same from the strings */
	uint64_t want_totals[4] = {0, 0, 0, 0};
	for (uint64_t i = 0; i < np; i++) {
		const int64_t r1 = B.read1[i], r2 = B.read2[i];
		bool ok = false, fl = false;
		std::vector<uint8_t> key;
		if (paired && r1 >= 0 && r2 >= 0) {
			if ((uint64_t)r1 >= n || (uint64_t)r2 >= n) want_totals[DEDUP_T_INVALID]++;
			else if (B.discarded[r1] || B.discarded[r2]) want_totals[DEDUP_T_DISCARD]++;
			else if (first_x(B.reads[r1]) < need || first_x(B.reads[r2]) < need) want_totals[DEDUP_T_SHORT]++;
			else {
				const std::string fwd = packed(B.reads[r1].substr(so, win)) + revcomp(packed(B.reads[r2].substr(so, win)));
				const std::string rev = revcomp(fwd);
				key = key_bytes(fwd);
				if (mode2) {
					const std::vector<uint8_t> rk = key_bytes(rev);
					if (memcmp(rk.data(), key.data(), key.size()) < 0) { key = rk; fl = true; }
					if (fl) n_flipped++; else n_forward++;
					if (key.size() > 8 && memcmp(key_bytes(fwd).data(), rk.data(), 8) == 0 && fwd != rev) n_ties_decided_late++;
					if (fwd == rev) n_palindromes++;
				}
				ok = true;
			}
		} else if (!paired && (r1 >= 0) != (r2 >= 0)) {
			const int64_t rid = r1 >= 0 ? r1 : r2;
			if ((uint64_t)rid >= n) want_totals[DEDUP_T_INVALID]++;
			else if (B.discarded[rid]) want_totals[DEDUP_T_DISCARD]++;
			else if (first_x(B.reads[rid]) < need) want_totals[DEDUP_T_SHORT]++;
			else { key = key_bytes(packed(B.reads[rid].substr(so, win))); ok = true; }
		} else want_totals[DEDUP_T_UNPAIRED]++;
		records++;
		bool bad = cand[i] != (ok ? 1u : 0u) || flip[i] != (fl ? 1 : 0);
		if (ok) for (uint32_t w = 0; w < W; w++) bad = bad || keys[(size_t)w * np + i] != key_word(key, w);
		else for (uint32_t w = 0; w < W; w++) bad = bad || keys[(size_t)w * np + i] != 0xa5a5a5a5a5a5a5a5ull;      /* a skipped record writes no key */
		if (paired && mode2 && i >= first_chosen && i < first_chosen + chosen.size() && ok) bad = bad || (int)flip[i] != expect_flip[i - first_chosen];
		if (bad) { wrong++; printf("WRONG L=%u so=%u mode=%d paired=%d record %llu: cand %u flip %u\n", L, so, mode2 ? 2 : 1, (int)paired, (unsigned long long)i, cand[i], (unsigned)flip[i]); }
	}
	for (int t = 0; t < 4; t++) if (totals[t] != want_totals[t]) { wrong++; printf("WRONG L=%u so=%u mode=%d paired=%d: counter %d is %llu, not %llu\n", L, so, mode2 ? 2 : 1, (int)paired, t, (unsigned long long)totals[t], (unsigned long long)want_totals[t]); }
	if (!(want_totals[0] && want_totals[1] && want_totals[2] && want_totals[3])) { wrong++; printf("WRONG L=%u so=%u paired=%d: a skip counter stayed 0\n", L, so, (int)paired); }
}

int main() {
	static const uint32_t OFFSETS[] = {0, 4, 60, 64};
	for (uint32_t L = 4; L <= 64; L += 4) {
		const int before = wrong;
		for (uint32_t so : OFFSETS) for (int mode = 1; mode <= 2; mode++) for (int paired = 1; paired >= 0; paired--) run(L, so, mode == 2, paired == 1);
		printf("dedup_length %u%s\n", L, wrong == before ? " ok" : " WRONG");
	}
	/* what the batches reached: both outcomes of the canonical choice, ties decided behind the first word, palindromes */
	if (n_flipped < 1000 || n_forward < 1000 || n_ties_decided_late < 50 || n_palindromes < 60) { wrong++; printf("WRONG reach: %lld flipped, %lld forward, %lld late ties, %lld palindromes\n", n_flipped, n_forward, n_ties_decided_late, n_palindromes); }
	printf("%lld records, %d wrong\n", records, wrong);
	return wrong ? 1 : 0;
}
