// check_image_layout (kmernator_amd/csrc/kmr_image_layout.hpp) on its own, so that it can run under the host sanitizers
// (-fsanitize=address,undefined): the check kmr_load_image and kmr_merge_image make of a stored map before a kernel sees it.  Every
// malformed image of tests/imagecases.py's list is made here again from a well-formed one by one edit, and handed over twice: from a
// heap block of exactly its length (a read past the end is the sanitizer's to see) and from an odd address (so is a misaligned u64
// or u32 read).  Every case names the reason it expects, or the bucket and entry counts.  Prints one line per case; exit status
// 0 = every expectation held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kmernator_amd/csrc/kmr_image_layout.hpp"

typedef std::vector<uint8_t> Bytes;
static int failures = 0;

static void put64(Bytes &b, size_t at, uint64_t v) { if (b.size() < at + 8) b.resize(at + 8); memcpy(&b[at], &v, 8); }
static void put32(Bytes &b, size_t at, uint32_t v) { if (b.size() < at + 4) b.resize(at + 4); memcpy(&b[at], &v, 4); }
static uint64_t get64(const Bytes &b, size_t at) { uint64_t v; memcpy(&v, &b[at], 8); return v; }

// store() (src/Kmer.h:3143-3159) of buckets with these entry counts; the entries' bytes are a running pattern
static Bytes image(const std::vector<uint32_t> &fills, uint32_t kb, uint32_t vbytes) {
	const uint64_t nb = fills.size();
	Bytes b(8 * (2 + nb), 0);
	put64(b, 0, nb); put64(b, 8, nb - 1);
	for (uint64_t i = 0; i < nb; i++) {
		put64(b, 16 + 8 * i, b.size());
		put32(b, b.size(), fills[i]);
		for (uint64_t j = 0; j < (uint64_t)fills[i] * (kb + vbytes); j++) b.push_back((uint8_t)(j * 7 + i));
	}
	return b;
}

static kmr_host::ImageLayout check_at(const Bytes &img, uint32_t kb, uint32_t vbytes, size_t shift) {
	uint8_t *block = (uint8_t *)malloc(img.size() + shift + (img.empty() && !shift ? 1 : 0));      /* exactly as long as the image */
	if (!img.empty()) memcpy(block + shift, img.data(), img.size());
	const kmr_host::ImageLayout r = kmr_host::check_image_layout(block + shift, img.size(), kb, vbytes);
	free(block);
	return r;
}

static void expect(const char *what, const Bytes &img, uint32_t kb, uint32_t vbytes, const char *reason, uint64_t nb = 0, uint64_t n = 0) {
	bool ok = true;
	for (size_t shift = 0; shift < 2; shift++) {
		const kmr_host::ImageLayout r = check_at(img, kb, vbytes, shift);
		if (reason) ok = ok && r.reason && strstr(r.reason, reason);
		else ok = ok && !r.reason && r.nb == nb && r.n == n;
	}
	std::printf("%-44s kb %-2u vbytes %-2u len %-7zu %-32s %s\n", what, kb, vbytes, img.size(), reason ? reason : "well formed", ok ? "ok" : "WRONG");
	if (!ok) failures++;
}

int main() {
	const std::vector<uint32_t> fills = {0, 1, 2, 63, 64, 65, 128, 255, 256, 257, 600, 0, 3, 66, 191, 0};
	uint64_t total = 0;
	for (uint32_t f : fills) total += f;
	const uint32_t shapes[4][3] = {{4, 12, 1}, {8, 1, 5}, {9, 60, 12}, {32, 5, 1}};      // kb, value bytes, another kind's value bytes: k = 13 weak, 31 singleton, 33 weak with extensions, 127 singleton with extensions
	for (const auto &s : shapes) {
		const uint32_t kb = s[0], vb = s[1], esz = kb + vb;
		const Bytes good = image(fills, kb, vb);
		expect("fills", good, kb, vb, nullptr, 16, total);
		expect("one bucket of 300", image({300}, kb, vb), kb, vb, nullptr, 1, 300);
		expect("one empty bucket", image({0}, kb, vb), kb, vb, nullptr, 1, 0);
		expect("64 empty buckets", image(std::vector<uint32_t>(64, 0), kb, vb), kb, vb, nullptr, 64, 0);
		{ std::vector<uint32_t> sp(4096, 0); sp[1024] = 50; sp[3071] = 50; expect("100 entries in 4096 buckets", image(sp, kb, vb), kb, vb, nullptr, 4096, 100); }

		expect("length 0", Bytes(), kb, vb, "image too short");
		expect("length 15", Bytes(good.begin(), good.begin() + 15), kb, vb, "image too short");
		expect("length 16", Bytes(good.begin(), good.begin() + 16), kb, vb, "bad image header");
		{ Bytes b = good; put64(b, 0, 0); put64(b, 8, ~0ull); expect("nb 0", b, kb, vb, "bad image header"); }
		{ Bytes b = good; put64(b, 0, 3); put64(b, 8, 2); expect("nb 3", b, kb, vb, "bad image header"); }
		for (int sh = 62; sh < 64; sh++) {      // 8 (2 + nb) + 4 nb wraps to 16: the buffer ends where the offsets would begin, or one offset later
			Bytes b; put64(b, 0, 1ull << sh); put64(b, 8, (1ull << sh) - 1);
			expect(sh == 62 ? "nb 2^62, 16 bytes" : "nb 2^63, 16 bytes", b, kb, vb, "bad image header");
			put64(b, 16, 16);
			expect(sh == 62 ? "nb 2^62, 24 bytes" : "nb 2^63, 24 bytes", b, kb, vb, "bad image header");
		}
		{ Bytes b = good; put64(b, 8, 16); expect("mask is not nb - 1", b, kb, vb, "bad image header"); }
		{ Bytes b = good; b.push_back(0); expect("one byte more", b, kb, vb, "image size does not match"); }
		{ Bytes b = good; b.pop_back(); expect("one byte less", b, kb, vb, "image size does not match"); }
		expect("the image of another k", image(fills, kb + 1, vb), kb, vb, "image size does not match");       // 1951 entries, a prime: nothing fits by chance
		expect("the image of another value kind", image(fills, kb, s[2]), kb, vb, "image size does not match");
		{ Bytes b = good; put64(b, 16 + 8 * 7, get64(b, 16 + 8 * 7) + 4); expect("one offset off by 4", b, kb, vb, "not the packed store() layout"); }
		{ Bytes b = good; for (int i = 0; i < 16; i++) put64(b, 16 + 8 * i, get64(good, 16 + 8 * (15 - i))); expect("offsets descending", b, kb, vb, "not the packed store() layout"); }
		{ Bytes b = good; put32(b, (size_t)get64(b, 16 + 8 * 15), 1); expect("last count raised by one", b, kb, vb, "runs past the end"); }
		{ Bytes b = good; put32(b, (size_t)get64(b, 16 + 8 * 15), 0xffffffffu); expect("last count 2^32 - 1", b, kb, vb, "runs past the end"); }
		{ Bytes b = good; put32(b, (size_t)get64(b, 16 + 8 * 10), 601); expect("a middle count raised by one", b, kb, vb, "not the packed store() layout"); }
		{ Bytes b = image({300}, kb, vb); put32(b, 24, 299); expect("only count lowered by one", b, kb, vb, "length mismatch"); }
		{ Bytes b = good; b.resize(b.size() - 4); expect("last count cut off", b, kb, vb, "image size does not match"); }
		if (esz % 4 == 0 && esz <= 20) {      // the size still fits the entries, the walk finds no room for a count
			std::vector<uint32_t> f = fills; for (int i = 11; i < 16; i++) f[i] = 0;
			Bytes b = image(f, kb, vb); b.resize(b.size() - esz);
			expect("last counts cut off by one entry's length", b, kb, vb, "not the packed store() layout");
		}
	}
	return failures ? 1 : 0;
}
