/* kmr_image_layout.hpp -- the host-side check of a stored map (KmerMapByKmerArrayPair::store, src/Kmer.h:3143-3159) that
 * kmr_load_image and kmr_merge_image make before any byte of it reaches a kernel: the header, the size against k and the value
 * type, and every bucket's offset and count against the one packed layout store() writes.  Plain C++, no HIP:
 * tests/cpp/image_layout_test.cpp includes it.  The caller's buffer may stand at any address, so every u64 and u32 is read with
 * memcpy; nothing is multiplied by a bucket count that has not been bounded by the length first. */
#ifndef KMR_IMAGE_LAYOUT_HPP_
#define KMR_IMAGE_LAYOUT_HPP_
#include <stdint.h>
#include <string.h>

namespace kmr_host {
struct ImageLayout {
	uint64_t nb, n;           /* buckets and entries, valid when reason == nullptr */
	const char *reason;       /* why the image is refused, nullptr when it is well formed */
};
/* src[0 .. len): {u64 nb, u64 mask, u64 offset[nb]}, then per bucket {u32 count; count keys of kb bytes; count values of vbytes}.
 * Content is not looked at: a key in the wrong bucket or stored twice passes, as it passes the reference's restore() */
inline ImageLayout check_image_layout(const uint8_t *src, uint64_t len, uint32_t kb, uint32_t vbytes) {
	ImageLayout r; r.nb = 0; r.n = 0; r.reason = nullptr;
	if (len < 16) { r.reason = "image too short"; return r; }
	uint64_t nb, mask; memcpy(&nb, src, 8); memcpy(&mask, src + 8, 8);
	/* a bucket costs 12 bytes at least (its offset and its count), so nb <= (len - 16) / 12 before 12 * nb is formed */
	if (nb == 0 || (nb & (nb - 1)) || mask != nb - 1 || nb > (len - 16) / 12) { r.reason = "bad image header"; return r; }
	const uint64_t esz = (uint64_t)kb + vbytes, body = len - 16 - 12 * nb;
	if (esz == 0 || body % esz != 0) { r.reason = "image size does not match k / value type"; return r; }
	uint64_t expect = 8 * (2 + nb);
	for (uint64_t b = 0; b < nb; b++) {
		uint64_t off; memcpy(&off, src + 16 + 8 * b, 8);
		if (off != expect || len - expect < 4) { r.reason = "image offsets are not the packed store() layout"; return r; }
		uint32_t cnt; memcpy(&cnt, src + expect, 4);
		expect += 4;
		if (cnt > (len - expect) / esz) { r.reason = "image bucket runs past the end"; return r; }
		expect += (uint64_t)cnt * esz;
	}
	if (expect != len) { r.reason = "image length mismatch"; return r; }
	r.nb = nb; r.n = body / esz;
	return r;
}
}  // namespace kmr_host
#endif
