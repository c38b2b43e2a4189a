/*
 * kmr_sort.hip -- the one device-wide sort of the library, in a translation unit of its own (rocPRIM's templates take a while to
 * compile): (u64 key, u32 value) pairs by key, stable.  As it is for the correction pass for k-mers seen more than 65 535 times
 * (finalize_superkmer_t: their sightings in stream order, a few pairs per build if any); over a SortBufs for the read stages' sorts;
 * and column by column for elements of several key words (sort_by_columns: duplicate fragments, CompareSpectrums' sorted path,
 * KmerMatch's table, ContigExtender), with where the groups of the sorted elements begin (group_starts).  Contracts: kmr_host.hpp.
 */
#include <rocprim/device/device_radix_sort.hpp>

#include "kmr_host.hpp"

namespace kmr {
/* tmp == nullptr: only the size of the temporary storage is returned in *tmp_bytes */
int sort_pairs_u64_u32(void *tmp, size_t *tmp_bytes, const unsigned long long *keys_in, unsigned long long *keys_out, const unsigned int *vals_in, unsigned int *vals_out,
                       size_t n, hipStream_t stream) {
	return (int)rocprim::radix_sort_pairs(tmp, *tmp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0, 64, stream);
}
}

namespace kmr_host {

/* the keys of one pass: the column's word of the elements in their current order.  Which of row / tags is set is uniform over a launch */
__global__ void sort_column_kernel(SortColumn col, const uint32_t *order, uint64_t n, unsigned long long *kin) {
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t p = order[j];
		kin[j] = col.tags ? (unsigned long long)col.tags[p] : col.words[(uint64_t)(col.row ? col.row[p] : p) * col.stride];
	}
}
__global__ void group_starts_kernel(const uint32_t *head, const uint64_t *hscan, uint64_t n, uint64_t *start) {
	for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x)
		if (head[j]) start[hscan[j]] = j;
	if (blockIdx.x == 0 && threadIdx.x == 0) start[hscan[n]] = n;
}

int sort_reserve(kmr_handle *h, SortBufs &bufs, size_t n, const char *who) {
	size_t bytes = 0;
	if (kmr::sort_pairs_u64_u32(nullptr, &bytes, nullptr, nullptr, nullptr, nullptr, n, h->stream) != 0) return fail(h, KMR_ERR_HIP, std::string(who) + ": radix sort (size query)");
	return bufs.tmp.reserve(h, "sort scratch", std::max<size_t>(bytes, 256));
}
int sort_pairs(kmr_handle *h, SortBufs &bufs, const unsigned long long *kin, unsigned long long *kout, const uint32_t *vin, uint32_t *vout, size_t n, const char *who) {
	size_t bytes = bufs.tmp.cap();
	if (kmr::sort_pairs_u64_u32(bufs.tmp.get(), &bytes, kin, kout, vin, vout, n, h->stream) != 0) return fail(h, KMR_ERR_HIP, std::string(who) + ": radix sort");
	return 0;
}

int sort_by_columns(kmr_handle *h, SortBufs &bufs, const SortColumn *cols, int ncols, uint32_t *order, uint64_t n, const char *who, const uint32_t **sorted, unsigned long long **last_keys) {
	int rc = sort_reserve(h, bufs, n, who); if (rc) return rc;      /* tmp first: it is held whenever any of the four is */
	rc = bufs.perm2.reserve(h, "sort order", 4 * n); if (rc) return rc;
	rc = bufs.kin.reserve(h, "sort keys", 8 * n); if (rc) return rc;
	rc = bufs.kout.reserve(h, "sort keys", 8 * n); if (rc) return rc;
	uint32_t *perm = order, *perm2 = bufs.perm2.get<uint32_t>();
	for (int i = 0; i < ncols; i++) {
		LAUNCH(h, sort_column_kernel, dim3(grid_for(n)), dim3(256), 0, cols[i], (const uint32_t *)perm, n, bufs.kin.get<unsigned long long>());
		rc = sort_pairs(h, bufs, bufs.kin.get<unsigned long long>(), bufs.kout.get<unsigned long long>(), perm, perm2, n, who); if (rc) return rc;
		std::swap(perm, perm2);
	}
	*sorted = perm;
	if (last_keys) *last_keys = bufs.kout.get<unsigned long long>();
	return 0;
}

int group_starts(kmr_handle *h, const uint32_t *head, const uint64_t *hscan, uint64_t n, uint64_t *start) {
	LAUNCH(h, group_starts_kernel, dim3(grid_for(n)), dim3(256), 0, head, hscan, n, start);
	return 0;
}

}  // namespace kmr_host
