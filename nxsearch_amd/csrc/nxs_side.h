/*
 * nxs_side.h -- the host-only logic of the side passes' kit (nxs_gpu_side.hip), free of HIP so that a
 * stand-alone program can run it over host arrays (tools/side_selftest.cpp): the host rankers' dictionary
 * and its df filter, and the all-or-nothing creation of a set of handles (the kit's profiling events).
 */
#ifndef NXS_SIDE_H
#define NXS_SIDE_H

#include <stdint.h>
#include <vector>

#include "nxs_gpu.h"

/*
 * The host rankers' dictionary (nxs_suggest_rank, nxs_complete_rank, nxs_wild_rank): the BK image copied back
 * (h_nodes, h_bytes) and, in node order, every node with df > 0 -- any length -- as term pointer (into h_bytes),
 * length, df and term id.  dict_host_build (nxs_gpu_side.hip) fills it.
 */
struct dict_host_t {
	std::vector<nxsgpu_bknode_t> h_nodes;
	std::vector<uint8_t> h_bytes;
	std::vector<const uint8_t *> h_terms;
	std::vector<uint32_t> h_lens, h_dfs, h_ids;
};

/* df of term t: the live posting count of the CSR (what nxsgpu_index_df reports); post_off is [n_terms + 2] */
static inline uint32_t
dict_df(const uint64_t *post_off, uint32_t n_terms, uint32_t t)
{
	return (t >= 1 && t <= n_terms) ? (uint32_t)(post_off[(size_t)t + 1] - post_off[t]) : 0;
}

/* bytes of the pool that h_nodes reach */
static inline uint64_t
dict_host_pool_len(const dict_host_t &d)
{
	uint64_t blen = 0;

	for (const nxsgpu_bknode_t &nd : d.h_nodes) {
		const uint64_t end = (uint64_t)nd.str_off + nd.str_len;
		blen = end > blen ? end : blen;
	}
	return blen;
}

/* h_terms / h_lens / h_dfs / h_ids from h_nodes and h_bytes (which must hold dict_host_pool_len bytes and stay put) */
static inline void
dict_host_filter(dict_host_t &d, const uint64_t *post_off, uint32_t n_terms)
{
	d.h_terms.clear();
	d.h_lens.clear();
	d.h_dfs.clear();
	d.h_ids.clear();
	for (const nxsgpu_bknode_t &nd : d.h_nodes) {
		const uint32_t df = dict_df(post_off, n_terms, nd.term_id);

		if (!df) {
			continue;
		}
		d.h_terms.push_back(d.h_bytes.data() + nd.str_off);
		d.h_lens.push_back(nd.str_len);
		d.h_dfs.push_back(df);
		d.h_ids.push_back(nd.term_id);
	}
}

/* h[0 .. n) all made or none: what was made before a failure is destroyed again, in reverse order */
template <typename H, typename C, typename D>
static inline bool
make_all_or_none(H *h, int n, C create, D destroy)
{
	int made = 0;

	while (made < n && create(&h[made])) {
		made++;
	}
	if (made == n) {
		return true;
	}
	while (made--) {
		destroy(h[made]);
	}
	return false;
}

#endif /* NXS_SIDE_H */
