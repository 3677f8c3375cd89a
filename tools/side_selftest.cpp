/*
 * side_selftest.cpp -- the host-only logic of the side passes' kit (nxs_side.h) as a stand-alone program: the df
 * filter of the host rankers' dictionary against a brute force over host arrays, and the all-or-nothing creation
 * of a set of handles with a creator that fails at every position.  Meant to be built with the sanitizers, from
 * the header alone (no HIP, no GPU):
 *
 *   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -Iinclude -Inxsearch_amd/csrc tools/side_selftest.cpp -o side_selftest && ./side_selftest
 *
 * Exit status 0 and "side_selftest OK" when every check holds.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>

#include "nxs_side.h"

#define	CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;

static uint64_t
rnd(void)
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return rng_state;
}

/* a dictionary of n nodes over n_terms terms: term ids 0 and beyond n_terms among them, empty and 300-byte strings,
 * lists of length 0; every array exactly as long as it must be (the sanitizer sees a byte too many) */
static void
filter_case(uint32_t n, uint32_t n_terms)
{
	std::unique_ptr<uint64_t[]> post_off(new uint64_t[(size_t)n_terms + 2]);
	dict_host_t d;
	uint64_t pos = 0, pool = 0;

	post_off[0] = 0;
	for (uint32_t t = 1; t <= n_terms + 1; t++) {
		post_off[t] = pos;
		pos += rnd() % 3 == 0 ? 0 : rnd() % 5;		/* a third of the lists are empty */
	}
	d.h_nodes.resize(n);
	for (uint32_t i = 0; i < n; i++) {
		nxsgpu_bknode_t nd;

		memset(&nd, 0, sizeof(nd));
		nd.term_id = rnd() % 8 == 0 ? (uint32_t)(rnd() % 2 ? 0 : n_terms + 1 + rnd() % 3) : 1 + (uint32_t)(rnd() % (n_terms ? n_terms : 1));
		nd.str_len = rnd() % 16 == 0 ? 0 : rnd() % 32 == 0 ? 300 : 1 + (uint32_t)(rnd() % 12);
		nd.str_off = (uint32_t)pool;
		pool += nd.str_len;
		d.h_nodes[i] = nd;
	}
	CHECK(dict_host_pool_len(d) == (n ? pool : 0));
	d.h_bytes.resize(pool);
	for (uint64_t b = 0; b < pool; b++) {
		d.h_bytes[b] = (uint8_t)(1 + rnd() % 255);
	}
	/* stale entries of an earlier build must go */
	d.h_terms.push_back(NULL);
	d.h_lens.push_back(7);
	d.h_dfs.push_back(7);
	d.h_ids.push_back(7);
	dict_host_filter(d, post_off.get(), n_terms);

	size_t j = 0;
	for (uint32_t i = 0; i < n; i++) {
		const nxsgpu_bknode_t &nd = d.h_nodes[i];
		const uint32_t t = nd.term_id;
		const uint64_t df = (t >= 1 && t <= n_terms) ? post_off[t + 1] - post_off[t] : 0;

		CHECK(dict_df(post_off.get(), n_terms, t) == df);
		if (!df) {
			continue;
		}
		CHECK(j < d.h_terms.size());
		CHECK(d.h_terms[j] == d.h_bytes.data() + nd.str_off && d.h_lens[j] == nd.str_len);
		CHECK(d.h_dfs[j] == df && d.h_ids[j] == t);
		/* the term's bytes are readable through the pointer */
		for (uint32_t b = 0; b < d.h_lens[j]; b++) {
			CHECK(d.h_terms[j][b] != 0);
		}
		j++;
	}
	CHECK(j == d.h_terms.size() && j == d.h_lens.size() && j == d.h_dfs.size() && j == d.h_ids.size());
}

/* handles are heap cells: one that is not destroyed leaks, one destroyed twice is a double free -- both are the
 * sanitizer's to report */
static int fail_at, created, live;

static bool
cell_create(int **h)
{
	if (created == fail_at) {
		return false;
	}
	*h = new int(created++);
	live++;
	return true;
}

static void
cell_destroy(int *h)
{
	CHECK(*h == live - 1);		/* reverse order of creation */
	delete h;
	live--;
}

static void
all_or_none_case(int n)
{
	for (fail_at = 0; fail_at <= n; fail_at++) {
		int *h[8] = { NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL };
		CHECK(n <= 8 && live == 0);
		created = 0;
		const bool ok = make_all_or_none(h, n, cell_create, cell_destroy);

		if (fail_at < n) {
			CHECK(!ok && live == 0);		/* none: what was made is gone again */
			continue;
		}
		CHECK(ok && live == n);
		for (int i = n; i-- > 0; ) {
			CHECK(h[i] && *h[i] == i);
			cell_destroy(h[i]);
		}
		CHECK(live == 0);
	}
}

int
main(void)
{
	filter_case(0, 0);
	filter_case(0, 5);
	filter_case(1, 1);
	filter_case(7, 0);
	for (int r = 0; r < 200; r++) {
		filter_case(1 + (uint32_t)(rnd() % 400), 1 + (uint32_t)(rnd() % 300));
	}
	for (int n = 0; n <= 6; n++) {
		all_or_none_case(n);
	}
	printf("side_selftest OK\n");
	return 0;
}
