/*
 * related_selftest.c -- the host logic of nxs_related.h (share, key, predicate, host ranker) against a brute
 * force, as a stand-alone program: meant to be built with the sanitizers, from the header alone.
 *
 *   gcc -std=c11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -Inxsearch_amd/csrc tools/related_selftest.c -o related_selftest -lm && ./related_selftest
 *
 * Exit status 0 and "related_selftest OK" when every check holds.
 */
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nxs_related.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;

static uint64_t
rnd(void)
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return rng_state;
}

#define	CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

/* the definition: does (c1, df1, t1) come before (c2, df2, t2)? */
static bool
before(int order, uint32_t c1, uint32_t df1, uint32_t t1, uint32_t c2, uint32_t df2, uint32_t t2)
{
	if (order == NXS_RT_COUNT) {
		return c1 != c2 ? c1 > c2 : t1 < t2;
	}
	const float s1 = (float)((double)c1 / (double)df1), s2 = (float)((double)c2 / (double)df2);
	return s1 != s2 ? s1 > s2 : t1 < t2;
}

int
main(void)
{
	/* keys: pairs of triples, the special ones first */
	static const uint32_t sp[][3] = { { 2, 4, 9 }, { 3, 6, 5 }, { 1, 2, 70 }, { 5, 5, 1 }, { 1, 1, 2 }, { 1, 4294967295u, 3 },
	    { 4294967295u, 4294967295u, 6 }, { 16777217, 33554434, 13 }, { 16777216, 33554432, 14 }, { 33554431, 33554432, 15 },
	    { 7, 7, 4294967295u } };
	const size_t nsp = sizeof(sp) / sizeof(sp[0]);

	for (int order = 0; order < 2; order++) {
		for (int i = 0; i < 200000; i++) {
			uint32_t a[3], b[3];

			for (int w = 0; w < 2; w++) {
				uint32_t *x = w ? b : a;

				if (rnd() % 4 == 0) {
					memcpy(x, sp[rnd() % nsp], sizeof(a));
				} else {
					x[1] = rnd() % 3 ? (uint32_t)(rnd() % 12) + 1 : (uint32_t)rnd() | 1u;
					x[0] = rnd() % 3 ? (uint32_t)(rnd() % x[1]) + 1 : x[1];
					x[2] = rnd() % 2 ? (uint32_t)(rnd() % 8) + 1 : ((uint32_t)rnd() | 1u);
				}
			}
			const uint64_t ka = nxs_rt_key(order, a[0], a[1], a[2]), kb = nxs_rt_key(order, b[0], b[1], b[2]);

			CHECK(ka != 0 && ka != UINT64_MAX && (uint32_t)ka == a[2]);
			if (a[2] != b[2]) {
				CHECK((ka < kb) == before(order, a[0], a[1], a[2], b[0], b[1], b[2]));
			}
		}
	}
	CHECK(nxs_rt_share(2, 4) == 0.5f && nxs_rt_share(3, 6) == 0.5f && nxs_rt_share(5, 5) == 1.0f);
	CHECK(nxs_rt_share(16777217, 33554434) == nxs_rt_share(16777216, 33554432));

	/* the ranker against a selection sort by the definition */
	for (int trial = 0; trial < 300; trial++) {
		const uint32_t T = (uint32_t)(rnd() % 3 ? rnd() % 70 : rnd() % 700);
		uint32_t *c = calloc((size_t)T + 1, 4), *df = calloc((size_t)T + 1, 4), excl[NXS_RT_EXCL_MAX], out[32], want[32];
		const uint32_t n_excl = (uint32_t)(rnd() % (NXS_RT_EXCL_MAX + 1)), k = (uint32_t)(rnd() % 32) + 1;
		const uint32_t mincount = (uint32_t)(rnd() % 3) + 1, mindf = (uint32_t)(rnd() % 4) + 1;
		const int order = (int)(rnd() % 2);
		uint64_t matches = 77, elig = 0;
		uint8_t *used;

		CHECK(c && df);
		for (uint32_t t = 1; t <= T; t++) {
			df[t] = (uint32_t)(rnd() % 9);
			c[t] = df[t] ? (uint32_t)(rnd() % (df[t] + 1)) : 0;
		}
		for (uint32_t i = 0; i < n_excl; i++) {
			excl[i] = (uint32_t)(rnd() % (T + 2));
		}
		used = calloc((size_t)T + 1, 1);
		CHECK(used);
		for (uint32_t t = 1; t <= T; t++) {
			if (!nxs_rt_eligible(c[t], df[t], mincount, mindf, t, excl, n_excl)) {
				used[t] = 1;
				bool ex = false;
				for (uint32_t i = 0; i < n_excl; i++) {
					ex = ex || excl[i] == t;
				}
				CHECK(c[t] < mincount || df[t] < mindf || ex);
			} else {
				elig++;
			}
		}
		uint32_t nw = 0;
		while (nw < k) {
			uint32_t best = 0;

			for (uint32_t t = 1; t <= T; t++) {
				if (!used[t] && (!best || before(order, c[t], df[t], t, c[best], df[best], best))) {
					best = t;
				}
			}
			if (!best) {
				break;
			}
			used[best] = 1;
			want[nw++] = best;
		}
		const int got = nxs_rt_rank(order, c, df, T, mincount, mindf, excl, n_excl, k, out, &matches);

		CHECK(got == (int)nw && matches == elig);
		CHECK(memcmp(out, want, (size_t)nw * 4) == 0);
		free(used);
		free(c);
		free(df);
	}
	printf("related_selftest OK\n");
	return 0;
}
