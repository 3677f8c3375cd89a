/*
 * matchdocs_selftest.c -- the host logic of nxs_matchdocs.h (the cursor's lower bound, the host definition of a page)
 * against a brute force, as a stand-alone program with every array malloc()ed at its exact size: meant to be built
 * with the sanitizers, from the header alone.
 *
 *   gcc -std=c11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -Inxsearch_amd/csrc tools/matchdocs_selftest.c -o matchdocs_selftest && ./matchdocs_selftest
 *
 * Exit status 0 and "matchdocs_selftest OK" when every check holds.
 */
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nxs_matchdocs.h"

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

/* exact-size copies, so that one element too far is the sanitizer's */
static void *
exact(const void *src, size_t bytes)
{
	void *p = malloc(bytes ? bytes : 1);

	CHECK(p);
	if (bytes) {
		memcpy(p, src, bytes);
	}
	return bytes ? p : (free(p), NULL);
}

static uint64_t checks;

/* one (set, cursor, limit) against the definition */
static void
one_page(const uint64_t *doc_ids, const uint8_t *member, uint64_t D, uint64_t from, uint64_t limit)
{
	const uint64_t words = (D + 31) / 32, cap = limit < D ? limit : D;
	uint32_t *bits_full = calloc(words ? words : 1, 4);
	uint64_t *want = malloc((D ? D : 1) * 8);
	uint64_t nw = 0, rest = 0, lb = 0;
	bool more = true;

	CHECK(bits_full && want);
	for (uint64_t d = 0; d < D; d++) {
		if (member[d]) {
			bits_full[d >> 5] |= 1u << (d & 31);
		}
		lb += doc_ids[d] < from;
		if (member[d] && doc_ids[d] >= from) {
			if (nw < limit) {
				want[nw++] = doc_ids[d];
			}
			rest++;
		}
	}
	uint32_t *bits = exact(bits_full, words * 4);
	uint64_t *ids = exact(doc_ids, D * 8);
	uint64_t *out = cap ? malloc(cap * 8) : NULL;

	CHECK(!cap || out);
	CHECK(nxs_md_lower_bound(ids, D, from) == lb);
	const uint64_t n = nxs_md_page(bits, ids, D, from, limit, out, &more);

	CHECK(n == nw && n <= cap);
	CHECK(n == 0 || memcmp(out, want, n * 8) == 0);
	CHECK(more == (rest > nw));
	checks++;
	free(bits_full);
	free(want);
	free(bits);
	free(ids);
	free(out);
}

int
main(void)
{
	static const uint64_t sizes[] = { 0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000 };
	static const unsigned shares[] = { 0, 5, 50, 95, 100 };

	for (size_t si = 0; si < sizeof(sizes) / sizeof(sizes[0]); si++) {
		const uint64_t D = sizes[si];

		for (size_t sh = 0; sh < sizeof(shares) / sizeof(shares[0]); sh++) {
			for (int top = 0; top < 2; top++) {
				uint64_t *doc_ids = malloc((D ? D : 1) * 8);
				uint8_t *member = malloc(D ? D : 1);
				uint64_t id = 0, in = 0;

				CHECK(doc_ids && member);
				for (uint64_t d = 0; d < D; d++) {
					id += 1 + rnd() % 9;
					doc_ids[d] = id;
					member[d] = rnd() % 100 < shares[sh];
					in += member[d];
				}
				if (top && D) {
					doc_ids[D - 1] = UINT64_MAX;	/* the largest id is a doc like any other */
				}
				for (int f = 0; f < 24; f++) {
					uint64_t from;

					switch (f) {
					case 0: from = 0; break;
					case 1: from = UINT64_MAX; break;
					case 2: from = D ? doc_ids[0] : 1; break;
					case 3: from = D ? doc_ids[D - 1] : 2; break;
					case 4: from = D ? doc_ids[D - 1] + 1 : 3; break;	/* (wraps to 0 under `top`: a cursor too) */
					case 5: from = D ? doc_ids[0] - 1 : 4; break;
					default: from = D ? doc_ids[rnd() % D] + rnd() % 3 - 1 : rnd(); break;
					}
					const uint64_t limits[] = { 1, 2, 63, 64, 65, in ? in - 1 : 1, in ? in : 1, in + 1, 1u << 22, 1 + rnd() % (D + 2) };

					for (size_t l = 0; l < sizeof(limits) / sizeof(limits[0]); l++) {
						if (limits[l] >= 1) {
							one_page(doc_ids, member, D, from, limits[l]);
						}
					}
				}
				free(doc_ids);
				free(member);
			}
		}
	}
	printf("matchdocs_selftest OK (%llu pages)\n", (unsigned long long)checks);
	return 0;
}
