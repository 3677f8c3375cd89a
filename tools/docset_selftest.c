/*
 * docset_selftest.c -- the host logic of nxs_docset.h (sort_unique, the postfix evaluator, the lane) against a brute
 * force, as a stand-alone program: meant to be built with the sanitizers, from the headers alone.  Every array the
 * lane reads is allocated at exactly its size, so a read past a list, a bitmap row or a rank directory is a report.
 *
 *   gcc -std=c11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -Iinclude -Inxsearch_amd/csrc tools/docset_selftest.c -o docset_selftest -lm && ./docset_selftest
 *
 * Exit status 0 and "docset_selftest OK" when every check holds.
 */
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nxs_docset.h"

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

/* ---- sort_unique ------------------------------------------------------------------------------------- */

static void
test_sort_unique(void)
{
	for (int trial = 0; trial < 2000; trial++) {
		const size_t n = (size_t)(rnd() % (trial % 50 ? 70 : 3000));
		uint64_t *a = malloc((n ? n : 1) * 8), *b = malloc((n ? n : 1) * 8);
		const int shape = (int)(rnd() % 4);
		size_t m = 0, got;

		CHECK(a && b);
		for (size_t i = 0; i < n; i++) {
			a[i] = shape == 0 ? rnd() : shape == 1 ? rnd() % 40 : shape == 2 ? (uint64_t)i * 3 + (1ull << 33) * (i & 1) :
			    (i ? a[i - 1] + 1 + rnd() % 5 : rnd() >> 8);		/* 3: ascending and distinct already */
		}
		/* the definition: every value once, by insertion into a sorted array */
		for (size_t i = 0; i < n; i++) {
			size_t at = 0;

			while (at < m && b[at] < a[i]) {
				at++;
			}
			if (at < m && b[at] == a[i]) {
				continue;
			}
			memmove(b + at + 1, b + at, (m - at) * 8);
			b[at] = a[i];
			m++;
		}
		got = nxs_ds_sort_unique(a, n);
		CHECK(got == m && memcmp(a, b, m * 8) == 0);
		free(a);
		free(b);
	}
}

/* ---- the evaluator ----------------------------------------------------------------------------------- */

/* a random expression over tokens 0 .. nt - 1 as a postfix program; its value on every mask by recursion */
typedef struct node { int op; int tok; struct node *l, *r; } node_t;

static node_t *
gen(uint32_t nt, int depth)
{
	node_t *n = calloc(1, sizeof(*n));

	CHECK(n);
	if (depth == 0 || rnd() % 3 == 0) {
		n->op = rnd() % 12 ? 0 : NXSGPU_OP_EMPTY;
		n->tok = (int)(rnd() % nt);
		return n;
	}
	n->op = (int[]){ NXSGPU_OP_AND, NXSGPU_OP_OR, NXSGPU_OP_ANDNOT }[rnd() % 3];
	n->l = gen(nt, depth - 1);
	n->r = gen(nt, depth - 1);
	return n;
}

static uint32_t
emit(const node_t *n, uint8_t *prog, uint32_t at)
{
	if (n->op == 0 || n->op == NXSGPU_OP_EMPTY) {
		prog[at] = n->op ? NXSGPU_OP_EMPTY : (uint8_t)n->tok;
		return at + 1;
	}
	at = emit(n->l, prog, at);
	at = emit(n->r, prog, at);
	prog[at] = (uint8_t)n->op;
	return at + 1;
}

static bool
value(const node_t *n, uint32_t m)
{
	switch (n->op) {
	case 0: return (m >> n->tok) & 1u;
	case NXSGPU_OP_EMPTY: return false;
	case NXSGPU_OP_AND: return value(n->l, m) && value(n->r, m);
	case NXSGPU_OP_OR: return value(n->l, m) || value(n->r, m);
	default: return value(n->l, m) && !value(n->r, m);
	}
}

static void
release(node_t *n)
{
	if (n) {
		release(n->l);
		release(n->r);
		free(n);
	}
}

/* ---- the lane ---------------------------------------------------------------------------------------- */

static void
test_lane(void)
{
	for (int trial = 0; trial < 60; trial++) {
		const uint32_t nt = (uint32_t[]){ 1, 2, 8, 9, 32, 5 }[trial % 6];
		const uint32_t n_docs = (uint32_t)(rnd() % 3 ? 4096 * (1 + rnd() % 3) - rnd() % 100 : 1 + rnd() % 200);
		const uint64_t words = ((uint64_t)n_docs + 4095) / 4096;
		const bool bitmap = trial & 1;
		uint64_t off[NXSGPU_MAX_TOKENS + 1] = { 0 };
		uint8_t *in = calloc((size_t)nt * n_docs, 1);
		nxs_ds_tok_t *toks = malloc(nt * sizeof(*toks));
		uint32_t truth[8] = { 0 };
		uint8_t *prog;
		uint32_t prog_len;
		node_t *ex = gen(nt, nt <= 2 ? 2 : 5);

		CHECK(in && toks);
		for (uint32_t j = 0; j < nt; j++) {
			const uint32_t per = (uint32_t[]){ 2, 7, 50, 997 }[rnd() % 4];
			uint64_t c = 0;

			for (uint32_t d = 0; d < n_docs; d++) {
				in[(size_t)j * n_docs + d] = rnd() % 1000 < per || d == 0 || d == n_docs - 1;
				c += in[(size_t)j * n_docs + d];
			}
			off[j + 1] = off[j] + (rnd() % 9 ? c : 0);	/* now and then a token without postings */
			if (off[j + 1] == off[j]) {
				memset(in + (size_t)j * n_docs, 0, n_docs);
			}
		}
		const uint64_t P = off[nt];
		uint64_t *dt = malloc((P ? P : 1) * 8);
		nxs_ds_post_t *post = malloc((P ? P : 1) * sizeof(*post));
		uint64_t *bm = bitmap ? calloc((size_t)nt * words, 8) : NULL;
		uint32_t *rk = bitmap ? calloc((size_t)nt * (words + 1), 4) : NULL;

		CHECK(dt && post && (!bitmap || (bm && rk)));
		for (uint32_t j = 0; j < nt; j++) {
			uint64_t p = off[j];

			for (uint32_t d = 0; d < n_docs; d++) {
				if (in[(size_t)j * n_docs + d]) {
					dt[p] = (uint64_t)d << 32 | (1 + rnd() % 5);
					post[p].doc = d;
					post[p].imp = rnd() % 6 ? (float)(rnd() % 100000) / 1000.0f : -1.0f;
					p++;
				}
			}
			CHECK(p == off[j + 1]);
			toks[j].beg = off[j];
			toks[j].end = off[j + 1];
			toks[j].row = bitmap ? j : NXS_DS_NONE;
			toks[j].pad = 0;
			for (uint64_t w = 0, i = off[j]; bitmap && w <= words; w++) {
				while (i < off[j + 1] && ((dt[i] >> 32) >> 12) < w) {
					i++;
				}
				rk[(size_t)j * (words + 1) + w] = (uint32_t)(i - off[j]);
			}
			for (uint64_t i = off[j]; bitmap && i < off[j + 1]; i++) {
				const uint32_t d = (uint32_t)(dt[i] >> 32);

				bm[(size_t)j * words + (d >> 12)] |= UINT64_C(1) << ((d >> 6) & 63);
			}
		}
		/* the plan: the truth table up to 8 tokens (from the expression's value), the program always, exact size */
		prog = malloc(NXSGPU_MAX_PROG);
		CHECK(prog);
		prog_len = emit(ex, prog, 0);
		CHECK(prog_len <= NXSGPU_MAX_PROG);
		/* what the evaluator may be handed: this program; not an empty one, not one whose first push is missing */
		CHECK(nxs_ds_prog_ok(prog, prog_len, nt));
		CHECK(!nxs_ds_prog_ok(prog, 0, nt));
		CHECK(prog_len == 1 || !nxs_ds_prog_ok(prog + 1, prog_len - 1, nt));
		prog = realloc(prog, prog_len);
		CHECK(prog);
		for (uint32_t m = 0; nt <= 8 && m < (1u << nt); m++) {
			if (value(ex, m)) {
				truth[m >> 5] |= 1u << (m & 31);
			}
			CHECK(nxs_ds_eval(prog, prog_len, m) == value(ex, m));
		}
		for (int i = 0; nt > 8 && i < 3000; i++) {
			const uint32_t m = (uint32_t)rnd() & (nt == 32 ? 0xffffffffu : (1u << nt) - 1);

			CHECK(nxs_ds_eval(prog, prog_len, m) == value(ex, m));
		}
		for (uint32_t d = 0; d < n_docs; d++) {
			uint32_t m = 0;
			float s = 0.0f, got = -7.0f;
			bool scored = false;

			for (uint32_t j = 0; j < nt; j++) {
				if (in[(size_t)j * n_docs + d]) {
					uint64_t p = off[j];

					while (post[p].doc != d) {
						p++;
					}
					m |= 1u << j;
					if (post[p].imp >= 0.0f) {
						s += post[p].imp;
						scored = true;
					}
				}
			}
			const bool hit = nxs_ds_lane(d, nt, toks, truth, prog, prog_len, dt, post, bm, rk, words, &got);

			CHECK(hit == (scored && value(ex, m)));
			CHECK(!hit || memcmp(&got, &s, 4) == 0);
		}
		release(ex);
		free(in);
		free(toks);
		free(dt);
		free(post);
		free(bm);
		free(rk);
		free(prog);
	}
}

/* ---- the precondition ------------------------------------------------------------------------------ */

static void
test_prog_ok(void)
{
	uint8_t deep[2 * 65];
	const uint8_t beyond[] = { 0, 5, NXSGPU_OP_OR }, unknown[] = { 0, 1, 0x90 }, under[] = { 0, NXSGPU_OP_AND };
	const uint8_t empty_set[] = { NXSGPU_OP_EMPTY, 1, NXSGPU_OP_ANDNOT };

	CHECK(!nxs_ds_prog_ok(beyond, 3, 5) && nxs_ds_prog_ok(beyond, 3, 6));	/* a token >= nt */
	CHECK(!nxs_ds_prog_ok(unknown, 3, 2) && !nxs_ds_prog_ok(under, 2, 1));
	CHECK(nxs_ds_prog_ok(empty_set, 3, 2) && !nxs_ds_eval(empty_set, 3, 3));
	/* 64 values on the stack are evaluated, 65 are refused */
	for (int n = 64; n <= 65; n++) {
		memset(deep, 0, (size_t)n);
		memset(deep + n, NXSGPU_OP_OR, (size_t)n - 1);
		CHECK(nxs_ds_prog_ok(deep, (uint32_t)(2 * n - 1), 1) == (n == 64));
	}
	memset(deep, 0, 64);
	memset(deep + 64, NXSGPU_OP_AND, 63);
	CHECK(nxs_ds_eval(deep, 127, 1) && !nxs_ds_eval(deep, 127, 0));
}

int
main(void)
{
	test_prog_ok();
	test_sort_unique();
	test_lane();
	printf("docset_selftest OK\n");
	return 0;
}
