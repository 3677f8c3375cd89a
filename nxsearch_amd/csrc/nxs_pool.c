/*
 * nxs_pool.c -- the host worker pool of an nxs_t: the per-query front half of a
 * batch (nxs_plan.c) and the device layer's per-query host work run on it.
 */
#include <stdlib.h>
#include <string.h>
#include <pthread.h>
#include <stdatomic.h>
#include <unistd.h>

#include "nxs_api_int.h"
#include "nxs_hooks.h"

/*
 * The front half of a batch -- lexing, parsing, token sets, dictionary lookups,
 * plan compilation -- is independent per query (query.c:75-115 works on one
 * query_t).  A small persistent pool spreads it over the host cores the process
 * may use; the pool belongs to the nxs_t (one per thread/process in the
 * reference's threading model, docs/c-api.md:5-8) and is created on the first
 * batch that is large enough to pay for a wake-up.
 */
struct nxs_pool {
	pthread_t *	thr;
	unsigned	n_thr;
	pthread_mutex_t	mu;
	pthread_cond_t	cv_work, cv_done;
	uint64_t	gen;		/* run number (under mu) */
	bool		stop;
	bool		waiting;	/* the caller sleeps on cv_done */
	pool_fn_t	fn;
	void *		arg;
	size_t		n, chunk;
	/*
	 * next item to hand out, tagged with the run it belongs to: (gen << 40) | index.
	 * A worker that wakes up late -- after its run has ended, maybe inside the next
	 * one -- draws a ticket of another run and leaves without touching anything:
	 * a run therefore never waits for its slowest sleeper, only for its items (on a
	 * busy host waking 15 threads took 0.3-0.7 ms, twice per batch: the whole front
	 * half of a C3 step is 0.2 ms of work).
	 */
	_Atomic uint64_t next;
	atomic_size_t	done;		/* items of the current run completed */
	atomic_flag	busy;		/* a run is under way (pool_run takes one caller at a time) */
	/*
	 * gen as the workers may read it without the lock: a worker that has just finished a run
	 * polls it for POOL_SPIN_NS before it goes to sleep -- a batch's front half is two runs
	 * (parse, compile) a few dozen microseconds apart, and a pipelined server's next batch is
	 * a millisecond away: the second run finds its workers awake instead of paying the wake-up.
	 */
	_Atomic uint64_t gen_pub;
	long long	spin_ns;	/* NXS_POOL_SPIN_US (120; 0: sleep at once), read when the pool is created */
};
#define	POOL_GEN_SHIFT	40

static void
pool_work(struct nxs_pool *p, uint64_t gen, pool_fn_t fn, void *arg, size_t n, size_t chunk)
{
	for (;;) {
		/* draw a ticket of THIS run only (compare-and-swap: a latecomer of an earlier
		 * run must not take items away from the current one) */
		uint64_t tk = atomic_load(&p->next);
		size_t i;

		for (;;) {
			i = (size_t)(tk & ((1ull << POOL_GEN_SHIFT) - 1));
			if ((tk >> POOL_GEN_SHIFT) != (gen & 0xffffff) || i >= n) {
				return;
			}
			if (atomic_compare_exchange_weak(&p->next, &tk, tk + (uint64_t)chunk)) {
				break;
			}
		}
		const size_t hi = i + chunk < n ? i + chunk : n;
		fn(arg, i, hi);
		if (atomic_fetch_add(&p->done, hi - i) + (hi - i) == n) {
			/* the last items of the run: wake the caller if it went to sleep */
			pthread_mutex_lock(&p->mu);
			if (p->waiting) {
				pthread_cond_signal(&p->cv_done);
			}
			pthread_mutex_unlock(&p->mu);
		}
	}
}

static void *
pool_main(void *arg)
{
	struct nxs_pool *p = arg;
	uint64_t seen = 0;

	pthread_mutex_lock(&p->mu);
	for (;;) {
		if (seen && p->spin_ns && p->gen == seen && !p->stop) {
			struct timespec t0, t1;

			pthread_mutex_unlock(&p->mu);
			clock_gettime(CLOCK_MONOTONIC, &t0);
			while (atomic_load_explicit(&p->gen_pub, memory_order_acquire) == seen) {
				for (int i = 0; i < 64; i++) {
					__builtin_ia32_pause();
				}
				clock_gettime(CLOCK_MONOTONIC, &t1);
				if ((t1.tv_sec - t0.tv_sec) * 1000000000ll + (t1.tv_nsec - t0.tv_nsec) > p->spin_ns) {
					break;
				}
			}
			pthread_mutex_lock(&p->mu);
		}
		while (p->gen == seen && !p->stop) {
			pthread_cond_wait(&p->cv_work, &p->mu);
		}
		if (p->stop) {
			break;
		}
		seen = p->gen;
		/* (the run's description, read under the lock; a stale one is harmless: its
		 * tickets do not match) */
		const pool_fn_t fn = p->fn;
		void *const farg = p->arg;
		const size_t n = p->n, chunk = p->chunk;
		pthread_mutex_unlock(&p->mu);
		pool_work(p, seen, fn, farg, n, chunk);
		pthread_mutex_lock(&p->mu);
	}
	pthread_mutex_unlock(&p->mu);
	return NULL;
}

static struct nxs_pool *
pool_create(unsigned n_thr)
{
	struct nxs_pool *p = calloc(1, sizeof(*p));

	if (!p) {
		return NULL;
	}
	{
		const char *e = getenv("NXS_POOL_SPIN_US");
		const long v = e ? strtol(e, NULL, 10) : 120;
		p->spin_ns = (v < 0 ? 0 : v > 5000 ? 5000 : v) * 1000ll;
	}
	pthread_mutex_init(&p->mu, NULL);
	pthread_cond_init(&p->cv_work, NULL);
	pthread_cond_init(&p->cv_done, NULL);
	p->thr = calloc(n_thr ? n_thr : 1, sizeof(pthread_t));
	for (unsigned i = 0; p->thr && i < n_thr; i++) {
		if (pthread_create(&p->thr[p->n_thr], NULL, pool_main, p) != 0) {
			break;
		}
		p->n_thr++;
	}
	return p;
}

void
pool_destroy(struct nxs_pool *p)
{
	if (!p) {
		return;
	}
	pthread_mutex_lock(&p->mu);
	p->stop = true;
	atomic_store_explicit(&p->gen_pub, ~0ull, memory_order_release);
	pthread_cond_broadcast(&p->cv_work);
	pthread_mutex_unlock(&p->mu);
	for (unsigned i = 0; i < p->n_thr; i++) {
		pthread_join(p->thr[i], NULL);
	}
	pthread_mutex_destroy(&p->mu);
	pthread_cond_destroy(&p->cv_work);
	pthread_cond_destroy(&p->cv_done);
	free(p->thr);
	free(p);
}

/* fn over [0, n) in chunks, on the pool's threads and the caller */
void
pool_run(struct nxs_pool *p, pool_fn_t fn, void *arg, size_t n, size_t chunk)
{
	uint64_t gen;

	/* (one run at a time: a second caller -- there should be none -- works its items itself) */
	if (!p || p->n_thr == 0 || n <= chunk || n >= (1ull << POOL_GEN_SHIFT) ||
	    atomic_flag_test_and_set_explicit(&p->busy, memory_order_acquire)) {
		if (n) {
			fn(arg, 0, n);
		}
		return;
	}
	pthread_mutex_lock(&p->mu);
	p->fn = fn;
	p->arg = arg;
	p->n = n;
	p->chunk = chunk;
	gen = ++p->gen;
	atomic_store(&p->done, 0);
	atomic_store(&p->next, (gen & 0xffffff) << POOL_GEN_SHIFT);
	atomic_store_explicit(&p->gen_pub, gen, memory_order_release);
	pthread_cond_broadcast(&p->cv_work);
	pthread_mutex_unlock(&p->mu);
	pool_work(p, gen, fn, arg, n, chunk);
	/* every item has been handed out; the last ones are still being worked on by
	 * whoever drew them: a short spin, then sleep */
	for (int spin = 0; spin < 4000 && atomic_load(&p->done) < n; spin++) {
		__builtin_ia32_pause();
	}
	if (atomic_load(&p->done) < n) {
		pthread_mutex_lock(&p->mu);
		p->waiting = true;
		while (atomic_load(&p->done) < n) {
			pthread_cond_wait(&p->cv_done, &p->mu);
		}
		p->waiting = false;
		pthread_mutex_unlock(&p->mu);
	}
	atomic_flag_clear_explicit(&p->busy, memory_order_release);
}

#ifdef NXS_TEST_HOOKS	/* (nxs_hooks.h: test hooks and bench accessors are not part of the production ABI) */
/* tests: `rounds` runs of `n` items each on a pool of `n_thr` threads; every item of
 * every run must be worked on exactly once.  Returns the number of items that were not. */
static void
pool_test_fn(void *arg, size_t lo, size_t hi)
{
	_Atomic unsigned char *hits = arg;

	for (size_t i = lo; i < hi; i++) {
		atomic_fetch_add(&hits[i], 1);
	}
}

size_t
nxs_test_pool(unsigned n_thr, size_t n, unsigned rounds, size_t chunk)
{
	struct nxs_pool *p = pool_create(n_thr);
	_Atomic unsigned char *hits = calloc(n ? n : 1, 1);
	size_t bad = 0;

	for (unsigned r = 0; p && hits && r < rounds; r++) {
		memset((void *)hits, 0, n);
		pool_run(p, pool_test_fn, (void *)hits, n, chunk);
		for (size_t i = 0; i < n; i++) {
			bad += hits[i] != 1;
		}
	}
	pool_destroy(p);
	free((void *)hits);
	return (p && hits) ? bad : (size_t)-1;
}

#endif /* NXS_TEST_HOOKS */

/* nxsgpu_parallel_t: the device layer's per-query host work on this nxs_t's pool */
void
api_parallel(void *ctx, nxsgpu_body_t body, void *arg, size_t n, size_t chunk)
{
	pool_run(nxs_pool_get((nxs_t *)ctx), body, arg, n, chunk);
}

/* the pool of an instance: NXS_HOST_THREADS (read once), else min(cores, 16) */
struct nxs_pool *
nxs_pool_get(nxs_t *nxs)
{
	if (!nxs->pool_tried) {
		const char *e = getenv("NXS_HOST_THREADS");
		long n = e ? atol(e) : sysconf(_SC_NPROCESSORS_ONLN);

		nxs->pool_tried = true;
		if (n > 16 && !e) {
			n = 16;
		}
		if (n > 64) {
			n = 64;
		}
		if (n > 1) {
			nxs->pool = pool_create((unsigned)n - 1);	/* the caller works too */
		}
	}
	return nxs->pool;
}
