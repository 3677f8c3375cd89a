/*
 * nxs_gpu_side.hip -- what the blocking side passes share (nxsgpu_suggest, _complete, _wildcard, _explain,
 * _doc_terms, _related): the stream / workspace / staging / events of a pass (side_t, nxs_gpu_int.h), the host
 * rankers' dictionary (dict_host_t, nxs_side.h) and the block a term-list pass brings back.  Host code only: no
 * kernel lives here, and none of it is on the batch path.
 */
#include "nxs_gpu_int.h"

double
now_ms(void)
{
	struct timespec ts;

	clock_gettime(CLOCK_MONOTONIC, &ts);
	return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

int
side_open(nxsgpu_index_t *ix, side_t *s, const char *what, int n_events, bool own_stream)
{
	if (own_stream && !s->st && hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking) != hipSuccess) {
		s->st = NULL;
		set_error("%s: no stream", what);
		return -1;
	}
	if (ix->profiling && !s->ev_ok) {
		if (n_events > SIDE_EVENTS ||
		    !make_all_or_none(s->ev, n_events, [](hipEvent_t *e) { return hipEventCreate(e) == hipSuccess; },
		    [](hipEvent_t e) { (void)hipEventDestroy(e); })) {
			set_error("%s: no events", what);
			return -1;
		}
		s->n_ev = n_events;
		s->ev_ok = true;
	}
	return 0;
}

int
side_room(side_t *s, const char *what, size_t pin_need, size_t ws_need, bool exact_pin)
{
	if (s->pin_len < pin_need) {
		const size_t len = exact_pin ? pin_need : pin_need + pin_need / 2;

		if (s->pin) {
			(void)hipHostFree(s->pin);
			s->pin = NULL;
			s->pin_len = 0;
		}
		if (hipHostMalloc((void **)&s->pin, len, hipHostMallocDefault) != hipSuccess) {
			s->pin = NULL;
			set_error("hipHostMalloc(%zu) for the %s staging failed", pin_need, what);
			return -1;
		}
		s->pin_len = len;
	}
	if (s->ws_len < ws_need) {
		if (s->ws) {
			(void)hipFree(s->ws);
			s->ws = NULL;
			s->ws_len = 0;
		}
		if (hipMalloc(&s->ws, ws_need) != hipSuccess) {
			s->ws = NULL;
			set_error("hipMalloc(%zu) for the %s workspace failed", ws_need, what);
			return -1;
		}
		s->ws_len = ws_need;
	}
	return 0;
}

double
side_elapsed(const side_t *s, int a, int b)
{
	float ms = 0;

	(void)hipEventElapsedTime(&ms, s->ev[a], s->ev[b]);
	return ms;
}

void
side_close(side_t *s, bool own_stream)
{
	if (s->st) {
		(void)hipStreamSynchronize(s->st);
		if (own_stream) {
			(void)hipStreamDestroy(s->st);
		}
	}
	for (int i = 0; s->ev_ok && i < s->n_ev; i++) {
		(void)hipEventDestroy(s->ev[i]);
	}
	(void)hipFree(s->ws);
	if (s->pin) {
		(void)hipHostFree(s->pin);
	}
	*s = side_t();
}

int
dict_host_build(nxsgpu_index_t *ix, hipStream_t st, dict_host_t *dict, const char *what)
{
	const uint32_t n = ix->n_bk;
	uint64_t blen;

	dict->h_terms.clear();
	dict->h_lens.clear();
	dict->h_dfs.clear();
	dict->h_ids.clear();
	dict->h_nodes.resize(n);
	if (n && (hipMemcpyAsync(dict->h_nodes.data(), ix->d_bk, (size_t)n * sizeof(nxsgpu_bknode_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipStreamSynchronize(st) != hipSuccess)) {
		set_error("%s: reading the BK image back failed", what);
		return -1;
	}
	blen = dict_host_pool_len(*dict);
	dict->h_bytes.resize(blen + 16);
	if (blen && (hipMemcpyAsync(dict->h_bytes.data(), ix->d_bk_bytes, blen, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipStreamSynchronize(st) != hipSuccess)) {
		set_error("%s: reading the BK image back failed", what);
		return -1;
	}
	dict_host_filter(*dict, ix->h_post_off.data(), ix->n_terms);
	return 0;
}

void
tl_copy_out(const uint8_t *h_block, uint32_t n, uint32_t k, uint32_t *term_ids, uint32_t *df, uint32_t *counts,
    uint32_t *matches)
{
	const tl_block_t b = tl_layout((uint8_t *)h_block, n, k);

	memcpy(term_ids, b.ids, (size_t)n * k * 4);
	memcpy(df, b.df, (size_t)n * k * 4);
	memcpy(counts, b.counts, (size_t)n * 4);
	memcpy(matches, b.matches, (size_t)n * 4);
}

int
tl_enter(nxsgpu_index_t *ix, const char *fn, const char *things, uint32_t k, uint32_t k_max, const uint32_t *off,
    uint32_t n, uint32_t *term_ids, uint32_t *df, uint32_t *counts, uint32_t *matches)
{
	if (k < 1 || k > k_max) {
		set_error("%s: k is 1..%u", fn, k_max);
		return -1;
	}
	if (n == 0) {
		return 1;
	}
	if (n > (1u << 24) || off[n] - off[0] > (1u << 30)) {
		set_error("%s: too many %s", fn, things);
		return -1;
	}
	if (hipSetDevice(ix->device) != hipSuccess) {
		set_error("hipSetDevice failed");
		return -1;
	}
	memset(term_ids, 0, (size_t)n * k * 4);
	memset(df, 0, (size_t)n * k * 4);
	memset(counts, 0, (size_t)n * 4);
	memset(matches, 0, (size_t)n * 4);
	return 0;
}
