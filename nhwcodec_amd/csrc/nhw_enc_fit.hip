/*
 * nhw_enc_fit.hip -- encode images to a byte or a distortion budget: the one walk of both quality searches (fit_walk), DESIGN.md
 * sections 9 and 10; its kernels are nhw_fit.hip's and nhw_metric.hip's.  The searches over pictures of any size: nhw_enc_hostpath.hip.
 */
#include "nhw_enc.h"

/* ------------------------------------------------------------------------------------------------ encode to a byte or distortion budget */
/* i * NHW_OUT_STRIDE for i < n */
__global__ void k_fit_doff(uint64_t *off, int n)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) off[i] = (uint64_t)i * NHW_OUT_STRIDE;
}
void fit_doff(uint64_t *d_off, int n, hipStream_t s) { k_fit_doff<<<(n + 255) / 256, 256, 0, s>>>(d_off, n); }

/* the search's buffers for max_batch images on the first fit call, and the distortion search's own (`sse`) on the first SSE-fit call */
static int fit_buffers(nhw_enc *e, bool sse)
{
	if (!e->fit.in) { const int rc = dev_alloc(fit_set(e), "budget search buffers", e->max_batch, nhw_enc_err); if (rc) return rc; }
	if (!sse || e->fit_sse.px) return NHW_OK;
	const int rc = [&]() -> int {
		{ const int rc_ = dev_alloc(fit_sse_set(e), "distortion search buffers", e->max_batch, nhw_enc_err); if (rc_) return rc_; }
		fit_doff(e->fit_sse.doff, e->max_batch, e->own_stream);
		HIPCHK(hipGetLastError());
		HIPCHK(hipStreamSynchronize(e->own_stream));
		return NHW_OK;
	}();
	if (rc != NHW_OK) dev_free(fit_sse_set(e));
	return rc;
}

/* One fit call: the images, the per-image limits in device memory (uint32_t bytes, or with `by_sse` uint64_t SSE scored by a decode of every
 * rung by `dec`), the ladder and the caller's outputs.  fit_check fills in the ladder's qualities and the stream. */
struct FitCall {
	const char *who;                     /* the entry point, for the messages */
	bool by_sse;
	nhw_dec *dec;
	const void *bgr;
	int n;
	const void *limit;
	const int *ladder;
	int ladder_len;
	void *out = nullptr; uint32_t *sizes = nullptr; int32_t *status = nullptr; int32_t *quality = nullptr; uint64_t *sse = nullptr;
	hipStream_t s = nullptr;
	int q[23] = {}, len = 0;
};

/* A search's ladder: ladder_len 0..23, 0 exactly with ladder NULL (NHW_E_ARG); NULL = 23 .. 1 for bytes, 1 .. 23 for SSE (`ascending`);
 * the entries distinct and in 1..23 (NHW_E_QUALITY).  The qualities go to q[0 .. *len). */
int ladder_check(const int *ladder, int ladder_len, bool ascending, int *q, int *len)
{
	if (ladder_len < 0 || ladder_len > 23 || (ladder_len == 0) != (ladder == nullptr)) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	*len = ladder ? ladder_len : 23;
	bool seen[24] = {};
	for (int r = 0; r < *len; r++) {
		q[r] = ladder ? ladder[r] : ascending ? r + 1 : 23 - r;
		if (!nhw_quality_supported(q[r]) || seen[q[r]]) { nhw_enc_err = "ladder: qualities must be distinct and in 1..23"; return NHW_E_QUALITY; }
		seen[q[r]] = true;
	}
	return NHW_OK;
}

/* the SSE searches' decoder: present, max_batch >= need, on e's device, no debug stop (NHW_E_ARG) */
int dec_check(const nhw_enc *e, nhw_dec *d, int need, const std::string &who, const char *need_name)
{
	if (!d) { nhw_enc_err = "bad argument: no decoder handle"; return NHW_E_ARG; }
	int device = 0, max_batch = 0, stop_after = 0;
	nhw_dec_props(d, &device, &max_batch, &stop_after);
	if (max_batch < need) { nhw_enc_err = who + ": the decoder's max_batch is below " + need_name; return NHW_E_ARG; }
	if (device != e->device) { nhw_enc_err = who + ": the decoder is on another device than the encoder"; return NHW_E_ARG; }
	if (stop_after) { nhw_enc_err = who + ": not with a decoder debug stop set (every rung must be a whole decode)"; return NHW_E_ARG; }
	return NHW_OK;
}

/* Everything a fit call refuses before it launches anything, in this order: NULL pointers (`ptrs` false), an unaligned c.bgr (NULL while
 * the host path checks: it uploads into an aligned buffer), n, a debug stop, the ladder (ladder_check), the SSE search's decoder, a
 * capturing stream.  Makes e's device current. */
static int fit_check(nhw_enc *e, FitCall &c, bool ptrs, void *stream)
{
	if (!e || !ptrs) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	const std::string who = c.who;
	if ((uintptr_t)c.bgr & 15) { nhw_enc_err = who + ": d_bgr must be 16-byte aligned"; return NHW_E_ARG; }
	if (c.n < 1 || c.n > e->max_batch) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (e->stop_after) { nhw_enc_err = who + ": not with nhw_debug_stop_after set (every rung must be a whole encode)"; return NHW_E_ARG; }
	{ const int rc = ladder_check(c.ladder, c.ladder_len, c.by_sse, c.q, &c.len); if (rc) return rc; }
	if (c.by_sse) { const int rc = dec_check(e, c.dec, c.n, who, "n"); if (rc) return rc; }
	HIPCHK(hipSetDevice(e->device));
	c.s = stream ? (hipStream_t)stream : e->own_stream;
	hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
	HIPCHK(hipStreamIsCapturing(c.s, &cs));
	if (cs != hipStreamCaptureStatusNone) { nhw_enc_err = who + " waits on the host between rungs and cannot be captured"; return NHW_E_ARG; }
	return NHW_OK;
}

/* The one walk of both searches, down the ladder.  Rung 1 encodes the whole batch straight into the caller's slots (the open list is the
 * identity); every later rung gathers the still-open images from c.bgr (by original index: never from a staging slot, so nothing is copied
 * onto itself) and encodes them as a batch of their own into the staging output.  The SSE search then decodes the rung's files as one batch
 * on the same stream (both arenas hold file j at j * NHW_OUT_STRIDE) and compares the decoded pictures with the rung's input pictures, so
 * list entry j's SSE lines up with its status; an image whose encode failed decodes an empty file (NHW_E_FORMAT) and is not counted as
 * fitting.  k_fit_select copies the files of the images that close into the caller's slots.  Between rungs the open list is compacted on
 * the device and its length waited for on the host. */
static int fit_walk(nhw_enc *e, const FitCall &c)
{
	const hipStream_t s = c.s;
	e->fit_done = false;
	nhw_fit_stats st;
	memset(&st, 0, sizeof st);
	int m = c.n, cur = 0;
	HIPCHK(hipEventRecord(e->fit_ev[0], s));
	for (int r = 0; r < c.len; r++) {
		const bool first = r == 0, last = r == c.len - 1;
		const int *idx = first ? nullptr : e->fit.idx[cur];
		st.quality[r] = c.q[r]; st.images[r] = m; st.rungs = r + 1;
		const uint8_t *pics = first ? (const uint8_t *)c.bgr : e->fit.in;   /* the rung's encode: its pictures and its outputs */
		uint8_t *files = first ? (uint8_t *)c.out : e->fit.out;
		uint32_t *lens = first ? c.sizes : e->fit.sizes;
		int32_t *codes = first ? c.status : e->fit.status;
		if (!first) {
			nhw_launch_fit_gather((const uint8_t *)c.bgr, idx, m, e->fit.in, s);
			HIPCHK(hipGetLastError());
		}
		{ const int rc = nhw_enc_batch_device(e, pics, m, c.q[r], files, lens, codes, s); if (rc) return rc; }
		if (c.by_sse) {
			const int rc = nhw_dec_batch_device(c.dec, files, e->fit_sse.doff, lens, m, e->fit_sse.px, e->fit_sse.dstatus, nullptr, s);
			if (rc) { nhw_enc_err = std::string("decode of a rung: ") + nhw_dec_last_error(); return rc; }
			HIPCHK(nhw_launch_sse(pics, e->fit_sse.px, m, e->fit_sse.sse, s));
		}
		nhw_launch_fit_select(idx, m, e->fit.out, e->fit.sizes, e->fit.status, c.limit, e->fit_sse.dstatus, c.by_sse ? e->fit_sse.sse : nullptr, c.q[r], last,
		                      (uint8_t *)c.out, c.sizes, c.status, c.quality, c.sse, e->fit.open, s);
		HIPCHK(hipGetLastError());
		if (last) break;
		nhw_launch_fit_compact(e->fit.open, idx, m, e->fit.idx[cur ^ 1], e->fit.count, s);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(e->h_fit_count, e->fit.count, sizeof(int), hipMemcpyDeviceToHost, s));
		HIPCHK(hipStreamSynchronize(s));
		m = *e->h_fit_count;
		cur ^= 1;
		if (m == 0) break;
	}
	HIPCHK(hipEventRecord(e->fit_ev[1], s));
	e->fit_stats = st;
	e->fit_done = true;
	return NHW_OK;
}

/* the device entry points: check, allocate, walk */
static int fit_device(nhw_enc *e, FitCall &c, bool ptrs, void *stream)
{
	int rc = fit_check(e, c, ptrs, stream);
	if (rc == NHW_OK) rc = fit_buffers(e, c.by_sse);
	return rc != NHW_OK ? rc : fit_walk(e, c);
}

/* the host conveniences: the images and the n limits uploaded, the search on the handle's own stream, the files compacted and brought back
 * as nhw_enc_batch does, then the qualities and (the SSE search) the achieved SSE */
static int fit_host(nhw_enc *e, FitCall &c, bool ptrs, const uint8_t *bgr, const void *limit, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off,
                    int32_t *status, int32_t *quality, uint64_t *sse)
{
	{ const int rc = fit_check(e, c, ptrs, nullptr); if (rc) return rc; }
	{ const int rc = host_buffers(e, c.n); if (rc) return rc; }
	{ const int rc = fit_buffers(e, c.by_sse); if (rc) return rc; }
	void *d_limit = c.by_sse ? (void *)e->fit_sse.maxsse : (void *)e->fit.budget;
	HIPCHK(hipMemcpyAsync(e->d_in, bgr, (size_t)c.n * NHW_IMG_BYTES, hipMemcpyHostToDevice, c.s));
	HIPCHK(hipMemcpyAsync(d_limit, limit, (c.by_sse ? sizeof(uint64_t) : sizeof(uint32_t)) * c.n, hipMemcpyHostToDevice, c.s));
	c.bgr = e->d_in; c.limit = d_limit;
	c.out = e->d_out; c.sizes = e->d_sizes; c.status = e->d_status; c.quality = e->fit.quality; c.sse = e->fit_sse.sse_out;
	{ const int rc = fit_walk(e, c); if (rc) return rc; }
	{ const int rc = host_download(e, c.n, out_arena, arena_cap, out_off, status); if (rc) return rc; }
	HIPCHK(hipMemcpy(quality, e->fit.quality, sizeof(int32_t) * c.n, hipMemcpyDeviceToHost));
	if (c.by_sse) HIPCHK(hipMemcpy(sse, e->fit_sse.sse_out, sizeof(uint64_t) * c.n, hipMemcpyDeviceToHost));
	return NHW_OK;
}

extern "C" int nhw_enc_fit_batch_device(nhw_enc *e, const void *d_bgr, int n, const uint32_t *d_max_bytes, const int *ladder, int ladder_len,
                                        void *d_out, uint32_t *d_sizes, int32_t *d_status, int32_t *d_quality, void *stream)
{
	FitCall c = { "nhw_enc_fit_batch_device", false, nullptr, d_bgr, n, d_max_bytes, ladder, ladder_len, d_out, d_sizes, d_status, d_quality, nullptr };
	return fit_device(e, c, d_bgr && d_max_bytes && d_out && d_sizes && d_status && d_quality, stream);
}

extern "C" int nhw_enc_fit_batch(nhw_enc *e, const uint8_t *bgr, int n, const uint32_t *max_bytes, const int *ladder, int ladder_len,
                                 uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status, int32_t *quality)
{
	FitCall c = { "nhw_enc_fit_batch", false, nullptr, nullptr, n, nullptr, ladder, ladder_len };
	return fit_host(e, c, bgr && max_bytes && out_arena && out_off && status && quality, bgr, max_bytes, out_arena, arena_cap, out_off, status, quality, nullptr);
}

extern "C" int nhw_enc_fit_sse_batch_device(nhw_enc *e, nhw_dec *d, const void *d_bgr, int n, const uint64_t *d_max_sse, const int *ladder, int ladder_len,
                                            void *d_out, uint32_t *d_sizes, int32_t *d_status, int32_t *d_quality, uint64_t *d_sse, void *stream)
{
	FitCall c = { "nhw_enc_fit_sse_batch_device", true, d, d_bgr, n, d_max_sse, ladder, ladder_len, d_out, d_sizes, d_status, d_quality, d_sse };
	return fit_device(e, c, d_bgr && d_max_sse && d_out && d_sizes && d_status && d_quality && d_sse, stream);
}

extern "C" int nhw_enc_fit_sse_batch(nhw_enc *e, nhw_dec *d, const uint8_t *bgr, int n, const uint64_t *max_sse, const int *ladder, int ladder_len,
                                     uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status, int32_t *quality, uint64_t *sse)
{
	FitCall c = { "nhw_enc_fit_sse_batch", true, d, nullptr, n, nullptr, ladder, ladder_len };
	return fit_host(e, c, bgr && max_sse && out_arena && out_off && status && quality && sse, bgr, max_sse, out_arena, arena_cap, out_off, status, quality, sse);
}

extern "C" int nhw_enc_last_fit_stats(nhw_enc *e, nhw_fit_stats *s)
{
	if (!e || !s || !e->fit_done) { nhw_enc_err = "no completed fit call"; return NHW_E_ARG; }
	HIPCHK(hipSetDevice(e->device));
	HIPCHK(hipEventSynchronize(e->fit_ev[1]));
	*s = e->fit_stats;
	HIPCHK(hipEventElapsedTime(&s->total_ms, e->fit_ev[0], e->fit_ev[1]));
	return NHW_OK;
}
