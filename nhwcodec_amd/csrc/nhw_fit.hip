/*
 * nhw_fit.hip -- the device side of the byte-budget search (nhw_enc_fit_batch_device, include/nhw_hip.h) and of the distortion search
 * (nhw_enc_fit_sse_batch_device, the same walk with a decode and an error pass per rung): gfx950 only.
 *
 * The search walks a ladder of qualities from the top.  At every rung the images that are still open are encoded at that rung's quality
 * as an ordinary batch (nhw_enc_fit.hip); the three kernels here move the images and files between the caller's per-image slots and the
 * compacted sub-batch the encoder works on:
 *
 *   k_fit_gather   staging[j] = d_bgr[idx[j]]: the open images, 786 432 bytes each, in list order (rungs 2 and later)
 *   k_fit_select   one workgroup per open image: does the rung's file fit the image's budget?  A closed image (or any image on the last
 *                  rung) gets its file, size, status and quality in the caller's slot i = idx[j]; an open one a flag.  The budget is a
 *                  template criterion: FitBytes (the file's size) or FitSse (the decoded picture's SSE, also written to the caller's slot)
 *   k_fit_compact  one workgroup: the flags -> the next open list, in ascending original order, and its length (a scan, not an atomic
 *                  append, so a rung's membership does not depend on the order the workgroups ran in)
 */
#include "nhw_host.h"

#define FIT_IMG_V4   (NHW_IMG_BYTES / 16u)    /* 49 152 sixteen-byte words an image */
#define FIT_GATHER_T 256
#define FIT_GATHER_U 4                        /* words a thread has in flight */
#define FIT_GATHER_X (FIT_IMG_V4 / (FIT_GATHER_T * FIT_GATHER_U))   /* 48 workgroups an image */
static_assert(FIT_GATHER_X * FIT_GATHER_T * FIT_GATHER_U == FIT_IMG_V4, "an image is a whole number of gather workgroups");

/* grid (FIT_GATHER_X, m): workgroup (x, j) copies words [x * 1024, x * 1024 + 1024) of image idx[j] into staging slot j; the four loads of a
 * thread go out together, then the four stores */
__global__ __launch_bounds__(FIT_GATHER_T) void k_fit_gather(const uint4 *__restrict__ src, const int *__restrict__ idx, uint4 *__restrict__ dst)
{
	const int j = blockIdx.y;
	const uint4 *s = src + (size_t)idx[j] * FIT_IMG_V4 + blockIdx.x * (FIT_GATHER_T * FIT_GATHER_U) + threadIdx.x;
	uint4 *d = dst + (size_t)j * FIT_IMG_V4 + blockIdx.x * (FIT_GATHER_T * FIT_GATHER_U) + threadIdx.x;
	uint4 v[FIT_GATHER_U];
#pragma unroll
	for (int k = 0; k < FIT_GATHER_U; k++) v[k] = s[k * FIT_GATHER_T];
#pragma unroll
	for (int k = 0; k < FIT_GATHER_U; k++) d[k * FIT_GATHER_T] = v[k];
}

/* The criteria of k_fit_select.  verdict(): NHW_OK if the rung's file of list entry j (image i) fits, else the status the image gets if
 * this is the last rung.  record(): anything else the criterion writes to the caller's slot of an image that closes. */
struct FitBytes {                /* a file within the image's byte budget */
	const uint32_t *budget;
	__device__ int32_t verdict(int, int i, uint32_t size, int32_t rc) const { return rc != NHW_OK ? rc : size <= budget[i] ? NHW_OK : NHW_E_BUDGET; }
	__device__ void record(int, int, int32_t) const {}
};
struct FitSse {                  /* a decoded picture within the image's SSE budget (rung entry j: its decode status and SSE) */
	const uint64_t *max_sse, *sse;
	const int32_t *dec_status;
	uint64_t *sse_out;
	__device__ int32_t verdict(int j, int i, uint32_t, int32_t rc) const
	{
		return rc != NHW_OK ? rc : dec_status[j] != NHW_OK ? NHW_E_FORMAT : sse[j] <= max_sse[i] ? NHW_OK : NHW_E_BUDGET;
	}
	__device__ void record(int j, int i, int32_t rc) const { sse_out[i] = rc == NHW_OK && dec_status[j] == NHW_OK ? sse[j] : UINT64_MAX; }
};

/* grid m, 256 threads.  idx == nullptr: the first rung, whose sub-batch is the whole batch in order and whose encode wrote the caller's
 * slots itself (nothing to copy: only the quality, and on the last rung the budget status).  Otherwise the rung's files are in staging
 * slot j (st_out / st_sizes / st_status) and a closed image's file is copied to slot idx[j] of the caller's arena.  open[j] = still open. */
template <class Crit>
__global__ __launch_bounds__(256) void k_fit_select(Crit crit, const int *__restrict__ idx, const uint8_t *__restrict__ st_out, const uint32_t *__restrict__ st_sizes,
                                                    const int32_t *__restrict__ st_status, int quality, int last,
                                                    uint8_t *__restrict__ out, uint32_t *__restrict__ sizes, int32_t *__restrict__ status,
                                                    int32_t *__restrict__ qual, uint8_t *__restrict__ open, int out_aligned)
{
	const int j = blockIdx.x;
	const int i = idx ? idx[j] : j;
	const uint32_t size = idx ? st_sizes[j] : sizes[i];
	const int32_t rc = idx ? st_status[j] : status[i];
	const int32_t verdict = crit.verdict(j, i, size, rc);
	const bool fits = verdict == NHW_OK;
	if (!fits && !last) {
		if (threadIdx.x == 0) open[j] = 1;
		return;
	}
	if (threadIdx.x == 0) {
		open[j] = 0;
		sizes[i] = size;
		status[i] = verdict;
		qual[i] = quality;
		crit.record(j, i, rc);
	}
	if (!idx || rc != NHW_OK) return;
	const uint8_t *s = st_out + (size_t)j * NHW_OUT_STRIDE;
	uint8_t *d = out + (size_t)i * NHW_OUT_STRIDE;
	if (out_aligned) {           /* whole 16-byte words: the last one may run up to 15 bytes past the file, still inside the image's slot */
		const uint4 *s4 = reinterpret_cast<const uint4 *>(s);
		uint4 *d4 = reinterpret_cast<uint4 *>(d);
		for (uint32_t w = threadIdx.x; w < (size + 15) / 16; w += 256) d4[w] = s4[w];
	} else
		for (uint32_t b = threadIdx.x; b < size; b += 256) d[b] = s[b];
}

/* one workgroup of 1024 threads: thread t owns flags [t * per, t * per + per); the owners' counts are scanned across the workgroup and every
 * thread writes its open entries at its offset.  next[] = the original indices (idx == nullptr: the first rung, list = 0 .. m-1), *count = total */
__global__ __launch_bounds__(1024) void k_fit_compact(const uint8_t *__restrict__ open, const int *__restrict__ idx, int m, int *__restrict__ next,
                                                      int *__restrict__ count)
{
	__shared__ int wsum[16];
	const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
	const int per = (m + 1023) / 1024;
	const int b = t * per, e = b + per < m ? b + per : m;
	int c = 0;
	for (int j = b; j < e; j++) c += open[j];
	int incl = c;                                      /* inclusive scan across the wavefront */
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const int v = __shfl_up(incl, o);
		if (lane >= o) incl += v;
	}
	if (lane == 63) wsum[wv] = incl;
	__syncthreads();
	int base = 0;
	for (int w = 0; w < wv; w++) base += wsum[w];
	int o = base + incl - c;
	for (int j = b; j < e; j++)
		if (open[j]) next[o++] = idx ? idx[j] : j;
	if (t == 1023) *count = base + incl;
}

void nhw_launch_fit_gather(const uint8_t *d_bgr, const int *idx, int m, uint8_t *staging, hipStream_t s)
{
	k_fit_gather<<<dim3(FIT_GATHER_X, m), FIT_GATHER_T, 0, s>>>(reinterpret_cast<const uint4 *>(d_bgr), idx, reinterpret_cast<uint4 *>(staging));
}

/* one launcher for both criteria: sse == nullptr selects FitBytes (limit: uint32_t budgets), otherwise FitSse (limit: uint64_t targets, with
 * the rung's decode status and SSE per list entry, and the caller's d_sse) */
void nhw_launch_fit_select(const int *idx, int m, const uint8_t *st_out, const uint32_t *st_sizes, const int32_t *st_status, const void *limit,
                           const int32_t *dec_status, const uint64_t *sse, int quality, int last, uint8_t *out, uint32_t *sizes, int32_t *status,
                           int32_t *qual, uint64_t *sse_out, uint8_t *open, hipStream_t s)
{
	const int aligned = ((uintptr_t)out & 15) == 0;     /* the staging arena is hipMalloc'd; the caller's may sit anywhere */
	if (sse)
		k_fit_select<<<m, 256, 0, s>>>(FitSse{ (const uint64_t *)limit, sse, dec_status, sse_out }, idx, st_out, st_sizes, st_status, quality, last, out, sizes,
		                               status, qual, open, aligned);
	else
		k_fit_select<<<m, 256, 0, s>>>(FitBytes{ (const uint32_t *)limit }, idx, st_out, st_sizes, st_status, quality, last, out, sizes, status, qual, open,
		                               aligned);
}

void nhw_launch_fit_compact(const uint8_t *open, const int *idx, int m, int *next, int *count, hipStream_t s)
{
	k_fit_compact<<<1, 1024, 0, s>>>(open, idx, m, next, count);
}
