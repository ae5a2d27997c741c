/*
 * nhw_metric.hip -- the distortion of a batch of pictures against another (nhw_sse_batch_device, include/nhw_hip.h): gfx950 only.
 *
 *   k_sse   grid (SSE_X, n): workgroup (x, i) sums (a - b)^2 over its slice of image i's 786 432 bytes and adds the slice's sum to
 *           sse[i] with one 64-bit integer atomic.  Integer addition is associative, so the result is exact and does not depend on the
 *           order the workgroups ran in.  sse[] is zeroed on the stream first.
 *
 * Per dword of four bytes, sum (a_k - b_k)^2 = udot4(a,a) + udot4(b,b) - 2 udot4(a,b): three v_dot4_u32_u8 (sse4, nhw_sse.h), exact in
 * 32 bits (at most 4 * 255^2 = 260 100 a dword).  A thread's sum over its 48 dwords (at most 12.5 M) and a wavefront's (at most 800 M)
 * stay in 32 bits; the workgroup's four wavefronts are added in 64 bits.
 */
#include "nhw_host.h"
#include "nhw_sse.h"

#define SSE_IMG_V4 (NHW_IMG_BYTES / 16u)     /* 49 152 sixteen-byte words an image */
#define SSE_T      256
#define SSE_U      4                         /* words of each picture a thread has in flight */
#define SSE_R      3                         /* rounds of SSE_U words a thread */
#define SSE_X      (SSE_IMG_V4 / (SSE_T * SSE_U * SSE_R))   /* 16 workgroups an image */
static_assert(SSE_X * SSE_T * SSE_U * SSE_R == SSE_IMG_V4, "an image is a whole number of workgroup slices");

/* workgroup (x, i): words [x * 3072, x * 3072 + 3072) of image i, in three rounds; in a round the eight loads of a thread go out together */
__global__ __launch_bounds__(SSE_T) void k_sse(const uint4 *__restrict__ a, const uint4 *__restrict__ b, unsigned long long *__restrict__ sse)
{
	__shared__ uint32_t wsum[SSE_T / 64];
	const size_t base = (size_t)blockIdx.y * SSE_IMG_V4 + (size_t)blockIdx.x * (SSE_T * SSE_U * SSE_R) + threadIdx.x;
	const uint4 *pa = a + base, *pb = b + base;
	uint32_t acc = 0;
#pragma unroll
	for (int r = 0; r < SSE_R; r++) {
		uint4 va[SSE_U], vb[SSE_U];
#pragma unroll
		for (int k = 0; k < SSE_U; k++) { va[k] = pa[(r * SSE_U + k) * SSE_T]; vb[k] = pb[(r * SSE_U + k) * SSE_T]; }
#pragma unroll
		for (int k = 0; k < SSE_U; k++) acc += sse16(va[k], vb[k]);
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
	if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
	__syncthreads();
	if (threadIdx.x == 0) {
		unsigned long long s = 0;
#pragma unroll
		for (int w = 0; w < SSE_T / 64; w++) s += wsum[w];
		atomicAdd(sse + blockIdx.y, s);
	}
}

/* a, b: n pictures of NHW_IMG_BYTES, 16-byte aligned (the caller checks); sse: n entries */
hipError_t nhw_launch_sse(const uint8_t *a, const uint8_t *b, int n, uint64_t *sse, hipStream_t s)
{
	const hipError_t e = hipMemsetAsync(sse, 0, sizeof(uint64_t) * (size_t)n, s);
	if (e != hipSuccess) return e;
	k_sse<<<dim3(SSE_X, n), SSE_T, 0, s>>>(reinterpret_cast<const uint4 *>(a), reinterpret_cast<const uint4 *>(b), reinterpret_cast<unsigned long long *>(sse));
	return hipGetLastError();
}
