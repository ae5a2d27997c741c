/*
 * nhw_sse.h -- the squared differences of packed bytes, shared by k_sse (nhw_metric.hip) and k_sse_crop (nhw_picture.hip).
 *
 * Per dword of four bytes, sum (a_k - b_k)^2 = udot4(a,a) + udot4(b,b) - 2 udot4(a,b): three v_dot4_u32_u8, exact in 32 bits (at most
 * 4 * 255^2 = 260 100 a dword, 1 040 400 a 16-byte word).
 */
#ifndef NHW_SSE_H
#define NHW_SSE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t sse4(uint32_t a, uint32_t b)
{
	return __builtin_amdgcn_udot4(a, a, 0u, false) + __builtin_amdgcn_udot4(b, b, 0u, false) - 2u * __builtin_amdgcn_udot4(a, b, 0u, false);
}

__device__ __forceinline__ uint32_t sse16(const uint4 &a, const uint4 &b)
{
	return sse4(a.x, b.x) + sse4(a.y, b.y) + sse4(a.z, b.z) + sse4(a.w, b.w);
}

#endif
