/*
 * nhw_colour.h -- the colour map of a sample (nhw_colour_map in include/nhw_hip.h), once, for host and device from the same text.
 *
 * A map is a 3 x 3 matrix m and an offset o in 1/65536, in the byte path's order B, G, R.  Of the bytes x a resampler's or the warp's blend has
 * made for a pixel it makes y_i = clamp((m[i][0] x0 + m[i][1] x1 + m[i][2] x2 + o[i] + 32768) >> 16, 0, 255).  Within the limits (each |m| <= 2^20,
 * each |o| <= 2^28) the sum is at most 3 x 255 x 2^20 + 2^28 = 1 070 596 096 in magnitude, so it and its + 32768 fit int32; the shift is arithmetic,
 * floor((t + 32768) / 65536): halves go up at either sign.  The one-channel form reads m[0][0] and o[0] alone.  Nothing here checks a map: the
 * caller has asked nhw_colour_within, and beyond the limits the sum may overflow.
 *
 * No HIP header is needed: without hipcc the qualifiers are empty and the header is plain C++.
 */
#ifndef NHW_COLOUR_H
#define NHW_COLOUR_H

#include <stdint.h>

#include "../../include/nhw_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NHW_COLOUR_FN __host__ __device__ inline
#else
#define NHW_COLOUR_FN inline
#endif

/* all twelve numbers within their bounds and the reserved words 0: what both families ask of a map, the one-channel calls too */
NHW_COLOUR_FN bool nhw_colour_within(const nhw_colour_map &c)
{
	const int32_t G = NHW_COLOUR_MAX_GAIN << 16, O = NHW_COLOUR_MAX_OFFSET << 16;
	bool ok = !(c.reserved[0] | c.reserved[1] | c.reserved[2] | c.reserved[3]);
	for (int i = 0; i < 3; i++) {
		ok = ok && c.o[i] >= -O && c.o[i] <= O;
		for (int j = 0; j < 3; j++) ok = ok && c.m[i][j] >= -G && c.m[i][j] <= G;
	}
	return ok;
}

/* a gain times a byte.  Within the limits both fit 24 signed bits (|m| <= 2^20, x <= 255), so the 24-bit multiply gives the same product: on the
 * device it is spelled out, because it runs at the full rate where the 32-bit one runs at a quarter, and left to itself the compiler takes it in
 * places only; it still does so with this spelling, but in more of them (DESIGN.md section 24 has the counts) */
#if defined(__HIP_DEVICE_COMPILE__)
extern "C" __device__ int __ockl_mul24_i32(int, int);                    /* the device library's 24-bit multiply: what HIP's __mul24 calls */
#endif
NHW_COLOUR_FN int32_t nhw_colour_mul(int32_t m, int32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __ockl_mul24_i32(m, x);
#else
	return m * x;
#endif
}

/* the rule on the C = 3 or 1 bytes of a pixel (each 0 .. 255), in place */
template <int C> NHW_COLOUR_FN void nhw_colour_apply(const nhw_colour_map &c, uint32_t *b)
{
	int32_t y[C];
	for (int i = 0; i < C; i++) {
		int32_t t = c.o[i] + 32768;
		for (int j = 0; j < C; j++) t += nhw_colour_mul(c.m[i][j], (int32_t)b[j]);
		t >>= 16;
		y[i] = t < 0 ? 0 : t > 255 ? 255 : t;
	}
	for (int i = 0; i < C; i++) b[i] = (uint32_t)y[i];
}

#endif
