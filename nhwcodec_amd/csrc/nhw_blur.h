/*
 * nhw_blur.h -- the separable filter of a sample (nhw_blur in include/nhw_hip.h), once, for host and device from the same text.
 *
 * A picture is W x H, C = 3 or 1 bytes a pixel; each channel is filtered on its own; p(y, x) is a byte of the picture.  A record holds 2 rx + 1
 * taps wx and 2 ry + 1 taps wy in 1/32768 (each list sums to 32768), a mix in 1/65536 and a border.  ix(i, n) is the border's index: reflect
 * without repeating the edge, i < 0 -> -i, i >= n -> 2 (n - 1) - i (torch's `reflect` padding); replicate, min(max(i, 0), n - 1).  Four steps:
 *   1. h(y, x) = (sum_{j = 0 .. 2 rx} wx[j] p(y, ix(x + j - rx, W)) + 64) >> 7: 0 .. 65280, eight fractional bits, held as 16 bits;
 *   2. b(y, x) = (sum_{j = 0 .. 2 ry} wy[j] h(ix(y + j - ry, H), x) + 2^22) >> 23: 0 .. 255; the sum is at most 32768 x 65280 = 2 139 095 040 and
 *      with the rounding term 2 143 289 344, below 2^31;
 *   3. z = clamp(p + floor((mix (b - p) + 32768) / 65536), 0, 255): an arithmetic shift of a signed 32-bit value, halves go up at either sign as in
 *      section 24; |mix (b - p)| <= 2^20 x 255 < 2^28;
 *   4. z takes the place of the byte in the pixel's store (nhw_tensor.h).
 * rx = ry = 0 with the one tap 32768 gives b = p and z = p for every mix; mix = 65536 gives z = b; a constant picture stays constant.
 * Nothing here but nhw_blur_within checks a record: the caller has asked it, and beyond it the sums may overflow and an index may leave the picture.
 *
 * No HIP header is needed: without hipcc the qualifiers are empty and the header is plain C++.
 */
#ifndef NHW_BLUR_H
#define NHW_BLUR_H

#include <stdint.h>

#include "../../include/nhw_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NHW_BLUR_FN __host__ __device__ inline
#else
#define NHW_BLUR_FN inline
#endif

/* the predicate: both radii at most 15, both tap lists summing to 32768, |mix| <= 16 x 65536, a border that exists and, under reflect, a radius
 * below the side it runs along.  reserved8 and reserved[] are not read */
NHW_BLUR_FN bool nhw_blur_within(const nhw_blur *f, uint32_t w, uint32_t h)
{
	const uint32_t rx = f->rx, ry = f->ry;
	if (rx > NHW_BLUR_MAX_RADIUS || ry > NHW_BLUR_MAX_RADIUS || f->border > NHW_BLUR_REPLICATE) return false;
	const int32_t M = NHW_BLUR_MAX_MIX * 65536;
	if (f->mix < -M || f->mix > M) return false;
	if (f->border == NHW_BLUR_REFLECT && (rx >= w || ry >= h)) return false;
	uint32_t sx = 0, sy = 0;
	for (uint32_t j = 0; j <= 2 * rx; j++) sx += f->wx[j];
	for (uint32_t j = 0; j <= 2 * ry; j++) sy += f->wy[j];
	return sx == NHW_BLUR_ONE && sy == NHW_BLUR_ONE;
}

/* ix(i, n): i of -r .. n - 1 + r with r <= 15, and r < n under reflect (the predicate) */
NHW_BLUR_FN uint32_t nhw_blur_ix(int32_t i, uint32_t n, uint32_t border)
{
	const int32_t last = (int32_t)n - 1;
	if (border == NHW_BLUR_REFLECT) return (uint32_t)(i < 0 ? -i : i > last ? 2 * last - i : i);
	return (uint32_t)(i < 0 ? 0 : i > last ? last : i);
}

/* the roundings of steps 1 and 2, of the sums in 32 unsigned bits */
NHW_BLUR_FN uint32_t nhw_blur_h(uint32_t sum) { return (sum + 64u) >> 7; }
NHW_BLUR_FN uint32_t nhw_blur_b(uint32_t sum) { return (sum + (1u << 22)) >> 23; }

/* step 3 on a byte p and its blurred byte b */
NHW_BLUR_FN uint32_t nhw_blur_mix(uint32_t p, uint32_t b, int32_t mix)
{
	const int32_t z = (int32_t)p + ((mix * ((int32_t)b - (int32_t)p) + 32768) >> 16);
	return (uint32_t)(z < 0 ? 0 : z > 255 ? 255 : z);
}

/* step 1 at column x of a row of w pixels of c bytes, channel ch; step 2 and 3 on top of it: byte ch of pixel (y, x) of the picture at `pic`, rows
 * `pitch` bytes apart.  What a host that wants a pixel calls; a kernel that walks tiles takes the functions above */
NHW_BLUR_FN uint32_t nhw_blur_h_at(const nhw_blur *f, const uint8_t *row, uint32_t w, uint32_t c, uint32_t x, uint32_t ch)
{
	uint32_t sum = 0;
	for (uint32_t j = 0; j <= 2u * f->rx; j++) sum += (uint32_t)f->wx[j] * row[c * nhw_blur_ix((int32_t)(x + j) - (int32_t)f->rx, w, f->border) + ch];
	return nhw_blur_h(sum);
}
NHW_BLUR_FN uint32_t nhw_blur_at(const nhw_blur *f, const uint8_t *pic, uint64_t pitch, uint32_t w, uint32_t h, uint32_t c, uint32_t y, uint32_t x, uint32_t ch)
{
	uint32_t sum = 0;
	for (uint32_t j = 0; j <= 2u * f->ry; j++)
		sum += (uint32_t)f->wy[j] * nhw_blur_h_at(f, pic + pitch * nhw_blur_ix((int32_t)(y + j) - (int32_t)f->ry, h, f->border), w, c, x, ch);
	return nhw_blur_mix(pic[pitch * y + c * x + ch], nhw_blur_b(sum), f->mix);
}

#endif
