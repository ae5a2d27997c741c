/*
 * nhw_tone.h -- the tone table of a sample (nhw_tone_table in include/nhw_hip.h), once, for host and device from the same text.
 *
 * A table is 256 bytes a channel, rows in the byte path's order B, G, R.  Of the bytes y that the blend, and then the colour map if the call has
 * one, have made for a pixel it makes z_i = t[i][y_i]; the one-channel form reads t[0] alone.  Every table is valid: nothing here or anywhere
 * else checks one.
 *
 * The same header holds the two rules that make a table's row from a histogram h of 256 uint32 counts, whole rows for a host (nhw_tone_equalize,
 * nhw_tone_autocontrast) and their entries (nhw_tone_equalize_at, nhw_tone_autocontrast_at) for a kernel that has the row's sums from a
 * wavefront.  All sums are 64 bits wide: 256 counts of 2^32 - 1 stay below 2^40, and step / 2 added to a running sum cannot wrap.
 *
 * Equalize is PIL's ImageOps.equalize and torchvision's _scale_channel, which agree: total = sum h, last = the count of the highest non-empty
 * bin, step = (total - last) / 255 (integer); step == 0: the identity; else row[0] = 0 and row[x] = min((h[0] + .. + h[x - 1] + step / 2) /
 * step, 255).
 * Autocontrast: lo and hi the lowest and the highest non-empty bin; lo >= hi or an empty histogram: the identity; else row[x] = clamp(floor(255
 * (x - lo) / (hi - lo)), 0, 255), the floor of a signed numerator.  This is torchvision's truncating rule in exact arithmetic: torchvision
 * computes (x - lo) (255 / (hi - lo)) in float32 and may differ by one level where the quotient is an integer that the float rounding misses.
 *
 * No HIP header is needed: without hipcc the qualifiers are empty and the header is plain C++.
 */
#ifndef NHW_TONE_H
#define NHW_TONE_H

#include <stdint.h>

#include "../../include/nhw_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NHW_TONE_FN __host__ __device__ inline
#else
#define NHW_TONE_FN inline
#endif

/* the table on the C = 3 or 1 bytes of a pixel (each 0 .. 255), in place; t: the table's rows, 256 bytes each, wherever they lie */
template <int C> NHW_TONE_FN void nhw_tone_apply(const uint8_t *t, uint32_t *b)
{
	for (int i = 0; i < C; i++) b[i] = t[256 * i + (b[i] & 255u)];
}

/* equalize's step: 0 means "the identity" */
NHW_TONE_FN uint64_t nhw_tone_equalize_step(uint64_t total, uint64_t last) { return (total - last) / 255u; }
/* ... and its entry x under a step above 0, `before` = h[0] + .. + h[x - 1] */
NHW_TONE_FN uint8_t nhw_tone_equalize_at(uint32_t x, uint64_t before, uint64_t step)
{
	if (!x) return 0;
	const uint64_t q = (before + step / 2) / step;
	return (uint8_t)(q < 255u ? q : 255u);
}

/* autocontrast's entry x under lo < hi */
NHW_TONE_FN uint8_t nhw_tone_autocontrast_at(uint32_t x, uint32_t lo, uint32_t hi)
{
	const int32_t num = 255 * ((int32_t)x - (int32_t)lo), den = (int32_t)hi - (int32_t)lo;
	const int32_t q = num >= 0 ? num / den : -((-num + den - 1) / den);   /* the floor at either sign */
	return (uint8_t)(q < 0 ? 0 : q > 255 ? 255 : q);
}

NHW_TONE_FN void nhw_tone_equalize(const uint32_t *h, uint8_t *row)
{
	uint64_t total = 0, last = 0;
	for (int x = 0; x < 256; x++) {
		total += h[x];
		if (h[x]) last = h[x];
	}
	const uint64_t step = nhw_tone_equalize_step(total, last);
	uint64_t before = 0;
	for (int x = 0; x < 256; x++) {
		row[x] = step ? nhw_tone_equalize_at((uint32_t)x, before, step) : (uint8_t)x;
		before += h[x];
	}
}

NHW_TONE_FN void nhw_tone_autocontrast(const uint32_t *h, uint8_t *row)
{
	uint32_t lo = 256, hi = 0;
	for (int x = 0; x < 256; x++)
		if (h[x]) {
			if (lo == 256) lo = (uint32_t)x;
			hi = (uint32_t)x;
		}
	for (int x = 0; x < 256; x++) row[x] = lo < hi ? nhw_tone_autocontrast_at((uint32_t)x, lo, hi) : (uint8_t)x;
}

#endif
