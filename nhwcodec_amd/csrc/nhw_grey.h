/*
 * nhw_grey.h -- the grey rule, once, for host and device from the same text.
 *
 * The grey byte of a luma byte y under quality q is what the file's own colour matrix (write_image_bmp, nhw_decoder_cli.c:135-286;
 * yuv_to_bytes in nhw_dec.hip) gives at neutral chroma, U = V = 128.  There the chroma terms of all four branches vanish -- 1.402 * 0 and its
 * sisters are +0.0, and the integer branch's three constants all come to -4768 -- so R = G = B: one value, a table of 256 entries a quality.
 * It is the identity from quality 20 on and a monotone gain curve below.  The widths are the reference's: a float product where it has one, a
 * double sum where a double constant widened it; the library builds with -ffp-contract=off, so product and sum stay two roundings.
 *
 * No HIP header is needed: without hipcc the qualifiers are empty and the header is plain C++.
 */
#ifndef NHW_GREY_H
#define NHW_GREY_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NHW_GREY_FN __host__ __device__ inline
#else
#define NHW_GREY_FN inline
#endif

/* G_q[y]: quality 1 .. 23, y 0 .. 255 (neither is checked here) */
NHW_GREY_FN int nhw_grey_value(int q, int y)
{
	int g;
	if (q >= 20) return y;                                             /* (int)(Y + 1.402 * 0 + 0.5f) */
	if (q >= 18) {
		const float yinv = q == 19 ? 1.025641f : 1.075269f;
		const float yq = (float)(y * yinv);                             /* a float product */
		g = (int)((double)yq + 0.0 + 0.5f);                             /* the sum in double */
	}
	else if (q == 17) g = (int)(((double)y + 0.0) * 1.063830f + 0.5f);    /* product and sum in double, the factor a float */
	else {
		const float inv_low[17] = { 0.0f, 2.060881f, 1.985939f, 1.916257f, 1.820444f, 1.741126f, 1.665887f, 1.587597f, 1.521263f,
			1.392014f, 1.281502f, 1.190611f, 1.177434f, 1.186945f, 1.138331f, 1.048174f, 1.012139f };   /* index = quality */
		const float p = (float)(y * 298 - 4768) * inv_low[q];           /* 409 * 128 - 57120 = -100 * 128 - 208 * 128 + 34656 = 516 * 128 - 70816 = -4768 */
		g = ((int)(p + 128.5f)) >> 8;                                   /* float sum; the truncation is towards zero, the shift arithmetic */
	}
	return g < 0 ? 0 : g > 255 ? 255 : g;
}

/* ---- the other direction: the encoder's luma of a grey pixel ----
 * L_q[g]: what the encoder's colour conversion (colorspace.c:55-214) gives for the pixel B = G = R = g under quality q.  The chroma of such a
 * pixel is 128 in every branch and behind the 4:2:0 filter, so this table is all a grey encode needs of the colour stage.  Each family is the
 * reference's expression with its own widths: three double products summed left to right, a float quality factor for 18 / 19, the double
 * constant 0.94 for 17, the integer form with the quality table's entry below.  q 1 .. 23, g 0 .. 255 (neither is checked here); the value is
 * not clipped (colorspace.c:80), it lies in 0 .. 255 anyway.  constexpr: the front kernels check their integer form of it when they compile. */
#if defined(__HIPCC__) || defined(__CUDACC__)
#define NHW_GREY_CONSTFN __host__ __device__ constexpr
#else
#define NHW_GREY_CONSTFN constexpr
#endif

NHW_GREY_CONSTFN int nhw_grey_luma(int q, int g)
{
	if (q <= 16) {                                                     /* colorspace.c:172-214: the weights 66 + 129 + 25 on one byte */
		const int qtz[17] = { 0, 15900, 16500, 17100, 18000, 18820, 19670, 20640, 21540, 23540, 25570, 27522, 27830, 27607, 28786, 31262, 32375 };   /* index = quality */
		return (((220 * g) * qtz[q < 1 ? 1 : q] + 4194304) >> 23) + 16;
	}
	const double ly = 0.299 * g + 0.587 * g + 0.114 * g;
	if (q >= 20) return (int)(ly + 0.5f);                              /* the identity (tests/grey_encode/check.cpp) */
	if (q >= 18) return (int)(ly * (q == 19 ? 0.975f : 0.93f) + 0.5f);
	return (int)(ly * 0.94 + 0.5f);
}

/* The same for quality 17 .. 19 without a double: L_q[g] = (g * M + A) >> 16 for every g, M in the low and A in the high half of the word.
 * The pairs were found by search; the half-way cases of 0.94 g (g = 25, 75, 125 round up, 175 and 225 down: the double sum of the three
 * products lies on either side of g) are why 17's M is not 0.94 * 65536.  nhw_front.hip holds them against nhw_grey_luma when it compiles. */
NHW_GREY_CONSTFN uint32_t nhw_grey_luma_fixed(int q)
{
	return q == 19 ? (33560u << 16 | 63894u) : q == 18 ? (33638u << 16 | 60945u) : (33248u << 16 | 61600u);
}

#endif
