/*
 * check.cpp -- the encoder's luma of a grey pixel (nhw_grey_luma, nhwcodec_amd/csrc/nhw_grey.h) held against the colour
 * conversion's own expressions (colorspace.c:55-214), written out here a second time with three terms on the pixel (g, g, g), for all 23 x 256
 * inputs; the chroma expressions of the same pixel, which must come to 128; the integer form of quality 17 .. 19 (nhw_grey_luma_fixed) and the
 * identity from quality 20 on.  A stand-alone program: plain C++, no HIP header, built with -ffp-contract=off as the library is.
 */
#include <cstdio>

#include "nhw_grey.h"

static const int k_qtz[17] = { 0, 15900, 16500, 17100, 18000, 18820, 19670, 20640, 21540, 23540, 25570, 27522, 27830, 27607, 28786, 31262, 32375 };

static int clip(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
static int chroma_round(float cb) { return cb >= 0 ? (int)(cb + 128.5f) : (int)(cb + 128.4f); }

/* Y, U, V of the pixel (b0, b1, b2) = (B, G, R) under quality q */
static void convert(int q, int b0, int b1, int b2, int *y, int *u, int *v)
{
	if (q <= 16) {
		const int qz = k_qtz[q];
		*y = (((66 * b0 + 129 * b1 + 25 * b2) * qz + 4194304) >> 23) + 16;
		*u = clip((((-38 * b0 - 74 * b1 + 112 * b2) * qz + 4194304) >> 23) + 128);
		*v = clip((((112 * b0 - 94 * b1 - 18 * b2) * qz + 4194304) >> 23) + 128);
		return;
	}
	const double ly = 0.299 * b0 + 0.587 * b1 + 0.114 * b2;
	const double cb = -0.1687 * b0 - 0.3313 * b1 + 0.5 * b2, cr = 0.5 * b0 - 0.4187 * b1 - 0.0813 * b2;
	if (q >= 20) *y = (int)(ly + 0.5f);
	else if (q >= 18) *y = (int)(ly * (q == 19 ? 0.975f : 0.93f) + 0.5f);
	else *y = (int)(ly * 0.94 + 0.5f);
	if (q == 17) { *u = clip(chroma_round((float)(cb * 0.94))); *v = clip(chroma_round((float)(cr * 0.94))); }
	else { *u = clip(chroma_round((float)cb)); *v = clip(chroma_round((float)cr)); }
}

int main()
{
	int checked = 0, mismatches = 0, chroma = 0, fixed = 0, identity = 0;
	for (int q = 1; q <= 23; q++)
		for (int g = 0; g < 256; g++) {
			int y, u, v;
			convert(q, g, g, g, &y, &u, &v);
			const int got = nhw_grey_luma(q, g);
			checked++;
			if (got != y) { if (mismatches++ < 10) printf("q%d g%d: nhw_grey_luma %d, the three-term expression %d\n", q, g, got, y); }
			if (u != 128 || v != 128) { if (chroma++ < 10) printf("q%d g%d: chroma %d %d\n", q, g, u, v); }
			if (q >= 17 && q <= 19) {
				const uint32_t fx = nhw_grey_luma_fixed(q);
				if ((int)(((uint32_t)g * (fx & 0xFFFFu) + (fx >> 16)) >> 16) != y) fixed++;
			}
			if (q >= 20 && y != g) identity++;
			if (y < 0 || y > 255) mismatches++;
		}
	printf("checked %d\nmismatches %d\nchroma not 128: %d\nfixed form differs: %d\nnot the identity from 20 on: %d\n", checked, mismatches, chroma, fixed, identity);
	return mismatches || chroma || fixed || identity ? 1 : 0;
}
