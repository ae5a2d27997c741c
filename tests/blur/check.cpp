/* The blur rule on crafted pictures: the per-pixel functions of nhwcodec_amd/csrc/nhw_blur.h -- nhw_blur_ix, nhw_blur_h,
 * nhw_blur_b, nhw_blur_mix, and nhw_blur_h_at / nhw_blur_at on top of them -- against a model in 64-bit arithmetic that takes every sum again with
 * an index rule and a floor division of its own, on the cases of the file named by argv[1] (tests/blur_cases.check_text: a line "W H C border rx
 * ry mix", the 2 rx + 1 and the 2 ry + 1 taps, the picture's W H C bytes, and the bytes the numpy model expects), every byte of every picture;
 * then nhw_blur_mix on all 65536 pairs (p, b) under the extreme and the tie-making mixes, the two roundings at their largest sums, and
 * nhw_blur_within at and one step beyond every limit.  The rule works in 32 bits: built with -fsanitize=undefined a signed overflow ends the
 * program, which is what proves the bounds at the extremes.
 * Prints "cases N", "checked N", "mismatches N" (header against the 64-bit model), "file mismatches N" (header against the file's bytes), "mix
 * checked N", "mix mismatches N", "predicate errors N"; exit status 0 only where every error count is 0.
 * Built by tests/test_blur_rule.py with g++ -Wall -Wextra -Werror, once plain and once sanitized. */
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "nhw_blur.h"

static int64_t floor_div(int64_t n, int64_t d)
{
	int64_t q = n / d;
	if (n % d < 0) q--;                                                  /* C's division truncates: make it the floor */
	return q;
}

static int64_t model_ix(int64_t i, int64_t n, int border)
{
	if (border == NHW_BLUR_REFLECT) {
		if (i < 0) i = -i;
		if (i >= n) i = 2 * (n - 1) - i;
		return i;
	}
	return i < 0 ? 0 : i >= n ? n - 1 : i;
}

static int model_mix(int64_t p, int64_t b, int64_t mix)
{
	const int64_t z = p + floor_div(mix * (b - p) + 32768, 65536);
	return z < 0 ? 0 : z > 255 ? 255 : (int)z;
}

static int model(const nhw_blur &f, const std::vector<uint8_t> &pic, int64_t w, int64_t h, int64_t c, int64_t y, int64_t x, int64_t ch)
{
	int64_t sum = 0;
	for (int64_t j = 0; j <= 2 * f.ry; j++) {
		const int64_t yy = model_ix(y + j - f.ry, h, f.border);
		int64_t row = 0;
		for (int64_t i = 0; i <= 2 * f.rx; i++) row += (int64_t)f.wx[i] * pic[(size_t)((yy * w + model_ix(x + i - f.rx, w, f.border)) * c + ch)];
		sum += (int64_t)f.wy[j] * floor_div(row + 64, 128);
	}
	return model_mix(pic[(size_t)((y * w + x) * c + ch)], floor_div(sum + (1ll << 22), 1ll << 23), f.mix);
}

static nhw_blur identity()
{
	nhw_blur f = {};
	f.wx[0] = f.wy[0] = NHW_BLUR_ONE;
	f.mix = 65536;
	return f;
}

static int predicate_errors()
{
	int bad = 0;
	const auto expect = [&](const nhw_blur &f, uint32_t w, uint32_t h, bool want, const char *what) {
		if (nhw_blur_within(&f, w, h) != want) { bad++; printf("predicate: %s: says %d\n", what, (int)!want); }
	};
	nhw_blur f = identity();
	expect(f, 1, 1, true, "the identity on one pixel");
	f.reserved8 = 0xFF; f.reserved[0] = f.reserved[1] = 0xFFFFFFFFu;
	for (int j = 1; j < 32; j++) f.wx[j] = f.wy[j] = 0xFFFF;             /* behind the taps: not read */
	expect(f, 1, 1, true, "reserved fields and the entries behind the taps");
	for (int axis = 0; axis < 2; axis++) {
		for (int r = 15; r <= 16; r++) {
			nhw_blur g = {};
			g.mix = 0; g.border = NHW_BLUR_REPLICATE;
			(axis ? g.wy : g.wx)[2 * r <= 31 ? 2 * r : 31] = NHW_BLUR_ONE;
			(axis ? g.wx : g.wy)[0] = NHW_BLUR_ONE;
			(axis ? g.ry : g.rx) = (uint8_t)r;
			expect(g, 1, 1, r == 15, axis ? "ry of 15 and of 16" : "rx of 15 and of 16");
		}
		for (int d = -1; d <= 1; d++) {
			nhw_blur g = identity();
			(axis ? g.ry : g.rx) = 1; g.border = NHW_BLUR_REPLICATE;
			uint16_t *t = axis ? g.wy : g.wx;
			t[0] = 10000; t[1] = 12768; t[2] = (uint16_t)(10000 + d);
			expect(g, 4, 4, d == 0, axis ? "a wy sum of 32767, 32768, 32769" : "a wx sum of 32767, 32768, 32769");
		}
		for (uint32_t side = 3; side <= 5; side++) {                         /* radius 4 against sides 3, 4, 5 */
			nhw_blur g = identity();
			(axis ? g.ry : g.rx) = 4;
			(axis ? g.wy : g.wx)[0] = 0; (axis ? g.wy : g.wx)[8] = NHW_BLUR_ONE;
			g.border = NHW_BLUR_REFLECT;
			expect(g, axis ? 100 : side, axis ? side : 100, side == 5, "reflect: a radius of the side - 1, the side, the side + 1");
			g.border = NHW_BLUR_REPLICATE;
			expect(g, axis ? 100 : side, axis ? side : 100, true, "replicate: any radius");
		}
	}
	for (int sign = -1; sign <= 1; sign += 2)
		for (int beyond = 0; beyond <= 1; beyond++) {
			nhw_blur g = identity();
			g.mix = sign * (NHW_BLUR_MAX_MIX * 65536 + beyond);
			expect(g, 2, 2, !beyond, "a mix at and one beyond the limit");
		}
	for (int extreme = 0; extreme < 2; extreme++) {
		nhw_blur g = identity();
		g.mix = extreme ? INT32_MIN : INT32_MAX;
		expect(g, 2, 2, false, "a mix at the end of int32");
	}
	for (int border = 1; border <= 3; border++) {
		nhw_blur g = identity();
		g.border = (uint8_t)(border == 3 ? 255 : border);
		expect(g, 2, 2, border == 1, "the borders 1, 2, 255");
	}
	return bad;
}

int main(int argc, char **argv)
{
	FILE *fp = argc > 1 ? fopen(argv[1], "r") : nullptr;
	if (!fp) { printf("usage: blur_check <file of cases>\n"); return 2; }
	long long cases = 0, checked = 0, wrong = 0, file_wrong = 0;
	for (;;) {
		int w, h, c, border, rx, ry, mix;
		if (fscanf(fp, "%d %d %d %d %d %d %d", &w, &h, &c, &border, &rx, &ry, &mix) != 7) break;
		nhw_blur f = {};
		f.rx = (uint8_t)rx; f.ry = (uint8_t)ry; f.border = (uint8_t)border; f.mix = mix;
		if (rx > 15 || ry > 15 || w < 1 || h < 1 || w > 4096 || h > 4096 || (c != 1 && c != 3)) { printf("case %lld: malformed\n", cases); return 2; }
		for (int j = 0; j <= 2 * rx; j++) { unsigned v; if (fscanf(fp, "%u", &v) != 1) return 2; f.wx[j] = (uint16_t)v; }
		for (int j = 0; j <= 2 * ry; j++) { unsigned v; if (fscanf(fp, "%u", &v) != 1) return 2; f.wy[j] = (uint16_t)v; }
		std::vector<uint8_t> pic((size_t)w * h * c), want(pic.size());
		for (uint8_t &b : pic) { unsigned v; if (fscanf(fp, "%u", &v) != 1) return 2; b = (uint8_t)v; }
		for (uint8_t &b : want) { unsigned v; if (fscanf(fp, "%u", &v) != 1) return 2; b = (uint8_t)v; }
		if (!nhw_blur_within(&f, (uint32_t)w, (uint32_t)h)) { printf("case %lld of the file is beyond the limits\n", cases); return 2; }
		for (int y = 0; y < h; y++)
			for (int x = 0; x < w; x++)
				for (int ch = 0; ch < c; ch++) {
					const uint32_t got = nhw_blur_at(&f, pic.data(), (uint64_t)w * c, (uint32_t)w, (uint32_t)h, (uint32_t)c, (uint32_t)y, (uint32_t)x, (uint32_t)ch);
					const int m = model(f, pic, w, h, c, y, x, ch);
					if ((int)got != m && wrong++ < 5) printf("case %lld, pixel (%d, %d) channel %d: the rule gives %u, the model %d\n", cases, y, x, ch, got, m);
					if (got != want[((size_t)y * w + x) * c + ch] && file_wrong++ < 5)
						printf("case %lld, pixel (%d, %d) channel %d: the rule gives %u, the file %u\n", cases, y, x, ch, got, (unsigned)want[((size_t)y * w + x) * c + ch]);
					checked++;
				}
		cases++;
	}
	fclose(fp);
	/* step 3 on every pair of bytes, at the limits of the mix and where the product lands on a half */
	static const int32_t mixes[] = { 0, 1, -1, 32768, -32768, 65536, -65536, 98304, -98304, 16 * 65536, -16 * 65536, 16 * 65536 - 1, -16 * 65536 + 1, 12345, -54321 };
	long long mix_checked = 0, mix_wrong = 0;
	for (const int32_t mix : mixes)
		for (uint32_t p = 0; p < 256; p++)
			for (uint32_t b = 0; b < 256; b++) {
				if ((int)nhw_blur_mix(p, b, mix) != model_mix(p, b, mix) && mix_wrong++ < 5) printf("mix %d on p %u, b %u: the rule gives %u, the model %d\n", (int)mix, p, b, nhw_blur_mix(p, b, mix), model_mix(p, b, mix));
				mix_checked++;
			}
	/* the roundings at their largest sums, and the index at the ends of its range */
	if (nhw_blur_h(32768u * 255u) != 65280u || nhw_blur_b(32768u * 65280u) != 255u || nhw_blur_h(0) != 0 || nhw_blur_b(0) != 0 || nhw_blur_h(63) != 0 || nhw_blur_h(64) != 1 ||
	    nhw_blur_b((1u << 22) - 1) != 0 || nhw_blur_b(1u << 22) != 1) { mix_wrong++; printf("a rounding is off\n"); }
	for (int64_t n = 1; n <= 40; n++)
		for (int border = 0; border <= 1; border++)
			for (int64_t i = -15; i < n + 15; i++) {
				if (border == NHW_BLUR_REFLECT && (i <= -n || i - (n - 1) >= n)) continue;     /* the predicate keeps the radius below the side */
				if ((int64_t)nhw_blur_ix((int32_t)i, (uint32_t)n, (uint32_t)border) != model_ix(i, n, border)) { mix_wrong++; printf("ix(%d, %d) under border %d\n", (int)i, (int)n, border); }
			}
	const int pe = predicate_errors();
	printf("cases %lld\nchecked %lld\nmismatches %lld\nfile mismatches %lld\nmix checked %lld\nmix mismatches %lld\npredicate errors %d\n", cases, checked, wrong, file_wrong,
	       mix_checked, mix_wrong, pe);
	return wrong || file_wrong || mix_wrong || pe || cases < 12;
}
