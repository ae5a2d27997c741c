/* The two rules that make a tone table's row from a histogram: nhw_tone_equalize and nhw_tone_autocontrast of
 * nhwcodec_amd/csrc/nhw_tone.h, and their entries nhw_tone_equalize_at / nhw_tone_autocontrast_at as a kernel calls them, against a
 * straightforward model -- every sum taken again from bin 0 in 128-bit arithmetic, every division with an explicit floor -- on the histograms of
 * the file named by argv[1] (256 counts a line, each below 2^32: tests/tone_cases.HISTS, the crafted ones) and on 400 seeded random ones made here;
 * then nhw_tone_apply on every byte under a table of three different rows.  The header works in uint64 and int32: built with -fsanitize=undefined
 * a signed overflow ends the program.
 * Prints, for every histogram of the file, "eq <512 hex digits>" and "ac <512 hex digits>", the header's rows, for the caller to hold against
 * its own restatement; then "file N", "random N", "mismatches N"; exit status 0 only where the count is 0.
 * Built by tests/test_tone_rule.py with g++ -Wall -Wextra -Werror, once plain and once sanitized. */
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "nhw_tone.h"

typedef unsigned __int128 wide;

static void model_equalize(const uint32_t *h, uint8_t *row)
{
	wide total = 0, last = 0;
	for (int x = 0; x < 256; x++) total += h[x];
	for (int x = 255; x >= 0; x--)
		if (h[x]) { last = h[x]; break; }
	const wide step = (total - last) / 255;
	for (int x = 0; x < 256; x++) {
		if (step == 0) { row[x] = (uint8_t)x; continue; }
		if (x == 0) { row[x] = 0; continue; }
		wide before = 0;
		for (int i = 0; i < x; i++) before += h[i];
		const wide q = (before + step / 2) / step;
		row[x] = (uint8_t)(q > 255 ? 255 : (int)q);
	}
}

static void model_autocontrast(const uint32_t *h, uint8_t *row)
{
	int lo = -1, hi = -1;
	for (int x = 0; x < 256; x++)
		if (h[x]) { if (lo < 0) lo = x; hi = x; }
	for (int x = 0; x < 256; x++) {
		if (lo < 0 || lo >= hi) { row[x] = (uint8_t)x; continue; }
		const int64_t n = 255 * ((int64_t)x - lo), d = hi - lo;
		int64_t q = n / d;
		if (n % d < 0) q--;                                              /* C's division truncates: make it the floor */
		row[x] = (uint8_t)(q < 0 ? 0 : q > 255 ? 255 : q);
	}
}

/* the rows as a kernel makes them: the sums first, then the entries one by one */
static void by_entries(const uint32_t *h, uint8_t *eq, uint8_t *ac)
{
	uint64_t total = 0, last = 0, before = 0;
	uint32_t lo = 256, hi = 0;
	for (uint32_t x = 0; x < 256; x++) {
		total += h[x];
		if (h[x]) { last = h[x]; hi = x; if (lo == 256) lo = x; }
	}
	const uint64_t step = nhw_tone_equalize_step(total, last);
	for (uint32_t x = 0; x < 256; x++) {
		eq[x] = step ? nhw_tone_equalize_at(x, before, step) : (uint8_t)x;
		ac[x] = lo < hi ? nhw_tone_autocontrast_at(x, lo, hi) : (uint8_t)x;
		before += h[x];
	}
}

static int differ(const uint8_t *a, const uint8_t *b)
{
	for (int x = 0; x < 256; x++)
		if (a[x] != b[x]) return 1;
	return 0;
}

static int check(const uint32_t *h, bool print)
{
	uint8_t eq[256], ac[256], meq[256], mac[256], keq[256], kac[256];
	nhw_tone_equalize(h, eq);
	nhw_tone_autocontrast(h, ac);
	model_equalize(h, meq);
	model_autocontrast(h, mac);
	by_entries(h, keq, kac);
	if (print) {
		printf("eq ");
		for (int x = 0; x < 256; x++) printf("%02x", eq[x]);
		printf("\nac ");
		for (int x = 0; x < 256; x++) printf("%02x", ac[x]);
		printf("\n");
	}
	return differ(eq, meq) + differ(ac, mac) + differ(keq, meq) + differ(kac, mac);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng()
{
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return rng_state;
}

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: %s histograms.txt\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "r");
	if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
	int from_file = 0, bad = 0;
	for (;;) {
		uint32_t h[256];
		int got = 0;
		for (; got < 256; got++) {
			unsigned long long v;
			if (fscanf(f, "%llu", &v) != 1) break;
			if (v > 0xFFFFFFFFull) { fprintf(stderr, "a count beyond 2^32 - 1\n"); fclose(f); return 2; }
			h[got] = (uint32_t)v;
		}
		if (got == 0) break;
		if (got != 256) { fprintf(stderr, "a line of %d counts\n", got); fclose(f); return 2; }
		bad += check(h, true);
		from_file++;
	}
	fclose(f);
	const int random = 400;
	for (int k = 0; k < random; k++) {
		uint32_t h[256];
		const int shift = (int)(rng() % 33);                             /* counts of 0 .. 2^32 - 1 down to 0 .. 0 */
		const uint64_t keep = rng() % 5;                                 /* how sparse: every bin, or about one in 2, 4, 8, 16 */
		for (int x = 0; x < 256; x++) h[x] = (rng() & ((1ull << keep) - 1)) ? 0u : (uint32_t)((rng() & 0xFFFFFFFFull) >> shift);
		bad += check(h, false);
	}
	/* the table on a pixel: row i for byte i, and row 0 alone for one channel */
	std::vector<uint8_t> t(768);
	for (int i = 0; i < 768; i++) t[(size_t)i] = (uint8_t)(i * 7 + i / 256 * 13 + 1);
	for (uint32_t v = 0; v < 256; v++) {
		uint32_t b[3] = { v, 255 - v, (v * 5 + 3) & 255 }, g[1] = { v };
		const uint32_t want[3] = { t[b[0]], t[256 + b[1]], t[512 + b[2]] };
		nhw_tone_apply<3>(t.data(), b);
		nhw_tone_apply<1>(t.data(), g);
		bad += (b[0] != want[0]) + (b[1] != want[1]) + (b[2] != want[2]) + (g[0] != t[v]);
	}
	printf("file %d\nrandom %d\nmismatches %d\n", from_file, random, bad);
	return bad ? 1 : 0;
}
