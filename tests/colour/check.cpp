/* The colour rule, exhaustively: nhw_colour_apply of nhwcodec_amd/csrc/nhw_colour.h against a model in 64-bit arithmetic
 * with an explicit floor division, on all 2^24 byte triples under every map of the table in the file named by argv[1] (twelve integers a line:
 * m[0][0] .. m[2][2], o[0] .. o[2]; tests/colour_cases.MAPS, at least twelve of them), and the one-channel form on all 256 bytes; then
 * nhw_colour_within at and one beyond every limit, at either sign, and with each reserved word set.  The rule works in int32: built with
 * -fsanitize=undefined a signed overflow ends the program, which is what proves the 32-bit bound at the sign corners.
 * Prints "maps N", "checked N", "mismatches N", "predicate errors N"; exit status 0 only where both counts are 0.
 * Built by tests/test_colour_rule.py with g++ -Wall -Wextra -Werror, once plain and once sanitized. */
#include <stdint.h>
#include <stdio.h>

#include <thread>
#include <vector>

#include "nhw_colour.h"

static int model(const nhw_colour_map &c, int i, const uint32_t *x, int channels)
{
	int64_t t = c.o[i];
	for (int j = 0; j < channels; j++) t += (int64_t)c.m[i][j] * (int64_t)x[j];
	const int64_t n = t + 32768;
	int64_t q = n / 65536;
	if (n % 65536 < 0) q--;                                          /* C's division truncates: make it the floor */
	return q < 0 ? 0 : q > 255 ? 255 : (int)q;
}

static int predicate_errors()
{
	const int32_t G = 1 << 20, O = 1 << 28;
	int bad = 0;
	nhw_colour_map zero = {};
	if (!nhw_colour_within(zero)) bad++;
	for (int k = 0; k < 12; k++)
		for (int sign = -1; sign <= 1; sign += 2)
			for (int beyond = 0; beyond <= 1; beyond++) {
				nhw_colour_map c = {};
				const int32_t v = sign * ((k < 9 ? G : O) + beyond);
				if (k < 9) c.m[k / 3][k % 3] = v; else c.o[k - 9] = v;
				if (nhw_colour_within(c) != !beyond) { bad++; printf("number %d = %d: the predicate says %d\n", k, (int)v, (int)nhw_colour_within(c)); }
			}
	for (int k = 0; k < 4; k++)
		for (uint32_t v : { 1u, 0x80000000u }) {
			nhw_colour_map c = {};
			c.reserved[k] = v;
			if (nhw_colour_within(c)) { bad++; printf("reserved[%d] = %u passes\n", k, (unsigned)v); }
		}
	nhw_colour_map c = {};
	c.m[1][2] = INT32_MIN; c.o[0] = INT32_MAX;
	if (nhw_colour_within(c)) bad++;
	return bad;
}

int main(int argc, char **argv)
{
	std::vector<nhw_colour_map> maps;
	FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
	if (!f) { printf("usage: colour_check <file of maps>\n"); return 2; }
	for (;;) {
		nhw_colour_map c = {};
		int got = 0;
		for (int k = 0; k < 12; k++) got += fscanf(f, "%d", k < 9 ? &c.m[k / 3][k % 3] : &c.o[k - 9]) == 1;
		if (got != 12) break;
		if (!nhw_colour_within(c)) { printf("map %d of the table is beyond the limits\n", (int)maps.size()); return 2; }
		maps.push_back(c);
	}
	fclose(f);
	/* a thread a map, eight at a time: each counts for itself */
	std::vector<long long> done(maps.size(), 0), wrong(maps.size(), 0);
	const auto walk = [&](size_t k) {
		const nhw_colour_map c = maps[k];
		long long n = 0, w = 0;
		for (uint32_t v = 0; v < (1u << 24); v++) {
			const uint32_t x[3] = { v & 255u, (v >> 8) & 255u, v >> 16 };
			uint32_t y[3] = { x[0], x[1], x[2] };
			nhw_colour_apply<3>(c, y);
			const bool bad = (int)y[0] != model(c, 0, x, 3) || (int)y[1] != model(c, 1, x, 3) || (int)y[2] != model(c, 2, x, 3);
			if (bad && w++ < 5) printf("map %d, bytes %u %u %u: the rule gives %u %u %u, the model %d %d %d\n", (int)k, x[0], x[1], x[2], y[0], y[1], y[2],
			                                  model(c, 0, x, 3), model(c, 1, x, 3), model(c, 2, x, 3));
			n++;
		}
		for (uint32_t v = 0; v < 256; v++) {
			uint32_t y[1] = { v };
			nhw_colour_apply<1>(c, y);
			if ((int)y[0] != model(c, 0, &v, 1) && w++ < 5) printf("map %d, byte %u: the one-channel rule gives %u, the model %d\n", (int)k, v, y[0], model(c, 0, &v, 1));
			n++;
		}
		done[k] = n; wrong[k] = w;
	};
	for (size_t k0 = 0; k0 < maps.size(); k0 += 8) {
		std::vector<std::thread> pool;
		for (size_t k = k0; k < maps.size() && k < k0 + 8; k++) pool.emplace_back(walk, k);
		for (std::thread &t : pool) t.join();
	}
	long long checked = 0, mismatches = 0;
	for (size_t k = 0; k < maps.size(); k++) { checked += done[k]; mismatches += wrong[k]; }
	const int pe = predicate_errors();
	printf("maps %d\nchecked %lld\nmismatches %lld\npredicate errors %d\n", (int)maps.size(), checked, mismatches, pe);
	return mismatches || pe || maps.size() < 12;
}
