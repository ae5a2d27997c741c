/* The grey rule, exhaustively: nhw_grey_value of nhwcodec_amd/csrc/nhw_grey.h against the oracle's colour matrix,
 * nhwo_dec_color of oracle/nhwo_dec.c, at neutral chroma -- every quality 1 .. 23 times every luma byte 0 .. 255.  The oracle's three
 * channels must be equal there, and the rule must be their value.  Prints "mismatches N"; exit status 0 only for N = 0.
 * Built by tests/test_grey_rule.py: this file with g++ -Wall -Wextra -Werror, oracle/nhwo_dec.c with gcc, once plain and once sanitized. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "nhw_grey.h"

extern "C" void nhwo_dec_color(const uint8_t *y, const uint8_t *u, const uint8_t *v, int q, uint8_t *out);   /* oracle/nhwo.h; it walks 512 x 512 pixels */

int main()
{
	const size_t px = 512 * 512;
	std::vector<uint8_t> y(px), uv(px, 128), out(3 * px);
	for (size_t i = 0; i < px; i++) y[i] = (uint8_t)(i & 255);
	int mismatches = 0, unequal = 0, checked = 0;
	for (int q = 1; q <= 23; q++) {
		memset(out.data(), 0x5A, out.size());
		nhwo_dec_color(y.data(), uv.data(), uv.data(), q, out.data());
		for (int b = 0; b < 256; b++) {
			const uint8_t *o = &out[3 * (size_t)b];
			if (o[0] != o[1] || o[1] != o[2]) { unequal++; printf("q%d y%d: the oracle's channels are %d %d %d\n", q, b, o[0], o[1], o[2]); }
			const int g = nhw_grey_value(q, b);
			if (g != o[0]) { mismatches++; printf("q%d y%d: the rule gives %d, the oracle %d\n", q, b, g, o[0]); }
			checked++;
		}
	}
	printf("checked %d\nunequal %d\nmismatches %d\n", checked, unequal, mismatches);
	return mismatches || unequal || checked != 23 * 256;
}
