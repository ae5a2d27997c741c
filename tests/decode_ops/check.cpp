/*
 * check.cpp -- the mirror of the full-file decode's last store on the CPU: nhw_reverse_packed and nhw_mirror_piece of
 * nhwcodec_amd/csrc/nhw_reverse.h against the same things written a second way.
 *
 *   the reversal   N pixels of B bytes, all bytes distinct (several fillings), packed little-endian into dwords, reversed by the header, unpacked,
 *                  and compared with a reversal done on the byte array itself: pixel p of the result is pixel N - 1 - p, its B bytes in order.
 *                  N = 4, 8 at 3 bytes a pixel, N = 8, 16 at 1 byte: what the kernels call it with.
 *   the columns    for S = 128, 256, 512 and every N above, every piece c of a row: the mirrored piece's first column is S - N (c + 1), a multiple
 *                  of N inside the row, it holds exactly the mirror images S - 1 - x of the piece's own columns x, last first, and the pieces of a
 *                  row are mirrored onto each other one to one.
 *
 * Prints "reversals <count>", "pieces <count>", "mismatches <count>"; exit status 1 on any mismatch.
 */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nhw_reverse.h"

static long mismatches = 0, reversals = 0, pieces = 0;

template <int N, int B> static void check_reversal(uint32_t seed)
{
	constexpr int BYTES = N * B, K = BYTES / 4;
	uint8_t in[BYTES], want[BYTES], got[BYTES];
	for (int i = 0; i < BYTES; i++) in[i] = (uint8_t)(seed + 5u * (uint32_t)i);       /* 5 is odd: BYTES <= 48 distinct bytes */
	for (int i = 0; i < BYTES; i++)
		for (int j = 0; j < i; j++)
			if (in[i] == in[j]) { printf("the filling repeats a byte\n"); mismatches++; }
	for (int p = 0; p < N; p++) memcpy(want + B * p, in + B * (N - 1 - p), B);        /* the second way: whole pixels moved in memory */
	uint32_t w[K], v[K];
	for (int k = 0; k < K; k++) w[k] = (uint32_t)in[4 * k] | (uint32_t)in[4 * k + 1] << 8 | (uint32_t)in[4 * k + 2] << 16 | (uint32_t)in[4 * k + 3] << 24;
	for (int k = 0; k < K; k++) v[k] = 0xDEADBEEFu;
	nhw_reverse_packed<N, B>(w, v);
	for (int k = 0; k < K; k++)
		for (int j = 0; j < 4; j++) got[4 * k + j] = (uint8_t)(v[k] >> (8 * j));
	reversals++;
	if (memcmp(got, want, BYTES)) {
		mismatches++;
		printf("N %d, B %d, seed %u: the reversal differs\n", N, B, seed);
	}
}

static void check_pieces(int S, int N)
{
	std::vector<int> hit((size_t)(S / N), 0);
	for (int c = 0; c < S / N; c++) {
		const int m = nhw_mirror_piece(S, N, c), first = N * m;
		pieces++;
		bool ok = m >= 0 && m < S / N && first == S - N * (c + 1) && first % N == 0 && first >= 0 && first + N <= S;
		for (int p = 0; ok && p < N; p++) ok = first + p == S - 1 - (N * c + (N - 1 - p));   /* reversed pixel p is the piece's pixel N - 1 - p, at its mirror column */
		if (ok) hit[(size_t)m]++;
		else { mismatches++; printf("S %d, N %d, piece %d: mirrored to piece %d\n", S, N, c, m); }
	}
	for (int c = 0; c < S / N; c++)
		if (hit[(size_t)c] != 1) { mismatches++; printf("S %d, N %d: piece %d is the mirror of %d pieces\n", S, N, c, hit[(size_t)c]); }
}

int main()
{
	for (uint32_t seed = 0; seed < 256; seed += 7) {
		check_reversal<4, 3>(seed);
		check_reversal<8, 3>(seed);
		check_reversal<8, 1>(seed);
		check_reversal<16, 1>(seed);
	}
	for (int S : { 128, 256, 512 })
		for (int N : { 4, 8, 16 }) check_pieces(S, N);
	printf("reversals %ld\npieces %ld\nmismatches %ld\n", reversals, pieces, mismatches);
	return mismatches ? 1 : 0;
}
