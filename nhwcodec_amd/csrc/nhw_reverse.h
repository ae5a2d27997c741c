/*
 * nhw_reverse.h -- the mirror of the full-file decode's last store, once, for host and device from the same text.
 *
 * A thread of the decoder's last kernels holds N consecutive pixels of one row of an S x S picture, pixels N c .. N c + N - 1, as B bytes a pixel (3:
 * B, G, R as the byte path stores them; 1: grey) packed into N B / 4 dwords, byte k of the run in bits 8 (k & 3) .. of dword k >> 2.  Mirrored
 * left-right, pixel x of the row goes to column S - 1 - x: the thread's pixels go to columns S - N (c + 1) .. S - N c - 1, its last pixel first.  So a
 * mirrored thread stores the same N pixels in reversed pixel order (nhw_reverse_packed; the bytes of a pixel keep their order) as piece
 * nhw_mirror_piece(S, N, c) = S / N - 1 - c of the row.  S is a multiple of N, so the piece's first column N (S / N - 1 - c) = S - N (c + 1) is a
 * multiple of N as the unmirrored N c is: every store keeps the alignment it has without the mirror.
 *
 * No HIP header is needed: without hipcc the qualifiers are empty and the header is plain C++.
 */
#ifndef NHW_REVERSE_H
#define NHW_REVERSE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NHW_REVERSE_FN __host__ __device__ inline
#else
#define NHW_REVERSE_FN inline
#endif

/* the piece (of N columns) that piece c of a row of S columns becomes under the mirror; its first column is N times this */
NHW_REVERSE_FN int nhw_mirror_piece(int S, int N, int c) { return S / N - 1 - c; }

/* N pixels of B bytes in w[0 .. N B / 4) -> the same pixels, last first, in v[0 .. N B / 4).  Every index is known when compiling: unrolled, this is
 * byte picks between registers (v_perm_b32 / v_alignbyte where the compiler finds them), no memory.  w and v must not overlap. */
template <int N, int B> NHW_REVERSE_FN void nhw_reverse_packed(const uint32_t *w, uint32_t *v)
{
	static_assert((N * B) % 4 == 0 && (B == 1 || B == 3), "whole dwords of one- or three-byte pixels");
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
	for (int k = 0; k < N * B / 4; k++) {
		uint32_t d = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
		for (int j = 0; j < 4; j++) {
			const int dst = 4 * k + j, px = dst / B, ch = dst % B, src = B * (N - 1 - px) + ch;
			d |= ((w[src >> 2] >> (8 * (src & 3))) & 0xFFu) << (8 * j);
		}
		v[k] = d;
	}
}

#endif
