/*
 * nhw_dwt.h -- what the block-resident filterbank kernels share (nhw_front.hip: k_dwt_ana / k_dwt_syn; nhw_tail.hip: k_l2_recon, k_chroma_loops).
 */
#ifndef NHW_DWT_H
#define NHW_DWT_H
#include <hip/hip_runtime.h>
#include <stdint.h>

/* workgroup barrier that orders LDS traffic only: global loads stay in flight across it */
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

/* the 5/3 synthesis on five loaded taps (upfilter53I / III / VI, filters.c:521-572): l0 and ln are low-band cell k and the one behind it, h0, hp and hn high-band
 * cell k, the one before and the one behind it; e / o: samples 2k and 2k + 1, un-normalised in 16 bits as the reference keeps them; the second direction normalises */
__device__ __forceinline__ void syn_taps(int16_t l0, int16_t ln, int16_t h0, int16_t hp, int16_t hn, bool normalise, int *e_out, int *o_out)
{
	int16_t e = (int16_t)(l0 << 3);
	int16_t o = (int16_t)((l0 + ln) << 2);
	e = (int16_t)(e - ((h0 + hp) << 1));
	o = (int16_t)(o + (6 * h0 - hp - hn));
	if (normalise) {
		if (e > 0) e = (int16_t)(e + 32);
		e >>= 6;
		if (o > 0) o = (int16_t)(o + 32);
		o >>= 6;
	}
	*e_out = e; *o_out = o;
}
/* one output pair of the synthesis (wavelet_filterbank.c:305-496): x holds the low band in cells 0 .. S/2-1 and the high band behind it, st apart; a line's
 * ends repeat their own cell */
template <int S>
__device__ __forceinline__ void syn_pair(const int16_t *x, int st, int k, bool normalise, int *e_out, int *o_out)
{
	constexpr int M = S / 2;
	const int16_t *lo = x, *hi = x + M * st;
	const int l0 = lo[k * st], ln = (k + 1 < M) ? lo[(k + 1) * st] : l0;
	const int h0 = hi[k * st], hp = k > 0 ? hi[(k - 1) * st] : hi[0], hn = (k + 1 < M) ? hi[(k + 1) * st] : h0;
	syn_taps(l0, ln, h0, hp, hn, normalise, e_out, o_out);
}

/* rounding of the analysis' second direction (filters.c:88-287) */
__device__ __forceinline__ int rnd_half_away(int v, int shift)
{
	/* v < 0: -((-v + half) >> shift) = ceil((v - half) / 2^shift) = (v + half - 1) >> shift -- no branch either way */
	return (v + (1 << (shift - 1)) + (v >> 31)) >> shift;
}
__device__ __forceinline__ int diffuse(int r)
{
	/* an odd function of r: |r| mod 64 read as a signed 6-bit number, divided by 4 towards zero, with the sign of r */
	const int s = r >> 31, a = (r ^ s) - s;
	const int t = (int)((unsigned)a << 26) >> 26;
	const int d = (t + ((t >> 31) & 3)) >> 2;
	return (d ^ s) - s;
}

/* the 5-tap low-pass numerator and the predicted odd sample of the analysis (filters.c:55-114, 203-287, 346-386), on cells st apart */
template <int S>
__device__ __forceinline__ int tap5s(const int16_t *x, int st, int k)
{
	const int c = 2 * k;
	const int l1 = c >= 1 ? x[(c - 1) * st] : x[st], l2 = c >= 2 ? x[(c - 2) * st] : x[2 * st];
	const int r1 = x[(c + 1) * st], r2 = (c + 2 < S) ? x[(c + 2) * st] : x[(S - 2) * st];
	return 6 * x[c * st] + 2 * (l1 + r1) - (l2 + r2);
}
__device__ __forceinline__ int pair_predict_s(const int16_t *x, int st, int k)
{
	int a = x[2 * k * st] + x[(2 * k + 2) * st];
	if ((k & 1) && (a & 1) && ((x[(2 * k - 2) * st] + x[2 * k * st]) & 1)) a++;
	return x[(2 * k + 1) * st] - (a >> 1);
}

/* packed 16-bit arithmetic: two cells to a dword */
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 as_s(uint32_t x) { return __builtin_bit_cast(s16x2, x); }
__device__ __forceinline__ u16x2 as_us(uint32_t x) { return __builtin_bit_cast(u16x2, x); }
__device__ __forceinline__ uint32_t as_w(s16x2 x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ uint32_t as_w(u16x2 x) { return __builtin_bit_cast(uint32_t, x); }
/* two 16-bit sums in a dword (no carry between the halves) */
__device__ __forceinline__ unsigned pk_add16(unsigned a, unsigned b)
{
	unsigned d;
	asm("v_pk_add_u16 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
	return d;
}

__device__ __forceinline__ uint32_t pk_max_u16x(uint32_t a, uint32_t b) { uint32_t d; asm("v_pk_max_u16 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
/* rnd_half_away and diffuse on both halves of a dword (operands must be the true values: nhw_front_image.h has the input domain) */
__device__ __forceinline__ s16x2 pk_rnd_half_away(s16x2 v, int shift) { return (v + (s16x2)(short)(1 << (shift - 1)) + (v >> 15)) >> shift; }
__device__ __forceinline__ s16x2 pk_diffuse(s16x2 r)
{
	const s16x2 s = r >> 15, a = (r ^ s) - s;
	const s16x2 t = (s16x2)(a << 10) >> 10;                           /* |r| mod 64 read as a signed 6-bit number */
	const s16x2 d = (t + ((t >> 15) & (s16x2)(short)3)) >> 2;
	return (d ^ s) - s;
}

/* The first direction's two un-normalised taps (filters.c:40-86) of one pair of cells (2k, 2k+1) of a line: d the pair, pv the pair before it, nx the
 * pair behind it (only its first cell counts; the line's last pair hands in itself: x[S] = x[S - 2]).  first: the line's first pair. */
__device__ __forceinline__ void ana_row_taps(uint32_t d, uint32_t pv, uint32_t nx, bool first, int *lo, int *hi)
{
	const int e0 = (int16_t)(d & 0xFFFF), o0 = (int)d >> 16, e1 = (int16_t)(nx & 0xFFFF);
	int em1 = (int16_t)(pv & 0xFFFF), om1 = (int)pv >> 16;
	if (first) { em1 = e1; om1 = o0; }                             /* x[-2] = x[2], x[-1] = x[1] */
	*lo = 6 * e0 + 2 * (om1 + o0) - (em1 + e1);
	*hi = (o0 << 1) - (e0 + e1);                                   /* the last one: (x[S-1] - x[S-2]) << 1, which is what e1 = e0 gives */
}

/* The first direction of one line held two cells to a dword, a lane its own pair (cells 2k, 2k+1, k = lane + 64 u): the pair on the
 * left and the first cell on the right come over the lanes (DPP shifts by one lane, the seam between the two halves of a 256-cell line through a
 * readlane).  lo / hi: the un-normalised taps the pair leaves. */
template <int PPL>
__device__ __forceinline__ void ana_row_pair(const uint32_t (&Dw)[PPL], int lane, int (&lo)[PPL], int (&hi)[PPL])
{
#pragma unroll
	for (int u = 0; u < PPL; u++) {
		uint32_t pv = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)Dw[u], 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
		uint32_t nx = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)Dw[u], 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
		if (u > 0) { const uint32_t seam = (uint32_t)__builtin_amdgcn_readlane((int)Dw[u > 0 ? u - 1 : 0], 63); if (lane == 0) pv = seam; }
		if (u + 1 < PPL) { const uint32_t seam = (uint32_t)__builtin_amdgcn_readlane((int)Dw[u + 1 < PPL ? u + 1 : u], 0); if (lane == 63) nx = seam; }
		else if (lane == 63) nx = Dw[u];                           /* x[S] = x[S - 2] */
		ana_row_taps(Dw[u], pv, nx, u == 0 && lane == 0, &lo[u], &hi[u]);
	}
}

/* The same of a 256-cell line held FOUR adjacent cells to a lane (a, b: cells 4 lane .. 4 lane + 3, as k_l2_recon's Y9 leaves a row): lo / hi [0] are
 * the taps of pair 2 lane, [1] those of pair 2 lane + 1.  Only the pair before a and the first cell behind b come over the lanes. */
__device__ __forceinline__ void ana_row_quad(uint32_t a, uint32_t b, int lane, int (&lo)[2], int (&hi)[2])
{
	const uint32_t pv = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)b, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
	uint32_t nx = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)a, 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
	if (lane == 63) nx = b;                                        /* x[S] = x[S - 2] */
	ana_row_taps(a, pv, b, lane == 0, &lo[0], &hi[0]);
	ana_row_taps(b, a, nx, false, &lo[1], &hi[1]);
}

/* The second direction (filters.c:88-287) of two columns at once: Ew / Ow hold the even / odd rows' cells of the two columns, a lane its own row pair
 * k = lane + 64 u; lo / hi: what the pair leaves for its two columns.  left: the columns lie in the first direction's low-pass half. */
template <int PPL, int HLF, bool IN_RANGE = false /* the caller vouches for the 16-bit range (cells made from bytes): no test, no 32-bit form */>
__device__ __forceinline__ void ana_col_pair(const uint32_t (&Ew)[PPL], const uint32_t (&Ow)[PPL], bool left, int lane, int (&lo)[PPL][2], int (&hi)[PPL][2])
{
	/* Two columns side by side in packed 16-bit arithmetic wherever nothing can leave 16 bits: with every cell of the wavefront's two columns in
	 * -1300 .. 3000 the un-normalised sums stay inside (10 x 3000 + 2 x 1300 < 32768) -- which is every block of the suite's images (below
	 * about 2200; the level-2 input is LL1, the level-1 chroma input a byte plane), not of every picture: hard edges in the filters' own sign
	 * pattern reach about 3480 in luma and 3095 in chroma ("The 16-bit gate of the second direction";
	 * tests/test_filterbank_gate.py).  A pair outside that range takes the 32-bit form below, which follows the reference's int arithmetic
	 * where it wraps. */
	bool wide = false;
	if (!IN_RANGE)
#pragma unroll
	for (int u = 0; u < PPL; u++) {
		const uint32_t mx = pk_max_u16x(pk_add16(Ew[u], 0x05140514u), pk_add16(Ow[u], 0x05140514u));   /* + 1300: in range = at most 4300 as unsigned */
		wide |= (mx & 0xFFFFu) > 4300u || (mx >> 16) > 4300u;
	}
	if (IN_RANGE || !__any(wide)) {
		uint32_t rlast = 0;
#pragma unroll
		for (int u = 0; u < PPL; u++) {
			const int k = lane + 64 * u;
			uint32_t em = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)Ew[u], 0x138, 0xF, 0xF, false), om = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)Ow[u], 0x138, 0xF, 0xF, false);
			uint32_t en = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)Ew[u], 0x130, 0xF, 0xF, false);
			if (u > 0) {
				const uint32_t se = (uint32_t)__builtin_amdgcn_readlane((int)Ew[u > 0 ? u - 1 : 0], 63), so_ = (uint32_t)__builtin_amdgcn_readlane((int)Ow[u > 0 ? u - 1 : 0], 63);
				if (lane == 0) { em = se; om = so_; }
			}
			if (u + 1 < PPL) { const uint32_t se = (uint32_t)__builtin_amdgcn_readlane((int)Ew[u + 1 < PPL ? u + 1 : u], 0); if (lane == 63) en = se; }
			else if (lane == 63) en = Ew[u];
			if (u == 0 && lane == 0) { em = en; om = Ow[u]; }
			const s16x2 e0 = as_s(Ew[u]), o0 = as_s(Ow[u]), em1 = as_s(em), om1 = as_s(om), e1 = as_s(en);
			const s16x2 r = e0 * (s16x2)(short)6 + ((om1 + o0) << 1) - (em1 + e1);
			s16x2 a = e0 + e1;
			a = a + (a & (em1 + e0) & as_s((k & 1) ? 0x00010001u : 0u));
			const s16x2 pp = o0 - (a >> 1), tail = o0 - e0;
			s16x2 l, h;
			if (left) {
				uint32_t rp = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)as_w(r), 0x138, 0xF, 0xF, false);
				if (lane == 0) rp = rlast;
				const s16x2 carry = k > 0 ? pk_diffuse(as_s(rp)) : (s16x2)(short)0;
				rlast = (uint32_t)__builtin_amdgcn_readlane((int)as_w(r), 63);
				l = pk_rnd_half_away(r + carry, 6);
				h = k < HLF - 1 ? pk_rnd_half_away(pp, 3) : (tail >> 3);
			} else {
				l = pk_rnd_half_away(r, 4);
				h = k < HLF - 1 ? pk_rnd_half_away(pp, 1) : ((tail + (s16x2)(short)1) >> 1);   /* pp > 0 ? (pp + 1) >> 1 : pp >> 1 is rounding half away at shift 1 */
			}
			lo[u][0] = l.x; lo[u][1] = l.y; hi[u][0] = h.x; hi[u][1] = h.y;
		}
	} else {
	int rlast[2] = { 0, 0 };                                    /* r of cell 63 of the half before (the seam of the carry) */
#pragma unroll
		for (int u = 0; u < PPL; u++) {
			const int k = lane + 64 * u;
			uint32_t em = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)Ew[u], 0x138, 0xF, 0xF, false), om = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)Ow[u], 0x138, 0xF, 0xF, false);
			uint32_t en = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)Ew[u], 0x130, 0xF, 0xF, false);
			if (u > 0) {
				const uint32_t se = (uint32_t)__builtin_amdgcn_readlane((int)Ew[u > 0 ? u - 1 : 0], 63), so_ = (uint32_t)__builtin_amdgcn_readlane((int)Ow[u > 0 ? u - 1 : 0], 63);
				if (lane == 0) { em = se; om = so_; }
			}
			if (u + 1 < PPL) { const uint32_t se = (uint32_t)__builtin_amdgcn_readlane((int)Ew[u + 1 < PPL ? u + 1 : u], 0); if (lane == 63) en = se; }
			else if (lane == 63) en = Ew[u];                           /* x[S] = x[S - 2] */
			if (u == 0 && lane == 0) { em = en; om = Ow[u]; }           /* x[-2] = x[2], x[-1] = x[1] */
#pragma unroll
			for (int h = 0; h < 2; h++) {
				const int e0 = h ? (int)Ew[u] >> 16 : (int16_t)(Ew[u] & 0xFFFF), o0 = h ? (int)Ow[u] >> 16 : (int16_t)(Ow[u] & 0xFFFF);
				const int em1 = h ? (int)em >> 16 : (int16_t)(em & 0xFFFF), om1 = h ? (int)om >> 16 : (int16_t)(om & 0xFFFF), e1 = h ? (int)en >> 16 : (int16_t)(en & 0xFFFF);
				const int r = 6 * e0 + 2 * (om1 + o0) - (em1 + e1);
				int a = e0 + e1;
				if ((k & 1) && (a & 1) && ((em1 + e0) & 1)) a++;
				const int pp = o0 - (a >> 1), tail = o0 - e0;          /* the predicted odd sample; the last one: x[S-1] - x[S-2] */
				if (left) {
					int rp = __builtin_amdgcn_update_dpp(0, r, 0x138, 0xF, 0xF, false);   /* the cell before: its carry comes in (filters.c:203-287) */
					if (lane == 0) rp = rlast[h];
					const int carry = k > 0 ? diffuse(rp) : 0;
					rlast[h] = __builtin_amdgcn_readlane(r, 63);
					lo[u][h] = rnd_half_away((int16_t)(r + carry), 6);
					hi[u][h] = k < HLF - 1 ? rnd_half_away(pp, 3) : (tail >> 3);
				} else {
					lo[u][h] = rnd_half_away(r, 4);
					hi[u][h] = k < HLF - 1 ? (pp > 0 ? (pp + 1) >> 1 : pp >> 1) : ((tail + 1) >> 1);
				}
			}
		}
	}
}

#endif
