/*
 * nhw_picture.hip -- pictures of any size as 512 x 512 tiles (DESIGN.md sections 11 to 17): the padding kernel k_tile_pad; the crops, which
 * share one body (crop_band over copy_rows) and differ in how a workgroup learns its tile and its rectangle -- k_untile_crop (k_tile_pad's
 * inverse: the whole picture, also from the 256 and 128 tiles of a scaled decode), k_untile_region (first_tile search) and k_untile_window (use
 * table) --; the picture-cropped error k_sse_crop; the conversions between bytes and tensor formats, k_bytes_to_tensor (section 16) and its
 * mirrors k_tensor_to_bytes and k_tile_pad_tensor (section 17); and the exports of the host's geometry of tiles, regions, windows and crop
 * scales and of the .nhwp container, whose rules are in nhw_container.h.  The resamplers (sections 18 to 20) are in nhw_resample.hip.
 *
 * Padding rule: a W x H picture (B, G, R bytes, rows in BMP file order) is padded to 512 nx x 512 ny, nx = ceil(W / 512),
 * ny = ceil(H / 512), by edge replication: padded pixel (r, c) = picture pixel (min(r, H - 1), min(c, W - 1)).  Tile (ty, tx) is padded
 * rows 512 ty .. and columns 512 tx .., index ty nx + tx; a picture's tiles are numbered from its descriptor's first_tile on.
 *
 * k_tile_pad and the crops are copies: a workgroup moves one band of TP_ROWS rows of one tile (k_sse_crop reads one the same way).  The
 * picture side may have any alignment and any pitch.  k_tile_pad reaches its bytes through the naturally aligned dwords that hold them,
 * funnelled together with v_alignbyte_b32 (fetch), and stores the 16-byte-aligned tile side in dwordx4; the crops store the 16-byte-aligned
 * words of the picture side and fetch the tile side at whatever phase that leaves.  No load touches a word that holds no byte of a picture
 * row (or, for the crops, of the tile bytes they store), and no store touches a byte outside a picture row.
 */
#include <string.h>
#include <type_traits>

#include "nhw_host.h"
#include "nhw_sse.h"
#include "nhw_tensor.h"

namespace {

constexpr int TP_ROWS = 32;                 /* tile rows per workgroup */
constexpr int TP_BANDS = 512 / TP_ROWS;     /* workgroups per tile */
constexpr int TP_WORDS = 1536 / 16;         /* 16-byte words per tile row */
constexpr int TP_THREADS = 256;

/* Bytes [j, e) of the 16 bytes at address p, at their places in the result (the other bytes 0).  Loads only the naturally aligned dwords
 * that hold one of those bytes (one dwordx4 when p is 16-byte aligned and all 16 are wanted), so it never reads a word the caller did not
 * name a byte of. */
__device__ __forceinline__ uint4 fetch(uintptr_t p, int j, int e)
{
	if (j == 0 && e == 16 && !(p & 15)) return *reinterpret_cast<const uint4 *>(p);
	const uint32_t *a = reinterpret_cast<const uint32_t *>(p & ~(uintptr_t)3);
	const int sh = (int)(p & 3), lo = sh + j, hi = sh + e;
	uint32_t d[5];
#pragma unroll
	for (int q = 0; q < 5; q++) d[q] = (4 * q + 4 > lo && 4 * q < hi) ? a[q] : 0u;
	return make_uint4(__builtin_amdgcn_alignbyte(d[1], d[0], sh), __builtin_amdgcn_alignbyte(d[2], d[1], sh),
	                  __builtin_amdgcn_alignbyte(d[3], d[2], sh), __builtin_amdgcn_alignbyte(d[4], d[3], sh));
}

/* the picture holding global tile t: the last descriptor with first_tile <= t.  A wave probes 64 evenly spaced entries at a time, so a
 * table of 65535 pictures takes three rounds of loads; the answer is the same in every lane.  P: nhw_picture or nhw_tensor_picture */
template <class P>
__device__ __forceinline__ int find_picture(const P *pics, int n, uint32_t t)
{
	int lo = 0, hi = n;
	const int lane = threadIdx.x & 63;
	while (hi - lo > 1) {
		const int step = (hi - lo + 63) / 64, idx = lo + lane * step;
		const bool le = idx < hi && pics[idx].first_tile <= t;
		const int c = __popcll(__ballot(le));
		lo += (c > 0 ? c - 1 : 0) * step;
		hi = lo + step < hi ? lo + step : hi;
	}
	return __builtin_amdgcn_readfirstlane(lo);
}

template <class P> struct TileRefOf {
	P p;
	uint32_t ty, tx;
	int k;                                  /* the picture's index in the table */
};
using TileRef = TileRefOf<nhw_picture>;

/* the workgroup's tile (tile0 + blockIdx.x / bands of a tile) and its picture; false for a tile no picture of the table holds.  T: the tile's
 * side, 512 or, for the tiles of a scaled decode, 256 or 128 -- the table then holds the scaled pictures */
template <int T = 512, class P>
__device__ __forceinline__ bool tile_of(const P *pics, int n, int tile0, TileRefOf<P> &r)
{
	const uint32_t t = (uint32_t)tile0 + blockIdx.x / (T / TP_ROWS);
	r.k = find_picture(pics, n, t);
	r.p = pics[r.k];
	if (!r.p.width || !r.p.height || t < r.p.first_tile) return false;
	const uint32_t nx = (r.p.width + T - 1) / T, ny = (r.p.height + T - 1) / T, in = t - r.p.first_tile;
	if (in >= nx * ny) return false;
	r.ty = in / nx; r.tx = in % nx;
	return true;
}

/* padded word w of padded row rr of the tile: 16 bytes of picture row min(512 ty + rr, H - 1) from byte column 512 C tx + 16 w on, C bytes a
 * pixel: 3, or 1 for the grey pictures of DESIGN.md section 27.  EDGE: the tile reaches column C W, so a word may cross it or lie beyond it;
 * those bytes repeat the row's last pixel (a C-byte period). */
template <bool EDGE, int C = 3>
__device__ __forceinline__ uint4 pad_word(const TileRef &r, int rr, int w)
{
	const uint32_t row = 512 * r.ty + rr < r.p.height ? 512 * r.ty + rr : r.p.height - 1;
	const uintptr_t R = (uintptr_t)(r.p.addr + (uint64_t)row * r.p.pitch);
	const int rb = C * (int)r.p.width, b0 = 512 * C * (int)r.tx + 16 * w, nin = rb - b0;
	if (!EDGE || nin >= 16) return fetch(R + b0, 0, 16);
	uint4 v = nin > 0 ? fetch(R + b0, 0, nin) : make_uint4(0, 0, 0, 0);
	const uint32_t px = fetch(R + rb - C, 0, C).x;                     /* B, G, R of the last pixel (C = 1: its byte) */
	const int r0 = b0 % C;                                             /* padded column b0 + j holds component (r0 + j) % C */
	uint32_t o[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
	for (int j = 0; j < 16; j++) {
		int c = r0 + j % C;
		c -= c >= C ? C : 0;
		const uint32_t byte = (px >> (8 * c)) & 0xFF, sh = 8 * (j & 3);
		if (j >= nin) o[j >> 2] = (o[j >> 2] & ~(0xFFu << sh)) | (byte << sh);
	}
	return make_uint4(o[0], o[1], o[2], o[3]);
}

template <bool EDGE, int C = 3>
__device__ __forceinline__ void pad_band(const TileRef &r, uint4 *__restrict__ dst, int band)
{
	constexpr int ROW_WORDS = C * 512 / 16, WORDS = TP_ROWS * ROW_WORDS, PER = WORDS / TP_THREADS, GROUP = 4;
	static_assert(ROW_WORDS * 3 == TP_WORDS * C && WORDS % TP_THREADS == 0 && PER % GROUP == 0, "band layout");
#pragma unroll
	for (int g = 0; g < PER; g += GROUP) {
		uint4 v[GROUP];
#pragma unroll
		for (int k = 0; k < GROUP; k++) {
			const int i = (g + k) * TP_THREADS + threadIdx.x;
			v[k] = pad_word<EDGE, C>(r, band * TP_ROWS + i / ROW_WORDS, i % ROW_WORDS);
		}
#pragma unroll
		for (int k = 0; k < GROUP; k++) dst[(g + k) * TP_THREADS + threadIdx.x] = v[k];
	}
}

__global__ __launch_bounds__(TP_THREADS) void k_tile_pad(const nhw_picture *__restrict__ pics, int n_pics, int tile0, uint8_t *__restrict__ tiles)
{
	TileRef r;
	if (!tile_of(pics, n_pics, tile0, r)) return;
	const int band = blockIdx.x % TP_BANDS;
	uint4 *dst = reinterpret_cast<uint4 *>(tiles + (size_t)(blockIdx.x / TP_BANDS) * NHW_IMG_BYTES) + band * TP_ROWS * TP_WORDS;
	if (1536 * (r.tx + 1) <= 3 * r.p.width) pad_band<false>(r, dst, band);   /* an interior tile column: never the replication path */
	else pad_band<true>(r, dst, band);
}

/* the same at one byte a pixel: [H][W] pictures into tiles of 512 x 512 bytes, the same grid and the same aligned access */
__global__ __launch_bounds__(TP_THREADS) void k_tile_pad_grey(const nhw_picture *__restrict__ pics, int n_pics, int tile0, uint8_t *__restrict__ tiles)
{
	TileRef r;
	if (!tile_of(pics, n_pics, tile0, r)) return;
	const int band = blockIdx.x % TP_BANDS;
	uint4 *dst = reinterpret_cast<uint4 *>(tiles + (size_t)(blockIdx.x / TP_BANDS) * (512 * 512)) + band * TP_ROWS * (512 / 16);
	if (512 * (r.tx + 1) <= r.p.width) pad_band<false, 1>(r, dst, band);
	else pad_band<true, 1>(r, dst, band);
}

/* the bytes [j, e) of v to the 16-byte-aligned destination word A, each store inside them: dwords where a whole one is covered, else
 * shorts and bytes (never a read-modify-write: the neighbouring bytes may be another row's, another thread's) */
__device__ __forceinline__ void store_part(uint8_t *A, uint4 v, int j, int e)
{
	const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
	for (int s = 0; s < 4; s++) {
		const int b = 4 * s;
		if (j <= b && b + 4 <= e) { *reinterpret_cast<uint32_t *>(A + b) = w[s]; continue; }
#pragma unroll
		for (int h = 0; h < 2; h++) {
			const int c = b + 2 * h;
			const bool c0 = j <= c && c < e, c1 = j <= c + 1 && c + 1 < e;
			if (c0 && c1) *reinterpret_cast<uint16_t *>(A + c) = (uint16_t)(w[s] >> (16 * h));
			else if (c0) A[c] = (uint8_t)(w[s] >> (16 * h));
			else if (c1) A[c + 1] = (uint8_t)(w[s] >> (16 * h + 8));
		}
	}
}

/* ---- the crops: what a tile and a rectangle of its picture have in common, from the tile to the rectangle's destination ----
 * The copy: `rows` rows of seg bytes (3 .. ROW), row q from src + q ROW (anywhere inside a tile row of ROW bytes) to dst + q pitch (any
 * alignment, any pitch).  The 16-byte-aligned destination words that cover a row's bytes, whole ones as dwordx4, the ragged head and tail
 * with store_part, the tile side through fetch, only the bytes it stores; the two sides have independent phases, and the words a row needs
 * (at most seg / 16 + 2; a whole row of a 512 tile: 97) depend on seg: the rows x that many slots are dealt out flat over the threads (slot
 * -> row by a multiply-high with the reciprocal, exact for the 32 x 97 slots a band can have), so that a 224-pixel crop does not walk 97
 * slots a row.  ONE: seg may be below 3 (the one-byte pixels of DESIGN.md section 23), down to 1, which has one slot a row: the reciprocal
 * of 1 is 2^32 and wraps to 0 in 32 bits, so the quotient is taken as the index itself there. */
template <int ROW, bool ONE = false>
__device__ __forceinline__ void copy_rows(uintptr_t src, uintptr_t dst, uint64_t pitch, int seg, uint32_t rows)
{
	const uint32_t slots = (uint32_t)(seg + 30) / 16, total = rows * slots;   /* 2 .. 97 words cover seg bytes at any phase (ONE: 1 .. 33) */
	const uint32_t rcp = 0xFFFFFFFFu / slots + 1;                         /* i / slots = umulhi(i, rcp) for i < 2^32 / slots, slots >= 2 */
	for (uint32_t i = threadIdx.x; i < total; i += TP_THREADS) {
		const uint32_t q = ONE && slots == 1 ? i : __umulhi(i, rcp), k = i - q * slots;   /* row q of the band's wanted rows, word k of it */
		const uintptr_t D0 = dst + (uint64_t)q * pitch, D1 = D0 + seg;
		const uintptr_t A = (D0 & ~(uintptr_t)15) + 16 * (uintptr_t)k;
		if (A >= D1) continue;
		const int j = A < D0 ? (int)(D0 - A) : 0, e = A + 16 > D1 ? (int)(D1 - A) : 16;
		const uint4 v = fetch(src + (uintptr_t)q * ROW + (A - D0), j, e);   /* (A - D0 wraps below 0 for the head word: fetch reads from byte j on) */
		if (j == 0 && e == 16) *reinterpret_cast<uint4 *>(A) = v;
		else store_part(reinterpret_cast<uint8_t *>(A), v, j, e);
	}
}

/* The workgroup's band of TP_ROWS rows of the tile (ty, tx) of side T at `tile` (C T bytes a row, C bytes a pixel: 3, or 1 for the grey tiles of
 * DESIGN.md section 23; T = 512, or 256 or 128: the tiles of a scaled decode, section 14), into the rectangle x, y, width, height of g: tile row rr
 * is picture row T ty + rr, wanted if y <= row < y + height; of it the picture columns [c0, c1) = [max(T tx, x), min(T tx + T, x + width)) go
 * from tile byte C (c0 - T tx) of the row to byte C (c0 - x) of destination row (row - y).  A band or a tile that shares nothing with the rectangle
 * stores nothing.  With C = 1 a segment has 1 .. T bytes where the colour form has 3 .. 3 T, and copy_rows is told so (ONE): a run of seg bytes
 * at phase ph touches the words 0 .. (ph + seg - 1) / 16, at most (seg + 30) / 16 of them (ph = 15), so its slot count is right for the short
 * segments too -- 1 for seg = 1, 2 for seg = 2 -- and a slot whose word starts at or behind the run's end is passed over by A >= D1; its
 * reciprocal is exact for 2 slots (2^31: a shift) but not for 1, where 2^32 does not fit, and there the quotient is the index itself. */
template <int T, int C = 3>
__device__ __forceinline__ void crop_band(const uint8_t *tile, uint32_t ty, uint32_t tx, const nhw_region &g)
{
	constexpr int ROW = C * T;
	const uint32_t top = T * ty + (blockIdx.x % (T / TP_ROWS)) * TP_ROWS;   /* picture row of the band's first row */
	const uint32_t lo = top > g.y ? top : g.y, hi = top + TP_ROWS < g.y + g.height ? top + TP_ROWS : g.y + g.height;
	const uint32_t c0 = T * tx > g.x ? T * tx : g.x, c1 = T * tx + T < g.x + g.width ? T * tx + T : g.x + g.width;
	if (lo >= hi || c0 >= c1) return;
	const uintptr_t src = (uintptr_t)tile + (uintptr_t)(lo - T * ty) * ROW + C * (c0 - T * tx);
	const uintptr_t dst = (uintptr_t)(g.addr + (uint64_t)(lo - g.y) * g.pitch) + C * (c0 - g.x);
	copy_rows<ROW, C == 1>(src, dst, g.pitch, C * (int)(c1 - c0), hi - lo);   /* C .. C T bytes a row */
}

/* a rectangle of a picture whose tiles have the side T: not empty, the picture's sides at most the largest scaled ones (65535, 32768, 16384),
 * the rectangle inside them */
template <int T>
__device__ __forceinline__ bool rect_of_picture(const nhw_region &g)
{
	constexpr uint32_t SIDE_MAX = (65535 + 512 / T - 1) / (512 / T);
	return g.width && g.height && g.pic_width <= SIDE_MAX && g.pic_height <= SIDE_MAX && (uint64_t)g.x + g.width <= g.pic_width && (uint64_t)g.y + g.height <= g.pic_height;
}

/* k_tile_pad's inverse: global tile tile0 + blockIdx.x / bands of a tile, into the picture that holds it -- the rectangle
 * that is all of the picture.  T = 256, 128: the tiles of a scaled decode, into the scaled pictures of the table. */
template <int T>
__global__ __launch_bounds__(TP_THREADS) void k_untile_crop(const uint8_t *__restrict__ tiles, const nhw_picture *__restrict__ pics, int n_pics, int tile0)
{
	TileRef r;
	if (!tile_of<T>(pics, n_pics, tile0, r)) return;
	crop_band<T>(tiles + (size_t)(blockIdx.x / (T / TP_ROWS)) * (size_t)(3 * T * T), r.ty, r.tx, { r.p.addr, r.p.pitch, 0, 0, r.p.width, r.p.height, r.p.width, r.p.height, 0, 0 });
}

/* A rectangle of a picture from the tiles it touches: tile t = tile0 + blockIdx.x / TP_BANDS of the call's running
 * selection belongs to the last descriptor with first_tile <= t and is tile t - first_tile of that region's selection, row by row. */
__global__ __launch_bounds__(TP_THREADS) void k_untile_region(const uint8_t *__restrict__ tiles, const nhw_region *__restrict__ regs, int n_regs, int tile0)
{
	const uint32_t t = (uint32_t)tile0 + blockIdx.x / TP_BANDS;
	const nhw_region g = regs[find_picture(regs, n_regs, t)];
	if (t < g.first_tile || !rect_of_picture<512>(g)) return;
	const uint32_t tx0 = g.x / 512, ty0 = g.y / 512, nx = (g.x + g.width - 1) / 512 - tx0 + 1, ny = (g.y + g.height - 1) / 512 - ty0 + 1;
	const uint32_t in = t - g.first_tile;
	if (in >= nx * ny) return;
	crop_band<512>(tiles + (size_t)(blockIdx.x / TP_BANDS) * NHW_IMG_BYTES, ty0 + in / nx, tx0 + in % nx, g);
}

/* Windows: rectangles of pictures at scale 1, 2 or 4, every tile decoded once.  One workgroup per band of a USE, a
 * (window, tile) pair of the table: tile (ty, tx) of the picture's grid, decoded into slot u.slot of the call's tiles, feeds window
 * regs[u.region].  The descriptor is section 13's, in the coordinates of the scaled picture (pic_width x pic_height: the scaled sides;
 * first_tile is not read).  A use that names no region of the table, a slot outside the buffer's [tile0, tile0 + m), a tile outside the
 * window's selection or a descriptor that is no window of a picture stores nothing.  k_untile_window_grey is the same over the one-byte
 * pixels of a grey decode: slots of T T bytes, descriptors as they are with a pitch of at least the width. */
template <int T, int C>
__device__ __forceinline__ void window_band(const uint8_t *__restrict__ tiles, const nhw_region *__restrict__ regs, int n_regs, const nhw_window_use *__restrict__ uses, int tile0, int m)
{
	const nhw_window_use u = uses[blockIdx.x / (T / TP_ROWS)];
	if (u.region >= (uint32_t)n_regs || u.slot < (uint32_t)tile0 || u.slot - (uint32_t)tile0 >= (uint32_t)m) return;
	const nhw_region g = regs[u.region];
	if (!rect_of_picture<T>(g)) return;
	if (u.tx < g.x / T || u.tx > (g.x + g.width - 1) / T || u.ty < g.y / T || u.ty > (g.y + g.height - 1) / T) return;   /* not a tile of the window's selection */
	crop_band<T, C>(tiles + (size_t)(u.slot - (uint32_t)tile0) * (size_t)(C * T * T), u.ty, u.tx, g);
}
template <int T>
__global__ __launch_bounds__(TP_THREADS) void k_untile_window(const uint8_t *__restrict__ tiles, const nhw_region *__restrict__ regs, int n_regs,
                                                               const nhw_window_use *__restrict__ uses, int tile0, int m)
{
	window_band<T, 3>(tiles, regs, n_regs, uses, tile0, m);
}
template <int T>
__global__ __launch_bounds__(TP_THREADS) void k_untile_window_grey(const uint8_t *__restrict__ tiles, const nhw_region *__restrict__ regs, int n_regs,
                                                                    const nhw_window_use *__restrict__ uses, int tile0, int m)
{
	window_band<T, 1>(tiles, regs, n_regs, uses, tile0, m);
}

/* The SSE of decoded tiles against the pictures' own bytes: tile row rr of tile (ty, tx) against picture row 512 ty + rr < H, bytes
 * [1536 tx, min(1536 tx + 1536, 3W)); rows past H and bytes past 3W (the padding) never count.  Word w of a row: the picture side through
 * fetch (only the dwords that hold picture bytes, any alignment and pitch), the tile side as an aligned dwordx4.  In a word that crosses
 * 3W the bytes from 3W on are masked to zero on both sides (on the picture side the dword that holds the row's last byte brings the bytes
 * behind it along: another row's, or whatever follows the picture), so they add 0.  Per word sse16 (nhw_sse.h): three v_dot4_u32_u8 a dword, exact.
 * Bounds: a band is 32 rows x 96 words; a thread takes 12 words (at most 12 x 16 x 255^2 = 12.5 M), a wavefront 64 threads (at most 799 M),
 * both in 32 bits; the four wavefronts are added in 64 bits (a band's sum is at most 49 152 x 255^2 = 3.2 G, a picture's far beyond 32 bits)
 * and the workgroup adds its band to sse[k] with one 64-bit integer atomic.  Integer addition is associative: the result is exact and does
 * not depend on the order the workgroups ran in.  Accumulates: the caller zeroes sse[]. */
/* bytes [0, nin) of v, the others 0 */
__device__ __forceinline__ uint4 keep_bytes(uint4 v, int nin)
{
	uint32_t o[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
	for (int d = 0; d < 4; d++) {
		const int keep = nin - 4 * d;                                  /* bytes of dword d that are wanted */
		o[d] = keep >= 4 ? o[d] : keep <= 0 ? 0u : o[d] & ((1u << (8 * keep)) - 1u);
	}
	return make_uint4(o[0], o[1], o[2], o[3]);
}

template <bool EDGE>
__device__ __forceinline__ uint32_t sse_band(const TileRef &r, const uint4 *__restrict__ tile, int band)
{
	constexpr int WORDS = TP_ROWS * TP_WORDS, PER = WORDS / TP_THREADS, GROUP = 4;
	static_assert(WORDS % TP_THREADS == 0 && PER % GROUP == 0, "band layout");
	const int seg = 3 * (int)r.p.width - 1536 * (int)r.tx;              /* picture bytes in a tile row (at least 1536 without EDGE) */
	const uint32_t row0 = 512 * r.ty + band * TP_ROWS;
	uint32_t acc = 0;
#pragma unroll
	for (int g = 0; g < PER; g += GROUP) {
		uint4 a[GROUP], b[GROUP];
#pragma unroll
		for (int k = 0; k < GROUP; k++) {
			const int i = (g + k) * TP_THREADS + threadIdx.x, rr = i / TP_WORDS, w = i % TP_WORDS;
			const int nin = EDGE ? (seg - 16 * w < 16 ? seg - 16 * w : 16) : 16;
			a[k] = b[k] = make_uint4(0, 0, 0, 0);
			if (row0 + rr < r.p.height && nin > 0) {
				const uintptr_t R = (uintptr_t)(r.p.addr + (uint64_t)(row0 + rr) * r.p.pitch) + 1536 * r.tx + 16 * w;
				a[k] = fetch(R, 0, nin);
				b[k] = tile[(band * TP_ROWS + rr) * TP_WORDS + w];
				if (EDGE && nin < 16) {
					a[k] = keep_bytes(a[k], nin);
					b[k] = keep_bytes(b[k], nin);
				}
			}
		}
#pragma unroll
		for (int k = 0; k < GROUP; k++) acc += sse16(a[k], b[k]);
	}
	return acc;
}

__global__ __launch_bounds__(TP_THREADS) void k_sse_crop(const uint8_t *__restrict__ tiles, const nhw_picture *__restrict__ pics, int n_pics, int tile0,
                                                          unsigned long long *__restrict__ sse)
{
	__shared__ uint32_t wsum[TP_THREADS / 64];
	TileRef r;
	if (!tile_of(pics, n_pics, tile0, r)) return;
	const int band = blockIdx.x % TP_BANDS;
	if (512 * r.ty + band * TP_ROWS >= r.p.height) return;             /* a band wholly below the picture: padding only */
	const uint4 *tile = reinterpret_cast<const uint4 *>(tiles + (size_t)(blockIdx.x / TP_BANDS) * NHW_IMG_BYTES);
	uint32_t acc = 1536 * (r.tx + 1) <= 3 * r.p.width ? sse_band<false>(r, tile, band) : sse_band<true>(r, tile, band);
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
	if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
	__syncthreads();
	if (threadIdx.x == 0) {
		unsigned long long s = 0;
#pragma unroll
		for (int w = 0; w < TP_THREADS / 64; w++) s += wsum[w];
		atomicAdd(sse + r.k, s);
	}
}

/* What is already bytes, to a tensor format: picture k of the table to [H][W][3] or [3][H][W] elements at out_addr[k], under the
 * value rule of nhw_tensor.h.  The host knows no picture's size (the table lives in device memory), so a picture gets `per` workgroups whatever its
 * size and workgroup `part` walks rows part, part + per, ...; a thread takes a pixel of the row at a time: three byte loads (any alignment and pitch:
 * consecutive lanes on consecutive 3-byte pieces, never a byte outside the row) and the pixel's three element stores (nhw_store_pixel) -- in CHW
 * consecutive lanes on consecutive elements of a plane, in HWC 3 elements apart.  Pictures and tensors have no alignment to build wider stores on
 * (W is any number).  The resampling forms of this kernel are in nhw_resample.hip. */
template <int DT, int CHW>
__global__ __launch_bounds__(TP_THREADS) void k_bytes_to_tensor(const nhw_picture *__restrict__ pics, int per, NhwTensorArgs a, const uint64_t *__restrict__ out_addr)
{
	using E = typename NhwElem<DT>::type;
	const int k = blockIdx.x / per, part = blockIdx.x % per;
	const nhw_picture p = pics[k];
	const uint64_t oa = out_addr[k];
	if (!p.width || !p.height || p.width > 65535u || p.height > 65535u || !oa || (oa & (sizeof(E) - 1))) return;
	E *out = reinterpret_cast<E *>(oa);
	const size_t W = p.width, H = p.height;
	for (uint32_t r = part; r < p.height; r += per) {
		const uint8_t *src = reinterpret_cast<const uint8_t *>(p.addr + (uint64_t)r * p.pitch);
		const size_t rr = a.flip ? H - 1 - r : r;
		for (uint32_t c = threadIdx.x; c < p.width; c += TP_THREADS) {
			const uint32_t b[3] = { src[3 * c], src[3 * c + 1], src[3 * c + 2] };
			nhw_store_pixel<DT, CHW>(out, H, W, rr, c, b, a);
		}
	}
}

/* ------------------------------------------------------------------------------------------------ tensors to bytes */
/* N = 4 pixels' elements by tensor channel from a run of a tensor row: CHW three runs of N elements, `plane` bytes apart, HWC one run of 3 N.
 * ALIGN > 0: p is a multiple of it (the batch kernel); 0: looked at when running (the picture kernel's crop views) */
template <int DT, int CHW, int ALIGN>
__device__ __forceinline__ void load_quad(const uint8_t *p, uint64_t plane, uint32_t (*e)[4])
{
	constexpr int EB = NhwElem<DT>::bytes;
	if (CHW) {
#pragma unroll
		for (int c = 0; c < 3; c++) {
			uint32_t d[EB];                                                 /* 4 EB bytes */
			if constexpr (ALIGN != 0) nhw_load_words<4 * EB, (ALIGN < 4 * EB ? ALIGN : 4 * EB)>(p + c * plane, d); else nhw_load_words_any<4 * EB, EB>(p + c * plane, d);
#pragma unroll
			for (int px = 0; px < 4; px++) e[c][px] = nhw_unpack_elem<DT>(d, px);
		}
	} else {
		uint32_t d[3 * EB];                                                 /* 12 EB bytes */
		if constexpr (ALIGN != 0) nhw_load_words<12 * EB, ALIGN>(p, d); else nhw_load_words_any<12 * EB, EB>(p, d);
#pragma unroll
		for (int px = 0; px < 4; px++)
#pragma unroll
			for (int c = 0; c < 3; c++) e[c][px] = nhw_unpack_elem<DT>(d, 3 * px + c);
	}
}

/* n contiguous 512 x 512 tensors to the byte path's pictures.  A thread takes 4 pixels of a row -- columns 4 q .. 4 q + 3 of byte-path row r -- so a
 * row is 128 threads and a workgroup two rows: CHW one load a plane of 16 (f32), 8 (f16, bf16) or 4 bytes (u8), HWC 48 (three 16-byte loads), 24
 * (three 8-byte loads) or 12 contiguous bytes (one 12-byte load), then one 12-byte store.  Consecutive lanes are on consecutive pieces in every load
 * and in the store; every address is a multiple of its access's size (12-byte ones: of 4) because both pointers are 16-byte aligned. */
constexpr int TB_THREADS = 256, TB_QUADS = 512 * 512 / 4;                 /* threads a picture: 65536 */
template <int DT, int CHW>
__global__ __launch_bounds__(TB_THREADS) void k_tensor_to_bytes(const uint8_t *__restrict__ in, NhwTensorArgs a, uint8_t *__restrict__ bgr)
{
	constexpr int EB = NhwElem<DT>::bytes;
	const size_t img = blockIdx.x / (TB_QUADS / TB_THREADS);
	const int i = (blockIdx.x % (TB_QUADS / TB_THREADS)) * TB_THREADS + threadIdx.x, r = i >> 7, q = i & 127;
	const int rr = a.flip ? 511 - r : r;
	const uint8_t *base = in + img * (size_t)(3 * 512 * 512 * EB);
	uint32_t e[3][4], w[3];
	if (CHW) load_quad<DT, 1, 4 * EB>(base + ((size_t)rr * 512 + 4 * q) * EB, (uint64_t)(512 * 512 * EB), e);
	else load_quad<DT, 0, (EB == 4 ? 16 : EB == 2 ? 8 : 4)>(base + ((size_t)rr * 512 + 4 * q) * (3 * EB), 0, e);
	nhw_pixels_to_bytes<DT, 4>(e, a, w);
	nhw_store_words<3, 3>(bgr + img * NHW_IMG_BYTES + ((size_t)r * 512 + 4 * q) * 3, w);
}

/* The one-channel form: n contiguous [512][512] tensors -- [n, 1, 512, 512] and [n, 512, 512, 1] are the same memory -- to
 * grey pictures of 512 x 512 bytes under scale[0] and bias[0].  The same grid and the same 4 pixels a thread: one load of 16, 8 or 4 bytes, one
 * dword store. */
template <int DT>
__global__ __launch_bounds__(TB_THREADS) void k_tensor_to_bytes_grey(const uint8_t *__restrict__ in, NhwTensorArgs a, uint8_t *__restrict__ grey)
{
	constexpr int EB = NhwElem<DT>::bytes;
	const size_t img = blockIdx.x / (TB_QUADS / TB_THREADS);
	const int i = (blockIdx.x % (TB_QUADS / TB_THREADS)) * TB_THREADS + threadIdx.x, r = i >> 7, q = i & 127;
	const int rr = a.flip ? 511 - r : r;
	uint32_t d[EB], w = 0;
	nhw_load_words<4 * EB, 4 * EB>(in + (img * (512 * 512) + (size_t)rr * 512 + 4 * q) * EB, d);
#pragma unroll
	for (int px = 0; px < 4; px++) w |= nhw_tensor_byte<DT>(nhw_unpack_elem<DT>(d, px), a.scale[0], a.bias[0]) << (8 * px);
	*reinterpret_cast<uint32_t *>(grey + img * (512 * 512) + (size_t)r * 512 + 4 * q) = w;
}

/* k_tile_pad for tensor pictures: the same grid (tiles x bands of TP_ROWS rows), a thread 4 pixels of a tile row at a time and one 12-byte store,
 * contiguous across the wavefront.  Tile pixel (rr, cc) of tile (ty, tx) is byte-picture pixel (min(512 ty + rr, H - 1), min(512 tx + cc, W - 1));
 * the row flip comes after the clamp of the row, so the replication acts in byte-picture coordinates.  EDGE false (an interior tile column: all
 * 512 columns lie inside the picture): every quad is a run of the tensor row, load_quad with the address's alignment looked at when running (16, 8
 * or 4 bytes wide; 2 or 1 where an f16 / u8 view starts there).  EDGE true: a quad that crosses or lies beyond column W loads its elements one at a
 * time from the clamped columns.  No load touches anything but an element of the picture. */
template <int DT, int CHW, bool EDGE>
__device__ __forceinline__ void pad_band_tensor(const TileRefOf<nhw_tensor_picture> &r, const NhwTensorArgs &a, uint8_t *__restrict__ dst, int band)
{
	constexpr int EB = NhwElem<DT>::bytes, QUADS = TP_ROWS * 128;
	using E = typename NhwElem<DT>::type;
	const uint32_t W = r.p.width, H = r.p.height;
	const uint64_t px_step = CHW ? EB : 3 * EB, ch_step = CHW ? r.p.plane : EB;
	for (int i = threadIdx.x; i < QUADS; i += TP_THREADS) {
		const int rr = band * TP_ROWS + (i >> 7), q = i & 127;
		const uint32_t R = 512 * r.ty + rr < H ? 512 * r.ty + rr : H - 1, row = a.flip ? H - 1 - R : R, c0 = 512 * r.tx + 4 * q;
		const uint8_t *rowp = reinterpret_cast<const uint8_t *>(r.p.addr + (uint64_t)row * r.p.pitch);
		uint32_t e[3][4], w[3];
		if (!EDGE || c0 + 4 <= W) load_quad<DT, CHW, 0>(rowp + c0 * px_step, r.p.plane, e);
		else {
#pragma unroll
			for (int px = 0; px < 4; px++) {
				const uint32_t col = c0 + px < W ? c0 + px : W - 1;
#pragma unroll
				for (int c = 0; c < 3; c++) e[c][px] = *reinterpret_cast<const E *>(rowp + col * px_step + c * ch_step);
			}
		}
		nhw_pixels_to_bytes<DT, 4>(e, a, w);
		nhw_store_words<3, 3>(dst + ((size_t)rr * 512 + 4 * q) * 3, w);
	}
}

template <int DT, int CHW>
__global__ __launch_bounds__(TP_THREADS) void k_tile_pad_tensor(const nhw_tensor_picture *__restrict__ pics, int n_pics, int tile0, NhwTensorArgs a, uint8_t *__restrict__ tiles)
{
	constexpr uint64_t EB = NhwElem<DT>::bytes;
	TileRefOf<nhw_tensor_picture> r;
	if (!tile_of(pics, n_pics, tile0, r)) return;
	if (r.p.width > 65535u || r.p.height > 65535u || !r.p.addr || ((r.p.addr | r.p.pitch | (CHW ? r.p.plane : 0)) & (EB - 1))) return;
	uint8_t *dst = tiles + (size_t)(blockIdx.x / TP_BANDS) * NHW_IMG_BYTES;
	if (512 * (r.tx + 1) <= r.p.width) pad_band_tensor<DT, CHW, false>(r, a, dst, blockIdx.x % TP_BANDS);
	else pad_band_tensor<DT, CHW, true>(r, a, dst, blockIdx.x % TP_BANDS);
}

} /* namespace */

hipError_t nhw_launch_tensor_to_bytes(const void *d_in, int n, int dtype, int layout, const NhwTensorArgs &a, uint8_t *d_bgr, hipStream_t s)
{
	nhw_with_tensor_store(dtype, layout, a, [&](auto st) {
		constexpr int DT = decltype(st)::dtype, CHW = decltype(st)::layout;
		k_tensor_to_bytes<DT, CHW><<<n * (TB_QUADS / TB_THREADS), TB_THREADS, 0, s>>>((const uint8_t *)d_in, a, d_bgr);
	});
	return hipGetLastError();
}

hipError_t nhw_launch_tensor_to_bytes_grey(const void *d_in, int n, int dtype, const NhwTensorArgs &a, uint8_t *d_grey, hipStream_t s)
{
	nhw_with_grey_store(dtype, NhwGreyArgs{}, [&](auto st) {
		constexpr int DT = decltype(st)::dtype;
		k_tensor_to_bytes_grey<DT><<<n * (TB_QUADS / TB_THREADS), TB_THREADS, 0, s>>>((const uint8_t *)d_in, a, d_grey);
	});
	return hipGetLastError();
}

hipError_t nhw_launch_tile_pad_tensor(const nhw_tensor_picture *d_pics, int n_pics, int tile0, int m, int dtype, int layout, const NhwTensorArgs &a, uint8_t *d_tiles, hipStream_t s)
{
	nhw_with_tensor_store(dtype, layout, a, [&](auto st) {
		constexpr int DT = decltype(st)::dtype, CHW = decltype(st)::layout;
		k_tile_pad_tensor<DT, CHW><<<m * TP_BANDS, TP_THREADS, 0, s>>>(d_pics, n_pics, tile0, a, d_tiles);
	});
	return hipGetLastError();
}

hipError_t nhw_launch_bytes_to_tensor(const nhw_picture *d_pics, int n_pics, int dtype, int layout, const NhwTensorArgs &a, const uint64_t *d_out_addr, hipStream_t s)
{
	const int per = n_pics >= 256 ? 16 : n_pics >= 4 ? 4096 / n_pics : 1024;   /* workgroups a picture: some 4096 in all, 16 .. 1024 each */
	nhw_with_tensor_store(dtype, layout, a, [&](auto st) {
		constexpr int DT = decltype(st)::dtype, CHW = decltype(st)::layout;
		k_bytes_to_tensor<DT, CHW><<<n_pics * per, TP_THREADS, 0, s>>>(d_pics, per, a, d_out_addr);
	});
	return hipGetLastError();
}

hipError_t nhw_launch_tile_pad(const nhw_picture *d_pics, int n_pics, int tile0, int m, uint8_t *d_tiles, hipStream_t s)
{
	k_tile_pad<<<m * TP_BANDS, TP_THREADS, 0, s>>>(d_pics, n_pics, tile0, d_tiles);
	return hipGetLastError();
}

hipError_t nhw_launch_tile_pad_grey(const nhw_picture *d_pics, int n_pics, int tile0, int m, uint8_t *d_tiles, hipStream_t s)
{
	k_tile_pad_grey<<<m * TP_BANDS, TP_THREADS, 0, s>>>(d_pics, n_pics, tile0, d_tiles);
	return hipGetLastError();
}

/* f(the tile side 512 / scale as a std::integral_constant) for a scale of 1, 2 or 4, and the launch's error; any other scale is refused */
template <class F> static hipError_t with_tile_side(int scale, F &&f)
{
	switch (scale) {
	case 1: f(std::integral_constant<int, 512>{}); break;
	case 2: f(std::integral_constant<int, 256>{}); break;
	case 4: f(std::integral_constant<int, 128>{}); break;
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

hipError_t nhw_launch_untile_crop(const uint8_t *d_tiles, const nhw_picture *d_pics, int n_pics, int tile0, int m, int scale, hipStream_t s)
{
	return with_tile_side(scale, [&](auto side) {
		constexpr int T = decltype(side)::value;
		k_untile_crop<T><<<m * (T / TP_ROWS), TP_THREADS, 0, s>>>(d_tiles, d_pics, n_pics, tile0);
	});
}

hipError_t nhw_launch_untile_region(const uint8_t *d_tiles, const nhw_region *d_regs, int n_regs, int tile0, int m, hipStream_t s)
{
	k_untile_region<<<m * TP_BANDS, TP_THREADS, 0, s>>>(d_tiles, d_regs, n_regs, tile0);
	return hipGetLastError();
}

hipError_t nhw_launch_untile_window(const uint8_t *d_tiles, const nhw_region *d_regs, int n_regs, const nhw_window_use *d_uses, int n_uses, int tile0, int m, int scale, hipStream_t s)
{
	return with_tile_side(scale, [&](auto side) {
		constexpr int T = decltype(side)::value;
		k_untile_window<T><<<n_uses * (T / TP_ROWS), TP_THREADS, 0, s>>>(d_tiles, d_regs, n_regs, d_uses, tile0, m);
	});
}

hipError_t nhw_launch_untile_window_grey(const uint8_t *d_tiles, const nhw_region *d_regs, int n_regs, const nhw_window_use *d_uses, int n_uses, int tile0, int m, int scale, hipStream_t s)
{
	return with_tile_side(scale, [&](auto side) {
		constexpr int T = decltype(side)::value;
		k_untile_window_grey<T><<<n_uses * (T / TP_ROWS), TP_THREADS, 0, s>>>(d_tiles, d_regs, n_regs, d_uses, tile0, m);
	});
}

hipError_t nhw_launch_sse_crop(const uint8_t *d_tiles, const nhw_picture *d_pics, int n_pics, int tile0, int m, uint64_t *d_sse, hipStream_t s)
{
	k_sse_crop<<<m * TP_BANDS, TP_THREADS, 0, s>>>(d_tiles, d_pics, n_pics, tile0, reinterpret_cast<unsigned long long *>(d_sse));
	return hipGetLastError();
}

/* ------------------------------------------------------------------------------------------------ the .nhwp container (host): nhw_container.h */
extern "C" int nhw_picture_tiles(uint32_t width, uint32_t height) { return nhw_rule_picture_tiles(width, height); }
extern "C" int nhw_picture_scaled_size(uint32_t width, uint32_t height, int scale, uint32_t *scaled_width, uint32_t *scaled_height) { return nhw_rule_picture_scaled_size(width, height, scale, scaled_width, scaled_height); }
extern "C" int nhw_region_tiles(uint32_t pic_width, uint32_t pic_height, uint32_t x, uint32_t y, uint32_t width, uint32_t height) { return nhw_rule_region_tiles(pic_width, pic_height, x, y, width, height); }
extern "C" int nhw_window_tiles(uint32_t pic_width, uint32_t pic_height, int scale, uint32_t x, uint32_t y, uint32_t width, uint32_t height) { return nhw_rule_window_tiles(pic_width, pic_height, scale, x, y, width, height); }
extern "C" int nhw_crop_scale(uint32_t width, uint32_t height, uint32_t out_width, uint32_t out_height) { return nhw_rule_crop_scale(width, height, out_width, out_height); }
extern "C" int nhw_picture_info(const uint8_t *container, size_t len, uint32_t *width, uint32_t *height) { return nhw_container_info(container, len, width, height); }
