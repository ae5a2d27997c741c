/*
 * nhw_picture.hip -- pictures of any size as 512 x 512 tiles (DESIGN.md sections 11 to 18): the padding kernel k_tile_pad; the crops, which
 * share one body (crop_band over copy_rows) and differ in how a workgroup learns its tile and its rectangle -- k_untile_crop (k_tile_pad's
 * inverse: the whole picture, also from the 256 and 128 tiles of a scaled decode), k_untile_region (first_tile search) and k_untile_window (use
 * table) --; the picture-cropped error k_sse_crop, the pointwise k_bytes_to_tensor (section 16) and its resampling form k_resize_to_tensor
 * (section 18) with its area-filter form k_area_to_tensor (section 19), its mirrors k_tensor_to_bytes and k_tile_pad_tensor (section 17), and the .nhwp container that holds a picture's width, height
 * and tile files.
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

/* padded word w of padded row rr of the tile: 16 bytes of picture row min(512 ty + rr, H - 1) from byte column 1536 tx + 16 w on.
 * EDGE: the tile reaches column 3W, so a word may cross it or lie beyond it; those bytes repeat the row's last pixel (a 3-byte period). */
template <bool EDGE>
__device__ __forceinline__ uint4 pad_word(const TileRef &r, int rr, int w)
{
	const uint32_t row = 512 * r.ty + rr < r.p.height ? 512 * r.ty + rr : r.p.height - 1;
	const uintptr_t R = (uintptr_t)(r.p.addr + (uint64_t)row * r.p.pitch);
	const int rb = 3 * (int)r.p.width, b0 = 1536 * (int)r.tx + 16 * w, nin = rb - b0;
	if (!EDGE || nin >= 16) return fetch(R + b0, 0, 16);
	uint4 v = nin > 0 ? fetch(R + b0, 0, nin) : make_uint4(0, 0, 0, 0);
	const uint32_t px = fetch(R + rb - 3, 0, 3).x;                     /* B, G, R of the last pixel */
	const int r0 = b0 % 3;                                             /* padded column b0 + j holds component (r0 + j) % 3 */
	uint32_t o[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
	for (int j = 0; j < 16; j++) {
		int c = r0 + j % 3;
		c -= c >= 3 ? 3 : 0;
		const uint32_t byte = (px >> (8 * c)) & 0xFF, sh = 8 * (j & 3);
		if (j >= nin) o[j >> 2] = (o[j >> 2] & ~(0xFFu << sh)) | (byte << sh);
	}
	return make_uint4(o[0], o[1], o[2], o[3]);
}

template <bool EDGE>
__device__ __forceinline__ void pad_band(const TileRef &r, uint4 *__restrict__ dst, int band)
{
	constexpr int WORDS = TP_ROWS * TP_WORDS, PER = WORDS / TP_THREADS, GROUP = 4;
	static_assert(WORDS % TP_THREADS == 0 && PER % GROUP == 0, "band layout");
#pragma unroll
	for (int g = 0; g < PER; g += GROUP) {
		uint4 v[GROUP];
#pragma unroll
		for (int k = 0; k < GROUP; k++) {
			const int i = (g + k) * TP_THREADS + threadIdx.x;
			v[k] = pad_word<EDGE>(r, band * TP_ROWS + i / TP_WORDS, i % TP_WORDS);
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
 * slots a row. */
template <int ROW>
__device__ __forceinline__ void copy_rows(uintptr_t src, uintptr_t dst, uint64_t pitch, int seg, uint32_t rows)
{
	const uint32_t slots = (uint32_t)(seg + 30) / 16, total = rows * slots;   /* 2 .. 97 words cover seg bytes at any phase */
	const uint32_t rcp = 0xFFFFFFFFu / slots + 1;                         /* i / slots = umulhi(i, rcp) for i < 2^32 / slots */
	for (uint32_t i = threadIdx.x; i < total; i += TP_THREADS) {
		const uint32_t q = __umulhi(i, rcp), k = i - q * slots;            /* row q of the band's wanted rows, word k of it */
		const uintptr_t D0 = dst + (uint64_t)q * pitch, D1 = D0 + seg;
		const uintptr_t A = (D0 & ~(uintptr_t)15) + 16 * (uintptr_t)k;
		if (A >= D1) continue;
		const int j = A < D0 ? (int)(D0 - A) : 0, e = A + 16 > D1 ? (int)(D1 - A) : 16;
		const uint4 v = fetch(src + (uintptr_t)q * ROW + (A - D0), j, e);   /* (A - D0 wraps below 0 for the head word: fetch reads from byte j on) */
		if (j == 0 && e == 16) *reinterpret_cast<uint4 *>(A) = v;
		else store_part(reinterpret_cast<uint8_t *>(A), v, j, e);
	}
}

/* The workgroup's band of TP_ROWS rows of the tile (ty, tx) of side T at `tile` (3 T bytes a row; T = 512, or 256 or 128: the tiles of a
 * scaled decode), into the rectangle x, y, width, height of g: tile row rr is picture row T ty + rr, wanted if
 * y <= row < y + height; of it the picture columns [c0, c1) = [max(T tx, x), min(T tx + T, x + width)) go from tile byte 3 (c0 - T tx) of
 * the row to byte 3 (c0 - x) of destination row (row - y).  A band or a tile that shares nothing with the rectangle stores nothing. */
template <int T>
__device__ __forceinline__ void crop_band(const uint8_t *tile, uint32_t ty, uint32_t tx, const nhw_region &g)
{
	constexpr int ROW = 3 * T;
	const uint32_t top = T * ty + (blockIdx.x % (T / TP_ROWS)) * TP_ROWS;   /* picture row of the band's first row */
	const uint32_t lo = top > g.y ? top : g.y, hi = top + TP_ROWS < g.y + g.height ? top + TP_ROWS : g.y + g.height;
	const uint32_t c0 = T * tx > g.x ? T * tx : g.x, c1 = T * tx + T < g.x + g.width ? T * tx + T : g.x + g.width;
	if (lo >= hi || c0 >= c1) return;
	const uintptr_t src = (uintptr_t)tile + (uintptr_t)(lo - T * ty) * ROW + 3 * (c0 - T * tx);
	const uintptr_t dst = (uintptr_t)(g.addr + (uint64_t)(lo - g.y) * g.pitch) + 3 * (c0 - g.x);
	copy_rows<ROW>(src, dst, g.pitch, 3 * (int)(c1 - c0), hi - lo);      /* 3 .. 3 T bytes a row */
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
 * window's selection or a descriptor that is no window of a picture stores nothing. */
template <int T>
__global__ __launch_bounds__(TP_THREADS) void k_untile_window(const uint8_t *__restrict__ tiles, const nhw_region *__restrict__ regs, int n_regs,
                                                               const nhw_window_use *__restrict__ uses, int tile0, int m)
{
	const nhw_window_use u = uses[blockIdx.x / (T / TP_ROWS)];
	if (u.region >= (uint32_t)n_regs || u.slot < (uint32_t)tile0 || u.slot - (uint32_t)tile0 >= (uint32_t)m) return;
	const nhw_region g = regs[u.region];
	if (!rect_of_picture<T>(g)) return;
	if (u.tx < g.x / T || u.tx > (g.x + g.width - 1) / T || u.ty < g.y / T || u.ty > (g.y + g.height - 1) / T) return;   /* not a tile of the window's selection */
	crop_band<T>(tiles + (size_t)(u.slot - (uint32_t)tile0) * (size_t)(3 * T * T), u.ty, u.tx, g);
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
 * consecutive lanes on consecutive 3-byte pieces, never a byte outside the row) and three element stores -- in CHW consecutive lanes on consecutive
 * elements of a plane, in HWC 3 elements apart.  Pictures and tensors have no alignment to build wider stores on (W is any number). */
template <int DT, int CHW>
__global__ __launch_bounds__(TP_THREADS) void k_bytes_to_tensor(const nhw_picture *__restrict__ pics, int per, NhwTensorArgs a, const uint64_t *__restrict__ out_addr)
{
	using E = typename std::conditional<DT == NHW_T_U8, uint8_t, typename std::conditional<DT == NHW_T_F32, uint32_t, uint16_t>::type>::type;
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
			const uint32_t b0 = src[3 * c], b1 = src[3 * c + 1], b2 = src[3 * c + 2];
			const E e0 = (E)nhw_tensor_elem<DT>(a.rgb ? b2 : b0, a.scale[0], a.bias[0]);
			const E e1 = (E)nhw_tensor_elem<DT>(b1, a.scale[1], a.bias[1]);
			const E e2 = (E)nhw_tensor_elem<DT>(a.rgb ? b0 : b2, a.scale[2], a.bias[2]);
			if (CHW) { E *o = out + rr * W + c; o[0] = e0; o[H * W] = e1; o[2 * H * W] = e2; }
			else { E *o = out + (rr * W + c) * 3; o[0] = e0; o[1] = e1; o[2] = e2; }
		}
	}
}

/* ---- crops resized into tensors of one size ----
 * The position of output index o along an axis of source length n (1 .. 65535) and output length m (1 .. 4096): X = min(floor(128 t / m),
 * 256 (n - 1)) with t = max((2 o + 1) n - m, 0), the centre-aligned (o + 1/2) n / m - 1/2 clamped to the axis, in 1/256 pixel.  t is below
 * 2^30, so with t = q m + r the quotient is 128 q + floor(128 r / m) in 32-bit arithmetic (128 r < 2^19).  Packed as X (i0 = X >> 8 in bits
 * 8 .. 23, f = X & 255) with i1 - i0 (0 or 1) in bit 24. */
__device__ __forceinline__ uint32_t resize_pos(uint32_t o, uint32_t n, uint32_t m)
{
	const uint32_t s = (2 * o + 1) * n, t = s > m ? s - m : 0, q = t / m, r = t - q * m;
	uint32_t X = 128 * q + 128 * r / m;
	if (X > 256 * (n - 1)) X = 256 * (n - 1);
	return X | ((X >> 8) + 1 < n ? 1u << 24 : 0u);
}

/* Picture k of the table, resampled to out_w x out_h under the rule of section 18 (two taps a direction, weights in 1/256, one rounding), mirrored
 * left-right where bit 0 of flags[k] says so, to [out_h][out_w][3] or [3][out_h][out_w] elements at out_addr[k] under the value rule of
 * nhw_tensor.h.  The host knows no picture's size, so the grid is crops x bands of `rows` output rows.  A workgroup puts the positions of all
 * out_w columns and of its band's rows into LDS -- the only divisions of the kernel --, and after the one barrier walks the band 256 >> lg
 * rows at a time, 1 << lg lanes a row (the power of two that holds out_w, 256 at the most: wider rows in steps).  A thread takes one output pixel
 * at a time: twelve byte loads (any alignment and pitch; consecutive lanes on neighbouring source pixels; never a byte outside a row's 3 W),
 * the blend, and three element stores as in k_bytes_to_tensor.  An entry with a zero or oversize side, a zero address or one that is no
 * multiple of the element size stores nothing. */
constexpr int RS_MAX = 4096, RS_ROWS = 64;      /* the largest output side; the most rows a band has */
template <int DT, int CHW>
__global__ __launch_bounds__(TP_THREADS) void k_resize_to_tensor(const nhw_picture *__restrict__ pics, uint32_t out_w, uint32_t out_h, int bands, int rows, int lg,
                                                                  NhwTensorArgs a, const uint8_t *__restrict__ flags, const uint64_t *__restrict__ out_addr)
{
	using E = typename std::conditional<DT == NHW_T_U8, uint8_t, typename std::conditional<DT == NHW_T_F32, uint32_t, uint16_t>::type>::type;
	__shared__ uint32_t col_pos[RS_MAX], row_pos[RS_ROWS];
	const int k = blockIdx.x / bands;
	const uint32_t r0 = (uint32_t)(blockIdx.x % bands) * (uint32_t)rows;     /* the band: output rows [r0, r0 + nr) */
	const nhw_picture p = pics[k];
	const uint64_t oa = out_addr[k];
	if (!p.width || !p.height || p.width > 65535u || p.height > 65535u || !oa || (oa & (sizeof(E) - 1))) return;
	if (out_w > (uint32_t)RS_MAX || rows > RS_ROWS || r0 >= out_h) return;     /* (the launcher sends neither) */
	const uint32_t nr = out_h - r0 < (uint32_t)rows ? out_h - r0 : (uint32_t)rows;
	const bool mirror = flags && (flags[k] & 1);
	for (uint32_t o = threadIdx.x; o < out_w; o += TP_THREADS) col_pos[o] = resize_pos(o, p.width, out_w);
	if (threadIdx.x < nr) row_pos[threadIdx.x] = resize_pos(r0 + threadIdx.x, p.height, out_h);
	__syncthreads();
	E *out = reinterpret_cast<E *>(oa);
	const size_t W = out_w, H = out_h;
	for (uint32_t r = threadIdx.x >> lg; r < nr; r += TP_THREADS >> lg) {
		const uint32_t py = row_pos[r], fy = py & 255u;
		const uint8_t *s0 = reinterpret_cast<const uint8_t *>(p.addr + (uint64_t)((py >> 8) & 0xFFFFu) * p.pitch);
		const uint8_t *s1 = s0 + (uint64_t)(py >> 24) * p.pitch;
		const size_t rr = a.flip ? H - 1 - (r0 + r) : r0 + r;
		for (uint32_t c = threadIdx.x & ((1u << lg) - 1); c < out_w; c += 1u << lg) {
			const uint32_t px = col_pos[mirror ? out_w - 1 - c : c], fx = px & 255u, x0 = 3 * ((px >> 8) & 0xFFFFu), x1 = x0 + 3 * (px >> 24);
			const uint32_t w00 = (256 - fx) * (256 - fy), w01 = fx * (256 - fy), w10 = (256 - fx) * fy, w11 = fx * fy;
			uint32_t b[3];
#pragma unroll
			for (int ch = 0; ch < 3; ch++)
				b[ch] = (w00 * s0[x0 + ch] + w01 * s0[x1 + ch] + w10 * s1[x0 + ch] + w11 * s1[x1 + ch] + 32768u) >> 16;
			const E e0 = (E)nhw_tensor_elem<DT>(a.rgb ? b[2] : b[0], a.scale[0], a.bias[0]);
			const E e1 = (E)nhw_tensor_elem<DT>(b[1], a.scale[1], a.bias[1]);
			const E e2 = (E)nhw_tensor_elem<DT>(a.rgb ? b[0] : b[2], a.scale[2], a.bias[2]);
			if (CHW) { E *o = out + rr * W + c; o[0] = e0; o[H * W] = e1; o[2 * H * W] = e2; }
			else { E *o = out + (rr * W + c) * 3; o[0] = e0; o[1] = e1; o[2] = e2; }
		}
	}
}

/* ---- the area filter: k_resize_to_tensor's rule where an axis does not shrink, the exact box mean where it does ----
 * The taps of output index o along an axis of source length n and output length m, as a run: source pixels first .. first + count - 1, the
 * first with weight wf, the last (count > 1) with wl, those between with m.  m >= n: section 18's two taps, 256 - f and f (one tap of 256
 * where i1 = i0; the axis total is 256).  m < n: in units of 1 / m pixel output o covers [o n, (o + 1) n) and source pixel i [i m, (i + 1) m):
 * first = floor(o n / m), the last pixel ceil((o + 1) n / m) - 1, each weight the overlap (the total is n).  n <= 128 m (the caller's check)
 * makes count at most 129 and (o + 1) n at most 4096 x 65535 < 2^28.  Packed as first | count << 16 and wf | wl << 16 (both at most 4096). */
__device__ __forceinline__ uint2 area_taps(uint32_t o, uint32_t n, uint32_t m)
{
	if (m >= n) {
		const uint32_t p = resize_pos(o, n, m), f = p & 255u, two = p >> 24;
		return make_uint2(((p >> 8) & 0xFFFFu) | (1u + two) << 16, (two ? 256u - f : 256u) | f << 16);
	}
	const uint32_t lo = o * n, hi = lo + n, first = lo / m, last = (hi + m - 1) / m - 1;
	const uint32_t wf = ((first + 1) * m < hi ? (first + 1) * m : hi) - lo;
	return make_uint2(first | (last - first + 1) << 16, wf | (hi - last * m) << 16);
}

/* sum of weight x byte over the run of x taps t (area_taps) of the row at s, a channel at a time: wf first + m (those between) + wl last;
 * at most 255 x the axis total, below 2^24 */
__device__ __forceinline__ void area_row(const uint8_t *__restrict__ s, uint2 t, uint32_t m, uint32_t *r)
{
	const uint32_t cnt = t.x >> 16, wf = t.y & 0xFFFFu, wl = t.y >> 16;
	const uint8_t *q = s + 3 * (t.x & 0xFFFFu);
	uint32_t mid[3] = { 0, 0, 0 };
	for (uint32_t i = 1; i + 1 < cnt; i++) { mid[0] += q[3 * i]; mid[1] += q[3 * i + 1]; mid[2] += q[3 * i + 2]; }
#pragma unroll
	for (int ch = 0; ch < 3; ch++) r[ch] = wf * q[ch] + m * mid[ch];
	if (cnt > 1) {
#pragma unroll
		for (int ch = 0; ch < 3; ch++) r[ch] += wl * q[3 * (cnt - 1) + ch];
	}
}

/* floor((2 S + D) / (2 D)) for S <= 255 D, D < 2^32: the quotient is at most 255, so the float estimate (three roundings of 2^-24 each on a
 * value below 256) is off by less than 1 and one 64-bit multiply-and-compare each way makes it exact */
__device__ __forceinline__ uint32_t area_mean(uint64_t S, uint64_t D)
{
	const uint64_t N = 2 * S + D, D2 = 2 * D;
	uint32_t q = (uint32_t)((float)N / (float)D2);
	if ((uint64_t)q * D2 > N) q--;
	else if ((uint64_t)(q + 1) * D2 <= N) q++;
	return q;
}

/* k_resize_to_tensor with the taps of area_taps: the same table, formats, flags, grid (entries x bands of `rows` output rows) and walk -- a
 * thread one output pixel at a time, 1 << lg lanes a row.  The tap runs of all out_w columns and of the band's rows go into LDS (out_w + rows
 * entries of 8 bytes, sized by the launch) before the one barrier; they hold the kernel's only integer divisions.  A pixel then reads its
 * rows x columns source bytes once (byte loads, any alignment and pitch, never a byte outside a row's 3 W; neighbouring lanes on neighbouring
 * runs): every row gives three 32-bit sums (area_row), the rows between the first and the last add up in 32 bits as well (127 x 2^24 < 2^31),
 * and only the three products with the row weights and the division are 64 bits wide.  The loops run `count` times, at most 129: an entry
 * beyond the reduction limit on either axis stores nothing, like one with a zero or oversize side, a zero address or one that is no multiple
 * of the element size. */
template <int DT, int CHW>
__global__ __launch_bounds__(TP_THREADS) void k_area_to_tensor(const nhw_picture *__restrict__ pics, uint32_t out_w, uint32_t out_h, int bands, int rows, int lg,
                                                                NhwTensorArgs a, const uint8_t *__restrict__ flags, const uint64_t *__restrict__ out_addr)
{
	using E = typename std::conditional<DT == NHW_T_U8, uint8_t, typename std::conditional<DT == NHW_T_F32, uint32_t, uint16_t>::type>::type;
	extern __shared__ uint2 area_tab[];                                    /* [out_w] columns, then [rows] rows */
	const int k = blockIdx.x / bands;
	const uint32_t r0 = (uint32_t)(blockIdx.x % bands) * (uint32_t)rows;     /* the band: output rows [r0, r0 + nr) */
	const nhw_picture p = pics[k];
	const uint64_t oa = out_addr[k];
	if (!p.width || !p.height || p.width > 65535u || p.height > 65535u || !oa || (oa & (sizeof(E) - 1))) return;
	if (out_w > (uint32_t)RS_MAX || out_h > (uint32_t)RS_MAX || rows > RS_ROWS || r0 >= out_h) return;   /* (the launcher sends neither) */
	if (p.width > NHW_AREA_MAX_REDUCTION * out_w || p.height > NHW_AREA_MAX_REDUCTION * out_h) return;
	const uint32_t nr = out_h - r0 < (uint32_t)rows ? out_h - r0 : (uint32_t)rows;
	const bool mirror = flags && (flags[k] & 1);
	uint2 *col_tap = area_tab, *row_tap = area_tab + out_w;
	for (uint32_t o = threadIdx.x; o < out_w; o += TP_THREADS) col_tap[o] = area_taps(o, p.width, out_w);
	if (threadIdx.x < nr) row_tap[threadIdx.x] = area_taps(r0 + threadIdx.x, p.height, out_h);
	__syncthreads();
	E *out = reinterpret_cast<E *>(oa);
	const size_t W = out_w, H = out_h;
	const uint64_t D = (uint64_t)(out_w >= p.width ? 256u : p.width) * (out_h >= p.height ? 256u : p.height);
	for (uint32_t r = threadIdx.x >> lg; r < nr; r += TP_THREADS >> lg) {
		const uint2 ty = row_tap[r];
		const uint32_t cy = ty.x >> 16;
		const uint8_t *s = reinterpret_cast<const uint8_t *>(p.addr + (uint64_t)(ty.x & 0xFFFFu) * p.pitch);
		const size_t rr = a.flip ? H - 1 - (r0 + r) : r0 + r;
		for (uint32_t c = threadIdx.x & ((1u << lg) - 1); c < out_w; c += 1u << lg) {
			const uint2 tx = col_tap[mirror ? out_w - 1 - c : c];
			uint32_t first[3], last[3] = { 0, 0, 0 }, mid[3] = { 0, 0, 0 }, b[3];
			area_row(s, tx, out_w, first);
			for (uint32_t i = 1; i + 1 < cy; i++) {
				uint32_t v[3];
				area_row(s + (uint64_t)i * p.pitch, tx, out_w, v);
				mid[0] += v[0]; mid[1] += v[1]; mid[2] += v[2];
			}
			if (cy > 1) area_row(s + (uint64_t)(cy - 1) * p.pitch, tx, out_w, last);
#pragma unroll
			for (int ch = 0; ch < 3; ch++)
				b[ch] = area_mean((uint64_t)(ty.y & 0xFFFFu) * first[ch] + (uint64_t)out_h * mid[ch] + (uint64_t)(ty.y >> 16) * last[ch], D);
			const E e0 = (E)nhw_tensor_elem<DT>(a.rgb ? b[2] : b[0], a.scale[0], a.bias[0]);
			const E e1 = (E)nhw_tensor_elem<DT>(b[1], a.scale[1], a.bias[1]);
			const E e2 = (E)nhw_tensor_elem<DT>(a.rgb ? b[0] : b[2], a.scale[2], a.bias[2]);
			if (CHW) { E *o = out + rr * W + c; o[0] = e0; o[H * W] = e1; o[2 * H * W] = e2; }
			else { E *o = out + (rr * W + c) * 3; o[0] = e0; o[1] = e1; o[2] = e2; }
		}
	}
}

/* ---- the cubic filter: the Keys cubic with a = -1/2, its support widened with the reduction, in integers ----
 * An axis of source length n (1 .. 65535) and output length m (1 .. 4096), n <= 32 m, D = max(n, m).  Source pixel i is at N = (2 i + 1) m -
 * (2 o + 1) n from output index o (2 m times the distance of the centres) and at U = floor((1024 |N| + D) / (2 D)) in 1/1024 of the kernel's
 * unit; the taps of o are the i in 0 .. n - 1 with U < 2048, which is |N| <= L = floor((4095 D - 1) / 1024): one run, from ceil((c - L - m) /
 * 2 m) to floor((c + L - m) / 2 m) with c = (2 o + 1) n, cut at the axis' ends.  c < 2^30 and L < 2^18, so all of it is 32-bit; L >= 3 D >= m
 * keeps the upper numerator positive, and the pixel nearest the output's centre has |N| <= m <= L: no run is empty.  The N of a run are 2 m
 * apart inside an interval shorter than 8 D: at most floor(4 D / m) + 1 taps, 129 under the limit.  Packed as first | count << 16. */
constexpr int CB_HP = 4096;                     /* pixels of the horizontal pass a workgroup holds (three int16 each) */
constexpr int CB_W = 2048;                      /* weights of a chunk of columns; of a chunk of rows */
constexpr int CB_COLS = 256;                    /* the most columns a chunk has: a thread each when their weights are made */
constexpr int CB_RUNS = 4;                      /* the source rows of a pass hold this many of the longest runs at least */
__device__ __forceinline__ uint32_t cubic_reach(uint32_t D) { return (4095u * D - 1u) >> 10; }
__device__ __forceinline__ uint32_t cubic_run(uint32_t o, uint32_t n, uint32_t m, uint32_t L)
{
	const int32_t c = (int32_t)((2 * o + 1) * n), a = c + (int32_t)m - 1 - (int32_t)L;
	const uint32_t lo = a > 0 ? (uint32_t)a / (2 * m) : 0u;
	uint32_t hi = (uint32_t)(c + (int32_t)L - (int32_t)m) / (2 * m);
	if (hi > n - 1) hi = n - 1;
	return lo | (hi >= lo ? hi - lo + 1 : 0u) << 16;
}

/* the Keys cubic times 2^31 at U < 2048, exact: 2^31 at 0, 0 at 1024, negative beyond */
__device__ __forceinline__ int64_t cubic_raw(uint32_t U)
{
	const int64_t u = (int64_t)U;
	if (U <= 1024u) return 3 * u * u * u - 5120 * u * u + (1ll << 31);
	return -u * u * u + 5120 * u * u - (8ll << 20) * u + (1ll << 32);
}
__device__ __forceinline__ int64_t cubic_tap(uint32_t i, int32_t c, uint32_t m, uint32_t D)
{
	const int32_t N = (int32_t)((2 * i + 1) * m) - c;
	return cubic_raw((1024u * (uint32_t)(N < 0 ? -N : N) + D) / (2 * D));     /* 1024 |N| + D < 4 x 1024 D + D < 2^29 */
}

/* The weights of the run `run` of output index o into w[0 .. count): q = floor((2^15 r + R) / (2 R)) with R the run's sum of r (positive), then
 * 2^14 - sum q onto the largest q (the first of equals).  The quotient lies inside +-2^15 (the tests bound sum |q|), so the float estimate --
 * three roundings of 2^-24 each -- is off by less than 1 and one 64-bit multiply-and-compare each way makes it the floor, also below zero.
 * `cap` is the room of w: count never exceeds it (above), and nothing is written beyond it. */
__device__ __forceinline__ void cubic_weights(int16_t *w, uint32_t o, uint32_t run, uint32_t n, uint32_t m, uint32_t D, uint32_t cap)
{
	const uint32_t first = run & 0xFFFFu, count = (run >> 16) < cap ? run >> 16 : cap;
	const int32_t c = (int32_t)((2 * o + 1) * n);
	int64_t R = 0;
	for (uint32_t k = 0; k < count; k++) R += cubic_tap(first + k, c, m, D);
	if (R <= 0) { for (uint32_t k = 0; k < count; k++) w[k] = 0; return; }   /* (no run of the rule) */
	const int64_t den = 2 * R;
	int32_t sum = 0, best = -65536;
	uint32_t at = 0;
	for (uint32_t k = 0; k < count; k++) {
		const int64_t num = cubic_tap(first + k, c, m, D) * 32768 + R;
		int32_t q = (int32_t)floorf((float)num / (float)den);
		if ((int64_t)q * den > num) q--;
		else if ((int64_t)(q + 1) * den <= num) q++;
		w[k] = (int16_t)q;
		sum += q;
		if (q > best) { best = q; at = k; }
	}
	if (count) w[at] = (int16_t)(w[at] + (16384 - sum));
}

/* k_resize_to_tensor under the cubic rule: the same table, formats, flags and grid (entries x bands of `rows` output rows).  The rule is
 * separable and fixes the rounding between the passes, so the kernel is: H[y][ox] = (sum_x qx P[y][x] + 128) >> 8 for the source rows a group
 * of output rows needs, as int16 in LDS, then byte = clamp((sum_y qy H[y][ox] + 2^19) >> 20) from there -- Tx + Ty multiply-adds a pixel where
 * the direct form has Tx Ty.  The host knows no source size, so the LDS is fixed: CB_HP pixels of H (24 576 bytes), CB_W int16 weights for a
 * chunk of columns and as many for a chunk of rows (8192), the runs of a chunk's columns and of the band's rows (1280): 34 048 bytes, four
 * workgroups a CU.  The workgroup cuts its band itself, uniformly, from sizes it has checked: tb = floor(4 D / m) + 1 bounds an axis' runs;
 * the weights of wc = min(out_w, CB_COLS, CB_W / tbx) columns are held at a time (all of them for a 224-wide output below a reduction of 2);
 * a pass takes cc = min(wc, CB_HP / (CB_RUNS tby)) of them, so that CB_HP / cc source rows (CB_RUNS runs at least) fit; a chunk of rows grows
 * while its weights fit (CB_W / tby rows) and its source rows -- first run's first to last run's end; firsts and ends do not decrease with
 * o -- fit.  Per chunk of columns: runs and weights (a thread a column); in it per chunk of rows: its weights (a thread a row), barrier; in
 * it per pass: H (a thread a source row and column at a time, byte loads, any alignment and pitch, never a byte outside a row's 3 W),
 * barrier, the vertical pass and the element stores, barrier.  Every loop bound is one of these sizes or a count clamped to its table's
 * room.  An entry beyond the reduction limit on either axis stores nothing, like one with a zero or oversize side, a zero address or one
 * that is no multiple of the element size. */
template <int DT, int CHW>
__global__ __launch_bounds__(TP_THREADS) void k_cubic_to_tensor(const nhw_picture *__restrict__ pics, uint32_t out_w, uint32_t out_h, int bands, int rows,
                                                                 NhwTensorArgs a, const uint8_t *__restrict__ flags, const uint64_t *__restrict__ out_addr)
{
	using E = typename std::conditional<DT == NHW_T_U8, uint8_t, typename std::conditional<DT == NHW_T_F32, uint32_t, uint16_t>::type>::type;
	__shared__ int16_t cb_h[3 * CB_HP], cb_wx[CB_W], cb_wy[CB_W];
	__shared__ uint32_t cb_col[CB_COLS], cb_row[RS_ROWS];
	static_assert(CB_COLS <= TP_THREADS && RS_ROWS <= TP_THREADS, "a thread a run");
	const int k = blockIdx.x / bands;
	const uint32_t r0 = (uint32_t)(blockIdx.x % bands) * (uint32_t)rows;     /* the band: output rows [r0, r0 + nr) */
	const nhw_picture p = pics[k];
	const uint64_t oa = out_addr[k];
	if (!p.width || !p.height || p.width > 65535u || p.height > 65535u || !oa || (oa & (sizeof(E) - 1))) return;
	if (!out_w || out_w > (uint32_t)RS_MAX || out_h > (uint32_t)RS_MAX || rows < 1 || rows > RS_ROWS || r0 >= out_h) return;   /* (the launcher sends neither) */
	if (p.width > NHW_CUBIC_MAX_REDUCTION * out_w || p.height > NHW_CUBIC_MAX_REDUCTION * out_h) return;
	const uint32_t nr = out_h - r0 < (uint32_t)rows ? out_h - r0 : (uint32_t)rows;
	const bool mirror = flags && (flags[k] & 1);
	const uint32_t Dx = p.width > out_w ? p.width : out_w, Dy = p.height > out_h ? p.height : out_h;
	const uint32_t tbx = 4 * Dx / out_w + 1, tby = 4 * Dy / out_h + 1;          /* 5 .. 129 */
	uint32_t wc = out_w < (uint32_t)CB_COLS ? out_w : (uint32_t)CB_COLS;        /* columns whose weights are held at a time */
	if (wc > CB_W / tbx) wc = CB_W / tbx;
	uint32_t cc = wc;                                                        /* ... and columns of a pass: 7 at the least, or out_w */
	if (cc > (uint32_t)CB_HP / (CB_RUNS * tby)) cc = (uint32_t)CB_HP / (CB_RUNS * tby);
	const uint32_t smax = CB_HP / cc, rcmax = CB_W / tby;
	uint32_t lanes = 1;
	while (lanes < cc) lanes <<= 1;                                          /* lanes a row of a pass: 1 .. 256 */
	if (threadIdx.x < nr) cb_row[threadIdx.x] = cubic_run(r0 + threadIdx.x, p.height, out_h, cubic_reach(Dy));
	__syncthreads();
	E *out = reinterpret_cast<E *>(oa);
	const size_t W = out_w, H = out_h;
	for (uint32_t ws = 0; ws < out_w; ws += wc) {
		const uint32_t nw = out_w - ws < wc ? out_w - ws : wc;
		if (threadIdx.x < nw) {
			const uint32_t run = cubic_run(ws + threadIdx.x, p.width, out_w, cubic_reach(Dx));
			cb_col[threadIdx.x] = run;
			cubic_weights(cb_wx + threadIdx.x * tbx, ws + threadIdx.x, run, p.width, out_w, Dx, tbx);
		}
		for (uint32_t rs = 0; rs < nr;) {
			const uint32_t ylo = cb_row[rs] & 0xFFFFu;
			uint32_t re = rs + 1;
			while (re < nr && re - rs < rcmax && (cb_row[re] & 0xFFFFu) + (cb_row[re] >> 16) - ylo <= smax) re++;
			const uint32_t span = (cb_row[re - 1] & 0xFFFFu) + (cb_row[re - 1] >> 16) - ylo;
			if (span > smax || ylo + span > p.height) return;                /* (no run of the rule: smax holds CB_RUNS of the longest) */
			if (threadIdx.x < re - rs) cubic_weights(cb_wy + threadIdx.x * tby, r0 + rs + threadIdx.x, cb_row[rs + threadIdx.x], p.height, out_h, Dy, tby);
			__syncthreads();                                                 /* the weights of the columns and of these rows are there */
			for (uint32_t cs = 0; cs < nw; cs += cc) {
				const uint32_t ncol = nw - cs < cc ? nw - cs : cc;
				for (uint32_t s = threadIdx.x / lanes; s < span; s += TP_THREADS / lanes) {
					const uint8_t *src = reinterpret_cast<const uint8_t *>(p.addr + (uint64_t)(ylo + s) * p.pitch);
					for (uint32_t j = threadIdx.x & (lanes - 1); j < ncol; j += lanes) {
						const uint32_t run = cb_col[cs + j], cnt = (run >> 16) < tbx ? run >> 16 : tbx;
						const uint8_t *q = src + 3 * (run & 0xFFFFu);
						const int16_t *wt = cb_wx + (cs + j) * tbx;
						int32_t acc[3] = { 0, 0, 0 };
						for (uint32_t i = 0; i < cnt; i++) {
							const int32_t wi = wt[i];
							acc[0] += wi * (int32_t)q[3 * i]; acc[1] += wi * (int32_t)q[3 * i + 1]; acc[2] += wi * (int32_t)q[3 * i + 2];
						}
						int16_t *hp = cb_h + 3 * (s * ncol + j);
#pragma unroll
						for (int ch = 0; ch < 3; ch++) hp[ch] = (int16_t)((acc[ch] + 128) >> 8);
					}
				}
				__syncthreads();
				for (uint32_t r = threadIdx.x / lanes; r < re - rs; r += TP_THREADS / lanes) {
					const uint32_t run = cb_row[rs + r], s0 = (run & 0xFFFFu) - ylo, cnt = (run >> 16) < tby ? run >> 16 : tby;
					const int16_t *wt = cb_wy + r * tby;
					const size_t rr = a.flip ? H - 1 - (r0 + rs + r) : r0 + rs + r;
					for (uint32_t j = threadIdx.x & (lanes - 1); j < ncol; j += lanes) {
						int32_t v[3] = { 0, 0, 0 };
						uint32_t b[3];
						for (uint32_t i = 0; i < cnt; i++) {
							const int32_t wi = wt[i];
							const int16_t *hp = cb_h + 3 * ((s0 + i) * ncol + j);
							v[0] += wi * hp[0]; v[1] += wi * hp[1]; v[2] += wi * hp[2];
						}
#pragma unroll
						for (int ch = 0; ch < 3; ch++) {
							const int32_t y = (v[ch] + (1 << 19)) >> 20;
							b[ch] = (uint32_t)(y < 0 ? 0 : y > 255 ? 255 : y);
						}
						const size_t c = mirror ? out_w - 1 - (ws + cs + j) : ws + cs + j;
						const E e0 = (E)nhw_tensor_elem<DT>(a.rgb ? b[2] : b[0], a.scale[0], a.bias[0]);
						const E e1 = (E)nhw_tensor_elem<DT>(b[1], a.scale[1], a.bias[1]);
						const E e2 = (E)nhw_tensor_elem<DT>(a.rgb ? b[0] : b[2], a.scale[2], a.bias[2]);
						if (CHW) { E *o = out + rr * W + c; o[0] = e0; o[H * W] = e1; o[2 * H * W] = e2; }
						else { E *o = out + (rr * W + c) * 3; o[0] = e0; o[1] = e1; o[2] = e2; }
					}
				}
				__syncthreads();                                             /* before H, these rows' weights or the columns' are written again */
			}
			rs = re;
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
	using E = typename std::conditional<DT == NHW_T_U8, uint8_t, typename std::conditional<DT == NHW_T_F32, uint32_t, uint16_t>::type>::type;
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

/* Bands: some 8192 workgroups in all where the crops are few, one band a crop where they are many; a band has at most RS_ROWS rows and, where
 * the output is narrow, at least the rows of one pass (256 >> lg), so that a pass has work for every lane. */
hipError_t nhw_launch_resize_to_tensor(const nhw_picture *d_pics, int n, uint32_t out_w, uint32_t out_h, int dtype, int layout, const NhwTensorArgs &a,
                                       const uint8_t *d_flags, const uint64_t *d_out_addr, hipStream_t s)
{
	if (n < 1 || n > (1 << 24) || out_w < 1 || out_h < 1 || out_w > (uint32_t)RS_MAX || out_h > (uint32_t)RS_MAX) return hipErrorInvalidValue;
	int lg = 0;
	while (lg < 8 && (1u << lg) < out_w) lg++;
	const uint32_t want = (8192u + (uint32_t)n - 1) / (uint32_t)n < out_h ? (8192u + (uint32_t)n - 1) / (uint32_t)n : out_h;   /* bands wanted: 1 .. out_h */
	uint32_t rows = (out_h + want - 1) / want;
	if (rows < (uint32_t)(TP_THREADS >> lg)) rows = TP_THREADS >> lg;
	if (rows > (uint32_t)RS_ROWS) rows = RS_ROWS;
	const int bands = (int)((out_h + rows - 1) / rows);                 /* 1 .. 4096; with n above 8192, 64 at the most: n * bands is below 2^31 */
	nhw_with_tensor_store(dtype, layout, a, [&](auto st) {
		constexpr int DT = decltype(st)::dtype, CHW = decltype(st)::layout;
		k_resize_to_tensor<DT, CHW><<<n * bands, TP_THREADS, 0, s>>>(d_pics, out_w, out_h, bands, (int)rows, lg, a, d_flags, d_out_addr);
	});
	return hipGetLastError();
}

/* The area filter: the bands of nhw_launch_resize_to_tensor (the same rule, so that both kernels meet the same launch shapes), and the LDS the
 * band's tap runs take: 8 (out_w + rows) bytes, 33 280 at the most. */
hipError_t nhw_launch_area_to_tensor(const nhw_picture *d_pics, int n, uint32_t out_w, uint32_t out_h, int dtype, int layout, const NhwTensorArgs &a,
                                     const uint8_t *d_flags, const uint64_t *d_out_addr, hipStream_t s)
{
	if (n < 1 || n > (1 << 24) || out_w < 1 || out_h < 1 || out_w > (uint32_t)RS_MAX || out_h > (uint32_t)RS_MAX) return hipErrorInvalidValue;
	int lg = 0;
	while (lg < 8 && (1u << lg) < out_w) lg++;
	const uint32_t want = (8192u + (uint32_t)n - 1) / (uint32_t)n < out_h ? (8192u + (uint32_t)n - 1) / (uint32_t)n : out_h;   /* bands wanted: 1 .. out_h */
	uint32_t rows = (out_h + want - 1) / want;
	if (rows < (uint32_t)(TP_THREADS >> lg)) rows = TP_THREADS >> lg;
	if (rows > (uint32_t)RS_ROWS) rows = RS_ROWS;
	const int bands = (int)((out_h + rows - 1) / rows);                 /* 1 .. 4096; with n above 8192, 64 at the most: n * bands is below 2^31 */
	const size_t lds = sizeof(uint2) * ((size_t)out_w + rows);
	nhw_with_tensor_store(dtype, layout, a, [&](auto st) {
		constexpr int DT = decltype(st)::dtype, CHW = decltype(st)::layout;
		k_area_to_tensor<DT, CHW><<<n * bands, TP_THREADS, lds, s>>>(d_pics, out_w, out_h, bands, (int)rows, lg, a, d_flags, d_out_addr);
	});
	return hipGetLastError();
}

/* The cubic filter: the bands of nhw_launch_resize_to_tensor again; the kernel's LDS is static and it cuts its band itself */
hipError_t nhw_launch_cubic_to_tensor(const nhw_picture *d_pics, int n, uint32_t out_w, uint32_t out_h, int dtype, int layout, const NhwTensorArgs &a,
                                      const uint8_t *d_flags, const uint64_t *d_out_addr, hipStream_t s)
{
	if (n < 1 || n > (1 << 24) || out_w < 1 || out_h < 1 || out_w > (uint32_t)RS_MAX || out_h > (uint32_t)RS_MAX) return hipErrorInvalidValue;
	int lg = 0;
	while (lg < 8 && (1u << lg) < out_w) lg++;
	const uint32_t want = (8192u + (uint32_t)n - 1) / (uint32_t)n < out_h ? (8192u + (uint32_t)n - 1) / (uint32_t)n : out_h;   /* bands wanted: 1 .. out_h */
	uint32_t rows = (out_h + want - 1) / want;
	if (rows < (uint32_t)(TP_THREADS >> lg)) rows = TP_THREADS >> lg;
	if (rows > (uint32_t)RS_ROWS) rows = RS_ROWS;
	const int bands = (int)((out_h + rows - 1) / rows);                 /* 1 .. 4096; with n above 8192, 64 at the most: n * bands is below 2^31 */
	nhw_with_tensor_store(dtype, layout, a, [&](auto st) {
		constexpr int DT = decltype(st)::dtype, CHW = decltype(st)::layout;
		k_cubic_to_tensor<DT, CHW><<<n * bands, TP_THREADS, 0, s>>>(d_pics, out_w, out_h, bands, (int)rows, a, d_flags, d_out_addr);
	});
	return hipGetLastError();
}

hipError_t nhw_launch_tile_pad(const nhw_picture *d_pics, int n_pics, int tile0, int m, uint8_t *d_tiles, hipStream_t s)
{
	k_tile_pad<<<m * TP_BANDS, TP_THREADS, 0, s>>>(d_pics, n_pics, tile0, d_tiles);
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

hipError_t nhw_launch_sse_crop(const uint8_t *d_tiles, const nhw_picture *d_pics, int n_pics, int tile0, int m, uint64_t *d_sse, hipStream_t s)
{
	k_sse_crop<<<m * TP_BANDS, TP_THREADS, 0, s>>>(d_tiles, d_pics, n_pics, tile0, reinterpret_cast<unsigned long long *>(d_sse));
	return hipGetLastError();
}

/* ------------------------------------------------------------------------------------------------ the .nhwp container (host) */
static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static void wr32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

extern "C" int nhw_picture_tiles(uint32_t width, uint32_t height)
{
	if (width < 1 || width > 65535 || height < 1 || height > 65535) return NHW_E_ARG;
	return (int)(((width + 511) / 512) * ((height + 511) / 512));
}

/* a W x H picture decoded at scale s is ceil(W / s) x ceil(H / s); its tile count does not change */
extern "C" int nhw_picture_scaled_size(uint32_t width, uint32_t height, int scale, uint32_t *scaled_width, uint32_t *scaled_height)
{
	if (nhw_picture_tiles(width, height) < 1 || (scale != 1 && scale != 2 && scale != 4) || !scaled_width || !scaled_height) return NHW_E_ARG;
	*scaled_width = (width + (uint32_t)scale - 1) / (uint32_t)scale;
	*scaled_height = (height + (uint32_t)scale - 1) / (uint32_t)scale;
	return NHW_OK;
}

/* the tiles a region x, y, w, h of a W x H picture selects: columns x / 512 .. (x + w - 1) / 512 times rows y / 512 .. (y + h - 1) / 512 */
extern "C" int nhw_region_tiles(uint32_t pic_width, uint32_t pic_height, uint32_t x, uint32_t y, uint32_t width, uint32_t height)
{
	if (nhw_picture_tiles(pic_width, pic_height) < 1 || width < 1 || height < 1) return NHW_E_ARG;
	if ((uint64_t)x + width > pic_width || (uint64_t)y + height > pic_height) return NHW_E_ARG;
	return (int)(((x + width - 1) / 512 - x / 512 + 1) * ((y + height - 1) / 512 - y / 512 + 1));
}

/* the tiles a window x, y, w, h of the picture at scale s selects: the rectangle is in the coordinates of the scaled
 * picture ceil(W / s) x ceil(H / s), whose tiles have the side T = 512 / s; at scale 1 it is nhw_region_tiles */
extern "C" int nhw_window_tiles(uint32_t pic_width, uint32_t pic_height, int scale, uint32_t x, uint32_t y, uint32_t width, uint32_t height)
{
	uint32_t sw = 0, sh = 0;
	if (nhw_picture_scaled_size(pic_width, pic_height, scale, &sw, &sh) != NHW_OK || width < 1 || height < 1) return NHW_E_ARG;
	if ((uint64_t)x + width > sw || (uint64_t)y + height > sh) return NHW_E_ARG;
	const uint32_t T = 512u / (uint32_t)scale;
	return (int)(((x + width - 1) / T - x / T + 1) * ((y + height - 1) / T - y / T + 1));
}

/* the scale to decode a width x height crop at that goes to out_width x out_height: the largest s of 4, 2, 1 with
 * s out_width <= width and s out_height <= height, so that what is left to the two-tap resize is a reduction below 2; 1 if there is none */
extern "C" int nhw_crop_scale(uint32_t width, uint32_t height, uint32_t out_width, uint32_t out_height)
{
	if (!width || !height || !out_width || !out_height || out_width > 4096u || out_height > 4096u) return NHW_E_ARG;
	for (uint32_t s = 4; s > 1; s >>= 1)
		if (s * out_width <= width && s * out_height <= height) return (int)s;
	return 1;
}

/* A well-formed container: magic, version 1, zero reserved bytes, W and H in 1..65535, T = nhw_picture_tiles(W, H) lengths of 1 ..
 * NHW_OUT_STRIDE each, and exactly 16 + 4 T + the sum of them bytes.  Returns NHW_OK with W, H, T and a pointer to the directory. */
int nhw_container_parse(const uint8_t *c, size_t len, uint32_t *width, uint32_t *height, int *tiles, const uint8_t **dir)
{
	if (!c || len < 16 || memcmp(c, "NHWP", 4) || c[4] != 1 || c[5] || c[6] || c[7]) return NHW_E_FORMAT;
	const uint32_t w = rd32(c + 8), h = rd32(c + 12);
	const int t = nhw_picture_tiles(w, h);
	if (t < 1 || (len - 16) / 4 < (size_t)t) return NHW_E_FORMAT;
	uint64_t total = 16 + 4 * (uint64_t)t;
	for (int i = 0; i < t; i++) {
		const uint32_t l = rd32(c + 16 + 4 * (size_t)i);
		if (l < 1 || l > NHW_OUT_STRIDE) return NHW_E_FORMAT;
		total += l;
	}
	if (total != len) return NHW_E_FORMAT;
	*width = w; *height = h; *tiles = t; *dir = c + 16;
	return NHW_OK;
}

/* header and directory of a container for a W x H picture whose T tile files have the lengths lens[]; returns 16 + 4 T (the files go
 * behind, back to back) */
size_t nhw_container_head(uint8_t *dst, uint32_t width, uint32_t height, const uint32_t *lens, int t)
{
	memcpy(dst, "NHWP\1\0\0\0", 8);
	wr32(dst + 8, width); wr32(dst + 12, height);
	for (int i = 0; i < t; i++) wr32(dst + 16 + 4 * (size_t)i, lens[i]);
	return 16 + 4 * (size_t)t;
}

extern "C" int nhw_picture_info(const uint8_t *container, size_t len, uint32_t *width, uint32_t *height)
{
	uint32_t w = 0, h = 0;
	int t = 0;
	const uint8_t *dir = nullptr;
	const int rc = nhw_container_parse(container, len, &w, &h, &t, &dir);
	if (rc != NHW_OK) return rc;
	if (width) *width = w;
	if (height) *height = h;
	return NHW_OK;
}
