/*
 * nhw_resample.hip -- pictures resampled into tensors of one size (DESIGN.md sections 18 to 20): the two-tap kernel k_resize_to_tensor, the
 * area filter k_area_to_tensor and the cubic filter k_cubic_to_tensor, and the axis helpers of each; pictures sampled along a tilted grid
 * (section 21): the affine warp k_warp_to_tensor; and the one launcher of all four, nhw_launch_sample, which takes a call as one record
 * (NhwSampleCall, nhw_tensor.h) and finds its kernel: the form (dtype, layout, bytes a pixel), the pack of its tables, the band rule, the filter.
 *
 * The three kernels have one shape.  The table (nhw_picture entries, addr, pitch, width and height read), the flags and the tensors'
 * addresses live in device memory, so the host knows no picture's size: the grid is entries x bands of `rows` output rows, cut by the one
 * band rule of the launcher.  A workgroup learns its entry and its band from resample_entry, which passes over an entry that stores nothing;
 * it puts what the axes need into LDS (the kernel's only integer divisions), and a thread then makes one output pixel at a time as three
 * bytes B, G, R, which nhw_store_pixel (nhw_tensor.h) stores under the format's value rule, channel order and layout.  Pictures have any
 * alignment and pitch and tensors any width: the loads are byte loads that never touch a byte outside a row's 3 W, the stores single elements.
 *
 * Each kernel has the bytes a pixel, C, as its last template parameter.  C = 3 is the colour form described here, and
 * what a kernel's name means without it.  C = 1 is the one-channel form, k_*_to_tensor<DT, 0, 1>: pictures of 1 byte a pixel (pitch >= W), the
 * same positions, taps, weights, roundings, limits and mirror on the one channel, one element a pixel under scale[0] and bias[0]; the layout
 * parameter means nothing there and is 0.
 *
 * Each kernel has a mapped form as well: its template parameters end in a pack M, empty in the forms above, and its
 * arguments in `M... maps`, which is then nothing at all -- those forms have the arguments, registers and instructions they had before the pack.
 * With M = const nhw_colour_map * the workgroup reads its entry's map once (EntryMap), stores nothing unless the map is within the limits, and puts
 * every pixel's bytes through nhw_colour_apply (nhw_colour.h) between the blend and resample_store.
 *
 * ... and a toned form: M = const nhw_colour_map *, const nhw_tone_table *.  The map pointer may be null -- a kernel argument, so
 * the branch is uniform -- and the workgroup then skips the map.  It copies its entry's table, 256 C bytes, into LDS (EntryMap::stage) once it has
 * accepted the entry and the map, in front of the kernel's first barrier (the warp kernel, which has none otherwise, gains one: EntryMap::barrier), and
 * a pixel's bytes take C byte reads from there behind the map.
 */
#include "nhw_tensor.h"
#include "nhw_colour.h"
#include "nhw_tone.h"
#include "../../include/nhw_hip_debug.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_MAX = 4096, RS_ROWS = 64;      /* the largest output side; the most rows a band has */

/* What a workgroup of the three kernels does first: its entry k = blockIdx.x / bands of the table and its band, the output rows [r0, r0 + nr),
 * with the entry's picture p, its tensor `out` and whether it is mirrored left-right (bit 0 of flags[k]; flags may be null).  False for an
 * entry that stores nothing: one with a zero or oversize side, a zero address or one that is no multiple of the element size, and, with a
 * filter's reduction limit (`limit`: 0 for the two-tap kernel, which has none), one beyond it on either axis.  False as well for what
 * nhw_launch_sample refuses before it launches -- an output side of 0 or above RS_MAX, a band of no rows or of more than RS_ROWS, a band
 * below the output -- so that no kernel depends on its launcher for the room of its tables. */
template <int DT>
__device__ __forceinline__ bool resample_entry_at(const nhw_picture *__restrict__ pics, const uint8_t *__restrict__ flags, const uint64_t *__restrict__ out_addr, uint32_t out_w,
                                                  uint32_t out_h, int bands, int rows, uint32_t limit, nhw_picture &p, typename NhwElem<DT>::type *&out, uint32_t &r0, uint32_t &nr,
                                                  bool &mirror, int &k)
{
	using E = typename NhwElem<DT>::type;
	k = blockIdx.x / bands;
	const uint32_t first = (uint32_t)(blockIdx.x % bands) * (uint32_t)rows;
	const nhw_picture q = pics[k];
	const uint64_t oa = out_addr[k];
	if (!q.width || !q.height || q.width > 65535u || q.height > 65535u || !oa || (oa & (sizeof(E) - 1))) return false;
	if (!out_w || out_w > (uint32_t)RS_MAX || out_h > (uint32_t)RS_MAX || rows < 1 || rows > RS_ROWS || first >= out_h) return false;
	if (limit && (q.width > limit * out_w || q.height > limit * out_h)) return false;
	p = q;
	r0 = first;
	nr = out_h - first < (uint32_t)rows ? out_h - first : (uint32_t)rows;
	mirror = flags && (flags[k] & 1);
	out = reinterpret_cast<E *>(oa);
	return true;
}
/* ... as the three resamplers call it; resample_entry_at hands the entry's index back as well, for a kernel with a table of its own (the warp) */
template <int DT>
__device__ __forceinline__ bool resample_entry(const nhw_picture *__restrict__ pics, const uint8_t *__restrict__ flags, const uint64_t *__restrict__ out_addr, uint32_t out_w,
                                               uint32_t out_h, int bands, int rows, uint32_t limit, nhw_picture &p, typename NhwElem<DT>::type *&out, uint32_t &r0, uint32_t &nr,
                                               bool &mirror)
{
	int k;
	return resample_entry_at<DT>(pics, flags, out_addr, out_w, out_h, bands, rows, limit, p, out, r0, nr, mirror, k);
}

/* The pixel's store.  C, the bytes a source pixel has and the elements an output pixel gets, is 3 (B, G, R: nhw_store_pixel) or 1 (the one-channel
 * forms of DESIGN.md section 23: one element at out[rr w + c], the value rule with scale[0] and bias[0]; with one channel CHW and HWC are the
 * same memory, and the grey kernels have no layout). */
template <int DT, int CHW, int C>
__device__ __forceinline__ void resample_store(typename NhwElem<DT>::type *out, size_t h, size_t w, size_t rr, size_t c, const uint32_t *b, const NhwTensorArgs &a)
{
	if constexpr (C == 3) nhw_store_pixel<DT, CHW>(out, h, w, rr, c, b, a);
	else out[rr * w + c] = (typename NhwElem<DT>::type)nhw_tensor_elem<DT>(b[0], a.scale[0], a.bias[0]);
}

/* The map of a workgroup's entry, by the kernel's pack M.  No table: nothing is held, read or done, and the kernel is what
 * it is without this.  A table: maps[k], read once -- k is uniform, so are the twelve numbers --, `load` false for a map beyond the limits (the
 * entry then stores nothing), `apply` the rule on a pixel's C bytes. */
template <class... M> struct EntryMap {
	__device__ __forceinline__ bool load(int, M...) { return true; }
	template <int C> __device__ __forceinline__ void stage() const {}
	__device__ __forceinline__ void barrier() const {}
	template <int C> __device__ __forceinline__ void apply(uint32_t *) const {}
};
template <> struct EntryMap<const nhw_colour_map *> {
	nhw_colour_map c;
	__device__ __forceinline__ bool load(int k, const nhw_colour_map *maps) { c = maps[k]; return nhw_colour_within(c); }
	template <int C> __device__ __forceinline__ void stage() const {}
	__device__ __forceinline__ void barrier() const {}
	template <int C> __device__ __forceinline__ void apply(uint32_t *b) const { nhw_colour_apply<C>(c, b); }
};
/* ... and the toned pack: the map, where the call has one (`mapped`: uniform for the grid), and the entry's tone table.  `stage`
 * copies the table's first 256 C bytes into LDS, a byte a thread at a time (a table has no alignment), for the whole workgroup: every thread
 * calls it, before a barrier that every thread meets; `barrier` is that barrier for a kernel that has none of its own; `apply` is the map and
 * then C byte reads from LDS. */
template <int C> __device__ __forceinline__ uint8_t *tone_lds()
{
	__shared__ uint8_t tone[256 * C];
	return tone;
}
template <> struct EntryMap<const nhw_colour_map *, const nhw_tone_table *> {
	nhw_colour_map c;
	bool mapped;
	const uint8_t *table;
	__device__ __forceinline__ bool load(int k, const nhw_colour_map *maps, const nhw_tone_table *tones)
	{
		mapped = maps != nullptr;
		table = &tones[k].t[0][0];
		if (!mapped) return true;
		c = maps[k];
		return nhw_colour_within(c);
	}
	template <int C> __device__ __forceinline__ void stage() const
	{
		uint8_t *t = tone_lds<C>();
		for (uint32_t i = threadIdx.x; i < 256u * C; i += RS_THREADS) t[i] = table[i];
	}
	__device__ __forceinline__ void barrier() const { __syncthreads(); }
	template <int C> __device__ __forceinline__ void apply(uint32_t *b) const
	{
		if (mapped) nhw_colour_apply<C>(c, b);
		nhw_tone_apply<C>(tone_lds<C>(), b);
	}
};

/* ---- the two taps ----
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
 * nhw_tensor.h.  A workgroup puts the positions of all out_w columns and of its band's rows into LDS, and after the one barrier walks the band
 * 256 >> lg rows at a time, 1 << lg lanes a row (the power of two that holds out_w, 256 at the most: wider rows in steps).  A thread takes
 * one output pixel at a time: twelve byte loads (consecutive lanes on neighbouring source pixels), the blend, and the pixel's store. */
template <int DT, int CHW, int C = 3, class... M>
__global__ __launch_bounds__(RS_THREADS) void k_resize_to_tensor(const nhw_picture *__restrict__ pics, uint32_t out_w, uint32_t out_h, int bands, int rows, int lg,
                                                                  NhwTensorArgs a, const uint8_t *__restrict__ flags, const uint64_t *__restrict__ out_addr, M... maps)
{
	__shared__ uint32_t col_pos[RS_MAX], row_pos[RS_ROWS];
	nhw_picture p;
	typename NhwElem<DT>::type *out;
	uint32_t r0, nr;
	bool mirror;
	if (!resample_entry<DT>(pics, flags, out_addr, out_w, out_h, bands, rows, 0, p, out, r0, nr, mirror)) return;
	EntryMap<M...> cm;
	if (!cm.load((int)(blockIdx.x / bands), maps...)) return;
	cm.template stage<C>();
	for (uint32_t o = threadIdx.x; o < out_w; o += RS_THREADS) col_pos[o] = resize_pos(o, p.width, out_w);
	if (threadIdx.x < nr) row_pos[threadIdx.x] = resize_pos(r0 + threadIdx.x, p.height, out_h);
	__syncthreads();
	const size_t W = out_w, H = out_h;
	for (uint32_t r = threadIdx.x >> lg; r < nr; r += RS_THREADS >> lg) {
		const uint32_t py = row_pos[r], fy = py & 255u;
		const uint8_t *s0 = reinterpret_cast<const uint8_t *>(p.addr + (uint64_t)((py >> 8) & 0xFFFFu) * p.pitch);
		const uint8_t *s1 = s0 + (uint64_t)(py >> 24) * p.pitch;
		const size_t rr = a.flip ? H - 1 - (r0 + r) : r0 + r;
		for (uint32_t c = threadIdx.x & ((1u << lg) - 1); c < out_w; c += 1u << lg) {
			const uint32_t px = col_pos[mirror ? out_w - 1 - c : c], fx = px & 255u, x0 = C * ((px >> 8) & 0xFFFFu), x1 = x0 + C * (px >> 24);
			const uint32_t w00 = (256 - fx) * (256 - fy), w01 = fx * (256 - fy), w10 = (256 - fx) * fy, w11 = fx * fy;
			uint32_t b[C];
#pragma unroll
			for (int ch = 0; ch < C; ch++)
				b[ch] = (w00 * s0[x0 + ch] + w01 * s0[x1 + ch] + w10 * s1[x0 + ch] + w11 * s1[x1 + ch] + 32768u) >> 16;
			cm.template apply<C>(b);
			resample_store<DT, CHW, C>(out, H, W, rr, c, b, a);
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
template <int C>
__device__ __forceinline__ void area_row(const uint8_t *__restrict__ s, uint2 t, uint32_t m, uint32_t *r)
{
	const uint32_t cnt = t.x >> 16, wf = t.y & 0xFFFFu, wl = t.y >> 16;
	const uint8_t *q = s + C * (t.x & 0xFFFFu);
	uint32_t mid[C] = {};
	for (uint32_t i = 1; i + 1 < cnt; i++) {
#pragma unroll
		for (int ch = 0; ch < C; ch++) mid[ch] += q[C * i + ch];
	}
#pragma unroll
	for (int ch = 0; ch < C; ch++) r[ch] = wf * q[ch] + m * mid[ch];
	if (cnt > 1) {
#pragma unroll
		for (int ch = 0; ch < C; ch++) r[ch] += wl * q[C * (cnt - 1) + ch];
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

/* k_resize_to_tensor with the taps of area_taps: the same table, formats, flags, grid and walk -- a thread one output pixel at a time, 1 << lg
 * lanes a row.  The tap runs of all out_w columns and of the band's rows go into LDS (out_w + rows entries of 8 bytes, sized by the launch)
 * before the one barrier.  A pixel then reads its rows x columns source bytes once (neighbouring lanes on neighbouring runs): every row gives
 * three 32-bit sums (area_row), the rows between the first and the last add up in 32 bits as well (127 x 2^24 < 2^31), and only the three
 * products with the row weights and the division are 64 bits wide.  The loops run `count` times, at most 129 under the reduction limit. */
template <int DT, int CHW, int C = 3, class... M>
__global__ __launch_bounds__(RS_THREADS) void k_area_to_tensor(const nhw_picture *__restrict__ pics, uint32_t out_w, uint32_t out_h, int bands, int rows, int lg,
                                                                NhwTensorArgs a, const uint8_t *__restrict__ flags, const uint64_t *__restrict__ out_addr, M... maps)
{
	extern __shared__ uint2 area_tab[];                                    /* [out_w] columns, then [rows] rows */
	nhw_picture p;
	typename NhwElem<DT>::type *out;
	uint32_t r0, nr;
	bool mirror;
	if (!resample_entry<DT>(pics, flags, out_addr, out_w, out_h, bands, rows, NHW_AREA_MAX_REDUCTION, p, out, r0, nr, mirror)) return;
	EntryMap<M...> cm;
	if (!cm.load((int)(blockIdx.x / bands), maps...)) return;
	cm.template stage<C>();
	uint2 *col_tap = area_tab, *row_tap = area_tab + out_w;
	for (uint32_t o = threadIdx.x; o < out_w; o += RS_THREADS) col_tap[o] = area_taps(o, p.width, out_w);
	if (threadIdx.x < nr) row_tap[threadIdx.x] = area_taps(r0 + threadIdx.x, p.height, out_h);
	__syncthreads();
	const size_t W = out_w, H = out_h;
	const uint64_t D = (uint64_t)(out_w >= p.width ? 256u : p.width) * (out_h >= p.height ? 256u : p.height);
	for (uint32_t r = threadIdx.x >> lg; r < nr; r += RS_THREADS >> lg) {
		const uint2 ty = row_tap[r];
		const uint32_t cy = ty.x >> 16;
		const uint8_t *s = reinterpret_cast<const uint8_t *>(p.addr + (uint64_t)(ty.x & 0xFFFFu) * p.pitch);
		const size_t rr = a.flip ? H - 1 - (r0 + r) : r0 + r;
		for (uint32_t c = threadIdx.x & ((1u << lg) - 1); c < out_w; c += 1u << lg) {
			const uint2 tx = col_tap[mirror ? out_w - 1 - c : c];
			uint32_t first[C], last[C] = {}, mid[C] = {}, b[C];
			area_row<C>(s, tx, out_w, first);
			for (uint32_t i = 1; i + 1 < cy; i++) {
				uint32_t v[C];
				area_row<C>(s + (uint64_t)i * p.pitch, tx, out_w, v);
				if constexpr (C == 3) { mid[0] += v[0]; mid[1] += v[1]; mid[2] += v[2]; } else mid[0] += v[0];   /* (spelled out: as a loop over the channels the colour form compiles to other instructions than it always had) */
			}
			if (cy > 1) area_row<C>(s + (uint64_t)(cy - 1) * p.pitch, tx, out_w, last);
#pragma unroll
			for (int ch = 0; ch < C; ch++)
				b[ch] = area_mean((uint64_t)(ty.y & 0xFFFFu) * first[ch] + (uint64_t)out_h * mid[ch] + (uint64_t)(ty.y >> 16) * last[ch], D);
			cm.template apply<C>(b);
			resample_store<DT, CHW, C>(out, H, W, rr, c, b, a);
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

/* k_resize_to_tensor under the cubic rule: the same table, formats, flags and grid.  The rule is separable and fixes the rounding between the
 * passes, so the kernel is: H[y][ox] = (sum_x qx P[y][x] + 128) >> 8 for the source rows a group of output rows needs, as int16 in LDS, then
 * byte = clamp((sum_y qy H[y][ox] + 2^19) >> 20) from there -- Tx + Ty multiply-adds a pixel where the direct form has Tx Ty.  The host knows
 * no source size, so the LDS is fixed: CB_HP pixels of H (24 576 bytes), CB_W int16 weights for a chunk of columns and as many for a chunk
 * of rows (8192), the runs of a chunk's columns and of the band's rows (1280): 34 048 bytes, four workgroups a CU.  The workgroup cuts its
 * band itself, uniformly, from sizes it has checked: tb = floor(4 D / m) + 1 bounds an axis' runs; the weights of wc = min(out_w, CB_COLS,
 * CB_W / tbx) columns are held at a time (all of them for a 224-wide output below a reduction of 2); a pass takes cc = min(wc, CB_HP /
 * (CB_RUNS tby)) of them, so that CB_HP / cc source rows (CB_RUNS runs at least) fit; a chunk of rows grows while its weights fit (CB_W / tby
 * rows) and its source rows -- first run's first to last run's end; firsts and ends do not decrease with o -- fit.  Per chunk of columns:
 * runs and weights (a thread a column); in it per chunk of rows: its weights (a thread a row), barrier; in it per pass: H (a thread a source
 * row and column at a time), barrier, the vertical pass and the pixels' stores, barrier.  Every loop bound is one of these sizes or a count
 * clamped to its table's room. */
template <int DT, int CHW, int C = 3, class... M>
__global__ __launch_bounds__(RS_THREADS) void k_cubic_to_tensor(const nhw_picture *__restrict__ pics, uint32_t out_w, uint32_t out_h, int bands, int rows,
                                                                 NhwTensorArgs a, const uint8_t *__restrict__ flags, const uint64_t *__restrict__ out_addr, M... maps)
{
	__shared__ int16_t cb_h[C * CB_HP], cb_wx[CB_W], cb_wy[CB_W];
	__shared__ uint32_t cb_col[CB_COLS], cb_row[RS_ROWS];
	static_assert(CB_COLS <= RS_THREADS && RS_ROWS <= RS_THREADS, "a thread a run");
	nhw_picture p;
	typename NhwElem<DT>::type *out;
	uint32_t r0, nr;
	bool mirror;
	if (!resample_entry<DT>(pics, flags, out_addr, out_w, out_h, bands, rows, NHW_CUBIC_MAX_REDUCTION, p, out, r0, nr, mirror)) return;
	EntryMap<M...> cm;
	if (!cm.load((int)(blockIdx.x / bands), maps...)) return;
	cm.template stage<C>();
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
				for (uint32_t s = threadIdx.x / lanes; s < span; s += RS_THREADS / lanes) {
					const uint8_t *src = reinterpret_cast<const uint8_t *>(p.addr + (uint64_t)(ylo + s) * p.pitch);
					for (uint32_t j = threadIdx.x & (lanes - 1); j < ncol; j += lanes) {
						const uint32_t run = cb_col[cs + j], cnt = (run >> 16) < tbx ? run >> 16 : tbx;
						const uint8_t *q = src + C * (run & 0xFFFFu);
						const int16_t *wt = cb_wx + (cs + j) * tbx;
						int32_t acc[C] = {};
						for (uint32_t i = 0; i < cnt; i++) {
							const int32_t wi = wt[i];
#pragma unroll
							for (int ch = 0; ch < C; ch++) acc[ch] += wi * (int32_t)q[C * i + ch];
						}
						int16_t *hp = cb_h + C * (s * ncol + j);
#pragma unroll
						for (int ch = 0; ch < C; ch++) hp[ch] = (int16_t)((acc[ch] + 128) >> 8);
					}
				}
				__syncthreads();
				for (uint32_t r = threadIdx.x / lanes; r < re - rs; r += RS_THREADS / lanes) {
					const uint32_t run = cb_row[rs + r], s0 = (run & 0xFFFFu) - ylo, cnt = (run >> 16) < tby ? run >> 16 : tby;
					const int16_t *wt = cb_wy + r * tby;
					const size_t rr = a.flip ? H - 1 - (r0 + rs + r) : r0 + rs + r;
					for (uint32_t j = threadIdx.x & (lanes - 1); j < ncol; j += lanes) {
						int32_t v[C] = {};
						uint32_t b[C];
						for (uint32_t i = 0; i < cnt; i++) {
							const int32_t wi = wt[i];
							const int16_t *hp = cb_h + C * ((s0 + i) * ncol + j);
#pragma unroll
							for (int ch = 0; ch < C; ch++) v[ch] += wi * hp[ch];
						}
#pragma unroll
						for (int ch = 0; ch < C; ch++) {
							const int32_t y = (v[ch] + (1 << 19)) >> 20;
							b[ch] = (uint32_t)(y < 0 ? 0 : y > 255 ? 255 : y);
						}
						cm.template apply<C>(b);
						resample_store<DT, CHW, C>(out, H, W, rr, mirror ? out_w - 1 - (ws + cs + j) : ws + cs + j, b, a);
					}
				}
				__syncthreads();                                             /* before H, these rows' weights or the columns' are written again */
			}
			rs = re;
		}
	}
}

/* ---- the affine warp: two taps a direction along a tilted grid ----
 * k_resize_to_tensor with the positions of an nhw_warp in place of an axis' table: the same picture table, formats, grid and band, no flags (a
 * mirror is a matrix), no LDS and no division beyond resample_entry's own.  The entry's limits are checked here (nhw_warp_within), so that every width below holds
 * whatever the table says: a (2 ox + 1) + b (2 oy + 1) is below 2^36, SX and SY below 2^41, X8 below 2^33 and ix, iy below 2^25 in magnitude.
 * warp_pixel makes one output pixel: the four taps are loaded from the indices clamped to the picture -- inside it for every position, since
 * resample_entry has seen the sides -- and a tap judged outside then gives way to the border colour unless the entry replicates: twelve byte
 * loads, the blend of section 18; the caller stores the pixel.  The row's part of the position (bx, ey) is the caller's; a pixel adds its
 * own with one 32 x 32 -> 64-bit multiply an axis.  iy x pitch is 64 bits wide.
 * Two walks over the band, chosen by the entry (uniformly for the workgroup).  Where the grid's rows are nearly the source's -- d, the source
 * rows a step along an output row crosses, is at most WARP_ROW_LANES / 65536 = 1/4: a wavefront's 64 columns stay within 16 source rows -- the
 * walk is k_resize_to_tensor's, 1 << lg lanes an output row: stores of consecutive lanes are consecutive elements, and the loads follow the
 * source's rows.  Elsewhere a wavefront takes an 8 x 8 block of output pixels at a time, which keeps its taps within a compact patch of the
 * source at any angle and cuts its stores into runs of 8 elements.  Measured (section 21), 4096 entries of 256 x 256 -> 224 x 224: rows 1.7,
 * 4.4 and 7.6 ms at 0, 30 and 90 degrees, blocks 2.6, 2.9 and 2.8 ms; the two meet at 15 degrees, d = 19 385, and the limit is the power of two below. */
constexpr int32_t WARP_ROW_LANES = 16384;
int32_t warp_row_limit = WARP_ROW_LANES;          /* host: what the launches pass as row_limit; nhw_debug_warp_row_limit (include/nhw_hip_debug.h) moves it */
template <int C>
__device__ __forceinline__ void warp_pixel(const nhw_warp &m, const nhw_picture &p, bool fill, int64_t bx, int64_t ey, uint32_t c, uint32_t *b)
{
	const int32_t xl = (int32_t)p.width - 1, yl = (int32_t)p.height - 1;     /* 0 .. 65534 */
	const uint8_t *src = reinterpret_cast<const uint8_t *>(p.addr);
	const int32_t tx = (int32_t)(2 * c + 1);
	const int64_t X8 = ((((int64_t)m.a * tx + bx) >> 1) + m.c + 128) >> 8, Y8 = ((((int64_t)m.d * tx + ey) >> 1) + m.f + 128) >> 8;
	const int32_t ix = (int32_t)(X8 >> 8), iy = (int32_t)(Y8 >> 8);
	const uint32_t fx = (uint32_t)X8 & 255u, fy = (uint32_t)Y8 & 255u;
	const int32_t x0 = ix < 0 ? 0 : ix > xl ? xl : ix, x1 = ix + 1 < 0 ? 0 : ix + 1 > xl ? xl : ix + 1;
	const int32_t y0 = iy < 0 ? 0 : iy > yl ? yl : iy, y1 = iy + 1 < 0 ? 0 : iy + 1 > yl ? yl : iy + 1;
	const bool ox0 = fill && x0 != ix, ox1 = fill && x1 != ix + 1, oy0 = fill && y0 != iy, oy1 = fill && y1 != iy + 1;
	const uint8_t *s0 = src + (uint64_t)(uint32_t)y0 * p.pitch, *s1 = src + (uint64_t)(uint32_t)y1 * p.pitch;
	const uint32_t w00 = (256 - fx) * (256 - fy), w01 = fx * (256 - fy), w10 = (256 - fx) * fy, w11 = fx * fy;
#pragma unroll
	for (int ch = 0; ch < C; ch++) {
		uint32_t t00 = s0[C * x0 + ch], t01 = s0[C * x1 + ch], t10 = s1[C * x0 + ch], t11 = s1[C * x1 + ch];
		if (oy0 || ox0) t00 = m.fill[ch];
		if (oy0 || ox1) t01 = m.fill[ch];
		if (oy1 || ox0) t10 = m.fill[ch];
		if (oy1 || ox1) t11 = m.fill[ch];
		b[ch] = (w00 * t00 + w01 * t01 + w10 * t10 + w11 * t11 + 32768u) >> 16;
	}
}

template <int DT, int CHW, int C = 3, class... M>
__global__ __launch_bounds__(RS_THREADS) void k_warp_to_tensor(const nhw_picture *__restrict__ pics, const nhw_warp *__restrict__ warps, uint32_t out_w, uint32_t out_h,
                                                                int bands, int rows, int lg, int32_t row_limit, NhwTensorArgs a, const uint64_t *__restrict__ out_addr, M... maps)
{
	nhw_picture p;
	typename NhwElem<DT>::type *out;
	uint32_t r0, nr;
	bool mirror;                                                             /* (never set: there is no flag table) */
	int k;
	if (!resample_entry_at<DT>(pics, nullptr, out_addr, out_w, out_h, bands, rows, 0, p, out, r0, nr, mirror, k)) return;
	const nhw_warp m = warps[k];
	if (!nhw_warp_within(m)) return;
	EntryMap<M...> cm;
	if (!cm.load(k, maps...)) return;
	cm.template stage<C>();
	cm.barrier();
	const bool fill = !(m.flags & NHW_WARP_REPLICATE);
	const size_t W = out_w, H = out_h;
	if ((m.d < 0 ? -m.d : m.d) > row_limit) {                                /* a wavefront an 8 x 8 block of output pixels (|d| <= 2^22: checked) */
		const uint32_t tiles_x = (out_w + 7) >> 3, tiles_y = (nr + 7) >> 3, lane = threadIdx.x & 63u;
		uint32_t tc = threadIdx.x >> 6, tr = 0;
		for (;;) {
			while (tc >= tiles_x) { tc -= tiles_x; tr++; }
			if (tr >= tiles_y) break;
			const uint32_t r = 8 * tr + (lane >> 3), c = 8 * tc + (lane & 7u);
			if (r < nr && c < out_w) {
				const int32_t ty = (int32_t)(2 * (r0 + r) + 1);
				uint32_t b[C];
				warp_pixel<C>(m, p, fill, (int64_t)m.b * ty, (int64_t)m.e * ty, c, b);
				cm.template apply<C>(b);
				resample_store<DT, CHW, C>(out, H, W, a.flip ? H - 1 - (r0 + r) : r0 + r, c, b, a);
			}
			tc += RS_THREADS >> 6;
		}
		return;
	}
	for (uint32_t r = threadIdx.x >> lg; r < nr; r += RS_THREADS >> lg) {
		const int32_t ty = (int32_t)(2 * (r0 + r) + 1);
		const int64_t bx = (int64_t)m.b * ty, ey = (int64_t)m.e * ty;
		const size_t rr = a.flip ? H - 1 - (r0 + r) : r0 + r;
		for (uint32_t c = threadIdx.x & ((1u << lg) - 1); c < out_w; c += 1u << lg) {
			uint32_t b[C];
			warp_pixel<C>(m, p, fill, bx, ey, c, b);
			cm.template apply<C>(b);
			resample_store<DT, CHW, C>(out, H, W, rr, c, b, a);
		}
	}
}

} /* namespace */

/* The band rule: some 8192 workgroups in all where the entries are few, one band an entry where they are many; a band has at most RS_ROWS rows
 * and, where the output is narrow, at least the rows of one pass (256 >> lg), so that a pass has work for every lane.  All four kernels meet
 * the same launch shapes, those of resample_bands: false for what no kernel is launched for.  The area kernel's LDS is sized by its launch: the
 * tap runs of the columns and of a band's rows, 8 (out_w + rows) bytes, 33 280 at the most; the cubic and the two-tap kernel have static LDS,
 * the warp has none, and the cubic kernel cuts its band itself (it takes no lg).  A toned form has its table's 256 C bytes of static LDS on top
 * (the area kernel's tap runs lie behind them). */
static bool resample_bands(int n, uint32_t out_w, uint32_t out_h, int &lg, uint32_t &rows, int &bands)
{
	if (n < 1 || n > (1 << 24) || out_w < 1 || out_h < 1 || out_w > (uint32_t)RS_MAX || out_h > (uint32_t)RS_MAX) return false;
	lg = 0;
	while (lg < 8 && (1u << lg) < out_w) lg++;
	const uint32_t want = (8192u + (uint32_t)n - 1) / (uint32_t)n < out_h ? (8192u + (uint32_t)n - 1) / (uint32_t)n : out_h;   /* bands wanted: 1 .. out_h */
	rows = (out_h + want - 1) / want;
	if (rows < (uint32_t)(RS_THREADS >> lg)) rows = RS_THREADS >> lg;
	if (rows > (uint32_t)RS_ROWS) rows = RS_ROWS;
	bands = (int)((out_h + rows - 1) / rows);                           /* 1 .. 4096; with n above 8192, 64 at the most: n * bands is below 2^31 */
	return true;
}

/* f(DT, CHW, C as std::integral_constants) for a checked format and the call's family: the dtype and layout of a colour call with C = 3; the dtype
 * alone of a grey one, with CHW = 0 and C = 1 */
template <int V> using Int = std::integral_constant<int, V>;
template <class F> static void with_form(bool grey, int dtype, int layout, F &&f)
{
	const auto of = [&](auto dt) {
		if (grey) f(dt, Int<0>{}, Int<1>{});
		else if (layout == NHW_T_HWC) f(dt, Int<NHW_T_HWC>{}, Int<3>{});
		else f(dt, Int<NHW_T_CHW>{}, Int<3>{});
	};
	switch (dtype) {
	case NHW_T_U8: of(Int<NHW_T_U8>{}); break;
	case NHW_T_F16: of(Int<NHW_T_F16>{}); break;
	case NHW_T_BF16: of(Int<NHW_T_BF16>{}); break;
	default: of(Int<NHW_T_F32>{}); break;
	}
}

/* f(the pack M... of the call's kernels) by its tables (DESIGN.md sections 24 and 25): nothing for a call without maps and tone tables, so that it
 * runs the kernels that have no such arguments; the maps alone; or, for a toned call, the maps -- null where it has none -- and the tone tables */
template <class F> static void with_pack(const NhwOpsArgs &o, F &&f)
{
	if (o.tones) f(o.maps, o.tones);
	else if (o.maps) f(o.maps);
	else f();
}

/* the developer's hook for measurements and tests: every later launch of the process walks by rows where |d| <= limit (-1: blocks for every
 * entry; 2^22: rows for every entry); a limit below -1 puts the rule's own back.  The results are the same bytes whatever the walk. */
extern "C" void nhw_debug_warp_row_limit(int limit) { warp_row_limit = limit < -1 ? WARP_ROW_LANES : limit; }

/* The one launch of a sampling call (NhwSampleCall, nhw_tensor.h): the form and the pack above, the band rule, and the call's kernel -- the warp's
 * where it has warps, else its filter's. */
hipError_t nhw_launch_sample(const NhwSampleCall &c, hipStream_t s)
{
	if (!c.warps && (c.filter < NHW_FILTER_TWO_TAP || c.filter > NHW_FILTER_CUBIC)) return hipErrorInvalidValue;
	const NhwTensorOut &o = c.out;
	int lg, bands;
	uint32_t rows;
	if (!resample_bands(c.n, o.w, o.h, lg, rows, bands)) return hipErrorInvalidValue;
	with_form(c.grey, o.dtype, o.layout, [&](auto dt, auto chw, auto ch) {
		with_pack(c.ops, [&](auto... m) {
			constexpr int DT = decltype(dt)::value, CHW = decltype(chw)::value, C = decltype(ch)::value;
			const int grid = c.n * bands;
			if (c.warps) {
				k_warp_to_tensor<DT, CHW, C, decltype(m)...><<<grid, RS_THREADS, 0, s>>>(c.pics, c.warps, o.w, o.h, bands, (int)rows, lg, warp_row_limit, o.a, c.out_addr, m...);
				return;
			}
			switch (c.filter) {
			case NHW_FILTER_TWO_TAP:
				k_resize_to_tensor<DT, CHW, C, decltype(m)...><<<grid, RS_THREADS, 0, s>>>(c.pics, o.w, o.h, bands, (int)rows, lg, o.a, c.ops.flags, c.out_addr, m...);
				break;
			case NHW_FILTER_AREA:
				k_area_to_tensor<DT, CHW, C, decltype(m)...><<<grid, RS_THREADS, sizeof(uint2) * ((size_t)o.w + rows), s>>>(c.pics, o.w, o.h, bands, (int)rows, lg, o.a, c.ops.flags, c.out_addr, m...);
				break;
			default:
				k_cubic_to_tensor<DT, CHW, C, decltype(m)...><<<grid, RS_THREADS, 0, s>>>(c.pics, o.w, o.h, bands, (int)rows, o.a, c.ops.flags, c.out_addr, m...);
			}
		});
	});
	return hipGetLastError();
}

