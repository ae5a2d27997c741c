/*
 * nhw_tail.hip -- kernels that run the order-dependent phases of the NHW encoder, one 256-thread workgroup
 * per image (see nhw_tail_par.h / nhw_tail_dev.h), plus the small block-copy kernel used between them.
 */
#include "nhw_host.h"
#include "nhw_tail_par.h"
#include "nhw_dwt.h"

using namespace nhw;

#ifndef NHW_DENSE_STREAM
#define NHW_DENSE_STREAM 0          /* 1: the luma byte stream is written (and rewritten by the dense Y31) next to the list -- a developer switch for comparing the two forms */
#endif

template <int PH>
__global__ __launch_bounds__(256) void k_phase(NhwWs ws, int comp)
{
	__shared__ int sh_counts[2];
	__shared__ int sh_pos[2 * NT + 2];
	__shared__ uint32_t sh_z[4 * Q / 16 / 32 + 4];
	extern __shared__ __attribute__((aligned(16))) int16_t dyn_lds[];   /* LDS tiles of the row-serial passes (size chosen per phase at launch) */
	const int img = blockIdx.x, tid = threadIdx.x;
	Ctx c;
	ctx_load(&c, ws, img, comp);
	if (PH == PH_L1) luma_p1_par(&c, tid, sh_pos);
	else if (PH == PH_L2) luma_p2_par(&c, tid, dyn_lds);
	else if (PH == PH_L3) luma_p3_par(&c, tid, sh_pos, sh_counts, dyn_lds, ws.q <= 12 || ws.dbg != 0);
	else if (PH == PH_L4A) luma_p4a_par(&c, tid, dyn_lds);
	else if (PH == PH_L4B) luma_p4b_par(&c, tid, sh_pos, dyn_lds);
	else if (PH == PH_L4C) luma_p4c_par(&c, tid, sh_pos, dyn_lds, ws.q > 21 || ws.dbg);
	else if (PH == PH_L4D) luma_p4d_par(&c, tid, sh_counts, sh_z, dyn_lds, NHW_DENSE_STREAM || ws.dbg);
	else if (PH == PH_L4C2) luma_p4c2_par(&c, tid, reinterpret_cast<unsigned *>(sh_z), sh_pos);
	else if (PH == PH_LLC) { PROF_BEGIN(); ll_code_chroma_par(&c, tid, reinterpret_cast<uint8_t *>(dyn_lds)); if (!tid) PROF(&c, 18); }
	else if (PH == PH_C0) chroma_p0_par(&c, comp, tid);
	else if (PH == PH_C2) { chroma_ll1_neighbour(&c, tid); dequant_sim_chroma_par(&c, 1, tid); }
	else if (PH == PH_C3) chroma_p3_par(&c, comp, tid);
	else if (PH == PH_C4) dequant_sim_chroma_par(&c, 0, tid);
	else if (PH == PH_C5) chroma_p5_par(&c, comp, tid, dyn_lds, sh_counts, ws.dbg != 0);
}

/* Z2 + the container as two kernels, each with one copy of the walks (pack_words_par).
 * k_pack_chroma packs the chroma part's words and ranks its book: its inputs are complete behind V's quantiser, before the luma part's,
 * and everything it writes is its own (B_CPACK, B_CPACKET), so the forked order runs it beside Z1 in front of the join (nhw_enc.hip,
 * run_batch); every other order launches it directly in front of k_final.  k_final packs the luma part, makes both books (book 2 reads on
 * into book 1's bytes: the one thing the chroma part needs of the luma part), puts the chroma part's words behind the luma part's and
 * writes the container.
 * Registers (gfx950 code objects).  While one kernel held both parts as two inlined copies of the walks the register allocator took 158
 * (three wavefronts a SIMD: +0.35 ms); held to 128 (four) it spilled 20 dwords, 84 bytes of scratch a lane.  With one copy k_final takes
 * 107 and k_pack_chroma 93 without scratch, and both fit the bound their LDS (22.9 KB a workgroup) allows: six workgroups a CU, 80
 * registers -- the 16 images a CU gets of a 4096-image batch in three rounds instead of four.  At 80 k_final spills 77 dwords (104 bytes
 * of scratch) and k_pack_chroma 23 (48 bytes), all in the code-book construction, off the walks.  Alone on the chip, 4096 images, q20:
 * k_final 1.222 ms at four wavefronts a SIMD, 1.228 at five (96 registers, 21 spilled), 1.171 at six; k_pack_chroma 0.321 / 0.300 / 0.312. */
#ifndef NHW_FINAL_WAVES
#define NHW_FINAL_WAVES 6
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NHW_FINAL_WAVES, NHW_FINAL_WAVES))) void k_final(NhwWs ws, uint8_t *out, uint32_t *sizes, int32_t *status)
{
	extern __shared__ __attribute__((aligned(16))) int16_t dyn_lds[];
	__shared__ PackShared sh_pack;
	const int img = blockIdx.x, tid = threadIdx.x;
	Ctx c;
	ctx_load(&c, ws, img);
	final_phase_par(&c, ws.buf<NhwChromaPack>(B_CPACK, img), ws.buf<uint32_t>(B_CPACKET, img), out + (size_t)img * (512u << 10), 512u << 10, &sizes[img], &status[img], &sh_pack, tid,
	                reinterpret_cast<uint32_t *>(dyn_lds));
}

#ifndef NHW_PACKC_WAVES
#define NHW_PACKC_WAVES 6
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NHW_PACKC_WAVES, NHW_PACKC_WAVES))) void k_pack_chroma(NhwWs ws)
{
	extern __shared__ __attribute__((aligned(16))) int16_t dyn_lds[];
	__shared__ PackShared sh_pack;
	const int img = blockIdx.x;
	Ctx c;
	ctx_load(&c, ws, img);
	pack_chroma_par(&c, ws.buf<NhwChromaPack>(B_CPACK, img), ws.buf<uint32_t>(B_CPACKET, img), &sh_pack, threadIdx.x, reinterpret_cast<uint32_t *>(dyn_lds));
}

/* Y31 on the symbol list as a kernel of 512 threads (production; the stage checks run k_phase<L4D>, which has the dense form behind it) */
__global__ __launch_bounds__(512) void k_y31(NhwWs ws)
{
	extern __shared__ __attribute__((aligned(16))) int16_t dyn_lds[];
	__shared__ int sh_counts[2];
	Ctx c;
	ctx_load(&c, ws, blockIdx.x);
	PROF_BEGIN();
	scan_rewrite_list_par<512>(&c, threadIdx.x, reinterpret_cast<uint8_t *>(dyn_lds), sh_counts);
	if (!threadIdx.x) PROF(&c, 17);
}

/* Y19-Y23 of quality 17 .. 23 as a kernel of its own, held to eight wavefronts a SIMD (64 registers): with its 20 KB of LDS that is eight
 * workgroups a CU -- the 16 images a CU gets of a 4096-image batch in two rounds (k_phase<PH_L4A> takes 67 registers: seven, 7 + 7 + 2).
 * The low qualities' Y20 (thin_l1_low_par) would spill at 64 and stays on k_phase. */
#ifndef NHW_L4A_WAVES
#define NHW_L4A_WAVES 8
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NHW_L4A_WAVES, NHW_L4A_WAVES))) void k_l4a(NhwWs ws)
{
	extern __shared__ __attribute__((aligned(16))) int16_t dyn_lds[];
	Ctx c;
	ctx_load(&c, ws, blockIdx.x);
	luma_p4a_par(&c, threadIdx.x, dyn_lds);
}

/* the chroma tail of a production batch as a kernel of its own (chroma_tail_once_par: each plane row read once, cproc not written); the stage
 * checks and NHW_CHROMA_TAIL_ONCE=0 run k_phase<PH_C5>, the staged form.  Its two sets of parked rows (35.6 KB of LDS) allow four workgroups
 * a CU; the register allocator took 129, one over what four wavefronts a SIMD allow, and takes 128 without scratch when held to four. */
#ifndef NHW_CTAIL_WAVES
#define NHW_CTAIL_WAVES 4
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NHW_CTAIL_WAVES, NHW_CTAIL_WAVES))) void k_chroma_tail(NhwWs ws, int comp)
{
	extern __shared__ __attribute__((aligned(16))) int16_t dyn_lds[];
	Ctx c;
	ctx_load(&c, ws, blockIdx.x, comp);
	chroma_tail_once_par(&c, comp, threadIdx.x, dyn_lds);
}

/* passes that run one wavefront per image (nhw_tail_wave.h): four images per workgroup, no workgroup barriers */
template <int PH>
__global__ __launch_bounds__(256) void k_wave(NhwWs ws, int flags /* bit 0, WV_EMIT and WV_DQ0: the LL2 bump walk is made once, by the emission (wave_emit_ll2); bit 1, WV_DQ0 and WV_QUANT: the simulation leaves the level-2 details behind the quantiser's loops 2 and 3 in B_KMAP, the quantiser takes them from there (wave_dequant_details) */)
{
	const int one_walk = flags & 1, marks = flags & 2;
	const int img = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	__shared__ uint32_t dq_lut[(PH == WV_DQ1 || PH == WV_DQ0) ? DQ_WORDS : 1];
	if (PH == WV_DQ1 || PH == WV_DQ0) {                            /* the one workgroup barrier of these kernels: the table of the dequantiser walk */
		for (int i = threadIdx.x; i < DQ_WORDS; i += 256) dq_lut[i] = dq_entry(i);
		__syncthreads();
	}
	if (img >= ws.n) return;
	Ctx c;
	ctx_load(&c, ws, img);
	if (PH == WV_DQ1) wave_dequant_sim_luma(&c, 1, lane, dq_lut, false, ws.dbg != 0);
	else if (PH == WV_DQ0) wave_dequant_sim_luma(&c, 0, lane, dq_lut, !ws.dbg, ws.dbg != 0, one_walk != 0, marks ? ws.buf<int16_t>(B_KMAP, img) : nullptr);   /* production: the level-2 block straight from l2save (Y17's restore of the work plane is not made: luma_p3_par) */
	else if (PH == WV_QUANT) {
		__shared__ __attribute__((aligned(16))) uint8_t park[4][16 * QROW];
		__shared__ uint32_t lut[4][QLUT + 3];
		PROF_BEGIN(); wave_quantise_luma(&c, lane, park[threadIdx.x >> 6], lut[threadIdx.x >> 6], ws.q > 21 || ws.dbg, NHW_DENSE_STREAM || ws.dbg, !(ws.q > 21 || ws.dbg), marks ? ws.buf<int16_t>(B_KMAP, img) : nullptr); if (!lane) PROF(&c, 15);
	}
	else if (PH == WV_EMIT) { PROF_BEGIN(); wave_emit_ll2(&c, lane, one_walk != 0); if (!lane) PROF(&c, 4); }
}
void nhw_launch_wave(int ph, const NhwWs &ws, hipStream_t s, bool one_walk, bool marks)
{
	const dim3 g((ws.n + 3) / 4), b(256);
	assert(!one_walk || ((ph == WV_EMIT || ph == WV_DQ0) && ws.q > 12 && !ws.dbg));
	assert(!marks || ((ph == WV_DQ0 || ph == WV_QUANT) && ws.q > 16 && !ws.dbg));
	(ph == WV_DQ1 ? k_wave<WV_DQ1> : ph == WV_DQ0 ? k_wave<WV_DQ0> : ph == WV_EMIT ? k_wave<WV_EMIT> : k_wave<WV_QUANT>)<<<g, b, 0, s>>>(ws, (one_walk ? 1 : 0) | (marks ? 2 : 0));
}

/* The middle of the first closed loop on one LDS residency of the 256 x 256 block: level-2 synthesis (wavelet_filterbank.c:305-496), Y8 (the
 * tags of the level-2 details nudge the reconstruction, nhw_encoder.c:183-216) and Y9 (LL1 pre-compensation, :218-279).  The reconstruction
 * is only ever read by Y9, and Y9 only hands on `ll1 + step` (the input of the analysis that follows): as three kernels the block went out
 * twice in two orientations, came back through Y8's tiles and Y9's rows and went out again (6.3 GB per 4096 images); here it never leaves
 * the LDS (2.2 GB: coefficients and LL1 in, LL1 without its tags and the pre-compensated LL1 out).
 *   * the synthesis leaves column c of the block as what the plane holds in row c: proc[y][x] = A[x][y];
 *   * a tag at (r, j) of the LL1 plane nudges proc[2(j-128)+1][2r], proc[2j][2(r-128)+1] or proc[2(j-128)+1][2(r-128)+1] (:205-213), i.e. a
 *     cell of ROW 2r / 2(r-128)+1 of the block: a wavefront takes an LL1 row, its targets are cells of one row of LDS, no two tags share one;
 *   * Y9 walks a row of proc = a column of the block (odd dword stride: no bank conflicts), a lane four cells, the step handed from lane to
 *     lane until nothing moves (precompensate_ll1_par).  Its two outer neighbours are cells of the planes outside the block.
 * One 1024-thread workgroup per CU works through the batch, the next block on its way in registers (k_dwt_syn).  The tests' stage checks
 * (nhw_debug_stop_after) run the three kernels instead, which leave every intermediate plane.
 *
 * ANA (q > 12): the kernel carries on into the level-2 analysis of the pre-compensated block (nhw_encoder.c:281, k_dwt_ana<256> until then) and
 * Y13's copy of the coefficient block.  The pre-compensated rows had one reader, a kernel of the same shape that loaded them into the same
 * LDS: 0.54 GB out and 0.54 GB back in per 4096 images, a launch and a drain of a one-workgroup-a-CU grid.  Here they never leave the CU:
 *   * Y9's wavefront reads only its own 16 columns of A (A[(c0 + k) * LS + r], r one of its 16 rows) and nobody else reads them behind the
 *     barrier in front of Y9, so it may write into them while the others are still in Y9.  It filters the settled row in registers
 *     (ana_row_quad: the analysis' first direction runs along an LL1 row) and parks output pos of row r at A[pos * LS + r];
 *   * behind ONE barrier A[i][j] is cell (i, j) of the TRANSPOSED first-direction plane, which is what the work plane keeps
 *     (jpeg[i * stride + j]: k_dwt_ana gathers it): a straight row copy.  The second direction runs along rows of A, and output row c is row
 *     c of proc and of l2save.  A wavefront takes its own 16 rows through all three steps (copy, filter in place, copy), two rows at a
 *     time: no further barrier, and every global store is 16 bytes a lane on whole 512-byte rows;
 *   * LEAN (run_batch outside the compatibility mode; the stage hooks keep every store) leaves out what nothing reads.  The transposed
 *     first-direction plane in the block of jpeg: the next kernels that touch the block are the LL2 emission and the second dequantiser
 *     simulation, which between them write every cell of it before wave_shrink and k_dwt_syn read it (the case list at wave_dequant_details).
 *     Rows 128 .. 255 of the block of the work plane: the LL2 emission (wave_emit_ll2: ll2_load_row takes rows 0 .. 127, columns 0 .. 191) is
 *     the one reader of the block -- the second simulation, k_phase<PH_L4C> and the quantiser take it from l2save, the put-backs of verbatim
 *     samples read LL2 cells the emission or the simulation's walk has just written -- and k_dwt_syn behind the simulation rewrites all of it.
 * The arithmetic is ana_row_taps' and ana_col_pair's (nhw_dwt.h), as in k_dwt_ana. */
template <bool ANA, bool LEAN = false>
__global__ __launch_bounds__(1024) void k_l2_recon(int16_t *__restrict__ jpegb, int16_t *__restrict__ procb, size_t plane_stride, int16_t *__restrict__ ll1b, size_t ll1_stride, int n,
                                                   int16_t *__restrict__ saveb, size_t save_stride)
{
	extern __shared__ __attribute__((aligned(16))) int16_t smem[];
	constexpr int S = H, LS = S + 2, HLF = S / 2, PPL = HLF / 64, NT_ = 1024, NPRE = S * (S / 8) / NT_;
	const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
	int16_t *A = smem;
	int8_t *ytab = reinterpret_cast<int8_t *>(A + S * LS);         /* Y9's step by (difference, what it sees of its neighbours) */
	if (t < PRECOMP_TAB) ytab[t] = (int8_t)precomp_pick(t / 11 - 12, t % 11 - 5);
	uint4 pre[NPRE];
	if ((int)blockIdx.x < n) {
		const int16_t *src = jpegb + (size_t)blockIdx.x * plane_stride;
#pragma unroll
		for (int u = 0; u < NPRE; u++) { const int v = t + u * NT_; pre[u] = *reinterpret_cast<const uint4 *>(src + (size_t)(v / (S / 8)) * W + 8 * (v % (S / 8))); }
	}
	for (int img = blockIdx.x; img < n; img += gridDim.x) {
		int16_t *jp = jpegb + (size_t)img * plane_stride, *o = ll1b + (size_t)img * ll1_stride;
		int16_t *p = procb + (size_t)img * plane_stride;
#pragma unroll
		for (int u = 0; u < NPRE; u++) {
			const int v = t + u * NT_, row = v / (S / 8), c8 = v % (S / 8);
			uint32_t *d = reinterpret_cast<uint32_t *>(A + row * LS + 8 * c8);
			d[0] = pre[u].x; d[1] = pre[u].y; d[2] = pre[u].z; d[3] = pre[u].w;
		}
		lds_barrier();
		if (img + (int)gridDim.x < n) {
			const int16_t *src = jpegb + (size_t)(img + gridDim.x) * plane_stride;
#pragma unroll
			for (int u = 0; u < NPRE; u++) { const int v = t + u * NT_; pre[u] = *reinterpret_cast<const uint4 *>(src + (size_t)(v / (S / 8)) * W + 8 * (v % (S / 8))); }
		}
		/* the cells of the planes around the block that Y9 looks at, requested now -- lane l < 16: the cell of proc before row l of mine, lanes
		 * 16 .. 31: the one behind it; lane 32 / 33: the LL1 cell before my first row / behind my last one (rows of my neighbours).  Taking a
		 * tag off an LL1 cell is a function of the cell, so nobody waits for the wavefront that writes the clean value back. */
		const int r0 = wv * 16, c0 = 4 * lane;
		int side = 0;
		if (lane < 16) side = p[(size_t)(r0 + lane) * W - 1];
		else if (lane < 32) side = p[(size_t)(r0 + lane - 16) * W + H];
		else if (lane == 32) { side = o[(size_t)r0 * H - 1]; if (wv > 0) side = side > 14000 ? side - 16000 : side > 10000 ? side - 12000 : side; }   /* (what lies outside the plane is left as it is) */
		else if (lane == 33) { side = o[(size_t)(r0 + 16) * H]; if (wv < 15) side = side > 14000 ? side - 16000 : side > 10000 ? side - 12000 : side; }
		for (int i = 0; i < 16; i++) {                             /* synthesis, first direction, un-normalised */
			int16_t *x = A + (wv * 16 + i) * LS;
			int e[PPL], od[PPL];
#pragma unroll
			for (int u = 0; u < PPL; u++) syn_pair<S>(x, 1, lane + 64 * u, false, &e[u], &od[u]);
#pragma unroll
			for (int u = 0; u < PPL; u++) reinterpret_cast<uint32_t *>(x)[lane + 64 * u] = (uint32_t)(uint16_t)e[u] | ((uint32_t)(uint16_t)od[u] << 16);
		}
		lds_barrier();
#pragma unroll 4                                                   /* (unrolled 16 times the compiler keeps every column's addresses across the image loop and spills 20 - 29 dwords) */
		for (int i = 0; i < 16; i++) {                             /* second direction along the columns, normalised, in place */
			int16_t *x = A + wv * 16 + i;
			int e[PPL], od[PPL];
#pragma unroll
			for (int u = 0; u < PPL; u++) syn_pair<S>(x, LS, lane + 64 * u, true, &e[u], &od[u]);
#pragma unroll
			for (int u = 0; u < PPL; u++) { const int k = lane + 64 * u; x[(2 * k) * LS] = (int16_t)e[u]; x[(2 * k + 1) * LS] = (int16_t)od[u]; }
		}
		lds_barrier();
		auto ll1_row = [&](int i) { return *reinterpret_cast<const uint2 *>(o + (size_t)(r0 + (i < 16 ? i : 15)) * H + c0); };   /* row i of mine */
		auto untag = [](int v) { return v > 14000 ? v - 16000 : v > 10000 ? v - 12000 : v; };
		/* both walks keep a window of four rows in registers: the row in hand and the three behind it, requested three rows ahead of their use
		 * (rolled loops: unrolled, the compiler interleaves the rows and spills) */
		uint2 w0 = ll1_row(0), w1 = ll1_row(1), w2 = ll1_row(2), w3 = ll1_row(3);
#pragma unroll 1
		for (int i = 0; i < 16; i++) {                             /* Y8: LL1 row r, a lane four cells */
			const int r = r0 + i;
			int v[4];
			unpack4(w0, v);
			w0 = w1; w1 = w2; w2 = w3; w3 = ll1_row(i + 4);
			bool any = false;
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const int step = v[k] > 14000 ? 1 : v[k] > 10000 ? -1 : 0;
				if (!step) continue;
				v[k] = untag(v[k]);
				any = true;
				const int j = c0 + k;
				if (r < HLF && j >= HLF) A[(2 * r) * LS + 2 * (j - HLF) + 1] += (int16_t)step;
				else if (r >= HLF && j < HLF) A[(2 * (r - HLF) + 1) * LS + 2 * j] += (int16_t)step;
				else if (r >= HLF && j >= HLF) A[(2 * (r - HLF) + 1) * LS + 2 * (j - HLF) + 1] += (int16_t)step;
			}
			if (any) {
				uint2 w;
				w.x = (uint32_t)(uint16_t)v[0] | ((uint32_t)(uint16_t)v[1] << 16); w.y = (uint32_t)(uint16_t)v[2] | ((uint32_t)(uint16_t)v[3] << 16);
				*reinterpret_cast<uint2 *>(o + (size_t)r * H + c0) = w;
			}
		}
		w0 = ll1_row(0); w1 = ll1_row(1); w2 = ll1_row(2); w3 = ll1_row(3);   /* (with or without their tags: whichever the memory system hands out) */
		lds_barrier();                                             /* the nudged block */
		int o_left = __builtin_amdgcn_readlane(side, 32);          /* the LL1 cell before the row in memory, without its tag */
#pragma unroll 1
		for (int i = 0; i < 16; i++) {                             /* Y9 */
			const int r = r0 + i;
			int pv[4], ov[4], d[4], st[4];
			unpack4(w0, ov);
			/* left of column 0 / right of column 255: the cells before and behind the row in memory, never updated */
			const int o_right = i == 15 ? __builtin_amdgcn_readlane(side, 33) : untag((int)(int16_t)(__builtin_amdgcn_readlane((int)w1.x, 0) & 0xFFFF));
			w0 = w1; w1 = w2; w2 = w3; w3 = ll1_row(i + 4);
#pragma unroll
			for (int k = 0; k < 4; k++) { ov[k] = untag(ov[k]); pv[k] = A[(c0 + k) * LS + r]; d[k] = (int16_t)(pv[k] - ov[k]); }
			const int p_left = __shfl(side, i), p_right = __shfl(side, 16 + i);
			const int my_edge = lane ? p_right - o_right : p_left - o_left;
			o_left = __builtin_amdgcn_readlane(ov[3], 63);
			const int sd = __shfl_down(d[0], 1), su = __shfl_up(d[3], 1);
			const int dn4 = lane < 63 ? sd : my_edge;                 /* the difference on the right of my last cell, as it was */
			const int first = lane ? su : my_edge;
			const int nb[4] = { precomp_right(d[1]), precomp_right(d[2]), precomp_right(d[3]), precomp_right(dn4) };
			int prev_in = first;
			for (;;) {
				int prev = prev_in;
#pragma unroll
				for (int k = 0; k < 4; k++) { st[k] = ytab[precomp_index(d[k], nb[k] + prev)]; prev = d[k] + st[k]; }
				int np = __shfl_up(prev, 1);
				if (!lane) np = first;
				if (!__any(np != prev_in)) break;
				prev_in = np;
			}
			uint2 w;
			w.x = (uint32_t)(uint16_t)(ov[0] + st[0]) | ((uint32_t)(uint16_t)(ov[1] + st[1]) << 16); w.y = (uint32_t)(uint16_t)(ov[2] + st[2]) | ((uint32_t)(uint16_t)(ov[3] + st[3]) << 16);
			if (!ANA) *reinterpret_cast<uint2 *>(jp + (size_t)r * W + c0) = w;
			else {                                                     /* analysis, first direction, of the row in hand: into my own column r */
				int lo[2], hi[2];
				ana_row_quad(w.x, w.y, lane, lo, hi);
				int16_t *x = A + (2 * lane) * LS + r;
				x[0] = (int16_t)lo[0]; x[LS] = (int16_t)lo[1]; x[HLF * LS] = (int16_t)hi[0]; x[(HLF + 1) * LS] = (int16_t)hi[1];
			}
		}
		if (ANA) {
			lds_barrier();                                         /* the transposed first-direction plane */
			int16_t *save = saveb + (size_t)img * save_stride;
			const int rr = lane >> 5, c8 = lane & 31;              /* the copies: two rows a turn, a lane eight cells */
#pragma unroll 1
			for (int i = 0; i < 8; i++) {                          /* my rows c, c + 1 = two columns of the first-direction plane (filters.c:88-287) */
				const int c = r0 + 2 * i;
				const uint32_t *g = reinterpret_cast<const uint32_t *>(A + (c + rr) * LS + 8 * c8);
				if (!LEAN) *reinterpret_cast<uint4 *>(jp + (size_t)(c + rr) * W + 8 * c8) = make_uint4(g[0], g[1], g[2], g[3]);
				uint32_t Ew[PPL], Ow[PPL];
				int lo[PPL][2], hi[PPL][2];
#pragma unroll
				for (int u = 0; u < PPL; u++) {                        /* a dword of row c holds column c's even and odd cell: regrouped into ana_col_pair's two columns side by side */
					const uint32_t a = reinterpret_cast<const uint32_t *>(A + c * LS)[lane + 64 * u], b = reinterpret_cast<const uint32_t *>(A + (c + 1) * LS)[lane + 64 * u];
					Ew[u] = (a & 0xFFFFu) | (b << 16); Ow[u] = (a >> 16) | (b & 0xFFFF0000u);
				}
				ana_col_pair<PPL, HLF>(Ew, Ow, c < HLF, lane, lo, hi);
				asm volatile("" ::: "memory");                         /* (the rows are read as dwords and written as shorts: the compiler keeps the order) */
#pragma unroll
				for (int h = 0; h < 2; h++) {
					int16_t *x = A + (c + h) * LS;
#pragma unroll
					for (int u = 0; u < PPL; u++) { x[lane + 64 * u] = (int16_t)lo[u][h]; x[HLF + lane + 64 * u] = (int16_t)hi[u][h]; }
				}
				asm volatile("" ::: "memory");
				const uint4 w = make_uint4(g[0], g[1], g[2], g[3]);   /* rows c, c + 1 of the coefficient block (written by this wavefront: LDS operations of a wavefront keep their order) */
				if (!LEAN || c < HLF) *reinterpret_cast<uint4 *>(p + (size_t)(c + rr) * W + 8 * c8) = w;   /* (LEAN: the rows the LL2 emission reads; c is the wavefront's) */
				*reinterpret_cast<uint4 *>(save + (size_t)(c + rr) * H + 8 * c8) = w;   /* Y13 (:623-631) */
			}
		}
		lds_barrier();                                             /* the block is done with before the next one moves in */
	}
}
void nhw_launch_l2_recon(Plane<int16_t> jpeg, Plane<int16_t> proc, Plane<int16_t> ll1, Plane<int16_t> l2save /* not empty: + the level-2 analysis of the pre-compensated block and its copy (rows of H cells) */, int n, hipStream_t s,
                         bool lean /* with l2save: the stores nothing reads behind a production batch's kernel are left out (k_l2_recon, LEAN) */)
{
	assert(jpeg.pitch == proc.pitch && (!lean || l2save.p));
	(!l2save.p ? k_l2_recon<false> : lean ? k_l2_recon<true, true> : k_l2_recon<true>)<<<n < 256 ? n : 256, 1024, H * (H + 2) * sizeof(int16_t) + 288, s>>>(jpeg.p, proc.p, jpeg.pitch, ll1.p, ll1.pitch, n, l2save.p, l2save.pitch);
}

/* Both closed loops of a chroma component on one LDS residency of its 128 x 128 level-2 block (nhw_encoder.c:2310-2370 for U, :2623-2680 for V):
 * level-2 analysis, dequantiser simulation 1, synthesis, the LL1 pre-compensation (chroma_p3_par), analysis, simulation 2, synthesis.  As seven
 * kernels the 32 KB block went to HBM and back seven times (4.7 GB per 4096 images, both components); here the LL1 copy comes in once and two
 * blocks go out: the coefficients behind the second analysis (cl2save) and the second reconstruction (the upper left of cproc).
 *   * The staged kernels transpose in every filterbank call (ana: proc[c][k] from column c; syn: proc[c][.] from column c again) and the
 *     pointwise passes in between work on the transposed plane.  In LDS nothing is transposed: cell (r, j) of the coefficient plane sits at
 *     A[j][r], so a row of the coefficient plane (what a wavefront of the simulation owns) is a column of A -- 65 dwords apart, no bank conflicts --
 *     and after the synthesis' second direction A is the reconstruction in natural orientation.
 *   * A wavefront owns 16 rows in the row phases (synthesis second direction -> pre-compensation -> analysis first direction, a row at a time in
 *     registers) and 16 columns in the column phases (analysis second direction -> simulation -> synthesis first direction): every pass reads its
 *     line into registers before it writes it, and what it reads was written by the same wavefront or lies behind a barrier.  Four barriers.
 *   * The original LL1 rows are read a second time for the pre-compensation, in the row phases' own layout, a window of four rows ahead: kept
 *     in registers from the first load (16 dwords a thread) the kernel does not fit the 64 registers that four workgroups a CU allow, and
 *     the compiler spills.  The second read does reach HBM (2 x FETCH_SIZE + WRITE_SIZE: 1.11 GB per 4096 images and both components, 0.8 without it).
 *   * Cells outside the block: column 128 of cproc's rows (a level-1 detail cell, the right neighbour of column 127 in all three pointwise
 *     passes), the first LL1 cell of the row behind a wavefront's last, and the cell behind cll1 (chroma_ll1_neighbour: worked out here, and still
 *     written for chroma_p5_par).  All are constant during the sequence and fetched at the start.
 *   * What is no longer stored: the block of cjpeg (read by nobody behind the head: chroma_p5_par, ll_code_chroma_par and final_phase_par take
 *     cproc, cll1 and cl2save) and the three earlier versions of cproc's block.  Cells outside the block are not touched.
 * The stage checks (nhw_debug_stop_after) run the seven kernels, which leave every intermediate plane. */
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_chroma_loops(int16_t *__restrict__ cprocb, size_t plane_stride, int16_t *__restrict__ cll1b, size_t ll1_stride,
                                                      int16_t *__restrict__ saveb, size_t save_stride, const uint8_t *__restrict__ pub, size_t pu_stride,
                                                      int q, int comp, int compat)
{
	constexpr int S = H / 2, LS = S + 2, HLF = S / 2;
	__shared__ __attribute__((aligned(16))) int16_t A[S * LS];
	const int t = threadIdx.x, lane = t & 63, wv = t >> 6, img = blockIdx.x, r0 = wv * 16;
	int16_t *p = cprocb + (size_t)img * plane_stride, *o = cll1b + (size_t)img * ll1_stride, *save = saveb + (size_t)img * save_stride;
	const uint8_t *pu = pub + (size_t)img * pu_stride;
	const int behind = compat ? (int16_t)(pu[32768] | (pu[32769] << 8)) : 0;   /* chroma_ll1_neighbour */
	auto ll1_row = [&](int i) { return reinterpret_cast<const uint32_t *>(o + (size_t)(r0 + (i < 16 ? i : 15)) * S)[lane]; };   /* row i of my 16 rows of LL1, a lane cells 2 lane, 2 lane + 1 */
	uint32_t w0 = ll1_row(0), w1 = ll1_row(1), w2 = ll1_row(2), w3 = ll1_row(3);   /* a window of four rows, requested three rows ahead of their use (rolled loops: unrolled, the compiler interleaves the rows and spills) */
	int side = 0;                                                  /* lane l < 16: column 128 of row (= coefficient row) r0 + l of cproc; lane 16: the LL1 cell behind my last row */
	if (lane < 16) side = p[(size_t)(r0 + lane) * H + S];
	else if (lane == 16) side = wv < 7 ? o[(size_t)(r0 + 16) * S] : behind;
	if (t == 0) o[Q >> 2] = (int16_t)behind;
	auto ana_row = [&](int16_t *x, uint32_t w) {                   /* analysis, first direction, of a row in registers */
		const uint32_t Dw[1] = { w };
		int lo[1], hi[1];
		ana_row_pair<1>(Dw, lane, lo, hi);
		x[lane] = (int16_t)lo[0]; x[HLF + lane] = (int16_t)hi[0];
	};
	auto columns = [&](const int loop /* dequant_sim_chroma_par's: 1 = the first simulation */, int16_t *out) {
		for (int i = 0; i < 8; i++) {                              /* analysis, second direction, two columns at a time, in place: cell (c, k) of the coefficient plane at A[k][c] */
			const int c = r0 + 2 * i;
			uint32_t Ew[1], Ow[1];
			int lo[1][2], hi[1][2];
			Ew[0] = *reinterpret_cast<const uint32_t *>(A + (2 * lane) * LS + c); Ow[0] = *reinterpret_cast<const uint32_t *>(A + (2 * lane + 1) * LS + c);
			ana_col_pair<1, HLF>(Ew, Ow, c < HLF, lane, lo, hi);
			*reinterpret_cast<uint32_t *>(A + lane * LS + c) = (uint32_t)(uint16_t)lo[0][0] | ((uint32_t)(uint16_t)lo[0][1] << 16);
			*reinterpret_cast<uint32_t *>(A + (HLF + lane) * LS + c) = (uint32_t)(uint16_t)hi[0][0] | ((uint32_t)(uint16_t)hi[0][1] << 16);
			if (out)
#pragma unroll
				for (int h = 0; h < 2; h++) { int16_t *d = out + (size_t)(c + h) * S; d[lane] = (int16_t)lo[0][h]; d[HLF + lane] = (int16_t)hi[0][h]; }
		}
		for (int i = 0; i < 16; i++) {                             /* dequant_sim_chroma_par on coefficient row r, then the synthesis' first direction along it */
			const int r = r0 + i, col0 = r < HLF ? HLF : 0;
			int16_t *x = A + r;
			int v[3] = { x[lane * LS], x[(HLF + lane) * LS], __builtin_amdgcn_readlane(side, i) };
			int ll = v[0];                                             /* r < 64: the LL2 cell (r, lane) */
			if (loop) {
				if (q <= 15) ll = (int16_t)((ll & 0xFFFC) + 1);
				else if ((r == 0) == (bool)(lane & 1)) ll = clear_bit0(ll);   /* row 0: the odd columns lose bit 0, every other row: the even ones */
			} else if (ll > 0 && ll < 256) ll = clear_bit0(ll);
			if (col0) v[0] = 0;
			uint64_t pair[2] = { 0, 0 };
			if (!loop) {
				const uint64_t m0 = __ballot(v[0] == -7 || v[0] == -8), m1 = __ballot(v[1] == -7 || v[1] == -8);
				const M4 m = M4{ { col0 ? 0 : m0, m1, 0, 0 } };
				const M4 fired = alt_runs(m & dn1(m) & col_range(col0, S - 2));
				const M4 both = fired | up1(fired);
				pair[0] = both.w[0]; pair[1] = both.w[1];
			}
			int dv[2] = { ll, 0 };
			for (int k = col0 ? 1 : 0; k < 2; k++) {
				int a = v[k];
				const int nx = right_of(v, k, 3, 1, lane);
				if (a < 0) {
					a = -a;
					if (nx < 0 && nx > -8) { if ((a & 7) < 6) a &= 0xFFF8; }
					else { if ((a & 7) < 7) a &= 0xFFF8; }
					a = -a;
				}
				dv[k] = ((pair[k] >> lane) & 1) ? -11 : dequant_value(a);
			}
			x[lane * LS] = (int16_t)dv[0]; x[(HLF + lane) * LS] = (int16_t)dv[1];
			int e, od;
			syn_pair<S>(x, LS, lane, false, &e, &od);
			x[(2 * lane) * LS] = (int16_t)e; x[(2 * lane + 1) * LS] = (int16_t)od;
		}
	};
	auto p3_step = [&](int d, int nx) {                            /* chroma_p3_par */
		int step = 0;
		if (d > 10) step = -6; else if (d > 7) step = -3; else if (d > 4) step = -2; else if (d > 3) step = -1;
		else if (d > 2 && (comp ? nx > 0 : nx >= 0)) step = -1;
		else if (d < -10) step = 6; else if (d < -7) step = 3; else if (d < -4) step = 2; else if (d < -3) step = 1;
		else if (d < -2 && (comp ? nx < 0 : nx <= 0)) step = 1;
		return step;
	};
#pragma unroll 1
	for (int i = 0; i < 16; i++) { ana_row(A + (r0 + i) * LS, w0); w0 = w1; w1 = w2; w2 = w3; w3 = ll1_row(i + 4); }
	lds_barrier();
	columns(1, nullptr);
	w0 = ll1_row(0); w1 = ll1_row(1); w2 = ll1_row(2); w3 = ll1_row(3);
	lds_barrier();
#pragma unroll 1
	for (int i = 0; i < 16; i++) {                                 /* synthesis, second direction -> the pre-compensated LL1 row -> analysis, first direction */
		int16_t *x = A + (r0 + i) * LS;
		int e, od;
		syn_pair<S>(x, 1, lane, true, &e, &od);
		const uint32_t ow = w0, ow_next = w1;
		w0 = w1; w1 = w2; w2 = w3; w3 = ll1_row(i + 4);
		const int oc0 = (int16_t)(ow & 0xFFFF), oc1 = (int)ow >> 16;
		int pn = __builtin_amdgcn_update_dpp(0, e, 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
		int on = (int16_t)(__builtin_amdgcn_update_dpp(0, (int)ow, 0x130, 0xF, 0xF, false) & 0xFFFF);
		if (lane == 63) {                                          /* behind column 127: column 128 of the row; the first LL1 cell of the next row */
			pn = __builtin_amdgcn_readlane(side, i);
			on = i < 15 ? (int16_t)(__builtin_amdgcn_readlane((int)ow_next, 0) & 0xFFFF) : __builtin_amdgcn_readlane(side, 16);
		}
		const int d0 = e - oc0, d1 = od - oc1, d2 = pn - on;
		ana_row(x, (uint32_t)(uint16_t)(oc0 + p3_step(d0, d1)) | ((uint32_t)(uint16_t)(oc1 + p3_step(d1, d2)) << 16));
	}
	lds_barrier();
	columns(0, save);
	lds_barrier();
#pragma unroll 1
	for (int i = 0; i < 16; i++) {                                 /* synthesis, second direction: the reconstruction, row r0 + i of cproc */
		int e, od;
		syn_pair<S>(A + (r0 + i) * LS, 1, lane, true, &e, &od);
		reinterpret_cast<uint32_t *>(p + (size_t)(r0 + i) * H)[lane] = (uint32_t)(uint16_t)e | ((uint32_t)(uint16_t)od << 16);
	}
}
void nhw_launch_chroma_loops(Plane<int16_t> cproc, Plane<int16_t> cll1, Plane<int16_t> cl2save, Plane<const uint8_t> pu, int q, int comp, int compat, int n, hipStream_t s)
{
	k_chroma_loops<<<n, 512, 0, s>>>(cproc.p, cproc.pitch, cll1.p, cll1.pitch, cl2save.p, cl2save.pitch, pu.p, pu.pitch, q, comp, compat);
}

/* rows x cols block of shorts between two strided planes, every image of the batch: a workgroup an image, 16 bytes a thread and turn, four
 * turns in flight (cols and both pitches are multiples of 8, every row 16-byte aligned: asserted by the launcher).  Until round 5 a thread
 * moved ONE short and a workgroup one row: 1.6 ms for the 128 KB block of 4096 images (q <= 12), 0.7 TB/s. */
__global__ __launch_bounds__(256) void k_copy_block(const int16_t *__restrict__ src, size_t src_plane, int src_row,
                                                    int16_t *__restrict__ dst, size_t dst_plane, int dst_row, int rows, int cols)
{
	const int16_t *sp = src + (size_t)blockIdx.x * src_plane;
	int16_t *dp = dst + (size_t)blockIdx.x * dst_plane;
	const int per = cols >> 3, n = rows * per;
	for (int i0 = threadIdx.x; i0 < n; i0 += 4 * 256) {
		uint4 v[4];
#pragma unroll
		for (int u = 0; u < 4; u++) { const int i = i0 + u * 256; if (i < n) v[u] = reinterpret_cast<const uint4 *>(sp + (size_t)(i / per) * src_row)[i % per]; }
#pragma unroll
		for (int u = 0; u < 4; u++) { const int i = i0 + u * 256; if (i < n) reinterpret_cast<uint4 *>(dp + (size_t)(i / per) * dst_row)[i % per] = v[u]; }
	}
}

/* dynamic LDS per phase: number of 256-row column tiles (TLS shorts per row) the phase stages at once */
static size_t phase_lds(int ph)
{
	const size_t tile = (size_t)NT * TLS * sizeof(int16_t);
	switch (ph) {
	case PH_L2: return 3 * 32 * 33 + 32;                          /* the three 32 x 32 blocks of steps of Y8 (Y9 works on the plane itself) */
	case PH_L3: return LL_LDS_BYTES;
	case PH_LLC: return LLC_LDS_BYTES;
	case PH_L4A: return RF_LDS_BYTES > (NT + 2) * TLS * sizeof(int16_t) ? RF_LDS_BYTES : (size_t)(NT + 2) * TLS * sizeof(int16_t);
	case PH_L4B: return (size_t)(NT + 2) * TLS * sizeof(int16_t);
	case PH_L4C: return 0;                                         /* Y26 is pointwise, Y27 a wavefront per row straight on the plane */
	case PH_L4D: return SL_LDS_BYTES;                              /* Y31 on the symbol list: the non-zero map and the slices' value offsets in stream order (the dense form of the stage checks: 4608 bytes of them for its list of run starts) */
	case PH_C5: return CQ_LDS_BYTES > 32 * 130 * 2 + (32 * 128 + 258) * 2 ? CQ_LDS_BYTES : 32 * 130 * 2 + (32 * 128 + 258) * 2;   /* the quantiser's parked rows; the marks' and the emission's tables */
	default: return 0;
	}
}

/* per device, from nhw_enc_create (see nhw_front_set_attrs) */
int nhw_tail_set_attrs(const char **where)
{
#define SETATTR(fn) do { const hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void *>(&fn), hipFuncAttributeMaxDynamicSharedMemorySize, 100 << 10); \
                         if (e_ != hipSuccess) { *where = "hipFuncSetAttribute(" #fn ", MaxDynamicSharedMemorySize)"; return (int)e_; } } while (0)
	SETATTR(k_phase<PH_L1>); SETATTR(k_phase<PH_L2>); SETATTR(k_phase<PH_L3>); SETATTR(k_phase<PH_C5>); SETATTR(k_chroma_tail);
	for (const void *fn : { reinterpret_cast<const void *>(&k_l2_recon<false>), reinterpret_cast<const void *>(&k_l2_recon<true>), reinterpret_cast<const void *>(&k_l2_recon<true, true>) }) {
		const hipError_t e_ = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(H * (H + 2) * sizeof(int16_t) + 288));
		if (e_ != hipSuccess) { *where = "hipFuncSetAttribute(k_l2_recon, MaxDynamicSharedMemorySize)"; return (int)e_; }
	}
#undef SETATTR
	return 0;
}

void nhw_launch_phase(int ph, const NhwWs &ws, int comp, hipStream_t s)
{
	const dim3 g(ws.n), b(256);
	const size_t lds = phase_lds(ph);
#define PHASE(P) case P: k_phase<P><<<g, b, lds, s>>>(ws, comp); break
	switch (ph) {
	PHASE(PH_L1); PHASE(PH_L2); PHASE(PH_L3);
	case PH_L4A: if (ws.q >= 17) k_l4a<<<g, b, lds, s>>>(ws); else k_phase<PH_L4A><<<g, b, lds, s>>>(ws, comp); break;
	PHASE(PH_L4B); PHASE(PH_L4C);
	case PH_L4D: if (NHW_DENSE_STREAM || ws.dbg) k_phase<PH_L4D><<<g, b, lds, s>>>(ws, comp); else k_y31<<<g, 512, lds, s>>>(ws); break;
	PHASE(PH_LLC); PHASE(PH_L4C2); PHASE(PH_C0); PHASE(PH_C2); PHASE(PH_C3); PHASE(PH_C4); PHASE(PH_C5);
	}
#undef PHASE
}
void nhw_launch_chroma_tail(const NhwWs &ws, int comp, bool once, hipStream_t s)
{
	if (once && !ws.dbg) k_chroma_tail<<<ws.n, 256, CT_LDS_BYTES, s>>>(ws, comp);
	else nhw_launch_phase(PH_C5, ws, comp, s);
}
void nhw_launch_pack_chroma(const NhwWs &ws, hipStream_t s)
{
	k_pack_chroma<<<ws.n, 256, PK_LDS_BYTES, s>>>(ws);
}
void nhw_launch_final(const NhwWs &ws, uint8_t *out, uint32_t *sizes, int32_t *status, hipStream_t s, bool chroma_packed)
{
	if (!chroma_packed) nhw_launch_pack_chroma(ws, s);
	k_final<<<ws.n, 256, PK_LDS_BYTES, s>>>(ws, out, sizes, status);
}

void nhw_launch_copy_block(Plane<const int16_t> src, int src_row, Plane<int16_t> dst, int dst_row, int rows, int cols, int n, hipStream_t s)
{
	if ((cols | src_row | dst_row) & 7 || (src.pitch | dst.pitch) & 7 || ((uintptr_t)src.p | (uintptr_t)dst.p) & 15) { fprintf(stderr, "nhw_launch_copy_block: block not 16-byte aligned\n"); abort(); }
	k_copy_block<<<n, 256, 0, s>>>(src.p, src.pitch, src_row, dst.p, dst.pitch, dst_row, rows, cols);
}
