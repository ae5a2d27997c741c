/*
 * nhw_enc.hip -- the encoder handle of libnhwhip.so's C ABI (include/nhw_hip.h): workspace, batch driver, hipEvent timing, stage entry
 * points, debug hooks (include/nhw_hip_debug.h).  gfx950 / ROCm only.
 *
 * Batch driver = encode_image (rcanut/nhwcodec encoder/nhw_encoder.c:103-2878) re-cut as a sequence of
 * batch-wide kernel launches: every launch processes the same stage of all n images.
 */
#include "nhw_enc.h"
#include "nhw_enc_plan.h"
#include "nhw_grey.h"

thread_local std::string nhw_enc_err;
extern "C" const char *nhw_last_error(void) { return nhw_enc_err.c_str(); }

static const size_t k_buf_bytes[B_COUNT] = {
	/* JPEG   */ 8 * Q, /* PROC */ 8 * Q, /* PU */ Q, /* PV */ Q, /* CJPEG */ 2 * Q, /* CPROC */ 2 * Q,
	/* LL1    */ 2 * Q, /* L2SAVE */ 2 * Q, /* CLL1 */ Q / 2, /* CL2SAVE */ Q / 2, /* KEEP */ 4 * Q, /* FIRST */ 2 * Q,
	/* BAND   */ 2 * Q, /* HS */ 4 * Q + 256, /* KMAP */ 8 * Q, /* ROWMAP (unused) */ 16, /* ROWSTATE */ 512, /* SCAN */ 6 * Q,
	/* LLBYTES*/ 24832, /* LLFULL */ 16384, /* EXW */ 16384 + 256, /* LLCOMP */ 32768, /* LLWORD */ 16384, /* LLMEM */ 32768,
	/* RES4   */ 8192, /* RAW */ 2 * Q + 1024, /* PAY */ 2 * Q + 256, /* CC */ 2 * Q + 1024, /* HALF */ 2 * Q + 1024, /* TMP16 */ Q / 2,
	/* R1     */ Q + 64, 8192 + 64, 16384 + 64, /* R3 */ Q + 64, 8192 + 64, 16384 + 64, /* R5 */ Q + 64, 8192 + 64, 16384 + 64,
	/* R6     */ 2 * Q + 1024, 16384 + 64, 16384 + 64, /* CHARRES */ 2048 + 64, /* QSET3 */ 8 * Q + 64,
	/* RESU64 */ 512, /* RESV64 */ 512, /* PACKET */ 320000, /* BOOK1 */ 768, /* BOOK2 */ 768, /* SEL1 */ 16384 + 64, /* SEL2 */ 16384 + 64,
	/* S1     */ 131072, /* S2 */ 131072, /* HIST */ 5632, /* META */ 256, /* PROF */ 512, /* ROWFLAG (unused) */ 16, /* SEGMAP (unused) */ 16, /* STALE */ (8 + 9 * 512) * 2,
	/* NZQ (32 x 128 words of 64 bits + 33 flush bases) */ Q / 2 + 256, /* NZS */ Q / 2, /* VOFF */ Q / 4, /* VALS (every symbol non-zero: 4 Q) */ 4 * Q,
	/* CNZQ (16 flushes x 64 lanes x 2 words of 64 bits + 17 flush bases) */ Q / 4 + 256, /* CVALS */ 2 * Q,
	/* CJPEG_V */ 2 * Q, /* CPROC_V */ 2 * Q, /* CLL1_V */ Q / 2, /* CL2SAVE_V */ Q / 2, /* UBYTES */ Q,
	/* LOWTAB (quality 1..16: pass A's five candidate masks, 64 bytes each, for every row) */ 320 * 512,
	/* CPACK */ sizeof(NhwChromaPack), /* CPACKET (80000 words, like PACKET) */ 320000
};

static size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

extern "C" int nhw_quality_supported(int quality) { return quality >= 1 && quality <= 23; }

/* L_quality (nhw_grey.h) into out[0 .. 256).  Host only: no handle, no GPU call */
extern "C" int nhw_grey_luma_table(int quality, int16_t out[256])
{
	if (!out || !nhw_quality_supported(quality)) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	for (int g = 0; g < 256; g++) out[g] = (int16_t)nhw_grey_luma(quality, g);
	return NHW_OK;
}

extern "C" int nhw_enc_set_compat(nhw_enc *e, int mode)
{
	if (!e || (mode != NHW_COMPAT_CANONICAL && mode != NHW_COMPAT_GLIBC_ONESHOT)) return NHW_E_ARG;
	if (e->ws.compat != mode && mode == NHW_COMPAT_CANONICAL) {      /* the compatibility mode writes behind ll1 and the level-2 copy: give the guards their zeros back */
		HIPCHK(hipSetDevice(e->device));
		HIPCHK(hipDeviceSynchronize());
		HIPCHK(hipMemset2D(e->ws.plane<uint8_t>(B_LL1).p + 2 * Q, e->ws.plane<uint8_t>(B_LL1).bytes(), 0, 1024, (size_t)e->max_batch));
		HIPCHK(hipMemset2D(e->ws.plane<uint8_t>(B_L2SAVE).p + 2 * Q, e->ws.plane<uint8_t>(B_L2SAVE).bytes(), 0, 256, (size_t)e->max_batch));
	}
	e->ws.compat = mode;
	return NHW_OK;
}

/* device bytes per image of the host path's staging (nhw_enc_batch / nhw_enc_synth_batch): input slot, output slot, compacted output */
#define HOST_PATH_BYTES ((size_t)NHW_IMG_BYTES + 2 * (size_t)NHW_OUT_STRIDE + 24)
extern "C" int nhw_enc_create_ex(int device, int max_batch, unsigned flags, nhw_enc **out)
{
	if (!out || max_batch < 1 || max_batch > 65535 || (flags & ~(unsigned)NHW_CREATE_DEVICE_ONLY)) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	const bool host_staging = !(flags & NHW_CREATE_DEVICE_ONLY);
	HIPCHK(hipSetDevice(device));
	nhw_enc *e = new nhw_enc();
	memset(e, 0, sizeof *e);
	e->device = device; e->max_batch = max_batch;
	size_t total = 0;
	for (int b = 0; b < B_COUNT; b++) {
		e->ws.stride[b] = round_up(k_buf_bytes[b] + GUARD, 256);
		e->ws.off[b] = total + GUARD;
		total += GUARD + e->ws.stride[b] * (size_t)max_batch;
	}
	const int rc = [&]() -> int {                                  /* a failure half-way leaves nothing behind: the handle is destroyed below */
		size_t free_b = 0, total_b = 0;
		HIPCHK(hipMemGetInfo(&free_b, &total_b));
		const size_t need = total + (host_staging ? HOST_PATH_BYTES * (size_t)max_batch : 0);
		if (need > free_b) {                                       /* 7.4 MB of workspace (+ 1.8 MB of host-path staging) per image: say so instead of failing inside hipMalloc */
			char b[200];
			snprintf(b, sizeof b, "encoder workspace for max_batch %d needs %zu MiB (%.1f MiB per image), %zu MiB of HBM are free", max_batch, need >> 20, (double)need / max_batch / 1048576.0, free_b >> 20);
			nhw_enc_err = b;
			return NHW_E_ARG;
		}
		{ const char *where = ""; int rc_ = nhw_front_set_attrs(&where); if (!rc_) rc_ = nhw_tail_set_attrs(&where);   /* before anything is launched on this device */
		  if (rc_) { nhw_enc_err = std::string(where) + " -> " + hipGetErrorString((hipError_t)rc_); return NHW_E_HIP; } }
		HIPCHK(hipMalloc((void **)&e->ws.base, total));
		HIPCHK(hipMemset(e->ws.base, 0, total));       /* guards must be zero; they are never written afterwards */
		HIPCHK(hipStreamCreate(&e->own_stream));
		for (int i = 0; i < EV_COUNT; i++) HIPCHK(hipEventCreate(&e->ev[i]));
		for (int i = 0; i < 4; i++) HIPCHK(hipStreamCreateWithFlags(&e->part_stream[i], hipStreamNonBlocking));
		for (int i = 0; i < PE_COUNT; i++) HIPCHK(hipEventCreateWithFlags(&e->part_ev[i], hipEventDisableTiming));
		for (int i = 0; i < 4; i++) HIPCHK(hipStreamCreateWithFlags(&e->low_stream[i], hipStreamNonBlocking));
		for (int i = 0; i < LOW_EV_COUNT; i++) HIPCHK(hipEventCreateWithFlags(&e->low_ev[i], hipEventDisableTiming));
		HIPCHK(hipStreamCreateWithFlags(&e->ll_stream, hipStreamNonBlocking));
		for (int i = 0; i < LL_EV_COUNT; i++) HIPCHK(hipEventCreateWithFlags(&e->ll_ev[i], hipEventDisableTiming));
		for (int i = 0; i < 2; i++) HIPCHK(hipEventCreate(&e->fit_ev[i]));
		HIPCHK(hipHostMalloc((void **)&e->h_fit_count, sizeof(int), hipHostMallocDefault));
		/* the host path's staging buffers, for the whole of max_batch, now: allocated on the first nhw_enc_batch they made that call twice as
		 * slow as the ones behind it (gigabytes of hipMalloc inside the timed region of whoever measured it).  A caller that only ever hands over
		 * device buffers says NHW_CREATE_DEVICE_ONLY and does not pay for them; should it call the host path after all, that call allocates. */
		return host_staging ? host_buffers(e, max_batch) : NHW_OK;
	}();
	if (rc != NHW_OK) { nhw_enc_destroy(e); return rc; }
	/* the schedule switches: (name, default), then (lowest, highest, what a value outside them means) */
	auto env = [](const char *name, int dflt) { const char *p = getenv(name); return p ? atoi(p) : dflt; };
	auto within = [](int v, int lo, int hi, int other) { return v < lo || v > hi ? other : v; };
	e->parts = within(env("NHW_PARTS", 1), 1, 4, 1);   /* sub-batches on streams of their own (NHW_PARTS=2..4) bought 4 % while the tail kernels were latency-bound; they no longer do */
	e->low_parts = within(env("NHW_LOW_PARTS", 2), 1, 4, 1);
	e->low_chroma = within(env("NHW_LOW_CHROMA", 2), 0, 2, 2);
	e->chroma_fork = env("NHW_CHROMA_FORK", 1) != 0;
	e->lists_fork = env("NHW_LISTS_FORK", 1) != 0;
	e->ll_fork = env("NHW_LL_FORK", 1) != 0;
	e->quant_join = env("NHW_QUANT_JOIN", 1) != 0;
	e->y5_fork = env("NHW_Y5_FORK", 1) != 0;
	e->ll2_once = env("NHW_LL2_ONCE", 1) != 0;
	e->quant_marks = env("NHW_QUANT_MARKS", 1) != 0;
	e->chroma_tail_once = env("NHW_CHROMA_TAIL_ONCE", 1) != 0;
	e->pack_fork = within(env("NHW_PACK_FORK", 2), 0, 2, 2);
	*out = e;
	return NHW_OK;
}

extern "C" int nhw_enc_create(int device, int max_batch, nhw_enc **out) { return nhw_enc_create_ex(device, max_batch, 0u, out); }

extern "C" void nhw_enc_destroy(nhw_enc *e)
{
	if (!e) return;
	(void)hipSetDevice(e->device);
	(void)hipDeviceSynchronize();
	if (e->ws.base) (void)hipFree(e->ws.base);
	dev_free(host_set(e, 0));
	dev_free({ dev_buf(e->d_tensor_bytes, 0) });
	dev_free(fit_set(e));
	dev_free(fit_sse_set(e));
	for (GrowBuf *g : { &e->pic_px, &e->pic_desc, &e->pfit_px, &e->pfit_aux, &e->pic_resized }) nhw_grow_free(*g);
	if (e->h_fit_count) (void)hipHostFree(e->h_fit_count);
	for (int i = 0; i < 2; i++) if (e->fit_ev[i]) (void)hipEventDestroy(e->fit_ev[i]);
	for (int i = 0; i < EV_COUNT; i++) if (e->ev[i]) (void)hipEventDestroy(e->ev[i]);
	if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
	for (int i = 0; i < 4; i++) if (e->part_stream[i]) (void)hipStreamDestroy(e->part_stream[i]);
	for (int i = 0; i < PE_COUNT; i++) if (e->part_ev[i]) (void)hipEventDestroy(e->part_ev[i]);
	for (int i = 0; i < 4; i++) if (e->low_stream[i]) (void)hipStreamDestroy(e->low_stream[i]);
	for (int i = 0; i < LOW_EV_COUNT; i++) if (e->low_ev[i]) (void)hipEventDestroy(e->low_ev[i]);
	if (e->ll_stream) (void)hipStreamDestroy(e->ll_stream);
	for (int i = 0; i < LL_EV_COUNT; i++) if (e->ll_ev[i]) (void)hipEventDestroy(e->ll_ev[i]);
	delete e;
}

int host_buffers(nhw_enc *e, int n)
{
	if (e->conv_cap >= n) return NHW_OK;
	dev_free(host_set(e, 0));
	e->conv_cap = 0;
	const int rc = dev_alloc(host_set(e, (size_t)n), nullptr, n, nhw_enc_err);
	if (rc == NHW_OK) e->conv_cap = n;
	return rc;
}

/* The executor of a plan's steps (nhw_enc_plan.h): every kernel step is one call of its launcher with the planes of the view ws, every event step
 * one call of the runtime.  The planner decides what is launched, in which order and on which stream; nothing here does. */
struct EncIo { const void *d_bgr; void *d_out; uint32_t *d_sizes; int32_t *d_status; bool grey; };   /* the caller's arrays (a stage hook: none, its plans have no step that takes them); grey: d_bgr holds grey pictures, one byte a pixel */
static_assert(EE_START == EV_START && EE_FRONT == EV_FRONT && EE_LUMA == EV_LUMA && EE_CHROMA == EV_CHROMA && EE_END == EV_END && EE_COLOR == EV_COLOR && EE_PREFILTER == EV_PREFILTER,
              "the plan's stamps are the handle's timing events");
static hipEvent_t enc_event(nhw_enc *e, int ev, int low_parts_used)
{
	switch (ev) {
	case EE_LUMA_LIST: return e->part_ev[PE_LUMA_LIST];
	case EE_CHROMA_DONE: return e->part_ev[PE_CHROMA];
	case EE_LISTS_FORK: return e->part_ev[PE_LISTS_FORK];
	case EE_LISTS: return e->part_ev[PE_LISTS];
	case EE_PART_FRONT: return e->part_ev[PE_FRONT];
	case EE_LL_FORK: return e->ll_ev[LL_EV_FORK];
	case EE_LL_DONE: return e->ll_ev[LL_EV_DONE];
	case EE_Y5_FORK: return e->ll_ev[LL_EV_Y5_FORK];
	case EE_Y5_DONE: return e->ll_ev[LL_EV_Y5_DONE];
	case EE_PACK_FORK: return e->ll_ev[LL_EV_PACK_FORK];
	case EE_PACK_DONE: return e->ll_ev[LL_EV_PACK_DONE];
	case EE_LOW_PASS_A: return e->low_ev[low_ev_pass_a(low_parts_used - 1)];
	default: assert(ev < EV_COUNT); return e->ev[ev];
	}
}
static int run_steps(nhw_enc *e, const NhwWs &ws, const EncPlan &plan, const EncIo &io, hipStream_t s)
{
	const int q = ws.q, n = ws.n;
	hipStream_t const stream[ES_COUNT] = { s, e->part_stream[0], e->part_stream[1], e->ll_stream };
	const Plane<int16_t> jpeg = ws.plane<int16_t>(B_JPEG), proc = ws.plane<int16_t>(B_PROC), ll1 = ws.plane<int16_t>(B_LL1), l2save = ws.plane<int16_t>(B_L2SAVE);
	const Plane<int16_t> yin = ws.plane<int16_t>(B_KMAP);
	const Plane<uint8_t> pu = ws.plane<uint8_t>(B_PU), pv = ws.plane<uint8_t>(B_PV);
	const NhwAnalysis l2{ jpeg, proc, n, W, H, 1 };
	assert(ws.dbg == plan.dbg && ws.split_chroma == plan.split_chroma && ws.defer_verbatim == plan.defer_verbatim);
	for (int i = 0; i < plan.n; i++) {
		const EncStep &st = plan.step[i];
		hipStream_t const on = stream[st.stream];
		/* a chroma step's component and planes */
		const int comp = st.a != 0;
		const bool vp = st.a == 2;
		const Plane<int16_t> cjpeg = ws.plane<int16_t>(vp ? B_CJPEG_V : B_CJPEG), cproc = ws.plane<int16_t>(vp ? B_CPROC_V : B_CPROC);
		const Plane<int16_t> cll1 = ws.plane<int16_t>(vp ? B_CLL1_V : B_CLL1), cl2save = ws.plane<int16_t>(vp ? B_CL2SAVE_V : B_CL2SAVE);
		const Plane<const uint8_t> bytes = ws.plane<const uint8_t>(comp ? B_PV : B_PU);
		const NhwAnalysis cl2{ cjpeg, cproc, n, H, H / 2, 1 };
		switch (st.op) {
		case ENC_STAMP: HIPCHK(hipEventRecord(e->ev[st.a], on)); break;
		case ENC_RECORD: HIPCHK(hipEventRecord(enc_event(e, st.a, plan.low_parts_used), on)); break;
		case ENC_WAIT: HIPCHK(hipStreamWaitEvent(on, enc_event(e, st.a, plan.low_parts_used), 0)); break;
		case ENC_STAGE: break;
		case ENC_COLOR: (io.grey ? nhw_launch_color_grey : nhw_launch_color)((const uint8_t *)io.d_bgr, n, q, st.a ? yin : jpeg, pu, pv, on); break;
		case ENC_LOW_PREFILTER:
			HIPCHK((hipError_t)nhw_launch_low_prefilter(jpeg, yin, proc, ws.plane<uint8_t>(B_SCAN), ws.plane<uint8_t>(B_KEEP), ws.plane<uint8_t>(B_LOWTAB), q, n, on, st.b ? 32 : 0,
			                                            st.a, e->low_stream, e->low_ev));
			break;
		case ENC_LOW_STALE: nhw_launch_low_stale(proc, ws.plane<uint8_t>(B_STALE), n, on); break;
		case ENC_FRONT: {
			NhwFront f;
			f.q = q; f.n = n; f.y = yin /* quality 17..23, developer builds only: a plane for a dump */; f.st = ws.plane<uint8_t>(B_ROWSTATE);
			f.proc = proc; f.jpeg = jpeg; f.ll1 = ll1; f.switches = (ws.dbg ? 2 : 0) | st.a;
			if (q > 16) { f.bgr = (const uint8_t *)io.d_bgr; f.grey = io.grey; f.pu = pu; f.pv = pv; f.with_prefilter = q < 22; }
			if (q > 21) f.keep = ws.plane<int16_t>(B_KEEP);
			nhw_launch_front_fused(f, on);
			break;
		}
		case ENC_FRONT_STALE: nhw_launch_front_stale(yin, ws.plane<const uint8_t>(B_ROWSTATE), ws.plane<uint8_t>(B_STALE), n, on); break;
		case ENC_C_PREFILTER: nhw_launch_low_prefilter_chroma(bytes, cjpeg, q, n, on); break;
		case ENC_C_WIDEN: nhw_launch_phase(PH_C0, ws, comp, on); break;
		case ENC_C_ANALYSIS1: {
			NhwAnalysis l1 = NhwAnalysis{ cjpeg, cproc, n, H, H, 0 }.saving(cll1, H / 2, ANA_SAVE_LL);
			l1.store = ws.dbg ? ANA_STORE_ALL : ANA_STORE_NO_T_LL_SAVED;
			if (st.b) l1.src8 = bytes;
			nhw_launch_analysis(l1, on);
			break;
		}
		case ENC_C_THIN: nhw_launch_low_chroma_thin(cproc, n, on); break;
		case ENC_C_LOOPS: nhw_launch_chroma_loops(cproc, cll1, cl2save, ws.plane<const uint8_t>(B_PU), q, comp, ws.compat, n, on); break;
		case ENC_C_ANALYSIS2: nhw_launch_analysis(st.b ? cl2.saving(cl2save, H / 2, ANA_SAVE_BLOCK) : cl2, on); break;
		case ENC_C_SIM1: nhw_launch_phase(PH_C2, ws, comp, on); break;
		case ENC_C_SYN: nhw_launch_synthesis(cjpeg, cproc, n, H, H / 2, 0, on); break;
		case ENC_C_PRECOMP: nhw_launch_phase(PH_C3, ws, comp, on); break;
		case ENC_C_SIM2: nhw_launch_phase(PH_C4, ws, comp, on); break;
		case ENC_C_TAIL: nhw_launch_chroma_tail(ws, comp, st.b != 0, on); break;
		case ENC_Y4: {
			NhwAnalysis first = l2.from(ll1, H);
			if (st.a) first.store = ANA_STORE_NO_T;
			nhw_launch_analysis(first, on);
			break;
		}
		case ENC_Y5: nhw_launch_phase(PH_L1, ws, 0, on); break;
		case ENC_DQ1: nhw_launch_wave(WV_DQ1, ws, on); break;
		case ENC_L_SYN1: nhw_launch_synthesis(jpeg, proc, n, W, H, 0, on); break;
		case ENC_Y8: nhw_launch_phase(PH_L2, ws, 0, on); break;
		case ENC_L2_RECON: nhw_launch_l2_recon(jpeg, proc, ll1, st.a ? l2save : Plane<int16_t>{}, n, on, st.b != 0); break;
		case ENC_L_ANALYSIS2: nhw_launch_analysis(st.a ? l2.saving(l2save, H, ANA_SAVE_BLOCK) : l2, on); break;
		case ENC_LOW_LL2: nhw_launch_low_ll2(proc, q, n, on); break;
		case ENC_COPY_BLOCK: nhw_launch_copy_block(proc, W, l2save, H, H, H, n, on); break;
		case ENC_EMIT: nhw_launch_wave(WV_EMIT, ws, on, st.a != 0); break;
		case ENC_LL_CODER: nhw_launch_phase(PH_L3, ws, 0, on); break;
		case ENC_DQ0: assert(st.b == ws.defer_verbatim); nhw_launch_wave(WV_DQ0, ws, on, (st.a & 1) != 0, (st.a & 2) != 0); break;
		case ENC_L_SYN2:
			if (st.b) {
				const Plane<const uint8_t> meta = ws.plane<const uint8_t>(B_META), len{ meta.p + offsetof(NhwMeta, ll_mem_len), meta.pitch };
				nhw_launch_synthesis(jpeg, proc, n, W, H, st.a, ws.plane<const uint8_t>(B_LLMEM), len, on);
			} else nhw_launch_synthesis(jpeg, proc, n, W, H, st.a, on);
			break;
		case ENC_L4A: nhw_launch_phase(PH_L4A, ws, 0, on); break;
		case ENC_L4B: nhw_launch_phase(PH_L4B, ws, 0, on); break;
		case ENC_L4C: nhw_launch_phase(PH_L4C, ws, 0, on); break;
		case ENC_QUANT: nhw_launch_wave(WV_QUANT, ws, on, false, st.a != 0); break;
		case ENC_L4C2: nhw_launch_phase(PH_L4C2, ws, 0, on); break;
		case ENC_Y31: nhw_launch_phase(PH_L4D, ws, 0, on); break;
		case ENC_PACK_CHROMA: nhw_launch_pack_chroma(ws, on); break;
		case ENC_LLC: nhw_launch_phase(PH_LLC, ws, 0, on); break;
		case ENC_FINAL: nhw_launch_final(ws, (uint8_t *)io.d_out, io.d_sizes, io.d_status, on, st.a != 0); break;
		default: assert(!"a step the executor does not know"); break;
		}
	}
	HIPCHK(hipGetLastError());
	return NHW_OK;
}

/* what the handle and one call put into the planner */
static EncIn plan_input(const nhw_enc *e, int n, int quality, int timed, int what)
{
	EncIn in = {};
	in.q = quality; in.stop = e->stop_after; in.compat = e->ws.compat; in.what = what; in.timed = timed; in.big = n >= 1024; in.front_fallback = e->front_fallback & 1;
	in.low_chroma = e->low_chroma; in.chroma_fork = e->chroma_fork; in.lists_fork = e->lists_fork; in.ll_fork = e->ll_fork; in.quant_join = e->quant_join;
	in.y5_fork = e->y5_fork; in.ll2_once = e->ll2_once; in.quant_marks = e->quant_marks; in.chroma_tail_once = e->chroma_tail_once; in.pack_fork = e->pack_fork;
	in.low_parts = e->low_parts;
	return in;
}

/* the launch sequence for the images of one workspace view on one stream: check, plan, run.  timed, what: EncIn (nhw_enc_plan.h) */
static int run_batch(nhw_enc *e, const NhwWs &ws_in, const void *d_bgr, bool grey, int n, int quality, void *d_out, uint32_t *d_sizes, int32_t *d_status, hipStream_t s,
                     int timed, int what, bool *counts_as_timed = nullptr)
{
	const EncPlan plan = enc_plan(plan_input(e, n, quality, timed, what));
	if (!plan.n) { nhw_enc_err = "no launch plan for this call"; return NHW_E_ARG; }
	NhwWs ws = ws_in;
	assert(ws.n == n && ws.q == quality && ws.dbg == plan.dbg);
	ws.split_chroma = plan.split_chroma; ws.defer_verbatim = plan.defer_verbatim;
	if (counts_as_timed) *counts_as_timed = plan.timed;
	return run_steps(e, ws, plan, EncIo{ d_bgr, d_out, d_sizes, d_status, grey }, s);
}

/* Most kernels of the sequence are bound by latency at the occupancy their LDS footprint allows, not by HBM or the ALUs, so a
 * large batch is cut into sub-batches whose sequences run on streams of their own: kernels of different stages overlap on the
 * CUs.  Images are independent and the workspace is indexed per image, so a sub-batch is just a shifted view of it. */
static int batch_device(nhw_enc *e, const void *d_bgr, bool grey, int n, int quality, void *d_out, uint32_t *d_sizes, int32_t *d_status, void *stream)
{
	if (!e || !d_bgr || !d_out || !d_sizes || !d_status || n < 1 || n > e->max_batch) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (grey && ((uintptr_t)d_bgr & 15)) { nhw_enc_err = "nhw_enc_batch_device_grey: d_grey must be 16-byte aligned"; return NHW_E_ARG; }
	if (!nhw_quality_supported(quality)) { nhw_enc_err = "quality outside 1..23"; return NHW_E_QUALITY; }
	const size_t picture = grey ? (size_t)W * W : (size_t)W * W * 3;  /* the input advances by the picture's own size */
	HIPCHK(hipSetDevice(e->device));
	hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
	const NhwSliceScope slices(e->slice_order);
	NhwWs ws = e->ws;
	ws.n = n; ws.q = quality; ws.dbg = e->stop_after != 0;
	e->timed = false;                                              /* set again only when a whole, un-stopped batch has recorded every event of nhw_timing */
	const int parts = (e->stop_after || n < 512) ? 1 : e->parts;
	if (parts == 1) {
		bool timed = false;
		const int rc = run_batch(e, ws, d_bgr, grey, n, quality, d_out, d_sizes, d_status, s, 1, 3, &timed);
		if (rc == NHW_OK && timed) { e->timed = true; e->timed_parts = 1; e->timed_front_images = n; e->last_n = n; e->last_q = quality; }
		return rc;
	}
	/* the front launch group is the part that is bound by the memory system and the ALUs: it runs once for the whole batch */
	HIPCHK(hipEventRecord(e->ev[EV_START], s));
	{ const int rc = run_batch(e, ws, d_bgr, grey, n, quality, d_out, d_sizes, d_status, s, 0, 1); if (rc != NHW_OK) return rc; }
	HIPCHK(hipEventRecord(e->ev[EV_FRONT], s));
	HIPCHK(hipEventRecord(e->part_ev[PE_FRONT], s));
	e->timed_front_images = n;
	for (int k = 0; k < parts; k++) {
		const int i0 = (int)((long long)n * k / parts), i1 = (int)((long long)n * (k + 1) / parts);
		NhwWs view = ws;
		view.n = i1 - i0;
		for (int b = 0; b < B_COUNT; b++) view.off[b] += (size_t)i0 * ws.stride[b];
		hipStream_t ps_ = e->part_stream[k];                           /* (its plan begins with the wait for PE_FRONT) */
		const int rc = run_batch(e, view, (const uint8_t *)d_bgr + (size_t)i0 * picture, grey, i1 - i0, quality, (uint8_t *)d_out + (size_t)i0 * NHW_OUT_STRIDE,
		                         d_sizes + i0, d_status + i0, ps_, k == 0 ? 2 : 0, 2);
		if (rc != NHW_OK) return rc;
		HIPCHK(hipEventRecord(e->part_ev[k], ps_));
		HIPCHK(hipStreamWaitEvent(s, e->part_ev[k], 0));
	}
	HIPCHK(hipEventRecord(e->ev[EV_END], s));
	e->timed = true; e->timed_parts = parts; e->last_n = n; e->last_q = quality;
	return NHW_OK;
}

extern "C" int nhw_enc_batch_device(nhw_enc *e, const void *d_bgr, int n, int quality, void *d_out, uint32_t *d_sizes,
                                    int32_t *d_status, void *stream)
{
	return batch_device(e, d_bgr, false, n, quality, d_out, d_sizes, d_status, stream);
}

/* the same from grey pictures, 512 x 512 bytes each: file i is the file of picture i with every byte in B, G and R */
extern "C" int nhw_enc_batch_device_grey(nhw_enc *e, const void *d_grey, int n, int quality, void *d_out, uint32_t *d_sizes,
                                         int32_t *d_status, void *stream)
{
	return batch_device(e, d_grey, true, n, quality, d_out, d_sizes, d_status, stream);
}

extern "C" int nhw_enc_last_timing(nhw_enc *e, nhw_timing *t)
{
	if (!e || !t || !e->timed) { nhw_enc_err = "no timed batch"; return NHW_E_ARG; }
	HIPCHK(hipEventSynchronize(e->ev[EV_END]));
	memset(t, 0, sizeof *t);
	HIPCHK(hipEventElapsedTime(&t->total_ms, e->ev[EV_START], e->ev[EV_END]));
	HIPCHK(hipEventElapsedTime(&t->front_ms, e->ev[EV_START], e->ev[EV_FRONT]));   /* several parts: the later stage times are those of the first sub-batch, on its stream */
	HIPCHK(hipEventElapsedTime(&t->luma_ms, e->ev[EV_FRONT], e->ev[EV_LUMA]));
	HIPCHK(hipEventElapsedTime(&t->chroma_ms, e->ev[EV_LUMA], e->ev[EV_CHROMA]));
	HIPCHK(hipEventElapsedTime(&t->entropy_ms, e->ev[EV_CHROMA], e->ev[EV_END]));
	HIPCHK(hipEventElapsedTime(&t->color_dwt_ms, e->ev[EV_START], e->ev[EV_COLOR]));
	HIPCHK(hipEventElapsedTime(&t->prefilter_ms, e->ev[EV_COLOR], e->ev[EV_PREFILTER]));
	t->parts = e->timed_parts; t->front_images = e->timed_front_images;
	return NHW_OK;
}

extern "C" int nhw_synth_batch_device(nhw_enc *e, void *d_bgr, int n, uint32_t seed_base, void *stream)
{
	if (!e || !d_bgr || n < 1) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	HIPCHK(hipSetDevice(e->device));
	nhw_launch_synth((uint8_t *)d_bgr, n, seed_base, stream ? (hipStream_t)stream : e->own_stream);
	HIPCHK(hipGetLastError());
	return NHW_OK;
}

/* ------------------------------------------------------------------------------------------------ stage entry points */
extern "C" int nhw_stage_color(nhw_enc *e, const void *d_bgr, int n, int quality, void *d_y, void *d_u, void *d_v, void *stream)
{
	if (!e || n < 1) return NHW_E_ARG;
	if (quality < 1 || quality > 23) return NHW_E_QUALITY;          /* this stage covers every quality (the whole encoder: 17..23) */
	HIPCHK(hipSetDevice(e->device));
	nhw_launch_color((const uint8_t *)d_bgr, n, quality, Plane<int16_t>{ (int16_t *)d_y, 4 * Q }, Plane<uint8_t>{ (uint8_t *)d_u, Q }, Plane<uint8_t>{ (uint8_t *)d_v, Q }, stream ? (hipStream_t)stream : e->own_stream);
	HIPCHK(hipGetLastError());
	return NHW_OK;
}

/* the luma pre-filter as a stage exists for quality 1..16 only (k_low_prefilter, the kernel the encoder runs); for 17..21 it is a step
 * inside the fused front kernel and has no output of its own: nhw_debug_stop_after + nhw_debug_read see the planes behind it */
extern "C" int nhw_stage_prefilter(nhw_enc *e, void *d_y, int n, int quality, void *stream)
{
	if (!e || !d_y || n < 1 || n > e->max_batch) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (quality < 1 || quality > 16) { nhw_enc_err = "the pre-filter is a stage of its own only for quality 1..16"; return NHW_E_QUALITY; }
	HIPCHK(hipSetDevice(e->device));
	const NhwWs &ws = e->ws;
	hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
	/* in place for the caller: filter into the workspace plane the encoder uses, copy back */
	const Plane<int16_t> filtered = ws.plane<int16_t>(B_KMAP);
	HIPCHK((hipError_t)nhw_launch_low_prefilter(Plane<const int16_t>{ (const int16_t *)d_y, 4 * Q }, filtered, ws.plane<int16_t>(B_PROC), ws.plane<uint8_t>(B_SCAN), ws.plane<uint8_t>(B_KEEP), ws.plane<uint8_t>(B_LOWTAB), quality, n, s, 0, 1 /* in line */, e->low_stream, e->low_ev));
	HIPCHK(hipMemcpy2DAsync(d_y, 8 * Q, filtered.p, filtered.bytes(), 8 * Q, (size_t)n, hipMemcpyDeviceToDevice, s));
	HIPCHK(hipGetLastError());
	return NHW_OK;
}

/* smallest and largest sample of n planes of W x W shorts (the domain check of the size-512 analysis stage) */
__global__ __launch_bounds__(256) void k_plane_range(const int16_t *__restrict__ base, size_t plane_stride, int *__restrict__ mnmx)
{
	const uint4 *p = reinterpret_cast<const uint4 *>(base + (size_t)blockIdx.y * plane_stride);
	int mn = 32767, mx = -32768;
	for (int i = blockIdx.x * 256 + threadIdx.x; i < W * W / 8; i += gridDim.x * 256) {
		const uint4 v = p[i];
		const uint32_t w[4] = { v.x, v.y, v.z, v.w };
		for (int k = 0; k < 4; k++) {
			const int a = (int16_t)(w[k] & 0xFFFF), b = (int16_t)(w[k] >> 16);
			mn = a < mn ? a : mn; mn = b < mn ? b : mn; mx = a > mx ? a : mx; mx = b > mx ? b : mx;
		}
	}
	for (int o = 32; o; o >>= 1) { const int a = __shfl_xor(mn, o), b = __shfl_xor(mx, o); mn = a < mn ? a : mn; mx = b > mx ? b : mx; }
	if ((threadIdx.x & 63) == 0) { atomicMin(&mnmx[0], mn); atomicMax(&mnmx[1], mx); }
}

/* one analysis level with the kernels the encoder runs: size 512 = the band kernel on a luma plane (its LL copy goes to the jpeg plane,
 * the second copy it makes to the workspace's ll1), 256 / 128 = the whole-block kernels.
 * Size 512 has a DOMAIN (include/nhw_hip.h, proof in nhw_front_image.h): the level-1 kernel runs both filter passes in packed 16-bit
 * arithmetic, which equals the reference's `int` accumulators (filters.c:203-287, 346-386) only while the second pass stays inside 16 bits.
 * Planes outside it are refused (NHW_E_ARG) -- never answered with a plane that differs from wavelet_analysis(). */
extern "C" int nhw_stage_analysis(nhw_enc *e, void *d_jpeg, void *d_proc, int n_img, size_t plane_stride, int stride, int size,
                                  int final_level, void *stream)
{
	if (!e || n_img < 1) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	HIPCHK(hipSetDevice(e->device));
	hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
	if (size == 512) {
		if (stride != W || final_level || n_img > e->max_batch) { nhw_enc_err = "size 512: stride 512, not the final level, n <= max_batch"; return NHW_E_ARG; }
		if (((uintptr_t)d_jpeg & 15) || ((uintptr_t)d_proc & 15) || (plane_stride & 7) || plane_stride < (size_t)W * W) {   /* the range check and the kernel read 16 bytes at a time */
			nhw_enc_err = "size 512: planes must be 16-byte aligned and plane_stride (in samples) a multiple of 8, at least 512 x 512"; return NHW_E_ARG;
		}
		const NhwWs &ws = e->ws;
		{                                                          /* the domain check: U = largest sample (or 0), L = -smallest (or 0); 104 U + 40 L and 104 L + 40 U at most NHW_ANA512_BOUND */
			int *d_mm = reinterpret_cast<int *>(ws.plane<uint8_t>(B_ROWSTATE).p), mm[2] = { 32767, -32768 };   /* (the front kernel's row-state bytes: free until it runs) */
			HIPCHK(hipMemcpyAsync(d_mm, mm, sizeof mm, hipMemcpyHostToDevice, s));
			k_plane_range<<<dim3(32, n_img), 256, 0, s>>>((const int16_t *)d_jpeg, plane_stride, d_mm);
			HIPCHK(hipMemcpyAsync(mm, d_mm, sizeof mm, hipMemcpyDeviceToHost, s));
			HIPCHK(hipStreamSynchronize(s));
			const long U = mm[1] > 0 ? mm[1] : 0, L = mm[0] < 0 ? -(long)mm[0] : 0;
			if (104 * U + 40 * L > NHW_ANA512_BOUND || 104 * L + 40 * U > NHW_ANA512_BOUND) {
				nhw_enc_err = "size 512: samples outside the level-1 kernel's 16-bit domain (104 U + 40 L <= 32720, see nhw_hip.h)";
				return NHW_E_ARG;
			}
		}
		/* the level-1 kernel's input is a plane of its own (the caller's jpeg plane receives the LL rows) */
		const Plane<int16_t> in = ws.plane<int16_t>(B_KMAP);
		HIPCHK(hipMemcpy2DAsync(in.p, in.bytes(), d_jpeg, plane_stride * 2, 8 * Q, (size_t)n_img, hipMemcpyDeviceToDevice, s));
		NhwFront f;
		f.q = 20; f.n = n_img; f.y = in; f.st = ws.plane<uint8_t>(B_ROWSTATE);
		f.proc = { (int16_t *)d_proc, plane_stride }; f.jpeg = { (int16_t *)d_jpeg, plane_stride }; f.ll1 = ws.plane<int16_t>(B_LL1); f.switches = 2;
		nhw_launch_front_fused(f, s);
	} else if (size == 256 || size == 128)
		nhw_launch_analysis(NhwAnalysis{ { (int16_t *)d_jpeg, plane_stride }, { (int16_t *)d_proc, plane_stride }, n_img, stride, size, final_level }, s);
	else { nhw_enc_err = "transform size must be 512, 256 or 128"; return NHW_E_ARG; }
	HIPCHK(hipGetLastError());
	return NHW_OK;
}

/* the two chroma level-1 analyses (wavelet_analysis(256, 0, 0) of U and of V, nhw_encoder.c:2265, 2576) exactly as the encoder launches them for quality >= 15:
 * from the 4:2:0 byte planes the front left in the workspace, without the store nothing reads.  A measurement hook: bench.py brackets it with
 * events to add these launches' time to the fused front kernel's (SURVEY 8(d) counts their output among that kernel's bytes). */
extern "C" int nhw_stage_chroma_l1(nhw_enc *e, int n, void *stream)
{
	if (!e || n < 1 || n > e->max_batch) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (!e->timed || n > e->last_n || e->last_q < 15) {             /* the byte planes must be those of a whole batch at a quality that launches this form (q >= 15: the analysis widens the bytes itself) */
		nhw_enc_err = "nhw_stage_chroma_l1: the handle's last batch does not cover the request (needs a completed batch of >= n images at quality >= 15)";
		return NHW_E_ARG;
	}
	HIPCHK(hipSetDevice(e->device));
	const NhwWs &ws = e->ws;
	hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
	HIPCHK(hipStreamWaitEvent(s, e->ev[EV_END], 0));                     /* behind that batch, whatever stream it ran on: its chroma sequence (a stream of the handle) works in the planes written here */
	NhwAnalysis l1 = NhwAnalysis{ ws.plane<int16_t>(B_CJPEG), ws.plane<int16_t>(B_CPROC), n, H, H, 0 }.saving(ws.plane<int16_t>(B_CLL1), H / 2, ANA_SAVE_LL);
	l1.store = ANA_STORE_NO_T_LL_SAVED;
	for (int comp = 0; comp < 2; comp++) { l1.src8 = ws.plane<const uint8_t>(comp ? B_PV : B_PU); nhw_launch_analysis(l1, s); }
	HIPCHK(hipGetLastError());
	return NHW_OK;
}

/* A test hook for the chroma closed loops of component comp, on the handle's first set of chroma planes, for the first n images of its last
 * whole batch at that batch's quality.
 *   form 0: the head exactly as a production batch launches it (pre-filter / level-1 analysis from the 4:2:0 byte plane, then k_chroma_loops).
 *           Behind a whole batch the marks and the quantiser have rewritten cproc, so the planes the fused kernel leaves are read behind this
 *           call.  It relies on the byte planes of that batch still standing (nothing behind the front writes them);
 *   form 1: k_chroma_loops alone, on cll1 and cproc as they stand (a test may have written them: nhw_debug_write);
 *   form 2 .. 8: the first form - 1 of the seven staged kernels alone (analysis from cll1, simulation 1, synthesis, pre-compensation, analysis
 *           + cl2save, simulation 2, synthesis), every plane stored, on the same inputs: 8 is the whole sequence, 4 stops behind the first
 *           synthesis (cproc = the reconstruction the pre-compensation compares with cll1). */
extern "C" int nhw_stage_chroma_loops(nhw_enc *e, int n, int comp, int form, void *stream)
{
	if (!e || n < 1 || n > e->max_batch || comp < 0 || comp > 1 || form < 0 || form > 8) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (!e->timed || n > e->last_n || e->stop_after) {
		nhw_enc_err = "nhw_stage_chroma_loops: needs a completed whole batch of >= n images and no debug stop";
		return NHW_E_ARG;
	}
	HIPCHK(hipSetDevice(e->device));
	NhwWs ws = e->ws;
	ws.n = n; ws.q = e->last_q; ws.dbg = 0; ws.split_chroma = false;
	hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
	HIPCHK(hipStreamWaitEvent(s, e->ev[EV_END], 0));
	const Plane<int16_t> cjpeg = ws.plane<int16_t>(B_CJPEG), cproc = ws.plane<int16_t>(B_CPROC), cll1 = ws.plane<int16_t>(B_CLL1), cl2save = ws.plane<int16_t>(B_CL2SAVE);
	if (form == 0) {
		EncBuilder b;
		enc_chroma_head(b, ws.q, false, comp, ES_MAIN);
		const int rc = run_steps(e, ws, b.p, EncIo{}, s);
		if (rc != NHW_OK) return rc;
	} else if (form == 1)
		nhw_launch_chroma_loops(cproc, cll1, cl2save, ws.plane<const uint8_t>(B_PU), ws.q, comp, ws.compat, n, s);
	else {
		const int k = form - 1;
		const NhwAnalysis l2{ cjpeg, cproc, n, H, H / 2, 1 };
		nhw_launch_analysis(l2.from(cll1, H / 2), s);
		if (k > 1) nhw_launch_phase(PH_C2, ws, comp, s);
		if (k > 2) nhw_launch_synthesis(cjpeg, cproc, n, H, H / 2, 0, s);
		if (k > 3) nhw_launch_phase(PH_C3, ws, comp, s);
		if (k > 4) nhw_launch_analysis(l2.saving(cl2save, H / 2, ANA_SAVE_BLOCK), s);
		if (k > 5) nhw_launch_phase(PH_C4, ws, comp, s);
		if (k > 6) nhw_launch_synthesis(cjpeg, cproc, n, H, H / 2, 0, s);
	}
	HIPCHK(hipGetLastError());
	return NHW_OK;
}

/* A test hook for the chroma tail (marks, LL2 emission, quantiser) of component comp, for the first n images of the handle's last whole batch at
 * that batch's quality, on the planes as they stand (a test writes them: nhw_debug_write): B_CPROC, B_CLL1, B_CL2SAVE -- for V the planes the
 * handle's order uses (B_CPROC_V, B_CLL1_V, B_CL2SAVE_V with the chroma fork, the same three without) -- and the exception list with its
 * length in B_META, to which the emission appends.  U is run before V: V merges the bytes U parked in B_UBYTES.
 *   form 0: the production form (k_chroma_tail): the symbol list in B_CNZQ / cfbase / B_CVALS; the work plane is not written;
 *   form 1: the staged body as a debug stop runs it (k_phase<PH_C5> with ws.dbg): the same list, the dense stream behind the luma part in
 *           B_SCAN as well, and every plane written. */
extern "C" int nhw_stage_chroma_tail(nhw_enc *e, int n, int comp, int form, void *stream)
{
	if (!e || n < 1 || n > e->max_batch || comp < 0 || comp > 1 || form < 0 || form > 1) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (!e->timed || n > e->last_n || e->stop_after) {
		nhw_enc_err = "nhw_stage_chroma_tail: needs a completed whole batch of >= n images and no debug stop";
		return NHW_E_ARG;
	}
	HIPCHK(hipSetDevice(e->device));
	NhwWs ws = e->ws;
	ws.n = n; ws.q = e->last_q; ws.dbg = form == 1; ws.split_chroma = e->chroma_fork;
	hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
	HIPCHK(hipStreamWaitEvent(s, e->ev[EV_END], 0));
	nhw_launch_chroma_tail(ws, comp, form == 0, s);
	HIPCHK(hipGetLastError());
	return NHW_OK;
}

/* A test hook for the luma plane's first closed loop, on B_JPEG, B_PROC, B_LL1 and B_L2SAVE as they stand (a test writes them: nhw_debug_write), for
 * the first n images of the handle's last whole batch at that batch's quality (7 .. 23: below it there is no first closed loop).
 *   form 0: the production kernels from the first level-2 analysis to the second (enc_luma_loop), every plane stored;
 *   form 1: their last part alone, from the synthesis on: k_l2_recon<true> for q > 12, k_l2_recon<false> and the analysis below it, every plane stored;
 *   forms 6, 7: forms 0, 1 as run_batch launches them outside the compatibility mode, without the stores of the level-2 block that nothing in a
 *           batch reads: the first analysis' transposed plane, and for q > 12 the fused kernel's transposed plane and rows 128 .. 255 of
 *           its block of the work plane.  What those cells hold behind these forms is what stood there (form 6: the first simulation's plane in B_JPEG);
 *   form 2: the staged kernels for form 1's part (synthesis, Y8 + Y9, analysis + Y13's copy), every plane stored;
 *   form 3: the staged kernels for form 0's part; form 4: the same, stopped behind the synthesis (proc = the reconstruction before Y8's nudges,
 *           B_LL1 with Y5's tags); form 5: the staged synthesis alone. */
extern "C" int nhw_stage_luma_loop(nhw_enc *e, int n, int form, void *stream)
{
	if (!e || n < 1 || n > e->max_batch || form < 0 || form > 7) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (!e->timed || n > e->last_n || e->stop_after || e->last_q < 7) {
		nhw_enc_err = "nhw_stage_luma_loop: needs a completed whole batch of >= n images at quality >= 7 and no debug stop";
		return NHW_E_ARG;
	}
	HIPCHK(hipSetDevice(e->device));
	NhwWs ws = e->ws;
	ws.n = n; ws.q = e->last_q; ws.dbg = 0;
	hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
	HIPCHK(hipStreamWaitEvent(s, e->ev[EV_END], 0));
	const Plane<int16_t> jpeg = ws.plane<int16_t>(B_JPEG), proc = ws.plane<int16_t>(B_PROC), ll1 = ws.plane<int16_t>(B_LL1), l2save = ws.plane<int16_t>(B_L2SAVE);
	const NhwAnalysis l2{ jpeg, proc, n, W, H, 1 };
	const bool save = ws.q > 12;
	const bool lean = form >= 6;
	if (lean && ws.compat) { nhw_enc_err = "nhw_stage_luma_loop: forms 6 and 7 are not launched in the compatibility mode"; return NHW_E_ARG; }
	if (form == 0 || form == 6) {
		EncBuilder b;
		enc_luma_loop(b, ws.q, false, false, lean);
		const int rc = run_steps(e, ws, b.p, EncIo{}, s);
		if (rc != NHW_OK) return rc;
	} else if (form == 1 || form == 7) {
		nhw_launch_l2_recon(jpeg, proc, ll1, save ? l2save : Plane<int16_t>{}, n, s, lean && save);
		if (!save) nhw_launch_analysis(l2, s);
	} else {
		if (form == 3 || form == 4) {
			nhw_launch_analysis(l2.from(ll1, H), s);
			nhw_launch_phase(PH_L1, ws, 0, s);
			nhw_launch_wave(WV_DQ1, ws, s);
		}
		nhw_launch_synthesis(jpeg, proc, n, W, H, 0, s);
		if (form < 4) {
			nhw_launch_phase(PH_L2, ws, 0, s);
			nhw_launch_analysis(save ? l2.saving(l2save, H, ANA_SAVE_BLOCK) : l2, s);
		}
	}
	HIPCHK(hipGetLastError());
	return NHW_OK;
}

/* A test hook for the LL2 bump walk of the second closed loop, on B_PROC, B_JPEG and B_L2SAVE as they stand (a test writes them), for the first n
 * images of the handle's last whole batch at that batch's quality (13 .. 23), on one stream: the emission (Y14, Y15), the LL coder (Y16) and the
 * second dequantiser simulation.
 *   form 0: the forked order's kernels -- the emission makes the walk and leaves the simulation's LL2 cells, the simulation skips it;
 *   form 1: the in-line order's -- the emission leaves zeros, the simulation makes the walk again;
 *   forms 2, 3: forms 0, 1 with the put-back of verbatim samples left to the level-2 synthesis, which follows (ws.defer_verbatim). */
extern "C" int nhw_stage_ll2_walk(nhw_enc *e, int n, int form, void *stream)
{
	if (!e || n < 1 || n > e->max_batch || form < 0 || form > 3) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (!e->timed || n > e->last_n || e->stop_after || e->last_q < 13) {
		nhw_enc_err = "nhw_stage_ll2_walk: needs a completed whole batch of >= n images at quality >= 13 and no debug stop";
		return NHW_E_ARG;
	}
	HIPCHK(hipSetDevice(e->device));
	NhwWs ws = e->ws;
	ws.n = n; ws.q = e->last_q; ws.dbg = 0; ws.defer_verbatim = form >= 2;
	hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
	HIPCHK(hipStreamWaitEvent(s, e->ev[EV_END], 0));
	const bool one_walk = !(form & 1);
	nhw_launch_wave(WV_EMIT, ws, s, one_walk);
	nhw_launch_phase(PH_L3, ws, 0, s);
	nhw_launch_wave(WV_DQ0, ws, s, one_walk);
	if (ws.defer_verbatim) {
		const Plane<const uint8_t> meta = ws.plane<const uint8_t>(B_META), len{ meta.p + offsetof(NhwMeta, ll_mem_len), meta.pitch };
		nhw_launch_synthesis(ws.plane<int16_t>(B_JPEG), ws.plane<int16_t>(B_PROC), n, W, H, ws.q <= 21, ws.plane<const uint8_t>(B_LLMEM), len, s);
	}
	HIPCHK(hipGetLastError());
	return NHW_OK;
}

/* A test hook for the hand-over of the second dequantiser simulation's marks to the luma quantiser, on B_L2SAVE, B_PROC and the other planes as they
 * stand (a test writes them), for the first n images of the handle's last whole batch at that batch's quality (17 .. 23), on one stream.
 *   form 0: the second simulation with the hand-over (its LL2 walk and the put-back of verbatim samples left out: neither plane the quantiser
 *           reads is written), then the quantiser reading it;
 *   form 1: the quantiser alone, with its own loops 2 and 3.
 * Both leave B_NZQ (with its fbase table) and B_VALS; above quality 21 the quantiser has then coded the work plane in place. */
extern "C" int nhw_stage_quant(nhw_enc *e, int n, int form, void *stream)
{
	if (!e || n < 1 || n > e->max_batch || form < 0 || form > 1) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (!e->timed || n > e->last_n || e->stop_after || e->last_q < 17) {
		nhw_enc_err = "nhw_stage_quant: needs a completed whole batch of >= n images at quality >= 17 and no debug stop";
		return NHW_E_ARG;
	}
	HIPCHK(hipSetDevice(e->device));
	NhwWs ws = e->ws;
	ws.n = n; ws.q = e->last_q; ws.dbg = 0; ws.defer_verbatim = 1;
	hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
	HIPCHK(hipStreamWaitEvent(s, e->ev[EV_END], 0));
	if (form == 0) nhw_launch_wave(WV_DQ0, ws, s, true, true);
	nhw_launch_wave(WV_QUANT, ws, s, false, form == 0);
	HIPCHK(hipGetLastError());
	return NHW_OK;
}

/* A test hook for the luma residual passes Y19 .. Y27, on B_JPEG, B_PROC, B_LL1, B_L2SAVE and B_FIRST as they stand (a test writes them), for the first
 * n images of the handle's last whole batch at that batch's quality, on one stream.
 *   form 0: k_l4a / k_phase<PH_L4A> (Y19 .. Y23), k_phase<PH_L4B> (Y24, Y25; q > 12) and k_phase<PH_L4C> (Y26, Y27) as production launches them:
 *           up to quality 21 Y26 is left out and HL1's first row looks up into l2save;
 *   form 1: the same launches as a debug stop makes them (ws.dbg = 1): Y26 puts the level-2 block back at every quality;
 *   form 2: k_phase<PH_L4B> alone, on the code plane B_LL1 (and B_FIRST) as it stands (q > 12);
 *   form 3: k_phase<PH_L4C> alone, as production launches it. */
extern "C" int nhw_stage_residuals(nhw_enc *e, int n, int form, void *stream)
{
	if (!e || n < 1 || n > e->max_batch || form < 0 || form > 3) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (!e->timed || n > e->last_n || e->stop_after || (form == 2 && e->last_q <= 12)) {
		nhw_enc_err = "nhw_stage_residuals: needs a completed whole batch of >= n images (form 2: at quality >= 13) and no debug stop";
		return NHW_E_ARG;
	}
	HIPCHK(hipSetDevice(e->device));
	NhwWs ws = e->ws;
	ws.n = n; ws.q = e->last_q; ws.dbg = form == 1;
	hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
	HIPCHK(hipStreamWaitEvent(s, e->ev[EV_END], 0));
	if (form < 2) nhw_launch_phase(PH_L4A, ws, 0, s);
	if (form < 3 && ws.q > 12) nhw_launch_phase(PH_L4B, ws, 0, s);
	if (form != 2) nhw_launch_phase(PH_L4C, ws, 0, s);
	HIPCHK(hipGetLastError());
	return NHW_OK;
}

/* A test hook for the stream stage -- the Y31 symbol rewrites and the RLE + VLC packetiser, a pure function of the symbol stream -- for the first n
 * images of the handle's last whole batch at that batch's quality, on the workspace as it stands (a test writes the lists: nhw_debug_write).
 *   form 0: k_y31, k_pack_chroma, k_final: from the lists as the quantisers leave them (B_NZQ with its fbase table, B_VALS; B_CNZQ with cfbase, B_CVALS);
 *   form 1: k_pack_chroma, k_final, on B_NZS / B_VOFF / B_VALS as they stand (and the chroma lists: k_pack_chroma puts them into stream order
 *           itself, in B_CPACK);
 *   form 2: k_y31 alone: B_NZS / B_VOFF / B_VALS behind it are Y31's; nothing is reported.
 * The chroma packetiser runs on the same stream directly in front of k_final, as in every order of run_batch but the forked one.
 * k_final writes the files into the handle's own output arena; what a test compares lies in the workspace behind the call (B_PACKET -- both
 * parts' words, the chroma part's copied behind the luma part's --, B_BOOK1/2, B_SEL1/2, B_META).  status, sizes (may be null): n entries each of the caller's, host memory -- what k_final reports for every image; the call
 * returns when they are there. */
extern "C" int nhw_stage_stream(nhw_enc *e, int n, int form, int32_t *status, uint32_t *sizes, void *stream)
{
	if (!e || (!status && form != 2) || n < 1 || n > e->max_batch || form < 0 || form > 2) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (!e->timed || n > e->last_n || e->stop_after) {
		nhw_enc_err = "nhw_stage_stream: needs a completed whole batch of >= n images and no debug stop";
		return NHW_E_ARG;
	}
	HIPCHK(hipSetDevice(e->device));
	{ const int rc = host_buffers(e, n); if (rc != NHW_OK) return rc; }
	NhwWs ws = e->ws;
	ws.n = n; ws.q = e->last_q; ws.dbg = 0;
	hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
	HIPCHK(hipStreamWaitEvent(s, e->ev[EV_END], 0));
	if (form != 1) nhw_launch_phase(PH_L4D, ws, 0, s);
	if (form == 2) { HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(s)); return NHW_OK; }
	nhw_launch_final(ws, e->d_out, e->d_sizes, e->d_status, s);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(status, e->d_status, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
	if (sizes) HIPCHK(hipMemcpyAsync(sizes, e->d_sizes, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return NHW_OK;
}

extern "C" int nhw_stage_synthesis(nhw_enc *e, void *d_jpeg, void *d_proc, int n_img, size_t plane_stride, int stride, int size, void *stream)
{
	if (!e || n_img < 1) return NHW_E_ARG;
	if (size != 256 && size != 128) { nhw_enc_err = "synthesis: transform size must be 256 or 128 (the encoder has no synthesis of size 512)"; return NHW_E_ARG; }
	HIPCHK(hipSetDevice(e->device));
	nhw_launch_synthesis({ (int16_t *)d_jpeg, plane_stride }, { (int16_t *)d_proc, plane_stride }, n_img, stride, size, 0, stream ? (hipStream_t)stream : e->own_stream);
	HIPCHK(hipGetLastError());
	return NHW_OK;
}

/* ------------------------------------------------------------------------------------------------ debug hooks (tests only) */
extern "C" int nhw_debug_front_fallback(nhw_enc *e, int on) { if (!e) return NHW_E_ARG; e->front_fallback = on; return NHW_OK; }
extern "C" int nhw_debug_stop_after(nhw_enc *e, int stage) { if (!e) return NHW_E_ARG; e->stop_after = stage; return NHW_OK; }
extern "C" int nhw_debug_slice_order(nhw_enc *e, int mode) { if (!e || mode < 0 || mode > 2) return NHW_E_ARG; e->slice_order = mode; return NHW_OK; }
/* developer hook: order-independent 64-bit digest of the first `bytes` bytes of workspace buffer `buf`, one per image, into device memory */
__global__ __launch_bounds__(256) void k_debug_hash(const uint8_t *base, size_t stride, size_t words, unsigned long long *out)
{
	const uint32_t *p = reinterpret_cast<const uint32_t *>(base + (size_t)blockIdx.x * stride);
	unsigned long long h = 0;
	for (size_t i = threadIdx.x; i < words; i += 256) {
		unsigned long long x = ((unsigned long long)p[i] + 0x9E3779B97F4A7C15ull) * (2 * i + 1);
		x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
		h += x;
	}
	if (threadIdx.x == 0) out[blockIdx.x] = 0;
	__syncthreads();
	atomicAdd(&out[blockIdx.x], h);
}
extern "C" int nhw_debug_hash(nhw_enc *e, int buf, size_t bytes, int n, void *d_out, void *stream)
{
	if (!e || buf < 0 || buf >= B_COUNT || n < 1 || n > e->max_batch || bytes > e->ws.stride[buf]) return NHW_E_ARG;
	HIPCHK(hipSetDevice(e->device));
	k_debug_hash<<<n, 256, 0, stream ? (hipStream_t)stream : e->own_stream>>>(e->ws.base + e->ws.off[buf], e->ws.stride[buf], bytes / 4, (unsigned long long *)d_out);
	HIPCHK(hipGetLastError());
	return NHW_OK;
}
extern "C" int nhw_debug_fill(nhw_enc *e, int buf, int byte, size_t bytes, int n)
{
	if (!e || buf < 0 || buf >= B_COUNT || n < 1 || n > e->max_batch || bytes + GUARD > e->ws.stride[buf]) return NHW_E_ARG;
	HIPCHK(hipSetDevice(e->device));
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemset2D(e->ws.base + e->ws.off[buf], e->ws.stride[buf], byte, bytes, (size_t)n));
	HIPCHK(hipDeviceSynchronize());
	return NHW_OK;
}
extern "C" int nhw_debug_write(nhw_enc *e, int buf, int img, const void *src, size_t bytes)
{
	if (!e || !src || buf < 0 || buf >= B_COUNT || img < 0 || img >= e->max_batch || bytes + GUARD > e->ws.stride[buf]) return NHW_E_ARG;
	HIPCHK(hipSetDevice(e->device));
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(e->ws.base + e->ws.off[buf] + (size_t)img * e->ws.stride[buf], src, bytes, hipMemcpyHostToDevice));
	return NHW_OK;
}
extern "C" int nhw_debug_read(nhw_enc *e, int buf, int img, void *dst, size_t bytes)
{
	if (!e || buf < 0 || buf >= B_COUNT || img < 0 || img >= e->max_batch || bytes > e->ws.stride[buf]) return NHW_E_ARG;
	HIPCHK(hipSetDevice(e->device));
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(dst, e->ws.base + e->ws.off[buf] + (size_t)img * e->ws.stride[buf], bytes, hipMemcpyDeviceToHost));
	return NHW_OK;
}
