/*
 * nhw_host.h -- everything of libnhwhip.so's host side that crosses a file, declared once: the launchers of the kernel files, the
 * forced slice order, and the helpers both handles (nhw_enc, nhw_dec) use for errors and device buffers (nhw_host.hip).  Private: the
 * public interface is include/nhw_hip.h.  Every file that defines one of these symbols includes this header, so a signature that
 * drifts does not compile.  No launcher has a default argument: a call says everything it passes.
 *
 * A per-image buffer crosses this header as a Plane<T>: image i starts at p + i * pitch, the pitch in ELEMENTS OF T.  A plane a kernel
 * addresses in bytes is a Plane<uint8_t>, whatever the kernel's pointer type.  The launcher converts to what its kernel takes (pitch, or
 * bytes()) at the <<< >>> and asserts that planes the kernel takes with one stride have one pitch; an absent optional plane is Plane{}.
 */
#ifndef NHW_HOST_H
#define NHW_HOST_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/nhw_hip.h"
#include "nhw_container.h"                  /* the .nhwp container's parser and writer (nhw_container_parse, nhw_container_head) and the tile geometry: inline, HIP-free */

struct NhwWs;                               /* nhw_ws.h: the encoder's workspace view; ws.plane<T>(B_x) makes the Plane of one of its buffers */

template <class T> struct Plane {
	T *p = nullptr; size_t pitch = 0;
	Plane at(size_t i) const { return { p + i * pitch, pitch }; }   /* the view that starts at image i */
	size_t bytes() const { return pitch * sizeof(T); }
	operator Plane<const T>() const { return { p, pitch }; }
};

/* ------------------------------------------------------------------------------------------------ the forced slice order of the tests
 * (nhw_debug_slice_order, nhw_dec_debug_slice_order in include/nhw_hip_debug.h)
 *
 * Several kernels split one item (a picture, a file) across workgroups: bands, quarters, row bands.  In production the workgroups of
 * one item are dispatched side by side, so a kernel that reads what another workgroup of the same launch writes can be right only by
 * timing.  With a forced order such a kernel runs one slice per launch on its own stream -- every item's slice i, then slice i + 1
 * (mode 1) or slice i - 1 (mode 2) -- and successive launches on a stream do not overlap, so a slice that reads what an earlier (mode 1)
 * or a later (mode 2) slice writes sees the written values and the output changes.
 *
 * A kernel in the mode takes one extra uniform argument: its slice, -1 for production (its block index decodes item and slice as it
 * always has), else the one slice every workgroup of the launch takes (block index -> item).  The mode is per thread: the batch entry
 * points (nhw_enc_batch_device, nhw_dec_batch_device) set it from their handle for the launches they enqueue and clear it behind them.
 */
extern thread_local int nhw_slice_mode;     /* 0: production; 1: ascending slices; 2: descending */

struct NhwSliceScope {                      /* the mode of one handle for the launches of one batch call */
	int saved;
	explicit NhwSliceScope(int mode) : saved(nhw_slice_mode) { nhw_slice_mode = mode; }
	~NhwSliceScope() { nhw_slice_mode = saved; }
};

/* launch(slice) once with slice -1 (production), or once a slice in the mode's order */
template <typename F> inline void nhw_slices(int nslices, F &&launch)
{
	if (nhw_slice_mode == 1) for (int i = 0; i < nslices; i++) launch(i);
	else if (nhw_slice_mode == 2) for (int i = nslices - 1; i >= 0; i--) launch(i);
	else launch(-1);
}

/* ------------------------------------------------------------------------------------------------ launchers */
/* nhw_front.hip */
void nhw_launch_color(const uint8_t *bgr, int n, int q, Plane<int16_t> y, Plane<uint8_t> u, Plane<uint8_t> v, hipStream_t s);
void nhw_launch_color_grey(const uint8_t *grey, int n, int q, Plane<int16_t> y, Plane<uint8_t> u, Plane<uint8_t> v, hipStream_t s);   /* the same from grey bytes, one a pixel */
/* One whole-block analysis level (size 256 or 128) of n images: NhwAnalysis{ jpeg, proc, n, row stride, size, final_level }, the optionals by name.
 * save: a second destination for what the reference copies right behind the transform; src8: the block comes as bytes (a 4:2:0 plane);
 * alt: it is read from another int16 plane.  NO_T: the transposed first-direction plane is not stored; NO_T_LL_SAVED: nor need the LL
 * quadrant reach more than `save` (the byte-plane kernel then leaves it out of the work plane) */
enum NhwAnaSave { ANA_SAVE_NONE, ANA_SAVE_BLOCK /* the coefficient block */, ANA_SAVE_LL /* the LL quadrant in natural orientation */ };
enum NhwAnaStore { ANA_STORE_ALL, ANA_STORE_NO_T, ANA_STORE_NO_T_LL_SAVED };
struct NhwAnalysis {
	Plane<int16_t> jpeg, proc; int n, stride, size, final_level;
	Plane<int16_t> save = {}; int save_row = 0; NhwAnaSave save_kind = ANA_SAVE_NONE; NhwAnaStore store = ANA_STORE_ALL;
	Plane<const uint8_t> src8 = {}; Plane<const int16_t> alt = {}; int alt_stride = 0;
	NhwAnalysis from(Plane<const int16_t> p, int row) const { NhwAnalysis a = *this; a.alt = p; a.alt_stride = row; return a; }
	NhwAnalysis saving(Plane<int16_t> p, int row, NhwAnaSave kind) const { NhwAnalysis a = *this; a.save = p; a.save_row = row; a.save_kind = kind; return a; }
};
void nhw_launch_analysis(const NhwAnalysis &a, hipStream_t s);
/* verb_list, verb_len (size 256): + puts back the samples the LL2 coder sent verbatim -- a list of uint16_t an image and the int that holds its length */
void nhw_launch_synthesis(Plane<int16_t> jpeg, Plane<int16_t> proc, int n, int stride, int size, int drop_nat, Plane<const uint8_t> verb_list, Plane<const uint8_t> verb_len, hipStream_t s);
inline void nhw_launch_synthesis(Plane<int16_t> jpeg, Plane<int16_t> proc, int n, int stride, int size, int drop_nat, hipStream_t s) { nhw_launch_synthesis(jpeg, proc, n, stride, size, drop_nat, {}, {}, s); }
void nhw_launch_synth(uint8_t *bgr, int n, uint32_t seed_base, hipStream_t s);
struct NhwFront {                           /* the front launch group of n images: the forms and the members are described at nhw_launch_front_fused */
	const uint8_t *bgr = nullptr; Plane<uint8_t> pu = {}, pv = {}, st = {}; Plane<const int16_t> y = {};
	Plane<int16_t> proc = {}, jpeg = {}, ll1 = {}, keep = {}; int q = 0, with_prefilter = 0, n = 0, switches = 0;
	bool grey = false;                       /* bgr holds grey pictures, 512 x 512 bytes each */
};
void nhw_launch_front_fused(const NhwFront &f, hipStream_t s);
void nhw_launch_front_stale(Plane<const int16_t> y, Plane<const uint8_t> st, Plane<uint8_t> stale, int n, hipStream_t s);
int nhw_front_set_attrs(const char **where);   /* nhw_front.hip, nhw_tail.hip: dynamic-LDS opt-ins of the device the handle lives on */
/* nhw_tail.hip */
enum { PH_L1, PH_L2, PH_L3, PH_L4A, PH_C0, PH_C2, PH_C3, PH_C4, PH_C5, PH_L4B = 10, PH_L4C, PH_L4D, PH_LLC, PH_L4C2 };   /* the numbers name k_phase's instances in recorded profiles (9 was the final phase: k_final) */
enum { WV_DQ1, WV_DQ0, WV_EMIT, WV_QUANT };
void nhw_launch_phase(int ph, const NhwWs &ws, int comp, hipStream_t s);
void nhw_launch_chroma_tail(const NhwWs &ws, int comp, bool once, hipStream_t s);   /* marks, LL2 emission, chroma quantiser of a component.  once: k_chroma_tail, which reads each row of the work plane once and does not write it (a production batch); else, and always under ws.dbg, the staged body k_phase<PH_C5>, whose planes the stage checks read */
void nhw_launch_pack_chroma(const NhwWs &ws, hipStream_t s);   /* Z2, the chroma part's words and ranked book entries: needs V's quantiser (k_phase<PH_C5>) and nothing of the luma tail */
void nhw_launch_final(const NhwWs &ws, uint8_t *out, uint32_t *sizes, int32_t *status, hipStream_t s, bool chroma_packed = false);   /* Z2 + the container; chroma_packed: nhw_launch_pack_chroma has run on these images (otherwise it is launched here, in front) */
void nhw_launch_wave(int ph, const NhwWs &ws, hipStream_t s, bool one_walk = false /* WV_EMIT and WV_DQ0 of one batch alike, quality > 12, production: the emission leaves the LL2 cells of the second simulation, which skips its walk (wave_emit_ll2) */,
                     bool marks = false /* WV_DQ0 and WV_QUANT of one batch alike, quality > 16, production: the simulation hands the quantiser the level-2 details behind its loops 2 and 3 (wave_dequant_details) */);
void nhw_launch_l2_recon(Plane<int16_t> jpeg, Plane<int16_t> proc, Plane<int16_t> ll1, Plane<int16_t> l2save /* or empty */, int n, hipStream_t s, bool lean = false /* production, with l2save: without the stores nothing reads (k_l2_recon) */);
void nhw_launch_chroma_loops(Plane<int16_t> cproc, Plane<int16_t> cll1, Plane<int16_t> cl2save, Plane<const uint8_t> pu, int q, int comp, int compat, int n, hipStream_t s);   /* both chroma closed loops of one component, from cll1 */
void nhw_launch_copy_block(Plane<const int16_t> src, int src_row, Plane<int16_t> dst, int dst_row, int rows, int cols, int n, hipStream_t s);
int nhw_tail_set_attrs(const char **where);
/* nhw_low.hip: quality 1..16 only.  The pre-filter's sub-batches (parts > 1) record into ev[LOW_EV_COUNT]: */
enum { LOW_EV_START = 0, LOW_EV_COUNT = 13 };                       /* the fork; then a pair of events a sub-batch: */
inline int low_ev_pass_a(int p) { return 1 + p; }                   /* sub-batch p is through its pass A */
inline int low_ev_done(int parts, int p) { return 1 + parts + p; }  /* ... and through the whole pre-filter */
int nhw_launch_low_prefilter(Plane<const int16_t> src, Plane<int16_t> y, Plane<int16_t> km, Plane<uint8_t> so, Plane<uint8_t> chain, Plane<uint8_t> tab,
                             int q, int n, hipStream_t s, int force, int parts, hipStream_t *aux, hipEvent_t *ev);
void nhw_launch_low_prefilter_chroma(Plane<const uint8_t> src, Plane<int16_t> dst, int q, int n, hipStream_t s);
void nhw_launch_low_chroma_thin(Plane<int16_t> plane, int n, hipStream_t s);
void nhw_launch_low_ll2(Plane<int16_t> proc, int q, int n, hipStream_t s);
void nhw_launch_low_stale(Plane<const int16_t> km, Plane<uint8_t> stale, int n, hipStream_t s);
/* nhw_fit.hip, nhw_metric.hip: the quality searches */
void nhw_launch_fit_gather(const uint8_t *d_bgr, const int *idx, int m, uint8_t *staging, hipStream_t s);
void nhw_launch_fit_select(const int *idx, int m, const uint8_t *st_out, const uint32_t *st_sizes, const int32_t *st_status, const void *limit,
                           const int32_t *dec_status, const uint64_t *sse, int quality, int last, uint8_t *out, uint32_t *sizes, int32_t *status,
                           int32_t *qual, uint64_t *sse_out, uint8_t *open, hipStream_t s);
void nhw_launch_fit_compact(const uint8_t *open, const int *idx, int m, int *next, int *count, hipStream_t s);
hipError_t nhw_launch_sse(const uint8_t *a, const uint8_t *b, int n, uint64_t *sse, hipStream_t s);
/* nhw_picture.hip: pictures of any size, the .nhwp container */
hipError_t nhw_launch_tile_pad(const nhw_picture *d_pics, int n_pics, int tile0, int m, uint8_t *d_tiles, hipStream_t s);
hipError_t nhw_launch_tile_pad_grey(const nhw_picture *d_pics, int n_pics, int tile0, int m, uint8_t *d_tiles, hipStream_t s);   /* [H][W] pictures, tiles of 512 x 512 bytes */
hipError_t nhw_launch_untile_crop(const uint8_t *d_tiles, const nhw_picture *d_pics, int n_pics, int tile0, int m, int scale /* 1, 2, 4: tiles of side 512 / scale, the table holds the scaled pictures */, hipStream_t s);
hipError_t nhw_launch_untile_region(const uint8_t *d_tiles, const nhw_region *d_regs, int n_regs, int tile0, int m, hipStream_t s);
hipError_t nhw_launch_untile_window(const uint8_t *d_tiles, const nhw_region *d_regs, int n_regs, const nhw_window_use *d_uses /* the launch's own range of the use table */, int n_uses, int tile0, int m, int scale, hipStream_t s);
hipError_t nhw_launch_untile_window_grey(const uint8_t *d_tiles /* slots of T T bytes: a grey decode's */, const nhw_region *d_regs, int n_regs, const nhw_window_use *d_uses, int n_uses, int tile0, int m, int scale, hipStream_t s);
hipError_t nhw_launch_sse_crop(const uint8_t *d_tiles, const nhw_picture *d_pics, int n_pics, int tile0, int m, uint64_t *d_sse, hipStream_t s);
/* nhw_dec.hip: what a caller needs to know about a decoder handle before it hands it work (the distortion searches) */
void nhw_dec_props(const nhw_dec *d, int *device, int *max_batch, int *stop_after);

/* ------------------------------------------------------------------------------------------------ errors
 * HIPCHK(call): a failed HIP call leaves "file:line call -> reason" in NHW_ERR and returns NHW_E_HIP.  NHW_ERR is the including file's
 * thread-local message: the encoder's files report into nhw_last_error()'s string, the decoder into nhw_dec_last_error()'s. */
int nhw_hip_error(std::string &err, hipError_t e, const char *file, int line, const char *call);
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return nhw_hip_error(NHW_ERR, e_, __FILE__, __LINE__, #x); } while (0)

/* ------------------------------------------------------------------------------------------------ device buffers
 * A handle's lazily allocated sets of device buffers, each a table of (pointer, bytes).  dev_alloc gets all of a set or none of it;
 * dev_free frees a set and nulls its pointers. */
struct DevBuf { void **p; size_t bytes; };
using DevSet = std::vector<DevBuf>;
template <class T> inline DevBuf dev_buf(T *&p, size_t count) { return { (void **)&p, count * sizeof(T) }; }
void dev_free(const DevSet &set);
/* what != nullptr: first refuse (NHW_E_ARG) a set larger than the free HBM, with a message that names it, instead of failing inside hipMalloc */
int dev_alloc(const DevSet &set, const char *what, int images, std::string &err);

/* A grow-only device buffer of a host path.  nhw_grow: it holds at least `bytes` afterwards, its old contents not kept; on a failed
 * allocation p is NULL and cap 0. */
struct GrowBuf {
	void *p; size_t cap;
	template <class T> T *as() const { return (T *)p; }
};
hipError_t nhw_grow(GrowBuf &b, size_t bytes);
void nhw_grow_free(GrowBuf &b);

#endif
