/*
 * nhw_host.h -- everything of libnhwhip.so's host side that crosses a file, declared once: the launchers of the kernel files, the
 * forced slice order, and the helpers both handles (nhw_enc, nhw_dec) use for errors and device buffers (nhw_host.hip).  Private: the
 * public interface is include/nhw_hip.h.  Every file that defines one of these symbols includes this header, so a signature that
 * drifts does not compile; default arguments live here only.
 */
#ifndef NHW_HOST_H
#define NHW_HOST_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/nhw_hip.h"

struct NhwWs;                               /* nhw_ws.h: the encoder's workspace view */

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
void nhw_launch_color(const uint8_t *bgr, int n, int q, int16_t *y, size_t y_stride, uint8_t *u, uint8_t *v, size_t c_stride, hipStream_t s);
void nhw_launch_analysis(int16_t *jpeg, int16_t *proc, int n, size_t plane_stride, int stride, int size, int final_level, hipStream_t s,
                         int16_t *save = nullptr, size_t save_plane = 0, int save_row = 0, int save_kind = 0, const uint8_t *src8 = nullptr, size_t src8_plane = 0, int drop_t = 0,
                         const int16_t *alt = nullptr, size_t alt_plane = 0, int alt_stride = 0);
void nhw_launch_synthesis(int16_t *jpeg, int16_t *proc, int n, size_t plane_stride, int stride, int size, hipStream_t s, int drop_nat = 0,
                          const uint16_t *verb_list = nullptr, size_t verb_list_stride = 0, const int *verb_len = nullptr, size_t verb_len_stride = 0);
void nhw_launch_synth(uint8_t *bgr, int n, uint32_t seed_base, hipStream_t s);
void nhw_launch_front_fused(const uint8_t *bgr, int q, uint8_t *pu, uint8_t *pv, size_t c_stride, const int16_t *y, size_t y_stride, int with_prefilter,
                            uint8_t *st, size_t s_stride, int16_t *proc, int16_t *jpeg, size_t plane_stride, int16_t *ll1, size_t ll1_stride,
                            int16_t *keep, size_t keep_stride, int n, hipStream_t s, int switches);
void nhw_launch_front_stale(const int16_t *y, size_t y_stride, const uint8_t *st, size_t s_stride, int16_t *stale, size_t stale_stride, int n, hipStream_t s);
int nhw_front_set_attrs(const char **where);   /* nhw_front.hip, nhw_tail.hip: dynamic-LDS opt-ins of the device the handle lives on */
/* nhw_tail.hip */
enum { PH_L1, PH_L2, PH_L3, PH_L4A, PH_C0, PH_C2, PH_C3, PH_C4, PH_C5, PH_FINAL, PH_L4B, PH_L4C, PH_L4D, PH_LLC, PH_L4C2 };
enum { WV_DQ1, WV_DQ0, WV_EMIT, WV_QUANT };
void nhw_launch_phase(int ph, const NhwWs &ws, int comp, uint8_t *out, uint32_t *sizes, int32_t *status, hipStream_t s);
void nhw_launch_wave(int ph, const NhwWs &ws, hipStream_t s);
void nhw_launch_l2_recon(int16_t *jpeg, int16_t *proc, size_t plane_stride, int16_t *ll1, size_t ll1_stride, int n, hipStream_t s, int16_t *l2save = nullptr, size_t save_stride = 0);
void nhw_launch_chroma_loops(int16_t *cproc, size_t plane_stride, int16_t *cll1, size_t ll1_stride, int16_t *cl2save, size_t save_stride,
                             const uint8_t *pu, size_t pu_stride, int q, int comp, int compat, int n, hipStream_t s);   /* both chroma closed loops of one component, from cll1 */
void nhw_launch_copy_block(const int16_t *src, size_t src_plane, int src_row, int16_t *dst, size_t dst_plane, int dst_row, int rows, int cols, int n, hipStream_t s);
int nhw_tail_set_attrs(const char **where);
/* nhw_low.hip: quality 1..16 only.  The pre-filter's sub-batches (parts > 1) record into ev[LOW_EV_COUNT]: */
enum { LOW_EV_START = 0, LOW_EV_COUNT = 13 };                       /* the fork; then a pair of events a sub-batch: */
inline int low_ev_pass_a(int p) { return 1 + p; }                   /* sub-batch p is through its pass A */
inline int low_ev_done(int parts, int p) { return 1 + parts + p; }  /* ... and through the whole pre-filter */
int nhw_launch_low_prefilter(const int16_t *src, size_t src_stride, int16_t *y, size_t y_stride, int16_t *km, size_t km_stride, uint8_t *so, size_t so_stride, uint8_t *chain, size_t chain_stride,
                             uint16_t *tab, size_t tab_stride, int q, int n, hipStream_t s, int force = 0, int parts = 1, hipStream_t *aux = nullptr, hipEvent_t *ev = nullptr);
void nhw_launch_low_prefilter_chroma(const uint8_t *src, size_t src_stride, int16_t *dst, size_t dst_stride, int q, int n, hipStream_t s);
void nhw_launch_low_chroma_thin(int16_t *plane, size_t plane_stride, int n, hipStream_t s);
void nhw_launch_low_ll2(int16_t *proc, size_t plane_stride, int q, int n, hipStream_t s);
void nhw_launch_low_stale(const int16_t *km, size_t km_stride, int16_t *stale, size_t stale_stride, int n, hipStream_t s);
/* nhw_fit.hip, nhw_metric.hip: the quality searches */
void nhw_launch_fit_gather(const uint8_t *d_bgr, const int *idx, int m, uint8_t *staging, hipStream_t s);
void nhw_launch_fit_select(const int *idx, int m, const uint8_t *st_out, const uint32_t *st_sizes, const int32_t *st_status, const void *limit,
                           const int32_t *dec_status, const uint64_t *sse, int quality, int last, uint8_t *out, uint32_t *sizes, int32_t *status,
                           int32_t *qual, uint64_t *sse_out, uint8_t *open, hipStream_t s);
void nhw_launch_fit_compact(const uint8_t *open, const int *idx, int m, int *next, int *count, hipStream_t s);
hipError_t nhw_launch_sse(const uint8_t *a, const uint8_t *b, int n, uint64_t *sse, hipStream_t s);
/* nhw_picture.hip: pictures of any size, the .nhwp container */
hipError_t nhw_launch_tile_pad(const nhw_picture *d_pics, int n_pics, int tile0, int m, uint8_t *d_tiles, hipStream_t s);
hipError_t nhw_launch_untile_crop(const uint8_t *d_tiles, const nhw_picture *d_pics, int n_pics, int tile0, int m, hipStream_t s);
hipError_t nhw_launch_untile_region(const uint8_t *d_tiles, const nhw_region *d_regs, int n_regs, int tile0, int m, hipStream_t s);
hipError_t nhw_launch_sse_crop(const uint8_t *d_tiles, const nhw_picture *d_pics, int n_pics, int tile0, int m, uint64_t *d_sse, hipStream_t s);
size_t nhw_container_head(uint8_t *dst, uint32_t width, uint32_t height, const uint32_t *lens, int t);
int nhw_container_parse(const uint8_t *c, size_t len, uint32_t *width, uint32_t *height, int *tiles, const uint8_t **dir);
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
