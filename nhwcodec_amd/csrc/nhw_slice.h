/*
 * nhw_slice.h -- the forced slice order of the tests (nhw_debug_slice_order, nhw_dec_debug_slice_order in include/nhw_hip_debug.h).
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
#ifndef NHW_SLICE_H
#define NHW_SLICE_H

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

#endif
