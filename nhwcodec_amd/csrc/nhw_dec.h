/* nhw_dec.h -- the decoder handle (struct nhw_dec) and what the decoder's files share: nhw_dec.hip (kernels, workspace, handle, batch driver, debug hooks),
 * nhw_dec_hostpath.hip (host path, pictures of any size, regions). */
#ifndef NHW_DEC_H
#define NHW_DEC_H

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <climits>

#include "nhw_host.h"

extern thread_local std::string nhw_dec_err;   /* nhw_dec_last_error() */
#define NHW_ERR nhw_dec_err

struct nhw_dec {
	int device, max_batch;
	uint8_t *ws_base;            /* the workspace of max_batch files (laid out by dec_ws, nhw_dec.hip) */
	hipStream_t own_stream;
	hipStream_t chroma_stream;   /* the chroma sequence runs here, next to the luma one (NHW_CHROMA_FORK=0: behind it, on the caller's stream) */
	hipEvent_t fork_ev, join_ev;
	uint16_t *vlc_table;         /* the prefix code's two-level lookup table (k_dec_vlc_table), 2.5 KB */
	int chroma_fork;
	int stop_after;
	bool l1_moved;               /* the last batch ran k_dec_luma_l2q (any stage of it): what it made of plane A's block is in plane_l1 (D_B) (nhw_dec_debug_read) */
	int slice_order;             /* debug: the forced slice order of the kernels that split a file (nhw_host.h; 0 = production) */
	hipEvent_t ev[4];         /* start, after the entropy stages, around the final reconstruction kernel (= end) */
	bool timed;
	/* host convenience path: the files (grow-only) and, for max_batch files, their offsets and lengths, the pictures, status and quality */
	GrowBuf blob;
	uint64_t *d_off; uint32_t *d_len; uint8_t *d_out; int32_t *d_status; int32_t *d_quality;
	/* nhw_dec_pictures, nhw_dec_regions*: the cropped pictures or regions, their descriptor table and the per-tile offsets, lengths and status, grow-only */
	GrowBuf pic_px, pic_desc, pic_tiles;
	GrowBuf crop_tab;            /* nhw_dec_crops_to_device: the staged windows as pictures, the tensors' addresses and the flags, grow-only */
	uint64_t reg_tiles, reg_bytes;   /* the last region call: tiles handed to the decoder, tile-file bytes uploaded (nhw_dec_last_region_stats) */
};

inline DevSet host_set(nhw_dec *d)   /* offsets, lengths, pictures, status, quality: the host path for max_batch files */
{
	const size_t mb = (size_t)d->max_batch;
	return { dev_buf(d->d_off, mb + 1), dev_buf(d->d_len, mb + 1), dev_buf(d->d_out, mb * NHW_IMG_BYTES), dev_buf(d->d_status, mb), dev_buf(d->d_quality, mb) };
}

#endif
