/*
 * nhw_enc.h -- the encoder handle (struct nhw_enc) and what the encoder's files share: nhw_enc.hip (handle, batch driver, timing, stage
 * entry points, debug hooks), nhw_enc_hostpath.hip (host path, pictures of any size and their searches), nhw_enc_fit.hip (the searches).
 */
#ifndef NHW_ENC_H
#define NHW_ENC_H

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <climits>

#include "nhw_host.h"
#include "nhw_ws.h"

extern thread_local std::string nhw_enc_err;   /* nhw_last_error() */
#define NHW_ERR nhw_enc_err

/* The handle's events by name.  ev[]: the stage marks of nhw_timing, in the order a batch records them up to EV_END; the colour kernel's
 * and the pre-filter's ends lie inside the front group. */
enum { EV_START, EV_FRONT, EV_LUMA, EV_CHROMA, EV_END, EV_COLOR, EV_PREFILTER, EV_COUNT };
/* part_ev[]: the forks and joins of one batch -- the luma plane's exception list is complete (the chroma emission appends to it), the
 * chroma stream is through, the position lists' fork and their end, the front group's end in front of the sub-batches.  With sub-batches
 * (NHW_PARTS > 1) the forks are off and slot k < 4 is sub-batch k's end instead. */
enum { PE_LUMA_LIST, PE_CHROMA, PE_LISTS_FORK, PE_LISTS, PE_FRONT, PE_COUNT };
/* ll_ev[]: the LL2 coder's fork beside the second dequantiser simulation, and its end; Y5's fork onto the same stream beside the first
 * simulation, and its end; the chroma packetiser's fork onto it beside Z1 (NHW_PACK_FORK=2), and its end */
enum { LL_EV_FORK, LL_EV_DONE, LL_EV_Y5_FORK, LL_EV_Y5_DONE, LL_EV_PACK_FORK, LL_EV_PACK_DONE, LL_EV_COUNT };

struct nhw_enc {
	int device, max_batch;
	NhwWs ws;
	hipStream_t own_stream;
	hipStream_t part_stream[4];   /* a large batch runs as up to four sub-batches on streams of their own (see nhw_enc_batch_device) */
	hipEvent_t part_ev[PE_COUNT];
	hipStream_t low_stream[4];    /* quality 1..16: the pre-filter's sub-batches (nhw_launch_low_prefilter) */
	hipEvent_t low_ev[LOW_EV_COUNT];
	int low_parts;                /* how many (NHW_LOW_PARTS; 1 = the whole batch in line) */
	int low_chroma;               /* quality 1..16: where the chroma sequence starts (NHW_LOW_CHROMA: 0 behind the front group, 1 behind the colour kernel, 2 behind the last sub-batch's pass A) */
	hipStream_t ll_stream;        /* the LL2 coder (Y16) beside the second dequantiser simulation; before that, Y5 beside the first */
	hipEvent_t ll_ev[LL_EV_COUNT];
	int ll_fork;
	int quant_join;               /* the side streams join in front of the luma quantiser (q <= 21) */
	int y5_fork;                  /* Y5 on ll_stream beside the first dequantiser simulation (NHW_Y5_FORK=0: in front of it on the luma stream) */
	int ll2_once;                 /* q > 12: the LL2 bump walk in the emission only (NHW_LL2_ONCE=0: again in the second simulation) */
	int chroma_tail_once;         /* the chroma tail as one walk that reads each plane row once and does not write cproc (NHW_CHROMA_TAIL_ONCE=0: the staged body, as the stage checks run it) */
	int quant_marks;              /* q > 16: the second simulation hands its marks to the quantiser, which skips its loops 2 and 3 (NHW_QUANT_MARKS=0: the quantiser runs them itself) */
	int pack_fork;                /* forked order: Z2's chroma part (k_pack_chroma) on ll_stream beside Z1 (2, the default), on the chroma stream behind Z1 (1); NHW_PACK_FORK=0: directly in front of k_final, as in every other order */
	int parts;
	hipEvent_t ev[EV_COUNT];
	bool timed;
	int timed_parts, timed_front_images;
	/* host convenience path */
	uint8_t *d_in, *d_out, *d_compact;
	uint32_t *d_sizes; int32_t *d_status; uint64_t *d_offs;
	int conv_cap;
	uint8_t *d_tensor_bytes;      /* nhw_enc_batch_device_tensor: the converted pictures of a batch, max_batch of them; allocated by the first tensor call */
	int chroma_fork;  /* the chroma sequence on a stream of its own next to the luma tail (NHW_CHROMA_FORK=0 turns it off) */
	int lists_fork;   /* the position lists (Y24/Y25) on a third stream (NHW_LISTS_FORK=0 turns it off: +0.75 ms per q20 batch) */
	int front_fallback; /* debug: every row / segment of the pre-filter carry takes its exact fallback path (tests) */
	int stop_after;   /* debug: leave the batch driver after this many stages (0 = run everything) */
	int slice_order;  /* debug: the forced slice order of the kernels that split a picture (nhw_host.h; 0 = production) */
	int last_n, last_q; /* images and quality of the last whole batch (nhw_stage_chroma_l1 works on what it left in the 4:2:0 planes) */
	/* the quality searches (fit_walk): two sets of buffers for max_batch images, each allocated all or nothing by the first call that
	 * needs it (fit_buffers) and present while its first pointer is */
	struct {                              /* every search */
		uint8_t *in, *out;                /* staging: the gathered open images, the files of their rung */
		uint32_t *sizes, *budget;         /* (the budgets: the host path's upload) */
		int32_t *status, *quality;        /* (the qualities: the host path's) */
		int *idx[2], *count;              /* the open list of this rung and of the next; its length */
		uint8_t *open;                    /* per list entry: still open after this rung */
	} fit;
	struct {                              /* the distortion search only: byte-budget callers never allocate it */
		uint8_t *px;                      /* the rung's decoded pictures */
		uint64_t *doff;                   /* decoder offsets: entry j at j * NHW_OUT_STRIDE (the caller's arena and the staging one alike) */
		uint64_t *sse, *maxsse;           /* per list entry: the SSE of its picture; (the targets: the host path's upload) */
		uint64_t *sse_out;                /* (the achieved SSE: the host path's) */
		int32_t *dstatus;                 /* per list entry: the decoder's status */
	} fit_sse;
	int *h_fit_count;                     /* page-locked: the open count the host waits for between rungs */
	hipEvent_t fit_ev[2];
	nhw_fit_stats fit_stats;
	bool fit_done;
	/* grow-only.  nhw_enc_pictures and the picture searches: the uploaded pictures and their descriptor table; nhw_enc_fit_sse_pictures: a
	 * chunk's decoded tiles; the decoder's offsets (a chunk), the open pictures' SSE, the decoder's status (a chunk);
	 * nhw_enc_pictures_resized: the resized pictures, their descriptor table and the resize's address table */
	GrowBuf pic_px, pic_desc, pfit_px, pfit_aux, pic_resized;
};

inline DevSet host_set(nhw_enc *e, size_t n)   /* input slot, output slot, compacted output, sizes, status, offsets: the host path for n images */
{
	return { dev_buf(e->d_in, n * NHW_IMG_BYTES), dev_buf(e->d_out, n * NHW_OUT_STRIDE), dev_buf(e->d_compact, n * NHW_OUT_STRIDE), dev_buf(e->d_sizes, n),
	         dev_buf(e->d_status, n), dev_buf(e->d_offs, n + 1) };
}
inline DevSet fit_set(nhw_enc *e)
{
	const size_t mb = (size_t)e->max_batch;
	return { dev_buf(e->fit.in, mb * NHW_IMG_BYTES), dev_buf(e->fit.out, mb * NHW_OUT_STRIDE), dev_buf(e->fit.sizes, mb), dev_buf(e->fit.budget, mb),
	         dev_buf(e->fit.status, mb), dev_buf(e->fit.quality, mb), dev_buf(e->fit.idx[0], mb), dev_buf(e->fit.idx[1], mb), dev_buf(e->fit.count, 1),
	         dev_buf(e->fit.open, mb) };
}
inline DevSet fit_sse_set(nhw_enc *e)
{
	const size_t mb = (size_t)e->max_batch;
	return { dev_buf(e->fit_sse.px, mb * NHW_IMG_BYTES), dev_buf(e->fit_sse.doff, mb), dev_buf(e->fit_sse.sse, mb), dev_buf(e->fit_sse.maxsse, mb),
	         dev_buf(e->fit_sse.sse_out, mb), dev_buf(e->fit_sse.dstatus, mb) };
}

/* nhw_enc.hip: buffers of the host path for up to n images; on a failed allocation nothing dangles and the capacity stays what really exists */
int host_buffers(nhw_enc *e, int n);
/* nhw_enc_hostpath.hip */
int host_download(nhw_enc *e, int n, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status);
/* nhw_enc_fit.hip, for the picture searches: a search's ladder and its decoder checked, the decoder's offsets j * NHW_OUT_STRIDE */
int ladder_check(const int *ladder, int ladder_len, bool ascending, int *q, int *len);
int dec_check(const nhw_enc *e, nhw_dec *d, int need, const std::string &who, const char *need_name);
void fit_doff(uint64_t *d_off, int n, hipStream_t s);

#endif
