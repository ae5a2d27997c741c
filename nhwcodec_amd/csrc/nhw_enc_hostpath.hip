/*
 * nhw_enc_hostpath.hip -- the encoder's host conveniences: images and pictures of any size come from host memory and the files go back
 * there (nhw_enc_batch, nhw_enc_synth_batch, nhw_enc_pictures, the picture searches of DESIGN.md section 12), and the device entry points
 * of the picture kernels and the SSE.
 */
#include "nhw_enc.h"
#include "nhw_tensor.h"

/* ------------------------------------------------------------------------------------------------ host path */
__global__ void k_offsets(const uint32_t *sizes, uint64_t *offs, int n)
{
	if (blockIdx.x || threadIdx.x) return;
	uint64_t acc = 0;
	for (int i = 0; i < n; i++) { offs[i] = acc; acc += sizes[i]; }
	offs[n] = acc;
}
__global__ __launch_bounds__(256) void k_compact(const uint8_t *out, const uint32_t *sizes, const uint64_t *offs, uint8_t *dst)
{
	const int img = blockIdx.x;
	const uint8_t *s = out + (size_t)img * NHW_OUT_STRIDE;
	uint8_t *d = dst + offs[img];
	for (uint32_t i = threadIdx.x; i < sizes[img]; i += 256) d[i] = s[i];
}

/* Compact the first m output slots of the host path behind what is queued on the handle's stream and bring them to the host: the offsets
 * offs[0 .. m] and the status first; then, the stream waited for, the files back to back to room(bytes) (nullptr: they do not fit). */
template <class Room> static int compact_download(nhw_enc *e, int m, uint64_t *offs, int32_t *status, Room room)
{
	hipStream_t s = e->own_stream;
	k_offsets<<<1, 1, 0, s>>>(e->d_sizes, e->d_offs, m);
	k_compact<<<m, 256, 0, s>>>(e->d_out, e->d_sizes, e->d_offs, e->d_compact);
	HIPCHK(hipMemcpyAsync(offs, e->d_offs, sizeof(uint64_t) * (m + 1), hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(status, e->d_status, sizeof(int32_t) * m, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	uint8_t *dst = room(offs[m]);
	if (!dst && offs[m]) { nhw_enc_err = "output arena too small"; return NHW_E_SPACE; }
	HIPCHK(hipMemcpy(dst, e->d_compact, offs[m], hipMemcpyDeviceToHost));
	return NHW_OK;
}

int host_download(nhw_enc *e, int n, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status)
{
	return compact_download(e, n, out_off, status, [&](uint64_t bytes) { return bytes > arena_cap ? nullptr : out_arena; });
}

/* page-locked host memory: buffers handed to nhw_enc_batch that come from here travel by DMA at PCIe speed while the previous chunk
 * is being encoded (pageable memory is staged by the runtime and moves at about half of that) */
extern "C" void *nhw_host_alloc(size_t bytes) { void *p = nullptr; return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr; }
extern "C" void nhw_host_free(void *p) { if (p) (void)hipHostFree(p); }
extern "C" int nhw_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }

extern "C" int nhw_enc_batch(nhw_enc *e, const uint8_t *bgr, int n, int quality, uint8_t *out_arena, size_t arena_cap,
                             uint64_t *out_off, int32_t *status)
{
	if (!e || !bgr || !out_arena || !out_off || !status || n < 1 || n > e->max_batch) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	HIPCHK(hipSetDevice(e->device));
	{ const int rc = host_buffers(e, n); if (rc) return rc; }
	hipStream_t s = e->own_stream, cs = e->part_stream[3];
	/* chunks of 1024 images: the upload of a chunk (its own stream) overlaps the encode of the one before; every chunk is
	 * encoded in the first workspace slots, one after the other on `s` */
	const int chunk = 1024;
	for (int i0 = 0; i0 < n; i0 += chunk) {
		const int m = n - i0 < chunk ? n - i0 : chunk;
		hipEvent_t up;
		HIPCHK(hipEventCreateWithFlags(&up, hipEventDisableTiming));
		HIPCHK(hipMemcpyAsync(e->d_in + (size_t)i0 * NHW_IMG_BYTES, bgr + (size_t)i0 * NHW_IMG_BYTES, (size_t)m * NHW_IMG_BYTES, hipMemcpyHostToDevice, cs));
		HIPCHK(hipEventRecord(up, cs));
		HIPCHK(hipStreamWaitEvent(s, up, 0));
		HIPCHK(hipEventDestroy(up));
		const int rc = nhw_enc_batch_device(e, e->d_in + (size_t)i0 * NHW_IMG_BYTES, m, quality, e->d_out + (size_t)i0 * NHW_OUT_STRIDE, e->d_sizes + i0, e->d_status + i0, s);
		if (rc) return rc;
	}
	return host_download(e, n, out_arena, arena_cap, out_off, status);
}

/* the same from grey pictures, 262144 bytes each, through the same staging: a picture's slot holds three of them */
extern "C" int nhw_enc_batch_grey(nhw_enc *e, const uint8_t *grey, int n, int quality, uint8_t *out_arena, size_t arena_cap,
                                  uint64_t *out_off, int32_t *status)
{
	if (!e || !grey || !out_arena || !out_off || !status || n < 1 || n > e->max_batch) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (!nhw_quality_supported(quality)) { nhw_enc_err = "quality outside 1..23"; return NHW_E_QUALITY; }
	HIPCHK(hipSetDevice(e->device));
	{ const int rc = host_buffers(e, n); if (rc) return rc; }
	hipStream_t s = e->own_stream;
	HIPCHK(hipMemcpyAsync(e->d_in, grey, (size_t)n * NHW_GREY_BYTES, hipMemcpyHostToDevice, s));
	{ const int rc = nhw_enc_batch_device_grey(e, e->d_in, n, quality, e->d_out, e->d_sizes, e->d_status, s); if (rc) return rc; }
	return host_download(e, n, out_arena, arena_cap, out_off, status);
}

/* SURVEY.md 8(d) synthetic images seed_base .. seed_base+n-1, generated on the device, encoded, and the files brought to the host:
 * `nhw-enc --synthetic` (tools/nhw_enc.c) */
extern "C" int nhw_enc_synth_batch(nhw_enc *e, int n, uint32_t seed_base, int quality, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status)
{
	if (!e || !out_arena || !out_off || !status || n < 1 || n > e->max_batch) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	HIPCHK(hipSetDevice(e->device));
	{ const int rc = host_buffers(e, n); if (rc) return rc; }
	nhw_launch_synth(e->d_in, n, seed_base, e->own_stream);
	HIPCHK(hipGetLastError());
	{ const int rc = nhw_enc_batch_device(e, e->d_in, n, quality, e->d_out, e->d_sizes, e->d_status, e->own_stream); if (rc) return rc; }
	return host_download(e, n, out_arena, arena_cap, out_off, status);
}

/* ------------------------------------------------------------------------------------------------ pictures of any size */
static int picture_args(const void *d_pics, int n_pics, int tile0, int m, const void *d_tiles, const char *who)
{
	if (!d_pics || !d_tiles || n_pics < 1 || m < 1 || tile0 < 0 || m > INT_MAX / 16 || tile0 > INT_MAX - m) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if ((uintptr_t)d_tiles & 15) { nhw_enc_err = std::string(who) + ": d_tiles must be 16-byte aligned"; return NHW_E_ARG; }
	return NHW_OK;
}

extern "C" int nhw_tile_pictures_device(const nhw_picture *d_pics, int n_pics, int tile0, int m, void *d_tiles, void *stream)
{
	if (const int rc = picture_args(d_pics, n_pics, tile0, m, d_tiles, "nhw_tile_pictures_device")) return rc;
	HIPCHK(nhw_launch_tile_pad(d_pics, n_pics, tile0, m, (uint8_t *)d_tiles, (hipStream_t)stream));
	return NHW_OK;
}

extern "C" int nhw_tile_pictures_grey_device(const nhw_picture *d_pics, int n_pics, int tile0, int m, void *d_tiles, void *stream)
{
	if (const int rc = picture_args(d_pics, n_pics, tile0, m, d_tiles, "nhw_tile_pictures_grey_device")) return rc;
	HIPCHK(nhw_launch_tile_pad_grey(d_pics, n_pics, tile0, m, (uint8_t *)d_tiles, (hipStream_t)stream));
	return NHW_OK;
}

extern "C" int nhw_untile_pictures_device(const void *d_tiles, const nhw_picture *d_pics, int n_pics, int tile0, int m, void *stream)
{
	if (const int rc = picture_args(d_pics, n_pics, tile0, m, d_tiles, "nhw_untile_pictures_device")) return rc;
	HIPCHK(nhw_launch_untile_crop((const uint8_t *)d_tiles, d_pics, n_pics, tile0, m, 1, (hipStream_t)stream));
	return NHW_OK;
}

/* the crop of a scaled decode: tiles of side 512 / scale, 3 T T bytes each, into the scaled pictures of the table */
extern "C" int nhw_untile_pictures_scaled_device(const void *d_tiles, const nhw_picture *d_pics, int n_pics, int tile0, int n_tiles, int scale, void *stream)
{
	if (const int rc = picture_args(d_pics, n_pics, tile0, n_tiles, d_tiles, "nhw_untile_pictures_scaled_device")) return rc;
	if (scale != 1 && scale != 2 && scale != 4) { nhw_enc_err = "nhw_untile_pictures_scaled_device: the scale must be 1, 2 or 4"; return NHW_E_ARG; }
	HIPCHK(nhw_launch_untile_crop((const uint8_t *)d_tiles, d_pics, n_pics, tile0, n_tiles, scale, (hipStream_t)stream));
	return NHW_OK;
}

extern "C" int nhw_untile_regions_device(const void *d_tiles, const nhw_region *d_regs, int n_regs, int tile0, int m, void *stream)
{
	if (const int rc = picture_args(d_regs, n_regs, tile0, m, d_tiles, "nhw_untile_regions_device")) return rc;
	HIPCHK(nhw_launch_untile_region((const uint8_t *)d_tiles, d_regs, n_regs, tile0, m, (hipStream_t)stream));
	return NHW_OK;
}

/* the crop of a window call: a table of (window, tile) uses over the decoded tiles of the slots [tile0, tile0 + m); and of
 * a grey window call (section 23): the same table and uses over slots of T T bytes, one byte a pixel */
static int untile_windows(const char *who, decltype(nhw_launch_untile_window) *launch, const void *d_tiles, const nhw_region *d_regs, int n_regs, const nhw_window_use *d_uses,
                          int n_uses, int tile0, int m, int scale, void *stream)
{
	if (const int rc = picture_args(d_regs, n_regs, tile0, m, d_tiles, who)) return rc;
	if (!d_uses || n_uses < 1 || n_uses > INT_MAX / 16) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (scale != 1 && scale != 2 && scale != 4) { nhw_enc_err = std::string(who) + ": the scale must be 1, 2 or 4"; return NHW_E_ARG; }
	HIPCHK(launch((const uint8_t *)d_tiles, d_regs, n_regs, d_uses, n_uses, tile0, m, scale, (hipStream_t)stream));
	return NHW_OK;
}

extern "C" int nhw_untile_windows_device(const void *d_tiles, const nhw_region *d_regs, int n_regs, const nhw_window_use *d_uses, int n_uses,
                                         int tile0, int m, int scale, void *stream)
{
	return untile_windows("nhw_untile_windows_device", nhw_launch_untile_window, d_tiles, d_regs, n_regs, d_uses, n_uses, tile0, m, scale, stream);
}

extern "C" int nhw_untile_windows_grey_device(const void *d_tiles, const nhw_region *d_regs, int n_regs, const nhw_window_use *d_uses, int n_uses,
                                              int tile0, int m, int scale, void *stream)
{
	return untile_windows("nhw_untile_windows_grey_device", nhw_launch_untile_window_grey, d_tiles, d_regs, n_regs, d_uses, n_uses, tile0, m, scale, stream);
}

/* the pictures of a table to tensors of a format, one pointwise pass */
extern "C" int nhw_bytes_to_tensor_device(const nhw_picture *d_pics, int n_pics, const nhw_tensor_format *fmt, const uint64_t *d_out_addr, void *stream)
{
	if (!d_pics || !d_out_addr || n_pics < 1 || n_pics > (1 << 24)) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	NhwTensorArgs a;
	if (const int rc = nhw_tensor_format_check(fmt, &a, nhw_enc_err)) return rc;
	HIPCHK(nhw_launch_bytes_to_tensor(d_pics, n_pics, fmt->dtype, fmt->layout, a, d_out_addr, (hipStream_t)stream));
	return NHW_OK;
}

/* ... and sampled into tensors of one size on the way: the pictures of a table to out_width x out_height tensors, one pass of one kernel -- resampled
 * under a filter (DESIGN.md sections 18 to 20) or along the tilted grids of a device table of warps (section 21), as colour or as grey (section 23),
 * with a colour map (section 24) or a tone table (section 25) an entry.  The ten entries are one body, sample_entry, which fills in the call's
 * record (NhwSampleCall, nhw_tensor.h) and launches it; a row of the table below says what an entry's checks are.  Their order is every entry's:
 * the filter (an entry that takes one), the NULL pointers and n, the sides, the format. */
struct SampleEntry {
	const char *who;             /* the entry as the filter's message and nhw_tensor_out_check's name it */
	bool warp;                   /* d_warps in place of a filter, and never NULL */
	NhwFamily family;
	bool maps, tones;            /* the tables that must not be NULL (a toned entry's d_maps may be) */
	bool by_filter;              /* the sides are refused under the name of the entry that brought the filter in (RESAMPLE alone) */
};
/* nhw_resize_, nhw_area_ and nhw_resample_to_tensor_device are one row.  Only the last can name a filter that does not exist, so the filter's message
 * names it; the sides' message names the entry of the filter: through the newest entry the filters 0 and 1 are the older calls themselves, texts included. */
static const char *const RESAMPLE_BY_FILTER[] = { "nhw_resize_to_tensor_device", "nhw_area_to_tensor_device", "nhw_resample_to_tensor_device" };
static const SampleEntry
	RESAMPLE        = { "nhw_resample_to_tensor_device",        false, NHW_FAMILY_COLOUR,    false, false, true  },
	WARP            = { "nhw_warp_to_tensor_device",            true,  NHW_FAMILY_COLOUR,    false, false, false },
	RESAMPLE_GREY   = { "nhw_resample_grey_to_tensor_device",   false, NHW_FAMILY_GREY,      false, false, false },
	WARP_GREY       = { "nhw_warp_grey_to_tensor_device",       true,  NHW_FAMILY_GREY,      false, false, false },
	RESAMPLE_MAPPED = { "nhw_resample_mapped_to_tensor_device", false, NHW_FAMILY_BY_FORMAT, true,  false, false },
	WARP_MAPPED     = { "nhw_warp_mapped_to_tensor_device",     true,  NHW_FAMILY_BY_FORMAT, true,  false, false },
	RESAMPLE_TONED  = { "nhw_resample_toned_to_tensor_device",  false, NHW_FAMILY_BY_FORMAT, false, true,  false },
	WARP_TONED      = { "nhw_warp_toned_to_tensor_device",      true,  NHW_FAMILY_BY_FORMAT, false, true,  false };

static int sample_entry(const SampleEntry &e, const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, int filter, const nhw_tensor_format *fmt,
                        const nhw_warp *d_warps, const NhwOpsArgs &ops, const uint64_t *d_out_addr, void *stream)
{
	if (!e.warp && (filter < NHW_FILTER_TWO_TAP || filter > NHW_FILTER_CUBIC)) { nhw_enc_err = std::string(e.who) + ": the filter must be NHW_FILTER_TWO_TAP, NHW_FILTER_AREA or NHW_FILTER_CUBIC"; return NHW_E_ARG; }
	if (!d_pics || (e.warp && !d_warps) || (e.maps && !ops.maps) || (e.tones && !ops.tones) || !d_out_addr || n < 1 || n > (1 << 24)) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	NhwSampleCall c = { d_pics, n, {}, nhw_family_grey(e.family, fmt), filter, d_warps, ops, d_out_addr };
	if (const int rc = nhw_tensor_out_check(e.by_filter ? RESAMPLE_BY_FILTER[filter] : e.who, out_width, out_height, fmt, &c.out, nhw_enc_err, c.grey)) return rc;
	HIPCHK(nhw_launch_sample(c, (hipStream_t)stream));
	return NHW_OK;
}

extern "C" int nhw_resize_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                                           const uint8_t *d_flags, const uint64_t *d_out_addr, void *stream)
{ return sample_entry(RESAMPLE, d_pics, n, out_width, out_height, NHW_FILTER_TWO_TAP, fmt, nullptr, { d_flags, nullptr, nullptr }, d_out_addr, stream); }

extern "C" int nhw_area_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                                         const uint8_t *d_flags, const uint64_t *d_out_addr, void *stream)
{ return sample_entry(RESAMPLE, d_pics, n, out_width, out_height, NHW_FILTER_AREA, fmt, nullptr, { d_flags, nullptr, nullptr }, d_out_addr, stream); }

extern "C" int nhw_resample_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, int filter, const nhw_tensor_format *fmt,
                                             const uint8_t *d_flags, const uint64_t *d_out_addr, void *stream)
{ return sample_entry(RESAMPLE, d_pics, n, out_width, out_height, filter, fmt, nullptr, { d_flags, nullptr, nullptr }, d_out_addr, stream); }

extern "C" int nhw_warp_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                                         const nhw_warp *d_warps, const uint64_t *d_out_addr, void *stream)
{ return sample_entry(WARP, d_pics, n, out_width, out_height, 0, fmt, d_warps, {}, d_out_addr, stream); }

extern "C" int nhw_resample_grey_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, int filter, const nhw_tensor_format *fmt,
                                                  const uint8_t *d_flags, const uint64_t *d_out_addr, void *stream)
{ return sample_entry(RESAMPLE_GREY, d_pics, n, out_width, out_height, filter, fmt, nullptr, { d_flags, nullptr, nullptr }, d_out_addr, stream); }

extern "C" int nhw_warp_grey_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                                              const nhw_warp *d_warps, const uint64_t *d_out_addr, void *stream)
{ return sample_entry(WARP_GREY, d_pics, n, out_width, out_height, 0, fmt, d_warps, {}, d_out_addr, stream); }

extern "C" int nhw_resample_mapped_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, int filter, const nhw_tensor_format *fmt,
                                                    const uint8_t *d_flags, const nhw_colour_map *d_maps, const uint64_t *d_out_addr, void *stream)
{ return sample_entry(RESAMPLE_MAPPED, d_pics, n, out_width, out_height, filter, fmt, nullptr, { d_flags, d_maps, nullptr }, d_out_addr, stream); }

extern "C" int nhw_warp_mapped_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                                                const nhw_warp *d_warps, const nhw_colour_map *d_maps, const uint64_t *d_out_addr, void *stream)
{ return sample_entry(WARP_MAPPED, d_pics, n, out_width, out_height, 0, fmt, d_warps, { nullptr, d_maps, nullptr }, d_out_addr, stream); }

extern "C" int nhw_resample_toned_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, int filter, const nhw_tensor_format *fmt,
                                                   const uint8_t *d_flags, const nhw_colour_map *d_maps, const nhw_tone_table *d_tones, const uint64_t *d_out_addr, void *stream)
{ return sample_entry(RESAMPLE_TONED, d_pics, n, out_width, out_height, filter, fmt, nullptr, { d_flags, d_maps, d_tones }, d_out_addr, stream); }

extern "C" int nhw_warp_toned_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                                               const nhw_warp *d_warps, const nhw_colour_map *d_maps, const nhw_tone_table *d_tones, const uint64_t *d_out_addr, void *stream)
{ return sample_entry(WARP_TONED, d_pics, n, out_width, out_height, 0, fmt, d_warps, { nullptr, d_maps, d_tones }, d_out_addr, stream); }

/* the histograms of a table's pictures, and tone tables' rows from histograms (nhw_tone.hip) */
extern "C" int nhw_hist_device(const nhw_picture *d_pics, int n, int channels, uint32_t *d_hist, void *stream)
{
	if (!d_pics || !d_hist || n < 1 || n > (1 << 24)) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (channels != 3 && channels != 1) { nhw_enc_err = "nhw_hist_device: channels must be 3 or 1"; return NHW_E_ARG; }
	HIPCHK(nhw_launch_hist(d_pics, n, channels, d_hist, (hipStream_t)stream));
	return NHW_OK;
}

extern "C" int nhw_tone_from_hist_device(const uint32_t *d_hist, int n, int channels, const uint8_t *d_ops, nhw_tone_table *d_tones, void *stream)
{
	if (!d_hist || !d_ops || !d_tones || n < 1 || n > (1 << 24)) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (channels != 3 && channels != 1) { nhw_enc_err = "nhw_tone_from_hist_device: channels must be 3 or 1"; return NHW_E_ARG; }
	HIPCHK(nhw_launch_tone_from_hist(d_hist, n, channels, d_ops, d_tones, (hipStream_t)stream));
	return NHW_OK;
}

/* ------------------------------------------------------------------------------------------------ encode from tensors */
static int tensor_in_args(const void *d_in, const nhw_tensor_format *fmt, NhwTensorArgs *a, const char *who)
{
	if (const int rc = nhw_tensor_format_check(fmt, a, nhw_enc_err)) return rc;
	if (!d_in || ((uintptr_t)d_in & 15)) { nhw_enc_err = std::string(who) + ": d_in must be a 16-byte aligned device pointer"; return NHW_E_ARG; }
	return NHW_OK;
}

extern "C" int nhw_tensor_to_bytes_device(const void *d_in, int n, const nhw_tensor_format *fmt, void *d_bgr, void *stream)
{
	NhwTensorArgs a;
	if (const int rc = tensor_in_args(d_in, fmt, &a, "nhw_tensor_to_bytes_device")) return rc;
	if (!d_bgr || ((uintptr_t)d_bgr & 15)) { nhw_enc_err = "nhw_tensor_to_bytes_device: d_bgr must be a 16-byte aligned device pointer"; return NHW_E_ARG; }
	if (n < 1 || n > (1 << 22)) { nhw_enc_err = "nhw_tensor_to_bytes_device: n outside 1 .. 2^22"; return NHW_E_ARG; }
	HIPCHK(nhw_launch_tensor_to_bytes(d_in, n, fmt->dtype, fmt->layout, a, (uint8_t *)d_bgr, (hipStream_t)stream));
	return NHW_OK;
}

extern "C" int nhw_enc_batch_device_tensor(nhw_enc *e, const void *d_in, int n, const nhw_tensor_format *fmt, int quality,
                                           void *d_out, int32_t *d_sizes, int32_t *d_status, void *stream)
{
	if (!e || !d_out || !d_sizes || !d_status || n < 1 || n > e->max_batch) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	NhwTensorArgs a;
	if (const int rc = tensor_in_args(d_in, fmt, &a, "nhw_enc_batch_device_tensor")) return rc;
	if (!nhw_quality_supported(quality)) { nhw_enc_err = "quality outside 1..23"; return NHW_E_QUALITY; }
	if (nhw_tensor_format_is_bytes(fmt)) return nhw_enc_batch_device(e, d_in, n, quality, d_out, (uint32_t *)d_sizes, d_status, stream);
	HIPCHK(hipSetDevice(e->device));
	if (!e->d_tensor_bytes) {                                          /* the first tensor call on the handle */
		const int rc = dev_alloc({ dev_buf(e->d_tensor_bytes, (size_t)e->max_batch * NHW_IMG_BYTES) }, "tensor encode scratch", e->max_batch, nhw_enc_err);
		if (rc) return rc;
	}
	hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;      /* as nhw_enc_batch_device reads it: the conversion goes in front of the encode */
	HIPCHK(nhw_launch_tensor_to_bytes(d_in, n, fmt->dtype, fmt->layout, a, e->d_tensor_bytes, s));
	return nhw_enc_batch_device(e, e->d_tensor_bytes, n, quality, d_out, (uint32_t *)d_sizes, d_status, s);
}

/* the one-channel forms of both: a format of NHW_T_GREY, [n][512][512] elements, grey pictures of 512 x 512 bytes */
static int tensor_in_args_grey(const void *d_in, const nhw_tensor_format *fmt, NhwTensorArgs *a, const char *who)
{
	if (fmt && (fmt->channels == NHW_T_BGR || fmt->channels == NHW_T_RGB)) { nhw_enc_err = std::string(who) + ": a grey call takes NHW_T_GREY, not NHW_T_BGR or NHW_T_RGB"; return NHW_E_ARG; }
	if (const int rc = nhw_tensor_format_check(fmt, a, nhw_enc_err, true)) return rc;
	if (!d_in || ((uintptr_t)d_in & 15)) { nhw_enc_err = std::string(who) + ": d_in must be a 16-byte aligned device pointer"; return NHW_E_ARG; }
	return NHW_OK;
}

extern "C" int nhw_tensor_to_bytes_grey_device(const void *d_in, int n, const nhw_tensor_format *fmt, void *d_grey, void *stream)
{
	NhwTensorArgs a;
	if (const int rc = tensor_in_args_grey(d_in, fmt, &a, "nhw_tensor_to_bytes_grey_device")) return rc;
	if (!d_grey || ((uintptr_t)d_grey & 15)) { nhw_enc_err = "nhw_tensor_to_bytes_grey_device: d_grey must be a 16-byte aligned device pointer"; return NHW_E_ARG; }
	if (n < 1 || n > (1 << 22)) { nhw_enc_err = "nhw_tensor_to_bytes_grey_device: n outside 1 .. 2^22"; return NHW_E_ARG; }
	HIPCHK(nhw_launch_tensor_to_bytes_grey(d_in, n, fmt->dtype, a, (uint8_t *)d_grey, (hipStream_t)stream));
	return NHW_OK;
}

extern "C" int nhw_enc_batch_device_grey_tensor(nhw_enc *e, const void *d_in, int n, const nhw_tensor_format *fmt, int quality,
                                                void *d_out, int32_t *d_sizes, int32_t *d_status, void *stream)
{
	if (!e || !d_out || !d_sizes || !d_status || n < 1 || n > e->max_batch) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	NhwTensorArgs a;
	if (const int rc = tensor_in_args_grey(d_in, fmt, &a, "nhw_enc_batch_device_grey_tensor")) return rc;
	if (!nhw_quality_supported(quality)) { nhw_enc_err = "quality outside 1..23"; return NHW_E_QUALITY; }
	if (fmt->dtype == NHW_T_U8 && fmt->rows == NHW_T_ROWS_FILE) return nhw_enc_batch_device_grey(e, d_in, n, quality, d_out, (uint32_t *)d_sizes, d_status, stream);   /* already the grey pictures */
	HIPCHK(hipSetDevice(e->device));
	if (!e->d_tensor_bytes) {                                          /* the first tensor call on the handle: the colour call's scratch, a third of it used here */
		const int rc = dev_alloc({ dev_buf(e->d_tensor_bytes, (size_t)e->max_batch * NHW_IMG_BYTES) }, "tensor encode scratch", e->max_batch, nhw_enc_err);
		if (rc) return rc;
	}
	hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
	HIPCHK(nhw_launch_tensor_to_bytes_grey(d_in, n, fmt->dtype, a, e->d_tensor_bytes, s));
	return nhw_enc_batch_device_grey(e, e->d_tensor_bytes, n, quality, d_out, (uint32_t *)d_sizes, d_status, s);
}

extern "C" int nhw_tile_tensors_device(const nhw_tensor_picture *d_pics, int n_pics, int tile0, int m, const nhw_tensor_format *fmt, void *d_tiles, void *stream)
{
	if (const int rc = picture_args(d_pics, n_pics, tile0, m, d_tiles, "nhw_tile_tensors_device")) return rc;
	NhwTensorArgs a;
	if (const int rc = nhw_tensor_format_check(fmt, &a, nhw_enc_err)) return rc;
	HIPCHK(nhw_launch_tile_pad_tensor(d_pics, n_pics, tile0, m, fmt->dtype, fmt->layout, a, (uint8_t *)d_tiles, (hipStream_t)stream));
	return NHW_OK;
}

extern "C" int nhw_sse_pictures_device(const void *d_tiles, const nhw_picture *d_pics, int n_pics, int tile0, int m, uint64_t *d_sse, void *stream)
{
	if (const int rc = picture_args(d_pics, n_pics, tile0, m, d_tiles, "nhw_sse_pictures_device")) return rc;
	if (!d_sse || ((uintptr_t)d_sse & 7)) { nhw_enc_err = "nhw_sse_pictures_device: d_sse must be 8-byte aligned"; return NHW_E_ARG; }
	HIPCHK(nhw_launch_sse_crop((const uint8_t *)d_tiles, d_pics, n_pics, tile0, m, d_sse, (hipStream_t)stream));
	return NHW_OK;
}

/* The pictures of a host call (nhw_enc_pictures, the picture searches): packed (pitch 3 W; bpp 1, the grey pictures of section 27: W) at bgr + in_off[i].  pictures_check: the sides
 * and the tile count; first[i] = picture i's first tile, first[n] = all tiles; the descriptors numbered so (addr still 0). */
struct PicCall {
	std::vector<nhw_picture> desc;
	std::vector<int> first;
	int tiles = 0;
	uint32_t bpp = 3;            /* bytes a pixel: 3, or 1 (nhw_enc_pictures_grey) */
};

static int pictures_check(const uint32_t *width, const uint32_t *height, int n, const char *who, PicCall &pc)
{
	pc.desc.assign((size_t)n, nhw_picture{});
	pc.first.assign((size_t)n + 1, 0);
	uint64_t tiles = 0;
	for (int i = 0; i < n; i++) {
		const int t = nhw_picture_tiles(width[i], height[i]);
		if (t < 1) { nhw_enc_err = std::string(who) + ": a picture side outside 1..65535"; return NHW_E_ARG; }
		pc.desc[i] = { 0, (uint64_t)pc.bpp * width[i], width[i], height[i], (uint32_t)tiles, 0 };
		pc.first[i] = (int)tiles;
		tiles += (uint64_t)t;
		if (tiles > INT_MAX / 16) { nhw_enc_err = std::string(who) + ": too many tiles in one call"; return NHW_E_ARG; }
	}
	pc.first[n] = (int)tiles;
	pc.tiles = (int)tiles;
	return NHW_OK;
}

/* Upload the pictures into the handle's grow-only buffer (one copy of the span they lie in when they lie close together, as a packed host
 * array does; else one copy each) on the handle's stream and fill in the descriptors' addresses; the table itself is the caller's to upload. */
static int pictures_upload(nhw_enc *e, const uint8_t *bgr, const uint64_t *in_off, PicCall &pc)
{
	const int n = (int)pc.desc.size();
	uint64_t bytes = 0, lo = UINT64_MAX, hi = 0;
	for (int i = 0; i < n; i++) {
		const uint64_t sz = (uint64_t)pc.bpp * pc.desc[i].width * pc.desc[i].height;
		bytes += sz;
		lo = in_off[i] < lo ? in_off[i] : lo;
		hi = in_off[i] + sz > hi ? in_off[i] + sz : hi;
	}
	const bool span = hi - lo <= bytes + bytes / 4 + (1u << 20);
	HIPCHK(nhw_grow(e->pic_px, span ? hi - lo : bytes));
	HIPCHK(nhw_grow(e->pic_desc, (size_t)n * sizeof(nhw_picture)));
	hipStream_t s = e->own_stream;
	uint8_t *px = e->pic_px.as<uint8_t>();
	if (span) HIPCHK(hipMemcpyAsync(px, bgr + lo, hi - lo, hipMemcpyHostToDevice, s));
	for (uint64_t i = 0, at = 0; i < (uint64_t)n; i++) {
		const uint64_t sz = (uint64_t)pc.bpp * pc.desc[i].width * pc.desc[i].height;
		if (span) pc.desc[i].addr = (uint64_t)(uintptr_t)(px + (in_off[i] - lo));
		else {
			HIPCHK(hipMemcpyAsync(px + at, bgr + in_off[i], sz, hipMemcpyHostToDevice, s));
			pc.desc[i].addr = (uint64_t)(uintptr_t)(px + at);
			at += sz;
		}
	}
	return NHW_OK;
}

/* The SSE search's per-chunk step (nhw_enc_fit_sse_pictures): decode the chunk's files from the host path's output slots by `dec` and add
 * their picture-cropped error to `sse` (one entry per picture of the table). */
struct ChunkSse {
	nhw_dec *dec;
	uint8_t *px;             /* the chunk's decoded tiles */
	const uint64_t *doff;    /* decoder offsets: tile j at j * NHW_OUT_STRIDE */
	int32_t *dstatus;        /* the decoder's status, a chunk */
	uint64_t *sse;
	int32_t *h_dstatus;      /* host: the decoder's status, every tile of the call */
};

/* Encode the global tiles [0, tiles) of the table d_desc (np pictures) at `quality` in chunks of at most max_batch into the host path's
 * slots: k_tile_pad straight from the uploaded pictures, the encode, (the SSE step), then the chunk's files compacted and brought back.
 * Tile t's file is files[.. + lens[t]) (back to back in tile order), its status tst[t]. */
static int encode_tiles(nhw_enc *e, const nhw_picture *d_desc, int np, int tiles, int quality, const ChunkSse *cs, std::vector<uint8_t> &files,
                        uint32_t *lens, int32_t *tst, bool grey = false /* pictures and tiles of one byte a pixel (section 27; no SSE step) */)
{
	hipStream_t s = e->own_stream;
	const int chunk = tiles < e->max_batch ? tiles : e->max_batch;
	std::vector<uint64_t> offs((size_t)chunk + 1);
	files.clear();
	for (int t0 = 0; t0 < tiles; t0 += chunk) {
		const int m = tiles - t0 < chunk ? tiles - t0 : chunk;
		HIPCHK((grey ? nhw_launch_tile_pad_grey : nhw_launch_tile_pad)(d_desc, np, t0, m, e->d_in, s));
		{ const int rc = (grey ? nhw_enc_batch_device_grey : nhw_enc_batch_device)(e, e->d_in, m, quality, e->d_out, e->d_sizes, e->d_status, s); if (rc) return rc; }
		if (cs) {
			const int rc = nhw_dec_batch_device(cs->dec, e->d_out, cs->doff, e->d_sizes, m, cs->px, cs->dstatus, nullptr, s);
			if (rc) { nhw_enc_err = std::string("decode of a rung: ") + nhw_dec_last_error(); return rc; }
			HIPCHK(nhw_launch_sse_crop(cs->px, d_desc, np, t0, m, cs->sse, s));
			HIPCHK(hipMemcpyAsync(cs->h_dstatus + t0, cs->dstatus, sizeof(int32_t) * m, hipMemcpyDeviceToHost, s));
		}
		const int rc = compact_download(e, m, offs.data(), tst + t0, [&](uint64_t bytes) { const size_t used = files.size(); files.resize(used + bytes); return files.data() + used; });
		if (rc) return rc;
		for (int k = 0; k < m; k++) lens[(size_t)t0 + k] = (uint32_t)(offs[k + 1] - offs[k]);
	}
	return NHW_OK;
}

/* picture i's container (t tiles of lengths lens[], files back to back) at out_arena + *at, which it advances; NHW_E_SPACE if it does not fit */
static int put_container(uint8_t *out_arena, size_t arena_cap, uint64_t *at, uint32_t width, uint32_t height, const uint32_t *lens, int t,
                         const uint8_t *files)
{
	uint64_t sum = 0;
	for (int k = 0; k < t; k++) sum += lens[k];
	const uint64_t size = 16 + 4 * (uint64_t)t + sum;
	if (*at + size > arena_cap) { nhw_enc_err = "output arena too small"; return NHW_E_SPACE; }
	const size_t head = nhw_container_head(out_arena + *at, width, height, lens, t);
	memcpy(out_arena + *at + head, files, sum);
	*at += size;
	return NHW_OK;
}

/* The tiles of a table encoded (encode_tiles), then one container per picture: picture i's status is its first tile's that is not NHW_OK, and
 * only a picture whose tiles all encoded gets a container. */
static int encode_containers(nhw_enc *e, const nhw_picture *d_desc, const PicCall &pc, int quality, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status)
{
	const int n = (int)pc.desc.size(), tiles = pc.tiles;
	std::vector<uint8_t> files;
	std::vector<uint32_t> lens((size_t)tiles);
	std::vector<int32_t> tst((size_t)tiles);
	{ const int rc = encode_tiles(e, d_desc, n, tiles, quality, nullptr, files, lens.data(), tst.data(), pc.bpp == 1); if (rc) return rc; }
	const int *first = pc.first.data();
	uint64_t at = 0, fpos = 0;
	for (int i = 0; i < n; i++) {
		uint64_t sum = 0;
		int32_t st = NHW_OK;
		for (int k = first[i]; k < first[i + 1]; k++) { sum += lens[k]; if (st == NHW_OK) st = tst[k]; }
		out_off[i] = at;
		status[i] = st;
		if (st == NHW_OK) {
			const int rc = put_container(out_arena, arena_cap, &at, pc.desc[i].width, pc.desc[i].height, lens.data() + first[i], first[i + 1] - first[i], files.data() + fpos);
			if (rc) return rc;
		}
		fpos += sum;
	}
	out_off[n] = at;
	return NHW_OK;
}

/* Upload the pictures, pad and tile them in chunks of max_batch tiles into the host path's input slot, encode each chunk, compact and fetch
 * its files; then one container per picture. */
static int enc_pictures(nhw_enc *e, const char *who, uint32_t bpp, const uint8_t *bgr, const uint64_t *in_off, const uint32_t *width, const uint32_t *height, int n,
                        int quality, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status)
{
	if (!e || !bgr || !in_off || !width || !height || !out_arena || !out_off || !status || n < 1) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (!nhw_quality_supported(quality)) { nhw_enc_err = "quality outside 1..23"; return NHW_E_QUALITY; }
	PicCall pc;
	pc.bpp = bpp;
	{ const int rc = pictures_check(width, height, n, who, pc); if (rc) return rc; }
	HIPCHK(hipSetDevice(e->device));
	{ const int rc = host_buffers(e, pc.tiles < e->max_batch ? pc.tiles : e->max_batch); if (rc) return rc; }
	{ const int rc = pictures_upload(e, bgr, in_off, pc); if (rc) return rc; }
	HIPCHK(hipMemcpyAsync(e->pic_desc.p, pc.desc.data(), (size_t)n * sizeof(nhw_picture), hipMemcpyHostToDevice, e->own_stream));
	return encode_containers(e, e->pic_desc.as<nhw_picture>(), pc, quality, out_arena, arena_cap, out_off, status);
}

extern "C" int nhw_enc_pictures(nhw_enc *e, const uint8_t *bgr, const uint64_t *in_off, const uint32_t *width, const uint32_t *height, int n,
                                int quality, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status)
{
	return enc_pictures(e, "nhw_enc_pictures", 3, bgr, in_off, width, height, n, quality, out_arena, arena_cap, out_off, status);
}

/* the same from grey pictures, [H][W] bytes packed at grey + in_off[i]: the container and its tile files are ordinary ones */
extern "C" int nhw_enc_pictures_grey(nhw_enc *e, const uint8_t *grey, const uint64_t *in_off, const uint32_t *width, const uint32_t *height, int n,
                                     int quality, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status)
{
	return enc_pictures(e, "nhw_enc_pictures_grey", 1, grey, in_off, width, height, n, quality, out_arena, arena_cap, out_off, status);
}

/* nhw_enc_pictures with the area filter in front: the pictures go up as there; one k_area_to_tensor (uint8, HWC, BGR, file
 * rows, no flags) resizes them into the handle's second picture buffer, packed out_width x out_height pictures one behind the other with their
 * descriptor table and the launch's address table behind them; the tiles are padded and encoded from that table. */
extern "C" int nhw_enc_pictures_resized(nhw_enc *e, const uint8_t *bgr, const uint64_t *in_off, const uint32_t *width, const uint32_t *height, int n,
                                        uint32_t out_width, uint32_t out_height, int quality, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status)
{
	if (!e || !bgr || !in_off || !width || !height || !out_arena || !out_off || !status || n < 1) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (!nhw_quality_supported(quality)) { nhw_enc_err = "quality outside 1..23"; return NHW_E_QUALITY; }
	if (out_width < 1 || out_height < 1 || out_width > 4096u || out_height > 4096u) { nhw_enc_err = "nhw_enc_pictures_resized: an output side outside 1 .. 4096"; return NHW_E_ARG; }
	PicCall src, pc;
	{ const int rc = pictures_check(width, height, n, "nhw_enc_pictures_resized", src); if (rc) return rc; }
	const uint32_t limit = nhw_filter_limit(NHW_FILTER_AREA);
	for (int i = 0; i < n; i++)
		if (width[i] > limit * out_width || height[i] > limit * out_height) {
			nhw_enc_err = "nhw_enc_pictures_resized: a picture more than " + std::to_string(limit) + " times the output size along a side";
			return NHW_E_ARG;
		}
	{
		const std::vector<uint32_t> ow((size_t)n, out_width), oh((size_t)n, out_height);
		const int rc = pictures_check(ow.data(), oh.data(), n, "nhw_enc_pictures_resized", pc);
		if (rc) return rc;
	}
	HIPCHK(hipSetDevice(e->device));
	{ const int rc = host_buffers(e, pc.tiles < e->max_batch ? pc.tiles : e->max_batch); if (rc) return rc; }
	{ const int rc = pictures_upload(e, bgr, in_off, src); if (rc) return rc; }
	const size_t per = 3 * (size_t)out_width * out_height, px_bytes = ((size_t)n * per + 15) & ~(size_t)15, desc_bytes = (size_t)n * sizeof(nhw_picture);
	HIPCHK(nhw_grow(e->pic_resized, px_bytes + desc_bytes + (size_t)n * 8));
	uint8_t *px = e->pic_resized.as<uint8_t>();
	std::vector<uint64_t> addr((size_t)n);
	for (int i = 0; i < n; i++) pc.desc[i].addr = addr[i] = (uint64_t)(uintptr_t)(px + (size_t)i * per);
	const nhw_picture *d_desc = (const nhw_picture *)(px + px_bytes);
	const uint64_t *d_addr = (const uint64_t *)(px + px_bytes + desc_bytes);
	hipStream_t s = e->own_stream;
	HIPCHK(hipMemcpyAsync(e->pic_desc.p, src.desc.data(), desc_bytes, hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync((void *)d_desc, pc.desc.data(), desc_bytes, hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync((void *)d_addr, addr.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
	const NhwTensorArgs bytes = { { 1.0f, 1.0f, 1.0f }, { 0.0f, 0.0f, 0.0f }, 0, 0 };
	HIPCHK(nhw_launch_sample({ e->pic_desc.as<nhw_picture>(), n, { out_width, out_height, NHW_T_U8, NHW_T_HWC, bytes }, false, NHW_FILTER_AREA, nullptr, {}, d_addr }, s));
	return encode_containers(e, d_desc, pc, quality, out_arena, arena_cap, out_off, status);
}

/* ------------------------------------------------------------------------------------------------ distortion */
extern "C" int nhw_sse_batch_device(const void *d_a, const void *d_b, int n, uint64_t *d_sse, void *stream)
{
	if (!d_a || !d_b || !d_sse || n < 1 || n > 65535) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	if (((uintptr_t)d_a | (uintptr_t)d_b) & 15) { nhw_enc_err = "nhw_sse_batch_device: the pictures must be 16-byte aligned"; return NHW_E_ARG; }
	if ((uintptr_t)d_sse & 7) { nhw_enc_err = "nhw_sse_batch_device: d_sse must be 8-byte aligned"; return NHW_E_ARG; }
	HIPCHK(nhw_launch_sse((const uint8_t *)d_a, (const uint8_t *)d_b, n, d_sse, (hipStream_t)stream));
	return NHW_OK;
}

/* ------------------------------------------------------------------------------------------------ pictures to a byte or distortion budget */
/* One picture search: the byte test (limit = max_bytes) or, with a decoder, the SSE test (limit = max_sse). */
struct PicFit {
	const char *who;
	nhw_dec *dec;                        /* NULL: the byte search */
	const uint64_t *limit;
	int q[23] = {}, len = 0;
};

/* The walk over pictures.  Every picture is open at the first rung.  A rung uploads the table of the open pictures only, first_tile
 * renumbered, and encodes their tiles (encode_tiles: k_tile_pad re-tiles them straight from the uploaded picture bytes); the SSE search
 * decodes each chunk and adds the picture-cropped error into one entry per open picture, zeroed once a rung.  After the rung the host
 * closes every open picture that passes (all tiles NHW_OK; the container size, or the SSE, within its limit; the SSE search: every tile
 * decoded NHW_OK) and keeps its files; at the last rung every picture still open keeps that rung's. */
static int fit_pictures(nhw_enc *e, const PicFit &f, const uint8_t *bgr, const uint64_t *in_off, const uint32_t *width, const uint32_t *height,
                        int n, PicCall &pc, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status, int32_t *quality, uint64_t *sse)
{
	hipStream_t s = e->own_stream;
	const int chunk = pc.tiles < e->max_batch ? pc.tiles : e->max_batch;
	e->fit_done = false;
	nhw_fit_stats st;
	memset(&st, 0, sizeof st);
	HIPCHK(hipEventRecord(e->fit_ev[0], s));
	{ const int rc = host_buffers(e, chunk); if (rc) return rc; }
	{ const int rc = pictures_upload(e, bgr, in_off, pc); if (rc) return rc; }
	ChunkSse cs = {};
	std::vector<int32_t> tdst;
	if (f.dec) {
		HIPCHK(nhw_grow(e->pfit_px, (size_t)chunk * NHW_IMG_BYTES));
		HIPCHK(nhw_grow(e->pfit_aux, (size_t)(chunk + n) * 8 + (size_t)chunk * 4));
		uint64_t *aux = e->pfit_aux.as<uint64_t>();
		fit_doff(aux, chunk, s);
		HIPCHK(hipGetLastError());
		tdst.resize((size_t)pc.tiles);
		cs = { f.dec, e->pfit_px.as<uint8_t>(), aux, (int32_t *)(aux + chunk + n), aux + chunk, tdst.data() };
	}
	std::vector<std::vector<uint8_t>> kept((size_t)n);    /* a closed picture's tile files, back to back */
	std::vector<std::vector<uint32_t>> kept_len((size_t)n);
	std::vector<uint64_t> psse((size_t)n);
	std::vector<int> open((size_t)n);                      /* the open pictures, ascending */
	for (int i = 0; i < n; i++) open[i] = i;
	std::vector<nhw_picture> desc;
	std::vector<uint8_t> files;
	std::vector<uint32_t> lens((size_t)pc.tiles);
	std::vector<int32_t> tst((size_t)pc.tiles);
	for (int r = 0; r < f.len && !open.empty(); r++) {
		const bool last = r == f.len - 1;
		const int no = (int)open.size();
		desc.resize((size_t)no);
		int tiles = 0;
		for (int j = 0; j < no; j++) {
			const int i = open[j];
			desc[j] = pc.desc[i];
			desc[j].first_tile = (uint32_t)tiles;
			tiles += pc.first[i + 1] - pc.first[i];
		}
		st.quality[r] = f.q[r]; st.images[r] = tiles; st.rungs = r + 1;
		HIPCHK(hipMemcpyAsync(e->pic_desc.p, desc.data(), (size_t)no * sizeof(nhw_picture), hipMemcpyHostToDevice, s));
		if (f.dec) HIPCHK(hipMemsetAsync(cs.sse, 0, (size_t)no * 8, s));
		{ const int rc = encode_tiles(e, e->pic_desc.as<nhw_picture>(), no, tiles, f.q[r], f.dec ? &cs : nullptr, files, lens.data(), tst.data()); if (rc) return rc; }
		if (f.dec) HIPCHK(hipMemcpy(psse.data(), cs.sse, (size_t)no * 8, hipMemcpyDeviceToHost));
		std::vector<int> still;
		uint64_t fpos = 0;
		for (int j = 0; j < no; j++) {
			const int i = open[j], t0 = (int)desc[j].first_tile, t = pc.first[i + 1] - pc.first[i];
			uint64_t sum = 0;
			int32_t enc_st = NHW_OK, dec_st = NHW_OK;
			for (int k = t0; k < t0 + t; k++) {
				sum += lens[k];
				if (enc_st == NHW_OK) enc_st = tst[k];
				if (f.dec && dec_st == NHW_OK) dec_st = tdst[k];
			}
			const bool pass = enc_st == NHW_OK && (f.dec ? dec_st == NHW_OK && psse[j] <= f.limit[i] : 16 + 4 * (uint64_t)t + sum <= f.limit[i]);
			if (pass || last) {
				quality[i] = f.q[r];
				status[i] = pass ? NHW_OK : enc_st != NHW_OK ? enc_st : dec_st != NHW_OK ? NHW_E_FORMAT : NHW_E_BUDGET;
				if (sse) sse[i] = enc_st != NHW_OK || dec_st != NHW_OK ? UINT64_MAX : psse[j];
				if (enc_st == NHW_OK) {
					kept[i].assign(files.begin() + fpos, files.begin() + fpos + sum);
					kept_len[i].assign(lens.begin() + t0, lens.begin() + t0 + t);
				}
			} else still.push_back(i);
			fpos += sum;
		}
		open.swap(still);
	}
	HIPCHK(hipEventRecord(e->fit_ev[1], s));
	e->fit_stats = st;
	e->fit_done = true;
	uint64_t at = 0;
	for (int i = 0; i < n; i++) {
		out_off[i] = at;
		if (status[i] == NHW_E_CODEBOOK) continue;                 /* an empty container, as nhw_enc_pictures gives */
		const int rc = put_container(out_arena, arena_cap, &at, width[i], height[i], kept_len[i].data(), (int)kept_len[i].size(), kept[i].data());
		if (rc) return rc;
	}
	out_off[n] = at;
	return NHW_OK;
}

/* the picture searches' checks, in this order: NULL pointers, n, the sides (and the tile count), a debug stop, the ladder, the decoder;
 * nothing is launched before all of them pass */
static int fit_pictures_host(nhw_enc *e, PicFit &f, bool ptrs, const int *ladder, int ladder_len, const uint8_t *bgr, const uint64_t *in_off,
                             const uint32_t *width, const uint32_t *height, int n, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off,
                             int32_t *status, int32_t *quality, uint64_t *sse)
{
	if (!e || !ptrs || !bgr || !in_off || !width || !height || !out_arena || !out_off || !status || !quality || n < 1) { nhw_enc_err = "bad argument"; return NHW_E_ARG; }
	const std::string who = f.who;
	PicCall pc;
	{ const int rc = pictures_check(width, height, n, f.who, pc); if (rc) return rc; }
	if (e->stop_after) { nhw_enc_err = who + ": not with nhw_debug_stop_after set (every rung must be a whole encode)"; return NHW_E_ARG; }
	{ const int rc = ladder_check(ladder, ladder_len, f.dec != nullptr, f.q, &f.len); if (rc) return rc; }
	if (f.dec) { const int rc = dec_check(e, f.dec, pc.tiles < e->max_batch ? pc.tiles : e->max_batch, who, "min(encoder max_batch, tiles)"); if (rc) return rc; }
	HIPCHK(hipSetDevice(e->device));
	return fit_pictures(e, f, bgr, in_off, width, height, n, pc, out_arena, arena_cap, out_off, status, quality, sse);
}

extern "C" int nhw_enc_fit_pictures(nhw_enc *e, const uint8_t *bgr, const uint64_t *in_off, const uint32_t *width, const uint32_t *height, int n,
                                    const uint64_t *max_bytes, const int *ladder, int ladder_len,
                                    uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status, int32_t *quality)
{
	PicFit f;
	f.who = "nhw_enc_fit_pictures"; f.dec = nullptr; f.limit = max_bytes;
	return fit_pictures_host(e, f, max_bytes != nullptr, ladder, ladder_len, bgr, in_off, width, height, n, out_arena, arena_cap, out_off, status, quality, nullptr);
}

extern "C" int nhw_enc_fit_sse_pictures(nhw_enc *e, nhw_dec *d, const uint8_t *bgr, const uint64_t *in_off, const uint32_t *width, const uint32_t *height,
                                        int n, const uint64_t *max_sse, const int *ladder, int ladder_len,
                                        uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status, int32_t *quality, uint64_t *sse)
{
	PicFit f;
	f.who = "nhw_enc_fit_sse_pictures"; f.dec = d; f.limit = max_sse;
	if (!d) { nhw_enc_err = "bad argument: no decoder handle"; return NHW_E_ARG; }
	return fit_pictures_host(e, f, max_sse != nullptr && sse != nullptr, ladder, ladder_len, bgr, in_off, width, height, n, out_arena, arena_cap, out_off, status, quality, sse);
}
