/* nhw_dec_hostpath.hip -- the decoder's host conveniences: files in host memory in, pictures out (nhw_dec_batch), pictures of any size and regions of them out of
 * .nhwp containers (nhw_dec_pictures, nhw_dec_regions*, nhw_dec_windows*, nhw_dec_crops_to_device*, and the window, crop and warp calls as grey, nhw_dec_*_grey*), the BMP header.  They reach the kernels only through nhw_dec_batch_device (nhw_dec.hip), nhw_picture.hip and nhw_resample.hip. */
#include "nhw_dec.h"
#include "nhw_tensor.h"
#include "nhw_colour.h"
#include "nhw_tile_plan.h"

/* the host paths' buffers: the blob (grow-only, room for `total` bytes of files) and, on the first call, the per-file arrays and the
 * decoded pictures of max_batch files */
static int host_buffers(nhw_dec *d, size_t total)
{
	if (total + 64 > d->blob.cap) HIPCHK(nhw_grow(d->blob, total + (total >> 2) + (1u << 20)));   /* 64 spare bytes at least; a quarter and 1 MiB more when it grows, so that batches of a similar size do not reallocate */
	return d->d_off ? NHW_OK : dev_alloc(host_set(d), nullptr, d->max_batch, nhw_dec_err);   /* all five or none: a half-made set would hand null pointers to the next call */
}

/* what every host call checks of its scale and of its offsets off[0 .. n] */
static bool scale_ok(int scale)
{
	if (scale == 1 || scale == 2 || scale == 4) return true;
	nhw_dec_err = "the scale must be 1, 2 or 4";
	return false;
}

static bool offsets_ok(const uint64_t *off, int n, const char *who)
{
	for (int i = 0; i < n; i++) if (off[i + 1] < off[i]) { nhw_dec_err = std::string(who) + ": off[] must not decrease"; return false; }
	return true;
}

/* host convenience: H2D of the files, decode, D2H of the pixels.  nhw: the files back to back, off[n+1].  At scale 1, 2 or 4 (DESIGN.md section
 * 14), for any n >= 1: the files go up once and are decoded in chunks of max_batch; file i's 3 T T bytes (T = 512 / scale) land at out + i * 3 T T;
 * as grey its T T bytes at out + i * T T */
static int dec_batch_host(nhw_dec *d, const uint8_t *nhw, const uint64_t *off, int n, int scale, uint8_t *out, int32_t *status, int32_t *quality, const char *who, bool grey = false)
{
	if (!d || !nhw || !off || !out || !status || n < 1) { nhw_dec_err = "bad argument"; return NHW_E_ARG; }
	if (!scale_ok(scale) || !offsets_ok(off, n, who)) return NHW_E_ARG;
	HIPCHK(hipSetDevice(d->device));
	const size_t total = (size_t)(off[n] - off[0]), per = (size_t)NHW_IMG_BYTES / (size_t)(scale * scale) / (grey ? 3 : 1);
	{ const int rc = host_buffers(d, total); if (rc) return rc; }
	hipStream_t s = d->own_stream;
	HIPCHK(hipMemcpyAsync(d->blob.p, nhw + off[0], total, hipMemcpyHostToDevice, s));
	std::vector<uint64_t> rel((size_t)d->max_batch);
	std::vector<uint32_t> len((size_t)d->max_batch);
	for (int i0 = 0; i0 < n; i0 += d->max_batch) {
		const int m = n - i0 < d->max_batch ? n - i0 : d->max_batch;
		for (int i = 0; i < m; i++) {
			rel[i] = off[i0 + i] - off[0];
			const uint64_t l = off[i0 + i + 1] - off[i0 + i];
			len[i] = l > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)l;
		}
		HIPCHK(hipMemcpyAsync(d->d_off, rel.data(), (size_t)m * 8, hipMemcpyHostToDevice, s));
		HIPCHK(hipMemcpyAsync(d->d_len, len.data(), (size_t)m * 4, hipMemcpyHostToDevice, s));
		HIPCHK(hipStreamSynchronize(s));                              /* rel and len are filled again for the next chunk */
		const int rc = grey ? nhw_dec_batch_device_grey(d, d->blob.p, d->d_off, d->d_len, m, scale, nullptr, d->d_out, d->d_status, d->d_quality, s)
		                    : nhw_dec_batch_device_scaled(d, d->blob.p, d->d_off, d->d_len, m, scale, d->d_out, d->d_status, d->d_quality, s);
		if (rc) return rc;
		HIPCHK(hipMemcpyAsync(out + (size_t)i0 * per, d->d_out, (size_t)m * per, hipMemcpyDeviceToHost, s));
		HIPCHK(hipMemcpyAsync(status + i0, d->d_status, (size_t)m * 4, hipMemcpyDeviceToHost, s));
		if (quality) HIPCHK(hipMemcpyAsync(quality + i0, d->d_quality, (size_t)m * 4, hipMemcpyDeviceToHost, s));
		HIPCHK(hipStreamSynchronize(s));
	}
	return NHW_OK;
}

/* the full-size call takes one chunk: n <= max_batch */
extern "C" int nhw_dec_batch(nhw_dec *d, const uint8_t *nhw, const uint64_t *off, int n, uint8_t *bgr, int32_t *status, int32_t *quality)
{
	if (d && n > d->max_batch) { nhw_dec_err = "bad argument"; return NHW_E_ARG; }
	return dec_batch_host(d, nhw, off, n, 1, bgr, status, quality, "nhw_dec_batch");
}

extern "C" int nhw_dec_batch_scaled(nhw_dec *d, const uint8_t *nhw, const uint64_t *off, int n, int scale, uint8_t *out, int32_t *status, int32_t *quality)
{
	return dec_batch_host(d, nhw, off, n, scale, out, status, quality, "nhw_dec_batch_scaled");
}

/* the same as grey bytes: file i's T T bytes at out + i * T T, rows in file order */
extern "C" int nhw_dec_batch_grey(nhw_dec *d, const uint8_t *nhw, const uint64_t *off, int n, int scale, uint8_t *out, int32_t *status, int32_t *quality)
{
	return dec_batch_host(d, nhw, off, n, scale, out, status, quality, "nhw_dec_batch_grey", true);
}

/* ---------------------------------------------------------------------------------------------- pictures of any size (DESIGN.md sections 11, 13, 14) */
/* What nhw_dec_pictures and the region calls share: the plan of a call's tile files (nhw_tile_plan.h), the chunked decode of a list of tile
 * files, the status gather and the download of the results. */
static const size_t MAX_CALL_TILES = (size_t)(INT_MAX / 16);       /* the tiles one host call takes */

/* The tile files of a call, in the handle's blob (already on its way there on the handle's stream): offsets and lengths go up, the tiles are
 * decoded at `scale` in chunks of max_batch into the host path's picture slots, each chunk followed by crop(t0, m) -- the launch that takes the
 * decoded tiles [t0, t0 + m) out of d->d_out --, and the per-tile status comes back.  Synchronises the stream.  grey: the grey batch decode
 *  without a format, T T bytes a slot where the colour decode leaves 3 T T. */
template <class Crop>
static int decode_tile_list(nhw_dec *d, const std::vector<uint64_t> &toff, const std::vector<uint32_t> &tlen, int scale, std::vector<int32_t> &tst, Crop &&crop, bool grey = false)
{
	const int tiles = (int)toff.size();
	HIPCHK(nhw_grow(d->pic_tiles, (size_t)tiles * 16));
	uint64_t *d_toff = d->pic_tiles.as<uint64_t>();
	uint32_t *d_tlen = (uint32_t *)(d_toff + tiles);
	int32_t *d_tst = (int32_t *)(d_tlen + tiles);
	hipStream_t s = d->own_stream;
	HIPCHK(hipMemcpyAsync(d_toff, toff.data(), (size_t)tiles * 8, hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync(d_tlen, tlen.data(), (size_t)tiles * 4, hipMemcpyHostToDevice, s));
	for (int t0 = 0; t0 < tiles; t0 += d->max_batch) {
		const int m = tiles - t0 < d->max_batch ? tiles - t0 : d->max_batch;
		const int rc = grey ? nhw_dec_batch_device_grey(d, d->blob.p, d_toff + t0, d_tlen + t0, m, scale, nullptr, d->d_out, d_tst + t0, nullptr, s)
		                    : nhw_dec_batch_device_scaled(d, d->blob.p, d_toff + t0, d_tlen + t0, m, scale, d->d_out, d_tst + t0, nullptr, s);
		if (rc) return rc;
		HIPCHK(crop(t0, m));
	}
	tst.resize((size_t)tiles);
	HIPCHK(hipMemcpyAsync(tst.data(), d_tst, (size_t)tiles * 4, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return NHW_OK;
}

static int32_t tiles_status(const std::vector<int32_t> &tst, int t0, int t1)   /* NHW_OK if the tiles [t0, t1) all decoded */
{
	for (int t = t0; t < t1; t++) if (tst[t] != NHW_OK) return NHW_E_FORMAT;
	return NHW_OK;
}

/* the results whose status is NHW_OK, device -> host: desc[k] (a picture or a region: px width height bytes at addr, px bytes a pixel) is
 * entry which[k] of the call and goes to bgr + out_off[which[k]]; neighbours that are contiguous on both sides go as one copy */
template <class D>
static int download_decoded(uint8_t *bgr, const uint64_t *out_off, const std::vector<D> &desc, const std::vector<int> &which, const int32_t *status, uint64_t px = 3)
{
	struct Span { uint64_t dev, host, len; };
	std::vector<Span> sp;
	for (size_t k = 0; k < desc.size(); k++)
		if (status[which[k]] == NHW_OK) sp.push_back({ desc[k].addr, out_off[which[k]], px * desc[k].width * desc[k].height });
	for (size_t k = 0; k < sp.size();) {
		uint64_t len = sp[k].len;
		size_t j = k + 1;
		while (j < sp.size() && sp[j].dev == sp[k].dev + len && sp[j].host == sp[k].host + len) len += sp[j++].len;
		HIPCHK(hipMemcpy(bgr + sp[k].host, (const void *)(uintptr_t)sp[k].dev, len, hipMemcpyDeviceToHost));
		k = j;
	}
	return NHW_OK;
}

/* Plan every container on the host (plan_pictures); upload the blob once; decode the tiles in chunks of max_batch into the host path's
 * picture slots and crop each chunk into the picture buffer (k_untile_crop); then bring back the pictures whose tiles all decoded. */
static int dec_pictures(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n, int scale, uint8_t *bgr, const uint64_t *out_off, int32_t *status)
{
	if (!d || !blob || !off || !bgr || !out_off || !status || n < 1) { nhw_dec_err = "bad argument"; return NHW_E_ARG; }
	if (!scale_ok(scale) || !offsets_ok(off, n, "nhw_dec_pictures")) return NHW_E_ARG;
	PicturePlan p;
	if (const int rc = plan_pictures(blob, off, n, scale, MAX_CALL_TILES, p, status, nhw_dec_err)) return rc;
	if (p.desc.empty()) return NHW_OK;
	const int tiles = (int)p.toff.size(), np = (int)p.desc.size();
	HIPCHK(hipSetDevice(d->device));
	if (const int rc = host_buffers(d, (size_t)(off[n] - off[0]))) return rc;
	HIPCHK(nhw_grow(d->pic_px, p.bytes));
	HIPCHK(nhw_grow(d->pic_desc, (size_t)np * sizeof(nhw_picture)));
	for (nhw_picture &g : p.desc) g.addr += (uint64_t)(uintptr_t)d->pic_px.p;
	const nhw_picture *d_desc = d->pic_desc.as<nhw_picture>();
	hipStream_t s = d->own_stream;
	HIPCHK(hipMemcpyAsync(d->blob.p, blob + off[0], (size_t)(off[n] - off[0]), hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync(d->pic_desc.p, p.desc.data(), (size_t)np * sizeof(nhw_picture), hipMemcpyHostToDevice, s));
	std::vector<int32_t> tst;
	if (const int rc = decode_tile_list(d, p.toff, p.tlen, scale, tst, [&](int t0, int m) { return nhw_launch_untile_crop(d->d_out, d_desc, np, t0, m, scale, s); })) return rc;
	for (int k = 0; k < np; k++) status[p.which[k]] = tiles_status(tst, (int)p.desc[k].first_tile, k + 1 < np ? (int)p.desc[k + 1].first_tile : tiles);
	return download_decoded(bgr, out_off, p.desc, p.which, status);
}

extern "C" int nhw_dec_pictures(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n, uint8_t *bgr, const uint64_t *out_off, int32_t *status)
{
	return dec_pictures(d, blob, off, n, 1, bgr, out_off, status);
}

/* the same at scale 2 or 4 (1: nhw_dec_pictures): picture i is ceil(W / scale) x ceil(H / scale), made from the half- or quarter-scale decode of its tiles */
extern "C" int nhw_dec_pictures_scaled(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n, int scale, uint8_t *out, const uint64_t *out_off, int32_t *status)
{
	return dec_pictures(d, blob, off, n, scale, out, out_off, status);
}

/* ---------------------------------------------------------------------------------------------- regions and windows (DESIGN.md sections 13, 15) */
/* The region, window, crop and warp calls are one function, dec_windows: checks, the plan of the call's tiles (plan_windows in
 * nhw_tile_plan.h: a window call takes the union of its windows' selections; a region call is a window call at scale 1 with `merge` off),
 * upload, the chunked decode with k_untile_window behind each chunk, the statuses, and one of three finishes.  A grey call (DESIGN.md
 * section 23) is the same function at one byte a pixel: the grey decode underneath, k_untile_window_grey behind each chunk, the one-channel
 * resamplers and warp at the end; the plan's tiles, and with them the statuses, are the colour call's. */
enum WindowsMode {
	WIN_TO_HOST,                                                 /* bgr / out_off: the rectangles packed in a device buffer of the handle, then downloaded (download_decoded) */
	WIN_TO_DEVICE,                                               /* dst_addr / dst_pitch: cropped straight into the caller's device memory; nothing is left to do */
	WIN_TO_TENSORS                                               /* crop, dst_addr the tensors' addresses: packed as for the host form, then resampled or warped (crops_finish) */
};
/* what a crop or warp call samples its windows with: NhwSampleCall's fields (nhw_tensor.h) as the caller gave them -- the warps (null: a crop call, under `filter`) and the
 * tables of ops, one entry a rect, each null for "none", are in HOST memory; crops_finish uploads them */
struct CropSpec { NhwTensorOut out; int filter; const nhw_warp *warps; NhwOpsArgs ops; };
struct WindowsCall {
	WindowsMode mode = WIN_TO_HOST;
	uint8_t *bgr = nullptr; const uint64_t *out_off = nullptr, *dst_addr = nullptr, *dst_pitch = nullptr;
	const CropSpec *crop = nullptr;
	bool merge = true;
	bool grey = false;
	const char *who = "";
};

static int windows_check(const nhw_dec *d, const uint8_t *blob, const uint64_t *off, int nc, const nhw_rect *rects, int nr, int scale, const int32_t *status, const WindowsCall &c)
{
	const bool dst = c.mode == WIN_TO_HOST ? c.bgr && c.out_off : c.mode == WIN_TO_DEVICE ? c.dst_addr && c.dst_pitch : c.dst_addr && c.crop;
	if (!d || !blob || !off || !rects || !status || nc < 1 || nr < 1 || !dst) { nhw_dec_err = "bad argument"; return NHW_E_ARG; }
	if (!scale_ok(scale)) return NHW_E_ARG;
	if (c.grey && d->stop_after) { nhw_dec_err = "a grey decode has no debug stops: the handle has one set"; return NHW_E_ARG; }
	if (scale != 1 && d->stop_after) { nhw_dec_err = "a scaled decode has no debug stops: the handle has one set"; return NHW_E_ARG; }
	if (!offsets_ok(off, nc, c.who)) return NHW_E_ARG;
	if (c.mode == WIN_TO_DEVICE) for (int i = 0; i < nr; i++) if (!c.dst_addr[i] || c.dst_pitch[i] < (c.grey ? 1ull : 3ull) * rects[i].width) { nhw_dec_err = std::string(c.who) + (c.grey ? ": a destination needs an address and a pitch of at least the width" : ": a destination needs an address and a pitch of at least 3 x width"); return NHW_E_ARG; }
	if (c.mode == WIN_TO_TENSORS) for (int i = 0; i < nr; i++) if (!c.dst_addr[i] || c.dst_addr[i] % (c.crop->out.dtype == NHW_T_U8 ? 1u : c.crop->out.dtype == NHW_T_F32 ? 4u : 2u)) { nhw_dec_err = std::string(c.who) + ": a destination needs an address that is a multiple of the element size"; return NHW_E_ARG; }
	return NHW_OK;
}

/* The rects a crop or warp call refuses (NHW_E_ARG) before they select a tile: with the area filter or the cubic one
 * (section 20), a rect whose window is beyond the filter's reduction limit for the output size; with warps (section 21), one whose warp is
 * beyond the limits; with maps (section 24), one whose map is. */
static std::vector<uint8_t> crop_refusals(const CropSpec &crop, const nhw_rect *rects, int nr)
{
	const uint64_t limit = nhw_filter_limit(crop.filter);               /* 0 for none */
	std::vector<uint8_t> refused((size_t)nr);
	for (int i = 0; i < nr; i++)
		refused[(size_t)i] = (limit && (rects[i].width > limit * crop.out.w || rects[i].height > limit * crop.out.h)) || (crop.warps && !nhw_warp_within(crop.warps[i])) ||
		                     (crop.ops.maps && !nhw_colour_within(crop.ops.maps[i]));
	return refused;
}

/* A plan on its way to the device on the handle's stream: the files as one blob, the descriptors into pic_desc and the use table behind
 * them.  With `staged` the windows are packed in pic_px: the descriptors' running offsets become addresses in it. */
static int upload_plan(nhw_dec *d, TilePlan &p, bool staged)
{
	HIPCHK(hipSetDevice(d->device));
	if (const int rc = host_buffers(d, p.files.size())) return rc;
	const size_t desc_bytes = p.desc.size() * sizeof(nhw_region), use_bytes = p.uses.size() * sizeof(nhw_window_use);   /* (48 a descriptor, a multiple of 16: the use table behind them is aligned) */
	HIPCHK(nhw_grow(d->pic_desc, desc_bytes + use_bytes));
	if (staged) {
		HIPCHK(nhw_grow(d->pic_px, p.bytes));
		for (nhw_region &g : p.desc) g.addr += (uint64_t)(uintptr_t)d->pic_px.p;
	}
	hipStream_t s = d->own_stream;
	HIPCHK(hipMemcpyAsync(d->blob.p, p.files.data(), p.files.size(), hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync(d->pic_desc.p, p.desc.data(), desc_bytes, hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync(d->pic_desc.as<uint8_t>() + desc_bytes, p.uses.data(), use_bytes, hipMemcpyHostToDevice, s));
	d->reg_tiles = p.toff.size(); d->reg_bytes = p.files.size();
	return NHW_OK;
}

/* The finish of the crop and warp calls (DESIGN.md sections 18 to 21).  The windows lie packed in the handle's staging; one launch takes every
 * window whose tiles all decoded to its tensor.  crop_tab holds what the launch reads, one entry a rect: nr pictures (32 bytes each; a rect
 * that has no window keeps a zero picture), nr tensor addresses (0 for a rect without a window or with a tile that failed, which the kernel
 * passes over), and behind them either the nr flag bytes -- k_resize_to_tensor, k_area_to_tensor or k_cubic_to_tensor by the filter -- or
 * the nr warps (32 + 8 bytes an entry in front: they are 8-byte aligned) -- k_warp_to_tensor, warps[i] sampling window i along its tilted grid.
 * A mapped call (section 24) has its nr colour maps behind that table, at the next multiple of 8, and launches the mapped forms of the same kernels.
 * A toned call (section 25) has its nr tone tables behind the maps (64 bytes each: a multiple of 8 again), or in their place where it has none,
 * and launches the toned forms.  The launch is one call: the tables that are there make the record's (NhwSampleCall), and nhw_launch_sample finds the kernel. */
static int crops_finish(nhw_dec *d, const TilePlan &p, const CropSpec &crop, const uint64_t *dst_addr, int nr, const int32_t *status, bool grey)
{
	static_assert(sizeof(nhw_warp) == 40 && sizeof(nhw_picture) == 32, "the crop table's layout");
	std::vector<nhw_picture> pics((size_t)nr, nhw_picture{ 0, 0, 0, 0, 0, 0 });
	std::vector<uint64_t> oaddr((size_t)nr, 0);
	for (size_t k = 0; k < p.desc.size(); k++) {
		const size_t i = (size_t)p.which[k];
		pics[i] = { p.desc[k].addr, p.desc[k].pitch, p.desc[k].width, p.desc[k].height, 0, 0 };
		if (status[i] == NHW_OK) oaddr[i] = dst_addr[i];
	}
	const NhwOpsArgs &h = crop.ops;                                      /* the caller's tables, in host memory */
	const size_t pics_bytes = (size_t)nr * sizeof(nhw_picture), addr_bytes = (size_t)nr * 8;
	const size_t last_bytes = ((size_t)nr * (crop.warps ? sizeof(nhw_warp) : 1) + 7) & ~(size_t)7, maps_bytes = h.maps ? (size_t)nr * sizeof(nhw_colour_map) : 0;
	const size_t tones_bytes = h.tones ? (size_t)nr * sizeof(nhw_tone_table) : 0;
	HIPCHK(nhw_grow(d->crop_tab, pics_bytes + addr_bytes + last_bytes + maps_bytes + tones_bytes));
	uint8_t *tab = d->crop_tab.as<uint8_t>(), *last = tab + pics_bytes + addr_bytes, *maps = last + last_bytes, *tones = maps + maps_bytes;
	hipStream_t s = d->own_stream;
	HIPCHK(hipMemcpyAsync(tab, pics.data(), pics_bytes, hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync(tab + pics_bytes, oaddr.data(), addr_bytes, hipMemcpyHostToDevice, s));
	if (h.maps) HIPCHK(hipMemcpyAsync(maps, h.maps, maps_bytes, hipMemcpyHostToDevice, s));
	if (h.tones) HIPCHK(hipMemcpyAsync(tones, h.tones, tones_bytes, hipMemcpyHostToDevice, s));
	if (crop.warps) HIPCHK(hipMemcpyAsync(last, crop.warps, (size_t)nr * sizeof(nhw_warp), hipMemcpyHostToDevice, s));
	else if (h.flags) HIPCHK(hipMemcpyAsync(last, h.flags, (size_t)nr, hipMemcpyHostToDevice, s));
	const NhwOpsArgs dev = { crop.warps || !h.flags ? nullptr : last, h.maps ? (const nhw_colour_map *)maps : nullptr, h.tones ? (const nhw_tone_table *)tones : nullptr };
	HIPCHK(nhw_launch_sample({ (const nhw_picture *)tab, nr, crop.out, grey, crop.filter, crop.warps ? (const nhw_warp *)last : nullptr, dev, (const uint64_t *)(tab + pics_bytes) }, s));
	HIPCHK(hipStreamSynchronize(s));
	return NHW_OK;
}

/* A rect's status is the worst of its own tiles': NHW_E_FORMAT where one of them did not decode. */
static int dec_windows(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int nc, const nhw_rect *rects, int nr, int scale, int32_t *status, const WindowsCall &c)
{
	if (const int rc = windows_check(d, blob, off, nc, rects, nr, scale, status, c)) return rc;
	d->reg_tiles = d->reg_bytes = 0;
	const std::vector<uint8_t> refused = c.crop ? crop_refusals(*c.crop, rects, nr) : std::vector<uint8_t>();
	const bool to_device = c.mode == WIN_TO_DEVICE;
	TilePlan p;
	if (const int rc = plan_windows({ blob, off, nc, rects, nr, scale, c.merge, c.crop ? refused.data() : nullptr, to_device ? c.dst_addr : nullptr, to_device ? c.dst_pitch : nullptr,
	                                  c.who, MAX_CALL_TILES, c.grey ? 1u : 3u }, p, status, nhw_dec_err)) return rc;
	if (p.desc.empty()) return NHW_OK;
	if (const int rc = upload_plan(d, p, !to_device)) return rc;
	const int ng = (int)p.desc.size();
	const nhw_region *d_desc = d->pic_desc.as<nhw_region>();
	const nhw_window_use *d_uses = (const nhw_window_use *)(d_desc + ng);
	std::vector<int32_t> tst;
	if (const int rc = decode_tile_list(d, p.toff, p.tlen, scale, tst, [&](int t0, int m) {
		const auto launch = c.grey ? nhw_launch_untile_window_grey : nhw_launch_untile_window;
		return launch(d->d_out, d_desc, ng, d_uses + p.first_use[t0], p.first_use[t0 + m] - p.first_use[t0], t0, m, scale, d->own_stream); }, c.grey)) return rc;
	for (const nhw_window_use &u : p.uses)
		if (tst[u.slot] != NHW_OK) status[p.which[u.region]] = NHW_E_FORMAT;
	switch (c.mode) {
	case WIN_TO_HOST: return download_decoded(c.bgr, c.out_off, p.desc, p.which, status, c.grey ? 1 : 3);
	case WIN_TO_TENSORS: return crops_finish(d, p, *c.crop, c.dst_addr, nr, status, c.grey);
	default: return NHW_OK;
	}
}

extern "C" int nhw_dec_regions(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects,
                               uint8_t *bgr, const uint64_t *out_off, int32_t *status)
{
	WindowsCall c;
	c.mode = WIN_TO_HOST; c.bgr = bgr; c.out_off = out_off; c.merge = false; c.who = "nhw_dec_regions";
	return dec_windows(d, blob, off, n_containers, rects, n_rects, 1, status, c);
}

extern "C" int nhw_dec_regions_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects,
                                         const uint64_t *dst_addr, const uint64_t *dst_pitch, int32_t *status)
{
	WindowsCall c;
	c.mode = WIN_TO_DEVICE; c.dst_addr = dst_addr; c.dst_pitch = dst_pitch; c.merge = false; c.who = "nhw_dec_regions_to_device";
	return dec_windows(d, blob, off, n_containers, rects, n_rects, 1, status, c);
}

extern "C" int nhw_dec_windows(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                               uint8_t *bgr, const uint64_t *out_off, int32_t *status)
{
	WindowsCall c;
	c.mode = WIN_TO_HOST; c.bgr = bgr; c.out_off = out_off; c.who = "nhw_dec_windows";
	return dec_windows(d, blob, off, n_containers, rects, n_rects, scale, status, c);
}

extern "C" int nhw_dec_windows_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                         const uint64_t *dst_addr, const uint64_t *dst_pitch, int32_t *status)
{
	WindowsCall c;
	c.mode = WIN_TO_DEVICE; c.dst_addr = dst_addr; c.dst_pitch = dst_pitch; c.who = "nhw_dec_windows_to_device";
	return dec_windows(d, blob, off, n_containers, rects, n_rects, scale, status, c);
}

/* nhw_dec_windows_to_device with a sampler behind it: window i to the tensor at dst_addr[i], out_width x out_height -- resampled under `filter` and
 * mirrored where bit 0 of flags[i] is set (DESIGN.md sections 18 to 20), or sampled along the tilted grid of warps[i] in place of filter and flags
 * (section 21); as colour or as grey (section 23), with a colour map (section 24) or a tone table (section 25) a rect.  The ten entries are one body,
 * dec_samples, and a row of the table below says what an entry's checks are.
 * A filter an entry does not take is refused in that entry's words and at that entry's place among the checks, which callers can tell apart by
 * the message they get for two mistakes at once: the two oldest entries look at dst_addr, the tables and n_rects first (`filter_first` off), every
 * later one at the filter.  Then come the sides and the format, and dec_windows' own checks. */
struct SamplesEntry {
	const char *who;             /* the entry as nhw_tensor_out_check and dec_windows' messages name it */
	const char *filter_who;      /* ... and as the filter's message does; null: a warp entry, whose `warps` must not be NULL */
	int last_filter;             /* the filters taken: NHW_FILTER_TWO_TAP .. this one */
	bool filter_first;
	NhwFamily family;
	bool maps, tones;            /* the tables that must not be NULL (a toned entry's maps may be) */
};
/* nhw_dec_crops_to_device and nhw_dec_crops_to_device_filter are the row CROPS: the second keeps refusing the cubic filter.  nhw_dec_crops_to_device_resample
 * takes it and says so under its own name, but is nhw_dec_crops_to_device in every other message */
static const SamplesEntry
	CROPS          = { "nhw_dec_crops_to_device",        "nhw_dec_crops_to_device",          NHW_FILTER_AREA,  false, NHW_FAMILY_COLOUR,    false, false },
	CROPS_RESAMPLE = { "nhw_dec_crops_to_device",        "nhw_dec_crops_to_device_resample", NHW_FILTER_CUBIC, true,  NHW_FAMILY_COLOUR,    false, false },
	WARPS          = { "nhw_dec_warps_to_device",        nullptr,                            0,                false, NHW_FAMILY_COLOUR,    false, false },
	CROPS_GREY     = { "nhw_dec_crops_grey_to_device",   "nhw_dec_crops_grey_to_device",     NHW_FILTER_CUBIC, true,  NHW_FAMILY_GREY,      false, false },
	WARPS_GREY     = { "nhw_dec_warps_grey_to_device",   nullptr,                            0,                false, NHW_FAMILY_GREY,      false, false },
	CROPS_MAPPED   = { "nhw_dec_crops_mapped_to_device", "nhw_dec_crops_mapped_to_device",   NHW_FILTER_CUBIC, true,  NHW_FAMILY_BY_FORMAT, true,  false },
	WARPS_MAPPED   = { "nhw_dec_warps_mapped_to_device", nullptr,                            0,                false, NHW_FAMILY_BY_FORMAT, true,  false },
	CROPS_TONED    = { "nhw_dec_crops_toned_to_device",  "nhw_dec_crops_toned_to_device",    NHW_FILTER_CUBIC, true,  NHW_FAMILY_BY_FORMAT, false, true  },
	WARPS_TONED    = { "nhw_dec_warps_toned_to_device",  nullptr,                            0,                false, NHW_FAMILY_BY_FORMAT, false, true  };

static int dec_samples(const SamplesEntry &e, nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                       uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, int filter, const nhw_warp *warps, const NhwOpsArgs &ops, const uint64_t *dst_addr, int32_t *status)
{
	static const char *const must[] = { ": the filter must be NHW_FILTER_TWO_TAP or NHW_FILTER_AREA", ": the filter must be NHW_FILTER_TWO_TAP, NHW_FILTER_AREA or NHW_FILTER_CUBIC" };
	const bool taken = !e.filter_who || (filter >= NHW_FILTER_TWO_TAP && filter <= e.last_filter);
	if (!taken && e.filter_first) { nhw_dec_err = std::string(e.filter_who) + must[e.last_filter == NHW_FILTER_CUBIC]; return NHW_E_ARG; }
	if (!dst_addr || (!e.filter_who && !warps) || (e.maps && !ops.maps) || (e.tones && !ops.tones) || n_rects > (1 << 24)) { nhw_dec_err = "bad argument"; return NHW_E_ARG; }
	if (!taken) { nhw_dec_err = std::string(e.filter_who) + must[e.last_filter == NHW_FILTER_CUBIC]; return NHW_E_ARG; }
	WindowsCall c;
	c.mode = WIN_TO_TENSORS; c.dst_addr = dst_addr; c.grey = nhw_family_grey(e.family, fmt); c.who = e.who;
	CropSpec crop = { {}, filter, warps, ops };
	if (const int rc = nhw_tensor_out_check(e.who, out_width, out_height, fmt, &crop.out, nhw_dec_err, c.grey)) return rc;
	c.crop = &crop;
	return dec_windows(d, blob, off, n_containers, rects, n_rects, scale, status, c);
}

extern "C" int nhw_dec_crops_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                       uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr, int32_t *status)
{ return dec_samples(CROPS, d, blob, off, n_containers, rects, n_rects, scale, out_width, out_height, fmt, NHW_FILTER_TWO_TAP, nullptr, { flags, nullptr, nullptr }, dst_addr, status); }

extern "C" int nhw_dec_crops_to_device_filter(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                              uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr, int32_t *status, int filter)
{ return dec_samples(CROPS, d, blob, off, n_containers, rects, n_rects, scale, out_width, out_height, fmt, filter, nullptr, { flags, nullptr, nullptr }, dst_addr, status); }

extern "C" int nhw_dec_crops_to_device_resample(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                                uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr, int *status, int filter)
{
	static_assert(sizeof(int) == sizeof(int32_t), "the statuses are 32 bits wide");
	return dec_samples(CROPS_RESAMPLE, d, blob, off, n_containers, rects, n_rects, scale, out_width, out_height, fmt, filter, nullptr, { flags, nullptr, nullptr }, dst_addr, (int32_t *)status);
}

extern "C" int nhw_dec_warps_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                       uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const nhw_warp *warps, const uint64_t *dst_addr, int32_t *status)
{ return dec_samples(WARPS, d, blob, off, n_containers, rects, n_rects, scale, out_width, out_height, fmt, NHW_FILTER_TWO_TAP, warps, {}, dst_addr, status); }

extern "C" int nhw_dec_crops_grey_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                            uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr, int32_t *status, int filter)
{ return dec_samples(CROPS_GREY, d, blob, off, n_containers, rects, n_rects, scale, out_width, out_height, fmt, filter, nullptr, { flags, nullptr, nullptr }, dst_addr, status); }

extern "C" int nhw_dec_warps_grey_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                            uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const nhw_warp *warps, const uint64_t *dst_addr, int32_t *status)
{ return dec_samples(WARPS_GREY, d, blob, off, n_containers, rects, n_rects, scale, out_width, out_height, fmt, NHW_FILTER_TWO_TAP, warps, {}, dst_addr, status); }

extern "C" int nhw_dec_crops_mapped_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                              uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const nhw_colour_map *maps, const uint64_t *dst_addr, int32_t *status, int filter)
{ return dec_samples(CROPS_MAPPED, d, blob, off, n_containers, rects, n_rects, scale, out_width, out_height, fmt, filter, nullptr, { flags, maps, nullptr }, dst_addr, status); }

extern "C" int nhw_dec_warps_mapped_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                              uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const nhw_warp *warps, const nhw_colour_map *maps, const uint64_t *dst_addr, int32_t *status)
{ return dec_samples(WARPS_MAPPED, d, blob, off, n_containers, rects, n_rects, scale, out_width, out_height, fmt, NHW_FILTER_TWO_TAP, warps, { nullptr, maps, nullptr }, dst_addr, status); }

extern "C" int nhw_dec_crops_toned_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                             uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const nhw_colour_map *maps, const nhw_tone_table *tones, const uint64_t *dst_addr, int32_t *status, int filter)
{ return dec_samples(CROPS_TONED, d, blob, off, n_containers, rects, n_rects, scale, out_width, out_height, fmt, filter, nullptr, { flags, maps, tones }, dst_addr, status); }

extern "C" int nhw_dec_warps_toned_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                             uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const nhw_warp *warps, const nhw_colour_map *maps, const nhw_tone_table *tones, const uint64_t *dst_addr, int32_t *status)
{ return dec_samples(WARPS_TONED, d, blob, off, n_containers, rects, n_rects, scale, out_width, out_height, fmt, NHW_FILTER_TWO_TAP, warps, { nullptr, maps, tones }, dst_addr, status); }

/* ---------------------------------------------------------------------------------------------- the window calls at one byte a pixel */
extern "C" int nhw_dec_windows_grey(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                    uint8_t *out, const uint64_t *out_off, int32_t *status)
{
	WindowsCall c;
	c.mode = WIN_TO_HOST; c.bgr = out; c.out_off = out_off; c.grey = true; c.who = "nhw_dec_windows_grey";
	return dec_windows(d, blob, off, n_containers, rects, n_rects, scale, status, c);
}

extern "C" int nhw_dec_windows_grey_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                              const uint64_t *dst_addr, const uint64_t *dst_pitch, int32_t *status)
{
	WindowsCall c;
	c.mode = WIN_TO_DEVICE; c.dst_addr = dst_addr; c.dst_pitch = dst_pitch; c.grey = true; c.who = "nhw_dec_windows_grey_to_device";
	return dec_windows(d, blob, off, n_containers, rects, n_rects, scale, status, c);
}

extern "C" int nhw_dec_last_region_stats(nhw_dec *d, uint64_t *tiles_decoded, uint64_t *bytes_uploaded)
{
	if (!d || !tiles_decoded || !bytes_uploaded) { nhw_dec_err = "bad argument"; return NHW_E_ARG; }
	*tiles_decoded = d->reg_tiles; *bytes_uploaded = d->reg_bytes;
	return NHW_OK;
}

/* the 54-byte header nhw-dec writes in front of the pixels (nhw_decoder_cli.c:61-65, :293-312) */
extern "C" void nhw_dec_bmp_header(uint8_t h[54])
{
	static const uint8_t base[54] = { 66,77,54,0,12,0,0,0,0,0, 54,0,0,0,40,0,0,0,0,2, 0,0,0,2,0,0,1,0,24,0, 0,0,0,0,0,0,12,0,0,0 };
	memcpy(h, base, 54);
}
