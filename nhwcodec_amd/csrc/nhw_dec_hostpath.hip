/* nhw_dec_hostpath.hip -- the decoder's host conveniences: files in host memory in, pictures out (nhw_dec_batch), pictures of any size and regions of them out of
 * .nhwp containers (nhw_dec_pictures, nhw_dec_regions*, nhw_dec_windows*, nhw_dec_crops_to_device*), the BMP header.  They reach the kernels only through nhw_dec_batch_device (nhw_dec.hip), nhw_picture.hip and nhw_resample.hip. */
#include "nhw_dec.h"
#include "nhw_tensor.h"

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
 * 14), for any n >= 1: the files go up once and are decoded in chunks of max_batch; file i's 3 T T bytes (T = 512 / scale) land at out + i * 3 T T */
static int dec_batch_host(nhw_dec *d, const uint8_t *nhw, const uint64_t *off, int n, int scale, uint8_t *out, int32_t *status, int32_t *quality, const char *who)
{
	if (!d || !nhw || !off || !out || !status || n < 1) { nhw_dec_err = "bad argument"; return NHW_E_ARG; }
	if (!scale_ok(scale) || !offsets_ok(off, n, who)) return NHW_E_ARG;
	HIPCHK(hipSetDevice(d->device));
	const size_t total = (size_t)(off[n] - off[0]), per = (size_t)NHW_IMG_BYTES / (size_t)(scale * scale);
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
		const int rc = nhw_dec_batch_device_scaled(d, d->blob.p, d->d_off, d->d_len, m, scale, d->d_out, d->d_status, d->d_quality, s);
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

/* ---------------------------------------------------------------------------------------------- pictures of any size (DESIGN.md sections 11, 13, 14) */
/* What nhw_dec_pictures and the region calls share: a container's directory, the chunked decode of a list of tile files, the status
 * gather and the download of the results. */
static uint32_t dir_len(const uint8_t *dir, int k)                /* length of tile file k in a container's directory */
{
	return (uint32_t)dir[4 * k] | ((uint32_t)dir[4 * k + 1] << 8) | ((uint32_t)dir[4 * k + 2] << 16) | ((uint32_t)dir[4 * k + 3] << 24);
}

static const size_t MAX_CALL_TILES = (size_t)(INT_MAX / 16);       /* the tiles one host call takes */

/* The tile files of a call, in the handle's blob (already on its way there on the handle's stream): offsets and lengths go up, the tiles are
 * decoded at `scale` in chunks of max_batch into the host path's picture slots, each chunk followed by crop(t0, m) -- the launch that takes the
 * decoded tiles [t0, t0 + m) out of d->d_out --, and the per-tile status comes back.  Synchronises the stream. */
template <class Crop>
static int decode_tile_list(nhw_dec *d, const std::vector<uint64_t> &toff, const std::vector<uint32_t> &tlen, int scale, std::vector<int32_t> &tst, Crop &&crop)
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
		const int rc = nhw_dec_batch_device_scaled(d, d->blob.p, d_toff + t0, d_tlen + t0, m, scale, d->d_out, d_tst + t0, nullptr, s);
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

/* the results whose status is NHW_OK, device -> host: desc[k] (a picture or a region: 3 width height bytes at addr) is entry which[k] of the
 * call and goes to bgr + out_off[which[k]]; neighbours that are contiguous on both sides go as one copy */
template <class D>
static int download_decoded(uint8_t *bgr, const uint64_t *out_off, const std::vector<D> &desc, const std::vector<int> &which, const int32_t *status)
{
	struct Span { uint64_t dev, host, len; };
	std::vector<Span> sp;
	for (size_t k = 0; k < desc.size(); k++)
		if (status[which[k]] == NHW_OK) sp.push_back({ desc[k].addr, out_off[which[k]], 3ull * desc[k].width * desc[k].height });
	for (size_t k = 0; k < sp.size();) {
		uint64_t len = sp[k].len;
		size_t j = k + 1;
		while (j < sp.size() && sp[j].dev == sp[k].dev + len && sp[j].host == sp[k].host + len) len += sp[j++].len;
		HIPCHK(hipMemcpy(bgr + sp[k].host, (const void *)(uintptr_t)sp[k].dev, len, hipMemcpyDeviceToHost));
		k = j;
	}
	return NHW_OK;
}

/* Parse every container on the host; upload the blob once (a container's tile files lie back to back, so the decoder's offsets and lengths
 * come from its directory); decode the tiles in chunks of max_batch into the host path's picture slots and crop each chunk into the
 * picture buffer (k_untile_crop); then bring back the pictures whose tiles all decoded. */
static int dec_pictures(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n, int scale, uint8_t *bgr, const uint64_t *out_off, int32_t *status)
{
	if (!d || !blob || !off || !bgr || !out_off || !status || n < 1) { nhw_dec_err = "bad argument"; return NHW_E_ARG; }
	if (!scale_ok(scale) || !offsets_ok(off, n, "nhw_dec_pictures")) return NHW_E_ARG;
	std::vector<nhw_picture> desc;
	std::vector<int> which;                                      /* desc[k] is container which[k] */
	std::vector<uint64_t> toff;
	std::vector<uint32_t> tlen;
	uint64_t bytes = 0;
	for (int i = 0; i < n; i++) {
		uint32_t w = 0, h = 0;
		int t = 0;
		const uint8_t *dir = nullptr;
		status[i] = NHW_E_FORMAT;
		if (nhw_container_parse(blob + off[i], (size_t)(off[i + 1] - off[i]), &w, &h, &t, &dir) != NHW_OK) continue;
		if (toff.size() + (size_t)t > MAX_CALL_TILES) { nhw_dec_err = "nhw_dec_pictures: too many tiles in one call"; return NHW_E_ARG; }
		status[i] = NHW_OK;
		nhw_picture_scaled_size(w, h, scale, &w, &h);                 /* the table describes the destination; the tile count is that of the whole picture */
		desc.push_back({ bytes, 3ull * w, w, h, (uint32_t)toff.size(), 0 });
		which.push_back(i);
		uint64_t fo = off[i] - off[0] + 16 + 4 * (uint64_t)t;
		for (int k = 0; k < t; k++) { toff.push_back(fo); tlen.push_back(dir_len(dir, k)); fo += tlen.back(); }
		bytes += 3ull * w * h;
	}
	if (desc.empty()) return NHW_OK;
	const int tiles = (int)toff.size(), np = (int)desc.size();
	HIPCHK(hipSetDevice(d->device));
	{ const int rc = host_buffers(d, (size_t)(off[n] - off[0])); if (rc) return rc; }
	HIPCHK(nhw_grow(d->pic_px, bytes));
	HIPCHK(nhw_grow(d->pic_desc, (size_t)np * sizeof(nhw_picture)));
	for (nhw_picture &p : desc) p.addr += (uint64_t)(uintptr_t)d->pic_px.p;
	const nhw_picture *d_desc = d->pic_desc.as<nhw_picture>();
	hipStream_t s = d->own_stream;
	HIPCHK(hipMemcpyAsync(d->blob.p, blob + off[0], (size_t)(off[n] - off[0]), hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync(d->pic_desc.p, desc.data(), (size_t)np * sizeof(nhw_picture), hipMemcpyHostToDevice, s));
	std::vector<int32_t> tst;
	{ const int rc = decode_tile_list(d, toff, tlen, scale, tst, [&](int t0, int m) { return nhw_launch_untile_crop(d->d_out, d_desc, np, t0, m, scale, s); }); if (rc) return rc; }
	for (int k = 0; k < np; k++) status[which[k]] = tiles_status(tst, (int)desc[k].first_tile, k + 1 < np ? (int)desc[k + 1].first_tile : tiles);
	return download_decoded(bgr, out_off, desc, which, status);
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

/* a container as the region and window calls see it: parsed once, when the first rect names it; start[k] = byte offset of tile file k in it */
struct RegionSource {
	int state;                                                   /* 0 not looked at, 1 well-formed, -1 malformed */
	uint32_t w, h;
	int t;
	const uint8_t *dir;
	std::vector<uint64_t> start;                                 /* t + 1 entries */
};

static void source_look(RegionSource &c, const uint8_t *base, size_t len)   /* the first look at a container */
{
	if (c.state != 0) return;
	c.state = nhw_container_parse(base, len, &c.w, &c.h, &c.t, &c.dir) == NHW_OK ? 1 : -1;
	if (c.state == 1) {
		c.start.resize((size_t)c.t + 1);
		c.start[0] = 16 + 4 * (uint64_t)c.t;
		for (int k = 0; k < c.t; k++) c.start[k + 1] = c.start[k] + dir_len(c.dir, k);
	}
}

/* ---------------------------------------------------------------------------------------------- regions and windows (DESIGN.md sections 13, 15) */
/* The region and window calls: bgr / out_off (the rectangles packed in a device buffer of the handle, then downloaded) or dst_addr / dst_pitch
 * (cropped straight into the caller's device memory).  The tiles of a window call are the union of the windows' selections: a tile gets a
 * slot when the first window selects it (slot_of, per container).  A region call is a window call at scale 1 with `merge` off: every selected
 * tile of every rect gets a slot and a copy of its file of its own (section 13's contract: nhw_dec_last_region_stats counts them).  Only the
 * files of the slots are gathered on the host, slot after slot, go up as one blob and are decoded as the tiles of whole pictures are; every
 * (window, tile) pair is a use, and the uses sorted by slot (without merging: the order they were made in) make the chunk [t0, t0 + m) of
 * decoded tiles the owner of the contiguous range [first_use[t0], first_use[t0 + m)), which k_untile_window crops behind the chunk.  A
 * window's status is the worst of its own tiles'.
 * The crop call is the third form: `crop` set, dst_addr the tensors' addresses.  The windows are cropped into the handle's
 * staging as for the host form and stay there; behind the last chunk one k_resize_to_tensor takes every window whose tiles all decoded to its
 * tensor -- the others get the address 0, which the kernel passes over.  With the area filter that launch is
 * k_area_to_tensor, with the cubic filter (section 20) k_cubic_to_tensor, and a rect whose window is beyond the filter's reduction limit for
 * the output size is NHW_E_ARG before it selects a tile.  With `warps` set the launch is k_warp_to_tensor instead: warps[i]
 * samples window i along its tilted grid, the table of warps goes up behind the addresses where the flags would, and a rect whose warp is
 * beyond the limits is NHW_E_ARG before it selects a tile. */
struct CropSpec { uint32_t out_w, out_h; int dtype, layout; NhwTensorArgs a; const uint8_t *flags; int filter; const nhw_warp *warps; };

static int dec_windows(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int nc, const nhw_rect *rects, int nr, int scale, uint8_t *bgr,
                       const uint64_t *out_off, const uint64_t *dst_addr, const uint64_t *dst_pitch, int32_t *status, const char *who, bool merge = true,
                       const CropSpec *crop = nullptr)
{
	const bool to_device = dst_addr != nullptr && !crop;
	if (!d || !blob || !off || !rects || !status || nc < 1 || nr < 1 || (crop ? !dst_addr : to_device ? !dst_pitch : (!bgr || !out_off))) { nhw_dec_err = "bad argument"; return NHW_E_ARG; }
	if (!scale_ok(scale)) return NHW_E_ARG;
	if (scale != 1 && d->stop_after) { nhw_dec_err = "a scaled decode has no debug stops: the handle has one set"; return NHW_E_ARG; }
	if (!offsets_ok(off, nc, who)) return NHW_E_ARG;
	if (to_device) for (int i = 0; i < nr; i++) if (!dst_addr[i] || dst_pitch[i] < 3ull * rects[i].width) { nhw_dec_err = std::string(who) + ": a destination needs an address and a pitch of at least 3 x width"; return NHW_E_ARG; }
	if (crop) for (int i = 0; i < nr; i++) if (!dst_addr[i] || dst_addr[i] % (crop->dtype == NHW_T_U8 ? 1u : crop->dtype == NHW_T_F32 ? 4u : 2u)) { nhw_dec_err = std::string(who) + ": a destination needs an address that is a multiple of the element size"; return NHW_E_ARG; }
	d->reg_tiles = d->reg_bytes = 0;
	const uint32_t T = 512u / (uint32_t)scale;
	const uint64_t limit = crop ? nhw_filter_limit(crop->filter) : 0;   /* the filter's reduction limit, 0 for none */
	std::vector<RegionSource> src((size_t)nc);
	std::vector<std::vector<int32_t>> slot_of((size_t)nc);        /* per container: a tile's (latest) slot, -1 while no window has selected it */
	std::vector<nhw_region> desc;
	std::vector<int> which;                                      /* desc[k] is rect which[k] */
	std::vector<nhw_window_use> uses;
	std::vector<uint64_t> toff;
	std::vector<uint32_t> tlen;
	std::vector<uint8_t> files;                                  /* the slots' tile files, slot after slot */
	const uint8_t *run = nullptr, *run_end = nullptr;            /* ... but for the latest slots' files, which lie back to back in their container: a row of a
	                                                              * selection goes in as one run (one append a tile measured a quarter more for the gather) */
	uint64_t bytes = 0;
	for (int i = 0; i < nr; i++) {
		const nhw_rect &r = rects[i];
		status[i] = NHW_E_ARG;
		if (!r.width || !r.height || r.container >= (uint32_t)nc) continue;
		if (limit && (r.width > limit * crop->out_w || r.height > limit * crop->out_h)) continue;
		if (crop && crop->warps && !nhw_warp_within(crop->warps[i])) continue;
		RegionSource &c = src[r.container];
		const uint8_t *base = blob + off[r.container];
		source_look(c, base, (size_t)(off[r.container + 1] - off[r.container]));
		if (c.state < 0) { status[i] = NHW_E_FORMAT; continue; }
		const int nt = nhw_window_tiles(c.w, c.h, scale, r.x, r.y, r.width, r.height);
		if (nt < 1) continue;
		if (uses.size() + (size_t)nt > MAX_CALL_TILES) { nhw_dec_err = std::string(who) + ": too many tiles in one call"; return NHW_E_ARG; }
		status[i] = NHW_OK;
		uint32_t sw = 0, sh = 0;
		nhw_picture_scaled_size(c.w, c.h, scale, &sw, &sh);           /* the table describes the destination */
		desc.push_back({ to_device ? dst_addr[i] : bytes, to_device ? dst_pitch[i] : 3ull * r.width, r.x, r.y, r.width, r.height, sw, sh, 0, 0 });
		which.push_back(i);
		bytes += 3ull * r.width * r.height;
		std::vector<int32_t> &slot = slot_of[r.container];
		if (slot.empty()) slot.assign((size_t)c.t, -1);
		const uint32_t nx = (c.w + 511) / 512;                        /* the grid does not change with the scale */
		for (uint32_t ty = r.y / T; ty <= (r.y + r.height - 1) / T; ty++)
			for (uint32_t tx = r.x / T; tx <= (r.x + r.width - 1) / T; tx++) {
				const uint32_t k = ty * nx + tx;
				if (!merge || slot[k] < 0) {
					slot[k] = (int32_t)toff.size();
					if (run_end != base + c.start[k]) {                     /* not the file behind the last one: the run so far goes in */
						files.insert(files.end(), run, run_end);
						run = base + c.start[k];
					}
					toff.push_back(files.size() + (uint64_t)(base + c.start[k] - run));
					tlen.push_back(dir_len(c.dir, (int)k));
					run_end = base + c.start[k + 1];
				}
				uses.push_back({ (uint32_t)desc.size() - 1, (uint32_t)slot[k], tx, ty });
			}
	}
	files.insert(files.end(), run, run_end);
	if (desc.empty()) return NHW_OK;
	const int tiles = (int)toff.size(), ng = (int)desc.size(), nu = (int)uses.size();
	std::vector<int> first_use((size_t)tiles + 1, 0);             /* sorted by slot (a counting sort): uses [first_use[t], first_use[t + 1]) are those of slot t */
	for (const nhw_window_use &u : uses) first_use[u.slot + 1]++;
	for (int t = 0; t < tiles; t++) first_use[t + 1] += first_use[t];
	{
		std::vector<nhw_window_use> sorted((size_t)nu);
		std::vector<int> at(first_use.begin(), first_use.end() - 1);
		for (const nhw_window_use &u : uses) sorted[(size_t)at[u.slot]++] = u;
		uses.swap(sorted);
	}
	HIPCHK(hipSetDevice(d->device));
	{ const int rc = host_buffers(d, files.size()); if (rc) return rc; }
	const size_t desc_bytes = (size_t)ng * sizeof(nhw_region);     /* (a multiple of 16: the use table behind it is aligned) */
	HIPCHK(nhw_grow(d->pic_desc, desc_bytes + (size_t)nu * sizeof(nhw_window_use)));
	if (!to_device) {
		HIPCHK(nhw_grow(d->pic_px, bytes));
		for (nhw_region &g : desc) g.addr += (uint64_t)(uintptr_t)d->pic_px.p;
	}
	const nhw_region *d_desc = d->pic_desc.as<nhw_region>();
	const nhw_window_use *d_uses = (const nhw_window_use *)(d->pic_desc.as<uint8_t>() + desc_bytes);
	hipStream_t s = d->own_stream;
	HIPCHK(hipMemcpyAsync(d->blob.p, files.data(), files.size(), hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync(d->pic_desc.p, desc.data(), desc_bytes, hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync((void *)d_uses, uses.data(), (size_t)nu * sizeof(nhw_window_use), hipMemcpyHostToDevice, s));
	d->reg_tiles = (uint64_t)tiles; d->reg_bytes = files.size();
	std::vector<int32_t> tst;
	{ const int rc = decode_tile_list(d, toff, tlen, scale, tst, [&](int t0, int m) {
		return nhw_launch_untile_window(d->d_out, d_desc, ng, d_uses + first_use[t0], first_use[t0 + m] - first_use[t0], t0, m, scale, s); }); if (rc) return rc; }
	for (const nhw_window_use &u : uses)
		if (tiles_status(tst, (int)u.slot, (int)u.slot + 1) != NHW_OK) status[which[u.region]] = NHW_E_FORMAT;
	if (crop) {                                                   /* one table entry a rect: a rect that has no window keeps a zero picture and a zero address */
		std::vector<nhw_picture> pics((size_t)nr, nhw_picture{ 0, 0, 0, 0, 0, 0 });
		std::vector<uint64_t> oaddr((size_t)nr, 0);
		for (int k = 0; k < ng; k++) {
			pics[(size_t)which[k]] = { desc[k].addr, desc[k].pitch, desc[k].width, desc[k].height, 0, 0 };
			if (status[which[k]] == NHW_OK) oaddr[(size_t)which[k]] = dst_addr[which[k]];
		}
		const size_t pics_bytes = (size_t)nr * sizeof(nhw_picture), addr_bytes = (size_t)nr * 8;
		HIPCHK(nhw_grow(d->crop_tab, pics_bytes + addr_bytes + (size_t)nr * (crop->warps ? sizeof(nhw_warp) : 1)));
		uint8_t *tab = d->crop_tab.as<uint8_t>();
		HIPCHK(hipMemcpyAsync(tab, pics.data(), pics_bytes, hipMemcpyHostToDevice, s));
		HIPCHK(hipMemcpyAsync(tab + pics_bytes, oaddr.data(), addr_bytes, hipMemcpyHostToDevice, s));
		if (crop->warps) {                                            /* (32 + 8 bytes an entry in front: the warps are 8-byte aligned) */
			HIPCHK(hipMemcpyAsync(tab + pics_bytes + addr_bytes, crop->warps, (size_t)nr * sizeof(nhw_warp), hipMemcpyHostToDevice, s));
			HIPCHK(nhw_launch_warp((const nhw_picture *)tab, (const nhw_warp *)(tab + pics_bytes + addr_bytes), nr, crop->out_w, crop->out_h, crop->dtype, crop->layout,
			                       crop->a, (const uint64_t *)(tab + pics_bytes), s));
			HIPCHK(hipStreamSynchronize(s));
			return NHW_OK;
		}
		if (crop->flags) HIPCHK(hipMemcpyAsync(tab + pics_bytes + addr_bytes, crop->flags, (size_t)nr, hipMemcpyHostToDevice, s));
		HIPCHK(nhw_launch_resample(crop->filter, (const nhw_picture *)tab, nr, crop->out_w, crop->out_h, crop->dtype, crop->layout, crop->a,
		                           crop->flags ? tab + pics_bytes + addr_bytes : nullptr, (const uint64_t *)(tab + pics_bytes), s));
		HIPCHK(hipStreamSynchronize(s));
		return NHW_OK;
	}
	return to_device ? NHW_OK : download_decoded(bgr, out_off, desc, which, status);
}

extern "C" int nhw_dec_regions(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects,
                               uint8_t *bgr, const uint64_t *out_off, int32_t *status)
{
	return dec_windows(d, blob, off, n_containers, rects, n_rects, 1, bgr, out_off, nullptr, nullptr, status, "nhw_dec_regions", false);
}

extern "C" int nhw_dec_regions_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects,
                                         const uint64_t *dst_addr, const uint64_t *dst_pitch, int32_t *status)
{
	if (!dst_addr) { nhw_dec_err = "bad argument"; return NHW_E_ARG; }
	return dec_windows(d, blob, off, n_containers, rects, n_rects, 1, nullptr, nullptr, dst_addr, dst_pitch, status, "nhw_dec_regions_to_device", false);
}

extern "C" int nhw_dec_windows(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                               uint8_t *bgr, const uint64_t *out_off, int32_t *status)
{
	return dec_windows(d, blob, off, n_containers, rects, n_rects, scale, bgr, out_off, nullptr, nullptr, status, "nhw_dec_windows");
}

extern "C" int nhw_dec_windows_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                         const uint64_t *dst_addr, const uint64_t *dst_pitch, int32_t *status)
{
	if (!dst_addr) { nhw_dec_err = "bad argument"; return NHW_E_ARG; }
	return dec_windows(d, blob, off, n_containers, rects, n_rects, scale, nullptr, nullptr, dst_addr, dst_pitch, status, "nhw_dec_windows_to_device");
}

/* nhw_dec_windows_to_device with a resize behind it (DESIGN.md sections 18 to 20): window i, resampled to out_width x out_height under `filter` and
 * mirrored where bit 0 of flags[i] is set, to the tensor at dst_addr[i].  The three entries are this body and differ in `accept`, the filters an
 * entry takes, a bit each: the two older ones take 0 and 1 (nhw_dec_crops_to_device_filter keeps refusing the cubic filter), the newest all
 * three.  A filter an entry does not take is refused in that entry's words and at that entry's place among the checks, which callers can tell
 * apart by the message they get for two mistakes at once: the newest entry looks at the filter first, the older ones at dst_addr and n_rects. */
constexpr unsigned CROPS_TWO = 1u << NHW_FILTER_TWO_TAP | 1u << NHW_FILTER_AREA, CROPS_ALL = CROPS_TWO | 1u << NHW_FILTER_CUBIC;
static int dec_crops(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale, uint32_t out_width,
                     uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr, int32_t *status, int filter, unsigned accept)
{
	const bool taken = filter >= NHW_FILTER_TWO_TAP && filter <= NHW_FILTER_CUBIC && (accept >> filter & 1), args = dst_addr && n_rects <= (1 << 24);
	if (!taken && (accept == CROPS_ALL || args)) {
		nhw_dec_err = accept == CROPS_ALL ? "nhw_dec_crops_to_device_resample: the filter must be NHW_FILTER_TWO_TAP, NHW_FILTER_AREA or NHW_FILTER_CUBIC"
		                                  : "nhw_dec_crops_to_device: the filter must be NHW_FILTER_TWO_TAP or NHW_FILTER_AREA";
		return NHW_E_ARG;
	}
	if (!args) { nhw_dec_err = "bad argument"; return NHW_E_ARG; }
	if (out_width < 1 || out_height < 1 || out_width > 4096u || out_height > 4096u) { nhw_dec_err = "nhw_dec_crops_to_device: an output side outside 1 .. 4096"; return NHW_E_ARG; }
	CropSpec c = { out_width, out_height, 0, 0, {}, flags, filter, nullptr };
	if (const int rc = nhw_tensor_format_check(fmt, &c.a, nhw_dec_err)) return rc;
	c.dtype = fmt->dtype; c.layout = fmt->layout;
	return dec_windows(d, blob, off, n_containers, rects, n_rects, scale, nullptr, nullptr, dst_addr, nullptr, status, "nhw_dec_crops_to_device", true, &c);
}

extern "C" int nhw_dec_crops_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                       uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr, int32_t *status)
{
	return dec_crops(d, blob, off, n_containers, rects, n_rects, scale, out_width, out_height, fmt, flags, dst_addr, status, NHW_FILTER_TWO_TAP, CROPS_TWO);
}

extern "C" int nhw_dec_crops_to_device_filter(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                              uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr, int32_t *status,
                                              int filter)
{
	return dec_crops(d, blob, off, n_containers, rects, n_rects, scale, out_width, out_height, fmt, flags, dst_addr, status, filter, CROPS_TWO);
}

extern "C" int nhw_dec_crops_to_device_resample(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                                uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr,
                                                int *status, int filter)
{
	static_assert(sizeof(int) == sizeof(int32_t), "the statuses are 32 bits wide");
	return dec_crops(d, blob, off, n_containers, rects, n_rects, scale, out_width, out_height, fmt, flags, dst_addr, (int32_t *)status, filter, CROPS_ALL);
}

/* the windows sampled along tilted grids: the crop call with a warp a rect in place of filter and flags */
extern "C" int nhw_dec_warps_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                       uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const nhw_warp *warps, const uint64_t *dst_addr,
                                       int32_t *status)
{
	static_assert(sizeof(nhw_warp) == 40 && sizeof(nhw_picture) == 32, "the crop table's layout");
	if (!warps || !dst_addr || n_rects > (1 << 24)) { nhw_dec_err = "bad argument"; return NHW_E_ARG; }
	if (out_width < 1 || out_height < 1 || out_width > 4096u || out_height > 4096u) { nhw_dec_err = "nhw_dec_warps_to_device: an output side outside 1 .. 4096"; return NHW_E_ARG; }
	CropSpec c = { out_width, out_height, 0, 0, {}, nullptr, NHW_FILTER_TWO_TAP, warps };
	if (const int rc = nhw_tensor_format_check(fmt, &c.a, nhw_dec_err)) return rc;
	c.dtype = fmt->dtype; c.layout = fmt->layout;
	return dec_windows(d, blob, off, n_containers, rects, n_rects, scale, nullptr, nullptr, dst_addr, nullptr, status, "nhw_dec_warps_to_device", true, &c);
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
