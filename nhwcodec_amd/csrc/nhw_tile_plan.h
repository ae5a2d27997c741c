/*
 * nhw_tile_plan.h -- which tile files a decode of .nhwp containers takes, worked out on the host before anything goes to the device
 * (DESIGN.md sections 13 and 15): for the region, window, crop and warp calls the union (or, for regions, the sum) of the tiles the rects
 * select, their files gathered into one blob, and the table of (rect, tile) uses; for nhw_dec_pictures every tile of every container over
 * the blob as it lies.  Arithmetic on host bytes without a HIP header: nhw_dec_hostpath.hip uploads and decodes what a plan says, and
 * tests/tile_plan/check.cpp holds the planners against a model on the CPU.
 */
#ifndef NHW_TILE_PLAN_H
#define NHW_TILE_PLAN_H

#include <string>
#include <vector>

#include "nhw_container.h"

/* a container as the planners see it: parsed once, at the first look; start[k] = byte offset of tile file k in it */
struct RegionSource {
	int state = 0;                                               /* 0 not looked at, 1 well-formed, -1 malformed */
	uint32_t w = 0, h = 0;
	int t = 0;
	const uint8_t *dir = nullptr;
	std::vector<uint64_t> start;                                 /* t + 1 entries */
};

inline void source_look(RegionSource &c, const uint8_t *base, size_t len)   /* the first look at a container */
{
	if (c.state != 0) return;
	c.state = nhw_container_parse(base, len, &c.w, &c.h, &c.t, &c.dir) == NHW_OK ? 1 : -1;
	if (c.state == 1) {
		c.start.resize((size_t)c.t + 1);
		c.start[0] = 16 + 4 * (uint64_t)c.t;
		for (int k = 0; k < c.t; k++) c.start[k + 1] = c.start[k] + dir_len(c.dir, k);
	}
}

/* ------------------------------------------------------------------------------------------------ regions and windows */
/* What a region or window call decodes and where it goes.  A tile the call decodes has a slot: its file is files[toff[slot] .. + tlen[slot]),
 * and it is decoded as tile `slot` of the call.  Every (rect, tile) pair is a use; the uses are sorted by slot, so the chunk [t0, t0 + m) of
 * decoded tiles owns the contiguous range [first_use[t0], first_use[t0 + m)) of them, which the crop launch behind the chunk takes. */
struct TilePlan {
	std::vector<nhw_region> desc;                                /* a rect that selects tiles: its destination (addr: see plan_windows) */
	std::vector<int> which;                                      /* desc[k] is rect which[k] */
	std::vector<nhw_window_use> uses;                            /* (index into desc, slot, tx, ty), sorted by slot; without merging that is the order they were made in */
	std::vector<int> first_use;                                  /* slots + 1 entries: uses [first_use[t], first_use[t + 1]) are those of slot t */
	std::vector<uint64_t> toff;
	std::vector<uint32_t> tlen;
	std::vector<uint8_t> files;                                  /* the slots' tile files, slot after slot */
	uint64_t bytes = 0;                                          /* px width height of every desc, summed: the packed pixels */
};

struct WindowsIn {
	const uint8_t *blob; const uint64_t *off; int nc;            /* container c is blob[off[c] .. off[c + 1]) */
	const nhw_rect *rects; int nr;
	int scale;
	bool merge;                                                  /* a tile gets one slot a call (windows); off: one every time a rect selects it (regions, section 13's contract) */
	const uint8_t *refused;                                      /* nr bytes or null: rect i is NHW_E_ARG without a look at its container where refused[i] is set */
	const uint64_t *dst_addr, *dst_pitch;                        /* both set: the descriptors' addresses and pitches; else running byte offsets and packed rows */
	const char *who;                                             /* the entry point, for the message */
	size_t max_tiles;                                            /* the uses one call takes */
	uint32_t px = 3;                                             /* bytes a pixel of the packed rows and of `bytes`: 3, or 1 for a grey call */
};

/* Fills `p` and every status[i]: NHW_E_ARG for a rect that is empty, names no container, is refused or does not lie in the scaled picture,
 * NHW_E_FORMAT for one whose container is malformed, else NHW_OK -- such a rect gets a descriptor, and each tile it selects a use and, when
 * the first rect selects it (without merging: every time), a slot.  Only the files of the slots are gathered, but for the latest slots'
 * files, which lie back to back in their container: [run, run_end) is appended when a slot's file is not the one behind it, so a row of a
 * selection goes in as one run (one append a tile measured a quarter more for the gather).  Returns NHW_OK, or NHW_E_ARG with the reason
 * in err when the uses exceed max_tiles; `p` then holds nothing that is meant to be used. */
inline int plan_windows(const WindowsIn &in, TilePlan &p, int32_t *status, std::string &err)
{
	const uint32_t T = 512u / (uint32_t)in.scale;
	const bool given = in.dst_addr && in.dst_pitch;
	std::vector<RegionSource> src((size_t)in.nc);
	std::vector<std::vector<int32_t>> slot_of((size_t)in.nc);     /* per container: a tile's (latest) slot, -1 while no rect has selected it */
	const uint8_t *run = nullptr, *run_end = nullptr;
	for (int i = 0; i < in.nr; i++) {
		const nhw_rect &r = in.rects[i];
		status[i] = NHW_E_ARG;
		if (!r.width || !r.height || r.container >= (uint32_t)in.nc) continue;
		if (in.refused && in.refused[i]) continue;
		RegionSource &c = src[r.container];
		const uint8_t *base = in.blob + in.off[r.container];
		source_look(c, base, (size_t)(in.off[r.container + 1] - in.off[r.container]));
		if (c.state < 0) { status[i] = NHW_E_FORMAT; continue; }
		const int nt = nhw_rule_window_tiles(c.w, c.h, in.scale, r.x, r.y, r.width, r.height);
		if (nt < 1) continue;
		if (p.uses.size() + (size_t)nt > in.max_tiles) { err = std::string(in.who) + ": too many tiles in one call"; return NHW_E_ARG; }
		status[i] = NHW_OK;
		uint32_t sw = 0, sh = 0;
		nhw_rule_picture_scaled_size(c.w, c.h, in.scale, &sw, &sh);   /* the table describes the destination */
		p.desc.push_back({ given ? in.dst_addr[i] : p.bytes, given ? in.dst_pitch[i] : (uint64_t)in.px * r.width, r.x, r.y, r.width, r.height, sw, sh, 0, 0 });
		p.which.push_back(i);
		p.bytes += (uint64_t)in.px * r.width * r.height;
		std::vector<int32_t> &slot = slot_of[r.container];
		if (slot.empty()) slot.assign((size_t)c.t, -1);
		const uint32_t nx = (c.w + 511) / 512;                        /* the grid does not change with the scale */
		for (uint32_t ty = r.y / T; ty <= (r.y + r.height - 1) / T; ty++)
			for (uint32_t tx = r.x / T; tx <= (r.x + r.width - 1) / T; tx++) {
				const uint32_t k = ty * nx + tx;
				if (!in.merge || slot[k] < 0) {
					slot[k] = (int32_t)p.toff.size();
					if (run_end != base + c.start[k]) {                     /* not the file behind the last one: the run so far goes in */
						p.files.insert(p.files.end(), run, run_end);
						run = base + c.start[k];
					}
					p.toff.push_back(p.files.size() + (uint64_t)(base + c.start[k] - run));
					p.tlen.push_back(dir_len(c.dir, (int)k));
					run_end = base + c.start[k + 1];
				}
				p.uses.push_back({ (uint32_t)p.desc.size() - 1, (uint32_t)slot[k], tx, ty });
			}
	}
	p.files.insert(p.files.end(), run, run_end);
	const size_t tiles = p.toff.size();
	p.first_use.assign(tiles + 1, 0);                             /* a counting sort by slot */
	for (const nhw_window_use &u : p.uses) p.first_use[u.slot + 1]++;
	for (size_t t = 0; t < tiles; t++) p.first_use[t + 1] += p.first_use[t];
	std::vector<nhw_window_use> sorted(p.uses.size());
	std::vector<int> at(p.first_use.begin(), p.first_use.end() - 1);
	for (const nhw_window_use &u : p.uses) sorted[(size_t)at[u.slot]++] = u;
	p.uses.swap(sorted);
	return NHW_OK;
}

/* ------------------------------------------------------------------------------------------------ whole pictures */
/* nhw_dec_pictures' plan: every tile of every well-formed container, over the blob as it lies from off[0] on -- a container's tile files lie
 * back to back, so the offsets and lengths come from its directory.  The table describes the destinations, packed one behind the other. */
struct PicturePlan {
	std::vector<nhw_picture> desc;                               /* addr: a running byte offset */
	std::vector<int> which;                                      /* desc[k] is container which[k] */
	std::vector<uint64_t> toff;                                  /* relative to off[0] */
	std::vector<uint32_t> tlen;
	uint64_t bytes = 0;
};

/* status[i] = NHW_E_FORMAT for a malformed container, which is passed over, else NHW_OK; NHW_E_ARG with the reason in err when the tiles
 * exceed max_tiles */
inline int plan_pictures(const uint8_t *blob, const uint64_t *off, int n, int scale, size_t max_tiles, PicturePlan &p, int32_t *status, std::string &err)
{
	RegionSource c;
	for (int i = 0; i < n; i++) {
		status[i] = NHW_E_FORMAT;
		c.state = 0;
		source_look(c, blob + off[i], (size_t)(off[i + 1] - off[i]));
		if (c.state < 0) continue;
		if (p.toff.size() + (size_t)c.t > max_tiles) { err = "nhw_dec_pictures: too many tiles in one call"; return NHW_E_ARG; }
		status[i] = NHW_OK;
		uint32_t w = 0, h = 0;
		nhw_rule_picture_scaled_size(c.w, c.h, scale, &w, &h);        /* the table describes the destination; the tile count is that of the whole picture */
		p.desc.push_back({ p.bytes, 3ull * w, w, h, (uint32_t)p.toff.size(), 0 });
		p.which.push_back(i);
		for (int k = 0; k < c.t; k++) { p.toff.push_back(off[i] - off[0] + c.start[k]); p.tlen.push_back((uint32_t)(c.start[k + 1] - c.start[k])); }
		p.bytes += 3ull * w * h;
	}
	return NHW_OK;
}

#endif
