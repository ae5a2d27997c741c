/*
 * nhw_container.h -- the .nhwp container and the geometry of its tiles on the host (DESIGN.md sections 11 to 15, 18): how many tiles a picture
 * has, its size at a scale, the tiles a region or a window selects, the scale a crop is decoded at, and the parser and writer of the header
 * and directory in front of the tile files.  Plain C++ without a HIP header: the library compiles it (the exports of nhw_picture.hip are one
 * call each into it, the host paths use it directly) and tests/tile_plan/check.cpp compiles it with the host compiler.
 */
#ifndef NHW_CONTAINER_H
#define NHW_CONTAINER_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nhw_hip.h"

inline uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline void wr32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

/* ------------------------------------------------------------------------------------------------ the rules behind the exports of the same names */
inline int nhw_rule_picture_tiles(uint32_t width, uint32_t height)
{
	if (width < 1 || width > 65535 || height < 1 || height > 65535) return NHW_E_ARG;
	return (int)(((width + 511) / 512) * ((height + 511) / 512));
}

/* a W x H picture decoded at scale s is ceil(W / s) x ceil(H / s); its tile count does not change */
inline int nhw_rule_picture_scaled_size(uint32_t width, uint32_t height, int scale, uint32_t *scaled_width, uint32_t *scaled_height)
{
	if (nhw_rule_picture_tiles(width, height) < 1 || (scale != 1 && scale != 2 && scale != 4) || !scaled_width || !scaled_height) return NHW_E_ARG;
	*scaled_width = (width + (uint32_t)scale - 1) / (uint32_t)scale;
	*scaled_height = (height + (uint32_t)scale - 1) / (uint32_t)scale;
	return NHW_OK;
}

/* the tiles a region x, y, w, h of a W x H picture selects: columns x / 512 .. (x + w - 1) / 512 times rows y / 512 .. (y + h - 1) / 512 */
inline int nhw_rule_region_tiles(uint32_t pic_width, uint32_t pic_height, uint32_t x, uint32_t y, uint32_t width, uint32_t height)
{
	if (nhw_rule_picture_tiles(pic_width, pic_height) < 1 || width < 1 || height < 1) return NHW_E_ARG;
	if ((uint64_t)x + width > pic_width || (uint64_t)y + height > pic_height) return NHW_E_ARG;
	return (int)(((x + width - 1) / 512 - x / 512 + 1) * ((y + height - 1) / 512 - y / 512 + 1));
}

/* the tiles a window x, y, w, h of the picture at scale s selects: the rectangle is in the coordinates of the scaled
 * picture ceil(W / s) x ceil(H / s), whose tiles have the side T = 512 / s; at scale 1 it is nhw_rule_region_tiles */
inline int nhw_rule_window_tiles(uint32_t pic_width, uint32_t pic_height, int scale, uint32_t x, uint32_t y, uint32_t width, uint32_t height)
{
	uint32_t sw = 0, sh = 0;
	if (nhw_rule_picture_scaled_size(pic_width, pic_height, scale, &sw, &sh) != NHW_OK || width < 1 || height < 1) return NHW_E_ARG;
	if ((uint64_t)x + width > sw || (uint64_t)y + height > sh) return NHW_E_ARG;
	const uint32_t T = 512u / (uint32_t)scale;
	return (int)(((x + width - 1) / T - x / T + 1) * ((y + height - 1) / T - y / T + 1));
}

/* the scale to decode a width x height crop at that goes to out_width x out_height: the largest s of 4, 2, 1 with
 * s out_width <= width and s out_height <= height, so that what is left to the two-tap resize is a reduction below 2; 1 if there is none */
inline int nhw_rule_crop_scale(uint32_t width, uint32_t height, uint32_t out_width, uint32_t out_height)
{
	if (!width || !height || !out_width || !out_height || out_width > 4096u || out_height > 4096u) return NHW_E_ARG;
	for (uint32_t s = 4; s > 1; s >>= 1)
		if (s * out_width <= width && s * out_height <= height) return (int)s;
	return 1;
}

/* ------------------------------------------------------------------------------------------------ the container */
/* A well-formed container: magic, version 1, zero reserved bytes, W and H in 1..65535, T = nhw_picture_tiles(W, H) lengths of 1 ..
 * NHW_OUT_STRIDE each, and exactly 16 + 4 T + the sum of them bytes.  Returns NHW_OK with W, H, T and a pointer to the directory. */
inline int nhw_container_parse(const uint8_t *c, size_t len, uint32_t *width, uint32_t *height, int *tiles, const uint8_t **dir)
{
	if (!c || len < 16 || memcmp(c, "NHWP", 4) || c[4] != 1 || c[5] || c[6] || c[7]) return NHW_E_FORMAT;
	const uint32_t w = rd32(c + 8), h = rd32(c + 12);
	const int t = nhw_rule_picture_tiles(w, h);
	if (t < 1 || (len - 16) / 4 < (size_t)t) return NHW_E_FORMAT;
	uint64_t total = 16 + 4 * (uint64_t)t;
	for (int i = 0; i < t; i++) {
		const uint32_t l = rd32(c + 16 + 4 * (size_t)i);
		if (l < 1 || l > NHW_OUT_STRIDE) return NHW_E_FORMAT;
		total += l;
	}
	if (total != len) return NHW_E_FORMAT;
	*width = w; *height = h; *tiles = t; *dir = c + 16;
	return NHW_OK;
}

inline uint32_t dir_len(const uint8_t *dir, int k) { return rd32(dir + 4 * (size_t)k); }   /* length of tile file k in a container's directory */

/* what nhw_picture_info says of a container: its status and, where asked for, the picture's size */
inline int nhw_container_info(const uint8_t *c, size_t len, uint32_t *width, uint32_t *height)
{
	uint32_t w = 0, h = 0;
	int t = 0;
	const uint8_t *dir = nullptr;
	const int rc = nhw_container_parse(c, len, &w, &h, &t, &dir);
	if (rc != NHW_OK) return rc;
	if (width) *width = w;
	if (height) *height = h;
	return NHW_OK;
}

/* header and directory of a container for a W x H picture whose T tile files have the lengths lens[]; returns 16 + 4 T (the files go
 * behind, back to back) */
inline size_t nhw_container_head(uint8_t *dst, uint32_t width, uint32_t height, const uint32_t *lens, int t)
{
	memcpy(dst, "NHWP\1\0\0\0", 8);
	wr32(dst + 8, width); wr32(dst + 12, height);
	for (int i = 0; i < t; i++) wr32(dst + 16 + 4 * (size_t)i, lens[i]);
	return 16 + 4 * (size_t)t;
}

#endif
