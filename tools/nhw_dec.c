/*
 * nhw-dec -- command-line decoder over libnhwhip.so (include/nhw_hip.h).
 *
 * Same interface as the reference CLI (rcanut/nhwcodec decoder/nhw_decoder_cli.c:70-118):
 *     nhw-dec image.nhw image.bmp          (with fewer arguments: the usage text, exit 0)
 * The BMP is the 54-byte header of decoder/nhw_decoder_cli.c:61-65,293-312 followed by the pixel bytes in the order
 * write_image_bmp (:108-291) writes them.  Exit codes: 0 ok, 1 cannot read / write a file (the reference prints and
 * carries on into undefined behaviour), 3 not an .nhw file (reference: "Not an .nhw file", exit(-1)).
 * Extension: --batch <dir> decodes every *.nhw of a directory to <name>.bmp in one GPU batch; --picture <in.nhwp> <out.bmp> decodes a
 * container of nhw-enc --picture to a bottom-up 24-bit BMP of the picture's own size; with --region X,Y,W,H behind it, only that rectangle
 * (X, Y from the left and the top of the picture as a viewer shows it), decoded from the tiles it touches.  --scale 2|4 (1: the same as
 * without it), anywhere on the line of a single file, --batch or --picture: the half- or quarter-scale picture straight from the wavelet
 * pyramid, under a header that carries the scaled size.  --window S,X,Y,W,H behind --picture <in> <out>: that rectangle
 * of the picture at scale S (1, 2 or 4), in the coordinates of the scaled picture, from the tiles it touches.
 * --grey <in.nhw> <out.pgm>, with or without --scale: the luma alone through the grey table of the file's quality, as a
 * binary PGM (P5) with its rows top-down; not with --batch, --tar, --tiles or --picture.
 */
#include <dirent.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/nhw_hip.h"

#define PROGRAM "nhw-dec"

static void show_usage(void)
{
	fprintf(stdout,
	"Usage: %s <image.nhw> <image.bmp>\n"
	"Convert image: nwh to bmp\n"
	" (with a bitmap color 512x512 image)\n"
	"\n"
	"  example: nhw-dec image.nhw image.bmp\n"
	"  batch:   nhw-dec --batch <directory of .nhw files>\n"
	"  tiles:   nhw-dec --tiles <rows> <columns> <stem> <image.bmp>   (joins <stem>_y<r>_x<c>.nhw, as written by nhw-enc --tiles)\n"
	"  tar:     nhw-dec --tar <in.tar> <out.tar>   (every x.nhw member of a ustar archive -> member x.bmp, in order)\n"
	"  picture: nhw-dec --picture <in.nhwp> <image.bmp>   (a container of nhw-enc --picture, any size)\n"
	"  region:  nhw-dec --picture <in.nhwp> <image.bmp> --region X,Y,W,H   (that rectangle only, X,Y from the top left; decodes the tiles it touches)\n"
	"  window:  nhw-dec --picture <in.nhwp> <image.bmp> --window S,X,Y,W,H   (that rectangle of the picture at scale S = 1, 2 or 4, X,Y from the top left of the scaled picture)\n"
	"  scale:   --scale 1|2|4 with a single file, --batch or --picture   (2, 4: the half- or quarter-scale picture, without the full reconstruction)\n",
	PROGRAM);
}

static int read_file(const char *path, uint8_t **buf, size_t *len)
{
	FILE *f = fopen(path, "rb");
	long n;
	if (!f) { printf("\nCould not open file\n"); return 1; }
	fseek(f, 0, SEEK_END); n = ftell(f); fseek(f, 0, SEEK_SET);
	*buf = (uint8_t *)malloc((size_t)n + 1);
	if (!*buf || fread(*buf, 1, (size_t)n, f) != (size_t)n) { fclose(f); return 1; }
	fclose(f);
	*len = (size_t)n;
	return 0;
}

static int g_scale = 1;                                               /* --scale */
static int g_grey = 0;                                                /* --grey */

/* the reference's 54 bytes with the size fields of a width x height picture of `bytes` pixel bytes (rows padded to 4) */
static void bmp_header_sized(uint8_t hdr[54], uint32_t width, uint32_t height, uint32_t bytes)
{
	nhw_dec_bmp_header(hdr);
	hdr[2] = (uint8_t)(bytes + 54); hdr[3] = (uint8_t)((bytes + 54) >> 8); hdr[4] = (uint8_t)((bytes + 54) >> 16); hdr[5] = (uint8_t)((bytes + 54) >> 24);
	hdr[18] = (uint8_t)width; hdr[19] = (uint8_t)(width >> 8); hdr[20] = (uint8_t)(width >> 16); hdr[21] = (uint8_t)(width >> 24);
	hdr[22] = (uint8_t)height; hdr[23] = (uint8_t)(height >> 8); hdr[24] = (uint8_t)(height >> 16); hdr[25] = (uint8_t)(height >> 24);
	hdr[34] = (uint8_t)bytes; hdr[35] = (uint8_t)(bytes >> 8); hdr[36] = (uint8_t)(bytes >> 16); hdr[37] = (uint8_t)(bytes >> 24);
}

static int write_bmp(const char *path, const uint8_t *pixels)
{
	uint8_t hdr[54];
	const uint32_t side = 512u / (uint32_t)g_scale;
	FILE *f = fopen(path, "wb");
	if (!f) { printf("Failed to open output decompressed .bmp file %s\n", path); return 1; }
	if (g_scale == 1) nhw_dec_bmp_header(hdr);
	else bmp_header_sized(hdr, side, side, 3u * side * side);
	fwrite(hdr, 54, 1, f);
	fwrite(pixels, (size_t)3 * side * side, 1, f);
	fclose(f);
	return 0;
}

/* --grey: "P5", the side twice, 255, then the rows top-down: the byte path's row 0 is the picture's bottom row, so PGM row r is row side - 1 - r */
static int write_pgm(const char *path, const uint8_t *grey)
{
	const uint32_t side = 512u / (uint32_t)g_scale;
	uint32_t r;
	FILE *f = fopen(path, "wb");
	if (!f) { printf("Failed to open output decompressed .pgm file %s\n", path); return 1; }
	fprintf(f, "P5\n%u %u\n255\n", (unsigned)side, (unsigned)side);
	for (r = 0; r < side; r++) fwrite(grey + (size_t)(side - 1 - r) * side, side, 1, f);
	fclose(f);
	return 0;
}

static int decode_files(char **in, char **out, int n)
{
	nhw_dec *d = NULL;
	uint8_t *blob = NULL, *pix;
	uint64_t *off = (uint64_t *)calloc((size_t)n + 1, sizeof *off);
	int32_t *status = (int32_t *)calloc((size_t)n, sizeof *status);
	size_t total = 0;
	int i, rc = 0;
	for (i = 0; i < n; i++) {
		uint8_t *b; size_t len;
		if (read_file(in[i], &b, &len)) return 1;
		blob = (uint8_t *)realloc(blob, total + len + 16);
		memcpy(blob + total, b, len); free(b);
		off[i] = total; total += len;
	}
	off[n] = total;
	pix = (uint8_t *)malloc((size_t)n * NHW_IMG_BYTES);
	if (nhw_dec_create(0, n, &d) ||
	    (g_grey ? nhw_dec_batch_grey(d, blob, off, n, g_scale, pix, status, NULL) :
	     g_scale == 1 ? nhw_dec_batch(d, blob, off, n, pix, status, NULL) : nhw_dec_batch_scaled(d, blob, off, n, g_scale, pix, status, NULL))) {
		fprintf(stderr, "%s: GPU decoder unavailable: %s\n", PROGRAM, nhw_dec_last_error());
		return 2;
	}
	for (i = 0; i < n; i++) {
		if (status[i]) { printf("\nNot an .nhw file"); if (n > 1) printf(": %s", in[i]); printf("\n"); rc = 3; continue; }
		if (g_grey ? write_pgm(out[i], pix + (size_t)i * (NHW_IMG_BYTES / 3 / (size_t)(g_scale * g_scale)))
		           : write_bmp(out[i], pix + (size_t)i * (NHW_IMG_BYTES / (size_t)(g_scale * g_scale)))) rc = rc ? rc : 1;
	}
	nhw_dec_destroy(d);
	free(blob); free(pix); free(off); free(status);
	return rc;
}

/* --tiles: the inverse of nhw-enc --tiles.  Every tile is a file of its own and decodes on its own; the tiles are put side by side in file
 * row order under one bottom-up BMP header of the whole size. */
static int decode_tiles(int ny, int nx, const char *stem, const char *out_path)
{
	const int n = ny * nx;
	nhw_dec *d = NULL;
	uint8_t *blob = NULL, *pix, hdr[54];
	uint64_t *off = (uint64_t *)calloc((size_t)n + 1, sizeof *off);
	int32_t *status = (int32_t *)calloc((size_t)n, sizeof *status);
	size_t total = 0;
	const uint32_t width = 512u * (uint32_t)nx, height = 512u * (uint32_t)ny, bytes = width * height * 3u;
	FILE *f;
	int t, r;
	if ((uint64_t)width * height * 3u + 54u > 0xFFFFFFFFull) {       /* the BMP header's 32-bit size fields */
		fprintf(stderr, "%s: a %d x %d grid of tiles does not fit a BMP file (4 GiB)\n", PROGRAM, ny, nx);
		return 1;
	}
	for (t = 0; t < n; t++) {
		char name[4096];
		uint8_t *b; size_t len;
		snprintf(name, sizeof name, "%s_y%d_x%d.nhw", stem, t / nx, t % nx);
		if (read_file(name, &b, &len)) return 1;
		{ uint8_t *grown = (uint8_t *)realloc(blob, total + len + 16);
		  if (!grown) { fprintf(stderr, "%s: out of memory\n", PROGRAM); return 1; }
		  blob = grown; }
		memcpy(blob + total, b, len); free(b);
		off[t] = total; total += len;
	}
	off[n] = total;
	pix = (uint8_t *)malloc((size_t)n * NHW_IMG_BYTES);
	if (nhw_dec_create(0, n, &d) || nhw_dec_batch(d, blob, off, n, pix, status, NULL)) {
		fprintf(stderr, "%s: GPU decoder unavailable: %s\n", PROGRAM, nhw_dec_last_error());
		return 2;
	}
	for (t = 0; t < n; t++) if (status[t]) { printf("\nNot an .nhw file: %s_y%d_x%d.nhw\n", stem, t / nx, t % nx); return 3; }
	bmp_header_sized(hdr, width, height, bytes);                      /* the reference's 54 bytes, with the size fields of the whole picture */
	f = fopen(out_path, "wb");
	if (!f) { printf("Failed to open output decompressed .bmp file %s\n", out_path); return 1; }
	fwrite(hdr, 54, 1, f);
	for (r = 0; r < (int)height; r++)
		for (t = 0; t < nx; t++)
			fwrite(pix + ((size_t)(r / 512) * nx + t) * NHW_IMG_BYTES + (size_t)(r % 512) * 1536, 1536, 1, f);
	fclose(f);
	nhw_dec_destroy(d);
	free(blob); free(pix); free(off); free(status);
	printf("%d x %d tiles\n", ny, nx);
	return 0;
}

/* n decimal numbers with commas between them, nothing else; 0 if the argument is that */
static int parse_numbers(const char *arg, uint32_t *out, int n)
{
	int i;
	for (i = 0; i < n; i++) {
		unsigned long v = 0;
		int digits = 0;
		for (; *arg >= '0' && *arg <= '9'; arg++, digits++) { v = v * 10 + (unsigned long)(*arg - '0'); if (v > 0xFFFFFFFFul) return 1; }
		if (!digits || *arg != (i < n - 1 ? ',' : '\0')) return 1;
		arg++;
		out[i] = (uint32_t)v;
	}
	return 0;
}

/* --region X,Y,W,H: four decimal numbers, nothing else; 0 if the argument is one */
static int parse_region(const char *arg, uint32_t reg[4]) { return parse_numbers(arg, reg, 4); }

/* --window S,X,Y,W,H: five decimal numbers, nothing else, S = 1, 2 or 4; 0 if the argument is one */
static int parse_window(const char *arg, uint32_t win[5])
{
	return parse_numbers(arg, win, 5) || (win[0] != 1 && win[0] != 2 && win[0] != 4);
}

/* --picture: the inverse of nhw-enc --picture.  The container's tiles are decoded and cropped by the library (nhw_dec_pictures); the
 * rows go out under the reference's 54-byte header with the size fields of the picture, each padded to 4 bytes.  With a region (X, Y from
 * the top left as a viewer shows the BMP, W, H; NULL: the whole picture) only the tiles it touches are decoded (nhw_dec_regions): the files
 * are bottom-up, so it is the library's rows H - Y - Hr .. H - Y - 1, and the BMP is that rectangle of the whole picture's BMP.  With a
 * window (S, X, Y, W, H; NULL: none) the same of the picture at scale S, in the scaled picture's coordinates (nhw_dec_windows). */
static int decode_picture(const char *in_path, const char *out_path, const uint32_t *region, const uint32_t *window)
{
	uint8_t *blob = NULL, *pix, hdr[54], pad[3] = { 0, 0, 0 };
	size_t len = 0;
	uint32_t width = 0, height = 0, row, stride, bytes, r;
	uint64_t off[2], out_off[1] = { 0 };
	int32_t status = 0;
	nhw_dec *d = NULL;
	nhw_rect rect;
	int t;
	FILE *f;
	if (read_file(in_path, &blob, &len)) return 1;
	if (nhw_picture_info(blob, len, &width, &height) != NHW_OK) { printf("\nNot an .nhwp file\n"); free(blob); return 3; }
	if (window) {
		uint32_t sw = 0, sh = 0;
		t = NHW_E_ARG;
		nhw_picture_scaled_size(width, height, (int)window[0], &sw, &sh);
		if (window[4] >= 1 && (uint64_t)window[2] + window[4] <= sh) {
			rect.container = 0; rect.x = window[1]; rect.y = sh - window[2] - window[4]; rect.width = window[3]; rect.height = window[4];
			t = nhw_window_tiles(width, height, (int)window[0], rect.x, rect.y, rect.width, rect.height);
		}
		if (t < 1) {
			fprintf(stderr, "%s: --window %u,%u,%u,%u,%u is empty or not inside the %u x %u picture (%u x %u at scale %u)\n", PROGRAM, (unsigned)window[0],
			        (unsigned)window[1], (unsigned)window[2], (unsigned)window[3], (unsigned)window[4], (unsigned)sw, (unsigned)sh, (unsigned)width,
			        (unsigned)height, (unsigned)window[0]);
			free(blob);
			return 1;
		}
		width = rect.width; height = rect.height;
	}
	else if (region) {
		t = NHW_E_ARG;
		if (region[3] >= 1 && (uint64_t)region[1] + region[3] <= height) {
			rect.container = 0; rect.x = region[0]; rect.y = height - region[1] - region[3]; rect.width = region[2]; rect.height = region[3];
			t = nhw_region_tiles(width, height, rect.x, rect.y, rect.width, rect.height);
		}
		if (t < 1) {
			fprintf(stderr, "%s: --region %u,%u,%u,%u is empty or not inside the %u x %u picture\n", PROGRAM, (unsigned)region[0], (unsigned)region[1],
			        (unsigned)region[2], (unsigned)region[3], (unsigned)width, (unsigned)height);
			free(blob);
			return 1;
		}
		width = rect.width; height = rect.height;
	}
	else {
		t = nhw_picture_tiles(width, height);
		if (g_scale != 1) nhw_picture_scaled_size(width, height, g_scale, &width, &height);   /* the tile count stays; the BMP has the scaled size */
	}
	row = width * 3; stride = (row + 3) & ~3u;
	if ((uint64_t)stride * height + 54u > 0xFFFFFFFFull) {           /* the BMP header's 32-bit size fields */
		fprintf(stderr, "%s: a %u x %u picture does not fit a BMP file (4 GiB)\n", PROGRAM, (unsigned)width, (unsigned)height);
		free(blob);
		return 1;
	}
	bytes = stride * height;
	pix = (uint8_t *)malloc((size_t)row * height);
	off[0] = 0; off[1] = len;
	if (!pix || nhw_dec_create(0, t < 1024 ? t : 1024, &d) ||
	    (window ? nhw_dec_windows(d, blob, off, 1, &rect, 1, (int)window[0], pix, out_off, &status) :
	     region ? nhw_dec_regions(d, blob, off, 1, &rect, 1, pix, out_off, &status) :
	     g_scale != 1 ? nhw_dec_pictures_scaled(d, blob, off, 1, g_scale, pix, out_off, &status) : nhw_dec_pictures(d, blob, off, 1, pix, out_off, &status))) {
		fprintf(stderr, "%s: GPU decoder unavailable: %s\n", PROGRAM, nhw_dec_last_error());
		return 2;
	}
	nhw_dec_destroy(d);
	free(blob);
	if (status) { printf("\nNot an .nhwp file\n"); free(pix); return 3; }
	bmp_header_sized(hdr, width, height, bytes);                      /* the reference's 54 bytes, with the size fields of the picture */
	f = fopen(out_path, "wb");
	if (!f) { printf("Failed to open output decompressed .bmp file %s\n", out_path); free(pix); return 1; }
	fwrite(hdr, 54, 1, f);
	for (r = 0; r < height; r++) {
		fwrite(pix + (size_t)r * row, 1, row, f);
		fwrite(pad, 1, stride - row, f);
	}
	fclose(f);
	free(pix);
	printf(window ? "%u x %u window\n" : region ? "%u x %u region\n" : "%u x %u picture\n", (unsigned)width, (unsigned)height);
	return 0;
}

/* --tar: the inverse of nhw-enc --tar; members are decoded in batches of up to 1024 */
static unsigned long tar_octal(const uint8_t *p, int n) { unsigned long v = 0; int i; for (i = 0; i < n && p[i] >= '0' && p[i] <= '7'; i++) v = v * 8 + (unsigned long)(p[i] - '0'); return v; }
static int tar_write_member(FILE *f, const char *name, const uint8_t *head, size_t head_len, const uint8_t *data, size_t len)
{
	uint8_t h[512];
	unsigned sum = 0;
	const size_t total = head_len + len, pad = (512 - total % 512) % 512;
	size_t i;
	static const uint8_t zeros[512];
	memset(h, 0, sizeof h);
	if (strlen(name) > 99) return -1;
	strcpy((char *)h, name);
	memcpy(h + 100, "0000644", 8); memcpy(h + 108, "0000000", 8); memcpy(h + 116, "0000000", 8);
	snprintf((char *)h + 124, 12, "%011lo", (unsigned long)total);
	memcpy(h + 136, "00000000000", 12);
	memset(h + 148, ' ', 8);
	h[156] = '0';
	memcpy(h + 257, "ustar", 6); memcpy(h + 263, "00", 2);
	for (i = 0; i < 512; i++) sum += h[i];
	snprintf((char *)h + 148, 8, "%06o", sum); h[155] = ' ';
	return (fwrite(h, 1, 512, f) == 512 && fwrite(head, 1, head_len, f) == head_len && fwrite(data, 1, len, f) == len && fwrite(zeros, 1, pad, f) == pad) ? 0 : -1;
}
#define TAR_NHW_MAX (1u << 20)      /* largest archive member taken for a .nhw file */
/* skip n bytes of the archive: by seeking, or by reading where the input cannot seek (a pipe); non-zero at the end of the input */
static int tar_skip(FILE *in, unsigned long n)
{
	uint8_t sink[4096];
	if (n == 0) return 0;
	if (fseek(in, (long)n, SEEK_CUR) == 0) return 0;
	while (n) { const size_t k = n < sizeof sink ? (size_t)n : sizeof sink; if (fread(sink, 1, k, in) != k) return 1; n -= (unsigned long)k; }
	return 0;
}
static int decode_tar(const char *in_path, const char *out_path)
{
	enum { CH = 1024 };
	FILE *in = fopen(in_path, "rb"), *out;
	nhw_dec *d = NULL;
	uint8_t hdr[512], bmp[54], *blob = NULL, *pix;
	size_t blob_cap = 0, total_bytes = 0;
	uint64_t *off = (uint64_t *)calloc(CH + 1, sizeof *off);
	int32_t *status = (int32_t *)calloc(CH, sizeof *status);
	char (*names)[104] = (char (*)[104])malloc((size_t)CH * 104);
	int n = 0, total = 0, bad = 0, eof = 0, i;
	static const uint8_t zeros[1024];
	if (!in) { printf("\nCould not open file\n"); return 1; }
	out = fopen(out_path, "wb");
	if (!out) { printf("Failed to open output decompressed .bmp file %s\n", out_path); return 1; }
	pix = (uint8_t *)malloc((size_t)CH * NHW_IMG_BYTES);
	nhw_dec_bmp_header(bmp);
	while (!eof) {
		if (fread(hdr, 1, 512, in) != 512 || hdr[0] == 0) eof = 1;
		else {
			const unsigned long size = tar_octal(hdr + 124, 12);
			size_t nl;
			hdr[99] = 0;
			nl = strlen((const char *)hdr);
			if ((hdr[156] == '0' || hdr[156] == 0) && nl > 4 && !strcmp((const char *)hdr + nl - 4, ".nhw")) {
				if (size > TAR_NHW_MAX) {                          /* the encoder never writes more than 512 KiB a file */
					fprintf(stderr, "%s: %s: member of %lu bytes is no .nhw file, left out\n", PROGRAM, (const char *)hdr, size); bad++;
					if (tar_skip(in, (size + 511) / 512 * 512)) eof = 1;
				}
				else {
				if (total_bytes + size + 16 > blob_cap) {
					uint8_t *grown = (uint8_t *)realloc(blob, (total_bytes + size + 16) * 2);
					if (!grown) { fprintf(stderr, "%s: out of memory\n", PROGRAM); return 1; }
					blob = grown; blob_cap = (total_bytes + size + 16) * 2;
				}
				if (fread(blob + total_bytes, 1, size, in) != size) { fprintf(stderr, "%s: %s: archive ends inside member %s\n", PROGRAM, in_path, (const char *)hdr); bad++; eof = 1; }
				else { off[n] = total_bytes; total_bytes += size; snprintf(names[n], 104, "%.*s.bmp", (int)(nl - 4), (const char *)hdr); n++; }
				if (size % 512 && tar_skip(in, 512 - size % 512)) eof = 1;
				}
			}
			else if (tar_skip(in, (size + 511) / 512 * 512)) eof = 1;
		}
		if (n == CH || (eof && n > 0)) {
			off[n] = total_bytes;
			if ((!d && nhw_dec_create(0, CH, &d)) || nhw_dec_batch(d, blob, off, n, pix, status, NULL)) {
				fprintf(stderr, "%s: GPU decoder unavailable: %s\n", PROGRAM, nhw_dec_last_error());
				return 2;
			}
			for (i = 0; i < n; i++) {
				if (status[i]) { printf("\nNot an .nhw file: %s\n", names[i]); bad++; continue; }
				if (tar_write_member(out, names[i], bmp, 54, pix + (size_t)i * NHW_IMG_BYTES, NHW_IMG_BYTES)) { bad++; break; }
			}
			total += n; n = 0; total_bytes = 0;
		}
	}
	fwrite(zeros, 1, 1024, out);
	fclose(out); fclose(in);
	if (d) nhw_dec_destroy(d);
	printf("%d file(s) decoded\n", total);
	free(blob); free(pix); free(off); free(status); free(names);
	return bad ? 3 : 0;
}

int main(int argc, char **argv)
{
	int a;
	for (a = 1; a < argc; a++)                                        /* --grey: with a single file only (and --scale); checked before any file is touched, then taken off the line */
		if (!strncmp(argv[a], "--grey", 6)) {
			int b;
			if (strcmp(argv[a], "--grey")) { fprintf(stderr, "%s: --grey takes no value: --grey <in.nhw> <out.pgm>\n", PROGRAM); return 1; }
			for (b = 1; b < argc; b++)
				if (!strcmp(argv[b], "--batch") || !strcmp(argv[b], "--tar") || !strcmp(argv[b], "--tiles") || !strcmp(argv[b], "--picture") ||
				    !strncmp(argv[b], "--region", 8) || !strncmp(argv[b], "--window", 8)) {
					fprintf(stderr, "%s: --grey goes with a single file (and --scale): not with %s\n", PROGRAM, argv[b]);
					return 1;
				}
			g_grey = 1;
			for (b = a; b + 1 < argc; b++) argv[b] = argv[b + 1];
			argc -= 1;
			break;
		}
	for (a = 1; a < argc; a++)                                        /* --window: behind --picture <in> <out> only, without --scale or --region; checked before any file is touched */
		if (!strncmp(argv[a], "--window", 8)) {
			uint32_t win[5];
			int b;
			for (b = 1; b < argc; b++) if (!strncmp(argv[b], "--scale", 7) || !strncmp(argv[b], "--region", 8)) { fprintf(stderr, "%s: --window carries its own scale and rectangle: not with --scale or --region\n", PROGRAM); return 1; }
			if (strcmp(argv[a], "--window") || strcmp(argv[1], "--picture") || a != 4) { fprintf(stderr, "%s: --window S,X,Y,W,H goes behind --picture <in.nhwp> <image.bmp>\n", PROGRAM); return 1; }
			if (argc != 6 || parse_window(argv[5], win)) { fprintf(stderr, "%s: --window wants S,X,Y,W,H: five decimal numbers, S = 1, 2 or 4\n", PROGRAM); return 1; }
			return decode_picture(argv[2], argv[3], NULL, win);
		}
	for (a = 1; a < argc; a++)                                        /* --scale 1|2|4: anywhere; checked before any file is touched, then taken off the line */
		if (!strncmp(argv[a], "--scale", 7)) {
			int b;
			if (strcmp(argv[a], "--scale") || a + 1 >= argc || strlen(argv[a + 1]) != 1 || !strchr("124", argv[a + 1][0])) { fprintf(stderr, "%s: --scale wants 1, 2 or 4\n", PROGRAM); return 1; }
			g_scale = argv[a + 1][0] - '0';
			for (b = 1; b < argc; b++) if (!strncmp(argv[b], "--region", 8)) { fprintf(stderr, "%s: --scale and --region do not go together (a rectangle at a scale: --window S,X,Y,W,H)\n", PROGRAM); return 1; }
			if (argc > 3 && (!strcmp(argv[1], "--tar") || !strcmp(argv[1], "--tiles"))) { fprintf(stderr, "%s: --scale goes with a single file, --batch or --picture\n", PROGRAM); return 1; }
			for (b = a; b + 2 < argc; b++) argv[b] = argv[b + 2];
			argc -= 2;
			break;
		}
	for (a = 1; a < argc; a++)                                        /* --region: behind --picture <in> <out> only, checked before any file is touched */
		if (!strncmp(argv[a], "--region", 8)) {
			uint32_t reg[4];
			if (strcmp(argv[a], "--region") || strcmp(argv[1], "--picture") || a != 4) { fprintf(stderr, "%s: --region X,Y,W,H goes behind --picture <in.nhwp> <image.bmp>\n", PROGRAM); return 1; }
			if (argc != 6 || parse_region(argv[5], reg)) { fprintf(stderr, "%s: --region wants X,Y,W,H: four decimal numbers\n", PROGRAM); return 1; }
			return decode_picture(argv[2], argv[3], reg, NULL);
		}
	if (g_grey && argc != 3) { fprintf(stderr, "%s: --grey wants <in.nhw> <out.pgm>\n", PROGRAM); return 1; }
	if (argc < 3) { show_usage(); return 0; }
	if (!strcmp(argv[1], "--tar")) {
		if (argc < 4) { show_usage(); return 1; }
		return decode_tar(argv[2], argv[3]);
	}
	if (!strcmp(argv[1], "--picture")) {
		if (argc < 4) { show_usage(); return 1; }
		return decode_picture(argv[2], argv[3], NULL, NULL);
	}
	if (!strcmp(argv[1], "--tiles")) {
		int ny, nx;
		if (argc < 6 || (ny = atoi(argv[2])) < 1 || (nx = atoi(argv[3])) < 1 || ny * nx > 65535) { show_usage(); return 1; }
		return decode_tiles(ny, nx, argv[4], argv[5]);
	}
	if (!strcmp(argv[1], "--batch")) {
		DIR *dir = opendir(argv[2]);
		struct dirent *e;
		char **in = NULL, **out = NULL;
		int n = 0, rc;
		if (!dir) { printf("\nCould not open file\n"); return 1; }
		while ((e = readdir(dir))) {
			const size_t l = strlen(e->d_name);
			if (l < 5 || strcmp(e->d_name + l - 4, ".nhw")) continue;
			in = (char **)realloc(in, (size_t)(n + 1) * sizeof *in); out = (char **)realloc(out, (size_t)(n + 1) * sizeof *out);
			in[n] = (char *)malloc(strlen(argv[2]) + l + 2); out[n] = (char *)malloc(strlen(argv[2]) + l + 2);
			sprintf(in[n], "%s/%s", argv[2], e->d_name);
			sprintf(out[n], "%s/%.*s.bmp", argv[2], (int)(l - 4), e->d_name);
			n++;
		}
		closedir(dir);
		if (!n) return 0;
		rc = decode_files(in, out, n);
		printf("%d file(s) decoded\n", n);
		return rc;
	}
	return decode_files(&argv[1], &argv[2], 1);
}
