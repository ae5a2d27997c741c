/*
 * nhw-enc -- drop-in command line encoder on top of libnhwhip.so (MI355X).
 *
 * Same flags, messages and exit codes as the reference CLI (rcanut/nhwcodec encoder/nhw_encoder_cli.c:88-186:
 * -q<N>, -f, -h, -V, <image.bmp> <image.nhw>) and the same BMP acceptance rules as its reader
 * (encoder/nhw_encoder.c:2902-3098: BIH sizes 12/40/52/56/108/124, 512 x +-512, 24 bpp, BI_RGB, bfOffBits
 * honoured, negative height = flipped rows, short pixel data zero-filled).  The pixel work is done by the HIP
 * library through its C ABI (include/nhw_hip.h); this file is host plumbing only.
 *
 * Batch extensions (not in the reference):
 *   nhw-enc [-q N] [--gpus G] --batch <dir>      every <dir>/x.bmp  -> <dir>/x.nhw, GPU batches of up to 1024 files
 *   nhw-enc [-q N] [--gpus G | --devices a,b,..] --synthetic <count> [--seed S] --outdir <dir>
 *                                                SURVEY 8d generator on the device -> <dir>/synth_<seed>.nhw
 *   --stock-compat   reproduce the stock one-image-per-process binary instead of the canonical output (include/nhw_hip.h)
 *   --max-bytes N [--min-quality M]   (single file, --batch, --tiles) every image at the highest quality from -q down to M (default 1)
 *                    whose file has at most N bytes (nhw_enc_fit_batch); an image that no quality fits is reported and not written
 *   --min-psnr DB [--min-quality M]   (single file, --batch, --tiles) every image at the lowest quality from M (default 1) up to -q whose
 *                    decoded picture reaches DB dB of PSNR (nhw_enc_fit_sse_batch); an image that reaches it at no quality is reported
 *                    and not written
 *   --picture <in.bmp> <out.nhwp>   any 24-bit BMP (W, H >= 1): padded to whole 512 x 512 tiles on the device, one .nhwp container
 *                    (nhw_enc_pictures); alone, not with --max-bytes, --min-psnr, --synthetic, --tar, --tiles or --batch
 *   --resize <W>x<H>   (with --picture, anywhere on the line) the picture is first shrunk or enlarged to W x H (1 .. 4096 each) on the device
 *                    under the area rule (nhw_enc_pictures_resized); a picture more than NHW_AREA_MAX_REDUCTION times W or H is refused
 * --gpus G: images are independent (encoder/nhw_encoder_cli.c:175-183 is a per-image sequence), so the job is a queue of chunks of up
 * to 1024 images; one host thread per GPU, each with its own encoder handle, takes the next chunk until the queue is empty.  The work
 * descriptor {first image, count, quality, seed} lives in this process; between processes (one per GPU under torchrun) it travels by
 * RCCL broadcast: nhwcodec_amd/dist.py, bench.py.
 */
#include <dirent.h>
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nhw_hip.h"

#define PROGRAM "nhw-enc"
#define VERSION "0.3.3-mi355x"
#define QUALITY_MIN 0
#define QUALITY_MAX 23
#define QUALITY_DEFAULT 20

/* header check result codes of the reference (nhw_encoder.c:63-71) -- they become process exit codes */
enum { HDR_OK = 0, HDR_NO_DATA = -12, HDR_NO_SIG = -13, HDR_BIH = -14, HDR_PLANES = -15, HDR_FORMAT = -16 };

static void usage(void)
{
	fprintf(stdout,
	        "Usage: %s [-hV][-q<quality>] <image.bmp> <image.nhw>\n"
	        "Convert image: bmp to nwh\n"
	        " (with a bitmap color 512x512 image)\n"
	        "Options:\n"
	        "  -q#       image quality #:[1..23] {default: 20}\n"
	        "  -h        print this help\n"
	        "  -V        show version and legal information\n\n"
	        "  example: nhw-enc -q15 image.bmp image.nhw\n"
	        "Batch (MI355X build): %s [-q#] [--gpus g | --devices a,b,..] --batch <dir> | --synthetic <n> [--seed s] --outdir <dir>\n"
	        "Tiles (MI355X build): %s [-q#] --tiles <big.bmp> <stem>   (width, height multiples of 512: one <stem>_y<r>_x<c>.nhw per 512x512 tile)\n"
	        "Tar   (MI355X build): %s [-q#] --tar <in.tar> <out.tar>    (every x.bmp member of a ustar archive -> member x.nhw, in order)\n"
	        "Budget (MI355X build): %s [-q#] --max-bytes <n> [--min-quality <m>] ...   (single file, --batch, --tiles: the highest quality from -q# down to m whose file fits n bytes)\n"
	        "PSNR (MI355X build): %s [-q#] --min-psnr <dB> [--min-quality <m>] ...   (single file, --batch, --tiles: the lowest quality from m up to -q# whose decoded picture reaches dB)\n"
	        "Picture (MI355X build): %s [-q#] --picture <in.bmp> <out.nhwp>   (any size: padded 512x512 tiles and the real size in one container)\n"
	        "Resize (MI355X build): %s [-q#] --picture <in.bmp> <out.nhwp> --resize <W>x<H>   (the picture resized to W x H, 1..4096 each, by the area filter first)\n"
	        "Grey  (MI355X build): %s [-q#] --grey <in.pgm> <out.nhw>   (a binary PGM, P5, 512x512, maxval 255, rows top-down: the file of the picture with every grey in B, G and R; the mirror of nhw-dec --grey)\n",
	        PROGRAM, PROGRAM, PROGRAM, PROGRAM, PROGRAM, PROGRAM, PROGRAM, PROGRAM, PROGRAM);
}

static void version(void)
{
	fprintf(stdout, PROGRAM " " VERSION "\nNHW Image encoder, MI355X-native hot path (from-scratch implementation of the\n"
	                "rcanut/nhwcodec .nhw format; see the repository's license and DESIGN.md).\n");
}

static uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static uint16_t le16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }

/* returns HDR_*; fills *offset and *flipped */
static int check_header(FILE *f, long *offset, int *flipped)
{
	uint8_t h[34];
	int bih, width, height, planes, bpp, compr;
	if (fseek(f, 0, SEEK_SET) != 0) return -11;
	if (fread(h, 1, sizeof h, f) < sizeof h) return HDR_NO_DATA;
	if (h[0] != 'B' || h[1] != 'M') return HDR_NO_SIG;
	*offset = (long)(int)le32(h + 10);
	bih = (int)le32(h + 14);
	if (bih != 12 && bih != 40 && bih != 52 && bih != 56 && bih != 108 && bih != 124) return HDR_BIH;
	if (bih == 12) { width = le16(h + 18); height = le16(h + 20); planes = (short)le16(h + 22); bpp = (short)le16(h + 24); compr = 0; }
	else { width = (int)le32(h + 18); height = (int)le32(h + 22); planes = (short)le16(h + 26); bpp = (short)le16(h + 28); compr = (int)le32(h + 30); }
	if (planes != 1) return HDR_PLANES;
	if (width != 512 || (height != 512 && height != -512) || bpp != 24 || compr != 0) return HDR_FORMAT;
	*flipped = height < 0;
	return HDR_OK;
}

/* loads one BMP into dst[786432] exactly like the reference's read path; exits like it on errors */
static void load_bmp(const char *path, uint8_t *dst)
{
	FILE *f = fopen(path, "rb");
	long off = 0;
	int flipped = 0, rc, r;
	if (!f) { printf("menu(): Could not open file: %s\n", path); exit(-1); }
	if ((rc = check_header(f, &off, &flipped)) != HDR_OK) { printf("invalid image file.\n"); exit(rc); }
	if (fseek(f, off, SEEK_SET) != 0) { printf("unable to seek to actual data.\n"); exit(-2); }
	memset(dst, 0, NHW_IMG_BYTES);
	if (fread(dst, 1, NHW_IMG_BYTES, f) < NHW_IMG_BYTES) { /* short read tolerated: tail stays zero */ }
	fclose(f);
	if (flipped) {
		uint8_t *tmp = (uint8_t *)malloc(512 * 3);
		for (r = 0; r < 256; r++) {
			memcpy(tmp, dst + (size_t)r * 1536, 1536);
			memcpy(dst + (size_t)r * 1536, dst + (size_t)(511 - r) * 1536, 1536);
			memcpy(dst + (size_t)(511 - r) * 1536, tmp, 1536);
		}
		free(tmp);
	}
}

/* a binary PGM (P5, 512 x 512, maxval 255; comments allowed in the header) into dst[262144], rows in the byte path's order: the PGM's rows are
 * top-down, as nhw-dec --grey writes them, so PGM row r is row 511 - r.  0, or 1 with a message */
static int load_pgm(const char *path, uint8_t *dst)
{
	FILE *f = fopen(path, "rb");
	int v[3], k = 0, c, r;
	if (!f) { printf("menu(): Could not open file: %s\n", path); return 1; }
	if (fgetc(f) != 'P' || fgetc(f) != '5') { fclose(f); fprintf(stderr, "%s: %s is not a binary PGM (P5)\n", PROGRAM, path); return 1; }
	while (k < 3) {
		c = fgetc(f);
		if (c == '#') { while (c != '\n' && c != EOF) c = fgetc(f); continue; }
		if (c == ' ' || c == '\t' || c == '\n' || c == '\r') continue;
		if (c < '0' || c > '9') { fclose(f); fprintf(stderr, "%s: %s: bad PGM header\n", PROGRAM, path); return 1; }
		for (v[k] = 0; c >= '0' && c <= '9' && v[k] < 100000; c = fgetc(f)) v[k] = 10 * v[k] + (c - '0');
		k++;                                                             /* c: the one white-space byte behind the number */
	}
	if (v[0] != 512 || v[1] != 512 || v[2] != 255) { fclose(f); fprintf(stderr, "%s: %s: --grey wants a 512 x 512 PGM of maxval 255, got %d x %d, maxval %d\n", PROGRAM, path, v[0], v[1], v[2]); return 1; }
	for (r = 0; r < 512; r++)
		if (fread(dst + (size_t)(511 - r) * 512, 1, 512, f) < 512) { fclose(f); fprintf(stderr, "%s: %s: the PGM ends before its 262144 bytes\n", PROGRAM, path); return 1; }
	fclose(f);
	return 0;
}

static int write_file(const char *path, const uint8_t *p, size_t n)
{
	FILE *f = fopen(path, "wb");
	if (!f) { printf("Failed to create file: %s\n", path); return -1; }
	fwrite(p, 1, n, f);
	fclose(f);
	return 0;
}

static void die_lib(const char *what, int rc)
{
	fprintf(stderr, "%s: %s failed (%d): %s\n", PROGRAM, what, rc, nhw_last_error());
	exit(2);
}

/* --tiles: a 24-bit BMP whose sides are multiples of 512 is cut into independent 512x512 tiles, every tile encoded exactly as
 * the reference would encode that crop saved as a BMP of its own (file row order kept; a top-down file is flipped as a whole first, as
 * the reference does with a single tile).  Returns the tiles (malloc), tile (r, c) at index r * nx + c. */
static uint8_t *load_bmp_tiles(const char *path, int *ny, int *nx)
{
	FILE *f = fopen(path, "rb");
	uint8_t h[34], *row, *tiles;
	int bih, width, height, planes, bpp, compr, flipped, r, c;
	long off;
	if (!f) { printf("menu(): Could not open file: %s\n", path); exit(-1); }
	if (fread(h, 1, sizeof h, f) < sizeof h) { printf("invalid image file.\n"); exit(HDR_NO_DATA); }
	if (h[0] != 'B' || h[1] != 'M') { printf("invalid image file.\n"); exit(HDR_NO_SIG); }
	off = (long)(int)le32(h + 10);
	bih = (int)le32(h + 14);
	if (bih != 40 && bih != 52 && bih != 56 && bih != 108 && bih != 124) { printf("invalid image file.\n"); exit(HDR_BIH); }
	width = (int)le32(h + 18); height = (int)le32(h + 22); planes = (short)le16(h + 26); bpp = (short)le16(h + 28); compr = (int)le32(h + 30);
	if (planes != 1) { printf("invalid image file.\n"); exit(HDR_PLANES); }
	flipped = height < 0;
	if (flipped) height = -height;
	if (width < 512 || height < 512 || width % 512 || height % 512 || bpp != 24 || compr != 0) {
		printf("invalid image file.\n");
		fprintf(stderr, "%s: --tiles wants a 24-bit uncompressed BMP whose width and height are multiples of 512 (got %dx%d, %d bpp)\n", PROGRAM, width, height, bpp);
		exit(HDR_FORMAT);
	}
	if (fseek(f, off, SEEK_SET) != 0) { printf("unable to seek to actual data.\n"); exit(-2); }
	*nx = width / 512; *ny = height / 512;
	tiles = (uint8_t *)calloc((size_t)*nx * *ny, NHW_IMG_BYTES);
	row = (uint8_t *)malloc((size_t)width * 3);
	for (r = 0; r < height; r++) {
		const int fr = flipped ? height - 1 - r : r;                  /* row of the picture as the encoder sees it */
		if (fread(row, 1, (size_t)width * 3, f) < (size_t)width * 3) break;   /* short file: the rest stays zero, like the reference's read */
		for (c = 0; c < *nx; c++)
			memcpy(tiles + ((size_t)(fr / 512) * *nx + c) * NHW_IMG_BYTES + (size_t)(fr % 512) * 1536, row + (size_t)c * 1536, 1536);
	}
	free(row);
	fclose(f);
	return tiles;
}

/* --picture: any 24-bit uncompressed BMP (W, H >= 1) as W x H x 3 bytes in file row order (rows are padded to 4 bytes in the file; a
 * top-down file is flipped as a whole first, as load_bmp_tiles does; a short file leaves the rest zero).  Returns the pixels (malloc). */
static uint8_t *load_bmp_picture(const char *path, uint32_t *w, uint32_t *h)
{
	FILE *f = fopen(path, "rb");
	uint8_t h34[34], *px;
	int bih, width, height, planes, bpp, compr, flipped, r;
	long off;
	size_t row, stride;
	if (!f) { printf("menu(): Could not open file: %s\n", path); exit(-1); }
	if (fread(h34, 1, sizeof h34, f) < sizeof h34) { printf("invalid image file.\n"); exit(HDR_NO_DATA); }
	if (h34[0] != 'B' || h34[1] != 'M') { printf("invalid image file.\n"); exit(HDR_NO_SIG); }
	off = (long)(int)le32(h34 + 10);
	bih = (int)le32(h34 + 14);
	if (bih != 40 && bih != 52 && bih != 56 && bih != 108 && bih != 124) { printf("invalid image file.\n"); exit(HDR_BIH); }
	width = (int)le32(h34 + 18); height = (int)le32(h34 + 22); planes = (short)le16(h34 + 26); bpp = (short)le16(h34 + 28); compr = (int)le32(h34 + 30);
	if (planes != 1) { printf("invalid image file.\n"); exit(HDR_PLANES); }
	flipped = height < 0;
	if (flipped) height = -height;
	if (width < 1 || width > 65535 || height < 1 || height > 65535 || bpp != 24 || compr != 0) {
		printf("invalid image file.\n");
		fprintf(stderr, "%s: --picture wants a 24-bit uncompressed BMP with sides 1..65535 (got %dx%d, %d bpp)\n", PROGRAM, width, height, bpp);
		exit(HDR_FORMAT);
	}
	if (fseek(f, off, SEEK_SET) != 0) { printf("unable to seek to actual data.\n"); exit(-2); }
	row = (size_t)width * 3; stride = (row + 3) & ~(size_t)3;
	px = (uint8_t *)calloc((size_t)height, row);
	if (!px) { fprintf(stderr, "%s: out of memory for a %dx%d picture\n", PROGRAM, width, height); exit(-1); }
	for (r = 0; r < height; r++) {
		const int fr = flipped ? height - 1 - r : r;                  /* row of the picture as the encoder sees it */
		if (fread(px + (size_t)fr * row, 1, row, f) < row) break;      /* short file: the rest stays zero */
		if (stride > row && fseek(f, (long)(stride - row), SEEK_CUR) != 0) break;
	}
	fclose(f);
	*w = (uint32_t)width; *h = (uint32_t)height;
	return px;
}

/* out_w, out_h: the size of --resize, 0 without it */
static int encode_picture(const char *in_path, const char *out_path, int quality, int stock_compat, uint32_t out_w, uint32_t out_h)
{
	uint32_t w = 0, h = 0;
	uint8_t *px = load_bmp_picture(in_path, &w, &h), *arena;
	const int t = out_w ? nhw_picture_tiles(out_w, out_h) : nhw_picture_tiles(w, h);
	const size_t cap = 16 + (size_t)t * (4 + NHW_OUT_STRIDE);
	uint64_t in_off[2] = { 0, 3ull * w * h }, off[2];
	int32_t st = 0;
	nhw_enc *enc = NULL;
	int rc;
	if (out_w && (w > NHW_AREA_MAX_REDUCTION * out_w || h > NHW_AREA_MAX_REDUCTION * out_h)) {   /* before any GPU work */
		fprintf(stderr, "%s: --resize: the %ux%u picture is more than %d times %ux%u along a side\n", PROGRAM, (unsigned)w, (unsigned)h, NHW_AREA_MAX_REDUCTION, (unsigned)out_w, (unsigned)out_h);
		return 1;
	}
	if ((rc = nhw_enc_create(0, t < 1024 ? t : 1024, &enc))) die_lib("nhw_enc_create", rc);   /* (the batch modes' chunk) */
	if (stock_compat) nhw_enc_set_compat(enc, NHW_COMPAT_GLIBC_ONESHOT);
	arena = (uint8_t *)malloc(cap);
	if (!arena) { fprintf(stderr, "%s: out of memory\n", PROGRAM); exit(-1); }
	if (out_w) {
		if ((rc = nhw_enc_pictures_resized(enc, px, in_off, &w, &h, 1, out_w, out_h, quality, arena, cap, off, &st))) die_lib("nhw_enc_pictures_resized", rc);
		w = out_w; h = out_h;
	} else if ((rc = nhw_enc_pictures(enc, px, in_off, &w, &h, 1, quality, arena, cap, off, &st))) die_lib("nhw_enc_pictures", rc);
	nhw_enc_destroy(enc);
	free(px);
	if (st) { fprintf(stderr, "%s: %s: encoder status %d (code book overflow)\n", PROGRAM, in_path, st); free(arena); return 1; }
	rc = write_file(out_path, arena + off[0], (size_t)(off[1] - off[0])) ? 1 : 0;
	if (!rc) printf("%u x %u picture, %d tile(s)\n", (unsigned)w, (unsigned)h, t);
	free(arena);
	return rc;
}

/* --max-bytes: the byte budget of every image (0: off) and the ladder, -q down to --min-quality;
 * --min-psnr: the PSNR target in dB (0: off), its SSE bound and the ladder, --min-quality up to -q */
static uint32_t g_max_bytes;
static double g_min_psnr;
static uint64_t g_max_sse;
static int g_ladder[23], g_ladder_len;

/* encode n images: at one quality, with --max-bytes at the first quality of the ladder that fits, with --min-psnr at the first whose decode
 * by `dec` reaches the target (qual[i], sse[i] may be NULL without them) */
static int encode_images(nhw_enc *enc, nhw_dec *dec, const uint8_t *imgs, int n, int quality, uint8_t *arena, size_t cap, uint64_t *off, int32_t *st,
                         int32_t *qual, uint64_t *sse)
{
	int i, rc;
	if (g_min_psnr > 0) {
		uint64_t *target = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)n);
		for (i = 0; i < n; i++) target[i] = g_max_sse;
		rc = nhw_enc_fit_sse_batch(enc, dec, imgs, n, target, g_ladder, g_ladder_len, arena, cap, off, st, qual, sse);
		free(target);
		return rc;
	}
	if (g_max_bytes) {
		uint32_t *budget = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)n);
		for (i = 0; i < n; i++) budget[i] = g_max_bytes;
		rc = nhw_enc_fit_batch(enc, imgs, n, budget, g_ladder, g_ladder_len, arena, cap, off, st, qual);
		free(budget);
		return rc;
	}
	return nhw_enc_batch(enc, imgs, n, quality, arena, cap, off, st);
}

/* a decoder handle next to the encoder when --min-psnr needs one, else NULL */
static nhw_dec *psnr_decoder(int device, int max_batch)
{
	nhw_dec *dec = NULL;
	int rc;
	if (g_min_psnr <= 0) return NULL;
	if ((rc = nhw_dec_create(device, max_batch, &dec))) { fprintf(stderr, "%s: nhw_dec_create failed (%d): %s\n", PROGRAM, rc, nhw_dec_last_error()); exit(2); }
	return dec;
}

static double psnr_of(uint64_t sse) { return sse ? 10.0 * log10(65025.0 * (double)NHW_IMG_BYTES / (double)sse) : INFINITY; }

/* write one image's file, or say why there is none; returns the number of failures (0 or 1) */
static int emit(const char *path, int32_t st, int32_t qual, uint64_t sse, const uint8_t *p, size_t n)
{
	if (st == NHW_E_BUDGET && g_min_psnr > 0) {
		fprintf(stderr, "%s: %s: no quality in q%d..q%d reaches %.2f dB (best, q%d: %.2f dB)\n", PROGRAM, path, g_ladder[0], g_ladder[g_ladder_len - 1], g_min_psnr,
		        (int)qual, psnr_of(sse));
		return 1;
	}
	if (st == NHW_E_BUDGET) {
		fprintf(stderr, "%s: %s: no quality in q%d..q%d fits %u bytes (q%d: %zu bytes)\n", PROGRAM, path, g_ladder[0], g_ladder[g_ladder_len - 1], (unsigned)g_max_bytes, (int)qual, n);
		return 1;
	}
	if (st) { fprintf(stderr, "%s: %s: encoder status %d (code book overflow)\n", PROGRAM, path, st); return 1; }
	return write_file(path, p, n) ? 1 : 0;
}

static int encode_host_batch(nhw_enc *enc, nhw_dec *dec, const uint8_t *imgs, int n, int quality, char **out_names)
{
	uint8_t *arena = (uint8_t *)malloc((size_t)n * NHW_OUT_STRIDE);
	uint64_t *off = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(n + 1));
	int32_t *st = (int32_t *)malloc(sizeof(int32_t) * (size_t)n);
	int32_t *qual = (int32_t *)malloc(sizeof(int32_t) * (size_t)n);
	uint64_t *sse = (uint64_t *)calloc((size_t)n, sizeof(uint64_t));
	int i, rc, bad = 0;
	rc = encode_images(enc, dec, imgs, n, quality, arena, (size_t)n * NHW_OUT_STRIDE, off, st, qual, sse);
	if (rc) die_lib(g_min_psnr > 0 ? "nhw_enc_fit_sse_batch" : g_max_bytes ? "nhw_enc_fit_batch" : "nhw_enc_batch", rc);
	for (i = 0; i < n; i++) bad += emit(out_names[i], st[i], qual[i], sse[i], arena + off[i], (size_t)(off[i + 1] - off[i]));
	free(sse); free(qual); free(st); free(off); free(arena);
	return bad;
}

static int ends_with(const char *s, const char *suf)
{
	size_t a = strlen(s), b = strlen(suf);
	return a >= b && strcmp(s + a - b, suf) == 0;
}

/* the job queue of the batch modes: chunks of up to 1024 images, taken in order by one host thread per GPU */
#define CHUNK 1024                 /* images per GPU batch at most */
static int g_chunk = CHUNK;        /* --chunk N: images a worker takes from the queue at a time (1 .. CHUNK) */
struct job {
	int n, next;                   /* images in the job, first image nobody has taken yet */
	int quality, stock_compat;
	uint32_t seed;                 /* --synthetic: image i is generator seed `seed + i` */
	char **in, **out;              /* --batch: file names */
	const char *outdir;            /* --synthetic */
	pthread_mutex_t lock;
};
struct worker { struct job *jb; int device, bad; };

static void *worker_main(void *arg)
{
	struct worker *w = (struct worker *)arg;
	struct job *jb = w->jb;
	nhw_enc *enc = NULL;
	uint8_t *imgs = NULL, *arena = NULL;
	int imgs_pinned = 0;
	uint64_t *off = (uint64_t *)malloc(sizeof(uint64_t) * (CHUNK + 1));
	int32_t *st = (int32_t *)malloc(sizeof(int32_t) * CHUNK);
	int32_t *qual = (int32_t *)malloc(sizeof(int32_t) * CHUNK);
	uint64_t *sse = (uint64_t *)calloc(CHUNK, sizeof(uint64_t));
	const int cap = jb->n < g_chunk ? jb->n : g_chunk;
	nhw_dec *dec = NULL;
	int rc, i;
	if ((rc = nhw_enc_create(w->device, cap, &enc))) die_lib("nhw_enc_create", rc);
	if (jb->stock_compat) nhw_enc_set_compat(enc, NHW_COMPAT_GLIBC_ONESHOT);
	dec = psnr_decoder(w->device, cap);
	arena = (uint8_t *)malloc((size_t)cap * NHW_OUT_STRIDE);
	if (!jb->outdir) {                                 /* page-locked input buffer: the upload runs at PCIe speed next to the encode */
		imgs = (uint8_t *)nhw_host_alloc((size_t)cap * NHW_IMG_BYTES);
		imgs_pinned = imgs != NULL;
		if (!imgs) imgs = (uint8_t *)malloc((size_t)cap * NHW_IMG_BYTES);
		if (!imgs) { fprintf(stderr, "%s: out of memory for %d input images\n", PROGRAM, cap); exit(-1); }
	}
	for (;;) {
		int base, m;
		pthread_mutex_lock(&jb->lock);
		base = jb->next; m = jb->n - base < g_chunk ? jb->n - base : g_chunk; jb->next += m > 0 ? m : 0;
		pthread_mutex_unlock(&jb->lock);
		if (m <= 0) break;
		if (jb->outdir) rc = nhw_enc_synth_batch(enc, m, jb->seed + (uint32_t)base, jb->quality, arena, (size_t)cap * NHW_OUT_STRIDE, off, st);
		else {
			for (i = 0; i < m; i++) load_bmp(jb->in[base + i], imgs + (size_t)i * NHW_IMG_BYTES);
			rc = encode_images(enc, dec, imgs, m, jb->quality, arena, (size_t)cap * NHW_OUT_STRIDE, off, st, qual, sse);
		}
		if (rc) die_lib("encode", rc);
		for (i = 0; i < m; i++) {
			char name[4096];
			const char *path = name;
			if (jb->outdir) snprintf(name, sizeof name, "%s/synth_%u.nhw", jb->outdir, (unsigned)(jb->seed + (uint32_t)(base + i)));
			else path = jb->out[base + i];
			w->bad += emit(path, st[i], qual[i], sse[i], arena + off[i], (size_t)(off[i + 1] - off[i]));
		}
	}
	if (imgs_pinned) nhw_host_free(imgs); else free(imgs);        /* before the handle goes: page-locked memory belongs to its device context */
	nhw_enc_destroy(enc);
	if (dec) nhw_dec_destroy(dec);
	free(sse); free(qual); free(st); free(off); free(arena);
	return NULL;
}

/* --tar: a POSIX ustar archive as the batch container.  Members are read in order; every regular member whose name ends in
 * .bmp goes through the same header checks as a file on its own (a member that fails them is reported and left out), the images are
 * encoded in chunks of CHUNK, and the .nhw files leave as members of the output archive under the same names with the suffix changed. */
static unsigned long tar_octal(const uint8_t *p, int n) { unsigned long v = 0; int i; for (i = 0; i < n && p[i] >= '0' && p[i] <= '7'; i++) v = v * 8 + (unsigned long)(p[i] - '0'); return v; }
static int tar_write_member(FILE *f, const char *name, const uint8_t *data, size_t len)
{
	uint8_t h[512];
	unsigned sum = 0;
	size_t i, pad = (512 - len % 512) % 512;
	static const uint8_t zeros[512];
	memset(h, 0, sizeof h);
	if (strlen(name) > 99) { fprintf(stderr, "%s: member name too long for the archive: %s\n", PROGRAM, name); return -1; }
	strcpy((char *)h, name);
	memcpy(h + 100, "0000644", 8); memcpy(h + 108, "0000000", 8); memcpy(h + 116, "0000000", 8);
	snprintf((char *)h + 124, 12, "%011lo", (unsigned long)len);
	memcpy(h + 136, "00000000000", 12);
	memset(h + 148, ' ', 8);
	h[156] = '0';
	memcpy(h + 257, "ustar", 6); memcpy(h + 263, "00", 2);
	for (i = 0; i < 512; i++) sum += h[i];
	snprintf((char *)h + 148, 8, "%06o", sum); h[155] = ' ';
	if (fwrite(h, 1, 512, f) != 512 || fwrite(data, 1, len, f) != len || fwrite(zeros, 1, pad, f) != pad) return -1;
	return 0;
}
/* a BMP held in memory -> dst[786432], the same acceptance rules as check_header + load_bmp; returns HDR_OK or the reference's code */
static int bmp_from_memory(const uint8_t *b, size_t len, uint8_t *dst)
{
	int bih, width, height, planes, bpp, compr, r;
	long off;
	if (len < 34) return HDR_NO_DATA;
	if (b[0] != 'B' || b[1] != 'M') return HDR_NO_SIG;
	off = (long)(int)le32(b + 10);
	bih = (int)le32(b + 14);
	if (bih != 12 && bih != 40 && bih != 52 && bih != 56 && bih != 108 && bih != 124) return HDR_BIH;
	if (bih == 12) { width = le16(b + 18); height = le16(b + 20); planes = (short)le16(b + 22); bpp = (short)le16(b + 24); compr = 0; }
	else { width = (int)le32(b + 18); height = (int)le32(b + 22); planes = (short)le16(b + 26); bpp = (short)le16(b + 28); compr = (int)le32(b + 30); }
	if (planes != 1) return HDR_PLANES;
	if (width != 512 || (height != 512 && height != -512) || bpp != 24 || compr != 0) return HDR_FORMAT;
	memset(dst, 0, NHW_IMG_BYTES);
	if (off >= 0 && (size_t)off < len) memcpy(dst, b + off, len - (size_t)off < NHW_IMG_BYTES ? len - (size_t)off : NHW_IMG_BYTES);   /* short data: the tail stays zero */
	if (height < 0)
		for (r = 0; r < 256; r++) {
			uint8_t tmp[1536];
			memcpy(tmp, dst + (size_t)r * 1536, 1536);
			memcpy(dst + (size_t)r * 1536, dst + (size_t)(511 - r) * 1536, 1536);
			memcpy(dst + (size_t)(511 - r) * 1536, tmp, 1536);
		}
	return HDR_OK;
}
#define TAR_BMP_MAX (4u << 20)      /* largest archive member taken for an image */
/* skip n bytes of the archive: by seeking, or by reading where the input cannot seek (a pipe); non-zero at the end of the input */
static int tar_skip(FILE *in, unsigned long n)
{
	uint8_t sink[4096];
	if (n == 0) return 0;
	if (fseek(in, (long)n, SEEK_CUR) == 0) return 0;
	while (n) { const size_t k = n < sizeof sink ? (size_t)n : sizeof sink; if (fread(sink, 1, k, in) != k) return 1; n -= (unsigned long)k; }
	return 0;
}
static int encode_tar(const char *in_path, const char *out_path, int quality, int stock_compat)
{
	FILE *in = fopen(in_path, "rb"), *out;
	nhw_enc *enc = NULL;
	uint8_t hdr[512], *imgs, *arena, *member = NULL;
	size_t member_cap = 0;
	uint64_t *off = (uint64_t *)malloc(sizeof(uint64_t) * (CHUNK + 1));
	int32_t *st = (int32_t *)malloc(sizeof(int32_t) * CHUNK);
	char (*names)[104] = (char (*)[104])malloc((size_t)CHUNK * 104);
	int n = 0, total = 0, bad = 0, rc, i, eof = 0;
	static const uint8_t zeros[1024];
	if (!in) { printf("menu(): Could not open file: %s\n", in_path); exit(-1); }
	out = fopen(out_path, "wb");
	if (!out) { printf("Failed to create file: %s\n", out_path); return 1; }
	imgs = (uint8_t *)malloc((size_t)CHUNK * NHW_IMG_BYTES);
	arena = (uint8_t *)malloc((size_t)CHUNK * NHW_OUT_STRIDE);
	while (!eof) {
		unsigned long size = 0;
		int is_bmp = 0;
		if (fread(hdr, 1, 512, in) != 512 || hdr[0] == 0) eof = 1;          /* end of archive: a zero block (or the file's end) */
		else {
			size_t nl;
			size = tar_octal(hdr + 124, 12);
			hdr[99] = 0;
			nl = strlen((const char *)hdr);
			is_bmp = (hdr[156] == '0' || hdr[156] == 0) && nl > 4 && !strcmp((const char *)hdr + nl - 4, ".bmp");
			if (is_bmp) {
				if (size > TAR_BMP_MAX) {                          /* a 512 x 512 24-bit BMP is 786 486 bytes; a header that claims gigabytes is damage */
					fprintf(stderr, "%s: %s: member of %lu bytes is no 512 x 512 image, left out\n", PROGRAM, (const char *)hdr, size); bad++;
					if (tar_skip(in, (size + 511) / 512 * 512)) { fprintf(stderr, "%s: %s: archive ends inside member %s\n", PROGRAM, in_path, (const char *)hdr); eof = 1; }
					is_bmp = 0;
				}
				else if (size + 1 > member_cap) {
					uint8_t *grown = (uint8_t *)realloc(member, size + 1);
					if (!grown) { fprintf(stderr, "%s: out of memory for a member of %lu bytes\n", PROGRAM, size); exit(-1); }
					member = grown; member_cap = size + 1;
				}
				if (!is_bmp) { }
				else if (fread(member, 1, size, in) != size) { fprintf(stderr, "%s: %s: archive ends inside member %s\n", PROGRAM, in_path, (const char *)hdr); bad++; eof = 1; is_bmp = 0; }
				else {
					const int hc = bmp_from_memory(member, size, imgs + (size_t)n * NHW_IMG_BYTES);
					if (hc != HDR_OK) { fprintf(stderr, "%s: %s: invalid image file (%d), left out\n", PROGRAM, (const char *)hdr, hc); bad++; }
					else { snprintf(names[n], 104, "%.*s.nhw", (int)(nl - 4), (const char *)hdr); n++; }
				}
				if (is_bmp && size % 512 && tar_skip(in, 512 - size % 512)) eof = 1;
			}
			else if (tar_skip(in, (size + 511) / 512 * 512)) eof = 1;
		}
		if (n == CHUNK || (eof && n > 0)) {
			if (!enc) {
				if ((rc = nhw_enc_create(0, CHUNK, &enc))) die_lib("nhw_enc_create", rc);
				if (stock_compat) nhw_enc_set_compat(enc, NHW_COMPAT_GLIBC_ONESHOT);
			}
			if ((rc = nhw_enc_batch(enc, imgs, n, quality, arena, (size_t)CHUNK * NHW_OUT_STRIDE, off, st))) die_lib("nhw_enc_batch", rc);
			for (i = 0; i < n; i++) {
				if (st[i]) { fprintf(stderr, "%s: %s: encoder status %d (code book overflow)\n", PROGRAM, names[i], st[i]); bad++; continue; }
				if (tar_write_member(out, names[i], arena + off[i], (size_t)(off[i + 1] - off[i]))) { bad++; break; }
			}
			total += n; n = 0;
		}
	}
	fwrite(zeros, 1, 1024, out);
	fclose(out); fclose(in);
	if (enc) nhw_enc_destroy(enc);
	printf("%d image(s) encoded\n", total);
	free(member); free(names); free(st); free(off); free(arena); free(imgs);
	return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
	int quality = QUALITY_DEFAULT, overwrite = 0, synthetic = 0, gpus = 1, i;
	int devlist[16], ndevlist = 0;
	uint32_t seed = 0;
	const char *batch_dir = NULL, *outdir = NULL;
	int tiles = 0, tar = 0, picture = 0, grey = 0;
	int stock_compat = 0;   /* --stock-compat: NHW_COMPAT_GLIBC_ONESHOT, the stock binary's out-of-bounds reads (include/nhw_hip.h) */
	const char *max_bytes_arg = NULL, *min_quality_arg = NULL;   /* --max-bytes, --min-quality, --min-psnr: checked once the flags are read */
	const char *min_psnr_arg = NULL;
	const char *resize_arg = NULL;                               /* --resize: may stand behind the file names, so it is taken off the line first */
	uint32_t resize_w = 0, resize_h = 0;
	nhw_dec *dec = NULL;
	nhw_enc *enc = NULL;
	int rc;

	for (i = 1; i < argc; i++)
		if (!strcmp(argv[i], "--resize")) {
			int k;
			const int took = i + 1 < argc ? 2 : 1;
			resize_arg = took == 2 ? argv[i + 1] : "";
			for (k = i; k + took < argc; k++) argv[k] = argv[k + took];
			argc -= took;
			break;
		}
	while (argc > 1 && argv[1][0] == '-') {
		if (!strcmp(argv[1], "--batch") && argc > 2) { batch_dir = argv[2]; argc -= 2; argv += 2; continue; }
		if (!strcmp(argv[1], "--synthetic") && argc > 2) { synthetic = atoi(argv[2]); argc -= 2; argv += 2; continue; }
		if (!strcmp(argv[1], "--seed") && argc > 2) { seed = (uint32_t)strtoul(argv[2], NULL, 10); argc -= 2; argv += 2; continue; }
		if (!strcmp(argv[1], "--outdir") && argc > 2) { outdir = argv[2]; argc -= 2; argv += 2; continue; }
		if (!strcmp(argv[1], "--gpus") && argc > 2) { gpus = atoi(argv[2]); argc -= 2; argv += 2; continue; }
		if (!strcmp(argv[1], "--chunk") && argc > 2) {
			char *end;
			const long v = strtol(argv[2], &end, 10);
			if (end == argv[2] || *end || v < 1 || v > CHUNK) { fprintf(stderr, "%s: --chunk wants a number 1..%d, got '%s'\n", PROGRAM, CHUNK, argv[2]); return 1; }
			g_chunk = (int)v; argc -= 2; argv += 2; continue;
		}
		if (!strcmp(argv[1], "--devices") && argc > 2) {            /* one worker per entry; a device may be named more than once (two handles, two workers on one GPU) */
			const char *p = argv[2];
			for (;;) {                                                /* digits, comma, digits, ..: anything else (empty list, trailing comma, garbage, more than 16 entries) is an error, not device 0 */
				char *end;
				const long v = strtol(p, &end, 10);
				if (end == p || v < 0 || v > 1023) { fprintf(stderr, "%s: --devices wants a comma-separated list of device numbers, got '%s'\n", PROGRAM, argv[2]); return 1; }
				if (ndevlist >= 16) { fprintf(stderr, "%s: --devices: at most 16 entries\n", PROGRAM); return 1; }
				devlist[ndevlist++] = (int)v;
				if (*end == '\0') break;
				if (*end != ',' || end[1] == '\0') { fprintf(stderr, "%s: --devices wants a comma-separated list of device numbers, got '%s'\n", PROGRAM, argv[2]); return 1; }
				p = end + 1;
			}
			argc -= 2; argv += 2; continue;
		}
		if (!strcmp(argv[1], "--max-bytes") && argc > 2) { max_bytes_arg = argv[2]; argc -= 2; argv += 2; continue; }
		if (!strcmp(argv[1], "--min-psnr") && argc > 2) { min_psnr_arg = argv[2]; argc -= 2; argv += 2; continue; }
		if (!strcmp(argv[1], "--min-quality") && argc > 2) { min_quality_arg = argv[2]; argc -= 2; argv += 2; continue; }
		if (!strcmp(argv[1], "--stock-compat")) { stock_compat = 1; argc -= 1; argv += 1; continue; }
		if (!strcmp(argv[1], "--tiles")) { tiles = 1; argc -= 1; argv += 1; continue; }
		if (!strcmp(argv[1], "--tar")) { tar = 1; argc -= 1; argv += 1; continue; }
		if (!strcmp(argv[1], "--picture")) { picture = 1; argc -= 1; argv += 1; continue; }
		if (!strcmp(argv[1], "--grey")) { grey = 1; argc -= 1; argv += 1; continue; }
		for (i = 1; argv[1][i] != '\0'; i++) {
			const char ch = argv[1][i];
			if (ch >= '0' && ch <= '9') continue;
			if (ch == 'q') {
				const char *num = &argv[1][i + 1];
				if (*num >= '0' && *num <= '9') {
					quality = atoi(num);
					if (quality < QUALITY_MIN || quality > QUALITY_MAX) { printf("quality=%d out of range\n", quality); exit(1); }
				} else { printf("invalid quality='%s'\n", num); exit(1); }
			}
			else if (ch == 'f') overwrite = 1;
			else if (ch == 'h') { usage(); exit(0); }
			else if (ch == 'V') { version(); exit(0); }
			else { fprintf(stderr, "Unknown option '-%c'\n", ch); exit(1); }
		}
		argc--; argv++;
	}
	(void)overwrite; /* the reference's overwrite check is effectively off (its flag is never initialised, nhw_encoder_cli.c:93,164) */

	if (!nhw_quality_supported(quality)) {
		fprintf(stderr, "%s: quality %d is not implemented (supported: 1..23; the reference accepts -q0 but has no tables for it)\n", PROGRAM, quality);
		return 3;
	}
	if (grey && (max_bytes_arg || min_psnr_arg || min_quality_arg || resize_arg || synthetic > 0 || tar || tiles || batch_dir || picture)) {   /* before any file is touched */
		fprintf(stderr, "%s: --grey works alone, not with --batch, --synthetic, --tar, --tiles, --picture, --max-bytes, --min-psnr, --min-quality or --resize\n", PROGRAM);
		return 1;
	}
	if (picture && (max_bytes_arg || min_psnr_arg || min_quality_arg || synthetic > 0 || tar || tiles || batch_dir)) {   /* before any GPU work */
		fprintf(stderr, "%s: --picture works alone, not with --max-bytes, --min-psnr, --min-quality, --synthetic, --tar, --tiles or --batch\n", PROGRAM);
		return 1;
	}
	if (resize_arg) {                                                /* before any GPU work */
		char *end, *end2 = NULL;
		long rw, rh;
		if (!picture) { fprintf(stderr, "%s: --resize works with --picture only\n", PROGRAM); return 1; }
		rw = strtol(resize_arg, &end, 10);
		rh = *end == 'x' ? strtol(end + 1, &end2, 10) : 0;
		if (end == resize_arg || *end != 'x' || end2 == end + 1 || *end2 || resize_arg[0] == '-' || resize_arg[0] == '+' || end[1] == '-' || end[1] == '+') {
			fprintf(stderr, "%s: --resize wants <W>x<H>, got '%s'\n", PROGRAM, resize_arg);
			return 1;
		}
		if (rw < 1 || rw > 4096 || rh < 1 || rh > 4096) { fprintf(stderr, "%s: --resize: the sides must be 1..4096, got '%s'\n", PROGRAM, resize_arg); return 1; }
		resize_w = (uint32_t)rw; resize_h = (uint32_t)rh;
	}
	if (max_bytes_arg || min_quality_arg || min_psnr_arg) {          /* before any GPU work */
		char *end;
		long v;
		int min_q = 1;
		if (!max_bytes_arg && !min_psnr_arg) { fprintf(stderr, "%s: --min-quality needs --max-bytes or --min-psnr\n", PROGRAM); return 1; }
		if (max_bytes_arg && min_psnr_arg) { fprintf(stderr, "%s: --max-bytes and --min-psnr are mutually exclusive\n", PROGRAM); return 1; }
		if (min_psnr_arg) {
			const double db = strtod(min_psnr_arg, &end);
			if (end == min_psnr_arg || *end || !isfinite(db) || !(db > 0)) { fprintf(stderr, "%s: --min-psnr wants a positive number of dB, got '%s'\n", PROGRAM, min_psnr_arg); return 1; }
			g_min_psnr = db;
			g_max_sse = (uint64_t)floor(65025.0 * (double)NHW_IMG_BYTES * pow(10.0, -db / 10.0));   /* nhwcodec_amd.psnr_to_max_sse */
		} else {
			v = strtol(max_bytes_arg, &end, 10);
			if (end == max_bytes_arg || *end || v < 1 || v > 0x7FFFFFFFL) { fprintf(stderr, "%s: --max-bytes wants a positive number of bytes, got '%s'\n", PROGRAM, max_bytes_arg); return 1; }
			g_max_bytes = (uint32_t)v;
		}
		if (min_quality_arg) {
			v = strtol(min_quality_arg, &end, 10);
			if (end == min_quality_arg || *end || !nhw_quality_supported((int)v)) { fprintf(stderr, "%s: --min-quality wants a quality 1..23, got '%s'\n", PROGRAM, min_quality_arg); return 1; }
			min_q = (int)v;
		}
		if (min_q > quality) { fprintf(stderr, "%s: --min-quality %d is above the top quality q%d\n", PROGRAM, min_q, quality); return 1; }
		if (synthetic > 0 || tar) { fprintf(stderr, "%s: %s works with a single file, --batch and --tiles, not with --synthetic or --tar\n", PROGRAM, min_psnr_arg ? "--min-psnr" : "--max-bytes"); return 1; }
		if (min_psnr_arg) for (g_ladder_len = 0; min_q + g_ladder_len <= quality; g_ladder_len++) g_ladder[g_ladder_len] = min_q + g_ladder_len;
		else for (g_ladder_len = 0; quality - g_ladder_len >= min_q; g_ladder_len++) g_ladder[g_ladder_len] = quality - g_ladder_len;
	}

	if (synthetic > 0 || batch_dir) {
		struct job jb;
		pthread_t th[16];
		struct worker wk[16];
		int ndev = nhw_device_count(), g, bad = 0;
		memset(&jb, 0, sizeof jb);
		jb.quality = quality; jb.stock_compat = stock_compat; jb.seed = seed;
		pthread_mutex_init(&jb.lock, NULL);
		if (synthetic > 0) {
			if (!outdir) { fprintf(stderr, "%s: --synthetic needs --outdir <dir>\n", PROGRAM); return 1; }
			jb.n = synthetic; jb.outdir = outdir;
		} else {
			DIR *d = opendir(batch_dir);
			struct dirent *de;
			int cap = 0;
			if (!d) { printf("menu(): Could not open file: %s\n", batch_dir); exit(-1); }
			while ((de = readdir(d))) {
				if (!ends_with(de->d_name, ".bmp")) continue;
				if (jb.n == cap) { cap = cap ? cap * 2 : 256; jb.in = (char **)realloc(jb.in, sizeof(char *) * cap); jb.out = (char **)realloc(jb.out, sizeof(char *) * cap); }
				jb.in[jb.n] = (char *)malloc(strlen(batch_dir) + strlen(de->d_name) + 2);
				sprintf(jb.in[jb.n], "%s/%s", batch_dir, de->d_name);
				jb.out[jb.n] = strdup(jb.in[jb.n]);
				strcpy(jb.out[jb.n] + strlen(jb.out[jb.n]) - 4, ".nhw");
				jb.n++;
			}
			closedir(d);
			if (!jb.n) { printf("Not enough arguments. Check help.\n"); return 0; }
		}
		if (ndev < 1) { fprintf(stderr, "%s: no GPU visible\n", PROGRAM); return 2; }
		if (gpus < 1) gpus = 1;
		if (ndevlist) {
			gpus = ndevlist;
			for (g = 0; g < gpus; g++) if (devlist[g] < 0 || devlist[g] >= ndev) { fprintf(stderr, "%s: --devices names device %d but %d device(s) visible\n", PROGRAM, devlist[g], ndev); return 1; }
		} else {
			if (gpus > ndev) { fprintf(stderr, "%s: --gpus %d but %d device(s) visible\n", PROGRAM, gpus, ndev); return 1; }
			if (gpus > 16) gpus = 16;
			for (g = 0; g < gpus; g++) devlist[g] = g;
		}
		for (g = 0; g < gpus; g++) { wk[g].jb = &jb; wk[g].device = devlist[g]; wk[g].bad = 0; pthread_create(&th[g], NULL, worker_main, &wk[g]); }
		for (g = 0; g < gpus; g++) { pthread_join(th[g], NULL); bad += wk[g].bad; }
		return bad ? 1 : 0;
	}

	if (argc < 3) { printf("Not enough arguments. Check help.\n"); usage(); return 0; }
	if (grey) {
		uint8_t *px = (uint8_t *)malloc(NHW_GREY_BYTES), *arena = (uint8_t *)malloc(NHW_OUT_STRIDE);
		uint64_t off[2];
		int32_t st = 0;
		int bad;
		if (strcmp(argv[1], argv[2]) == 0) { fprintf(stdout, "Input and output are the same file: '%s'.\n", argv[1]); return 1; }
		if (load_pgm(argv[1], px)) return 1;
		if ((rc = nhw_enc_create(0, 1, &enc))) die_lib("nhw_enc_create", rc);
		if (stock_compat) nhw_enc_set_compat(enc, NHW_COMPAT_GLIBC_ONESHOT);
		if ((rc = nhw_enc_batch_grey(enc, px, 1, quality, arena, NHW_OUT_STRIDE, off, &st))) die_lib("nhw_enc_batch_grey", rc);
		bad = emit(argv[2], st, -1, 0, arena + off[0], (size_t)(off[1] - off[0]));
		nhw_enc_destroy(enc);
		free(px); free(arena);
		return bad ? 1 : 0;
	}
	if (tar) return encode_tar(argv[1], argv[2], quality, stock_compat);
	if (picture) return encode_picture(argv[1], argv[2], quality, stock_compat, resize_w, resize_h);
	if (tiles) {
		int ny = 0, nx = 0, n, bad, t;
		uint8_t *imgs = load_bmp_tiles(argv[1], &ny, &nx);
		char **names;
		n = ny * nx;
		names = (char **)malloc(sizeof(char *) * (size_t)n);
		for (t = 0; t < n; t++) {
			names[t] = (char *)malloc(strlen(argv[2]) + 48);
			sprintf(names[t], "%s_y%d_x%d.nhw", argv[2], t / nx, t % nx);
		}
		if ((rc = nhw_enc_create(0, n, &enc))) die_lib("nhw_enc_create", rc);
		if (stock_compat) nhw_enc_set_compat(enc, NHW_COMPAT_GLIBC_ONESHOT);
		dec = psnr_decoder(0, n);
		bad = encode_host_batch(enc, dec, imgs, n, quality, names);
		nhw_enc_destroy(enc);
		if (dec) nhw_dec_destroy(dec);
		printf("%d x %d tiles\n", ny, nx);
		free(imgs);
		return bad ? 1 : 0;
	}
	if (strcmp(argv[1], argv[2]) == 0) { fprintf(stdout, "Input and output are the same file: '%s'.\n", argv[1]); return 1; }
	{
		uint8_t *img = (uint8_t *)malloc(NHW_IMG_BYTES);
		char *names[1];
		int bad;
		load_bmp(argv[1], img);
		if ((rc = nhw_enc_create(0, 1, &enc))) die_lib("nhw_enc_create", rc);
		if (stock_compat) nhw_enc_set_compat(enc, NHW_COMPAT_GLIBC_ONESHOT);
		dec = psnr_decoder(0, 1);
		names[0] = argv[2];
		bad = encode_host_batch(enc, dec, img, 1, quality, names);
		nhw_enc_destroy(enc);
		if (dec) nhw_dec_destroy(dec);
		free(img);
		return bad ? 1 : 0;
	}
}
