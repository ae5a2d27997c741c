/*
 * asan_dec.c -- the oracle's decoder on one file, for the sanitizer build (make -C oracle asan -> oracle/_asan/nhwo_dec_asan).
 * TEST INFRASTRUCTURE ONLY (tests/nhw_surgery.py): the file sits in a heap block of exactly its length, so a read behind its end is reported.
 *
 *   nhwo_dec_asan FILE   exit 0: decoded, stdout = one byte of quality + the 786432 pixel bytes
 *                        exit 3: the oracle refused the file
 *                        anything else: a sanitizer report on stderr (the build stops at the first one)
 */
#include <stdio.h>
#include <stdlib.h>
#include "nhwo.h"

int main(int argc, char **argv)
{
	FILE *fp;
	long n;
	uint8_t *nhw, *px, qb;
	int q = 0, rc;
	if (argc != 2 || !(fp = fopen(argv[1], "rb"))) return 2;
	fseek(fp, 0, SEEK_END); n = ftell(fp); fseek(fp, 0, SEEK_SET);
	nhw = (uint8_t *)malloc((size_t)n ? (size_t)n : 1);
	px = (uint8_t *)malloc(512 * 512 * 3);
	if (!nhw || !px || fread(nhw, 1, (size_t)n, fp) != (size_t)n) return 2;
	fclose(fp);
	rc = nhwo_decode(nhw, (size_t)n, px, &q);
	if (!rc) {
		qb = (uint8_t)q;
		fwrite(&qb, 1, 1, stdout);
		fwrite(px, 1, 512 * 512 * 3, stdout);
	}
	free(nhw); free(px);
	return rc ? 3 : 0;
}
