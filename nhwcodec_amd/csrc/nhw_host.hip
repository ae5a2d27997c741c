/*
 * nhw_host.hip -- the host helpers both handles share (nhw_host.h): the message of a failed HIP call, the all-or-nothing sets of device
 * buffers, the grow-only buffers, the forced slice order's mode.  No kernels.
 */
#include <stdio.h>

#include "nhw_host.h"

thread_local int nhw_slice_mode = 0;

int nhw_hip_error(std::string &err, hipError_t e, const char *file, int line, const char *call)
{
	char b[256];
	snprintf(b, sizeof b, "%s:%d %s -> %s", file, line, call, hipGetErrorString(e));
	err = b;
	return NHW_E_HIP;
}
#define NHW_ERR err

void dev_free(const DevSet &set)
{
	for (const DevBuf &b : set) { if (*b.p) (void)hipFree(*b.p); *b.p = nullptr; }
}

int dev_alloc(const DevSet &set, const char *what, int images, std::string &err)
{
	if (what) {
		size_t need = 0, free_b = 0, total_b = 0;
		for (const DevBuf &b : set) need += b.bytes;
		HIPCHK(hipMemGetInfo(&free_b, &total_b));
		if (need > free_b) {
			char m[200];
			snprintf(m, sizeof m, "%s for max_batch %d need %zu MiB (%.1f MiB per image), %zu MiB of HBM are free", what, images, need >> 20, (double)need / images / 1048576.0, free_b >> 20);
			err = m;
			return NHW_E_ARG;
		}
	}
	const int rc = [&]() -> int { for (const DevBuf &b : set) HIPCHK(hipMalloc(b.p, b.bytes)); return NHW_OK; }();
	if (rc != NHW_OK) dev_free(set);
	return rc;
}

hipError_t nhw_grow(GrowBuf &b, size_t bytes)
{
	if (b.cap >= bytes) return hipSuccess;
	nhw_grow_free(b);
	const hipError_t e = hipMalloc(&b.p, bytes);
	if (e == hipSuccess) b.cap = bytes;
	else b.p = nullptr;
	return e;
}

void nhw_grow_free(GrowBuf &b)
{
	if (b.p) (void)hipFree(b.p);
	b.p = nullptr; b.cap = 0;
}
