/*
 * nhw_tone.hip -- what makes a tone table on the device: k_hist_bytes, the byte histograms of the pictures of a table, and
 * k_tone_from_hist, the rows of nhw_tone.h's equalize and autocontrast from such histograms; and their launchers.  The table itself is applied in
 * the stores of nhw_resample.hip.
 */
#include "nhw_tensor.h"
#include "nhw_tone.h"

namespace {

constexpr int HIST_THREADS = 256;
constexpr int HIST_BANDS = 64;                  /* the most bands a picture is cut into */

/* Picture k = blockIdx.x / bands of the table (nhw_picture entries as the resamplers read them: any address and pitch, sides of 1 .. 65535, C bytes
 * a pixel), its band blockIdx.x % bands: the rows [band x rows, (band + 1) x rows) with rows = ceil(height / bands), cut at the picture's end -- the
 * workgroup makes the cut itself, the host knows no picture's size.  A picture with a zero address or a zero or oversize side, and a band below
 * the picture, count nothing and return before the barriers, the whole workgroup.  A wavefront takes a row of the band at a time, its lanes
 * consecutive bytes of the row's C W (never a byte beyond them), and counts into the workgroup's one LDS histogram of 256 C words with LDS atomic
 * adds; behind the barrier a thread adds C of the bins, those that are not zero, to hist[k][c][v] with global atomic adds.  The sums are integers:
 * the result does not depend on the order.  A picture has fewer than 2^32 pixels, so no word wraps. */
template <int C>
__global__ __launch_bounds__(HIST_THREADS) void k_hist_bytes(const nhw_picture *__restrict__ pics, int bands, uint32_t *__restrict__ hist)
{
	__shared__ uint32_t bins[256 * C];
	const int k = blockIdx.x / bands;
	const uint32_t band = (uint32_t)(blockIdx.x % bands);
	const nhw_picture p = pics[k];
	if (!p.addr || !p.width || !p.height || p.width > 65535u || p.height > 65535u) return;
	const uint32_t rows = (p.height + (uint32_t)bands - 1) / (uint32_t)bands, y0 = band * rows;
	if (y0 >= p.height) return;
	const uint32_t y1 = p.height - y0 < rows ? p.height : y0 + rows, nb = C * p.width;
	for (uint32_t i = threadIdx.x; i < 256u * C; i += HIST_THREADS) bins[i] = 0;
	__syncthreads();
	for (uint32_t y = y0 + (threadIdx.x >> 6); y < y1; y += HIST_THREADS >> 6) {
		const uint8_t *row = reinterpret_cast<const uint8_t *>(p.addr + (uint64_t)y * p.pitch);
		for (uint32_t i = threadIdx.x & 63u; i < nb; i += 64) atomicAdd(&bins[256u * (i % C) + row[i]], 1u);
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < 256u * C; i += HIST_THREADS)
		if (bins[i]) atomicAdd(&hist[(size_t)k * (256 * C) + i], bins[i]);
}

/* A wavefront a (sample, channel): blockIdx.x = k C + ch, lane l holds the bins 4 l .. 4 l + 3 of hist[k][ch].  ops[k] (uniform) says what becomes of
 * tones[k].t[ch]: NHW_TONE_EQUALIZE or NHW_TONE_AUTOCONTRAST the rule of nhw_tone.h, anything else nothing at all -- the row keeps its bytes.  The
 * sums a row needs come from the wavefront: an inclusive scan of the lanes' sums (64 bits wide) for the counts in front of a bin and the total,
 * the highest non-empty bin with its count as the maximum of (bin + 1) << 32 | count, the lowest as a minimum.  A lane writes its four bytes. */
template <int C>
__global__ __launch_bounds__(64) void k_tone_from_hist(const uint32_t *__restrict__ hist, const uint8_t *__restrict__ ops, nhw_tone_table *__restrict__ tones)
{
	const int k = blockIdx.x / C, ch = blockIdx.x % C;
	const uint32_t op = ops[k], lane = threadIdx.x;
	if (op != NHW_TONE_EQUALIZE && op != NHW_TONE_AUTOCONTRAST) return;
	const uint32_t *h = hist + ((size_t)k * C + ch) * 256 + 4 * lane;
	uint32_t v[4];
	unsigned long long sum = 0, top = 0;
	uint32_t lo = 256;
#pragma unroll
	for (uint32_t j = 0; j < 4; j++) {
		v[j] = h[j];
		sum += v[j];
		if (v[j]) {
			top = (unsigned long long)(4 * lane + j + 1) << 32 | v[j];
			if (lo == 256) lo = 4 * lane + j;
		}
	}
	unsigned long long upto = sum;
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned long long o = __shfl_up(upto, d, 64);
		if (lane >= (uint32_t)d) upto += o;
	}
	const unsigned long long total = __shfl(upto, 63, 64);
	for (int d = 32; d; d >>= 1) {
		const unsigned long long o = __shfl_xor(top, d, 64);
		const uint32_t l = __shfl_xor(lo, d, 64);
		top = o > top ? o : top;
		lo = l < lo ? l : lo;
	}
	uint8_t *row = &tones[k].t[ch][4 * lane];
	if (op == NHW_TONE_EQUALIZE) {
		const uint64_t step = nhw_tone_equalize_step(total, top & 0xFFFFFFFFull);
		uint64_t before = upto - sum;
#pragma unroll
		for (uint32_t j = 0; j < 4; j++) {
			row[j] = step ? nhw_tone_equalize_at(4 * lane + j, before, step) : (uint8_t)(4 * lane + j);
			before += v[j];
		}
	} else {
		const uint32_t hi = top ? (uint32_t)(top >> 32) - 1 : 0;
#pragma unroll
		for (uint32_t j = 0; j < 4; j++) row[j] = lo < hi ? nhw_tone_autocontrast_at(4 * lane + j, lo, hi) : (uint8_t)(4 * lane + j);
	}
}

} /* namespace */

/* The band rule, resample_bands' in small: some 8192 workgroups in all where the pictures are few, one band a picture where they are many, never
 * more than HIST_BANDS; a band's rows are the kernel's to cut.  The histograms are zeroed on the stream first, so the call overwrites. */
hipError_t nhw_launch_hist(const nhw_picture *d_pics, int n, int channels, uint32_t *d_hist, hipStream_t s)
{
	if (!d_pics || !d_hist || n < 1 || n > (1 << 24) || (channels != 3 && channels != 1)) return hipErrorInvalidValue;
	int bands = (8192 + n - 1) / n;
	if (bands > HIST_BANDS) bands = HIST_BANDS;                         /* 1 .. 64: n * bands is below 2^31 */
	const hipError_t e = hipMemsetAsync(d_hist, 0, (size_t)n * channels * 256 * sizeof(uint32_t), s);
	if (e != hipSuccess) return e;
	if (channels == 3) k_hist_bytes<3><<<n * bands, HIST_THREADS, 0, s>>>(d_pics, bands, d_hist);
	else k_hist_bytes<1><<<n * bands, HIST_THREADS, 0, s>>>(d_pics, bands, d_hist);
	return hipGetLastError();
}

hipError_t nhw_launch_tone_from_hist(const uint32_t *d_hist, int n, int channels, const uint8_t *d_ops, nhw_tone_table *d_tones, hipStream_t s)
{
	if (!d_hist || !d_ops || !d_tones || n < 1 || n > (1 << 24) || (channels != 3 && channels != 1)) return hipErrorInvalidValue;
	if (channels == 3) k_tone_from_hist<3><<<n * 3, 64, 0, s>>>(d_hist, d_ops, d_tones);
	else k_tone_from_hist<1><<<n, 64, 0, s>>>(d_hist, d_ops, d_tones);
	return hipGetLastError();
}
