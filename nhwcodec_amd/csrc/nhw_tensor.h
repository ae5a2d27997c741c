/*
 * nhw_tensor.h -- the tensor formats of a decode and of an encode (section 17; nhw_tensor_format in include/nhw_hip.h):
 * the value rule of each direction, the check of a format, the store shapes of the decoder's last kernels (nhw_dec.hip), the pixel store
 * of the pointwise kernel (nhw_picture.hip) and the resamplers (nhw_resample.hip), and the load shapes of the encoder's conversion kernels (nhw_picture.hip).
 *
 * Value rule of a decode: the element for byte b of output channel c is fmaf((float)b, scale[c], bias[c]) in single precision, rounded once, to
 * nearest even, to the output type; NHW_T_U8 passes the byte on.  The fma is explicit (the library builds with -ffp-contract=off).  That rounding
 * comes after the fma's own, of the exact b * scale + bias to float32: two roundings in all, both to nearest even, and the two-step result is
 * normative (it is not always the exact sum rounded once to the type).  Subnormals of float32 and of the output type are kept, what lies beyond
 * the type's range is an infinity.  Zero's sign is the fma's: a nonzero value that rounds to zero keeps its sign at either rounding; an exact
 * sum of zero is +0, unless the product (b = 0 or scale 0, with a scale below zero or -0) and the bias are both -0, which is -0.
 * Value rule of an encode: element x of tensor channel c, widened exactly to float, gives y = fmaf(x, scale[c], bias[c]); the byte is 0 for a
 * NaN, else rint(y), ties to even, clamped to 0 .. 255 (the clamp in float, before the conversion); NHW_T_U8 passes the byte on.
 */
#ifndef NHW_TENSOR_H
#define NHW_TENSOR_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string>
#include <type_traits>

#include "../../include/nhw_hip.h"

/* what a kernel gets of a format: dtype and layout are template parameters, the rest are kernel arguments (six floats and two flags, uniform) */
struct NhwTensorArgs { float scale[3], bias[3]; int rgb, flip; };

/* NHW_OK and the kernel's view of the format, or NHW_E_ARG with the reason in err.  grey: the caller is the grey decode or a one-channel entry (section 23), which
 * takes NHW_T_GREY and nothing else; every other caller takes BGR and RGB and nothing else */
inline int nhw_tensor_format_check(const nhw_tensor_format *f, NhwTensorArgs *a, std::string &err, bool grey = false)
{
	if (!f) { err = "bad argument"; return NHW_E_ARG; }
	if (grey && (f->channels == NHW_T_BGR || f->channels == NHW_T_RGB)) { err = "tensor format: a grey decode takes NHW_T_GREY, not NHW_T_BGR or NHW_T_RGB"; return NHW_E_ARG; }
	if (f->dtype < NHW_T_U8 || f->dtype > NHW_T_F32 || (f->layout != NHW_T_HWC && f->layout != NHW_T_CHW) || (grey ? f->channels != NHW_T_GREY : f->channels != NHW_T_BGR && f->channels != NHW_T_RGB) ||
	    (f->rows != NHW_T_ROWS_FILE && f->rows != NHW_T_ROWS_REVERSED)) { err = "tensor format: unknown dtype, layout, channels or rows value"; return NHW_E_ARG; }
	if (f->reserved) { err = "tensor format: the reserved word must be 0"; return NHW_E_ARG; }
	for (int c = 0; c < 3; c++) {
		if (!isfinite(f->scale[c]) || !isfinite(f->bias[c])) { err = "tensor format: scale and bias must be finite"; return NHW_E_ARG; }
		if (f->dtype == NHW_T_U8 && (f->scale[c] != 1.0f || f->bias[c] != 0.0f)) { err = "tensor format: NHW_T_U8 takes scale 1 and bias 0 only"; return NHW_E_ARG; }
		a->scale[c] = f->scale[c]; a->bias[c] = f->bias[c];
	}
	a->rgb = f->channels == NHW_T_RGB; a->flip = f->rows == NHW_T_ROWS_REVERSED;
	return NHW_OK;
}
/* the tensors of one size that a resampling or warping call makes, as its launcher takes them */
struct NhwTensorOut { uint32_t w, h; int dtype, layout; NhwTensorArgs a; };
/* the per-sample tables of a call, entry i for sample i, each null for "none": the flag bytes (bit 0: mirror left-right), the colour maps (DESIGN.md
 * section 24) and the tone tables (section 25).  What the samplers' call (NhwSampleCall below) and the decode's store policies (nhw_tensor_ops.h) share */
struct NhwOpsArgs { const uint8_t *flags; const nhw_colour_map *maps; const nhw_tone_table *tones; };
/* ... and what every such entry checks of them, in this order: the sides, 1 .. 4096 each (the message names the entry), then the format -- as a
 * one-channel entry where `grey` is set */
inline int nhw_tensor_out_check(const char *who, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *f, NhwTensorOut *o, std::string &err, bool grey = false)
{
	if (out_width < 1 || out_height < 1 || out_width > 4096u || out_height > 4096u) { err = std::string(who) + ": an output side outside 1 .. 4096"; return NHW_E_ARG; }
	if (const int rc = nhw_tensor_format_check(f, &o->a, err, grey)) return rc;
	o->w = out_width; o->h = out_height; o->dtype = f->dtype; o->layout = f->layout;
	return NHW_OK;
}
inline bool nhw_tensor_format_is_bytes(const nhw_tensor_format *f)    /* what the byte entry points write */
{
	return f->dtype == NHW_T_U8 && f->layout == NHW_T_HWC && f->channels == NHW_T_BGR && f->rows == NHW_T_ROWS_FILE;
}

/* an element of a dtype: its size, and the unsigned integer that holds its bits */
template <int DT> struct NhwElem {
	static constexpr int bytes = DT == NHW_T_U8 ? 1 : DT == NHW_T_F32 ? 4 : 2;
	using type = typename std::conditional<DT == NHW_T_U8, uint8_t, typename std::conditional<DT == NHW_T_F32, uint32_t, uint16_t>::type>::type;
};

/* the element of byte b, in the low bits of a dword */
template <int DT> __device__ __forceinline__ uint32_t nhw_tensor_elem(uint32_t b, float scale, float bias)
{
	if (DT == NHW_T_U8) return b;
	const float x = __fmaf_rn((float)b, scale, bias);
	if (DT == NHW_T_F32) return __float_as_uint(x);
	if (DT == NHW_T_F16) {
		/* the fma's float32 result has to exist before it is converted: left to itself the compiler folds fma and conversion into
		 * v_fma_mixlo_f16, which rounds the exact sum ONCE, to float16 -- not the rule (scale 1 + 2^-11, bias 2^-40, b = 1 would give
		 * 0x3C01 for 0x3C00).  The empty asm takes x in a vector register and hands it back; it emits nothing */
		float y = x;
		asm("" : "+v"(y));
		return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)y);                                /* v_cvt_f16_f32: to nearest even, f16 denormals kept */
	}
	/* bfloat16: the float's upper half, rounded to nearest even on the lower.  x is finite or an infinity the fma overflowed to (b, scale, bias are
	 * finite), never a NaN, and an infinity's lower half is 0: the integer form is exact for every value that occurs */
	const uint32_t u = __float_as_uint(x);
	return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

/* One pixel, its bytes b[0 .. 2] as the byte path holds them (B, G, R), to row rr, column c of the h x w tensor at out: the channel order, the
 * value rule and three element stores -- in CHW a plane apart, in HWC side by side.  What the kernels that make a pixel at a time share (the
 * pointwise k_bytes_to_tensor, the resamplers of nhw_resample.hip); the caller has turned the row (a.flip) and, where it mirrors, the column. */
template <int DT, int CHW>
__device__ __forceinline__ void nhw_store_pixel(typename NhwElem<DT>::type *out, size_t h, size_t w, size_t rr, size_t c, const uint32_t *b, const NhwTensorArgs &a)
{
	using E = typename NhwElem<DT>::type;
	const E e0 = (E)nhw_tensor_elem<DT>(a.rgb ? b[2] : b[0], a.scale[0], a.bias[0]);
	const E e1 = (E)nhw_tensor_elem<DT>(b[1], a.scale[1], a.bias[1]);
	const E e2 = (E)nhw_tensor_elem<DT>(a.rgb ? b[0] : b[2], a.scale[2], a.bias[2]);
	if (CHW) { E *o = out + rr * w + c; o[0] = e0; o[h * w] = e1; o[2 * h * w] = e2; }
	else { E *o = out + (rr * w + c) * 3; o[0] = e0; o[1] = e1; o[2] = e2; }
}

/* K dwords to p in vectors of V dwords (p aligned to 4 V bytes; 12-byte vectors to 4): plain vector stores.  The 16- and 8-byte ones are native
 * vector types, one store instruction each as written here: as structs of dwords the compiler takes them apart and groups the dwords anew. */
typedef uint32_t nhw_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t nhw_u32x2 __attribute__((ext_vector_type(2)));
template <int K, int V> __device__ __forceinline__ void nhw_store_words(uint8_t *p, const uint32_t *w)
{
	static_assert(K % V == 0 && V >= 1 && V <= 4, "whole vectors");
#pragma unroll
	for (int k = 0; k < K; k += V) {
		if (V == 4) *reinterpret_cast<nhw_u32x4 *>(p + 4 * k) = (nhw_u32x4){ w[k], w[k + 1], w[k + 2], w[k + 3] };
		else if (V == 3) *reinterpret_cast<uint3 *>(p + 4 * k) = make_uint3(w[k], w[k + 1], w[k + 2]);
		else if (V == 2) *reinterpret_cast<nhw_u32x2 *>(p + 4 * k) = (nhw_u32x2){ w[k], w[k + 1] };
		else *reinterpret_cast<uint32_t *>(p + 4 * k) = w[k];
	}
}

/* N elements (in the low bits of e[]) packed into N * bytes / 4 dwords */
template <int DT, int N> __device__ __forceinline__ void nhw_pack_elems(const uint32_t *e, uint32_t *w)
{
	constexpr int PER = 4 / NhwElem<DT>::bytes;
	static_assert(N % PER == 0, "whole dwords");
#pragma unroll
	for (int k = 0; k < N / PER; k++) {
		uint32_t v = 0;
#pragma unroll
		for (int j = 0; j < PER; j++) v |= e[PER * k + j] << (8 * NhwElem<DT>::bytes * j);
		w[k] = v;
	}
}

/* The store of N = 8 or 4 pixels of one row of an S x S picture, columns N c .. N c + N - 1 of byte-path row r of file img: `w` holds their 3 N bytes
 * as the byte path stores them (B, G, R a pixel).  The thread owns
 *   CHW: N consecutive elements in each of the three planes -- N * bytes each: 32 (two 16-byte stores), 16 (one), 8 or 4 bytes;
 *   HWC: 3 N consecutive elements -- 96, 48 (16-byte stores), 24 (8-byte stores) or 12 bytes (one store).
 * Consecutive lanes take consecutive pieces either way.  Every address is a multiple of its store's size when `out` is 16-byte aligned (12-byte
 * stores: of 4).
 * WHO changes nothing in `put`; it only gives a second caller an instantiation of its own.  The policies of nhw_tensor_ops.h end in this `put` with a
 * piece c that is not the kernel's.  The helpers have internal linkage on the device, and the compiler's interprocedural value propagation runs before
 * it inlines them: with both callers on ONE instantiation it loses what it knows of c at the kernels' call (c < S / N), and ten of the kernels that
 * were here before came out with other address arithmetic.  With WHO = 1 for the other caller they are the code they were. */
template <int DT, int CHW> struct NhwStoreTensor {
	static constexpr int dtype = DT, layout = CHW, lds = 0;             /* lds: the bytes of LDS a policy asks of the kernel for itself; ops: nhw_tensor_ops.h */
	static constexpr bool bytes = false, grey = false, ops = false;
	NhwTensorArgs a;
	template <int S, int N, int WHO = 0 /* the caller: see above NhwStoreTensor */> __device__ __forceinline__ void put(uint8_t *out, int img, int r, int c, const uint32_t *w) const
	{
		constexpr int EB = NhwElem<DT>::bytes;
		const int rr = a.flip ? S - 1 - r : r;
		uint32_t e[3][N];                                                   /* [output channel][pixel] */
#pragma unroll
		for (int px = 0; px < N; px++) {
			uint32_t b[3];
#pragma unroll
			for (int ch = 0; ch < 3; ch++) b[ch] = (w[(3 * px + ch) >> 2] >> (8 * ((3 * px + ch) & 3))) & 0xFFu;
			e[0][px] = nhw_tensor_elem<DT>(a.rgb ? b[2] : b[0], a.scale[0], a.bias[0]);
			e[1][px] = nhw_tensor_elem<DT>(b[1], a.scale[1], a.bias[1]);
			e[2][px] = nhw_tensor_elem<DT>(a.rgb ? b[0] : b[2], a.scale[2], a.bias[2]);
		}
		uint8_t *base = out + (size_t)img * (3 * S * S * EB);
		if (CHW) {
			constexpr int K = N * EB / 4;                                   /* dwords a plane: 8, 4, 2 or 1 */
#pragma unroll
			for (int oc = 0; oc < 3; oc++) {
				uint32_t v[K];
				nhw_pack_elems<DT, N>(e[oc], v);
				nhw_store_words<K, (K > 4 ? 4 : K)>(base + ((size_t)oc * S * S + (size_t)rr * S + N * c) * EB, v);
			}
		} else {
			constexpr int K = 3 * N * EB / 4;                               /* 24, 12, 6 or 3 dwords */
			uint32_t il[3 * N], v[K];
#pragma unroll
			for (int px = 0; px < N; px++) { il[3 * px] = e[0][px]; il[3 * px + 1] = e[1][px]; il[3 * px + 2] = e[2][px]; }
			nhw_pack_elems<DT, 3 * N>(il, v);
			nhw_store_words<K, (K % 4 == 0 ? 4 : K == 6 ? 2 : 3)>(base + ((size_t)rr * S + N * c) * (3 * EB), v);
		}
	}
};

/* The one-channel store: N = 16 or 8 grey bytes of one row of an S x S picture, columns N c .. N c + N - 1 of byte-path row r of
 * file img, N / 4 dwords in `w`, under the value rule with scale[0] and bias[0].  With one channel HWC and CHW are the same memory, so the layout is
 * no parameter.  The thread owns N consecutive elements, N * bytes: 64 (four 16-byte stores), 32, 16 (one) or 8 bytes; consecutive lanes take
 * consecutive pieces, and every address is a multiple of its store's size when `out` is 16-byte aligned.  `slice` is no part of the format: the
 * slice of the launch (nhw_host.h) for a kernel that has no argument of its own for it, -1 in production. */
struct NhwGreyArgs { float scale, bias; int flip, slice; };
template <int DT> struct NhwStoreGrey {
	static constexpr int dtype = DT, lds = 0;
	static constexpr bool bytes = false, grey = true, ops = false;
	NhwGreyArgs a;
	template <int S, int N, int WHO = 0 /* the caller: see above NhwStoreTensor */> __device__ __forceinline__ void put(uint8_t *out, int img, int r, int c, const uint32_t *w) const
	{
		constexpr int EB = NhwElem<DT>::bytes, K = N * EB / 4;              /* dwords: 16, 8, 4 or 2 */
		const int rr = a.flip ? S - 1 - r : r;
		uint32_t e[N], v[K];
#pragma unroll
		for (int px = 0; px < N; px++) e[px] = nhw_tensor_elem<DT>((w[px >> 2] >> (8 * (px & 3))) & 0xFFu, a.scale, a.bias);
		nhw_pack_elems<DT, N>(e, v);
		nhw_store_words<K, (K > 4 ? 4 : K)>(out + ((size_t)img * S * S + (size_t)rr * S + N * c) * EB, v);
	}
};
/* f(NhwStoreGrey<dtype>{ a }) for a checked format */
template <class F> inline void nhw_with_grey_store(int dtype, const NhwGreyArgs &a, F &&f)
{
	switch (dtype) {
	case NHW_T_U8: f(NhwStoreGrey<NHW_T_U8>{ a }); break;
	case NHW_T_F16: f(NhwStoreGrey<NHW_T_F16>{ a }); break;
	case NHW_T_BF16: f(NhwStoreGrey<NHW_T_BF16>{ a }); break;
	default: f(NhwStoreGrey<NHW_T_F32>{ a }); break;
	}
}

/* ------------------------------------------------------------------------------------------------ the other direction */
/* the element whose bits are the low bits of e, widened exactly to float: IEEE half with its denormals (v_cvt_f32_f16), bfloat16 as bits << 16 */
template <int DT> __device__ __forceinline__ float nhw_tensor_widen(uint32_t e)
{
	if (DT == NHW_T_F32) return __uint_as_float(e);
	if (DT == NHW_T_F16) return (float)__builtin_bit_cast(_Float16, (uint16_t)e);
	if (DT == NHW_T_BF16) return __uint_as_float(e << 16);
	return (float)(e & 0xFFu);
}
/* the byte of element e: one fma, the clamp in float (a NaN fails the first comparison and gives 0), then the rounding to nearest even; what
 * reaches rintf lies in [0, 255] */
template <int DT> __device__ __forceinline__ uint32_t nhw_tensor_byte(uint32_t e, float scale, float bias)
{
	if (DT == NHW_T_U8) return e & 0xFFu;
	const float y = __fmaf_rn(nhw_tensor_widen<DT>(e), scale, bias);
	const float c = y > 0.0f ? (y < 255.0f ? y : 255.0f) : 0.0f;
	return (uint32_t)rintf(c);
}

/* BYTES (a multiple of 4) from address p to d[], p a multiple of ALIGN (a power of two, 1 .. 16, known when compiling): the widest vector
 * loads that BYTES and ALIGN both allow (12 bytes on a 4-byte alignment: one 12-byte load), as native vector types; below 4 bytes of alignment, shorts or bytes put together.  Reads [p, p + BYTES)
 * and nothing else. */
template <int BYTES, int ALIGN> __device__ __forceinline__ void nhw_load_words(const uint8_t *p, uint32_t *d)
{
	static_assert(BYTES % 4 == 0, "whole dwords");
	constexpr int V = ALIGN >= 16 && BYTES % 16 == 0 ? 4 : ALIGN >= 8 && BYTES % 8 == 0 ? 2 : ALIGN >= 4 && BYTES == 12 ? 3 : 1;
#pragma unroll
	for (int k = 0; k < BYTES / 4; k += V) {
		if (ALIGN >= 4) {
			if (V == 3) { const uint3 v = *reinterpret_cast<const uint3 *>(p); d[0] = v.x; d[1] = v.y; d[2] = v.z; }
			else if (V == 4) { const nhw_u32x4 v = *reinterpret_cast<const nhw_u32x4 *>(p + 4 * k); d[k] = v.x; d[k + 1] = v.y; d[k + 2] = v.z; d[k + 3] = v.w; }
			else if (V == 2) { const nhw_u32x2 v = *reinterpret_cast<const nhw_u32x2 *>(p + 4 * k); d[k] = v.x; d[k + 1] = v.y; }
			else d[k] = *reinterpret_cast<const uint32_t *>(p + 4 * k);
		} else if (ALIGN == 2) {
			const uint16_t *h = reinterpret_cast<const uint16_t *>(p + 4 * k);
			d[k] = (uint32_t)h[0] | (uint32_t)h[1] << 16;
		} else {
			const uint8_t *b = reinterpret_cast<const uint8_t *>(p + 4 * k);
			d[k] = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
		}
	}
}
/* the same with the alignment looked at when running (p a multiple of the element size EB at least): the crop views of the picture kernel */
template <int BYTES, int EB> __device__ __forceinline__ void nhw_load_words_any(const uint8_t *q, uint32_t *d)
{
	const uintptr_t p = (uintptr_t)q;
	if (BYTES % 16 == 0 && !(p & 15)) nhw_load_words<BYTES, 16>(q, d);
	else if (BYTES % 8 == 0 && !(p & 7)) nhw_load_words<BYTES, 8>(q, d);
	else if (EB == 4 || !(p & 3)) nhw_load_words<BYTES, 4>(q, d);
	else if (EB == 2 || !(p & 1)) nhw_load_words<BYTES, 2>(q, d);
	else nhw_load_words<BYTES, 1>(q, d);
}
/* element i of the elements packed in d[] */
template <int DT> __device__ __forceinline__ uint32_t nhw_unpack_elem(const uint32_t *d, int i)
{
	constexpr int EB = NhwElem<DT>::bytes, PER = 4 / EB;
	return EB == 4 ? d[i] : (d[i / PER] >> (8 * EB * (i % PER))) & (EB == 2 ? 0xFFFFu : 0xFFu);
}
/* e[c][px]: the elements of N pixels by TENSOR channel -> their 3 N bytes as the byte path holds them (B, G, R a pixel), 3 N / 4 dwords */
template <int DT, int N> __device__ __forceinline__ void nhw_pixels_to_bytes(const uint32_t (*e)[N], const NhwTensorArgs &a, uint32_t *w)
{
	static_assert(N % 4 == 0, "whole dwords");
	uint32_t b[3 * N];
#pragma unroll
	for (int px = 0; px < N; px++) {
		const uint32_t t0 = nhw_tensor_byte<DT>(e[0][px], a.scale[0], a.bias[0]), t1 = nhw_tensor_byte<DT>(e[1][px], a.scale[1], a.bias[1]),
		               t2 = nhw_tensor_byte<DT>(e[2][px], a.scale[2], a.bias[2]);
		b[3 * px] = a.rgb ? t2 : t0; b[3 * px + 1] = t1; b[3 * px + 2] = a.rgb ? t0 : t2;
	}
#pragma unroll
	for (int k = 0; k < 3 * N / 4; k++) w[k] = b[4 * k] | b[4 * k + 1] << 8 | b[4 * k + 2] << 16 | b[4 * k + 3] << 24;
}

/* f(NhwStoreTensor<dtype, layout>{ a }) for a checked format */
template <class F> inline void nhw_with_tensor_store(int dtype, int layout, const NhwTensorArgs &a, F &&f)
{
	switch (2 * dtype + layout) {
	case 2 * NHW_T_U8 + NHW_T_HWC: f(NhwStoreTensor<NHW_T_U8, NHW_T_HWC>{ a }); break;
	case 2 * NHW_T_U8 + NHW_T_CHW: f(NhwStoreTensor<NHW_T_U8, NHW_T_CHW>{ a }); break;
	case 2 * NHW_T_F16 + NHW_T_HWC: f(NhwStoreTensor<NHW_T_F16, NHW_T_HWC>{ a }); break;
	case 2 * NHW_T_F16 + NHW_T_CHW: f(NhwStoreTensor<NHW_T_F16, NHW_T_CHW>{ a }); break;
	case 2 * NHW_T_BF16 + NHW_T_HWC: f(NhwStoreTensor<NHW_T_BF16, NHW_T_HWC>{ a }); break;
	case 2 * NHW_T_BF16 + NHW_T_CHW: f(NhwStoreTensor<NHW_T_BF16, NHW_T_CHW>{ a }); break;
	case 2 * NHW_T_F32 + NHW_T_HWC: f(NhwStoreTensor<NHW_T_F32, NHW_T_HWC>{ a }); break;
	default: f(NhwStoreTensor<NHW_T_F32, NHW_T_CHW>{ a }); break;
	}
}

/* nhw_picture.hip: every picture of the table to a tensor of its own size, one pass */
hipError_t nhw_launch_bytes_to_tensor(const nhw_picture *d_pics, int n_pics, int dtype, int layout, const NhwTensorArgs &a, const uint64_t *d_out_addr, hipStream_t s);
/* nhw_resample.hip: one sampling call, as it goes from a public entry to the launch.  Every picture of the table is sampled into a tensor of out.w x
 * out.h (1 .. 4096 each) at out_addr[k], with 3 bytes a pixel or, with `grey`, 1 ([out.h][out.w] elements under scale[0] and
 * bias[0]; no layout is read, and of a warp fill[0] alone).
 * Without `warps` the call resamples: under the filter NHW_FILTER_TWO_TAP (section 18), NHW_FILTER_AREA (section 19: the exact box mean along an axis
 * that shrinks, the two taps along one that does not) or NHW_FILTER_CUBIC (section 20: the Keys cubic, a = -1/2, widened with the reduction),
 * mirrored where bit 0 of ops.flags[k] is set.  An entry whose width exceeds nhw_filter_limit(filter) out.w, or its height that many out.h, stores
 * nothing (0: the two taps have no limit).
 * With `warps`, a device table of n, entry k is sampled along the tilted grid of warps[k] (section 21) under the same band rule; filter and ops.flags
 * are not read.  An entry whose warp is not nhw_warp_within stores nothing: the kernel checks it, and the host paths that know a warp refuse it
 * with the same words before they launch.
 * ops.maps and ops.tones are device tables of n, entry k for picture k, each null for "none", and choose the form of the kernel: none of them the
 * plain one, maps alone the mapped one (section 24; the rule and nhw_colour_within are in nhw_colour.h), tones the toned one (section 25; nhw_tone.h),
 * which takes the maps as well where there are some.  An entry whose map is not within the limits stores nothing: the kernel checks it, and the
 * host paths that know a map refuse it before they launch.  Every tone table is valid.
 * A further per-sample step is one more table here, one more pack in nhw_resample.hip and one more row in the entries' descriptor tables. */
inline uint32_t nhw_filter_limit(int filter) { return filter == NHW_FILTER_CUBIC ? NHW_CUBIC_MAX_REDUCTION : filter == NHW_FILTER_AREA ? NHW_AREA_MAX_REDUCTION : 0; }
__host__ __device__ inline bool nhw_warp_within(const nhw_warp &m)
{
	constexpr int32_t S = NHW_WARP_MAX_STEP << 16;
	constexpr int64_t O = 1ll << 40;
	return m.a >= -S && m.a <= S && m.b >= -S && m.b <= S && m.d >= -S && m.d <= S && m.e >= -S && m.e <= S && m.c >= -O && m.c <= O && m.f >= -O && m.f <= O;
}
struct NhwSampleCall {
	const nhw_picture *pics; int n;
	NhwTensorOut out;
	bool grey;
	int filter;
	const nhw_warp *warps;
	NhwOpsArgs ops;
	const uint64_t *out_addr;
};
hipError_t nhw_launch_sample(const NhwSampleCall &c, hipStream_t s);
/* the family of a public entry, in its row of the descriptor tables (nhw_enc_hostpath.hip, nhw_dec_hostpath.hip): colour, grey, or -- the mapped and
 * toned entries -- by the format, where one that names NHW_T_GREY makes the call the one-channel one */
enum NhwFamily { NHW_FAMILY_COLOUR, NHW_FAMILY_GREY, NHW_FAMILY_BY_FORMAT };
inline bool nhw_family_grey(NhwFamily family, const nhw_tensor_format *f) { return family == NHW_FAMILY_BY_FORMAT ? f && f->channels == NHW_T_GREY : family == NHW_FAMILY_GREY; }
/* nhw_tone.hip: the histograms of n pictures of `channels` (3 or 1) bytes a pixel, uint32 [n][channels][256], zeroed on the
 * stream and then counted; and the rows of n tone tables from such histograms under one op byte a sample */
hipError_t nhw_launch_hist(const nhw_picture *d_pics, int n, int channels, uint32_t *d_hist, hipStream_t s);
hipError_t nhw_launch_tone_from_hist(const uint32_t *d_hist, int n, int channels, const uint8_t *d_ops, nhw_tone_table *d_tones, hipStream_t s);
/* nhw_picture.hip again, the encoder's side: n 512 x 512 tensors to the byte path's pictures; the tiles [tile0, tile0 + m) of tensor pictures of any size */
hipError_t nhw_launch_tensor_to_bytes(const void *d_in, int n, int dtype, int layout, const NhwTensorArgs &a, uint8_t *d_bgr, hipStream_t s);
hipError_t nhw_launch_tile_pad_tensor(const nhw_tensor_picture *d_pics, int n_pics, int tile0, int m, int dtype, int layout, const NhwTensorArgs &a, uint8_t *d_tiles, hipStream_t s);
/* the one-channel form (section 27): n [512][512] tensors to grey pictures of 512 x 512 bytes under scale[0] and bias[0] */
hipError_t nhw_launch_tensor_to_bytes_grey(const void *d_in, int n, int dtype, const NhwTensorArgs &a, uint8_t *d_grey, hipStream_t s);

#endif
