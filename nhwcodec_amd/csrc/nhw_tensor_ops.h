/*
 * nhw_tensor_ops.h -- the store policies of the full-file decode with the per-sample operations (the rule is in
 * include/nhw_hip.h): mirror, colour map, tone table, then the format's own store.  What k_dec_final and k_dec_scaled (nhw_dec.hip) take as their
 * store in a call of nhw_dec_batch_device_tensor_ops / nhw_dec_batch_device_grey_ops that has at least one table.
 *
 * The three tables are kernel arguments behind the format's, each null for "the call has none": uniform pointers, tested in uniform branches, so
 * that there is one form a dtype and layout, not eight.  A workgroup works on one file.  Its `begin` reads the file's flag byte and the map's
 * sixteen words once (a uniform address: the words are scalar loads and live in scalar registers), refuses a map that is not nhw_colour_within
 * (the workgroup then stores nothing), and copies the file's tone table into LDS, in front of a barrier of the kernel.
 */
#ifndef NHW_TENSOR_OPS_H
#define NHW_TENSOR_OPS_H

#include "nhw_tensor.h"
#include "nhw_colour.h"
#include "nhw_tone.h"
#include "nhw_grey.h"
#include "nhw_reverse.h"

/* (the device tables of a call, NhwOpsArgs, entry i for file i: nhw_tensor.h) */

/* bit 0 of the file's flag byte, as a scalar: one byte load a workgroup */
__device__ __forceinline__ bool nhw_ops_mirror(const uint8_t *flags, int img)
{
	return flags && (__builtin_amdgcn_readfirstlane((int)flags[img]) & 1);
}

/* NhwStoreTensor<DT, CHW> behind the three operations.  The kernel gives `begin` 768 bytes of LDS (`lds`) for the tone table; a thread's N pixels are
 * reversed in their packed dwords where the file is mirrored (one uniform branch) and go out as piece S / N - 1 - c, then every pixel's bytes take
 * the map (twelve scalar operands) and three byte reads from LDS. */
template <int DT, int CHW> struct NhwStoreTensorOps {
	static constexpr int dtype = DT, layout = CHW, lds = 768;
	static constexpr bool bytes = false, grey = false, ops = true;
	NhwTensorArgs a;
	NhwOpsArgs o;
	/* what `begin` leaves for the workgroup's puts (the kernels hold their policy as a constant, hence mutable) */
	mutable nhw_colour_map cm;            /* the file's map, where the call has maps */
	mutable const uint8_t *tone;          /* the file's table in LDS, or null */
	mutable bool mirror;
	__device__ __forceinline__ bool begin(int img, int tid, uint8_t *tab) const
	{
		mirror = nhw_ops_mirror(o.flags, img);
		if (o.maps) {
			cm = o.maps[img];
			if (!nhw_colour_within(cm)) return false;
		}
		tone = nullptr;
		if (o.tones) {
			const uint8_t *t = &o.tones[img].t[0][0];                         /* (a table has no alignment: a byte a thread at a time) */
			for (int i = tid; i < 768; i += 256) tab[i] = t[i];
			tone = tab;
		}
		return true;
	}
	template <int S, int N> __device__ __forceinline__ void put(uint8_t *out, int img, int r, int c, const uint32_t *w) const
	{
		constexpr int K = 3 * N / 4;
		uint32_t v[K];
		if (mirror) { nhw_reverse_packed<N, 3>(w, v); c = nhw_mirror_piece(S, N, c); }
		else {
#pragma unroll
			for (int k = 0; k < K; k++) v[k] = w[k];
		}
		if (o.maps || tone) {                                               /* the pixels' bytes taken apart, through map and table, and packed again */
			uint32_t b[N][3];
#pragma unroll
			for (int px = 0; px < N; px++)
#pragma unroll
				for (int ch = 0; ch < 3; ch++) b[px][ch] = (v[(3 * px + ch) >> 2] >> (8 * ((3 * px + ch) & 3))) & 0xFFu;
			if (o.maps) {
#pragma unroll
				for (int px = 0; px < N; px++) nhw_colour_apply<3>(cm, b[px]);
			}
			if (tone) {
#pragma unroll
				for (int px = 0; px < N; px++) nhw_tone_apply<3>(tone, b[px]);
			}
#pragma unroll
			for (int k = 0; k < K; k++) v[k] = 0;
#pragma unroll
			for (int px = 0; px < N; px++)
#pragma unroll
				for (int ch = 0; ch < 3; ch++) v[(3 * px + ch) >> 2] |= b[px][ch] << (8 * ((3 * px + ch) & 3));
		}
		const NhwStoreTensor<DT, CHW> plain{ a };
		plain.template put<S, N, 1>(out, img, r, c, v);
	}
};

/* NhwStoreGrey<DT> behind the three operations.  With one channel the grey table of the file's quality, the map and the tone table are all functions
 * of one byte: the workgroup's 256 threads make their composition, tone[map[grey_q[y]]], in the 256 bytes of LDS where the kernel keeps its grey
 * table (`table`, in place of grey_table_fill), so a pixel costs the one table read it costs a grey decode below quality 20 and no LDS is added.
 * `lut`: whether the kernel reads the table at all -- as ever below quality 20, and at every quality once there is a map or a tone table.  What
 * is left for `put` is the mirror. */
template <int DT> struct NhwStoreGreyOps {
	static constexpr int dtype = DT, lds = 0;
	static constexpr bool bytes = false, grey = true, ops = true;
	NhwGreyArgs a;
	NhwOpsArgs o;
	mutable nhw_colour_map cm;
	mutable bool mirror;
	__device__ __forceinline__ bool begin(int img, int, uint8_t *) const
	{
		mirror = nhw_ops_mirror(o.flags, img);
		if (o.maps) {
			cm = o.maps[img];
			if (!nhw_colour_within(cm)) return false;
		}
		return true;
	}
	__device__ __forceinline__ bool lut(int q) const { return q < 20 || o.maps || o.tones; }
	__device__ __forceinline__ void table(uint8_t *tab, int img, int q, int tid) const
	{
		if (!lut(q)) return;
		uint32_t b = (uint32_t)nhw_grey_value(q, tid);
		if (o.maps) nhw_colour_apply<1>(cm, &b);
		if (o.tones) nhw_tone_apply<1>(&o.tones[img].t[0][0], &b);
		tab[tid] = (uint8_t)b;
	}
	template <int S, int N> __device__ __forceinline__ void put(uint8_t *out, int img, int r, int c, const uint32_t *w) const
	{
		const NhwStoreGrey<DT> plain{ a };
		if (mirror) {
			uint32_t v[N / 4];
			nhw_reverse_packed<N, 1>(w, v);
			plain.template put<S, N, 1>(out, img, r, nhw_mirror_piece(S, N, c), v);
		}
		else plain.template put<S, N, 1>(out, img, r, c, w);
	}
};

/* f(the policy object) for a checked format, as nhw_with_tensor_store and nhw_with_grey_store */
template <class F> inline void nhw_with_tensor_ops_store(int dtype, int layout, const NhwTensorArgs &a, const NhwOpsArgs &o, F &&f)
{
	switch (2 * dtype + layout) {
	case 2 * NHW_T_U8 + NHW_T_HWC: f(NhwStoreTensorOps<NHW_T_U8, NHW_T_HWC>{ a, o }); break;
	case 2 * NHW_T_U8 + NHW_T_CHW: f(NhwStoreTensorOps<NHW_T_U8, NHW_T_CHW>{ a, o }); break;
	case 2 * NHW_T_F16 + NHW_T_HWC: f(NhwStoreTensorOps<NHW_T_F16, NHW_T_HWC>{ a, o }); break;
	case 2 * NHW_T_F16 + NHW_T_CHW: f(NhwStoreTensorOps<NHW_T_F16, NHW_T_CHW>{ a, o }); break;
	case 2 * NHW_T_BF16 + NHW_T_HWC: f(NhwStoreTensorOps<NHW_T_BF16, NHW_T_HWC>{ a, o }); break;
	case 2 * NHW_T_BF16 + NHW_T_CHW: f(NhwStoreTensorOps<NHW_T_BF16, NHW_T_CHW>{ a, o }); break;
	case 2 * NHW_T_F32 + NHW_T_HWC: f(NhwStoreTensorOps<NHW_T_F32, NHW_T_HWC>{ a, o }); break;
	default: f(NhwStoreTensorOps<NHW_T_F32, NHW_T_CHW>{ a, o }); break;
	}
}
template <class F> inline void nhw_with_grey_ops_store(int dtype, const NhwGreyArgs &a, const NhwOpsArgs &o, F &&f)
{
	switch (dtype) {
	case NHW_T_U8: f(NhwStoreGreyOps<NHW_T_U8>{ a, o }); break;
	case NHW_T_F16: f(NhwStoreGreyOps<NHW_T_F16>{ a, o }); break;
	case NHW_T_BF16: f(NhwStoreGreyOps<NHW_T_BF16>{ a, o }); break;
	default: f(NhwStoreGreyOps<NHW_T_F32>{ a, o }); break;
	}
}

#endif
