// 2-D evaluation metrics of FIND (reference src/eval/eval_2d.py:92-121 with src/eval/eval_metrics.py:4-40): one pass over a predicted
// and a ground-truth render that forms every per-image sum PSNR_A / _B / _C, MSE, IOU and MSE_masked are made of.  The reference's
// in-place edit of the prediction under the GT's mask-out map (eval_2d.py:92-94: image := 1, mask := 0 where hidden) is applied to the
// values as they are read; nothing is written but the sums.  HBM-bound: pred + gt + two masks + hide = 33 B per RGB pixel, read once.
//
// Deterministic: the split of an image into blocks depends on (n_img, n_pix) only; a thread adds the terms of one group of pixels in
// fp32 (at most 4 pixels x C channels), carries its running sums in fp64 and the wave / block / partial reductions stay in fp64 in a
// fixed order.  No atomics.
#include "common.h"

namespace find {
namespace eval2d {

constexpr int THREADS = 256;
constexpr int TARGET_BLOCKS = 2048;   // whole grid: ~8 blocks per CU, grid-strided beyond that

// blocks per image: enough to fill the chip over all images, at most one per 1024 pixels (a 4-pixel group per thread)
inline int blocks_per_image(int64_t n_img, int64_t n_pix) {
	const int64_t want = cdiv(TARGET_BLOCKS, n_img);
	const int64_t cap = cdiv(n_pix, (int64_t)THREADS * 4);
	return (int)std::max<int64_t>(1, std::min(want, cap));
}

// Terms of one pixel: g / p (C values), gm / pm its masks, h the mask-out bit, w its weight.  t[0..6] follow FIND_IMAGE_METRIC_*.
template <int C>
__device__ __forceinline__ void pixel_terms(const float* g, const float* p, float gm, float pm, bool h, float w, float* t) {
	const float mt = h ? 0.f : pm;
	const float bg = gm > 0.f ? 1.f : 0.f, bp = mt > 0.f ? 1.f : 0.f, bc = bg * bp;
	float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
	for (int c = 0; c < C; ++c) {
		const float pt = h ? 1.f : p[c];
		const float d = g[c] - pt, e = g[c] * bg - pt * bp, f = g[c] * bc - pt * bc;
		s0 += d * d; s1 += e * e; s2 += f * f;
	}
	t[0] += s0; t[1] += s1; t[2] += s2;
	t[3] += gm * mt;
	t[4] += fmaxf(gm, mt);
	t[5] += w * s0;
	t[6] += w;
}

// grid: n_img * bpi blocks, block b of image i = blockIdx.x - i * bpi.  partial: (n_img * bpi, 7) fp64.
// VEC: n_pix % 4 == 0 and 16-byte aligned rows -- a thread reads 4 pixels as C float4 of each image, a float4 of each mask / weight
// and a 32-bit word of hide bytes.
template <int C, bool VEC>
__global__ __launch_bounds__(THREADS) void image_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
																 const float* __restrict__ pred_mask, const float* __restrict__ gt_mask,
																 const uint8_t* __restrict__ hide, const float* __restrict__ weight,
																 int64_t n_pix, int Cdyn, int bpi, double* __restrict__ partial) {
	__shared__ double red[THREADS / 64][FIND_IMAGE_METRIC_COUNT];
	const int64_t img = blockIdx.x / bpi;
	const int blk = (int)(blockIdx.x - img * bpi);
	const int64_t pix0 = img * n_pix;   // first pixel of this image in the (n_img * n_pix) masks
	double acc[FIND_IMAGE_METRIC_COUNT];
#pragma unroll
	for (int k = 0; k < FIND_IMAGE_METRIC_COUNT; ++k) acc[k] = 0.0;
	if constexpr (VEC) {
		const int64_t nq = n_pix >> 2, q0 = pix0 >> 2;
		const float4 one = make_float4(1.f, 1.f, 1.f, 1.f);
		for (int64_t q = (int64_t)blk * THREADS + threadIdx.x; q < nq; q += (int64_t)bpi * THREADS) {
			float vg[4 * C], vp[4 * C];
#pragma unroll
			for (int k = 0; k < C; ++k) {
				const float4 x = reinterpret_cast<const float4*>(gt)[(q0 + q) * C + k], y = reinterpret_cast<const float4*>(pred)[(q0 + q) * C + k];
				vg[4 * k] = x.x; vg[4 * k + 1] = x.y; vg[4 * k + 2] = x.z; vg[4 * k + 3] = x.w;
				vp[4 * k] = y.x; vp[4 * k + 1] = y.y; vp[4 * k + 2] = y.z; vp[4 * k + 3] = y.w;
			}
			const float4 gm = gt_mask ? reinterpret_cast<const float4*>(gt_mask)[q0 + q] : one;
			const float4 pm = pred_mask ? reinterpret_cast<const float4*>(pred_mask)[q0 + q] : one;
			const float4 w = weight ? reinterpret_cast<const float4*>(weight)[q0 + q] : one;
			const uint32_t h = hide ? reinterpret_cast<const uint32_t*>(hide)[q0 + q] : 0u;
			const float gma[4] = {gm.x, gm.y, gm.z, gm.w}, pma[4] = {pm.x, pm.y, pm.z, pm.w}, wa[4] = {w.x, w.y, w.z, w.w};
			float t[FIND_IMAGE_METRIC_COUNT] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
			for (int i = 0; i < 4; ++i) pixel_terms<C>(vg + i * C, vp + i * C, gma[i], pma[i], ((h >> (8 * i)) & 0xffu) != 0u, wa[i], t);
#pragma unroll
			for (int k = 0; k < FIND_IMAGE_METRIC_COUNT; ++k) acc[k] += (double)t[k];
		}
	} else {
		for (int64_t p = (int64_t)blk * THREADS + threadIdx.x; p < n_pix; p += (int64_t)bpi * THREADS) {
			const int64_t o = pix0 + p;
			const float gm = gt_mask ? gt_mask[o] : 1.f, pm = pred_mask ? pred_mask[o] : 1.f, w = weight ? weight[o] : 1.f;
			const bool h = hide && hide[o] != 0;
			float t[FIND_IMAGE_METRIC_COUNT] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
			// channels one at a time through the C = 1 body; only the per-pixel terms (3, 4, 6) must not repeat per channel
			for (int c = 0; c < Cdyn; ++c) {
				float u[FIND_IMAGE_METRIC_COUNT] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
				pixel_terms<1>(gt + o * Cdyn + c, pred + o * Cdyn + c, gm, pm, h, w, u);
				t[0] += u[0]; t[1] += u[1]; t[2] += u[2]; t[5] += u[5];
				if (c == 0) { t[3] = u[3]; t[4] = u[4]; t[6] = u[6]; }
			}
#pragma unroll
			for (int k = 0; k < FIND_IMAGE_METRIC_COUNT; ++k) acc[k] += (double)t[k];
		}
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
	for (int k = 0; k < FIND_IMAGE_METRIC_COUNT; ++k) {
		const double v = wave_sum(acc[k]);
		if (lane == 0) red[wave][k] = v;
	}
	__syncthreads();
	if (threadIdx.x < FIND_IMAGE_METRIC_COUNT) {
		double s = 0.0;
		for (int w = 0; w < THREADS / 64; ++w) s += red[w][threadIdx.x];
		partial[(int64_t)blockIdx.x * FIND_IMAGE_METRIC_COUNT + threadIdx.x] = s;
	}
}

// one thread per (image, sum): the image's bpi partials added in block order
__global__ __launch_bounds__(THREADS) void image_metrics_finalize_kernel(const double* __restrict__ partial, int64_t n_img, int bpi,
																		  double* __restrict__ sums) {
	const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
	if (i >= n_img * FIND_IMAGE_METRIC_COUNT) return;
	const int64_t img = i / FIND_IMAGE_METRIC_COUNT;
	const int k = (int)(i - img * FIND_IMAGE_METRIC_COUNT);
	const double* p = partial + img * bpi * FIND_IMAGE_METRIC_COUNT + k;
	double s = 0.0;
	for (int b = 0; b < bpi; ++b) s += p[(int64_t)b * FIND_IMAGE_METRIC_COUNT];
	sums[i] = s;
}

inline bool bad_dims(int64_t n_img, int64_t n_pix) {
	return n_img < 1 || n_pix < 1 || n_img > (1ll << 24) || n_pix > (1ll << 32) || n_img * n_pix > (1ll << 40);
}

inline bool al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace eval2d
}  // namespace find

using namespace find;
using namespace find::eval2d;

extern "C" int64_t find_image_metrics_ws_bytes(int64_t n_img, int64_t n_pix) {
	if (bad_dims(n_img, n_pix)) return -1;
	return align_up(n_img * blocks_per_image(n_img, n_pix) * FIND_IMAGE_METRIC_COUNT * (int64_t)sizeof(double), 256);
}

extern "C" int find_image_metrics(const float* pred, const float* gt, const float* pred_mask, const float* gt_mask, const uint8_t* hide,
								  const float* weight, int64_t n_img, int64_t n_pix, int64_t channels, double* sums, void* ws, int64_t ws_bytes,
								  void* stream) {
	FIND_REQUIRE(pred && gt && sums && ws, "find_image_metrics: NULL argument");
	FIND_REQUIRE(!bad_dims(n_img, n_pix) && channels >= 1 && channels <= 16, "find_image_metrics: bad sizes (n_img %lld, n_pix %lld, channels %lld)",
				 (long long)n_img, (long long)n_pix, (long long)channels);
	if (ws_bytes < find_image_metrics_ws_bytes(n_img, n_pix)) {
		set_error("find_image_metrics: workspace too small (%lld < %lld bytes)", (long long)ws_bytes, (long long)find_image_metrics_ws_bytes(n_img, n_pix));
		return FIND_EWORKSPACE;
	}
	const int bpi = blocks_per_image(n_img, n_pix);
	const int64_t nblk = n_img * bpi;
	FIND_REQUIRE(nblk <= 0x7fffffffll, "find_image_metrics: too many blocks");
	hipStream_t s = (hipStream_t)stream;
	double* partial = (double*)ws;
	const bool vec = (n_pix & 3) == 0 && (channels == 3 || channels == 1) && al(pred, 16) && al(gt, 16) && al(pred_mask, 16) && al(gt_mask, 16) &&
					 al(weight, 16) && al(hide, 4);
	if (vec && channels == 3)
		hipLaunchKernelGGL((image_metrics_kernel<3, true>), dim3((unsigned)nblk), dim3(THREADS), 0, s, pred, gt, pred_mask, gt_mask, hide, weight, n_pix, 3, bpi,
						   partial);
	else if (vec)
		hipLaunchKernelGGL((image_metrics_kernel<1, true>), dim3((unsigned)nblk), dim3(THREADS), 0, s, pred, gt, pred_mask, gt_mask, hide, weight, n_pix, 1, bpi,
						   partial);
	else
		hipLaunchKernelGGL((image_metrics_kernel<1, false>), dim3((unsigned)nblk), dim3(THREADS), 0, s, pred, gt, pred_mask, gt_mask, hide, weight, n_pix,
						   (int)channels, bpi, partial);
	FIND_LAUNCH_CHECK("image_metrics_kernel");
	hipLaunchKernelGGL(image_metrics_finalize_kernel, dim3((unsigned)cdiv(n_img * FIND_IMAGE_METRIC_COUNT, THREADS)), dim3(THREADS), 0, s,
					   (const double*)partial, n_img, bpi, sums);
	FIND_LAUNCH_CHECK("image_metrics_finalize_kernel");
	return FIND_OK;
}
