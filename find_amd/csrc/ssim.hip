// SSIM (Wang et al. 2004) between two channel-last image batches, one pass each way, no atomics: two runs agree bit for bit.
//   a = x * xm, b = y * ym (masks optional) are formed at load time.  With the separable 11-tap Gaussian window (sigma 1.5, normalised in
//   double on the host, fp32 constants in the launch arguments) and the window means m1 = E[a], m2 = E[b], s11 = E[a^2], s22 = E[b^2],
//   s12 = E[ab], per pixel and channel
//     ssim = (2 m1 m2 + C1)(2 (s12 - m1 m2) + C2) / ((m1^2 + m2^2 + C1)((s11 - m1^2) + (s22 - m2^2) + C2)).
//   `same`: zero padding, the mean over H W C values;  `valid`: the mean over the (H - 10)(W - 10) C values whose window lies inside.
//
// Tile: a workgroup of 256 threads owns 16 x 16 output pixels and stages the 26 x 26 pixels of tile + 5-pixel halo.  Why 16 x 16: the halo
//   makes a workgroup read (26 * 26) / 256 = 2.6 pixels per output pixel (32 x 8 would read 2.95), and the vertical pass then has a wave
//   read four full rows of 16 = 64 consecutive words of a moment plane, which is conflict-free WITHOUT padding the plane's row stride (a
//   stride of 17 would wrap three lanes of the fourth row onto the first row's banks).  LDS at C = 4: a and b planar per channel
//   2 * 4 * 26 * 26 * 4 = 21.6 KiB, five moment planes of 26 x 16 doubles 16.6 KiB: 38.3 KiB, four workgroups (16 waves) per CU of 160 KiB.
//   The horizontal pass (26 rows x 16 columns, 416 items over two rounds of the 256 threads) reads the staged rows, whose stride is 26 words:
//   a half-wave -- the unit that conflicts on a 4-byte LDS read -- takes rows r and r + 8 (8 * 26 = 16 mod 32), so its 32 lanes fall on 32
//   banks; hrow() is that assignment.  Both statements are about the READS.  The row pass's 8-byte stores of the moment planes go out in
//   groups of 16 lanes, a row of 16 doubles each, and rows r and r + 8 lie 256 words apart: no conflict counter was read for them.
// Loads: a staged row starts at pixel 16 k - 5 of an image row of W C floats, which is 16-byte aligned only by accident, so the stage reads
//   single floats, consecutive lanes consecutive addresses (a 26 C float run per row); nothing outside the image is read.
// Arithmetic: a, b, the window and every stored map are fp32; the eleven-tap sums of both passes and the formula are double.  s11 - m1^2
//   cancels against C2 = 9e-4 L^2: moments rounded to fp32 leave a relative error of 1e-4 in a flat pixel's value and more in its gradient,
//   doubles leave what the fp32 inputs and window carry.  The kernel moves 8 (C + 1) bytes in and 12 C bytes out per pixel and runs about
//   275 double FMAs per pixel and channel: measured, those and their LDS passes set its time, not the traffic.
// Backward: dmaps was chosen over recomputing the moments on a doubled halo.  The forward stores A1, A2, A3 = d ssim / d (m1, s11, s12),
//   scaled by 1 / (n_img count), zero where a pixel does not count, planar as (n_img, C, 3, H, W) fp32 -- a wave's store is four 64-byte
//   runs -- and the backward is one separable gather of those three maps over the same tile + halo:
//     d a(q) = sum_p w(p - q) [A1(p) + 2 a(q) A2(p) + b(q) A3(p)],   d_x = xm d a g,   d_xm = sum_c x_c d a_c g.
//   Recomputing would stage a 36 x 36 halo of a and b and run the double moment passes over 26 x 26 pixels per 16 x 16 tile, 2.6 times the
//   forward's arithmetic, to save 24 C bytes of traffic per pixel: the arithmetic is the dearer of the two here.  The maps are fp32 (their
//   rounding is relative to each value); the gather and the last combination are double, a third of the forward's arithmetic: 2 a G2 and
//   b G3 are each 1 / C2 times larger than their sum in a flat region, and with a == b, A3 = -2 A2 and they cancel exactly.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "find_hip.h"
#include "common.h"

namespace find {
namespace ssim {

constexpr int TW = 16, TH = 16, RAD = 5, TAPS = 2 * RAD + 1;
constexpr int SW = TW + 2 * RAD, SH = TH + 2 * RAD;   // the staged tile
constexpr int THREADS = TW * TH;
constexpr int HITEMS = 2 * THREADS;                   // rounds of the horizontal pass cover 32 rows; the staged tile has 26

struct Args {
	const float *x, *xm, *y, *ym;   // (n_img, H, W, C), (n_img, H, W) or nullptr: 1
	int H, W, valid;
	double c1, c2, scale;           // scale: 1 / (n_img * values per image)
	float w[TAPS];
};

struct BwdArgs {
	const float *x, *xm, *y, *ym, *g, *dmaps;
	float *d_x, *d_xm;
	int H, W;
	float w[TAPS];
};

// the staged row of item `it` of the horizontal pass: lanes 0-15 and 16-31 of a half-wave get rows r and r + 8 (see the header)
__device__ __forceinline__ int hrow(int it) {
	const int j = it >> 5;
	return (j >> 3) * 16 + (j & 7) + 8 * ((it >> 4) & 1);
}

// grid (tiles in x, tiles in y, images): partial[(img * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = the sum of the tile's counting ssim values
template <int C>
__global__ __launch_bounds__(THREADS) void ssim_fwd_kernel(const Args a, double* __restrict__ partial, float* __restrict__ dmaps) {
	__shared__ float sa[C * SH * SW], sb[C * SH * SW];
	__shared__ double mom[5][SH * TW];
	__shared__ double wsum[THREADS / 64];
	const int tid = threadIdx.x, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
	const int64_t HW = (int64_t)a.H * a.W, ibase = (int64_t)blockIdx.z * HW;
	for (int i = tid; i < SH * SW * C; i += THREADS) {
		const int r = i / (SW * C), e = i - r * (SW * C), col = e / C, c = e - col * C;
		const int gy = y0 - RAD + r, gx = x0 - RAD + col;
		float va = 0.f, vb = 0.f;
		if ((unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W) {
			const int64_t p = ibase + (int64_t)gy * a.W + gx;
			va = a.x[p * C + c];
			vb = a.y[p * C + c];
			if (a.xm) va *= a.xm[p];
			if (a.ym) vb *= a.ym[p];
		}
		sa[(c * SH + r) * SW + col] = va;
		sb[(c * SH + r) * SW + col] = vb;
	}
	__syncthreads();
	const int ty = tid >> 4, tx = tid & 15, gy = y0 + ty, gx = x0 + tx;
	const bool inside = gy < a.H && gx < a.W;
	const bool counts = inside && (!a.valid || (gy >= RAD && gy < a.H - RAD && gx >= RAD && gx < a.W - RAD));
	double acc = 0.0;
	for (int c = 0; c < C; ++c) {
		for (int it = tid; it < HITEMS; it += THREADS) {
			const int row = hrow(it), col = it & 15;
			if (row >= SH) continue;
			const float* pa = sa + (c * SH + row) * SW + col;
			const float* pb = sb + (c * SH + row) * SW + col;
			double m1 = 0.0, m2 = 0.0, s11 = 0.0, s22 = 0.0, s12 = 0.0;
#pragma unroll
			for (int k = 0; k < TAPS; ++k) {
				const double va = pa[k], vb = pb[k];
				const double wa = (double)a.w[k] * va, wb = (double)a.w[k] * vb;   // (exact: 24 x 24 bits)
				m1 += wa;
				m2 += wb;
				s11 = fma(wa, va, s11);
				s22 = fma(wb, vb, s22);
				s12 = fma(wa, vb, s12);
			}
			mom[0][row * TW + col] = m1;
			mom[1][row * TW + col] = m2;
			mom[2][row * TW + col] = s11;
			mom[3][row * TW + col] = s22;
			mom[4][row * TW + col] = s12;
		}
		__syncthreads();
		double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
		for (int k = 0; k < TAPS; ++k) {
			const double w = a.w[k];
#pragma unroll
			for (int j = 0; j < 5; ++j) m[j] = fma(w, mom[j][(ty + k) * TW + tx], m[j]);
		}
		if (inside) {
			double A1 = 0.0, A2 = 0.0, A3 = 0.0;
			if (counts) {
				const double m1 = m[0], m2 = m[1];
				const double N1 = 2.0 * m1 * m2 + a.c1, N2 = 2.0 * (m[4] - m1 * m2) + a.c2;
				const double D1 = m1 * m1 + m2 * m2 + a.c1, D2 = (m[2] - m1 * m1) + (m[3] - m2 * m2) + a.c2;
				const double inv = 1.0 / (D1 * D2);
				const double S = N1 * N2 * inv;
				acc += S;
				A1 = (2.0 * m2 * (N2 - N1) - 2.0 * m1 * S * (D2 - D1)) * inv * a.scale;
				A2 = -S * D1 * inv * a.scale;
				A3 = 2.0 * N1 * inv * a.scale;
			}
			if (dmaps) {
				float* d = dmaps + ((int64_t)blockIdx.z * C + c) * 3 * HW + (int64_t)gy * a.W + gx;
				d[0] = (float)A1;
				d[HW] = (float)A2;
				d[2 * HW] = (float)A3;
			}
		}
		__syncthreads();
	}
	acc = wave_sum(acc);
	if ((tid & 63) == 0) wsum[tid >> 6] = acc;
	__syncthreads();
	if (tid == 0) {
		double s = 0.0;
		for (int k = 0; k < THREADS / 64; ++k) s += wsum[k];
		partial[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
	}
}

// One workgroup.  Wave v adds the tiles of the images v, v + 4, ...: lane l the tiles l, l + 64, ... of the image, then the butterfly; it
// writes per_image and keeps a running sum of its images.  Thread 0 adds the four waves' sums.
__global__ __launch_bounds__(THREADS) void ssim_sum_kernel(const double* __restrict__ partial, int64_t n_img, int64_t tpi, double count,
														   double* __restrict__ per_image, float* __restrict__ mean_out) {
	__shared__ double wsum[THREADS / 64];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	double t = 0.0;
	for (int64_t img = wave; img < n_img; img += THREADS / 64) {
		double s = 0.0;
		for (int64_t i = lane; i < tpi; i += 64) s += partial[img * tpi + i];
		s = wave_sum(s);
		t += s;
		if (per_image && lane == 0) per_image[img] = s / count;
	}
	if (lane == 0) wsum[wave] = t;
	__syncthreads();
	if (threadIdx.x == 0) {
		double s = 0.0;
		for (int k = 0; k < THREADS / 64; ++k) s += wsum[k];
		*mean_out = (float)(s / (count * (double)n_img));
	}
}

// grid as the forward's; every pixel of d_x / d_xm is written
template <int C>
__global__ __launch_bounds__(THREADS) void ssim_bwd_kernel(const BwdArgs a) {
	__shared__ float st[3 * SH * SW];
	__shared__ double hp[3][SH * TW];
	const int tid = threadIdx.x, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
	const int64_t HW = (int64_t)a.H * a.W, ibase = (int64_t)blockIdx.z * HW;
	const int ty = tid >> 4, tx = tid & 15, gy = y0 + ty, gx = x0 + tx;
	const bool inside = gy < a.H && gx < a.W;
	const int64_t p = ibase + (int64_t)gy * a.W + gx;
	const double g = *a.g;
	const float mv = inside && a.xm ? a.xm[p] : 1.f;
	const float nv = inside && a.ym ? a.ym[p] : 1.f;
	float dx[C];
	double dm = 0.0;
#pragma unroll
	for (int c = 0; c < C; ++c) {
		const float* src = a.dmaps + ((int64_t)blockIdx.z * C + c) * 3 * HW;
		for (int i = tid; i < 3 * SH * SW; i += THREADS) {
			const int j = i / (SH * SW), e = i - j * (SH * SW), r = e / SW, col = e - r * SW;
			const int sy = y0 - RAD + r, sx = x0 - RAD + col;
			st[i] = ((unsigned)sy < (unsigned)a.H && (unsigned)sx < (unsigned)a.W) ? src[j * HW + (int64_t)sy * a.W + sx] : 0.f;
		}
		__syncthreads();
		for (int it = tid; it < HITEMS; it += THREADS) {
			const int row = hrow(it), col = it & 15;
			if (row >= SH) continue;
#pragma unroll
			for (int j = 0; j < 3; ++j) {
				const float* ps = st + (j * SH + row) * SW + col;
				double s = 0.0;
#pragma unroll
				for (int k = 0; k < TAPS; ++k) s = fma((double)a.w[k], (double)ps[k], s);
				hp[j][row * TW + col] = s;
			}
		}
		__syncthreads();
		double G[3] = {0.0, 0.0, 0.0};
#pragma unroll
		for (int k = 0; k < TAPS; ++k)
#pragma unroll
			for (int j = 0; j < 3; ++j) G[j] = fma((double)a.w[k], hp[j][(ty + k) * TW + tx], G[j]);
		dx[c] = 0.f;
		if (inside) {
			const float xv = a.x[p * C + c];
			const float av = xv * mv, bv = a.y[p * C + c] * nv;
			const double da = (G[0] + (2.0 * (double)av * G[1] + (double)bv * G[2])) * g;
			dx[c] = (float)((double)mv * da);
			dm += (double)xv * da;
		}
		// (the next channel's stage is written behind the barrier above, its horizontal pass writes hp behind the next one)
	}
	if (!inside) return;
	if (a.d_x) {
#pragma unroll
		for (int c = 0; c < C; ++c) a.d_x[p * C + c] = dx[c];
	}
	if (a.d_xm) a.d_xm[p] = (float)dm;
}

inline void window(float w[TAPS]) {
	double g[TAPS], sum = 0.0;
	for (int k = 0; k < TAPS; ++k) {
		g[k] = exp(-(double)((k - RAD) * (k - RAD)) / (2.0 * 1.5 * 1.5));
		sum += g[k];
	}
	for (int k = 0; k < TAPS; ++k) w[k] = (float)(g[k] / sum);
}

inline bool sizes_ok(int64_t n_img, int64_t H, int64_t W, int64_t C) {
	return n_img >= 1 && n_img < 65536 && H >= 1 && H <= 32768 && W >= 1 && W <= 32768 && C >= 1 && C <= 4 && n_img * H * W * C < ((int64_t)1 << 36);
}
inline int64_t tiles(int64_t H, int64_t W) { return cdiv(H, (int64_t)TH) * cdiv(W, (int64_t)TW); }

static int check_args(const char* who, const void* x, const void* y, int64_t n_img, int64_t H, int64_t W, int64_t C, float L, int valid) {
	if (!x || !y) {
		set_error("%s: NULL argument", who);
		return FIND_EINVAL;
	}
	if (!sizes_ok(n_img, H, W, C)) {
		set_error("%s: bad sizes: %lld images of %lld x %lld x %lld", who, (long long)n_img, (long long)H, (long long)W, (long long)C);
		return FIND_EINVAL;
	}
	if (!(L > 0.f)) {
		set_error("%s: data_range > 0 expected", who);
		return FIND_EINVAL;
	}
	if (valid && (H < TAPS || W < TAPS)) {
		set_error("%s: the valid border needs H, W >= %d, got %lld x %lld", who, TAPS, (long long)H, (long long)W);
		return FIND_EINVAL;
	}
	return FIND_OK;
}

}  // namespace ssim
}  // namespace find

using namespace find;

extern "C" int64_t find_ssim_ws_bytes(int64_t n_img, int64_t H, int64_t W, int64_t C, int want_grad) {
	if (!ssim::sizes_ok(n_img, H, W, C)) {
		set_error("find_ssim_ws_bytes: bad sizes: %lld images of %lld x %lld x %lld", (long long)n_img, (long long)H, (long long)W, (long long)C);
		return -1;
	}
	if (want_grad) return n_img * H * W * C * 3 * (int64_t)sizeof(float);
	return n_img * ssim::tiles(H, W) * (int64_t)sizeof(double);
}

extern "C" int find_ssim_fwd(const float* x, const float* xm, const float* y, const float* ym, int64_t n_img, int64_t H, int64_t W, int64_t C, float L,
							 int valid, float* mean_out, double* per_image, float* dmaps, void* ws, int64_t ws_bytes, void* stream) {
	if (ssim::check_args("find_ssim_fwd", x, y, n_img, H, W, C, L, valid) != FIND_OK) return FIND_EINVAL;
	FIND_REQUIRE(mean_out && ws, "find_ssim_fwd: NULL argument");
	const int64_t tpi = ssim::tiles(H, W);
	if (ws_bytes < n_img * tpi * (int64_t)sizeof(double) || (reinterpret_cast<uintptr_t>(ws) & 7) || (reinterpret_cast<uintptr_t>(per_image) & 7)) {
		set_error("find_ssim_fwd: workspace of %lld bytes, %lld needed (8-byte aligned, as per_image)", (long long)ws_bytes,
				  (long long)(n_img * tpi * (int64_t)sizeof(double)));
		return FIND_EWORKSPACE;
	}
	const double count = valid ? (double)((H - 2 * ssim::RAD) * (W - 2 * ssim::RAD) * C) : (double)(H * W * C);
	ssim::Args a;
	a.x = x; a.xm = xm; a.y = y; a.ym = ym;
	a.H = (int)H; a.W = (int)W; a.valid = valid ? 1 : 0;
	a.c1 = (0.01 * (double)L) * (0.01 * (double)L);
	a.c2 = (0.03 * (double)L) * (0.03 * (double)L);
	a.scale = 1.0 / ((double)n_img * count);
	ssim::window(a.w);
	hipStream_t s = reinterpret_cast<hipStream_t>(stream);
	double* partial = reinterpret_cast<double*>(ws);
	const dim3 grid((unsigned)cdiv(W, (int64_t)ssim::TW), (unsigned)cdiv(H, (int64_t)ssim::TH), (unsigned)n_img), block(ssim::THREADS);
	switch (C) {
		case 1: hipLaunchKernelGGL(ssim::ssim_fwd_kernel<1>, grid, block, 0, s, a, partial, dmaps); break;
		case 2: hipLaunchKernelGGL(ssim::ssim_fwd_kernel<2>, grid, block, 0, s, a, partial, dmaps); break;
		case 3: hipLaunchKernelGGL(ssim::ssim_fwd_kernel<3>, grid, block, 0, s, a, partial, dmaps); break;
		default: hipLaunchKernelGGL(ssim::ssim_fwd_kernel<4>, grid, block, 0, s, a, partial, dmaps); break;
	}
	FIND_LAUNCH_CHECK("ssim ssim_fwd_kernel");
	hipLaunchKernelGGL(ssim::ssim_sum_kernel, dim3(1), block, 0, s, (const double*)partial, n_img, tpi, count, per_image, mean_out);
	FIND_LAUNCH_CHECK("ssim ssim_sum_kernel");
	return FIND_OK;
}

extern "C" int find_ssim_bwd(const float* x, const float* xm, const float* y, const float* ym, int64_t n_img, int64_t H, int64_t W, int64_t C, float L,
							 int valid, const float* g, const float* dmaps, float* d_x, float* d_xm, void* stream) {
	if (ssim::check_args("find_ssim_bwd", x, y, n_img, H, W, C, L, valid) != FIND_OK) return FIND_EINVAL;
	FIND_REQUIRE(g && dmaps && (d_x || d_xm), "find_ssim_bwd: NULL argument");
	FIND_REQUIRE(!d_xm || xm, "find_ssim_bwd: d_xm without xm");
	ssim::BwdArgs a;
	a.x = x; a.xm = xm; a.y = y; a.ym = ym; a.g = g; a.dmaps = dmaps; a.d_x = d_x; a.d_xm = d_xm;
	a.H = (int)H; a.W = (int)W;
	ssim::window(a.w);
	hipStream_t s = reinterpret_cast<hipStream_t>(stream);
	const dim3 grid((unsigned)cdiv(W, (int64_t)ssim::TW), (unsigned)cdiv(H, (int64_t)ssim::TH), (unsigned)n_img), block(ssim::THREADS);
	switch (C) {
		case 1: hipLaunchKernelGGL(ssim::ssim_bwd_kernel<1>, grid, block, 0, s, a); break;
		case 2: hipLaunchKernelGGL(ssim::ssim_bwd_kernel<2>, grid, block, 0, s, a); break;
		case 3: hipLaunchKernelGGL(ssim::ssim_bwd_kernel<3>, grid, block, 0, s, a); break;
		default: hipLaunchKernelGGL(ssim::ssim_bwd_kernel<4>, grid, block, 0, s, a); break;
	}
	FIND_LAUNCH_CHECK("ssim ssim_bwd_kernel");
	return FIND_OK;
}
