// Depth: the backward of the K = 1 z-buffer find_render_fwd hands out, and a masked, robust loss between two depth maps.
//   depth_bwd_kernel   a thread per pixel: the face pix_to_face names, its corners in view space, the pixel's ray d, and
//                      z = (n . p0) / (n . d) differentiated in the corners: d p_k = g b_k n / (n . d), b_k the barycentrics of the hit point
//                      X = z d in the face's plane.  It reads no render workspace.  d v_k = d p_k @ R^T goes to d_verts with float atomics
//                      (nine per covered pixel with a gradient), as the render backward's do: two runs may differ in the last bits.
//   dloss_fwd / _bwd   sum_i w_i rho(r_i) / max(sum_i w_i, 1e-12), r = pred - target, rho one of |r|, r^2, Huber; a pixel counts where
//                      both depths are positive and |r| <= trunc.  A thread takes four pixels (16-byte loads where pointers and the
//                      image's first pixel allow), a workgroup 1024 pixels of ONE image, one pair of double partials each;
//                      dloss_sum_kernel adds the pairs per image (a wave per image, fixed order), then the images.
// A face or vertex index out of range contributes nothing and is never read through.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "find_hip.h"
#include "common.h"

namespace find {
namespace depth {

constexpr int THREADS = 256;
constexpr int PX = 4;   // pixels per thread of the loss kernels

struct BwdArgs {
	const float* verts;         // (N, V, 3)
	const int32_t* faces;       // (fb, F, 3)
	const float* R;             // (M, 3, 3)
	const float* T;             // (M, 3)
	const int32_t* pix_to_face; // (N * M, H * W)
	const float* d_depth;       // (N * M, H * W)
	float* d_verts;             // (N, V, 3)
	int64_t fstride;            // 0 (shared faces) or 3 F
	int M, V, F, H, W;
	float inv_s;                // tan(fov / 2)
};

__global__ __launch_bounds__(THREADS) void depth_bwd_kernel(const BwdArgs a) {
	const int img = blockIdx.y;
	const int pix = blockIdx.x * blockDim.x + threadIdx.x;
	if (pix >= a.H * a.W) return;
	const int64_t o = (int64_t)img * a.H * a.W + pix;
	const int32_t packed = a.pix_to_face[o];
	if (packed < 0) return;
	const float g = a.d_depth[o];
	if (g == 0.f) return;
	const int64_t f = (int64_t)packed - (int64_t)img * a.F;
	if (f < 0 || f >= a.F) return;
	const int mesh = img / a.M, view = img - mesh * a.M;
	const int32_t* fp = a.faces + (int64_t)mesh * a.fstride + 3 * f;
	const int idx[3] = {fp[0], fp[1], fp[2]};
	if ((unsigned)idx[0] >= (unsigned)a.V || (unsigned)idx[1] >= (unsigned)a.V || (unsigned)idx[2] >= (unsigned)a.V) return;
	const float* r = a.R + 9 * view;
	const float* t = a.T + 3 * view;
	const float* vm = a.verts + (int64_t)mesh * a.V * 3;
	float p[3][3];
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const float* v = vm + 3 * (int64_t)idx[k];
		const float x = v[0], y = v[1], z = v[2];
#pragma unroll
		for (int j = 0; j < 3; ++j) p[k][j] = x * r[j] + y * r[3 + j] + z * r[6 + j] + t[j];
	}
	const int yi = pix / a.W, xi = pix - yi * a.W;
	const float d[3] = {(1.0f - (2.0f * xi + 1.0f) / (float)a.W) * a.inv_s, (1.0f - (2.0f * yi + 1.0f) / (float)a.H) * a.inv_s, 1.0f};
	const float u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
	const float w[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
	const float n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
	const float nd = n[0] * d[0] + n[1] * d[1] + n[2] * d[2];
	const float nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
	if (nd == 0.f || nn == 0.f) return;
	const float z = (n[0] * p[0][0] + n[1] * p[0][1] + n[2] * p[0][2]) / nd;
	const float X[3] = {z * d[0], z * d[1], z * d[2]};
	float e[3][3];   // p_k - X
#pragma unroll
	for (int k = 0; k < 3; ++k)
#pragma unroll
		for (int j = 0; j < 3; ++j) e[k][j] = p[k][j] - X[j];
	const float scale = g / (nd * nn);
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const float* q = e[(k + 1) % 3];
		const float* s = e[(k + 2) % 3];
		const float cx = q[1] * s[2] - q[2] * s[1], cy = q[2] * s[0] - q[0] * s[2], cz = q[0] * s[1] - q[1] * s[0];
		const float c = (cx * n[0] + cy * n[1] + cz * n[2]) * scale;   // g b_k / (n . d)
		if (!(fabsf(c) <= 3.402823466e38f)) continue;                   // (a degenerate face in fp32: nothing rather than inf / nan)
		const float dp[3] = {c * n[0], c * n[1], c * n[2]};
		float* dv = a.d_verts + ((int64_t)mesh * a.V + idx[k]) * 3;
#pragma unroll
		for (int i = 0; i < 3; ++i) atomicAdd(dv + i, dp[0] * r[3 * i] + dp[1] * r[3 * i + 1] + dp[2] * r[3 * i + 2]);
	}
}

// ------------------------------------------------------------------------------------------------ depth loss
struct LossArgs {
	const float* pred;
	const float* target;
	const float* weight;   // or nullptr: 1
	int64_t n_pix;
	int kind;
	float delta, trunc;
};

// the n <= PX pixels of image `img` from `base` on; VEC: the full group of four with 16-byte loads
template <bool VEC>
__device__ __forceinline__ void load_px(const LossArgs& a, int64_t at, int n, bool vec, float pp[PX], float tt[PX], float ww[PX]) {
	if (VEC && vec && n == PX) {
		const float4 p4 = *reinterpret_cast<const float4*>(a.pred + at);
		const float4 t4 = *reinterpret_cast<const float4*>(a.target + at);
		pp[0] = p4.x; pp[1] = p4.y; pp[2] = p4.z; pp[3] = p4.w;
		tt[0] = t4.x; tt[1] = t4.y; tt[2] = t4.z; tt[3] = t4.w;
		if (a.weight) {
			const float4 w4 = *reinterpret_cast<const float4*>(a.weight + at);
			ww[0] = w4.x; ww[1] = w4.y; ww[2] = w4.z; ww[3] = w4.w;
		} else {
			ww[0] = ww[1] = ww[2] = ww[3] = 1.f;
		}
		return;
	}
#pragma unroll
	for (int k = 0; k < PX; ++k) {
		const bool in = k < n;
		pp[k] = in ? a.pred[at + k] : 0.f;
		tt[k] = in ? a.target[at + k] : 0.f;
		ww[k] = in ? (a.weight ? a.weight[at + k] : 1.f) : 0.f;
	}
}

// w_i (0 on an invalid pixel), rho(r) and rho'(r) of one pixel
__device__ __forceinline__ float pixel(const LossArgs& a, float p, float t, float w, float& rho, float& drho) {
	const float r = p - t, ar = fabsf(r);
	const bool valid = p > 0.f && t > 0.f && (a.trunc <= 0.f || ar <= a.trunc);
	const float sgn = r > 0.f ? 1.f : (r < 0.f ? -1.f : 0.f);
	if (a.kind == FIND_DEPTH_L1) {
		rho = ar; drho = sgn;
	} else if (a.kind == FIND_DEPTH_L2) {
		rho = r * r; drho = 2.f * r;
	} else if (ar <= a.delta) {
		rho = r * r / (2.f * a.delta); drho = r / a.delta;
	} else {
		rho = ar - 0.5f * a.delta; drho = sgn;
	}
	if (!valid) rho = drho = 0.f;   // (an inf or a nan of an invalid pixel must not reach the sums through 0 * x)
	return valid ? w : 0.f;
}

// the workgroup's sums of a and b in double, fixed order: thread 0 returns them
__device__ __forceinline__ void block_sum2(double& a, double& b, double* wsum) {
	a = wave_sum(a); b = wave_sum(b);
	if ((threadIdx.x & 63) == 0) {
		wsum[2 * (threadIdx.x >> 6)] = a;
		wsum[2 * (threadIdx.x >> 6) + 1] = b;
	}
	__syncthreads();
	a = b = 0.0;
	if (threadIdx.x == 0)
		for (int k = 0; k < (int)(blockDim.x >> 6); ++k) {
			a += wsum[2 * k];
			b += wsum[2 * k + 1];
		}
}

// grid (workgroups per image, images): partial[(img * gridDim.x + block) * 2 ..] = [sum w rho, sum w] of the workgroup's pixels
template <bool VEC>
__global__ __launch_bounds__(THREADS) void dloss_fwd_kernel(const LossArgs a, double* __restrict__ partial) {
	__shared__ double wsum[2 * THREADS / 64];
	const int64_t img0 = (int64_t)blockIdx.y * a.n_pix;
	const int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * PX;
	const int n = (int)max((int64_t)0, min((int64_t)PX, a.n_pix - base));
	double num = 0.0, den = 0.0;
	if (n > 0) {
		float pp[PX], tt[PX], ww[PX];
		load_px<VEC>(a, img0 + base, n, (img0 & 3) == 0, pp, tt, ww);
#pragma unroll
		for (int k = 0; k < PX; ++k) {
			float rho, drho;
			const float w = pixel(a, pp[k], tt[k], ww[k], rho, drho);   // (a pixel past the end has weight 0 and depth 0)
			num += (double)(w * rho);
			den += (double)w;
		}
	}
	block_sum2(num, den, wsum);
	if (threadIdx.x == 0) {
		const int64_t b = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
		partial[2 * b] = num;
		partial[2 * b + 1] = den;
	}
}

// One workgroup.  Wave v adds the pairs of the images v, v + 4, ...: lane l those of the blocks l, l + 64, ... of the image, then the
// butterfly; it writes per_image and keeps a running sum of its images.  Thread 0 adds the four waves' sums: sums[0], sums[1], *loss.
__global__ __launch_bounds__(THREADS) void dloss_sum_kernel(const double* __restrict__ partial, int64_t n_img, int64_t bpi, double* __restrict__ sums,
															double* __restrict__ per_image, float* __restrict__ loss_out) {
	__shared__ double wsum[2 * THREADS / 64];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	double ta = 0.0, tb = 0.0;
	for (int64_t img = wave; img < n_img; img += THREADS / 64) {
		double x = 0.0, y = 0.0;
		for (int64_t i = lane; i < bpi; i += 64) {
			x += partial[2 * (img * bpi + i)];
			y += partial[2 * (img * bpi + i) + 1];
		}
		x = wave_sum(x); y = wave_sum(y);
		ta += x; tb += y;
		if (per_image && lane == 0) {
			per_image[2 * img] = x;
			per_image[2 * img + 1] = y;
		}
	}
	if (lane == 0) {
		wsum[2 * wave] = ta;
		wsum[2 * wave + 1] = tb;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		double x = 0.0, y = 0.0;
		for (int k = 0; k < THREADS / 64; ++k) {
			x += wsum[2 * k];
			y += wsum[2 * k + 1];
		}
		sums[0] = x;
		sums[1] = y;
		*loss_out = (float)(x / fmax(y, 1e-12));
	}
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void dloss_bwd_kernel(const LossArgs a, const float* __restrict__ d_loss, const double* __restrict__ sums,
															float* __restrict__ d_pred) {
	const int64_t img0 = (int64_t)blockIdx.y * a.n_pix;
	const int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * PX;
	const int n = (int)max((int64_t)0, min((int64_t)PX, a.n_pix - base));
	if (n <= 0) return;
	const float scale = (float)((double)*d_loss / fmax(sums[1], 1e-12));
	const bool vec = (img0 & 3) == 0;
	float pp[PX], tt[PX], ww[PX], dd[PX];
	load_px<VEC>(a, img0 + base, n, vec, pp, tt, ww);
#pragma unroll
	for (int k = 0; k < PX; ++k) {
		float rho, drho;
		const float w = pixel(a, pp[k], tt[k], ww[k], rho, drho);
		dd[k] = w != 0.f ? scale * w * drho : 0.f;
	}
	if (VEC && vec && n == PX) {
		*reinterpret_cast<float4*>(d_pred + img0 + base) = make_float4(dd[0], dd[1], dd[2], dd[3]);
	} else {
		for (int k = 0; k < n; ++k) d_pred[img0 + base + k] = dd[k];
	}
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int64_t blocks_per_image(int64_t n_pix) { return cdiv(n_pix, (int64_t)THREADS * PX); }
inline bool sizes_ok(int64_t n_img, int64_t n_pix) {
	return n_img >= 1 && n_img < 65536 && n_pix >= 1 && n_pix < ((int64_t)1 << 31) && n_img * n_pix < ((int64_t)1 << 36);
}
inline int64_t ws_need(int64_t n_img, int64_t n_pix) { return (2 + 2 * n_img * blocks_per_image(n_pix)) * (int64_t)sizeof(double); }

}  // namespace depth
}  // namespace find

using namespace find;

extern "C" int find_depth_bwd(const find_render_params* rp, const float* verts, const int32_t* faces, int64_t faces_batch, const float* R, const float* T,
							  int64_t n_meshes, int64_t n_views, int64_t n_verts, int64_t n_faces, const int32_t* pix_to_face, const float* d_depth,
							  float* d_verts, void* stream) {
	FIND_REQUIRE(rp != nullptr, "find_depth_bwd: params is NULL");
	FIND_REQUIRE(verts && faces && R && T && pix_to_face && d_depth && d_verts, "find_depth_bwd: NULL argument");
	FIND_REQUIRE(rp->image_h >= 1 && rp->image_w >= 1 && rp->image_h <= 2048 && rp->image_w <= 2048, "find_depth_bwd: image size out of range (1 .. 2048)");
	FIND_REQUIRE(n_meshes >= 1 && n_views >= 1 && n_views <= 256 && n_meshes * n_views < 65536, "find_depth_bwd: bad batch (%lld meshes x %lld views)",
				 (long long)n_meshes, (long long)n_views);
	FIND_REQUIRE(n_verts >= 1 && n_faces >= 1 && n_verts < (1ll << 28) && n_faces < (1ll << 24), "find_depth_bwd: bad mesh size V=%lld F=%lld",
				 (long long)n_verts, (long long)n_faces);
	FIND_REQUIRE(faces_batch == 1 || faces_batch == n_meshes, "find_depth_bwd: faces_batch must be 1 or n_meshes");
	FIND_REQUIRE(rp->fov_deg > 0.f && rp->fov_deg < 180.f, "find_depth_bwd: fov_deg outside (0, 180)");
	hipStream_t s = reinterpret_cast<hipStream_t>(stream);
	depth::BwdArgs a;
	a.verts = verts; a.faces = faces; a.R = R; a.T = T; a.pix_to_face = pix_to_face; a.d_depth = d_depth; a.d_verts = d_verts;
	a.fstride = faces_batch == 1 ? 0 : n_faces * 3;
	a.M = (int)n_views; a.V = (int)n_verts; a.F = (int)n_faces; a.H = rp->image_h; a.W = rp->image_w;
	a.inv_s = tanf(rp->fov_deg * 3.14159265358979323846f / 180.0f * 0.5f);
	if (hipMemsetAsync(d_verts, 0, (size_t)(n_meshes * n_verts * 3) * sizeof(float), s) != hipSuccess) {
		(void)hipGetLastError();
		set_error("find_depth_bwd: clearing d_verts failed");
		return FIND_ELAUNCH;
	}
	const int64_t HW = (int64_t)a.H * a.W;
	hipLaunchKernelGGL(depth::depth_bwd_kernel, dim3((unsigned)cdiv(HW, depth::THREADS), (unsigned)(n_meshes * n_views)), dim3(depth::THREADS), 0, s, a);
	FIND_LAUNCH_CHECK("depth depth_bwd_kernel");
	return FIND_OK;
}

extern "C" int64_t find_depth_loss_ws_bytes(int64_t n_img, int64_t n_pix) {
	if (!depth::sizes_ok(n_img, n_pix)) {
		set_error("find_depth_loss_ws_bytes: bad sizes: %lld images of %lld pixels", (long long)n_img, (long long)n_pix);
		return -1;
	}
	return depth::ws_need(n_img, n_pix);
}

static int dloss_args(const char* who, const void* pred, const void* target, int64_t n_img, int64_t n_pix, int kind, float delta, depth::LossArgs* a) {
	if (!pred || !target) {
		set_error("%s: NULL argument", who);
		return FIND_EINVAL;
	}
	if (!depth::sizes_ok(n_img, n_pix)) {
		set_error("%s: bad sizes: %lld images of %lld pixels", who, (long long)n_img, (long long)n_pix);
		return FIND_EINVAL;
	}
	if (kind != FIND_DEPTH_L1 && kind != FIND_DEPTH_L2 && kind != FIND_DEPTH_HUBER) {
		set_error("%s: kind %d (0 = l1, 1 = l2, 2 = huber)", who, kind);
		return FIND_EINVAL;
	}
	if (kind == FIND_DEPTH_HUBER && !(delta > 0.f)) {
		set_error("%s: the Huber loss needs delta > 0", who);
		return FIND_EINVAL;
	}
	a->n_pix = n_pix; a->kind = kind; a->delta = delta;
	return FIND_OK;
}

extern "C" int find_depth_loss_fwd(const float* pred, const float* target, const float* weight, int64_t n_img, int64_t n_pix, int kind, float delta,
								   float trunc, float* loss_out, double* per_image, void* ws, int64_t ws_bytes, void* stream) {
	depth::LossArgs a;
	if (dloss_args("find_depth_loss_fwd", pred, target, n_img, n_pix, kind, delta, &a) != FIND_OK) return FIND_EINVAL;
	FIND_REQUIRE(loss_out && ws, "find_depth_loss_fwd: NULL argument");
	if (ws_bytes < depth::ws_need(n_img, n_pix) || (reinterpret_cast<uintptr_t>(ws) & 7) || (reinterpret_cast<uintptr_t>(per_image) & 7)) {
		set_error("find_depth_loss_fwd: workspace of %lld bytes, %lld needed (8-byte aligned, as per_image)", (long long)ws_bytes,
				  (long long)depth::ws_need(n_img, n_pix));
		return FIND_EWORKSPACE;
	}
	a.pred = pred; a.target = target; a.weight = weight; a.trunc = trunc;
	hipStream_t s = reinterpret_cast<hipStream_t>(stream);
	double* sums = reinterpret_cast<double*>(ws);
	double* partial = sums + 2;
	const int64_t bpi = depth::blocks_per_image(n_pix);
	const dim3 grid((unsigned)bpi, (unsigned)n_img), block(depth::THREADS);
	if (depth::aligned16(pred) && depth::aligned16(target) && depth::aligned16(weight))
		hipLaunchKernelGGL(depth::dloss_fwd_kernel<true>, grid, block, 0, s, a, partial);
	else
		hipLaunchKernelGGL(depth::dloss_fwd_kernel<false>, grid, block, 0, s, a, partial);
	FIND_LAUNCH_CHECK("depth dloss_fwd_kernel");
	hipLaunchKernelGGL(depth::dloss_sum_kernel, dim3(1), block, 0, s, (const double*)partial, n_img, bpi, sums, per_image, loss_out);
	FIND_LAUNCH_CHECK("depth dloss_sum_kernel");
	return FIND_OK;
}

extern "C" int find_depth_loss_bwd(const float* pred, const float* target, const float* weight, int64_t n_img, int64_t n_pix, int kind, float delta,
								   float trunc, const float* d_loss, const void* ws, float* d_pred, void* stream) {
	depth::LossArgs a;
	if (dloss_args("find_depth_loss_bwd", pred, target, n_img, n_pix, kind, delta, &a) != FIND_OK) return FIND_EINVAL;
	FIND_REQUIRE(d_loss && ws && d_pred, "find_depth_loss_bwd: NULL argument");
	FIND_REQUIRE(!(reinterpret_cast<uintptr_t>(ws) & 7), "find_depth_loss_bwd: the workspace of the forward (8-byte aligned) is expected");
	a.pred = pred; a.target = target; a.weight = weight; a.trunc = trunc;
	hipStream_t s = reinterpret_cast<hipStream_t>(stream);
	const double* sums = reinterpret_cast<const double*>(ws);
	const dim3 grid((unsigned)depth::blocks_per_image(n_pix), (unsigned)n_img), block(depth::THREADS);
	if (depth::aligned16(pred) && depth::aligned16(target) && depth::aligned16(weight) && depth::aligned16(d_pred))
		hipLaunchKernelGGL(depth::dloss_bwd_kernel<true>, grid, block, 0, s, a, d_loss, sums, d_pred);
	else
		hipLaunchKernelGGL(depth::dloss_bwd_kernel<false>, grid, block, 0, s, a, d_loss, sums, d_pred);
	FIND_LAUNCH_CHECK("depth dloss_bwd_kernel");
	return FIND_OK;
}
