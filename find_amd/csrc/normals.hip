// Surface normals: vertex normals as PyTorch3D's Meshes.verts_normals_padded forms them, the normal-map stage behind the feature render,
// and a fused cosine loss between two normal maps.
//   vnormals_fwd_kernel   n_v = s_v / max(|s_v|, 1e-6),  s_v = sum over the faces f at v of (v1 - v0) x (v2 - v0): a GATHER over a
//                         vertex -> incident-corner table (item = face * 3 + corner, ascending per vertex), a thread per vertex, the terms
//                         added in the table's order.  render.hip's shader forms the same sums with float atomics, in whatever order they land.
//   vnormals_draw_kernel  backward, step 1: d s_v from d n_v through the normalisation ((g - n (n . g)) / |s|; g / 1e-6 under the clamp, as
//                         render.hip's normals_bwd_prepare_kernel), s_v gathered again;
//   vnormals_bwd_kernel   step 2: corner k of face f gives vertex v_k  (v_{k+1} - v_{k+2}) x G_f,  G_f = d s_{v0} + d s_{v1} + d s_{v2}: the
//                         same gather.  No atomics either way: two calls agree bit for bit.
//   nmap_fwd / _bwd       n = f / |f| (0 where |f| <= 1e-6), then n @ R[image % M] unless `world`.
//   nloss_fwd / _bwd      sum_i w_i (1 - p^_i . t^_i) / max(sum_i w_i, 1e-12): a thread takes four pixels (seven 16-byte loads when the three
//                         pointers are 16-byte aligned), one pair of double partials per workgroup, nloss_sum_kernel adds the pairs in a fixed order.
// A face with an index outside [0, V) (the -1 rows that pad ragged meshes) contributes nothing and is never read through.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "find_hip.h"
#include "common.h"

namespace find {
namespace normals {

constexpr int THREADS = 256;
constexpr int PX = 4;                 // pixels per thread of the loss kernels
constexpr float EPS = 1e-6f;

struct Tables {
	const int32_t* faces;   // (fb, F, 3)
	const int32_t* off;     // (fb, V + 1)
	const int32_t* items;   // (fb, 3 F)
	int64_t fb;
	int V, F;
};

// the three indices of face f of `fm`; false when one lies outside [0, V)
__device__ __forceinline__ bool face_of(const int32_t* __restrict__ fm, int f, int V, int& i0, int& i1, int& i2) {
	i0 = fm[3 * f]; i1 = fm[3 * f + 1]; i2 = fm[3 * f + 2];
	return (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V;
}

// s_v of vertex v: the face terms of its incident corners, in the table's order
__device__ __forceinline__ void raw_normal(const Tables& t, int mesh, int v, const float* __restrict__ vp, float s[3]) {
	const int tb = t.fb == 1 ? 0 : mesh;
	const int32_t* fm = t.faces + (int64_t)tb * t.F * 3;
	const int32_t* off = t.off + (int64_t)tb * (t.V + 1);
	const int32_t* items = t.items + (int64_t)tb * t.F * 3;
	const int b = max(off[v], 0), e = min(off[v + 1], 3 * t.F);
	s[0] = s[1] = s[2] = 0.f;
	for (int j = b; j < e; ++j) {
		const int item = items[j];
		if ((unsigned)item >= (unsigned)(3 * t.F)) continue;
		int i0, i1, i2;
		if (!face_of(fm, item / 3, t.V, i0, i1, i2)) continue;
		const float* a = vp + 3 * i0; const float* b1 = vp + 3 * i1; const float* c = vp + 3 * i2;
		const float ux = b1[0] - a[0], uy = b1[1] - a[1], uz = b1[2] - a[2];
		const float wx = c[0] - a[0], wy = c[1] - a[1], wz = c[2] - a[2];
		s[0] += uy * wz - uz * wy; s[1] += uz * wx - ux * wz; s[2] += ux * wy - uy * wx;
	}
}

__global__ __launch_bounds__(THREADS) void vnormals_fwd_kernel(const float* __restrict__ verts, const Tables t, float* __restrict__ out) {
	const int mesh = blockIdx.y, v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= t.V) return;
	float s[3];
	raw_normal(t, mesh, v, verts + (int64_t)mesh * t.V * 3, s);
	const float l = fmaxf(sqrtf(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]), EPS);
	float* o = out + ((int64_t)mesh * t.V + v) * 3;
	o[0] = s[0] / l; o[1] = s[1] / l; o[2] = s[2] / l;
}

__global__ __launch_bounds__(THREADS) void vnormals_draw_kernel(const float* __restrict__ verts, const Tables t, const float* __restrict__ d_n,
																float* __restrict__ d_raw) {
	const int mesh = blockIdx.y, v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= t.V) return;
	float s[3];
	raw_normal(t, mesh, v, verts + (int64_t)mesh * t.V * 3, s);
	const int64_t o = ((int64_t)mesh * t.V + v) * 3;
	float gx = d_n[o], gy = d_n[o + 1], gz = d_n[o + 2];
	const float len = sqrtf(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
	if (len > EPS) {
		const float ux = s[0] / len, uy = s[1] / len, uz = s[2] / len;
		const float dot = ux * gx + uy * gy + uz * gz;
		gx = (gx - ux * dot) / len; gy = (gy - uy * dot) / len; gz = (gz - uz * dot) / len;
	} else {
		gx /= EPS; gy /= EPS; gz /= EPS;
	}
	d_raw[o] = gx; d_raw[o + 1] = gy; d_raw[o + 2] = gz;
}

__global__ __launch_bounds__(THREADS) void vnormals_bwd_kernel(const float* __restrict__ verts, const Tables t, const float* __restrict__ d_raw,
															   float* __restrict__ d_verts) {
	const int mesh = blockIdx.y, v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= t.V) return;
	const int tb = t.fb == 1 ? 0 : mesh;
	const int32_t* fm = t.faces + (int64_t)tb * t.F * 3;
	const int32_t* off = t.off + (int64_t)tb * (t.V + 1);
	const int32_t* items = t.items + (int64_t)tb * t.F * 3;
	const float* vp = verts + (int64_t)mesh * t.V * 3;
	const float* dr = d_raw + (int64_t)mesh * t.V * 3;
	const int b = max(off[v], 0), e = min(off[v + 1], 3 * t.F);
	float dx = 0.f, dy = 0.f, dz = 0.f;
	for (int j = b; j < e; ++j) {
		const int item = items[j];
		if ((unsigned)item >= (unsigned)(3 * t.F)) continue;
		const int f = item / 3, k = item - 3 * f;
		int idx[3];
		if (!face_of(fm, f, t.V, idx[0], idx[1], idx[2])) continue;
		const float Gx = dr[3 * idx[0]] + dr[3 * idx[1]] + dr[3 * idx[2]];
		const float Gy = dr[3 * idx[0] + 1] + dr[3 * idx[1] + 1] + dr[3 * idx[2] + 1];
		const float Gz = dr[3 * idx[0] + 2] + dr[3 * idx[1] + 2] + dr[3 * idx[2] + 2];
		const float* p = vp + 3 * idx[k == 2 ? 0 : k + 1];
		const float* q = vp + 3 * idx[k == 0 ? 2 : k - 1];
		const float ex = p[0] - q[0], ey = p[1] - q[1], ez = p[2] - q[2];
		dx += ey * Gz - ez * Gy; dy += ez * Gx - ex * Gz; dz += ex * Gy - ey * Gx;
	}
	float* o = d_verts + ((int64_t)mesh * t.V + v) * 3;
	o[0] = dx; o[1] = dy; o[2] = dz;
}

// ------------------------------------------------------------------------------------------------ normal map
__global__ __launch_bounds__(THREADS) void nmap_fwd_kernel(const float* __restrict__ raw, const float* __restrict__ R, int64_t P, int64_t HW, int M,
														   int world, float* __restrict__ out) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= P) return;
	const float x = raw[3 * i], y = raw[3 * i + 1], z = raw[3 * i + 2];
	const float len = sqrtf(x * x + y * y + z * z);
	float ox = 0.f, oy = 0.f, oz = 0.f;
	if (len > EPS) {
		const float nx = x / len, ny = y / len, nz = z / len;
		if (world) {
			ox = nx; oy = ny; oz = nz;
		} else {
			const float* r = R + (int64_t)((i / HW) % M) * 9;
			ox = nx * r[0] + ny * r[3] + nz * r[6];
			oy = nx * r[1] + ny * r[4] + nz * r[7];
			oz = nx * r[2] + ny * r[5] + nz * r[8];
		}
	}
	out[3 * i] = ox; out[3 * i + 1] = oy; out[3 * i + 2] = oz;
}

__global__ __launch_bounds__(THREADS) void nmap_bwd_kernel(const float* __restrict__ raw, const float* __restrict__ R, const float* __restrict__ g,
														   int64_t P, int64_t HW, int M, int world, float* __restrict__ d_raw) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= P) return;
	const float x = raw[3 * i], y = raw[3 * i + 1], z = raw[3 * i + 2];
	const float len = sqrtf(x * x + y * y + z * z);
	float dx = 0.f, dy = 0.f, dz = 0.f;
	if (len > EPS) {
		const float nx = x / len, ny = y / len, nz = z / len;
		const float g0 = g[3 * i], g1 = g[3 * i + 1], g2 = g[3 * i + 2];
		float ax = g0, ay = g1, az = g2;   // d n = g @ R^T
		if (!world) {
			const float* r = R + (int64_t)((i / HW) % M) * 9;
			ax = g0 * r[0] + g1 * r[1] + g2 * r[2];
			ay = g0 * r[3] + g1 * r[4] + g2 * r[5];
			az = g0 * r[6] + g1 * r[7] + g2 * r[8];
		}
		const float dot = nx * ax + ny * ay + nz * az;
		dx = (ax - nx * dot) / len; dy = (ay - ny * dot) / len; dz = (az - nz * dot) / len;
	}
	d_raw[3 * i] = dx; d_raw[3 * i + 1] = dy; d_raw[3 * i + 2] = dz;
}

// ------------------------------------------------------------------------------------------------ normal loss
// the n <= PX pixels from `base` on: 3 n floats of p and t, n of w; VEC: the full group of four with 16-byte loads
template <bool VEC>
__device__ __forceinline__ void load_px(const float* __restrict__ p, const float* __restrict__ t, const float* __restrict__ w, int64_t base, int n,
										float pp[3 * PX], float tt[3 * PX], float ww[PX]) {
	if (VEC && n == PX) {
		const float4* p4 = reinterpret_cast<const float4*>(p + 3 * base);
		const float4* t4 = reinterpret_cast<const float4*>(t + 3 * base);
#pragma unroll
		for (int k = 0; k < 3; ++k) {
			const float4 a = p4[k], b = t4[k];
			pp[4 * k] = a.x; pp[4 * k + 1] = a.y; pp[4 * k + 2] = a.z; pp[4 * k + 3] = a.w;
			tt[4 * k] = b.x; tt[4 * k + 1] = b.y; tt[4 * k + 2] = b.z; tt[4 * k + 3] = b.w;
		}
		const float4 c = *reinterpret_cast<const float4*>(w + base);
		ww[0] = c.x; ww[1] = c.y; ww[2] = c.z; ww[3] = c.w;
		return;
	}
#pragma unroll
	for (int k = 0; k < PX; ++k) {
		const bool in = k < n;
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			pp[3 * k + c] = in ? p[3 * (base + k) + c] : 0.f;
			tt[3 * k + c] = in ? t[3 * (base + k) + c] : 0.f;
		}
		ww[k] = in ? w[base + k] : 0.f;
	}
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

template <bool VEC>
__global__ __launch_bounds__(THREADS) void nloss_fwd_kernel(const float* __restrict__ p, const float* __restrict__ t, const float* __restrict__ w,
															int64_t P, double* __restrict__ partial) {
	__shared__ double wsum[2 * THREADS / 64];
	const int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * PX;
	const int n = (int)max((int64_t)0, min((int64_t)PX, P - base));
	double num = 0.0, den = 0.0;
	if (n > 0) {
		float pp[3 * PX], tt[3 * PX], ww[PX];
		load_px<VEC>(p, t, w, base, n, pp, tt, ww);
#pragma unroll
		for (int k = 0; k < PX; ++k) {
			const float px = pp[3 * k], py = pp[3 * k + 1], pz = pp[3 * k + 2], tx = tt[3 * k], ty = tt[3 * k + 1], tz = tt[3 * k + 2];
			const float lp = sqrtf(px * px + py * py + pz * pz), lt = sqrtf(tx * tx + ty * ty + tz * tz);
			const float c = (lp > EPS && lt > EPS) ? (px * tx + py * ty + pz * tz) / (lp * lt) : 0.f;
			num += (double)(ww[k] * (1.f - c));   // (a pixel past the end has weight 0)
			den += (double)ww[k];
		}
	}
	block_sum2(num, den, wsum);
	if (threadIdx.x == 0) {
		partial[2 * (int64_t)blockIdx.x] = num;
		partial[2 * (int64_t)blockIdx.x + 1] = den;
	}
}

// sums[0] = sum of the numerators, sums[1] = sum of the weights, *loss = sums[0] / max(sums[1], 1e-12): thread t adds the pairs t, t + 256, ...
__global__ __launch_bounds__(THREADS) void nloss_sum_kernel(const double* __restrict__ partial, int64_t n, double* __restrict__ sums,
															float* __restrict__ loss_out) {
	__shared__ double wsum[2 * THREADS / 64];
	double a = 0.0, b = 0.0;
	for (int64_t i = threadIdx.x; i < n; i += THREADS) {
		a += partial[2 * i];
		b += partial[2 * i + 1];
	}
	block_sum2(a, b, wsum);
	if (threadIdx.x == 0) {
		sums[0] = a;
		sums[1] = b;
		*loss_out = (float)(a / fmax(b, 1e-12));
	}
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void nloss_bwd_kernel(const float* __restrict__ p, const float* __restrict__ t, const float* __restrict__ w,
															int64_t P, const float* __restrict__ d_loss, const double* __restrict__ sums,
															float* __restrict__ d_p) {
	const int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * PX;
	const int n = (int)max((int64_t)0, min((int64_t)PX, P - base));
	if (n <= 0) return;
	const float scale = (float)(-(double)*d_loss / fmax(sums[1], 1e-12));
	float pp[3 * PX], tt[3 * PX], ww[PX], dd[3 * PX];
	load_px<VEC>(p, t, w, base, n, pp, tt, ww);
#pragma unroll
	for (int k = 0; k < PX; ++k) {
		const float px = pp[3 * k], py = pp[3 * k + 1], pz = pp[3 * k + 2], tx = tt[3 * k], ty = tt[3 * k + 1], tz = tt[3 * k + 2];
		const float lp = sqrtf(px * px + py * py + pz * pz), lt = sqrtf(tx * tx + ty * ty + tz * tz);
		float dx = 0.f, dy = 0.f, dz = 0.f;
		if (lp > EPS && lt > EPS) {
			const float ux = px / lp, uy = py / lp, uz = pz / lp, vx = tx / lt, vy = ty / lt, vz = tz / lt;
			const float c = ux * vx + uy * vy + uz * vz;
			const float s = scale * ww[k] / lp;
			dx = s * (vx - c * ux); dy = s * (vy - c * uy); dz = s * (vz - c * uz);
		}
		dd[3 * k] = dx; dd[3 * k + 1] = dy; dd[3 * k + 2] = dz;
	}
	if (VEC && n == PX) {
		float4* o = reinterpret_cast<float4*>(d_p + 3 * base);
#pragma unroll
		for (int k = 0; k < 3; ++k) o[k] = make_float4(dd[4 * k], dd[4 * k + 1], dd[4 * k + 2], dd[4 * k + 3]);
	} else {
		for (int k = 0; k < 3 * n; ++k) d_p[3 * base + k] = dd[k];
	}
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int64_t loss_blocks(int64_t P) { return cdiv(P, (int64_t)THREADS * PX); }

}  // namespace normals
}  // namespace find

using namespace find;

static int vnormals_args(const char* who, const void* verts, const int32_t* faces, int64_t faces_batch, const int32_t* vf_off, const int32_t* vf_items,
						 int64_t N, int64_t V, int64_t F, normals::Tables* t) {
	if (!verts || !faces || !vf_off || !vf_items) {
		set_error("%s: NULL argument", who);
		return FIND_EINVAL;
	}
	if (!(N >= 1 && N < 65536 && V >= 1 && V < ((int64_t)1 << 28) && F >= 1 && F < ((int64_t)1 << 28) && (faces_batch == 1 || faces_batch == N))) {
		set_error("%s: bad sizes N=%lld V=%lld F=%lld faces_batch=%lld (1 or N)", who, (long long)N, (long long)V, (long long)F, (long long)faces_batch);
		return FIND_EINVAL;
	}
	t->faces = faces; t->off = vf_off; t->items = vf_items; t->fb = faces_batch; t->V = (int)V; t->F = (int)F;
	return FIND_OK;
}

extern "C" int find_vertex_normals_fwd(const float* verts, const int32_t* faces, int64_t faces_batch, const int32_t* vf_off, const int32_t* vf_items,
									   int64_t N, int64_t V, int64_t F, float* normals_out, void* stream) {
	normals::Tables t;
	if (vnormals_args("find_vertex_normals_fwd", verts, faces, faces_batch, vf_off, vf_items, N, V, F, &t) != FIND_OK) return FIND_EINVAL;
	FIND_REQUIRE(normals_out, "find_vertex_normals_fwd: NULL argument");
	hipLaunchKernelGGL(normals::vnormals_fwd_kernel, dim3((unsigned)cdiv(V, normals::THREADS), (unsigned)N), dim3(normals::THREADS), 0,
					   reinterpret_cast<hipStream_t>(stream), verts, t, normals_out);
	FIND_LAUNCH_CHECK("normals vnormals_fwd_kernel");
	return FIND_OK;
}

extern "C" int find_vertex_normals_bwd(const float* verts, const int32_t* faces, int64_t faces_batch, const int32_t* vf_off, const int32_t* vf_items,
									   int64_t N, int64_t V, int64_t F, const float* d_normals, float* d_raw_ws, float* d_verts, void* stream) {
	normals::Tables t;
	if (vnormals_args("find_vertex_normals_bwd", verts, faces, faces_batch, vf_off, vf_items, N, V, F, &t) != FIND_OK) return FIND_EINVAL;
	FIND_REQUIRE(d_normals && d_raw_ws && d_verts, "find_vertex_normals_bwd: NULL argument");
	hipStream_t s = reinterpret_cast<hipStream_t>(stream);
	const dim3 grid((unsigned)cdiv(V, normals::THREADS), (unsigned)N), block(normals::THREADS);
	hipLaunchKernelGGL(normals::vnormals_draw_kernel, grid, block, 0, s, verts, t, d_normals, d_raw_ws);
	FIND_LAUNCH_CHECK("normals vnormals_draw_kernel");
	hipLaunchKernelGGL(normals::vnormals_bwd_kernel, grid, block, 0, s, verts, t, (const float*)d_raw_ws, d_verts);
	FIND_LAUNCH_CHECK("normals vnormals_bwd_kernel");
	return FIND_OK;
}

static int nmap_args(const char* who, const void* raw, const void* R, const void* out, int64_t n_images, int64_t n_views, int64_t H, int64_t W, int world) {
	if (!raw || !out || (!world && !R)) {
		set_error("%s: NULL argument", who);
		return FIND_EINVAL;
	}
	if (!(n_images >= 1 && n_views >= 1 && n_views < (1 << 20) && n_images % n_views == 0 && H >= 1 && W >= 1 && H < (1 << 15) && W < (1 << 15)
		  && n_images * H * W < ((int64_t)1 << 36))) {
		set_error("%s: bad sizes: %lld images (a multiple of the %lld views) of %lldx%lld", who, (long long)n_images, (long long)n_views, (long long)H,
				  (long long)W);
		return FIND_EINVAL;
	}
	return FIND_OK;
}

extern "C" int find_normal_map_fwd(const float* raw, const float* R, int64_t n_images, int64_t n_views, int64_t H, int64_t W, int world, float* out,
								   void* stream) {
	if (nmap_args("find_normal_map_fwd", raw, R, out, n_images, n_views, H, W, world) != FIND_OK) return FIND_EINVAL;
	const int64_t P = n_images * H * W;
	hipLaunchKernelGGL(normals::nmap_fwd_kernel, dim3((unsigned)cdiv(P, normals::THREADS)), dim3(normals::THREADS), 0, reinterpret_cast<hipStream_t>(stream),
					   raw, R, P, H * W, (int)n_views, world, out);
	FIND_LAUNCH_CHECK("normals nmap_fwd_kernel");
	return FIND_OK;
}

extern "C" int find_normal_map_bwd(const float* raw, const float* R, const float* d_out, int64_t n_images, int64_t n_views, int64_t H, int64_t W,
								   int world, float* d_raw, void* stream) {
	if (nmap_args("find_normal_map_bwd", raw, R, d_raw, n_images, n_views, H, W, world) != FIND_OK) return FIND_EINVAL;
	FIND_REQUIRE(d_out, "find_normal_map_bwd: NULL argument");
	const int64_t P = n_images * H * W;
	hipLaunchKernelGGL(normals::nmap_bwd_kernel, dim3((unsigned)cdiv(P, normals::THREADS)), dim3(normals::THREADS), 0, reinterpret_cast<hipStream_t>(stream),
					   raw, R, d_out, P, H * W, (int)n_views, world, d_raw);
	FIND_LAUNCH_CHECK("normals nmap_bwd_kernel");
	return FIND_OK;
}

extern "C" int64_t find_normal_loss_ws_bytes(int64_t P) {
	if (P < 1 || P >= ((int64_t)1 << 36)) {
		set_error("find_normal_loss_ws_bytes: bad size P=%lld", (long long)P);
		return -1;
	}
	return (2 + 2 * normals::loss_blocks(P)) * (int64_t)sizeof(double);
}

extern "C" int find_normal_loss_fwd(const float* pred, const float* target, const float* weight, int64_t P, float* loss_out, void* ws, int64_t ws_bytes,
									void* stream) {
	FIND_REQUIRE(pred && target && weight && loss_out && ws, "find_normal_loss_fwd: NULL argument");
	FIND_REQUIRE(P >= 1 && P < ((int64_t)1 << 36), "find_normal_loss_fwd: bad size P=%lld", (long long)P);
	const int64_t blocks = normals::loss_blocks(P);
	if (ws_bytes < (2 + 2 * blocks) * (int64_t)sizeof(double) || (reinterpret_cast<uintptr_t>(ws) & 7)) {
		set_error("find_normal_loss_fwd: workspace of %lld bytes, %lld needed (8-byte aligned)", (long long)ws_bytes,
				  (long long)((2 + 2 * blocks) * (int64_t)sizeof(double)));
		return FIND_EWORKSPACE;
	}
	hipStream_t s = reinterpret_cast<hipStream_t>(stream);
	double* sums = reinterpret_cast<double*>(ws);
	double* partial = sums + 2;
	if (normals::aligned16(pred) && normals::aligned16(target) && normals::aligned16(weight))
		hipLaunchKernelGGL(normals::nloss_fwd_kernel<true>, dim3((unsigned)blocks), dim3(normals::THREADS), 0, s, pred, target, weight, P, partial);
	else
		hipLaunchKernelGGL(normals::nloss_fwd_kernel<false>, dim3((unsigned)blocks), dim3(normals::THREADS), 0, s, pred, target, weight, P, partial);
	FIND_LAUNCH_CHECK("normals nloss_fwd_kernel");
	hipLaunchKernelGGL(normals::nloss_sum_kernel, dim3(1), dim3(normals::THREADS), 0, s, (const double*)partial, blocks, sums, loss_out);
	FIND_LAUNCH_CHECK("normals nloss_sum_kernel");
	return FIND_OK;
}

extern "C" int find_normal_loss_bwd(const float* pred, const float* target, const float* weight, int64_t P, const float* d_loss, const void* ws,
									float* d_pred, void* stream) {
	FIND_REQUIRE(pred && target && weight && d_loss && ws && d_pred, "find_normal_loss_bwd: NULL argument");
	FIND_REQUIRE(P >= 1 && P < ((int64_t)1 << 36), "find_normal_loss_bwd: bad size P=%lld", (long long)P);
	FIND_REQUIRE(!(reinterpret_cast<uintptr_t>(ws) & 7), "find_normal_loss_bwd: the workspace of the forward (8-byte aligned) is expected");
	hipStream_t s = reinterpret_cast<hipStream_t>(stream);
	const int64_t blocks = normals::loss_blocks(P);
	const double* sums = reinterpret_cast<const double*>(ws);
	if (normals::aligned16(pred) && normals::aligned16(target) && normals::aligned16(weight) && normals::aligned16(d_pred))
		hipLaunchKernelGGL(normals::nloss_bwd_kernel<true>, dim3((unsigned)blocks), dim3(normals::THREADS), 0, s, pred, target, weight, P, d_loss, sums, d_pred);
	else
		hipLaunchKernelGGL(normals::nloss_bwd_kernel<false>, dim3((unsigned)blocks), dim3(normals::THREADS), 0, s, pred, target, weight, P, d_loss, sums, d_pred);
	FIND_LAUNCH_CHECK("normals nloss_bwd_kernel");
	return FIND_OK;
}
