// Baking into UV maps: which face owns a texel, and where an uncovered texel copies from (find_hip.h: find_uv_raster, find_uv_dilate_map).
//   raster_faces_kernel   a wave per face and slice (blockIdx.y): the face's bounding box in texels, clamped to the map, is walked in 8 x 8
//                         tiles, a texel per lane; a lane whose texel centre lies in the closed triangle takes atomicMin(face[texel], f).
//                         The map is preset to INT32_MAX; the minimum does not depend on the order of the atomics.  The waves of the
//                         SLICES slices of a face take its tiles round robin: a face of one tile costs fifteen waves that read it and leave,
//                         two faces that cover a 4096^2 map are rastered by 32 waves instead of 2.
//   raster_finish_kernel  a texel per lane: INT32_MAX -> -1, and the barycentrics of the winner, edge function over signed area.
//   dilate_kernel         a 16 x 16 block of texels with a halo of `pad`: the coverage flags go to LDS, a lane per texel scans its window in
//                         row-major order and keeps the first strict minimum of di^2 + dj^2: ties fall to the smallest flat index.
// Every product and difference of the edge functions rounds on its own (no contraction): the face pass and the finish pass form the same
// numbers, and so does a float32 restatement off the device.  A face with an index out of range is never read through.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "find_hip.h"
#include "common.h"

namespace find {
namespace bake {

constexpr int THREADS = 256;
constexpr int SLICES = 16;           // waves that share the tiles of one face
constexpr int32_t EMPTY = 0x7fffffff;
constexpr int DT = 16;               // the dilate kernel's block of texels is DT x DT
constexpr int MAX_PAD = 16;
constexpr int MAX_SIDE = 4096;

struct RasterArgs {
	const float* uv;         // (Vt, 2)
	const int32_t* faces;    // (F, 3)
	int32_t* face;           // (H, W)
	float* bary;             // (H, W, 3)
	int64_t F;
	int Vt, H, W;
};

struct Tri {
	float x0, y0, x1, y1, x2, y2, area;
};

// the UV triangle of face f; false for a face the rules skip
__device__ __forceinline__ bool load_tri(const RasterArgs& a, int64_t f, Tri& t) {
#pragma clang fp contract(off)
	const int32_t* fp = a.faces + 3 * f;
	const int i0 = fp[0], i1 = fp[1], i2 = fp[2];
	if ((unsigned)i0 >= (unsigned)a.Vt || (unsigned)i1 >= (unsigned)a.Vt || (unsigned)i2 >= (unsigned)a.Vt) return false;
	t.x0 = a.uv[2 * (int64_t)i0]; t.y0 = a.uv[2 * (int64_t)i0 + 1];
	t.x1 = a.uv[2 * (int64_t)i1]; t.y1 = a.uv[2 * (int64_t)i1 + 1];
	t.x2 = a.uv[2 * (int64_t)i2]; t.y2 = a.uv[2 * (int64_t)i2 + 1];
	t.area = (t.x1 - t.x0) * (t.y2 - t.y0) - (t.y1 - t.y0) * (t.x2 - t.x0);
	return t.area != 0.f && t.area == t.area;
}

// the three edge functions at the centre of texel (i, j): w_k / area is the barycentric of corner k
__device__ __forceinline__ void edges(const RasterArgs& a, const Tri& t, int i, int j, float w[3]) {
#pragma clang fp contract(off)
	const float px = (float)j / (float)(a.W - 1);
	const float py = 1.0f - (float)i / (float)(a.H - 1);
	w[0] = (t.x2 - t.x1) * (py - t.y1) - (t.y2 - t.y1) * (px - t.x1);
	w[1] = (t.x0 - t.x2) * (py - t.y2) - (t.y0 - t.y2) * (px - t.x2);
	w[2] = (t.x1 - t.x0) * (py - t.y0) - (t.y1 - t.y0) * (px - t.x0);
}

// grid (faces / 4, SLICES)
__global__ __launch_bounds__(THREADS) void raster_faces_kernel(const RasterArgs a) {
	const int64_t f = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	if (f >= a.F) return;
	Tri t;
	if (!load_tri(a, f, t)) return;
	// the box, one texel wider than the triangle on every side (the products below are off by far less), clamped in float: a UV may be
	// anything, an infinity included
	const float wm = (float)(a.W - 1), hm = (float)(a.H - 1);
	const float umin = fminf(t.x0, fminf(t.x1, t.x2)), umax = fmaxf(t.x0, fmaxf(t.x1, t.x2));
	const float vmin = fminf(t.y0, fminf(t.y1, t.y2)), vmax = fmaxf(t.y0, fmaxf(t.y1, t.y2));
	const int j0 = (int)fminf(fmaxf(ceilf(umin * wm) - 1.f, 0.f), (float)a.W);
	const int j1 = (int)fminf(fmaxf(floorf(umax * wm) + 1.f, -1.f), (float)(a.W - 1));
	const int i0 = (int)fminf(fmaxf(ceilf((1.0f - vmax) * hm) - 1.f, 0.f), (float)a.H);
	const int i1 = (int)fminf(fmaxf(floorf((1.0f - vmin) * hm) + 1.f, -1.f), (float)(a.H - 1));
	if (j1 < j0 || i1 < i0) return;
	const int tx = (j1 - j0 + 8) >> 3, ty = (i1 - i0 + 8) >> 3;
	const int n_tiles = tx * ty;   // at most 512 x 512
	const bool pos = t.area > 0.f;
	for (int tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
		const int by = tile / tx, bx = tile - by * tx;
		const int i = i0 + 8 * by + (lane >> 3), j = j0 + 8 * bx + (lane & 7);
		if (i > i1 || j > j1) continue;   // (0 <= i0 <= i <= i1 <= H - 1, and the same for j)
		float w[3];
		edges(a, t, i, j, w);
		const bool in = pos ? (w[0] >= 0.f && w[1] >= 0.f && w[2] >= 0.f) : (w[0] <= 0.f && w[1] <= 0.f && w[2] <= 0.f);
		if (!in) continue;
		int32_t* slot = a.face + (int64_t)i * a.W + j;
		if (*slot > (int32_t)f) atomicMin(slot, (int32_t)f);   // (a stale read is only ever too large: the atomic decides)
	}
}

__global__ __launch_bounds__(THREADS) void raster_finish_kernel(const RasterArgs a) {
	const int64_t at = (int64_t)blockIdx.x * THREADS + threadIdx.x;
	if (at >= (int64_t)a.H * a.W) return;
	const int32_t f = a.face[at];
	float b[3] = {0.f, 0.f, 0.f};
	Tri t;
	if (f >= 0 && (int64_t)f < a.F && load_tri(a, f, t)) {
		const int i = (int)(at / a.W), j = (int)(at - (int64_t)i * a.W);
		float w[3];
		edges(a, t, i, j, w);
#pragma unroll
		for (int k = 0; k < 3; ++k) b[k] = w[k] / t.area;
	} else {
		a.face[at] = -1;
	}
#pragma unroll
	for (int k = 0; k < 3; ++k) a.bary[3 * at + k] = b[k];
}

// grid (W / DT, H / DT), a texel per thread
__global__ __launch_bounds__(DT * DT) void dilate_kernel(const int32_t* __restrict__ face, int H, int W, int pad, int32_t* __restrict__ src) {
	__shared__ unsigned char cov[(DT + 2 * MAX_PAD) * (DT + 2 * MAX_PAD)];
	const int side = DT + 2 * pad;
	const int i_lo = blockIdx.y * DT - pad, j_lo = blockIdx.x * DT - pad;
	for (int k = threadIdx.x; k < side * side; k += DT * DT) {
		const int r = k / side, c = k - r * side;
		const int i = i_lo + r, j = j_lo + c;
		cov[k] = (i >= 0 && i < H && j >= 0 && j < W) ? (unsigned char)(face[(int64_t)i * W + j] >= 0) : (unsigned char)0;
	}
	__syncthreads();
	const int ti = threadIdx.x / DT, tj = threadIdx.x - ti * DT;
	const int i = blockIdx.y * DT + ti, j = blockIdx.x * DT + tj;
	if (i >= H || j >= W) return;
	const unsigned char* mine = cov + (ti + pad) * side + (tj + pad);
	int out = i * W + j;   // (H W <= 2^24)
	if (!*mine) {
		int best = 0x7fffffff;
		out = -1;
		for (int di = -pad; di <= pad; ++di) {
			const int d = di * di;
			if (d >= best) {   // no texel of this row is strictly nearer; below the centre the rows only get farther
				if (di > 0) break;
				continue;
			}
			const unsigned char* row = mine + di * side;
			for (int dj = -pad; dj <= pad; ++dj) {
				const int d2 = d + dj * dj;
				if (row[dj] && d2 < best) {
					best = d2;
					out = (i + di) * W + (j + dj);
				}
			}
		}
	}
	src[(int64_t)i * W + j] = out;
}

inline bool side_ok(int64_t n) { return n >= 2 && n <= MAX_SIDE; }

}  // namespace bake
}  // namespace find

using namespace find;

extern "C" int find_uv_raster(const float* verts_uvs, int64_t n_uv_verts, const int32_t* faces_uvs, int64_t n_faces, int64_t map_h, int64_t map_w,
							  int32_t* face, float* bary, void* stream) {
	FIND_REQUIRE(face && bary, "find_uv_raster: NULL argument");
	FIND_REQUIRE(bake::side_ok(map_h) && bake::side_ok(map_w), "find_uv_raster: map size %lld x %lld out of range (2 .. %d)", (long long)map_h,
				 (long long)map_w, bake::MAX_SIDE);
	FIND_REQUIRE(n_faces >= 0 && n_faces < (1ll << 30) && n_uv_verts >= 0 && n_uv_verts < (1ll << 31), "find_uv_raster: bad sizes Vt=%lld F=%lld",
				 (long long)n_uv_verts, (long long)n_faces);
	FIND_REQUIRE(n_faces == 0 || (faces_uvs && (verts_uvs || n_uv_verts == 0)), "find_uv_raster: NULL argument");
	hipStream_t s = reinterpret_cast<hipStream_t>(stream);
	bake::RasterArgs a;
	a.uv = verts_uvs; a.faces = faces_uvs; a.face = face; a.bary = bary;
	a.F = n_faces; a.Vt = (int)n_uv_verts; a.H = (int)map_h; a.W = (int)map_w;
	const int64_t HW = map_h * map_w;
	if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(face), bake::EMPTY, (size_t)HW, s) != hipSuccess) {
		(void)hipGetLastError();
		set_error("find_uv_raster: presetting the face map failed");
		return FIND_ELAUNCH;
	}
	if (n_faces > 0) {
		hipLaunchKernelGGL(bake::raster_faces_kernel, dim3((unsigned)cdiv(n_faces, bake::THREADS / 64), bake::SLICES), dim3(bake::THREADS), 0, s, a);
		FIND_LAUNCH_CHECK("bake raster_faces_kernel");
	}
	hipLaunchKernelGGL(bake::raster_finish_kernel, dim3((unsigned)cdiv(HW, bake::THREADS)), dim3(bake::THREADS), 0, s, a);
	FIND_LAUNCH_CHECK("bake raster_finish_kernel");
	return FIND_OK;
}

extern "C" int find_uv_dilate_map(const int32_t* face, int64_t map_h, int64_t map_w, int64_t pad, int32_t* src, void* stream) {
	FIND_REQUIRE(face && src, "find_uv_dilate_map: NULL argument");
	FIND_REQUIRE(bake::side_ok(map_h) && bake::side_ok(map_w), "find_uv_dilate_map: map size %lld x %lld out of range (2 .. %d)", (long long)map_h,
				 (long long)map_w, bake::MAX_SIDE);
	FIND_REQUIRE(pad >= 0 && pad <= bake::MAX_PAD, "find_uv_dilate_map: pad %lld out of range (0 .. %d)", (long long)pad, bake::MAX_PAD);
	hipStream_t s = reinterpret_cast<hipStream_t>(stream);
	hipLaunchKernelGGL(bake::dilate_kernel, dim3((unsigned)cdiv(map_w, bake::DT), (unsigned)cdiv(map_h, bake::DT)), dim3(bake::DT * bake::DT), 0, s, face,
					   (int)map_h, (int)map_w, (int)pad, src);
	FIND_LAUNCH_CHECK("bake dilate_kernel");
	return FIND_OK;
}
