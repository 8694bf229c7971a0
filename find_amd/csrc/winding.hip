// Generalised winding numbers (gfx950; Jacobson, Kavan & Sorkine-Hornung 2013): for every query point the sum over the faces of its mesh of
// the solid angle the face subtends there, over 4 pi -- 1 inside an outward-oriented closed mesh, 0 outside, and a smooth field that
// closes the hole of an open one about flat at w = 0.5.  Not in the reference; find_amd.inside builds inside tests, a signed distance, occupancy
// grids, grid volumes and the volumetric IoU on it.
//
// The pass has the shape of point_face_kernel (surface.hip) without its cull: a lane owns WN_NQ queries in registers, the four waves of a
// block own the SAME 64 * WN_NQ queries, a tile of WN_TILE faces (three float4 each: a corner and, in the first, whether the face counts) is
// staged through LDS and every lane of a wave reads the same face (a broadcast); wave k takes the k-th quarter of the tile, which is one
// sub-chunk of WN_SUB faces.  Every (query, face) pair is evaluated (winding_math.h: solid_angle), so the inner loop is VALU and transcendental
// work: per pair nine subtractions, 9 + 9 + 14 + 5 multiply-adds for the three lengths, the three dot products, det (unfused, see there) and den,
// three square roots, an atan2f (a reciprocal, an eleven-term polynomial, the quadrant fix-ups) and a conversion and an addition in double.
//
// Sums: in double, no atomics, in the order winding_math.h: ordered_sum writes down -- sub-chunks of 128 faces in face order, the eight
// sub-chunks of a chunk of 1024 faces in their order, the chunks in their order, each level from 0.0 (a sub-chunk past the end adds 0.0,
// which changes no bit).  A block of the unsplit path walks all chunks; at a small N * P the chunks are spread over blockIdx.z, each block
// stores its chunk's sum (n_meshes, n_chunks, n_points doubles of workspace) and a finish kernel adds them in chunk order: the same additions
// of the same doubles.  So two runs agree bit for bit, and a row's value does not depend on N, P, its position or the split.
#include "common.h"
#include "winding_math.h"

namespace find {
namespace winding {

constexpr int WN_TILE = 512;   // faces per tile: 4 waves x WN_SUB, 24 KiB of LDS
constexpr int WN_NQ = 2;       // queries per lane
constexpr int WN_MAX_SPLIT_CHUNKS = 64;
constexpr int WN_SPLIT_BELOW_BLOCKS = 2048;   // (splits_by_size)
static_assert(WN_TILE == 4 * WN_SUB && WN_CHUNK % WN_TILE == 0, "a wave's quarter of a tile is one sub-chunk");

// grid (ceil(p_max / (64 WN_NQ)), n_meshes, split ? n_chunks : 1).  Unsplit: w (n_meshes, p_max) is written, every row of the block (0 at
// or past p_len).  Split: part (n_meshes, n_chunks, p_max), rows below p_len only; winding_finish_kernel writes w.
__global__ __launch_bounds__(256) void winding_kernel(const float* __restrict__ points, const int32_t* __restrict__ p_len, const float* __restrict__ verts,
													  const int32_t* __restrict__ faces, int64_t faces_mesh_stride, int p_max, int n_verts, int n_faces,
													  int n_chunks, int split, float* __restrict__ w, double* __restrict__ part) {
	constexpr int NQB = 64 * WN_NQ;
	__shared__ float4 fa[WN_TILE];   // a, and 1.f / 0.f: the face counts / does not (a -1 row, an index outside [0, n_verts))
	__shared__ float4 fb[WN_TILE];
	__shared__ float4 fc[WN_TILE];
	__shared__ double sub[4][NQB];   // per wave: its sub-chunk's sum for every query of the block
	const int n = blockIdx.y;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int p1 = p_len ? min(max(p_len[n], 0), p_max) : p_max;
	const int q0 = blockIdx.x * NQB;
	if (q0 >= p1) {   // (the whole block: no barrier is left waiting)
		if (!split)
			for (int i = q0 + (int)threadIdx.x; i < min(q0 + NQB, p_max); i += 256) w[(int64_t)n * p_max + i] = 0.f;
		return;
	}
	const float* pp = points + (int64_t)n * p_max * 3;
	const float* vp = verts + (int64_t)n * n_verts * 3;
	const int32_t* fp = faces + (int64_t)n * faces_mesh_stride;
	float qx[WN_NQ], qy[WN_NQ], qz[WN_NQ];
	int qi[WN_NQ];
	double total[WN_NQ];
#pragma unroll
	for (int k = 0; k < WN_NQ; ++k) {
		qi[k] = q0 + k * 64 + lane;
		const float* q = pp + 3 * (int64_t)min(qi[k], p_max - 1);
		qx[k] = q[0]; qy[k] = q[1]; qz[k] = q[2];
		total[k] = 0.;
	}
	const int c_lo = split ? (int)blockIdx.z : 0, c_hi = split ? c_lo + 1 : n_chunks;
	for (int c = c_lo; c < c_hi; ++c) {
		double chunk[WN_NQ];
#pragma unroll
		for (int k = 0; k < WN_NQ; ++k) chunk[k] = 0.;
		for (int t = 0; t < WN_CHUNK / WN_TILE; ++t) {
			const int j0 = c * WN_CHUNK + t * WN_TILE;
			if (j0 >= n_faces) break;   // (block-uniform)
			const int cnt = min(WN_TILE, n_faces - j0);
			// (the barrier that ends the tile before, after every wave's last read of the faces, is also this staging's)
			for (int j = threadIdx.x; j < cnt; j += 256) {
				const int32_t* f = fp + 3 * (int64_t)(j0 + j);
				const int i0 = f[0], i1 = f[1], i2 = f[2];
				if ((unsigned)i0 < (unsigned)n_verts && (unsigned)i1 < (unsigned)n_verts && (unsigned)i2 < (unsigned)n_verts) {
					const float *a = vp + 3 * (int64_t)i0, *b = vp + 3 * (int64_t)i1, *cc = vp + 3 * (int64_t)i2;
					fa[j] = make_float4(a[0], a[1], a[2], 1.f);
					fb[j] = make_float4(b[0], b[1], b[2], 0.f);
					fc[j] = make_float4(cc[0], cc[1], cc[2], 0.f);
				} else {
					fa[j] = make_float4(0.f, 0.f, 0.f, 0.f);
				}
			}
			__syncthreads();
			const int ja = __builtin_amdgcn_readfirstlane(wave * WN_SUB);
			const int jb = __builtin_amdgcn_readfirstlane(min(cnt, ja + WN_SUB));
			double s[WN_NQ];
#pragma unroll
			for (int k = 0; k < WN_NQ; ++k) s[k] = 0.;
			for (int j = ja; j < jb; ++j) {
				const float4 A = fa[j];
				if (__builtin_amdgcn_readfirstlane(__float_as_int(A.w)) == 0) continue;   // (wave-uniform: every lane reads the same face)
				const float4 B = fb[j], C = fc[j];
#pragma unroll
				for (int k = 0; k < WN_NQ; ++k)
					s[k] += (double)solid_angle(A.x - qx[k], A.y - qy[k], A.z - qz[k], B.x - qx[k], B.y - qy[k], B.z - qz[k], C.x - qx[k], C.y - qy[k],
												C.z - qz[k]);
			}
#pragma unroll
			for (int k = 0; k < WN_NQ; ++k) sub[wave][k * 64 + lane] = s[k];
			__syncthreads();
			// every wave adds the four sub-chunks in their order, for the queries all four share: the same value in every wave
#pragma unroll
			for (int k = 0; k < WN_NQ; ++k) {
#pragma unroll
				for (int u = 0; u < 4; ++u) chunk[k] += sub[u][k * 64 + lane];
			}
			// (sub is written again only behind the next tile's first barrier, which every wave reaches after these reads)
		}
#pragma unroll
		for (int k = 0; k < WN_NQ; ++k) {
			if (split) {
				if (wave == 0 && qi[k] < p1) part[((int64_t)n * n_chunks + c) * p_max + qi[k]] = chunk[k];
			} else {
				total[k] += chunk[k];
			}
		}
	}
	if (!split && wave == 0) {
#pragma unroll
		for (int k = 0; k < WN_NQ; ++k)
			if (qi[k] < p_max) w[(int64_t)n * p_max + qi[k]] = qi[k] < p1 ? to_winding(total[k]) : 0.f;
	}
}

// One thread per query: the chunks' sums in chunk order (n_chunks == 0: a mesh without faces, every row 0).
__global__ void winding_finish_kernel(const int32_t* __restrict__ p_len, int p_max, int n_chunks, const double* __restrict__ part, float* __restrict__ w) {
	const int n = blockIdx.y;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= p_max) return;
	const int p1 = p_len ? p_len[n] : p_max;
	double total = 0.;
	if (i < p1)
		for (int c = 0; c < n_chunks; ++c) total += part[((int64_t)n * n_chunks + c) * p_max + i];
	w[(int64_t)n * p_max + i] = i < p1 ? to_winding(total) : 0.f;
}

static inline bool bad_dims(int64_t n, int64_t p, int64_t v, int64_t f) {
	return n < 0 || n >= (1 << 16) || p < 0 || p >= (1ll << 30) || v < 0 || v >= (1ll << 30) || f < 0 || f >= (1ll << 30);
}

// The chunks go to blocks of their own when the queries alone give the chip fewer than 2048 blocks.  The chip holds 1280 at once (5 per CU by
// registers, a wave per SIMD each); 16 x 5000 points are 640 blocks, two or three waves per SIMD between barriers, and ran at 235 G pairs/s
// unsplit against 362 G for a 128^3 grid.  Bit 8192 of find_render_switches: never -- the tests' way to the unsplit path at a small batch, as for find_point_face_fwd.
static bool splits_by_size(int64_t n_meshes, int64_t n_points, int64_t n_faces) {
	const int64_t chunks = cdiv(n_faces, WN_CHUNK);
	return cdiv(n_points, 64 * WN_NQ) * n_meshes < WN_SPLIT_BELOW_BLOCKS && chunks >= 2 && chunks <= WN_MAX_SPLIT_CHUNKS;
}

}  // namespace winding
}  // namespace find

using namespace find;
using namespace find::winding;

extern "C" int64_t find_winding_ws_bytes(int64_t n_meshes, int64_t n_points, int64_t n_faces) {
	if (winding::bad_dims(n_meshes, n_points, 0, n_faces)) return -1;
	if (!splits_by_size(n_meshes, n_points, n_faces)) return 256;
	return align_up(n_meshes * cdiv(n_faces, WN_CHUNK) * n_points * (int64_t)sizeof(double), 256);
}

extern "C" int find_winding_fwd(const float* points, const int32_t* p_len, const float* verts, const int32_t* faces, int64_t faces_batch, int64_t n_meshes,
								int64_t n_points, int64_t n_verts, int64_t n_faces, float* w, void* ws, int64_t ws_bytes, void* stream) {
	FIND_REQUIRE(!winding::bad_dims(n_meshes, n_points, n_verts, n_faces), "find_winding_fwd: bad sizes");
	if (n_meshes == 0 || n_points == 0) return FIND_OK;
	FIND_REQUIRE(points && w && ws, "find_winding_fwd: NULL argument");
	FIND_REQUIRE((verts && faces) || n_faces == 0, "find_winding_fwd: NULL argument");
	FIND_REQUIRE(n_verts >= 1 || n_faces == 0, "find_winding_fwd: faces without vertices");
	FIND_REQUIRE(faces_batch == 1 || faces_batch == n_meshes, "find_winding_fwd: faces_batch must be 1 or n_meshes");
	if (ws_bytes < find_winding_ws_bytes(n_meshes, n_points, n_faces)) { set_error("find_winding_fwd: workspace too small"); return FIND_EWORKSPACE; }
	hipStream_t s = (hipStream_t)stream;
	const int64_t stride = faces_batch == 1 ? 0 : n_faces * 3;
	const int n_chunks = (int)cdiv(n_faces, WN_CHUNK);
	const bool split = splits_by_size(n_meshes, n_points, n_faces) && !(g_raster_ablate & 8192);
	double* part = reinterpret_cast<double*>(ws);
	if (n_faces > 0) {
		hipLaunchKernelGGL(winding_kernel, dim3((unsigned)cdiv(n_points, 64 * WN_NQ), (unsigned)n_meshes, split ? (unsigned)n_chunks : 1u), dim3(256), 0, s, points,
						   p_len, verts, faces, stride, (int)n_points, (int)n_verts, (int)n_faces, n_chunks, split ? 1 : 0, w, part);
		FIND_LAUNCH_CHECK("winding_kernel");
	}
	if (split || n_faces == 0) {
		hipLaunchKernelGGL(winding_finish_kernel, dim3((unsigned)cdiv(n_points, 256), (unsigned)n_meshes), dim3(256), 0, s, p_len, (int)n_points, n_chunks, part, w);
		FIND_LAUNCH_CHECK("winding_finish_kernel");
	}
	return FIND_OK;
}
