// Ray casting against triangle meshes (gfx950): for every ray the closest hit -- t, the face, the barycentrics -- or whether anything is hit
// at all, by the watertight pair test of raycast_math.h (Woop, Benthin & Wald 2013).  Not in the reference; find_amd.rays builds vertex
// visibility and ambient occlusion on it, find_amd.bake an AO map.
//
// The pass has the shape of winding_kernel (winding.hip): a lane owns RC_NQ rays in registers (origin, direction, e1, e2, d . d, the ray's
// upper bound, its skip face and its running key), the four waves of a block own the SAME 64 * RC_NQ rays, a tile of RC_TILE faces (three
// float4 each: a corner and, in the first, whether the face counts) is staged through LDS and every lane of a wave reads the same face (a
// broadcast); wave k scans the k-th quarter of the tile.  Every (ray, face) pair is evaluated -- no cull, no BVH: per pair nine
// subtractions, 30 multiplies and adds for the six projected coordinates, nine for the edge functions and their signs' six comparisons;
// the distance and the key only for the pairs that pass the inside test.
//
// Results are 64-bit keys, t bits << 32 | face, merged by integer minimum: in registers per lane, through LDS over the four waves, and --
// when the face range is split over blockIdx.z at a small N * R -- by atomicMin into a buffer preset to ~0.  A minimum does not depend on
// its order, so two runs agree bit for bit and a row does not depend on N, R, its position or the split; there is no float atomic in the
// forward.  ray_finish_kernel writes t, idx and bary (or hit) from the winning key, the barycentrics from the winning face itself.
//
// any_hit: the same kernel with an early exit -- after every tile the four waves pool which rays have hit, a ray that has hit stops
// testing, and the block stops walking tiles when all of its rays have hit or are dead.  Every wave forms that decision from the same
// LDS words, so it is block-uniform and no barrier is left waiting.
#include "common.h"
#include "raycast_math.h"

namespace find {
namespace raycast {

constexpr int RC_NQ = 2;   // rays per lane
constexpr int RC_MAX_SPLITS = 16;
constexpr int RC_SPLIT_BELOW_BLOCKS = 1024;   // (face_splits)

__device__ __forceinline__ bool load_corners(const float* __restrict__ vp, const int32_t* __restrict__ f, int n_verts, float4& A, float4& B, float4& C) {
	const int i0 = f[0], i1 = f[1], i2 = f[2];
	if (!((unsigned)i0 < (unsigned)n_verts && (unsigned)i1 < (unsigned)n_verts && (unsigned)i2 < (unsigned)n_verts)) return false;
	const float *a = vp + 3 * (int64_t)i0, *b = vp + 3 * (int64_t)i1, *c = vp + 3 * (int64_t)i2;
	A = make_float4(a[0], a[1], a[2], 1.f);
	B = make_float4(b[0], b[1], b[2], 0.f);
	C = make_float4(c[0], c[1], c[2], 0.f);
	return true;
}

// grid (ceil(r_max / (64 RC_NQ)), n_meshes, splits).  key (n_meshes, r_max): plain store when splits == 1, atomicMin into a buffer preset
// to ~0 otherwise; rows at or past r_len are left to the finish kernel, which does not read their keys.
template <bool ANY>
__global__ __launch_bounds__(256) void ray_kernel(const float* __restrict__ origins, const float* __restrict__ dirs, const int32_t* __restrict__ r_len,
												  const int32_t* __restrict__ skip, const float* __restrict__ verts, const int32_t* __restrict__ faces,
												  int64_t faces_mesh_stride, int r_max, int n_verts, int n_faces, int splits, float t_min, float t_max,
												  unsigned long long* __restrict__ key_out) {
	constexpr int NQB = 64 * RC_NQ;
	__shared__ float4 fa[RC_TILE];   // a, and 1.f / 0.f: the face counts / does not (a -1 row, an index outside [0, n_verts))
	__shared__ float4 fb[RC_TILE];
	__shared__ float4 fc[RC_TILE];
	__shared__ unsigned long long kbest[4][NQB];   // per wave: its best key for every ray of the block
	const int n = blockIdx.y, split = blockIdx.z;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int r1 = r_len ? min(max(r_len[n], 0), r_max) : r_max;
	const int q0 = blockIdx.x * NQB;
	if (q0 >= r1) return;   // (the whole block: no barrier is left waiting)
	const float* op = origins + (int64_t)n * r_max * 3;
	const float* dp = dirs + (int64_t)n * r_max * 3;
	const float* vp = verts + (int64_t)n * n_verts * 3;
	const int32_t* fp = faces + (int64_t)n * faces_mesh_stride;
	const int share = (int)(((int64_t)n_faces + splits - 1) / splits);
	const int lo = min(n_faces, split * share), hi = min(n_faces, lo + share);
	Frame fr[RC_NQ];
	float t_hi[RC_NQ];   // t_max, or -1 for a ray that tests nothing (more): dead, past r_len, or -- any_hit -- already hit
	int sk[RC_NQ], qi[RC_NQ];
	unsigned long long best[RC_NQ];
#pragma unroll
	for (int k = 0; k < RC_NQ; ++k) {
		qi[k] = q0 + k * 64 + lane;
		const int64_t r = (int64_t)min(qi[k], r_max - 1);
		const float *o = op + 3 * r, *d = dp + 3 * r;
		fr[k] = ray_frame(o[0], o[1], o[2], d[0], d[1], d[2]);
		t_hi[k] = (fr[k].live && qi[k] < r1) ? t_max : -1.f;
		sk[k] = skip ? skip[(int64_t)n * r_max + r] : -1;
		best[k] = ~0ull;
	}
	for (int j0 = lo; j0 < hi; j0 += RC_TILE) {
		const int cnt = min(RC_TILE, hi - j0);
		// (the barrier that ends the tile before, after every wave's last read of the faces, is also this staging's)
		for (int j = threadIdx.x; j < cnt; j += 256) {
			float4 A, B, C;
			if (load_corners(vp, fp + 3 * (int64_t)(j0 + j), n_verts, A, B, C)) {
				fa[j] = A; fb[j] = B; fc[j] = C;
			} else {
				fa[j] = make_float4(0.f, 0.f, 0.f, 0.f);
			}
		}
		__syncthreads();
		const int ja = __builtin_amdgcn_readfirstlane(wave * RC_SUB);
		const int jb = __builtin_amdgcn_readfirstlane(min(cnt, ja + RC_SUB));
		for (int j = ja; j < jb; ++j) {
			const float4 A = fa[j];
			if (__builtin_amdgcn_readfirstlane(__float_as_int(A.w)) == 0) continue;   // (wave-uniform: every lane reads the same face)
			const float4 B = fb[j], C = fc[j];
#pragma unroll
			for (int k = 0; k < RC_NQ; ++k) {
				Hit h;
				if (pair_test(A.x - fr[k].ox, A.y - fr[k].oy, A.z - fr[k].oz, B.x - fr[k].ox, B.y - fr[k].oy, B.z - fr[k].oz, C.x - fr[k].ox, C.y - fr[k].oy,
							  C.z - fr[k].oz, fr[k].e1x, fr[k].e1y, fr[k].e1z, fr[k].e2x, fr[k].e2y, fr[k].e2z, fr[k].dx, fr[k].dy, fr[k].dz, fr[k].dd, t_min,
							  t_hi[k], h) &&
					j0 + j != sk[k])
					best[k] = min(best[k], hit_key(h.t, j0 + j));
			}
		}
		if (ANY) {
			// pool the hits of the four waves: the same words read by every wave, so `done` is the same in all four
#pragma unroll
			for (int k = 0; k < RC_NQ; ++k) kbest[wave][k * 64 + lane] = best[k];
			__syncthreads();
			bool done = true;
#pragma unroll
			for (int k = 0; k < RC_NQ; ++k) {
#pragma unroll
				for (int u = 0; u < 4; ++u) best[k] = min(best[k], kbest[u][k * 64 + lane]);
				if (best[k] != ~0ull) t_hi[k] = -1.f;
				done = done && t_hi[k] < 0.f;
			}
			if (__all(done)) break;   // (block-uniform)
			// (kbest is written again only behind the next tile's first barrier, which every wave reaches after these reads)
		} else {
			__syncthreads();
		}
	}
	if (!ANY) {
#pragma unroll
		for (int k = 0; k < RC_NQ; ++k) kbest[wave][k * 64 + lane] = best[k];
		__syncthreads();
	}
	if (wave == 0) {
#pragma unroll
		for (int k = 0; k < RC_NQ; ++k) {
			unsigned long long b = best[k];
			if (!ANY) {
#pragma unroll
				for (int u = 1; u < 4; ++u) b = min(b, kbest[u][k * 64 + lane]);
			}
			if (qi[k] >= r1) continue;
			unsigned long long* o = key_out + (int64_t)n * r_max + qi[k];
			if (splits == 1) *o = b;
			else if (b != ~0ull) atomicMin(o, b);
		}
	}
}

// One thread per ray: t from the winning key, the barycentrics from the winning face itself (the pair test again: the same bits).
// have_keys == 0: a mesh list without faces, every row a miss.  hit != NULL: the any_hit call, which writes hit alone.
__global__ void ray_finish_kernel(const float* __restrict__ origins, const float* __restrict__ dirs, const int32_t* __restrict__ r_len,
								  const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t faces_mesh_stride, int r_max, int n_verts,
								  int n_faces, int have_keys, const unsigned long long* __restrict__ key, float* __restrict__ t, int32_t* __restrict__ idx,
								  float* __restrict__ bary, uint8_t* __restrict__ hit) {
	const int n = blockIdx.y;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= r_max) return;
	const int64_t o = (int64_t)n * r_max + i;
	const int r1 = r_len ? r_len[n] : r_max;
	float tt = INFINITY, w0 = 0.f, w1 = 0.f, w2 = 0.f;
	int fi = -1;
	if (i < r1 && have_keys) {
		const unsigned long long k = key[o];
		const int cand = (int)(unsigned)k;
		if (k != ~0ull && cand >= 0 && cand < n_faces) {
			fi = cand;
			tt = key_time(k);
			if (!hit) {
				float4 A, B, C;
				Hit h;
				const Frame f = ray_frame(origins[o * 3], origins[o * 3 + 1], origins[o * 3 + 2], dirs[o * 3], dirs[o * 3 + 1], dirs[o * 3 + 2]);
				// (the interval is left open here: the key says the pair passed it)
				if (load_corners(verts + (int64_t)n * n_verts * 3, faces + (int64_t)n * faces_mesh_stride + 3 * (int64_t)cand, n_verts, A, B, C) &&
					pair_test(A.x - f.ox, A.y - f.oy, A.z - f.oz, B.x - f.ox, B.y - f.oy, B.z - f.oz, C.x - f.ox, C.y - f.oy, C.z - f.oz, f.e1x, f.e1y, f.e1z,
							  f.e2x, f.e2y, f.e2z, f.dx, f.dy, f.dz, f.dd, -INFINITY, INFINITY, h)) {
					w0 = h.u; w1 = h.v; w2 = h.w;
				}
			}
		}
	}
	if (hit) {
		hit[o] = fi >= 0 ? 1 : 0;
		return;
	}
	t[o] = tt;
	idx[o] = fi;
	bary[o * 3 + 0] = w0; bary[o * 3 + 1] = w1; bary[o * 3 + 2] = w2;
}

// With n = (b - a) x (c - a), g = n . d and w the stored barycentrics: dt/do = -n / g, dt/dd = -t n / g, dt/dv_i = w_i n / g (the hit
// point o + t d = sum w_i v_i stays on the face's plane; the face and the barycentrics are constants).  d_origins and d_dirs are
// overwritten, every row (0 for a miss, and where g == 0); d_verts is added to with float atomics (zeroed by the caller), as
// point_face_bwd_kernel does.
__global__ void ray_bwd_kernel(const float* __restrict__ dirs, const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t faces_mesh_stride,
							   const int32_t* __restrict__ idx, const float* __restrict__ bary, const float* __restrict__ t, const float* __restrict__ d_t,
							   int r_max, int n_verts, int n_faces, float* __restrict__ d_origins, float* __restrict__ d_dirs, float* __restrict__ d_verts) {
	const int n = blockIdx.y;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= r_max) return;
	const int64_t o = (int64_t)n * r_max + i;
	const int fi = idx[o];
	float gx = 0.f, gy = 0.f, gz = 0.f, tt = 0.f;   // d_t n / g
	int vi[3] = {-1, -1, -1};
	float4 A, B, C;
	if (fi >= 0 && fi < n_faces) {
		const int32_t* fp = faces + (int64_t)n * faces_mesh_stride + 3 * (int64_t)fi;
		if (load_corners(verts + (int64_t)n * n_verts * 3, fp, n_verts, A, B, C)) {
			const float ux = B.x - A.x, uy = B.y - A.y, uz = B.z - A.z, vx = C.x - A.x, vy = C.y - A.y, vz = C.z - A.z;
			const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
			const float g = nx * dirs[o * 3] + ny * dirs[o * 3 + 1] + nz * dirs[o * 3 + 2];
			tt = t[o];
			if (g != 0.f && fabsf(tt) <= 3.4028234663852886e38f) {
				const float s = d_t[o] / g;
				gx = s * nx; gy = s * ny; gz = s * nz;
				vi[0] = fp[0]; vi[1] = fp[1]; vi[2] = fp[2];
			}
		}
	}
	if (d_origins) { d_origins[o * 3 + 0] = -gx; d_origins[o * 3 + 1] = -gy; d_origins[o * 3 + 2] = -gz; }
	if (d_dirs) { d_dirs[o * 3 + 0] = vi[0] >= 0 ? -tt * gx : 0.f; d_dirs[o * 3 + 1] = vi[0] >= 0 ? -tt * gy : 0.f; d_dirs[o * 3 + 2] = vi[0] >= 0 ? -tt * gz : 0.f; }
	if (d_verts && vi[0] >= 0) {
		float* dv = d_verts + (int64_t)n * n_verts * 3;
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			const float w = bary[o * 3 + c];
			atomicAdd(dv + 3 * (int64_t)vi[c] + 0, w * gx);
			atomicAdd(dv + 3 * (int64_t)vi[c] + 1, w * gy);
			atomicAdd(dv + 3 * (int64_t)vi[c] + 2, w * gz);
		}
	}
}

static inline bool bad_dims(int64_t n, int64_t r, int64_t v, int64_t f) {
	return n < 0 || n >= (1 << 16) || r < 0 || r >= (1ll << 30) || v < 0 || v >= (1ll << 30) || f < 0 || f >= (1ll << 30);
}

// Blocks that split the face range of one launch: at a small N * R the rays alone give the chip too few blocks (it holds about 1280 of
// these at once).  Every piece keeps at least two tiles.  Bit 8192 of find_render_switches: never split -- the tests' way to the unsplit
// path at a small batch, as for find_point_face_fwd.
static int face_splits(int64_t blocks, int64_t n_faces) {
	int splits = 1;
	if (g_raster_ablate & 8192) return splits;
	while (blocks * splits < RC_SPLIT_BELOW_BLOCKS && splits < RC_MAX_SPLITS && n_faces / (splits * 2) >= 2 * RC_TILE) splits *= 2;
	return splits;
}

// The last launch of find_ray_fwd and of find_ray_bvh_fwd (bvh.hip): t, idx, bary -- or hit alone when hit != NULL -- from the keys.
int ray_finish_launch(const float* origins, const float* dirs, const int32_t* r_len, const float* verts, const int32_t* faces, int64_t faces_mesh_stride,
					  int64_t n_meshes, int64_t n_rays, int64_t n_verts, int64_t n_faces, const unsigned long long* key, float* t, int32_t* idx, float* bary,
					  uint8_t* hit, void* stream) {
	hipLaunchKernelGGL(ray_finish_kernel, dim3((unsigned)cdiv(n_rays, 256), (unsigned)n_meshes), dim3(256), 0, (hipStream_t)stream, origins, dirs, r_len, verts,
					   faces, faces_mesh_stride, (int)n_rays, (int)n_verts, (int)n_faces, n_faces > 0 ? 1 : 0, key, t, idx, bary, hit);
	FIND_LAUNCH_CHECK("ray_finish_kernel");
	return FIND_OK;
}

}  // namespace raycast
}  // namespace find

using namespace find;
using namespace find::raycast;

extern "C" int64_t find_ray_ws_bytes(int64_t n_meshes, int64_t n_rays, int64_t n_faces) {
	if (raycast::bad_dims(n_meshes, n_rays, 0, n_faces)) return -1;
	return align_up(std::max<int64_t>(n_meshes * n_rays, 1) * (int64_t)sizeof(unsigned long long), 256);
}

extern "C" int find_ray_fwd(const float* origins, const float* dirs, const int32_t* r_len, const int32_t* skip, const float* verts, const int32_t* faces,
							int64_t faces_batch, int64_t n_meshes, int64_t n_rays, int64_t n_verts, int64_t n_faces, float t_min, float t_max, int any_hit,
							float* t, int32_t* idx, float* bary, uint8_t* hit, void* ws, int64_t ws_bytes, void* stream) {
	FIND_REQUIRE(!raycast::bad_dims(n_meshes, n_rays, n_verts, n_faces), "find_ray_fwd: bad sizes");
	FIND_REQUIRE(t_min >= 0.f, "find_ray_fwd: t_min must be >= 0 (and not NaN)");
	FIND_REQUIRE(!(t_max != t_max), "find_ray_fwd: t_max is NaN");
	FIND_REQUIRE(any_hit == 0 || any_hit == 1, "find_ray_fwd: any_hit must be 0 or 1");
	if (n_meshes == 0 || n_rays == 0) return FIND_OK;
	FIND_REQUIRE(origins && dirs && ws, "find_ray_fwd: NULL argument");
	FIND_REQUIRE(any_hit ? hit != nullptr : (t && idx && bary), "find_ray_fwd: NULL argument");
	FIND_REQUIRE((verts && faces) || n_faces == 0, "find_ray_fwd: NULL argument");
	FIND_REQUIRE(n_verts >= 1 || n_faces == 0, "find_ray_fwd: faces without vertices");
	FIND_REQUIRE(faces_batch == 1 || faces_batch == n_meshes, "find_ray_fwd: faces_batch must be 1 or n_meshes");
	if (ws_bytes < find_ray_ws_bytes(n_meshes, n_rays, n_faces)) { set_error("find_ray_fwd: workspace too small"); return FIND_EWORKSPACE; }
	hipStream_t s = (hipStream_t)stream;
	unsigned long long* key = reinterpret_cast<unsigned long long*>(ws);
	const int64_t stride = faces_batch == 1 ? 0 : n_faces * 3;
	if (n_faces > 0) {
		const int64_t bx = cdiv(n_rays, 64 * RC_NQ);
		const int splits = face_splits(bx * n_meshes, n_faces);
		if (splits > 1) {
			hipError_t e = hipMemsetAsync(ws, 0xff, (size_t)(n_meshes * n_rays) * sizeof(unsigned long long), s);
			if (e != hipSuccess) { set_error("find_ray_fwd: hipMemsetAsync: %s", hipGetErrorString(e)); return FIND_ELAUNCH; }
		}
		const dim3 grid((unsigned)bx, (unsigned)n_meshes, (unsigned)splits);
		if (any_hit)
			hipLaunchKernelGGL(ray_kernel<true>, grid, dim3(256), 0, s, origins, dirs, r_len, skip, verts, faces, stride, (int)n_rays, (int)n_verts, (int)n_faces,
							   splits, t_min, t_max, key);
		else
			hipLaunchKernelGGL(ray_kernel<false>, grid, dim3(256), 0, s, origins, dirs, r_len, skip, verts, faces, stride, (int)n_rays, (int)n_verts, (int)n_faces,
							   splits, t_min, t_max, key);
		FIND_LAUNCH_CHECK("ray_kernel");
	}
	return ray_finish_launch(origins, dirs, r_len, verts, faces, stride, n_meshes, n_rays, n_verts, n_faces, key, t, idx, bary, any_hit ? hit : (uint8_t*)nullptr, stream);
}

extern "C" int find_ray_bwd(const float* origins, const float* dirs, const float* verts, const int32_t* faces, int64_t faces_batch, const int32_t* idx,
							const float* bary, const float* t, const float* d_t, int64_t n_meshes, int64_t n_rays, int64_t n_verts, int64_t n_faces,
							float* d_origins, float* d_dirs, float* d_verts, void* stream) {
	FIND_REQUIRE(!raycast::bad_dims(n_meshes, n_rays, n_verts, n_faces), "find_ray_bwd: bad sizes");
	FIND_REQUIRE(d_origins || d_dirs || d_verts, "find_ray_bwd: every gradient output NULL");
	if (n_meshes == 0 || n_rays == 0) return FIND_OK;
	FIND_REQUIRE(origins && dirs && idx && bary && t && d_t, "find_ray_bwd: NULL argument");
	FIND_REQUIRE((verts && faces) || n_faces == 0, "find_ray_bwd: NULL argument");
	FIND_REQUIRE(faces_batch == 1 || faces_batch == n_meshes, "find_ray_bwd: faces_batch must be 1 or n_meshes");
	hipLaunchKernelGGL(ray_bwd_kernel, dim3((unsigned)cdiv(n_rays, 256), (unsigned)n_meshes), dim3(256), 0, (hipStream_t)stream, dirs, verts, faces,
					   faces_batch == 1 ? (int64_t)0 : n_faces * 3, idx, bary, t, d_t, (int)n_rays, (int)n_verts, (int)n_faces, d_origins, d_dirs, d_verts);
	FIND_LAUNCH_CHECK("ray_bwd_kernel");
	return FIND_OK;
}
