// Exact point-to-surface distance (gfx950): for every query point the nearest closed triangle of its mesh, the barycentrics of the closest
// point and the squared distance; the gradient to the points and, through the closest point, to the vertices.  Not in the reference
// (PyTorch3D users know it as point_mesh_face_distance); find_amd.losses.SurfaceDistanceLoss and eval_3d_metrics(surface=True) use it.
//
// The search has the shape of nn_kernel (geom.hip): a lane owns PF_NQ queries in registers, the four waves of a block own the SAME
// 64 * PF_NQ queries and each scans one quarter of every face tile; a tile is staged through LDS and every lane of a wave reads the same
// face (a broadcast); the waves' results, and at small batches the results of the blocks that split the face range over blockIdx.z, are
// merged as 64-bit keys (distance bits << 32 | face): unsigned order = (distance, face), the smallest face wins among equal distances.
// Two things differ:
//  - what depends on the face alone is computed ONCE, by the thread that stages it: corner a, the edges ab = b - a and ac = c - a, their
//    dot products, and a bounding sphere (the centroid and the largest distance from it to a corner);
//  - a pair goes through the full region test only when the sphere's lower bound (|p - centre| - r)^2 can still beat the query's running
//    best: |p - centre|^2 < (r + sqrt(best))^2, nine VALU instructions; the pairs that pass are tested 64 at a time (point_face_kernel).
//    r is the distance from the ROUNDED centre to the corners, so the sphere holds the triangle whatever the centre's rounding; r and
//    sqrt(best) are both stored 1e-4 too large, a thousand times the rounding of the four operations of the bound, so the true winner
//    (and a face that ties with it) is never culled.  Every query starts from a bound: its distance to the nearest of 512 corners.
// Everything is formed relative to corner a (p - a is rounded at the size of the distance, not of the coordinates).  The winner's
// barycentrics and distance are recomputed from the winning face by a finish kernel: dist2 = |(p - a) - w1 ab - w2 ac|^2 = |p - sum w_i v_i|^2
// of exactly the barycentrics stored.  No float atomics in the forward: two runs agree bit for bit.
#include "common.h"

namespace find {
namespace surface {

constexpr int PF_TILE = 512;   // faces per tile: four float4 each, 32 KiB of the CU's 160 KiB
constexpr int PF_NQ = 2;       // queries per lane
constexpr int PF_GROUP = 4;    // faces culled between two looks at the list (PF_TILE / 4 is a multiple)
constexpr float PF_SLACK = 1.0001f;

__host__ __device__ __forceinline__ float3 ld3(const float* p) { return make_float3(p[0], p[1], p[2]); }
__host__ __device__ __forceinline__ float3 sub3(float3 a, float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
__host__ __device__ __forceinline__ float dot3(float3 a, float3 b) { return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ unsigned long long pf_key(float d, int i) { return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i; }
// (the face arithmetic below also compiles for the host: a CPU program can run the search's every step on its own data)

// (b - a) x (c - a) == 0 exactly, every product rounded on its own: fused, u.y * v.z - u.z * v.y of two equal edges is the rounding error
// of one product instead of zero, and the face (3, 7, 7) would count as a triangle
__host__ __device__ __forceinline__ bool cross_is_zero(float3 u, float3 v) {
#pragma clang fp contract(off)
	const float cx = u.y * v.z - u.z * v.y, cy = u.z * v.x - u.x * v.z, cz = u.x * v.y - u.y * v.x;
	return cx == 0.f && cy == 0.f && cz == 0.f;
}

struct Face {
	float3 a, ab, ac;
	float d00, d01, d11;   // ab.ab, ab.ac, ac.ac
};

// false: a -1 row, an index outside [0, n_verts), or a face without area -- never a candidate
__host__ __device__ __forceinline__ bool load_face(const float* __restrict__ vp, const int32_t* __restrict__ fp, int n_verts, Face& f) {
	const int i0 = fp[0], i1 = fp[1], i2 = fp[2];
	if ((unsigned)i0 >= (unsigned)n_verts || (unsigned)i1 >= (unsigned)n_verts || (unsigned)i2 >= (unsigned)n_verts) return false;
	f.a = ld3(vp + 3 * (int64_t)i0);
	f.ab = sub3(ld3(vp + 3 * (int64_t)i1), f.a);
	f.ac = sub3(ld3(vp + 3 * (int64_t)i2), f.a);
	if (cross_is_zero(f.ab, f.ac)) return false;
	f.d00 = dot3(f.ab, f.ab); f.d01 = dot3(f.ab, f.ac); f.d11 = dot3(f.ac, f.ac);
	return true;
}

// The point of the closed triangle nearest to a + ap, as a + v ab + w ac: the seven Voronoi regions (Ericson, Real-Time Collision
// Detection, 5.1.5) with the six dot products written in terms of ab.ap, ac.ap and the face's own three: ab.bp = ab.ap - ab.ab, ...
// The clamps change nothing inside a region; they keep a face thin enough for the regions to contradict each other in float32 from
// producing a weight outside [0, 1], an infinity or a NaN (fmaxf / fminf return the other operand for a NaN).
__host__ __device__ __forceinline__ void closest_vw(const Face& f, float3 ap, float& v, float& w) {
	const float d1 = dot3(f.ab, ap), d2 = dot3(f.ac, ap);
	const float d3 = d1 - f.d00, d4 = d2 - f.d01, d5 = d1 - f.d01, d6 = d2 - f.d11;
	if (d1 <= 0.f && d2 <= 0.f) { v = 0.f; w = 0.f; return; }           // corner a
	if (d3 >= 0.f && d4 <= d3) { v = 1.f; w = 0.f; return; }             // corner b
	const float vc = d1 * d4 - d3 * d2;
	if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {                            // edge ab
		v = fminf(fmaxf(d1 / (d1 - d3), 0.f), 1.f); w = 0.f; return;
	}
	if (d6 >= 0.f && d5 <= d6) { v = 0.f; w = 1.f; return; }             // corner c
	const float vb = d5 * d2 - d1 * d6;
	if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {                            // edge ac
		v = 0.f; w = fminf(fmaxf(d2 / (d2 - d6), 0.f), 1.f); return;
	}
	const float va = d3 * d6 - d5 * d4;
	if (va <= 0.f && d4 - d3 >= 0.f && d5 - d6 >= 0.f) {                  // edge bc
		w = fminf(fmaxf((d4 - d3) / ((d4 - d3) + (d5 - d6)), 0.f), 1.f); v = 1.f - w; return;
	}
	const float den = va + vb + vc;                                       // inside
	v = fminf(fmaxf(vb / den, 0.f), 1.f);
	w = fminf(fmaxf(vc / den, 0.f), 1.f - v);
}

__host__ __device__ __forceinline__ float3 offset_to(const Face& f, float3 ap, float v, float w) {   // p - (a + v ab + w ac)
	return make_float3(__builtin_fmaf(-w, f.ac.x, __builtin_fmaf(-v, f.ab.x, ap.x)), __builtin_fmaf(-w, f.ac.y, __builtin_fmaf(-v, f.ab.y, ap.y)),
					   __builtin_fmaf(-w, f.ac.z, __builtin_fmaf(-v, f.ab.z, ap.z)));
}

// The full test of one (query, face) pair that passed the cull, by whichever lane drew it from the wave's list.
__device__ __forceinline__ float pair_dist2(float4 A, float4 B, float4 C, float4 q) {
	Face f;
	f.a = make_float3(A.x, A.y, A.z); f.ab = make_float3(B.x, B.y, B.z); f.ac = make_float3(C.x, C.y, C.z);
	f.d00 = A.w; f.d01 = B.w; f.d11 = C.w;
	const float3 ap = sub3(make_float3(q.x, q.y, q.z), f.a);
	float v, w;
	closest_vw(f, ap, v, w);
	const float3 o = offset_to(f, ap, v, w);
	return dot3(o, o);
}

// grid (ceil(p_max / (64 PF_NQ)), n_meshes, splits).  key (n_meshes, p_max): plain store when splits == 1, atomicMin into a buffer preset
// to ~0 otherwise; rows at or past p_len are left to the finish kernel, which does not read their keys.
//
// The queries of a wave are surface samples in no spatial order: nearly every face passes the cull for ONE OR TWO of a wave's 128
// queries, so running the region test where the cull passed would run it for nearly every face with two lanes in sixty-four at work
// (measured so: 2.5 ms for 16 x 5000 queries x 13 776 faces).  Instead a lane whose pair passes only APPENDS it (face slot, query slot) to
// its wave's list in LDS; whenever the list holds 64 pairs, all 64 lanes take one each, run the test and merge the result into the
// wave's per-query keys with an LDS atomicMin (so the order in which pairs are drawn changes nothing); the lanes then reload their own
// running best.  A list is emptied before its tile is replaced.  Only one wave touches a list and a row of keys, and a wave's LDS
// operations execute in order: the fences below are for the compiler.  (The arrays are indexed as they are declared: through a
// pointer variable the accesses lose their address space and become flat stores, each waited for.)
__global__ __launch_bounds__(256) void point_face_kernel(const float* __restrict__ points, const int32_t* __restrict__ p_len,
														 const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t faces_mesh_stride,
														 int p_max, int n_verts, int n_faces, int splits, unsigned long long* __restrict__ key_out) {
	constexpr int NQB = 64 * PF_NQ;   // queries of a block
	__shared__ float4 sph[PF_TILE];   // centre, radius (no candidate: a centre no query is near)
	__shared__ float4 fa[PF_TILE];    // a, ab.ab
	__shared__ float4 fb[PF_TILE];    // ab, ab.ac
	__shared__ float4 fc[PF_TILE];    // ac, ac.ac
	__shared__ float4 qpos[NQB];
	__shared__ unsigned long long kbest[4][NQB];   // per wave: the running best of every query, as a key
	__shared__ unsigned pairs[4][64 + PF_GROUP * NQB];   // per wave: face slot | query slot << 16; at most 63 left over + a group's 64 PF_NQ each
	const int n = blockIdx.y, split = blockIdx.z;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int p1 = p_len ? min(max(p_len[n], 0), p_max) : p_max;
	if ((int)blockIdx.x * NQB >= p1) return;   // (the whole block: no barrier is left waiting)
	const float* pp = points + (int64_t)n * p_max * 3;
	const float* vp = verts + (int64_t)n * n_verts * 3;
	const int32_t* fp = faces + (int64_t)n * faces_mesh_stride;
	const int share = (int)(((int64_t)n_faces + splits - 1) / splits);
	const int lo = min(n_faces, split * share), hi = min(n_faces, lo + share);
	float3 q[PF_NQ];
	float reach[PF_NQ];   // sqrt(running best), rounded up
	int qi[PF_NQ];
#pragma unroll
	for (int k = 0; k < PF_NQ; ++k) {
		qi[k] = (blockIdx.x * PF_NQ + k) * 64 + lane;
		q[k] = ld3(pp + 3 * (int64_t)min(qi[k], p_max - 1));
		reach[k] = INFINITY;
		kbest[wave][k * 64 + lane] = ~0ull;
		if (wave == 0) qpos[k * 64 + lane] = make_float4(q[k].x, q[k].y, q[k].z, 0.f);
	}
	// A first bound before the search: the nearest of up to PF_TILE corners, of faces spread evenly over the mesh's whole list (a corner of a
	// candidate face lies on the surface; that face passes the cull in whichever block owns it).  Without it a query's running best shrinks
	// only as the scan comes near it, and on meshes listed ring by ring the faces of every new ring pass the cull on the way.
	float seed[PF_NQ];
	{
		const int n_seed = min(n_faces, PF_TILE), step = n_faces / max(n_seed, 1);
		for (int j = threadIdx.x; j < n_seed; j += 256) {
			Face f;
			const bool ok = load_face(vp, fp + 3 * (int64_t)j * step, n_verts, f);
			sph[j] = ok ? make_float4(f.a.x, f.a.y, f.a.z, 0.f) : make_float4(0.f, 0.f, 0.f, -1.f);
		}
		__syncthreads();
#pragma unroll
		for (int k = 0; k < PF_NQ; ++k) seed[k] = INFINITY;
		for (int j = 0; j < n_seed; ++j) {
			const float4 s = sph[j];
			if (__builtin_amdgcn_readfirstlane(__float_as_int(s.w)) < 0) continue;
#pragma unroll
			for (int k = 0; k < PF_NQ; ++k) {
				const float dx = q[k].x - s.x, dy = q[k].y - s.y, dz = q[k].z - s.z;
				seed[k] = fminf(seed[k], __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
			}
		}
#pragma unroll
		for (int k = 0; k < PF_NQ; ++k) reach[k] = seed[k] = sqrtf(seed[k]) * PF_SLACK;
	}
	int held = 0;   // pairs on the wave's list (wave-uniform)
	for (int j0 = lo; j0 < hi; j0 += PF_TILE) {
		const int cnt = min(PF_TILE, hi - j0);
		const int cnt_up = (cnt + PF_GROUP - 1) / PF_GROUP * PF_GROUP;
		__syncthreads();
		for (int j = threadIdx.x; j < cnt_up; j += 256) {
			Face f;
			if (j < cnt && load_face(vp, fp + 3 * (int64_t)(j0 + j), n_verts, f)) {
				const float3 g = make_float3((f.ab.x + f.ac.x) * (1.f / 3.f), (f.ab.y + f.ac.y) * (1.f / 3.f), (f.ab.z + f.ac.z) * (1.f / 3.f));
				const float3 ctr = make_float3(f.a.x + g.x, f.a.y + g.y, f.a.z + g.z);
				const float3 ra = sub3(f.a, ctr), rb = sub3(make_float3(f.a.x + f.ab.x, f.a.y + f.ab.y, f.a.z + f.ab.z), ctr),
							 rc = sub3(make_float3(f.a.x + f.ac.x, f.a.y + f.ac.y, f.a.z + f.ac.z), ctr);
				// (a + ab is b up to one rounding of a coordinate; the centre-sized term below covers it)
				const float r2 = fmaxf(dot3(ra, ra), fmaxf(dot3(rb, rb), dot3(rc, rc)));
				const float r = sqrtf(r2) * PF_SLACK + 1e-6f * (fabsf(ctr.x) + fabsf(ctr.y) + fabsf(ctr.z));
				sph[j] = make_float4(ctr.x, ctr.y, ctr.z, r);
				fa[j] = make_float4(f.a.x, f.a.y, f.a.z, f.d00);
				fb[j] = make_float4(f.ab.x, f.ab.y, f.ab.z, f.d01);
				fc[j] = make_float4(f.ac.x, f.ac.y, f.ac.z, f.d11);
			} else {
				// |p - centre|^2 overflows to +inf, which is below no bound, an infinite one included: never on a list
				sph[j] = make_float4(1e30f, 1e30f, 1e30f, 0.f);
			}
		}
		__syncthreads();
		const int ja = __builtin_amdgcn_readfirstlane(wave * (PF_TILE / 4));
		const int jb = __builtin_amdgcn_readfirstlane(min(cnt_up, ja + PF_TILE / 4));
		for (int j = ja; j <= jb; j += PF_GROUP) {
			// j == jb: past the wave's share of the tile -- nothing new, whatever is left on the list is tested
			if (j < jb) {
				// a group of faces at a time: one wait for their spheres, one branch when no lane has a pair among them
				float4 s[PF_GROUP];
#pragma unroll
				for (int u = 0; u < PF_GROUP; ++u) s[u] = sph[j + u];
				unsigned hits = 0;
#pragma unroll
				for (int u = 0; u < PF_GROUP; ++u) {
#pragma unroll
					for (int k = 0; k < PF_NQ; ++k) {
						const float dx = q[k].x - s[u].x, dy = q[k].y - s[u].y, dz = q[k].z - s[u].z;
						const float t = s[u].w + reach[k];
						hits |= (unsigned)(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)) < t * t) << (u * PF_NQ + k);
					}
				}
				if (__ballot(hits != 0)) {   // (wave-uniform, as is every `m` below)
#pragma unroll
					for (int u = 0; u < PF_GROUP; ++u) {
#pragma unroll
						for (int k = 0; k < PF_NQ; ++k) {
							const bool hit = (hits >> (u * PF_NQ + k)) & 1u;
							const unsigned long long m = __ballot(hit);
							if (m) {
								if (hit) pairs[wave][held + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = (unsigned)(j + u) | ((unsigned)(k * 64 + lane) << 16);
								held += __popcll(m);
							}
						}
					}
				}
			}
			const int floor_ = j < jb ? 64 : 1;   // a full wave's worth at a time; at the end the rest
			if (held < floor_) continue;
			__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
			while (held >= floor_) {
				const int take = min(held, 64);
				held -= take;
				if (lane < take) {
					const unsigned e = pairs[wave][held + lane];
					const int fj = (int)(e & 0xffffu), qs = (int)(e >> 16);
					const float d = pair_dist2(fa[fj], fb[fj], fc[fj], qpos[qs]);
					atomicMin(&kbest[wave][qs], pf_key(d, j0 + fj));
				}
			}
			__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
			// (the other waves' rows as they stand: each entry is the distance to some face, whenever it is read -- a bound that is as good)
#pragma unroll
			for (int k = 0; k < PF_NQ; ++k) {
				unsigned long long b = kbest[0][k * 64 + lane];
#pragma unroll
				for (int w = 1; w < 4; ++w) b = min(b, kbest[w][k * 64 + lane]);
				reach[k] = b == ~0ull ? seed[k] : fminf(seed[k], sqrtf(__uint_as_float((unsigned)(b >> 32))) * PF_SLACK);
			}
		}
	}
	__syncthreads();
	if (wave == 0) {
#pragma unroll
		for (int k = 0; k < PF_NQ; ++k) {
			unsigned long long b = kbest[0][k * 64 + lane];
#pragma unroll
			for (int w = 1; w < 4; ++w) b = min(b, kbest[w][k * 64 + lane]);
			if (qi[k] >= p1) continue;
			unsigned long long* o = key_out + (int64_t)n * p_max + qi[k];
			if (splits == 1) *o = b;
			else if (b != ~0ull) atomicMin(o, b);
		}
	}
}

// One thread per query: the winner's barycentrics and distance from the winning face itself.
__global__ void point_face_finish_kernel(const float* __restrict__ points, const int32_t* __restrict__ p_len, const float* __restrict__ verts,
										 const int32_t* __restrict__ faces, int64_t faces_mesh_stride, int p_max, int n_verts, int n_faces,
										 const unsigned long long* __restrict__ key, float* __restrict__ dist2, int32_t* __restrict__ idx,
										 float* __restrict__ bary) {
	const int n = blockIdx.y;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= p_max) return;
	const int64_t o = (int64_t)n * p_max + i;
	const int p1 = p_len ? p_len[n] : p_max;
	float d = 0.f, w0 = 0.f, w1 = 0.f, w2 = 0.f;
	int fi = -1;
	if (i < p1 && n_faces > 0) {
		const unsigned long long k = key[o];
		const int cand = (int)(unsigned)k;
		Face f;
		if (k != ~0ull && cand >= 0 && cand < n_faces &&
			load_face(verts + (int64_t)n * n_verts * 3, faces + (int64_t)n * faces_mesh_stride + 3 * (int64_t)cand, n_verts, f)) {
			const float3 ap = sub3(ld3(points + o * 3), f.a);
			closest_vw(f, ap, w1, w2);
			w0 = fmaxf((1.f - w1) - w2, 0.f);
			const float3 r = offset_to(f, ap, w1, w2);
			d = dot3(r, r);
			fi = cand;
		}
	}
	dist2[o] = d;
	idx[o] = fi;
	bary[o * 3 + 0] = w0; bary[o * 3 + 1] = w1; bary[o * 3 + 2] = w2;
}

// d dist2 / d p = 2 (p - c), d dist2 / d v_i = -2 w_i (p - c) with c = sum w_i v_i the closest point: the barycentrics are constants (c
// minimises the distance over the triangle: the envelope theorem).  d_points is overwritten, every row; d_verts is added to with float
// atomics (zeroed by the caller), as sample_bwd_kernel does.
__global__ void point_face_bwd_kernel(const float* __restrict__ points, const float* __restrict__ verts, const int32_t* __restrict__ faces,
									  int64_t faces_mesh_stride, const int32_t* __restrict__ idx, const float* __restrict__ bary,
									  const float* __restrict__ g, int p_max, int n_verts, int n_faces, float* __restrict__ d_points,
									  float* __restrict__ d_verts) {
	const int n = blockIdx.y;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= p_max) return;
	const int64_t o = (int64_t)n * p_max + i;
	const int fi = idx[o];
	float3 gd = make_float3(0.f, 0.f, 0.f);
	int vi[3] = {-1, -1, -1};
	float w[3] = {0.f, 0.f, 0.f};
	if (fi >= 0 && fi < n_faces) {
		const int32_t* fp = faces + (int64_t)n * faces_mesh_stride + 3 * (int64_t)fi;
		const int i0 = fp[0], i1 = fp[1], i2 = fp[2];
		if ((unsigned)i0 < (unsigned)n_verts && (unsigned)i1 < (unsigned)n_verts && (unsigned)i2 < (unsigned)n_verts) {
			const float* vp = verts + (int64_t)n * n_verts * 3;
			Face f;
			f.a = ld3(vp + 3 * (int64_t)i0);
			f.ab = sub3(ld3(vp + 3 * (int64_t)i1), f.a);
			f.ac = sub3(ld3(vp + 3 * (int64_t)i2), f.a);
			w[0] = bary[o * 3 + 0]; w[1] = bary[o * 3 + 1]; w[2] = bary[o * 3 + 2];
			const float3 r = offset_to(f, sub3(ld3(points + o * 3), f.a), w[1], w[2]);
			const float s = 2.f * g[o];
			gd = make_float3(s * r.x, s * r.y, s * r.z);
			vi[0] = i0; vi[1] = i1; vi[2] = i2;
		}
	}
	if (d_points) { d_points[o * 3 + 0] = gd.x; d_points[o * 3 + 1] = gd.y; d_points[o * 3 + 2] = gd.z; }
	if (d_verts && vi[0] >= 0) {
		float* dv = d_verts + (int64_t)n * n_verts * 3;
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			atomicAdd(dv + 3 * (int64_t)vi[c] + 0, -w[c] * gd.x);
			atomicAdd(dv + 3 * (int64_t)vi[c] + 1, -w[c] * gd.y);
			atomicAdd(dv + 3 * (int64_t)vi[c] + 2, -w[c] * gd.z);
		}
	}
}

static inline bool bad_dims(int64_t n, int64_t p, int64_t v, int64_t f) {
	return n < 0 || n >= (1 << 16) || p < 0 || p >= (1ll << 30) || v < 0 || v >= (1ll << 30) || f < 0 || f >= (1ll << 30);
}

// Blocks that split the face range of one launch: enough blocks to give every SIMD work at batch 1 (bit 8192 of find_render_switches:
// never split -- the tests' way to the unsplit path at a small batch)
static int face_splits(int64_t blocks, int64_t n_faces) {
	int splits = 1;
	if (g_raster_ablate & 8192) return splits;
	while (blocks * splits < 512 && splits < 16 && n_faces / (splits * 2) >= PF_TILE) splits *= 2;
	return splits;
}

}  // namespace surface
}  // namespace find

using namespace find;
using namespace find::surface;

extern "C" int64_t find_point_face_ws_bytes(int64_t n_meshes, int64_t n_points) {
	if (surface::bad_dims(n_meshes, n_points, 0, 0)) return -1;
	return align_up(std::max<int64_t>(n_meshes * n_points, 1) * (int64_t)sizeof(unsigned long long), 256);
}

extern "C" int find_point_face_fwd(const float* points, const int32_t* p_len, const float* verts, const int32_t* faces, int64_t faces_batch,
								   int64_t n_meshes, int64_t n_points, int64_t n_verts, int64_t n_faces, float* dist2, int32_t* idx, float* bary,
								   void* ws, int64_t ws_bytes, void* stream) {
	FIND_REQUIRE(!surface::bad_dims(n_meshes, n_points, n_verts, n_faces), "find_point_face_fwd: bad sizes");
	if (n_meshes == 0 || n_points == 0) return FIND_OK;
	FIND_REQUIRE(points && dist2 && idx && bary && ws, "find_point_face_fwd: NULL argument");
	FIND_REQUIRE((verts && faces) || n_faces == 0, "find_point_face_fwd: NULL argument");
	FIND_REQUIRE(n_verts >= 1 || n_faces == 0, "find_point_face_fwd: faces without vertices");
	FIND_REQUIRE(faces_batch == 1 || faces_batch == n_meshes, "find_point_face_fwd: faces_batch must be 1 or n_meshes");
	if (ws_bytes < find_point_face_ws_bytes(n_meshes, n_points)) { set_error("find_point_face_fwd: workspace too small"); return FIND_EWORKSPACE; }
	hipStream_t s = (hipStream_t)stream;
	unsigned long long* key = reinterpret_cast<unsigned long long*>(ws);
	const int64_t stride = faces_batch == 1 ? 0 : n_faces * 3;
	if (n_faces > 0) {
		const int64_t bx = cdiv(n_points, 64 * PF_NQ);
		const int splits = face_splits(bx * n_meshes, n_faces);
		if (splits > 1) {
			hipError_t e = hipMemsetAsync(ws, 0xff, (size_t)(n_meshes * n_points) * sizeof(unsigned long long), s);
			if (e != hipSuccess) { set_error("find_point_face_fwd: hipMemsetAsync: %s", hipGetErrorString(e)); return FIND_ELAUNCH; }
		}
		hipLaunchKernelGGL(point_face_kernel, dim3((unsigned)bx, (unsigned)n_meshes, (unsigned)splits), dim3(256), 0, s, points, p_len, verts, faces, stride,
						   (int)n_points, (int)n_verts, (int)n_faces, splits, key);
		FIND_LAUNCH_CHECK("point_face_kernel");
	}
	hipLaunchKernelGGL(point_face_finish_kernel, dim3((unsigned)cdiv(n_points, 256), (unsigned)n_meshes), dim3(256), 0, s, points, p_len, verts, faces, stride,
					   (int)n_points, (int)n_verts, (int)n_faces, key, dist2, idx, bary);
	FIND_LAUNCH_CHECK("point_face_finish_kernel");
	return FIND_OK;
}

extern "C" int find_point_face_bwd(const float* points, const float* verts, const int32_t* faces, int64_t faces_batch, const int32_t* idx,
								   const float* bary, const float* g, int64_t n_meshes, int64_t n_points, int64_t n_verts, int64_t n_faces,
								   float* d_points, float* d_verts, void* stream) {
	FIND_REQUIRE(!surface::bad_dims(n_meshes, n_points, n_verts, n_faces), "find_point_face_bwd: bad sizes");
	FIND_REQUIRE(d_points || d_verts, "find_point_face_bwd: both gradient outputs NULL");
	if (n_meshes == 0 || n_points == 0) return FIND_OK;
	FIND_REQUIRE(points && idx && bary && g, "find_point_face_bwd: NULL argument");
	FIND_REQUIRE((verts && faces) || n_faces == 0, "find_point_face_bwd: NULL argument");
	FIND_REQUIRE(faces_batch == 1 || faces_batch == n_meshes, "find_point_face_bwd: faces_batch must be 1 or n_meshes");
	hipLaunchKernelGGL(point_face_bwd_kernel, dim3((unsigned)cdiv(n_points, 256), (unsigned)n_meshes), dim3(256), 0, (hipStream_t)stream, points, verts, faces,
					   faces_batch == 1 ? (int64_t)0 : n_faces * 3, idx, bary, g, (int)n_points, (int)n_verts, (int)n_faces, d_points, d_verts);
	FIND_LAUNCH_CHECK("point_face_bwd_kernel");
	return FIND_OK;
}
