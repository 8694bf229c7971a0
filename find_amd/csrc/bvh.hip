// A bounding-volume hierarchy over a mesh's faces for ray queries (gfx950): keys, build, refit, and the culled closest / any hit.  Not in
// the reference.  The layout, the keys and the conservative ray / box test are bvh_math.h's; the pair test, the merge key and the last
// launch are raycast.hip's, so find_ray_bvh_fwd gives find_ray_fwd's bits: a box is skipped only when no pair inside it can be accepted,
// every accepted pair merges hit_key(t, face) by integer minimum, and a minimum does not depend on the order of the walk.
//
// Build: find_bvh_keys reduces the box of the valid faces' centroid sums in two passes without atomics (BVH_HEAD_BLOCKS partial boxes per
// mesh in the structure's head, reduced again by every block of the key pass) and writes morton << 32 | face; the CALLER sorts each row;
// find_bvh_build stores the order and calls the refit: a thread per leaf forms its box from the faces it holds, then one launch per level
// forms the inner boxes bottom-up, a thread per node from its four children.  Validity is decided from the data at hand -- the index range,
// finite corners -- in the leaf pass and again in the walk, never from the key, so a refit with other vertices is exact whatever the order.
//
// Walk: a lane owns one ray.  At an inner node it reads the four child boxes (128 contiguous bytes), tests them, keeps the mask of those
// that may hold a hit in a 64-bit register, four bits per level (at most 14 levels below the root at F < 2^30), and descends into the
// lowest set bit; at a leaf it runs the pair test on the BVH_LEAF faces; with no bit left it climbs.  Node indices are computed, the
// stack is that one register: no LDS, no scratch, no atomics, no barrier.  any_hit stops at the first accepted pair.
#include "common.h"
#include "bvh_math.h"
#include "raycast_math.h"

namespace find {
namespace bvh {

static_assert(BVH_LEAF == FIND_BVH_LEAF && BVH_ARITY == FIND_BVH_ARITY && BVH_ARITY == 4, "find_hip.h and bvh_math.h disagree");

using raycast::Frame;
using raycast::Hit;

static inline bool bad_dims(int64_t n, int64_t r, int64_t v, int64_t f) {
	return n < 0 || n >= (1 << 16) || r < 0 || r >= (1ll << 30) || v < 0 || v >= (1ll << 30) || f < 0 || f >= (1ll << 30);
}

// The corners of face f of a mesh, or false: a -1 row, an index outside [0, n_verts), a non-finite corner.
__device__ __forceinline__ bool load_tri(const float* __restrict__ vp, const int32_t* __restrict__ fp, int f, int n_verts, float a[3], float b[3], float c[3]) {
	const int32_t* p = fp + 3 * (int64_t)f;
	const int i0 = p[0], i1 = p[1], i2 = p[2];
	if (!((unsigned)i0 < (unsigned)n_verts && (unsigned)i1 < (unsigned)n_verts && (unsigned)i2 < (unsigned)n_verts)) return false;
	const float *pa = vp + 3 * (int64_t)i0, *pb = vp + 3 * (int64_t)i1, *pc = vp + 3 * (int64_t)i2;
	a[0] = pa[0]; a[1] = pa[1]; a[2] = pa[2];
	b[0] = pb[0]; b[1] = pb[1]; b[2] = pb[2];
	c[0] = pc[0]; c[1] = pc[1]; c[2] = pc[2];
	return finite_tri(a, b, c);
}

struct Mesh {   // the parts of one mesh's structure
	float* head;
	int32_t* order;
	float4* boxes;
};
__host__ __device__ inline Mesh mesh_of(void* bvh, int64_t mesh_bytes, int depth, int n) {
	char* p = reinterpret_cast<char*>(bvh) + (int64_t)n * mesh_bytes;
	Mesh m;
	m.head = reinterpret_cast<float*>(p);
	m.order = reinterpret_cast<int32_t*>(p + bvh_head_bytes());
	m.boxes = reinterpret_cast<float4*>(p + bvh_head_bytes() + bvh_order_bytes(depth));
	return m;
}

__device__ __forceinline__ void wave_box(Box& b) {
#pragma unroll
	for (int k = 0; k < 3; ++k) {
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) {
			b.lo[k] = fminf(b.lo[k], __shfl_xor(b.lo[k], o, 64));
			b.hi[k] = fmaxf(b.hi[k], __shfl_xor(b.hi[k], o, 64));
		}
	}
}

// grid (BVH_HEAD_BLOCKS, n_meshes), 256 threads: block x writes the box of the centroid sums of its share of the valid faces to head[8 x ..].
__global__ __launch_bounds__(256) void centroid_box_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t faces_mesh_stride,
															int n_verts, int n_faces, void* bvh, int64_t mesh_bytes, int depth) {
	__shared__ float part[4][6];
	const int n = blockIdx.y;
	const float* vp = verts + (int64_t)n * n_verts * 3;
	const int32_t* fp = faces + (int64_t)n * faces_mesh_stride;
	Box box = box_empty();
	for (int f = blockIdx.x * 256 + threadIdx.x; f < n_faces; f += BVH_HEAD_BLOCKS * 256) {
		float a[3], b[3], c[3], s[3];
		if (!load_tri(vp, fp, f, n_verts, a, b, c)) continue;
		centroid3(a, b, c, s);
		box_point(box, s);
	}
	wave_box(box);
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (lane == 0) {
#pragma unroll
		for (int k = 0; k < 3; ++k) { part[wave][k] = box.lo[k]; part[wave][3 + k] = box.hi[k]; }
	}
	__syncthreads();
	if (threadIdx.x < 6) {
		float x = part[0][threadIdx.x];
		for (int w = 1; w < 4; ++w) x = threadIdx.x < 3 ? fminf(x, part[w][threadIdx.x]) : fmaxf(x, part[w][threadIdx.x]);
		mesh_of(bvh, mesh_bytes, depth, n).head[8 * blockIdx.x + threadIdx.x] = x;
	}
}

// grid (ceil(n_faces / 256), n_meshes): every block reduces the partial boxes again (the same min / max in every block), a thread per face
// writes its key.
__global__ __launch_bounds__(256) void keys_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t faces_mesh_stride, int n_verts,
													int n_faces, const void* bvh, int64_t mesh_bytes, int depth, unsigned long long* __restrict__ keys) {
	__shared__ float whole[6];
	const int n = blockIdx.y;
	if (threadIdx.x < 64) {
		const float* head = mesh_of(const_cast<void*>(bvh), mesh_bytes, depth, n).head;
		Box box;
		static_assert(BVH_HEAD_BLOCKS == 64, "a lane per partial box");
#pragma unroll
		for (int k = 0; k < 3; ++k) { box.lo[k] = head[8 * threadIdx.x + k]; box.hi[k] = head[8 * threadIdx.x + 3 + k]; }
		wave_box(box);
		if (threadIdx.x == 0) {
#pragma unroll
			for (int k = 0; k < 3; ++k) { whole[k] = box.lo[k]; whole[3 + k] = box.hi[k]; }
		}
	}
	__syncthreads();
	const int f = blockIdx.x * 256 + threadIdx.x;
	if (f >= n_faces) return;
	float a[3], b[3], c[3], s[3];
	uint32_t hi = BVH_INVALID_HI;
	if (load_tri(verts + (int64_t)n * n_verts * 3, faces + (int64_t)n * faces_mesh_stride, f, n_verts, a, b, c)) {
		const float lo3[3] = {whole[0], whole[1], whole[2]}, hi3[3] = {whole[3], whole[4], whole[5]};
		centroid3(a, b, c, s);
		hi = morton30(s[0], s[1], s[2], lo3, hi3);
	}
	keys[(int64_t)n * n_faces + f] = face_key(hi, f);
}

// grid (ceil(slots / 256), n_meshes): order[i] = the face of the i-th sorted key, -1 behind the last face.
__global__ void order_kernel(const unsigned long long* __restrict__ keys, int n_faces, int64_t slots, void* bvh, int64_t mesh_bytes, int depth) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= slots) return;
	const int n = blockIdx.y;
	mesh_of(bvh, mesh_bytes, depth, n).order[i] = i < n_faces ? (int32_t)(uint32_t)keys[(int64_t)n * n_faces + i] : -1;
}

__device__ __forceinline__ void store_box(float4* boxes, int64_t node, const Box& b) {
	boxes[2 * node] = make_float4(b.lo[0], b.lo[1], b.lo[2], 0.f);
	boxes[2 * node + 1] = make_float4(b.hi[0], b.hi[1], b.hi[2], 0.f);
}

// grid (ceil(leaves / 256), n_meshes): the box of every leaf from the faces it holds.
__global__ void leaf_box_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t faces_mesh_stride, int n_verts, int n_faces,
								void* bvh, int64_t mesh_bytes, int depth) {
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= bvh_leaf_count(depth)) return;
	const int n = blockIdx.y;
	const Mesh m = mesh_of(bvh, mesh_bytes, depth, n);
	const float* vp = verts + (int64_t)n * n_verts * 3;
	const int32_t* fp = faces + (int64_t)n * faces_mesh_stride;
	Box box = box_empty();
#pragma unroll
	for (int k = 0; k < BVH_LEAF; ++k) {
		const int f = m.order[j * BVH_LEAF + k];
		float a[3], b[3], c[3];
		if ((unsigned)f < (unsigned)n_faces && load_tri(vp, fp, f, n_verts, a, b, c)) {
			box_point(box, a); box_point(box, b); box_point(box, c);
		}
	}
	store_box(m.boxes, bvh_level_offset(depth) + j, box);
}

// grid (ceil(4^level / 256), n_meshes): the boxes of one level from the level below.
__global__ void inner_box_kernel(void* bvh, int64_t mesh_bytes, int depth, int level) {
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= bvh_leaf_count(level)) return;
	const Mesh m = mesh_of(bvh, mesh_bytes, depth, blockIdx.y);
	const int64_t node = bvh_level_offset(level) + j;
	Box box = box_empty();
#pragma unroll
	for (int c = 0; c < BVH_ARITY; ++c) {
		const float4 lo = m.boxes[2 * (BVH_ARITY * node + 1 + c)], hi = m.boxes[2 * (BVH_ARITY * node + 1 + c) + 1];
		Box ch;
		ch.lo[0] = lo.x; ch.lo[1] = lo.y; ch.lo[2] = lo.z; ch.hi[0] = hi.x; ch.hi[1] = hi.y; ch.hi[2] = hi.z;
		// a child that is no box (lo > hi, or a NaN from stale bytes) counts as empty: fminf / fmaxf drop a NaN, but not reliably both
		if (ch.lo[0] <= ch.hi[0] && ch.lo[1] <= ch.hi[1] && ch.lo[2] <= ch.hi[2]) box_union(box, ch);
	}
	store_box(m.boxes, node, box);
}

// grid (ceil(r_max / 256), n_meshes), a lane per ray.  key (n_meshes, r_max): a plain store for every row below r_len.
template <bool ANY>
__global__ __launch_bounds__(256) void ray_bvh_kernel(const float* __restrict__ origins, const float* __restrict__ dirs, const int32_t* __restrict__ r_len,
													   const int32_t* __restrict__ skip, const float* __restrict__ verts, const int32_t* __restrict__ faces,
													   int64_t faces_mesh_stride, int r_max, int n_verts, int n_faces, float t_min, float t_max, const void* bvh,
													   int64_t mesh_bytes, int depth, unsigned long long* __restrict__ key_out) {
	const int n = blockIdx.y;
	const int q = blockIdx.x * 256 + threadIdx.x;
	const int r1 = r_len ? min(max(r_len[n], 0), r_max) : r_max;
	if (q >= r1) return;
	const int64_t row = (int64_t)n * r_max + q;
	const float *o = origins + 3 * row, *d = dirs + 3 * row;
	const Frame fr = raycast::ray_frame(o[0], o[1], o[2], d[0], d[1], d[2]);
	const Slab sl = ray_slab(fr.ox, fr.oy, fr.oz, fr.dx, fr.dy, fr.dz, fr.dd, fr.live);
	const int sk = skip ? skip[row] : -1;
	const float* vp = verts + (int64_t)n * n_verts * 3;
	const int32_t* fp = faces + (int64_t)n * faces_mesh_stride;
	const Mesh m = mesh_of(const_cast<void*>(bvh), mesh_bytes, depth, n);
	const float4* __restrict__ boxes = m.boxes;
	const int32_t* __restrict__ order = m.order;
	const int64_t leaf0 = bvh_level_offset(depth);
	unsigned long long best = ~0ull;
	float t_hi = t_max;

	// the pair tests of one leaf; true: any_hit is done
	auto leaf = [&](int64_t j) -> bool {
#pragma unroll
		for (int k = 0; k < BVH_LEAF; ++k) {
			const int f = order[j * BVH_LEAF + k];
			if ((unsigned)f >= (unsigned)n_faces) continue;
			float a[3], b[3], c[3];
			if (!load_tri(vp, fp, f, n_verts, a, b, c)) continue;
			Hit h;
			if (raycast::pair_test(a[0] - fr.ox, a[1] - fr.oy, a[2] - fr.oz, b[0] - fr.ox, b[1] - fr.oy, b[2] - fr.oz, c[0] - fr.ox, c[1] - fr.oy, c[2] - fr.oz,
								   fr.e1x, fr.e1y, fr.e1z, fr.e2x, fr.e2y, fr.e2z, fr.dx, fr.dy, fr.dz, fr.dd, t_min, t_hi, h) &&
				f != sk) {
				best = min(best, raycast::hit_key(h.t, f));
				t_hi = raycast::key_time(best);   // (pair_test accepts t <= t_hi: an equal t on a smaller face still wins)
				if (ANY) return true;
			}
		}
		return false;
	};

	if (sl.live) {
		if (depth == 0) {
			leaf(0);
		} else {
			const float4 rl = boxes[0], rh = boxes[1];
			if (box_hit(sl, rl.x, rl.y, rl.z, rh.x, rh.y, rh.z, t_min, t_hi)) {
				int64_t node = 0;
				int level = 0;
				unsigned long long pend = 0;   // four bits per level: the children of the path's node at that level still to visit
				bool fresh = true;             // node was just entered: test its children
				unsigned mask = 0;
				for (;;) {
					if (fresh) {
						const float4* cb = boxes + 2 * (BVH_ARITY * node + 1);
						mask = 0;
#pragma unroll
						for (int c = 0; c < BVH_ARITY; ++c) {
							const float4 lo = cb[2 * c], hi = cb[2 * c + 1];
							if (box_hit(sl, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, t_min, t_hi)) mask |= 1u << c;
						}
						fresh = false;
					}
					if (mask == 0) {
						if (level == 0) break;
						--level;
						node = (node - 1) >> 2;
						mask = (unsigned)(pend >> (4 * level)) & 15u;
						continue;
					}
					const int c = __builtin_ctz(mask);
					mask &= mask - 1;
					const int64_t child = BVH_ARITY * node + 1 + c;
					if (level + 1 == depth) {
						if (leaf(child - leaf0)) break;
					} else {
						pend = (pend & ~(15ull << (4 * level))) | ((unsigned long long)mask << (4 * level));
						node = child;
						++level;
						fresh = true;
					}
				}
			}
		}
	}
	key_out[row] = best;
}

}  // namespace bvh
}  // namespace find

using namespace find;
using namespace find::bvh;

extern "C" int64_t find_bvh_bytes(int64_t n_meshes, int64_t n_faces) {
	if (bvh::bad_dims(n_meshes, 0, 0, n_faces)) return -1;
	return std::max<int64_t>(n_meshes * bvh_mesh_bytes(n_faces), 256);
}

// The checks the four entry points share; 1: nothing to do.
static int bvh_args(const char* who, const float* verts, const int32_t* faces, int64_t faces_batch, int64_t n_meshes, int64_t n_verts, int64_t n_faces,
					const void* bvh, int64_t bvh_bytes) {
	if (bvh::bad_dims(n_meshes, 0, n_verts, n_faces)) { set_error("%s: bad sizes", who); return FIND_EINVAL; }
	if (n_meshes == 0) return 1;
	if (!bvh || !((verts && faces) || n_faces == 0)) { set_error("%s: NULL argument", who); return FIND_EINVAL; }
	if (!(n_verts >= 1 || n_faces == 0)) { set_error("%s: faces without vertices", who); return FIND_EINVAL; }
	if (!(faces_batch == 1 || faces_batch == n_meshes)) { set_error("%s: faces_batch must be 1 or n_meshes", who); return FIND_EINVAL; }
	if (bvh_bytes < find_bvh_bytes(n_meshes, n_faces)) { set_error("%s: structure buffer too small", who); return FIND_EWORKSPACE; }
	return FIND_OK;
}

extern "C" int find_bvh_keys(const float* verts, const int32_t* faces, int64_t faces_batch, int64_t n_meshes, int64_t n_verts, int64_t n_faces, uint64_t* keys,
							 void* bvh, int64_t bvh_bytes, void* stream) {
	const int rc = bvh_args("find_bvh_keys", verts, faces, faces_batch, n_meshes, n_verts, n_faces, bvh, bvh_bytes);
	if (rc) return rc == 1 ? FIND_OK : rc;
	if (n_faces == 0) return FIND_OK;
	FIND_REQUIRE(keys, "find_bvh_keys: NULL argument");
	hipStream_t s = (hipStream_t)stream;
	const int64_t stride = faces_batch == 1 ? 0 : n_faces * 3;
	const int depth = bvh_depth(n_faces);
	const int64_t mesh_bytes = bvh_mesh_bytes(n_faces);
	hipLaunchKernelGGL(centroid_box_kernel, dim3(BVH_HEAD_BLOCKS, (unsigned)n_meshes), dim3(256), 0, s, verts, faces, stride, (int)n_verts, (int)n_faces, bvh,
					   mesh_bytes, depth);
	FIND_LAUNCH_CHECK("centroid_box_kernel");
	hipLaunchKernelGGL(keys_kernel, dim3((unsigned)cdiv(n_faces, 256), (unsigned)n_meshes), dim3(256), 0, s, verts, faces, stride, (int)n_verts, (int)n_faces,
					   (const void*)bvh, mesh_bytes, depth, reinterpret_cast<unsigned long long*>(keys));
	FIND_LAUNCH_CHECK("keys_kernel");
	return FIND_OK;
}

static int refit_launches(const float* verts, const int32_t* faces, int64_t faces_batch, int64_t n_meshes, int64_t n_verts, int64_t n_faces, void* bvh,
						  hipStream_t s) {
	const int64_t stride = faces_batch == 1 ? 0 : n_faces * 3;
	const int depth = bvh_depth(n_faces);
	const int64_t mesh_bytes = bvh_mesh_bytes(n_faces);
	hipLaunchKernelGGL(leaf_box_kernel, dim3((unsigned)cdiv(bvh_leaf_count(depth), 256), (unsigned)n_meshes), dim3(256), 0, s, verts, faces, stride, (int)n_verts,
					   (int)n_faces, bvh, mesh_bytes, depth);
	FIND_LAUNCH_CHECK("leaf_box_kernel");
	for (int level = depth - 1; level >= 0; --level) {
		hipLaunchKernelGGL(inner_box_kernel, dim3((unsigned)cdiv(bvh_leaf_count(level), 256), (unsigned)n_meshes), dim3(256), 0, s, bvh, mesh_bytes, depth, level);
		FIND_LAUNCH_CHECK("inner_box_kernel");
	}
	return FIND_OK;
}

extern "C" int find_bvh_build(const float* verts, const int32_t* faces, int64_t faces_batch, int64_t n_meshes, int64_t n_verts, int64_t n_faces,
							  const uint64_t* sorted_keys, void* bvh, int64_t bvh_bytes, void* stream) {
	const int rc = bvh_args("find_bvh_build", verts, faces, faces_batch, n_meshes, n_verts, n_faces, bvh, bvh_bytes);
	if (rc) return rc == 1 ? FIND_OK : rc;
	FIND_REQUIRE(sorted_keys || n_faces == 0, "find_bvh_build: NULL argument");
	hipStream_t s = (hipStream_t)stream;
	const int depth = bvh_depth(n_faces);
	const int64_t slots = bvh_leaf_count(depth) * BVH_LEAF;
	hipLaunchKernelGGL(order_kernel, dim3((unsigned)cdiv(slots, 256), (unsigned)n_meshes), dim3(256), 0, s, reinterpret_cast<const unsigned long long*>(sorted_keys),
					   (int)n_faces, slots, bvh, bvh_mesh_bytes(n_faces), depth);
	FIND_LAUNCH_CHECK("order_kernel");
	return refit_launches(verts, faces, faces_batch, n_meshes, n_verts, n_faces, bvh, s);
}

extern "C" int find_bvh_refit(const float* verts, const int32_t* faces, int64_t faces_batch, int64_t n_meshes, int64_t n_verts, int64_t n_faces, void* bvh,
							  int64_t bvh_bytes, void* stream) {
	const int rc = bvh_args("find_bvh_refit", verts, faces, faces_batch, n_meshes, n_verts, n_faces, bvh, bvh_bytes);
	if (rc) return rc == 1 ? FIND_OK : rc;
	return refit_launches(verts, faces, faces_batch, n_meshes, n_verts, n_faces, bvh, (hipStream_t)stream);
}

extern "C" int find_ray_bvh_fwd(const float* origins, const float* dirs, const int32_t* r_len, const int32_t* skip, const float* verts, const int32_t* faces,
								int64_t faces_batch, int64_t n_meshes, int64_t n_rays, int64_t n_verts, int64_t n_faces, float t_min, float t_max, int any_hit,
								float* t, int32_t* idx, float* bary, uint8_t* hit, const void* bvh, int64_t bvh_bytes, void* ws, int64_t ws_bytes, void* stream) {
	FIND_REQUIRE(!bvh::bad_dims(n_meshes, n_rays, n_verts, n_faces), "find_ray_bvh_fwd: bad sizes");
	FIND_REQUIRE(t_min >= 0.f, "find_ray_bvh_fwd: t_min must be >= 0 (and not NaN)");
	FIND_REQUIRE(!(t_max != t_max), "find_ray_bvh_fwd: t_max is NaN");
	FIND_REQUIRE(any_hit == 0 || any_hit == 1, "find_ray_bvh_fwd: any_hit must be 0 or 1");
	if (n_meshes == 0 || n_rays == 0) return FIND_OK;
	FIND_REQUIRE(origins && dirs && ws, "find_ray_bvh_fwd: NULL argument");
	FIND_REQUIRE(any_hit ? hit != nullptr : (t && idx && bary), "find_ray_bvh_fwd: NULL argument");
	FIND_REQUIRE((verts && faces && bvh) || n_faces == 0, "find_ray_bvh_fwd: NULL argument");
	FIND_REQUIRE(n_verts >= 1 || n_faces == 0, "find_ray_bvh_fwd: faces without vertices");
	FIND_REQUIRE(faces_batch == 1 || faces_batch == n_meshes, "find_ray_bvh_fwd: faces_batch must be 1 or n_meshes");
	if (n_faces > 0 && bvh_bytes < find_bvh_bytes(n_meshes, n_faces)) { set_error("find_ray_bvh_fwd: structure buffer too small"); return FIND_EWORKSPACE; }
	if (ws_bytes < find_ray_ws_bytes(n_meshes, n_rays, n_faces)) { set_error("find_ray_bvh_fwd: workspace too small"); return FIND_EWORKSPACE; }
	hipStream_t s = (hipStream_t)stream;
	unsigned long long* key = reinterpret_cast<unsigned long long*>(ws);
	const int64_t stride = faces_batch == 1 ? 0 : n_faces * 3;
	if (n_faces > 0) {
		const dim3 grid((unsigned)cdiv(n_rays, 256), (unsigned)n_meshes);
		const int depth = bvh_depth(n_faces);
		const int64_t mesh_bytes = bvh_mesh_bytes(n_faces);
		if (any_hit)
			hipLaunchKernelGGL(ray_bvh_kernel<true>, grid, dim3(256), 0, s, origins, dirs, r_len, skip, verts, faces, stride, (int)n_rays, (int)n_verts, (int)n_faces,
							   t_min, t_max, bvh, mesh_bytes, depth, key);
		else
			hipLaunchKernelGGL(ray_bvh_kernel<false>, grid, dim3(256), 0, s, origins, dirs, r_len, skip, verts, faces, stride, (int)n_rays, (int)n_verts, (int)n_faces,
							   t_min, t_max, bvh, mesh_bytes, depth, key);
		FIND_LAUNCH_CHECK("ray_bvh_kernel");
	}
	return raycast::ray_finish_launch(origins, dirs, r_len, verts, faces, stride, n_meshes, n_rays, n_verts, n_faces, key, t, idx, bary,
									  any_hit ? hit : (uint8_t*)nullptr, stream);
}
