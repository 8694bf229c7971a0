// The arithmetic of bvh.hip that needs no GPU: the layout of the implicit tree, the Morton key of a face, the boxes and the conservative
// ray / box test.  Plain functions, compiled for the device by bvh.hip and for the host by tools/bvh_host_check.cpp.
//
// Layout, a function of n_faces alone.  The faces stand in Morton order; a LEAF is BVH_LEAF consecutive sorted faces; the leaf count is
// padded to BVH_ARITY^D, D = bvh_depth(n_faces) the smallest power that holds them; the tree is complete and BVH_ARITY wide: level l has
// 4^l nodes, node i has the children 4 i + 1 .. 4 i + 4 and the parent (i - 1) / 4, the leaves are the nodes (4^D - 1) / 3 + j.  Nothing is
// stored but the order (int32, -1 behind the last face) and one box per node (lo, hi as two float4): child and parent indices are computed,
// so a walk cannot cycle or leave the buffer whatever the buffer holds.  A padding leaf, and every node above padding alone, is the EMPTY
// box lo = +inf, hi = -inf, which box_hit refuses first.
//
// Keys.  morton << 32 | face: the 30-bit code of the face's centroid sum a + b + c, each axis quantised to 10 bits on the box of the valid
// faces' centroid sums (an axis without extent quantises to 0).  An invalid face -- a -1 row, an index outside [0, V), a non-finite corner --
// gets the high word 0x7fffffff: every key is below 2^63, so a SIGNED 64-bit sort orders the rows as an unsigned one does, invalid faces
// last.  The keys of a row are distinct (the face is in the low word), so every correct sort gives the same order.  The order only decides
// which faces share a box: it changes the speed of a walk and never its result.
//
// The ray / box test (box_hit).  raycast_math.h's pair test works on P = fl(p - o) per corner, and rounding is monotone: with lo <= p <= hi
// (plain min / max, exact) the box B' = [fl(lo - o), fl(hi - o)] holds the computed P of every corner EXACTLY.  Let M be the largest
// |coordinate| of B' and u = 2^-24.  An accepted pair has the origin of the ray's plane inside the triangle of the computed projections
// x' = P_kx - P_kz r (r = fl(d_kx / d_kz), |r| <= 1; one rounded product, one rounded sum: |x' - x| <= 3 u M, likewise y'), so the exact
// line through o along d passes within 3 u M + u M (r against d_kx / d_kz) + 2 u M (an edge function that rounds to 0 with the other sign)
// of a point Q of B' in the two minor axes, at Q's own major coordinate.  The pair's t is a convex combination of z_i / dd, z_i = P_i . d,
// whatever the computed weights are, so it lies between the least and the largest X . d / dd over X in B' up to the rounding of the nine
// products and sums and the division, <= 33 u M / |d_kz|.  box_hit therefore asks two things, each with the margin e = 2^-17 M + 1e-30
// (128 u M, which also pays for its own roundings: fl(lo' - e), the product with the rounded reciprocal 1 / r_k, 3 u M in all, and twelve
// u M / |d_kz| for the depth sums; the 1e-30 is for products that underflow):
//   the LINE meets B' grown by e: slabs in w = the coordinate along the major axis, position_k = w r_k with r_major = 1 exactly; an axis
//   with |r_k| < 2^-100 moves less than 2^-100 (M + e) inside the major slab and is tested as constant, 0 in [lo'_k - e, hi'_k + e]; no
//   0 * inf arises because no reciprocal of 0 is formed, a flat box (lo == hi) and a ray in a box's face plane are the closed comparisons;
//   the DEPTHS of B', [sum_k min(lo'_k g_k, hi'_k g_k), sum_k max(..)] with g_k = fl(d_k / dd), grown by e / |d_kz|, meet [t_min, t_hi].
// A box is culled only by a comparison that is TRUE (entry strictly beyond t_hi: a pair with t equal to the current best on another face
// is still reached); every NaN and every overflow (M not finite) keeps the box.  The margin depends on the ray's origin, so it cannot be
// stored: the boxes themselves carry no inflation, they are the exact min / max of their corners.
// That is why the ray's own interval is NOT cut into the slabs: the point where the line meets the box may lie a little outside the
// interval in which the pair's computed t lies (a sliver seen edge-on); only the depth test speaks about t.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define FIND_BVH_HD __host__ __device__ inline
#else
#define FIND_BVH_HD inline
#endif

namespace find {
namespace bvh {

constexpr int BVH_LEAF = 4;    // faces per leaf
constexpr int BVH_ARITY = 4;   // children per node
constexpr int BVH_HEAD_BLOCKS = 64;                  // partial centroid boxes per mesh (find_bvh_keys), eight floats each
constexpr uint32_t BVH_INVALID_HI = 0x7fffffffu;     // the high word of an invalid face's key
constexpr float BVH_FLT_MAX = 3.4028234663852886e38f;

// ------------------------------------------------------------------ layout
FIND_BVH_HD int bvh_depth(int64_t n_faces) {
	const int64_t leaves = (n_faces + BVH_LEAF - 1) / BVH_LEAF;
	int d = 0;
	while (((int64_t)1 << (2 * d)) < leaves) ++d;
	return d;   // <= 14 at n_faces < 2^30
}
FIND_BVH_HD int64_t bvh_level_offset(int level) { return (((int64_t)1 << (2 * level)) - 1) / 3; }   // nodes above the level
FIND_BVH_HD int64_t bvh_leaf_count(int depth) { return (int64_t)1 << (2 * depth); }
FIND_BVH_HD int64_t bvh_node_count(int depth) { return bvh_level_offset(depth + 1); }
FIND_BVH_HD int64_t bvh_align(int64_t x) { return (x + 255) / 256 * 256; }
// per mesh: the head (the partial centroid boxes of the keys call), the order, the boxes -- each 256-byte aligned
FIND_BVH_HD int64_t bvh_head_bytes() { return (int64_t)BVH_HEAD_BLOCKS * 8 * 4; }
FIND_BVH_HD int64_t bvh_order_bytes(int depth) { return bvh_align(bvh_leaf_count(depth) * BVH_LEAF * 4); }
FIND_BVH_HD int64_t bvh_mesh_bytes(int64_t n_faces) {
	const int d = bvh_depth(n_faces);
	return bvh_head_bytes() + bvh_order_bytes(d) + bvh_align(bvh_node_count(d) * 32);
}

// ------------------------------------------------------------------ keys
FIND_BVH_HD uint32_t spread10(uint32_t x) {   // 10 bits -> every third bit
	x &= 0x3ffu;
	x = (x | (x << 16)) & 0x030000ffu;
	x = (x | (x << 8)) & 0x0300f00fu;
	x = (x | (x << 4)) & 0x030c30c3u;
	x = (x | (x << 2)) & 0x09249249u;
	return x;
}
// 0 .. 1023 of c on [lo, hi]; an axis without extent, and whatever is not a number, gives 0
FIND_BVH_HD uint32_t quantise10(float c, float lo, float hi) {
#pragma clang fp contract(off)
	const float ext = hi - lo;
	if (!(ext > 0.f)) return 0u;
	const float x = (c - lo) / ext * 1024.f;
	if (!(x >= 0.f)) return 0u;
	return x >= 1023.f ? 1023u : (uint32_t)x;
}
FIND_BVH_HD uint32_t morton30(float cx, float cy, float cz, const float lo[3], const float hi[3]) {
	return (spread10(quantise10(cx, lo[0], hi[0])) << 2) | (spread10(quantise10(cy, lo[1], hi[1])) << 1) | spread10(quantise10(cz, lo[2], hi[2]));
}
FIND_BVH_HD unsigned long long face_key(uint32_t hi_word, int face) { return ((unsigned long long)hi_word << 32) | (unsigned long long)(uint32_t)face; }

FIND_BVH_HD bool finite1(float x) { return fabsf(x) <= BVH_FLT_MAX; }
FIND_BVH_HD bool finite_tri(const float a[3], const float b[3], const float c[3]) {
	return finite1(a[0]) && finite1(a[1]) && finite1(a[2]) && finite1(b[0]) && finite1(b[1]) && finite1(b[2]) && finite1(c[0]) && finite1(c[1]) && finite1(c[2]);
}
// the centroid sum of a face, (a + b) + c per axis
FIND_BVH_HD void centroid3(const float a[3], const float b[3], const float c[3], float s[3]) {
#pragma clang fp contract(off)
	for (int k = 0; k < 3; ++k) s[k] = (a[k] + b[k]) + c[k];
}

// ------------------------------------------------------------------ boxes
struct Box {
	float lo[3], hi[3];
};
FIND_BVH_HD Box box_empty() {
	Box b;
	for (int k = 0; k < 3; ++k) { b.lo[k] = INFINITY; b.hi[k] = -INFINITY; }
	return b;
}
FIND_BVH_HD void box_point(Box& b, const float p[3]) {
	for (int k = 0; k < 3; ++k) { b.lo[k] = fminf(b.lo[k], p[k]); b.hi[k] = fmaxf(b.hi[k], p[k]); }
}
FIND_BVH_HD void box_union(Box& b, const Box& o) {   // (an empty box changes nothing: min with +inf, max with -inf)
	for (int k = 0; k < 3; ++k) { b.lo[k] = fminf(b.lo[k], o.lo[k]); b.hi[k] = fmaxf(b.hi[k], o.hi[k]); }
}

// ------------------------------------------------------------------ the ray / box test
struct Slab {
	float ox, oy, oz;
	float ix, iy, iz;   // 1 / r_k, r_k = d_k / d_major; 0: the axis counts as constant (|r_k| < 2^-100)
	float gx, gy, gz;   // d_k / dd
	float im;           // 1 / |d_major|
	bool live;          // false: the ray can hit nothing (raycast_math.h's rule, or dd is 0 or not finite: no t passes the interval)
};

FIND_BVH_HD float slab_inv(float d, float m) {
#pragma clang fp contract(off)
	const float r = d / m;
	return fabsf(r) < 7.888609052210118e-31f ? 0.f : 1.f / r;   // 2^-100
}

FIND_BVH_HD Slab ray_slab(float ox, float oy, float oz, float dx, float dy, float dz, float dd, bool frame_live) {
#pragma clang fp contract(off)
	Slab s;
	s.ox = ox; s.oy = oy; s.oz = oz;
	float m = dx;   // the major component: ray_frame's rule, the first of equals
	if (fabsf(dy) > fabsf(m)) m = dy;
	if (fabsf(dz) > fabsf(m)) m = dz;
	s.live = frame_live && dd > 0.f && dd <= BVH_FLT_MAX;
	if (!s.live) m = 1.f;
	s.ix = slab_inv(dx, m); s.iy = slab_inv(dy, m); s.iz = slab_inv(dz, m);
	s.gx = dx / dd; s.gy = dy / dd; s.gz = dz / dd;
	s.im = 1.f / fabsf(m);
	return s;
}

// One axis of the line test: cuts [w0, w1] by the slab, or says false when a constant axis lies outside.
FIND_BVH_HD bool slab_axis(float a, float b, float inv, float e, float& w0, float& w1) {
#pragma clang fp contract(off)
	a = a - e;
	b = b + e;
	if (inv == 0.f) return !((a > 0.f) | (b < 0.f));
	const float p = a * inv, q = b * inv;
	w0 = fmaxf(w0, fminf(p, q));
	w1 = fminf(w1, fmaxf(p, q));
	return true;
}

// May a pair of this ray with a face inside [lo, hi], with t_min < t <= t_hi, exist?  False only when it cannot.
FIND_BVH_HD bool box_hit(const Slab& s, float lox, float loy, float loz, float hix, float hiy, float hiz, float t_min, float t_hi) {
#pragma clang fp contract(off)
	if (!(lox <= hix)) return false;   // the empty box (and a NaN)
	const float ax = lox - s.ox, ay = loy - s.oy, az = loz - s.oz, bx = hix - s.ox, by = hiy - s.oy, bz = hiz - s.oz;
	const float M = fmaxf(fmaxf(fmaxf(fabsf(ax), fabsf(bx)), fmaxf(fabsf(ay), fabsf(by))), fmaxf(fabsf(az), fabsf(bz)));
	if (!(M <= BVH_FLT_MAX)) return true;   // B' overflowed: no statement
	const float e = M * 7.62939453125e-06f + 1e-30f;   // 2^-17 M
	float w0 = -INFINITY, w1 = INFINITY;
	if (!slab_axis(ax, bx, s.ix, e, w0, w1)) return false;
	if (!slab_axis(ay, by, s.iy, e, w0, w1)) return false;
	if (!slab_axis(az, bz, s.iz, e, w0, w1)) return false;
	if (w0 > w1) return false;
	const float px = ax * s.gx, qx = bx * s.gx, py = ay * s.gy, qy = by * s.gy, pz = az * s.gz, qz = bz * s.gz;
	const float near_t = (fminf(px, qx) + fminf(py, qy)) + fminf(pz, qz), far_t = (fmaxf(px, qx) + fmaxf(py, qy)) + fmaxf(pz, qz);
	const float et = e * s.im;
	if (near_t - et > t_hi) return false;   // (a NaN -- inf - inf -- compares false: the box is kept)
	if (far_t + et < t_min) return false;
	return true;
}

}  // namespace bvh
}  // namespace find
