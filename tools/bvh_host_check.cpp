// Host check of csrc/bvh_math.h: the tree of bvh.hip built on the host from the same functions, walked as ray_bvh_kernel walks it with
// raycast_math.h's pair test, against a brute-force loop over the same faces.  A stand-alone program for a sanitizer run on the CPU:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I find_amd/csrc tools/bvh_host_check.cpp -o bvh_host_check
// Without arguments: the layout's closed forms, the keys' order, and box_hit's rules on the unit cube (zero direction components, rays in a
// face plane, flat boxes, the empty box, the interval's ends).
// With `cases IN`: IN holds int32 n_cases, then per case int32 V, F, R, float32 verts (V, 3), int32 faces (F, 3), float32 rays (R, 8) --
// o, d, t_min, t_max -- and int32 skip (R).  Per case and ray it compares
//   the walk's (t bits, face) with brute force (the minimum of hit_key over every accepted pair),
//   the any_hit walk with "brute force hit something",
// and, for EVERY pair that brute force accepts, asks box_hit for every box above the face with t_hi lowered to that pair's own t (the
// lowest bound under which the pair must still be reached): conservativeness itself, not only its effect on the winner.
// Prints the counts; exit status 0 and "ok" when nothing differs.
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "bvh_math.h"
#include "raycast_math.h"

using namespace find::bvh;
using namespace find::raycast;

static int failures = 0;
#define CHECK(cond, ...)                                  \
	do {                                                  \
		if (!(cond)) {                                    \
			++failures;                                   \
			printf("FAILED %s:%d: ", __FILE__, __LINE__); \
			printf(__VA_ARGS__);                          \
			printf("\n");                                 \
		}                                                 \
	} while (0)

struct Tree {
	int n_verts = 0, n_faces = 0, depth = 0;
	const float* verts = nullptr;
	const int32_t* faces = nullptr;
	std::vector<int32_t> order;
	std::vector<Box> boxes;

	bool tri(int f, float a[3], float b[3], float c[3]) const {
		const int32_t* p = faces + 3 * (int64_t)f;
		for (int k = 0; k < 3; ++k)
			if (!((unsigned)p[k] < (unsigned)n_verts)) return false;
		for (int k = 0; k < 3; ++k) { a[k] = verts[3 * p[0] + k]; b[k] = verts[3 * p[1] + k]; c[k] = verts[3 * p[2] + k]; }
		return finite_tri(a, b, c);
	}

	void refit() {
		boxes.assign(bvh_node_count(depth), box_empty());
		const int64_t leaf0 = bvh_level_offset(depth);
		for (int64_t j = 0; j < bvh_leaf_count(depth); ++j)
			for (int k = 0; k < BVH_LEAF; ++k) {
				const int f = order[j * BVH_LEAF + k];
				float a[3], b[3], c[3];
				if ((unsigned)f < (unsigned)n_faces && tri(f, a, b, c)) { box_point(boxes[leaf0 + j], a); box_point(boxes[leaf0 + j], b); box_point(boxes[leaf0 + j], c); }
			}
		for (int level = depth - 1; level >= 0; --level)
			for (int64_t j = 0; j < bvh_leaf_count(level); ++j) {
				const int64_t node = bvh_level_offset(level) + j;
				for (int c = 0; c < BVH_ARITY; ++c) box_union(boxes[node], boxes[BVH_ARITY * node + 1 + c]);
			}
	}

	void build(const float* v, int nv, const int32_t* f, int nf) {
		verts = v; faces = f; n_verts = nv; n_faces = nf;
		depth = bvh_depth(nf);
		Box cb = box_empty();
		for (int i = 0; i < nf; ++i) {
			float a[3], b[3], c[3], s[3];
			if (!tri(i, a, b, c)) continue;
			centroid3(a, b, c, s);
			box_point(cb, s);
		}
		std::vector<unsigned long long> keys(nf);
		for (int i = 0; i < nf; ++i) {
			float a[3], b[3], c[3], s[3];
			uint32_t hi = BVH_INVALID_HI;
			if (tri(i, a, b, c)) { centroid3(a, b, c, s); hi = morton30(s[0], s[1], s[2], cb.lo, cb.hi); }
			keys[i] = face_key(hi, i);
		}
		std::vector<long long> as_signed(keys.begin(), keys.end());   // the caller's sort may be a signed one
		std::sort(keys.begin(), keys.end());
		std::sort(as_signed.begin(), as_signed.end());
		for (int i = 0; i < nf; ++i) CHECK((unsigned long long)as_signed[i] == keys[i], "a signed sort orders the keys differently at %d", i);
		order.assign(bvh_leaf_count(depth) * BVH_LEAF, -1);
		for (int i = 0; i < nf; ++i) order[i] = (int32_t)(uint32_t)keys[i];
		refit();
	}

	bool hit_box(const Slab& s, int64_t node, float t_min, float t_hi) const {
		const Box& b = boxes[node];
		return box_hit(s, b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2], t_min, t_hi);
	}

	// ray_bvh_kernel's walk.  boxes_tested: how many box tests it took.
	unsigned long long walk(const float* r, int skip, bool any, long long& boxes_tested) const {
		const Frame fr = ray_frame(r[0], r[1], r[2], r[3], r[4], r[5]);
		const Slab sl = ray_slab(fr.ox, fr.oy, fr.oz, fr.dx, fr.dy, fr.dz, fr.dd, fr.live);
		const float t_min = r[6];
		float t_hi = r[7];
		unsigned long long best = ~0ull;
		const int64_t leaf0 = bvh_level_offset(depth);
		auto leaf = [&](int64_t j) -> bool {
			for (int k = 0; k < BVH_LEAF; ++k) {
				const int f = order[j * BVH_LEAF + k];
				float a[3], b[3], c[3];
				if ((unsigned)f >= (unsigned)n_faces || !tri(f, a, b, c)) continue;
				Hit h;
				if (ray_face(fr, a, b, c, t_min, t_hi, h) && f != skip) {
					best = std::min(best, hit_key(h.t, f));
					t_hi = key_time(best);
					if (any) return true;
				}
			}
			return false;
		};
		if (!sl.live) return best;
		if (depth == 0) { leaf(0); return best; }
		++boxes_tested;
		if (!hit_box(sl, 0, t_min, t_hi)) return best;
		int64_t node = 0;
		int level = 0;
		unsigned long long pend = 0;
		bool fresh = true;
		unsigned mask = 0;
		for (;;) {
			if (fresh) {
				mask = 0;
				for (int c = 0; c < BVH_ARITY; ++c)
					if (hit_box(sl, BVH_ARITY * node + 1 + c, t_min, t_hi)) mask |= 1u << c;
				boxes_tested += BVH_ARITY;
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
		return best;
	}
};

static int run_cases(const char* in) {
	FILE* fi = fopen(in, "rb");
	if (!fi) { printf("cannot open %s\n", in); return 2; }
	int32_t n_cases = 0;
	if (fread(&n_cases, 4, 1, fi) != 1) { fclose(fi); printf("short file\n"); return 2; }
	long long total_diff = 0;
	for (int cs = 0; cs < n_cases; ++cs) {
		int32_t hdr[3];
		if (fread(hdr, 4, 3, fi) != 3 || hdr[0] < 0 || hdr[1] < 0 || hdr[2] < 0) { fclose(fi); printf("short file\n"); return 2; }
		const int V = hdr[0], F = hdr[1], R = hdr[2];
		std::vector<float> verts((size_t)V * 3), rays((size_t)R * 8);
		std::vector<int32_t> faces((size_t)F * 3), skip(R);
		if (fread(verts.data(), 4, verts.size(), fi) != verts.size() || fread(faces.data(), 4, faces.size(), fi) != faces.size() ||
			fread(rays.data(), 4, rays.size(), fi) != rays.size() || fread(skip.data(), 4, skip.size(), fi) != skip.size()) {
			fclose(fi); printf("short file\n"); return 2;
		}
		Tree tr;
		tr.build(verts.data(), V, faces.data(), F);
		// where each face stands: its leaf, for the walk up through its ancestors
		std::vector<int64_t> leaf_of(F, -1);
		for (size_t i = 0; i < tr.order.size(); ++i)
			if ((unsigned)tr.order[i] < (unsigned)F) leaf_of[tr.order[i]] = bvh_level_offset(tr.depth) + (int64_t)i / BVH_LEAF;
		long long diff = 0, diff_any = 0, unreached = 0, hits = 0, pairs = 0, tested = 0, tested_any = 0;
		for (int q = 0; q < R; ++q) {
			const float* r = &rays[(size_t)q * 8];
			const Frame fr = ray_frame(r[0], r[1], r[2], r[3], r[4], r[5]);
			const Slab sl = ray_slab(fr.ox, fr.oy, fr.oz, fr.dx, fr.dy, fr.dz, fr.dd, fr.live);
			unsigned long long want = ~0ull;
			for (int f = 0; f < F; ++f) {
				float a[3], b[3], c[3];
				Hit h;
				if (!tr.tri(f, a, b, c) || !ray_face(fr, a, b, c, r[6], r[7], h) || f == skip[q]) continue;
				want = std::min(want, hit_key(h.t, f));
				++pairs;
				if (!sl.live) { ++unreached; continue; }
				if (tr.depth == 0) continue;
				for (int64_t node = leaf_of[f];; node = (node - 1) >> 2) {
					if (!tr.hit_box(sl, node, r[6], h.t)) { ++unreached; break; }
					if (node == 0) break;
				}
			}
			const unsigned long long got = tr.walk(r, skip[q], false, tested), got_any = tr.walk(r, skip[q], true, tested_any);
			hits += want != ~0ull;
			if (got != want) {
				if (diff < 5) printf("case %d ray %d: walk %016llx, brute force %016llx\n", cs, q, got, want);
				++diff;
			}
			diff_any += (got_any != ~0ull) != (want != ~0ull);
		}
		printf("case %d: V %d F %d depth %d, %d rays, %lld hit, %lld accepted pairs; differences %lld, any_hit %lld, pairs behind a refused box %lld; "
			   "boxes tested per ray %.1f (any_hit %.1f)\n", cs, V, F, tr.depth, R, hits, pairs, diff, diff_any, unreached, R ? (double)tested / R : 0., R ? (double)tested_any / R : 0.);
		total_diff += diff + diff_any + unreached;
	}
	fclose(fi);
	if (total_diff || failures) { printf("%lld differences, %d checks failed\n", total_diff, failures); return 1; }
	printf("ok\n");
	return 0;
}

int main(int argc, char** argv) {
	if (argc == 3 && !strcmp(argv[1], "cases")) return run_cases(argv[2]);
	const float inf = INFINITY;
	{   // layout
		CHECK(bvh_depth(0) == 0 && bvh_depth(1) == 0 && bvh_depth(BVH_LEAF) == 0 && bvh_depth(BVH_LEAF + 1) == 1 && bvh_depth(4 * BVH_LEAF) == 1 && bvh_depth(4 * BVH_LEAF + 1) == 2, "depth");
		CHECK(bvh_depth((1ll << 30) - 1) == 14, "depth at the largest face count: %d", bvh_depth((1ll << 30) - 1));
		CHECK(bvh_level_offset(0) == 0 && bvh_level_offset(1) == 1 && bvh_level_offset(2) == 5 && bvh_level_offset(3) == 21 && bvh_node_count(2) == 21, "level offsets");
		for (int d = 1; d < 6; ++d)
			for (int64_t j = 0; j < bvh_leaf_count(d); ++j) {
				const int64_t node = bvh_level_offset(d) + j, parent = (node - 1) >> 2;
				CHECK(parent >= bvh_level_offset(d - 1) && parent < bvh_level_offset(d) && BVH_ARITY * parent + 1 <= node && node <= BVH_ARITY * parent + BVH_ARITY, "parent of %lld", (long long)node);
			}
		int64_t last = 0;
		for (int64_t f = 0; f < 5000; ++f) { CHECK(bvh_mesh_bytes(f) >= last && bvh_mesh_bytes(f) % 256 == 0, "bytes at %lld", (long long)f); last = bvh_mesh_bytes(f); }
	}
	{   // keys
		const float lo[3] = {0, 0, 0}, hi[3] = {1, 0, 2};
		CHECK(quantise10(0.f, 0.f, 1.f) == 0 && quantise10(1.f, 0.f, 1.f) == 1023 && quantise10(0.5f, 0.f, 1.f) == 512 && quantise10(7.f, 7.f, 7.f) == 0, "quantise");
		CHECK(quantise10(NAN, 0.f, 1.f) == 0 && quantise10(0.5f, -inf, inf) == 0 && quantise10(-3.f, 0.f, 1.f) == 0 && quantise10(9.f, 0.f, 1.f) == 1023, "quantise, odd inputs");
		CHECK(morton30(1.f, 5.f, 2.f, lo, hi) == ((spread10(1023) << 2) | spread10(1023)) && spread10(1023) == 0x09249249u && morton30(1.f, 0.f, 2.f, lo, hi) < (1u << 30), "morton");
		CHECK(face_key(BVH_INVALID_HI, 5) > face_key((1u << 30) - 1, (1 << 30) - 1) && (long long)face_key(BVH_INVALID_HI, (1 << 30) - 1) > 0, "the invalid key sorts last, signed too");
	}
	{   // box_hit on the unit cube and on its flat sides
		auto slab = [](float ox, float oy, float oz, float dx, float dy, float dz) {
			const Frame f = ray_frame(ox, oy, oz, dx, dy, dz);
			return ray_slab(f.ox, f.oy, f.oz, f.dx, f.dy, f.dz, f.dd, f.live);
		};
		const Slab axis = slab(0.25f, 0.5f, -1.f, 0, 0, 2);   // two zero components
		CHECK(box_hit(axis, 0, 0, 0, 1, 1, 1, 0.f, inf), "an axis ray misses the cube's box");
		CHECK(box_hit(axis, 0, 0, 0, 1, 1, 0, 0.f, inf) && box_hit(axis, 0, 0, 1, 1, 1, 1, 0.f, inf), "an axis ray misses a flat box");
		CHECK(!box_hit(axis, 0.5f, 0, 0, 1, 1, 1, 0.f, inf) && !box_hit(axis, 0, 0, 0, 1, 0.25f, 1, 0.f, inf), "an axis ray hits a box beside it");
		CHECK(box_hit(axis, 0.25f, 0, 0, 1, 1, 1, 0.f, inf) && box_hit(axis, 0, 0, 0, 0.25f, 0.5f, 1, 0.f, inf), "an axis ray in a box's face plane (and along its edge) misses");
		CHECK(box_hit(axis, 0, 0, 0, 1, 1, 1, 0.f, 0.5f) && !box_hit(axis, 0, 0, 0, 1, 1, 1, 0.f, 0.4999f), "t_hi at the entry");
		CHECK(box_hit(axis, 0, 0, 0, 1, 1, 1, 1.f, inf) && !box_hit(axis, 0, 0, 0, 1, 1, 1, 1.0001f, inf), "t_min at the exit");
		CHECK(!box_hit(axis, inf, inf, inf, -inf, -inf, -inf, 0.f, inf) && !box_hit(axis, NAN, 0, 0, 1, 1, 1, 0.f, inf), "the empty box is entered");
		const Slab back = slab(0.25f, 0.5f, -1.f, 0, 0, -2);
		CHECK(!box_hit(back, 0, 0, 0, 1, 1, 1, 0.f, inf), "a box behind the ray is entered");
		const Slab plane = slab(-1.f, 0.5f, 0.f, 1, 0, 0);   // in the plane z = 0 of the cube, one zero component pair
		CHECK(box_hit(plane, 0, 0, 0, 1, 1, 0, 0.f, inf) && box_hit(plane, 0, 0, 0, 1, 1, 1, 0.f, inf) && !box_hit(plane, 0, 0, 0.001f, 1, 1, 1, 0.f, inf), "a ray in a face plane");
		const Slab diag = slab(-1.f, -1.f, 0.5f, 1, 1, 0);   // one zero component
		CHECK(box_hit(diag, 0, 0, 0, 1, 1, 1, 0.f, inf) && box_hit(diag, 0, 0, 0.5f, 1, 1, 0.5f, 0.f, inf) && !box_hit(diag, 0, 0, 0.6f, 1, 1, 1, 0.f, inf), "one zero component");
		CHECK(box_hit(diag, 0, 0, 0, 0, 0, 1, 0.f, inf) && !box_hit(diag, 0.5f, 0, 0, 1, 0.25f, 1, 0.f, inf), "a diagonal ray through an edge / past a box");
		const Slab on = slab(0.f, 0.5f, 0.5f, 1, 0.25f, 0);   // starts on a box plane
		CHECK(box_hit(on, 0, 0, 0, 1, 1, 1, 0.f, inf) && box_hit(on, -1, 0, 0, 0, 1, 1, 0.f, inf), "a ray that starts on a box plane");
		const Slab tiny = slab(0.25f, 0.5f, -1.f, 1e-38f, 0, 2);   // a denormal ratio counts as a constant axis
		CHECK(tiny.ix == 0.f && box_hit(tiny, 0, 0, 0, 1, 1, 1, 0.f, inf), "a denormal direction ratio");
		const Slab far_ = slab(3e38f, 0, 0, -1, 0, 0);   // lo - o overflows: no statement, the box is kept
		CHECK(box_hit(far_, -3e38f, -1, -1, -2e38f, 1, 1, 0.f, inf), "an overflowed box is refused");
		CHECK(!slab(0, 0, 0, 0, 0, 0).live && !slab(0, 0, 0, NAN, 1, 0).live && !slab(0, 0, 0, 1e20f, 0, 0).live && !slab(0, 0, 0, 1e-30f, 0, 0).live && slab(0, 0, 0, 1e-20f, 0, 0).live, "live");
	}
	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("ok\n");
	return 0;
}
