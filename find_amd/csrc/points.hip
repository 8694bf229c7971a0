// Keypoint splats of FootRenderer (reference src/model/renderer.py:139-142, 365-376): PyTorch3D's PointsRasterizer (K nearest points per
// pixel within a radius) fused with PointsRenderer + AlphaCompositor, forward only.  PyTorch3D is restated from recall ([P3D-recall],
// DESIGN.md 2):
//   - points go to view space and NDC with the view-space z kept: (s x / z, s y / z, z), the operation order of render.hip's project_kernel
//     (here without fused multiply-adds);
//   - pixel centres are the mesh rasteriser's, 1 - (2 i + 1) / S on each axis;
//   - a point with z < 0 is skipped; it counts for a pixel if d^2 = dx^2 + dy^2 < r^2 (strict);
//   - a pixel keeps the K points of smallest z, sorted by z; equal z goes to the lower point index; empty slots: idx, zbuf, dists -1;
//   - w = 1 - d^2 / r^2; front to back out = sum_k c_k w_k f_k, c_0 = 1, c_k+1 = c_k (1 - w_k); no background (an empty pixel is 0).
//
// One 256-thread workgroup per 16x16-pixel tile of one image (image = cloud * n_views + view).  The workgroup streams its cloud's points in
// chunks of 256, one per thread: each thread projects its point and keeps it if z >= 0 and its splat box [x +- r] x [y +- r] meets the tile's
// NDC box widened by one pixel.  The survivors go to an LDS list in point-index order (a 64-bit wave ballot, the rank below the lane, per-wave
// offsets), and every thread walks that list for its own pixel with the exact test.  The K-buffer lives in registers: KMAX slots, indexed
// statically only, kept sorted by z with a compare-and-shift insertion; strict comparisons on walking the points in index order give the
// tie rule.  No atomics and no state across workgroups: the result does not depend on the tile or the chunk size, and repeats are
// bit-identical.
#include "common.h"

namespace find {
namespace points {

constexpr int TILE = 16;                 // tile edge in pixels
constexpr int THREADS = TILE * TILE;     // one pixel per thread, one point per thread while collecting
constexpr int WAVES = THREADS / 64;
constexpr int64_t MAX_IMAGE = 1 << 14;   // image edge
constexpr int64_t MAX_POINTS = 1 << 30;  // per cloud (the index goes through an LDS float as its bits)

template <int KMAX>
__global__ __launch_bounds__(THREADS) void points_render_kernel(const float* __restrict__ points, const float* __restrict__ features,
																const float* __restrict__ R, const float* __restrict__ T, float s, int n_views,
																int P, int H, int W, int tiles_x, int n_tiles, float radius, int K,
																float* __restrict__ image, int32_t* __restrict__ idx_out,
																float* __restrict__ zbuf_out, float* __restrict__ dists_out) {
	__shared__ float4 list[THREADS];   // (x_ndc, y_ndc, z_view, point index as bits)
	__shared__ int wave_count[WAVES];
	const int img = (int)(blockIdx.x / (unsigned)n_tiles);
	const int tile = (int)(blockIdx.x - (unsigned)img * (unsigned)n_tiles);
	const int cloud = img / n_views, view = img - cloud * n_views;
	const int tx0 = (tile % tiles_x) * TILE, ty0 = (tile / tiles_x) * TILE;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int xi = tx0 + (tid & (TILE - 1)), yi = ty0 + tid / TILE;
	const float px = 1.0f - (2.0f * xi + 1.0f) / (float)W;
	const float py = 1.0f - (2.0f * yi + 1.0f) / (float)H;
	// the tile's NDC box (+x left, +y up: the last column / row has the smallest centre) widened by one pixel
	const int xl = min(tx0 + TILE - 1, W - 1), yl = min(ty0 + TILE - 1, H - 1);
	const float bx_lo = 1.0f - (2.0f * xl + 1.0f) / (float)W - 2.0f / (float)W - radius;
	const float bx_hi = 1.0f - (2.0f * tx0 + 1.0f) / (float)W + 2.0f / (float)W + radius;
	const float by_lo = 1.0f - (2.0f * yl + 1.0f) / (float)H - 2.0f / (float)H - radius;
	const float by_hi = 1.0f - (2.0f * ty0 + 1.0f) / (float)H + 2.0f / (float)H + radius;
	const float r2 = radius * radius;
	const float* Rm = R + view * 9;
	const float* Tm = T + view * 3;
	const float* cp = points + (int64_t)cloud * P * 3;

	float bz[KMAX], bd[KMAX];
	int bi[KMAX];
#pragma unroll
	for (int k = 0; k < KMAX; ++k) { bz[k] = __builtin_inff(); bd[k] = -1.f; bi[k] = -1; }

	for (int base = 0; base < P; base += THREADS) {
		// ---- collect: project, cull against the tile, append the survivors in point order
		const int p = base + tid;
		float4 e = make_float4(0.f, 0.f, -1.f, 0.f);
		if (p < P) {
			// (no contraction: every product and sum rounds on its own, so the projection is reproducible off the device to the bit -- the
			// splat weight amplifies an NDC rounding by 2 / r = 67, and the tests compare weights to 1e-5)
#pragma clang fp contract(off)
			const float* q = cp + (int64_t)p * 3;
			const float x = q[0] * Rm[0] + q[1] * Rm[3] + q[2] * Rm[6] + Tm[0];
			const float y = q[0] * Rm[1] + q[1] * Rm[4] + q[2] * Rm[7] + Tm[1];
			const float z = q[0] * Rm[2] + q[1] * Rm[5] + q[2] * Rm[8] + Tm[2];
			e = make_float4(s * x / z, s * y / z, z, __int_as_float(p));
		}
		// (NaN coordinates fail every comparison and are dropped, as they fail the per-pixel test)
		const bool keep = p < P && e.z >= 0.f && e.x >= bx_lo && e.x <= bx_hi && e.y >= by_lo && e.y <= by_hi;
		const uint64_t ballot = __ballot(keep);
		const int rank = __popcll(ballot & ((1ull << lane) - 1ull));
		if (lane == 0) wave_count[wave] = __popcll(ballot);
		__syncthreads();
		int off = 0, n = 0;
#pragma unroll
		for (int w = 0; w < WAVES; ++w) {
			const int c = wave_count[w];
			off += w < wave ? c : 0;
			n += c;
		}
		if (keep) list[off + rank] = e;
		__syncthreads();
		// ---- walk: every thread tests its pixel against the list, in point order
		for (int j = 0; j < n; ++j) {
			const float4 c = list[j];
			float d2;
			{
#pragma clang fp contract(off)
				const float dx = px - c.x, dy = py - c.y;
				d2 = dx * dx + dy * dy;
			}
			// sorted insertion: the first slot of larger z takes the candidate, every slot behind it moves one down.  Only slots 0 .. K-1
			// are read out; what is pushed beyond them is dropped, so a candidate not nearer than slot K-1 changes nothing read (no
			// runtime-K test in the loop: it cost a mask register per slot).  The branch is wave-uniform: a divergent one doubled the
			// registers of the K-buffer.
			const bool take = d2 < r2;
			if (__any(take)) {
				float z = take ? c.z : __builtin_inff(), d = d2;
				int i = __float_as_int(c.w);
				bool shift = false;
#pragma unroll
				for (int k = 0; k < KMAX; ++k) {
					shift = shift || z < bz[k];
					const float tz = bz[k], td = bd[k];
					const int ti = bi[k];
					bz[k] = shift ? z : tz; bd[k] = shift ? d : td; bi[k] = shift ? i : ti;
					z = shift ? tz : z; d = shift ? td : d; i = shift ? ti : i;
				}
			}
		}
		__syncthreads();   // (the list is rewritten by the next chunk)
	}
	if (xi >= W || yi >= H) return;

	const int64_t pix = ((int64_t)img * H + yi) * W + xi;
	if (image) {
		const float* cf = features + (int64_t)cloud * P * 3;
		float o0 = 0.f, o1 = 0.f, o2 = 0.f, cum = 1.f;
#pragma unroll
		for (int k = 0; k < KMAX; ++k) {
			if (k < K && bi[k] >= 0) {
				const float w = 1.0f - bd[k] / r2;
				const float* f = cf + (int64_t)bi[k] * 3;
				o0 += f[0] * cum * w;
				o1 += f[1] * cum * w;
				o2 += f[2] * cum * w;
				cum = cum * (1.0f - w);
			}
		}
		image[pix * 3 + 0] = o0;
		image[pix * 3 + 1] = o1;
		image[pix * 3 + 2] = o2;
	}
	const int64_t fo = pix * K;
#pragma unroll
	for (int k = 0; k < KMAX; ++k) {
		if (k < K) {
			const bool full = bi[k] >= 0;
			if (idx_out) idx_out[fo + k] = bi[k];
			if (zbuf_out) zbuf_out[fo + k] = full ? bz[k] : -1.f;
			if (dists_out) dists_out[fo + k] = full ? bd[k] : -1.f;
		}
	}
}

}  // namespace points
}  // namespace find

using namespace find;
using namespace find::points;

extern "C" int find_points_render(const find_points_params* pp, const float* points, const float* features, const float* R, const float* T,
								  int64_t n_clouds, int64_t n_views, int64_t P, float* image, int32_t* idx, float* zbuf, float* dists,
								  void* stream) {
	FIND_REQUIRE(pp && points && R && T, "find_points_render: NULL argument");
	FIND_REQUIRE(image || idx || zbuf || dists, "find_points_render: no output requested");
	FIND_REQUIRE(!image || features, "find_points_render: the image needs features");
	const int K = pp->points_per_pixel;
	FIND_REQUIRE(K >= 1 && K <= 32, "find_points_render: points_per_pixel %d outside 1 .. 32", K);
	FIND_REQUIRE(pp->radius > 0.f && pp->radius < 1e30f, "find_points_render: radius %g must be > 0 and finite", (double)pp->radius);
	FIND_REQUIRE(pp->fov_deg > 0.f && pp->fov_deg < 180.f, "find_points_render: fov_deg %g outside (0, 180)", (double)pp->fov_deg);
	const int64_t H = pp->image_h, W = pp->image_w;
	FIND_REQUIRE(H >= 1 && W >= 1 && H <= MAX_IMAGE && W <= MAX_IMAGE, "find_points_render: image %lld x %lld outside 1 .. %lld", (long long)H,
				 (long long)W, (long long)MAX_IMAGE);
	FIND_REQUIRE(n_clouds >= 1 && n_views >= 1 && P >= 0 && P <= MAX_POINTS && n_clouds * n_views <= (1 << 24),
				 "find_points_render: bad sizes (n_clouds %lld, n_views %lld, P %lld)", (long long)n_clouds, (long long)n_views, (long long)P);
	const int64_t tiles_x = cdiv(W, TILE), n_tiles = tiles_x * cdiv(H, TILE);
	const int64_t n_blocks = n_clouds * n_views * n_tiles;
	FIND_REQUIRE(n_blocks <= 0x7fffffffll, "find_points_render: too many tiles (%lld)", (long long)n_blocks);
	const float s = 1.0f / tanf(pp->fov_deg * 3.14159265358979323846f / 180.0f * 0.5f);
	hipStream_t st = (hipStream_t)stream;
	if (K <= 16)
		hipLaunchKernelGGL((points_render_kernel<16>), dim3((unsigned)n_blocks), dim3(THREADS), 0, st, points, features, R, T, s, (int)n_views, (int)P,
						   (int)H, (int)W, (int)tiles_x, (int)n_tiles, pp->radius, K, image, idx, zbuf, dists);
	else
		hipLaunchKernelGGL((points_render_kernel<32>), dim3((unsigned)n_blocks), dim3(THREADS), 0, st, points, features, R, T, s, (int)n_views, (int)P,
						   (int)H, (int)W, (int)tiles_x, (int)n_tiles, pp->radius, K, image, idx, zbuf, dists);
	FIND_LAUNCH_CHECK("points_render_kernel");
	return FIND_OK;
}
