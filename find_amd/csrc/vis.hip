// Frames of a turntable spin (reference src/vis/mesh_turntable.py:60-61): a float render (n, h, w, c) becomes the bytes a video writer takes,
//   out = (uint8) min(max(255.f * x, 0.f), 255.f)          -- numpy's (255 * image).astype(np.uint8) for the in-range values a render holds:
//                                                            truncation toward zero; NaN -> 0, below 0 -> 0, above 1 -> 255
// and, with rot180, pixel (y, x) of image i is written to (h-1-y, w-1-x) (cv2.rotate(..., ROTATE_180): the pixels of an image in reverse
// order, the channels of a pixel in theirs).  HBM-bound: 4 B in and 1 B out per value, every value touched once.
//
// Two kernels.  frames_vec_kernel: a thread owns FOUR consecutive output pixels: C float4 loads of the four source pixels (consecutive too,
// read back to front under rot180) and C packed 32-bit stores.  It needs the pixels of an image to be a multiple of 4 and 16- / 4-byte
// aligned bases, which keeps every group inside one image and aligned.  frames_scalar_kernel: a thread per pixel, for every other shape
// (odd sizes; nothing is assumed about w * c).  Both are grid-stride loops with 64-bit indices.
#include "common.h"

namespace find {
namespace vis {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 4096;   // 16 blocks per CU: grid-strided beyond that

__device__ __forceinline__ uint32_t to_u8(float x) {
	// (fmaxf returns the operand that is a number: NaN -> 0.  The product is rounded to fp32 before the conversion, as numpy's is.)
	return (uint32_t)fminf(fmaxf(255.f * x, 0.f), 255.f);
}

// n_groups = n_img * (n_pix / 4); group g covers output pixels 4 * gi .. 4 * gi + 3 of image g / (n_pix / 4)
template <int C, bool ROT>
__global__ __launch_bounds__(THREADS) void frames_vec_kernel(const float* __restrict__ img, int64_t n_groups, int64_t groups_per_img,
															  uint32_t* __restrict__ out) {
	for (int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x; g < n_groups; g += (int64_t)gridDim.x * THREADS) {
		int64_t src = g;
		if constexpr (ROT) {
			const int64_t i = g / groups_per_img, gi = g - i * groups_per_img;
			src = i * groups_per_img + (groups_per_img - 1 - gi);
		}
		float v[4 * C];   // the four source pixels, in memory order
#pragma unroll
		for (int k = 0; k < C; ++k) {
			const float4 x = reinterpret_cast<const float4*>(img)[src * C + k];
			v[4 * k] = x.x; v[4 * k + 1] = x.y; v[4 * k + 2] = x.z; v[4 * k + 3] = x.w;
		}
		uint32_t b[4 * C];   // the four output pixels, in memory order
#pragma unroll
		for (int p = 0; p < 4; ++p)
#pragma unroll
			for (int ch = 0; ch < C; ++ch) b[p * C + ch] = to_u8(v[(ROT ? 3 - p : p) * C + ch]);
#pragma unroll
		for (int k = 0; k < C; ++k) out[g * C + k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
	}
}

__global__ __launch_bounds__(THREADS) void frames_scalar_kernel(const float* __restrict__ img, int64_t n_img, int64_t n_pix, int C, int rot180,
																 uint8_t* __restrict__ out) {
	const int64_t total = n_img * n_pix;
	for (int64_t o = (int64_t)blockIdx.x * THREADS + threadIdx.x; o < total; o += (int64_t)gridDim.x * THREADS) {
		int64_t s = o;
		if (rot180) {
			const int64_t i = o / n_pix, p = o - i * n_pix;
			s = i * n_pix + (n_pix - 1 - p);
		}
		for (int ch = 0; ch < C; ++ch) out[o * C + ch] = (uint8_t)to_u8(img[s * C + ch]);
	}
}

inline bool al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <int C>
inline void launch_vec(const float* img, int64_t n_img, int64_t n_pix, bool rot, uint32_t* out, hipStream_t s) {
	const int64_t gpi = n_pix >> 2, n_groups = n_img * gpi;
	const dim3 grid((unsigned)std::min<int64_t>(cdiv(n_groups, THREADS), MAX_BLOCKS));
	if (rot)
		hipLaunchKernelGGL((frames_vec_kernel<C, true>), grid, dim3(THREADS), 0, s, img, n_groups, gpi, out);
	else
		hipLaunchKernelGGL((frames_vec_kernel<C, false>), grid, dim3(THREADS), 0, s, img, n_groups, gpi, out);
}

}  // namespace vis
}  // namespace find

using namespace find;
using namespace find::vis;

extern "C" int find_frames_u8(const float* img, int64_t n, int64_t h, int64_t w, int64_t c, int rot180, uint8_t* out, void* stream) {
	FIND_REQUIRE(img && out, "find_frames_u8: NULL argument");
	FIND_REQUIRE(n >= 1 && h >= 1 && w >= 1 && c >= 1 && c <= 16 && n <= (1ll << 24) && h <= (1ll << 16) && w <= (1ll << 16) && n * h * w * c <= (1ll << 40),
				 "find_frames_u8: bad sizes (n %lld, h %lld, w %lld, c %lld)", (long long)n, (long long)h, (long long)w, (long long)c);
	hipStream_t s = (hipStream_t)stream;
	int64_t n_img = n, n_pix = h * w;
	if (!rot180) {   // nothing ties a pixel to its image: one long row (more shapes reach the vector kernel)
		n_pix *= n_img;
		n_img = 1;
	}
	if ((n_pix & 3) == 0 && (c == 3 || c == 1) && al(img, 16) && al(out, 4)) {
		if (c == 3)
			launch_vec<3>(img, n_img, n_pix, rot180 != 0, (uint32_t*)out, s);
		else
			launch_vec<1>(img, n_img, n_pix, rot180 != 0, (uint32_t*)out, s);
		FIND_LAUNCH_CHECK("frames_vec_kernel");
		return FIND_OK;
	}
	const dim3 grid((unsigned)std::min<int64_t>(cdiv(n_img * n_pix, THREADS), MAX_BLOCKS));
	hipLaunchKernelGGL(frames_scalar_kernel, grid, dim3(THREADS), 0, s, img, n_img, n_pix, (int)c, rot180 != 0 ? 1 : 0, out);
	FIND_LAUNCH_CHECK("frames_scalar_kernel");
	return FIND_OK;
}
