// 2-D part loss: what the reference's RestylePerceptualLoss.forward(mode='cluster', pred_logit=...) does after its encoder
// (src/model/losses.py:251-302; applied in ModelWithLoss.forward, src/model/model.py:1129-1147).  Upstream permutes the rendered logits
// to (B, C, H, W), resamples both logit tensors to the render size, writes channel 0, and runs CrossEntropyLoss, a product and a mean:
// six or more passes over B*H*W*C floats each way.  Here:
//   labels_kernel   label = argmax_c bilinear(gt_logits -> (H, W)), the resampled tensor never stored;
//   ce_fwd_kernel   z_0 = 100 where mask == 0 else 0, z_c = logits_c (c >= 1);  ce = logsumexp z - z_label;  ce_out = ce * mask;
//                   one double partial per workgroup;  sum_kernel adds the partials in a fixed order and divides by P;
//   ce_bwd_kernel   d_logits_c = g / P * mask * (softmax(z)_c - [c == label]) (c >= 1), d_logits_0 = 0, d_mask = g / P * ce.
// The logits are channel-last (P, C), exactly as the feature render returns them.  These kernels are bound by memory: the STAGED form
// moves a tile of pixels between global memory and LDS with 16-byte accesses (consecutive lanes, consecutive addresses) and gives every
// lane one LDS row of odd pitch (lane l, channel c -> bank (l * pitch + c) % 32: no conflict); the DIRECT form lets a lane walk its
// pixel's C floats in global memory with stride-C scalar accesses (any C, any alignment).  No atomics: two runs agree bit for bit.
// A label outside [0, C) gives NaN for that pixel and the loss; nothing is read through it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "find_hip.h"
#include "common.h"

namespace find {
namespace partloss {

constexpr int MAX_THREADS = 256;               // pixels per tile = threads per workgroup: 256, 128 or 64 (what fits TILE_BYTES)
constexpr int64_t TILE_BYTES = 40 * 1024;      // LDS per workgroup of the staged form: three or more workgroups per CU
constexpr int SUM_THREADS = 256;

__device__ __forceinline__ int pitch_of(int C) { return C | 1; }

// tile rows [0, np) of pitch `pitch` <- the np * C floats at src (16-byte aligned): 16-byte loads, consecutive lanes consecutive addresses
__device__ __forceinline__ void tile_load(float* tile, const float* __restrict__ src, int np, int C, int pitch) {
	const int n = np * C, n4 = n >> 2;
	for (int i = threadIdx.x; i < n4; i += blockDim.x) {
		const float4 v = reinterpret_cast<const float4*>(src)[i];
		const float vv[4] = {v.x, v.y, v.z, v.w};
		const int e = 4 * i, p = e / C;
		int c = e - p * C;
		float* d = tile + p * pitch + c;
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			*d++ = vv[k];
			if (++c == C) {
				c = 0;
				d += pitch - C;
			}
		}
	}
	for (int e = 4 * n4 + threadIdx.x; e < n; e += blockDim.x) tile[(e / C) * pitch + e % C] = src[e];
}

// the reverse: np * C floats at dst (16-byte aligned) <- tile rows [0, np), 16-byte stores
__device__ __forceinline__ void tile_store(float* __restrict__ dst, const float* tile, int np, int C, int pitch) {
	const int n = np * C, n4 = n >> 2;
	for (int i = threadIdx.x; i < n4; i += blockDim.x) {
		const int e = 4 * i, p = e / C;
		int c = e - p * C;
		const float* s = tile + p * pitch + c;
		float vv[4];
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			vv[k] = *s++;
			if (++c == C) {
				c = 0;
				s += pitch - C;
			}
		}
		reinterpret_cast<float4*>(dst)[i] = make_float4(vv[0], vv[1], vv[2], vv[3]);
	}
	for (int e = 4 * n4 + threadIdx.x; e < n; e += blockDim.x) dst[e] = tile[(e / C) * pitch + e % C];
}

// max and sum of exp(z - max) over one pixel's z (z_0 given, channels 1 .. C-1 from row)
template <typename Row>
__device__ __forceinline__ void softmax_stats(Row row, int C, float z0, float& mx, float& s) {
	mx = z0;
	for (int c = 1; c < C; ++c) mx = fmaxf(mx, row[c]);
	s = expf(z0 - mx);
	for (int c = 1; c < C; ++c) s += expf(row[c] - mx);
}

// the workgroup's sum of v in double, fixed order (butterfly per wave, then the waves in order): thread 0 returns it
__device__ __forceinline__ double block_sum(double v, double* wsum) {
	v = wave_sum(v);
	if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
	__syncthreads();
	double t = 0.0;
	if (threadIdx.x == 0)
		for (int k = 0; k < (int)(blockDim.x >> 6); ++k) t += wsum[k];
	return t;
}

template <bool STAGED>
__global__ __launch_bounds__(MAX_THREADS) void ce_fwd_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
															 const float* __restrict__ mask, int64_t P, int C, float* __restrict__ ce_out,
															 double* __restrict__ partial) {
	extern __shared__ double smem[];
	double* wsum = smem;                                   // MAX_THREADS / 64 doubles
	float* tile = reinterpret_cast<float*>(smem + MAX_THREADS / 64);
	const int64_t p0 = (int64_t)blockIdx.x * blockDim.x;
	const int np = (int)min((int64_t)blockDim.x, P - p0);
	const int pitch = pitch_of(C);
	if (STAGED) {
		tile_load(tile, logits + p0 * C, np, C, pitch);
		__syncthreads();
	}
	double v = 0.0;
	if ((int)threadIdx.x < np) {
		const int64_t p = p0 + threadIdx.x;
		const float m = mask[p];
		const int lab = labels[p];
		const float z0 = (m == 0.f) ? 100.f : 0.f;
		float mx, s, ce;
		if (STAGED) {
			const float* row = tile + threadIdx.x * pitch;
			softmax_stats(row, C, z0, mx, s);
			ce = (lab < 0 || lab >= C) ? __builtin_nanf("") : (mx - (lab == 0 ? z0 : row[lab])) + logf(s);
		} else {
			const float* __restrict__ row = logits + p * C;
			softmax_stats(row, C, z0, mx, s);
			ce = (lab < 0 || lab >= C) ? __builtin_nanf("") : (mx - (lab == 0 ? z0 : row[lab])) + logf(s);
		}
		const float out = ce * m;
		ce_out[p] = out;
		v = (double)out;
	}
	const double t = block_sum(v, wsum);
	if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// loss = (sum of the n partials) / P: thread t adds partials t, t + 256, ... in that order, then the threads are added in a fixed order
__global__ __launch_bounds__(SUM_THREADS) void sum_kernel(const double* __restrict__ partial, int64_t n, double inv_p, float* __restrict__ loss_out) {
	__shared__ double wsum[SUM_THREADS / 64];
	double acc = 0.0;
	for (int64_t i = threadIdx.x; i < n; i += SUM_THREADS) acc += partial[i];
	const double t = block_sum(acc, wsum);
	if (threadIdx.x == 0) *loss_out = (float)(t * inv_p);
}

template <bool STAGED>
__global__ __launch_bounds__(MAX_THREADS) void ce_bwd_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
															 const float* __restrict__ mask, int64_t P, int C, const float* __restrict__ d_loss,
															 double inv_p, float* __restrict__ d_logits, float* __restrict__ d_mask) {
	extern __shared__ double smem[];
	float* tile = reinterpret_cast<float*>(smem);
	const int64_t p0 = (int64_t)blockIdx.x * blockDim.x;
	const int np = (int)min((int64_t)blockDim.x, P - p0);
	const int pitch = pitch_of(C);
	if (STAGED) {
		tile_load(tile, logits + p0 * C, np, C, pitch);
		__syncthreads();
	}
	if ((int)threadIdx.x < np) {
		const int64_t p = p0 + threadIdx.x;
		const float m = mask[p];
		const int lab = labels[p];
		const float z0 = (m == 0.f) ? 100.f : 0.f;
		const float g = (float)((double)*d_loss * inv_p);
		const bool bad = lab < 0 || lab >= C;
		const float nan = __builtin_nanf("");
		// the gradient replaces the logits of the lane's own LDS row (STAGED) or goes straight to global memory (DIRECT)
		const float* in = STAGED ? tile + threadIdx.x * pitch : logits + p * C;
		float* out = STAGED ? tile + threadIdx.x * pitch : d_logits + p * C;
		float mx, s;
		softmax_stats(in, C, z0, mx, s);
		const float ce = bad ? nan : (mx - (lab == 0 ? z0 : in[lab])) + logf(s);
		const float coef = bad ? nan : g * m, inv_s = 1.f / s;
		for (int c = 1; c < C; ++c) out[c] = coef * (expf(in[c] - mx) * inv_s - (c == lab ? 1.f : 0.f));
		out[0] = bad ? nan : 0.f;
		d_mask[p] = g * ce;
	}
	if (STAGED) {
		__syncthreads();
		tile_store(d_logits + p0 * C, tile, np, C, pitch);
	}
}

__global__ __launch_bounds__(256) void labels_kernel(const float* __restrict__ g, int64_t total, int C, int h, int w, int H, int W, float sy, float sx,
													 int32_t* __restrict__ labels) {
	const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= total) return;
	const int x = (int)(idx % W);
	const int y = (int)((idx / W) % H);
	const int64_t b = idx / ((int64_t)W * H);
	// torch's upsample_bilinear2d, align_corners=False: source index, its two neighbours (the last row / column repeats) and weights
	const float fy = fmaxf(sy * ((float)y + 0.5f) - 0.5f, 0.f), fx = fmaxf(sx * ((float)x + 0.5f) - 0.5f, 0.f);
	const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
	const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
	const float ly1 = fy - (float)y0, ly0 = 1.f - ly1, lx1 = fx - (float)x0, lx0 = 1.f - lx1;
	const int64_t plane = (int64_t)h * w;
	const float* gb = g + b * C * plane;
	const int o00 = y0 * w + x0, o01 = y0 * w + x1, o10 = y1 * w + x0, o11 = y1 * w + x1;
	float best = 0.f;
	int at = 0;
	for (int c = 0; c < C; ++c) {
		const float* q = gb + c * plane;
		const float v = ly0 * (lx0 * q[o00] + lx1 * q[o01]) + ly1 * (lx0 * q[o10] + lx1 * q[o11]);
		if (c == 0 || v > best || (v != v && best == best)) {   // first maximum; a NaN counts as the maximum (torch.argmax)
			best = v;
			at = c;
		}
	}
	labels[idx] = at;
}

// threads per workgroup (= pixels per tile) of the staged form, 0 when not even 64 pixels fit
inline int staged_threads(int64_t C) {
	const int64_t pitch = C | 1;
	for (int t = MAX_THREADS; t >= 64; t >>= 1)
		if (t * pitch * 4 <= TILE_BYTES) return t;
	return 0;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace partloss
}  // namespace find

using namespace find;

extern "C" int find_part_labels(const float* gt_logits, int64_t B, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W, int32_t* labels, void* stream) {
	FIND_REQUIRE(gt_logits && labels, "find_part_labels: NULL argument");
	FIND_REQUIRE(B >= 1 && C >= 1 && C < (1 << 16) && h >= 1 && w >= 1 && h < (1 << 15) && w < (1 << 15) && H >= 1 && W >= 1 && H < (1 << 15) && W < (1 << 15),
				 "find_part_labels: bad sizes B=%lld C=%lld %lldx%lld -> %lldx%lld", (long long)B, (long long)C, (long long)h, (long long)w, (long long)H,
				 (long long)W);
	const int64_t total = B * H * W;
	FIND_REQUIRE(total < ((int64_t)1 << 38), "find_part_labels: %lld pixels", (long long)total);
	hipLaunchKernelGGL(partloss::labels_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), gt_logits, total,
					   (int)C, (int)h, (int)w, (int)H, (int)W, (float)h / (float)H, (float)w / (float)W, labels);
	FIND_LAUNCH_CHECK("partloss labels_kernel");
	return FIND_OK;
}

// the form a call runs: FIND_PART_DIRECT or FIND_PART_STAGED, or -1 with the error set
static int part_form(const char* who, int64_t form, int64_t C, const void* a, const void* b, int* threads) {
	const int t = partloss::staged_threads(C);
	const bool fits = t > 0 && partloss::aligned16(a) && partloss::aligned16(b);
	if (form == FIND_PART_STAGED && !fits) {
		set_error("%s: the staged form needs C <= %lld and 16-byte aligned logits (C=%lld)", who, (long long)(partloss::TILE_BYTES / 256 - 1), (long long)C);
		return -1;
	}
	if (form != FIND_PART_AUTO && form != FIND_PART_DIRECT && form != FIND_PART_STAGED) {
		set_error("%s: form %lld (FIND_PART_AUTO / _DIRECT / _STAGED)", who, (long long)form);
		return -1;
	}
	const bool staged = form == FIND_PART_STAGED || (form == FIND_PART_AUTO && fits);
	*threads = staged ? t : partloss::MAX_THREADS;
	return staged ? FIND_PART_STAGED : FIND_PART_DIRECT;
}

extern "C" int find_part_ce_fwd(const float* logits, const int32_t* labels, const float* mask, int64_t P, int64_t C, float* loss_out, float* ce_out,
								double* partial_ws, int64_t form, void* stream) {
	FIND_REQUIRE(logits && labels && mask && loss_out && ce_out && partial_ws, "find_part_ce_fwd: NULL argument");
	FIND_REQUIRE(P >= 1 && P < ((int64_t)1 << 36) && C >= 1 && C < (1 << 16), "find_part_ce_fwd: bad sizes P=%lld C=%lld", (long long)P, (long long)C);
	int threads = 0;
	const int f = part_form("find_part_ce_fwd", form, C, logits, logits, &threads);
	if (f < 0) return FIND_EINVAL;
	hipStream_t s = reinterpret_cast<hipStream_t>(stream);
	const int64_t blocks = cdiv(P, threads);   // (<= cdiv(P, 64): the size of partial_ws)
	const size_t wsum = partloss::MAX_THREADS / 64 * sizeof(double);
	if (f == FIND_PART_STAGED)
		hipLaunchKernelGGL(partloss::ce_fwd_kernel<true>, dim3((unsigned)blocks), dim3(threads), wsum + (size_t)threads * (C | 1) * 4, s, logits, labels, mask,
						   P, (int)C, ce_out, partial_ws);
	else
		hipLaunchKernelGGL(partloss::ce_fwd_kernel<false>, dim3((unsigned)blocks), dim3(threads), wsum, s, logits, labels, mask, P, (int)C, ce_out,
						   partial_ws);
	FIND_LAUNCH_CHECK("partloss ce_fwd_kernel");
	hipLaunchKernelGGL(partloss::sum_kernel, dim3(1), dim3(partloss::SUM_THREADS), 0, s, partial_ws, blocks, 1.0 / (double)P, loss_out);
	FIND_LAUNCH_CHECK("partloss sum_kernel");
	return FIND_OK;
}

extern "C" int find_part_ce_bwd(const float* logits, const int32_t* labels, const float* mask, int64_t P, int64_t C, const float* d_loss, float* d_logits,
								float* d_mask, int64_t form, void* stream) {
	FIND_REQUIRE(logits && labels && mask && d_loss && d_logits && d_mask, "find_part_ce_bwd: NULL argument");
	FIND_REQUIRE(P >= 1 && P < ((int64_t)1 << 36) && C >= 1 && C < (1 << 16), "find_part_ce_bwd: bad sizes P=%lld C=%lld", (long long)P, (long long)C);
	int threads = 0;
	const int f = part_form("find_part_ce_bwd", form, C, logits, d_logits, &threads);
	if (f < 0) return FIND_EINVAL;
	hipStream_t s = reinterpret_cast<hipStream_t>(stream);
	const int64_t blocks = cdiv(P, threads);
	if (f == FIND_PART_STAGED)
		hipLaunchKernelGGL(partloss::ce_bwd_kernel<true>, dim3((unsigned)blocks), dim3(threads), (size_t)threads * (C | 1) * 4, s, logits, labels, mask, P,
						   (int)C, d_loss, 1.0 / (double)P, d_logits, d_mask);
	else
		hipLaunchKernelGGL(partloss::ce_bwd_kernel<false>, dim3((unsigned)blocks), dim3(threads), 0, s, logits, labels, mask, P, (int)C, d_loss,
						   1.0 / (double)P, d_logits, d_mask);
	FIND_LAUNCH_CHECK("partloss ce_bwd_kernel");
	return FIND_OK;
}
