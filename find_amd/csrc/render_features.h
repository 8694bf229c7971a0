// Per-vertex feature render (FootRenderer.forward(..., return_features=True, features=...)): reference src/model/renderer.py:293-299,
// FeatureShader (lines 74-105) = TexturesVertex.sample_textures [P3D-recall: interpolate_face_attributes] on the SILHOUETTE fragments
// (K nearest, blurred, clipped perspective-correct barycentrics), then softmax_blend (lines 23-72) called with its DEFAULT znear = 1,
// zfar = 100 (not the camera's 0.02), sigma = gamma = 1e-4 and a background of C zeros.  Included by render.hip; runs after a
// find_render_fwd that formed the mask and reads its workspace: the tile lists (tinfo / pool), the face records, and the K-set the
// rasteriser settled per pixel (zthr / tie_face, the same test sil_bwd_kernel makes).
//
// Per pixel, over the candidates k of its K-set (p_k = sigmoid(-d_k / sigma), z_k the clipped depth, t_k the interpolated feature):
//   w_k = p_k exp((z_inv_k - z_inv_max) / gamma),  z_inv = (zfar - z) / (zfar - znear),  z_inv_max = max(eps, max_k z_inv_k)
//   out = sum_k w_k t_k / (sum_k w_k + delta),      delta = max(exp((eps - z_inv_max) / gamma), eps)
// The exponent is formed from depth differences, (z_min - z_k) / ((zfar - znear) gamma): the fp32 z_inv of the reference loses ~8e-4 of
// each weight to the rounding of (100 - z) / 99 (the tests hold both to float64).  Empty slots of the reference hold z_inv = 0 and weight
// 0: they never win the max over eps, and add nothing.
//
// Backward (a_k = dL/dw_k = (G . t_k - G . out) / D, D the denominator, G = dL/dout):
//   own path      dL/dz_k = -a_k w_k / ((zfar - znear) gamma),  dL/dp_k = a_k w_k / p_k
//   z_inv_max     sum_k a_k (-w_k / gamma) + dL/ddelta ddelta/dz_inv_max = -(G . out) delta / (gamma D) + [delta unclamped] (G . out) delta / (gamma D)
//                 (sum_k a_k w_k = (G . out) delta / D exactly): zero unless delta sits at its eps clamp -- FIND's case, where it is
//                 (G . out) eps / (gamma D), routed to the candidate that torch.max returns: the nearest, ties to the earlier K-buffer
//                 slot, which is the lower face index.  It cancels the own path of that candidate to the last digit for a pixel with one
//                 candidate, and must not be dropped.
namespace find {
namespace render {

constexpr int FEAT_CC = 16;              // channels per pass (registers of the accumulators; more channels: one more walk per 16)
constexpr float FEAT_ZNEAR = 1.0f, FEAT_ZFAR = 100.0f, FEAT_EPS = 1e-10f;   // softmax_blend's defaults (renderer.py:27-28, 44)
constexpr int FREC_STRIDE = REC_DW + 4;  // floats between two staged records (a stride of 32 dwords put every record on the same banks)

struct FeatArgs {
	const FaceRec* recs;
	const float4* frec;
	const uint32_t* tb;
	const int32_t* zinfo;
	const int2* tinfo;
	const uint32_t* pool;
	int64_t pool_cap;
	const float* zthr;
	const int32_t* tie_face;
	const int32_t* faces;
	int64_t faces_mesh_stride;
	const float* feat;       // (n_meshes, V, C)
	float* out;              // (n_img, H, W, C)
	float4* fpix;            // (n_img, H, W): z_min, D, face of z_min, G . out (the backward's prepass)
	int C, V, F, n_views, H, W, tiles_x, tiles_per_img, total_tiles;
	float blur, inv_sigma, gamma;
	int ablate;
};

// z_inv_max's clamp: the factor exp((z_inv(z_min) - z_inv_max) / gamma) that takes exp((z_min - z) / ((zfar - znear) gamma)) to the
// reference's weight (1 unless every candidate lies behind zfar), and delta
__device__ __forceinline__ void feat_norm(float zmin, float gamma, float* fsc, float* delta, bool* delta_clamped) {
	const float zi = zmin < INFINITY ? (FEAT_ZFAR - zmin) / (FEAT_ZFAR - FEAT_ZNEAR) : 0.f;
	const float zimax = fmaxf(FEAT_EPS, zi);
	*fsc = zi >= FEAT_EPS ? 1.0f : expf((zi - FEAT_EPS) / gamma);
	const float raw = expf((FEAT_EPS - zimax) / gamma);
	*delta_clamped = !(raw >= FEAT_EPS);
	*delta = fmaxf(raw, FEAT_EPS);
}

// Forward: one wave per 8 x 8 tile, a lane per pixel.  The wave walks the tile's face list (depth-slab order; every face of the image when
// the pool had no room) 64 faces at a time: each lane stages one face record and its three vertices' features (FEAT_CC channels) in LDS,
// then every lane evaluates the 64 for its own pixel with eval_core -- the rasteriser's rounding, so the depth compared with the K-set
// bound is the rasteriser's to the bit.  The blend is an online softmax (a running nearest depth, the sums rescaled when it moves: the
// list is only roughly front to back).  A wave leaves the list when every pixel's K-set bound lies in front of the next batch's slab.
// More than FEAT_CC channels: one more launch per FEAT_CC, c0 (the nearest depth is then known, no rescaling).  No atomics.
__global__ __launch_bounds__(64) void feat_fwd_kernel(const FeatArgs a, int c0) {
	// (one wave per workgroup: the 21.5 kB of staging per wave then let seven waves share a CU's LDS; four per workgroup left one workgroup)
	__shared__ __attribute__((aligned(16))) float srec[64 * FREC_STRIDE];
	__shared__ float sfeat[64 * 3 * FEAT_CC];
	const int lane = threadIdx.x & 63;
	const int t_id = blockIdx.x;
	const unsigned long long lt = (1ull << lane) - 1ull;
	const int img = t_id / a.tiles_per_img, tile = t_id - img * a.tiles_per_img;
	const int mesh = img / a.n_views;
	const int tile_x = tile % a.tiles_x, tile_y = tile / a.tiles_x;
	const int H = a.H, W = a.W, C = a.C;
	const int xi = tile_x * T8 + (lane & 7), yi = tile_y * T8 + (lane >> 3);
	const bool in_img = xi < W && yi < H;
	const float px = 1.0f - (2.0f * xi + 1.0f) / (float)W;
	const float py = 1.0f - (2.0f * yi + 1.0f) / (float)H;
	const int64_t pix = ((int64_t)img * H + min(yi, H - 1)) * W + min(xi, W - 1);
	const float zt = in_img ? a.zthr[pix] : 0.f;
	const int tfc = (in_img && zt < 0.f) ? a.tie_face[pix] : 0;
	const float zbound = fabsf(zt);   // every member of the K-set lies at or in front of it (+inf: every candidate is a member)
	int2 ti = a.tinfo[t_id];
	ti.x = __builtin_amdgcn_readfirstlane(ti.x); ti.y = __builtin_amdgcn_readfirstlane(ti.y);
	const bool binned = ti.y >= 0;
	const int n_list = binned ? (int)((uint32_t)ti.y & ~LIST_UNSORTED) : a.F;
	const bool sorted = binned && !((uint32_t)ti.y & LIST_UNSORTED);
	const bool early = sorted && !(a.ablate & 8);
	float zlo = 0.f, sw = 1.f;
	slab_layout(a.zinfo + img * 8, &zlo, &sw);
	const uint32_t* tbp = a.tb + (int64_t)img * a.F;
	const FaceRec* rp_img = a.recs + (int64_t)img * a.F;
	const uint32_t* lp = a.pool + (int64_t)img * a.pool_cap + ti.x;
	const int32_t* fmesh = a.faces + (int64_t)mesh * a.faces_mesh_stride;
	const float* feat_mesh = a.feat + (int64_t)mesh * a.V * C;
	const float s_inv = 1.0f / ((FEAT_ZFAR - FEAT_ZNEAR) * a.gamma);
	const int n_batches = (n_list + 63) >> 6;
	// chunk c0 > 0: the nearest depth and the denominator are the first chunk's (fpix), the weights need no rescaling
	const bool first = c0 == 0;
	float zmin = INFINITY, S = 0.f, D = 1.f, fsc = 1.f, delta = 1.f;
	int kf = -1;
	bool dcl;
	if (!first && in_img) {
		const float4 st = a.fpix[pix];
		zmin = st.x; D = st.y;
		feat_norm(zmin, a.gamma, &fsc, &delta, &dcl);
	}
	const int cn = min(FEAT_CC, C - c0);
	float acc[FEAT_CC];
#pragma unroll
	for (int c = 0; c < FEAT_CC; ++c) acc[c] = 0.f;
	for (int b = 0; b < n_batches; ++b) {
		if (early) {
			// every face from this batch on has its fragments behind the lower edge of the batch's first slab
			const float front = slab_front((int)(lp[b * 64] >> 24), zlo, sw);
			if (__ballot(in_img && !(front > zbound)) == 0ull) break;
		}
		const int i = b * 64 + lane;
		int f = -1;
		if (i < n_list) {
			if (binned) f = (int)(lp[i] & FACE_MASK);
			else if (tile_hit(tbp[i], tile_x, tile_y)) f = i;
		}
		const unsigned long long have = __ballot(f >= 0);
		const int nb = (int)__popcll(have);
		if (nb == 0) continue;
		if (f >= 0) {
			const int pos = (int)__popcll(have & lt);
			const float4* src = reinterpret_cast<const float4*>(rp_img + f);
			float4* d = reinterpret_cast<float4*>(&srec[pos * FREC_STRIDE]);
#pragma unroll
			for (int k = 0; k < REC_F4; ++k) d[k] = src[k];
			const int32_t* fv = fmesh + (int64_t)f * 3;
			float* sf = &sfeat[pos * 3 * FEAT_CC];
			for (int v = 0; v < 3; ++v) {
				const float* fp = feat_mesh + (int64_t)fv[v] * C + c0;
#pragma unroll
				for (int c = 0; c < FEAT_CC; ++c) sf[v * FEAT_CC + c] = c < cn ? fp[c] : 0.f;
			}
		}
		wave_lds_sync();
		for (int j = 0; j < nb; ++j) {
			const float* rr = &srec[j * FREC_STRIDE];
			const float4 bb = *reinterpret_cast<const float4*>(rr + 28);   // blurred bbox: xmin xmax ymin ymax
			const bool inb = in_img && px <= bb.y && px >= bb.x && py <= bb.w && py >= bb.z;
			if (__ballot(inb) == 0ull) continue;
			if (!inb) continue;
			const FaceRec r = load_rec(reinterpret_cast<const float4*>(rr));
			Frag fr;
			eval_core(r, px, py, &fr);
			if (!(fr.pz_clip >= 0.f && (fr.inside || fr.dist < a.blur))) continue;
			const float z = fr.pz_clip;
			if (zt < 0.f ? (z > zbound || (z == zbound && r.f > tfc)) : z > zt) continue;   // not among the K nearest
			const float p = silhouette_prob(fr.inside ? -fr.dist : fr.dist, a.inv_sigma);
			if (first && (z < zmin || (z == zmin && r.f < kf))) {
				if (z < zmin) {
					const float rs = zmin < INFINITY ? __expf((z - zmin) * s_inv) : 0.f;
					S *= rs;
#pragma unroll
					for (int c = 0; c < FEAT_CC; ++c) acc[c] *= rs;
					zmin = z;
				}
				kf = r.f;
			}
			const float w = p * __expf((zmin - z) * s_inv);
			S += w;
			const float c0w = fmaxf(fr.w0, 0.f), c1w = fmaxf(fr.w1, 0.f), c2w = fmaxf(fr.w2, 0.f);
			const float isum = 1.0f / fmaxf(c0w + c1w + c2w, 1e-5f);
			const float b0 = c0w * isum * w, b1 = c1w * isum * w, b2 = c2w * isum * w;
			const float* sf = &sfeat[j * 3 * FEAT_CC];
#pragma unroll
			for (int c = 0; c < FEAT_CC; ++c) acc[c] += b0 * sf[c] + b1 * sf[FEAT_CC + c] + b2 * sf[2 * FEAT_CC + c];
		}
		wave_lds_sync();   // the next batch overwrites the staging
	}
	if (!in_img) return;
	if (first) {
		feat_norm(zmin, a.gamma, &fsc, &delta, &dcl);
		D = S * fsc + delta;
		a.fpix[pix] = make_float4(zmin, D, __int_as_float(kf), 0.f);
	}
	const float sc = fsc / D;
	float* o = a.out + pix * C + c0;
#pragma unroll
	for (int c = 0; c < FEAT_CC; ++c)
		if (c < cn) o[c] = acc[c] * sc;
}

// Backward prepass: G . out per pixel, beside the forward's state
__global__ __launch_bounds__(256) void feat_gdot_kernel(const float* __restrict__ out, const float* __restrict__ d_out, int64_t n_px, int C,
														float4* __restrict__ fpix) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_px) return;
	const float* o = out + i * C;
	const float* g = d_out + i * C;
	float s = 0.f;
	for (int c = 0; c < C; ++c) s += g[c] * o[c];
	fpix[i].w = s;
}

// d w'_i (perspective-correct, unclipped barycentrics) -> NDC (x, y) and view depth of the face's three vertices, added into g[9]
// (BarycentricPerspectiveCorrectionBackward + BarycentricCoordsBackward, the chain rgb_pixel_grad uses; x0..z2 the fp32 vertices)
__device__ __forceinline__ void bary_ndc_bwd(float x0, float y0, float z0, float x1, float y1, float z1, float x2, float y2, float z2,
											 float px, float py, const float* d_bw, float* g) {
	const float area = edge_fn(x2, y2, x0, y0, x1, y1) + KEPS;
	const float e0 = edge_fn(px, py, x1, y1, x2, y2), e1 = edge_fn(px, py, x2, y2, x0, y0), e2 = edge_fn(px, py, x0, y0, x1, y1);
	const float inv_area = 1.0f / area;
	const float w0 = e0 * inv_area, w1 = e1 * inv_area, w2 = e2 * inv_area;
	const float t0 = w0 * z1 * z2, t1 = z0 * w1 * z2, t2 = z0 * z1 * w2;
	// w'_i = t_i / max(sum t, eps): below eps (a sliver seen far outside its outline: the perspective sum changes sign) the divisor is the
	// constant eps, as the forward's (and the reference's) clamp -- the gradient still flows through t (rgb_pixel_grad stops there instead:
	// its pixels lie inside their face)
	const float den = t0 + t1 + t2;
	const bool live = den > KEPS;
	const float inv_den = 1.0f / (live ? den : KEPS);
	const float sdb = live ? (d_bw[0] * t0 + d_bw[1] * t1 + d_bw[2] * t2) * inv_den : 0.f;
	const float d_t0 = (d_bw[0] - sdb) * inv_den, d_t1 = (d_bw[1] - sdb) * inv_den, d_t2 = (d_bw[2] - sdb) * inv_den;
	const float d_w0 = d_t0 * z1 * z2, d_w1 = d_t1 * z0 * z2, d_w2 = d_t2 * z0 * z1;
	g[2] += d_t1 * w1 * z2 + d_t2 * z1 * w2;
	g[5] += d_t0 * w0 * z2 + d_t2 * z0 * w2;
	g[8] += d_t0 * w0 * z1 + d_t1 * z0 * w1;
	const float d_e0 = d_w0 * inv_area, d_e1 = d_w1 * inv_area, d_e2 = d_w2 * inv_area;
	const float d_area = -(d_w0 * w0 + d_w1 * w1 + d_w2 * w2) * inv_area;
	auto edge_bwd = [](float qx, float qy, float ax, float ay, float bx, float by, float ge, float& gax, float& gay, float& gbx, float& gby) {
		gax += ge * (-(by - ay) + (qy - ay));
		gay += ge * (-(qx - ax) + (bx - ax));
		gbx += ge * (-(qy - ay));
		gby += ge * (qx - ax);
	};
	edge_bwd(px, py, x1, y1, x2, y2, d_e0, g[3], g[4], g[6], g[7]);
	edge_bwd(px, py, x2, y2, x0, y0, d_e1, g[6], g[7], g[0], g[1]);
	edge_bwd(px, py, x0, y0, x1, y1, d_e2, g[0], g[1], g[3], g[4]);
	g[6] += d_area * (y1 - y0); g[7] += d_area * (-(x1 - x0));
	g[0] += d_area * (-(y1 - y0) + (y2 - y0)); g[1] += d_area * (-(x2 - x0) + (x1 - x0));
	g[3] += d_area * (-(y2 - y0)); g[4] += d_area * (x2 - x0);
}

// Backward, face-centric as sil_bwd_kernel: LPF lanes per (image, face) stride over the face's blurred bbox, recompute each fragment with
// eval_frag, keep the K-set members, and accumulate in registers the gradients of the face's three NDC vertices (GEOM: through the
// distance, the depth -- own path and z_inv_max path --, and the clipped perspective-correct barycentrics) and of their features
// (FEAT: channels c0 .. c0 + FEAT_CC).  One commit per (image, face): atomics into d_vproj and d_feat (the views of a mesh add up there).
template <int LPF, bool GEOM, bool FEAT>
__global__ __launch_bounds__(256) void feat_bwd_kernel(const FeatArgs a, const float* __restrict__ d_out, int c0, float* __restrict__ d_vproj,
													   float* __restrict__ d_feat) {
	const int img = blockIdx.y;
	const int sub = threadIdx.x & (LPF - 1);
	const int F = a.F, H = a.H, W = a.W, C = a.C;
	const int f = blockIdx.x * (256 / LPF) + threadIdx.x / LPF;
	const int64_t o = (int64_t)img * F + min(f, F - 1);
	const bool act = f < F && a.tb[o] != TB_EMPTY;
	const FaceRec r = a.recs[o];
	int xlo, xhi, ylo, yhi;
	pix_range(r.xmin, r.xmax, W, &xlo, &xhi);
	pix_range(r.ymin, r.ymax, H, &ylo, &yhi);
	const int bw = xhi - xlo + 1;
	const int npx = act ? max(bw, 0) * max(yhi - ylo + 1, 0) : 0;
	const int mesh = img / a.n_views;
	const int32_t* fp = a.faces + (int64_t)mesh * a.faces_mesh_stride + (int64_t)min(f, F - 1) * 3;
	const int v0 = fp[0], v1 = fp[1], v2 = fp[2];
	const float* F0 = a.feat + ((int64_t)mesh * a.V + v0) * C;
	const float* F1 = a.feat + ((int64_t)mesh * a.V + v1) * C;
	const float* F2 = a.feat + ((int64_t)mesh * a.V + v2) * C;
	const float4 fa = a.frec[o * 3], fb = a.frec[o * 3 + 1], fc = a.frec[o * 3 + 2];
	const float s_inv = 1.0f / ((FEAT_ZFAR - FEAT_ZNEAR) * a.gamma);
	const int cn = min(FEAT_CC, C - c0);
	float g[9];
#pragma unroll
	for (int k = 0; k < 9; ++k) g[k] = 0.f;
	float dF[3][FEAT_CC];
#pragma unroll
	for (int v = 0; v < 3; ++v)
#pragma unroll
		for (int c = 0; c < FEAT_CC; ++c) dF[v][c] = 0.f;
	const int bws = max(bw, 1);
	for (int pi = sub; pi < npx; pi += LPF) {
		const int yi = ylo + pi / bws, xi = xlo + pi % bws;
		const int64_t pix = ((int64_t)img * H + yi) * W + xi;
		const float px = 1.0f - (2.0f * xi + 1.0f) / (float)W;
		const float py = 1.0f - (2.0f * yi + 1.0f) / (float)H;
		Frag fr;
		if (!eval_frag(r, px, py, &fr)) continue;
		if (!(fr.pz_clip >= 0.f && (fr.inside || fr.dist < a.blur))) continue;
		const float z = fr.pz_clip;
		const float zt = a.zthr[pix];
		if (zt < 0.f ? (z > -zt || (z == -zt && f > a.tie_face[pix])) : z > zt) continue;
		const float4 st = a.fpix[pix];   // z_min, D, face of z_min, G . out
		float fsc, delta;
		bool dcl;
		feat_norm(st.x, a.gamma, &fsc, &delta, &dcl);
		const float invD = 1.0f / st.y;
		const float p = silhouette_prob(fr.inside ? -fr.dist : fr.dist, a.inv_sigma);
		const float e = __expf((st.x - z) * s_inv) * fsc;
		const float w = p * e;
		const float c0w = fmaxf(fr.w0, 0.f), c1w = fmaxf(fr.w1, 0.f), c2w = fmaxf(fr.w2, 0.f);
		const float csum = c0w + c1w + c2w;
		const float isum = 1.0f / fmaxf(csum, 1e-5f);
		const float cb[3] = {c0w * isum, c1w * isum, c2w * isum};
		const float* G = d_out + pix * C;
		if constexpr (FEAT) {
			const float wd = w * invD;
#pragma unroll
			for (int c = 0; c < FEAT_CC; ++c) {
				const float gc = c < cn ? G[c0 + c] * wd : 0.f;
				dF[0][c] += cb[0] * gc; dF[1][c] += cb[1] * gc; dF[2][c] += cb[2] * gc;
			}
		}
		if constexpr (GEOM) {
			float h0 = 0.f, h1 = 0.f, h2 = 0.f;   // G . feature of each vertex
			for (int c = 0; c < C; ++c) { const float gc = G[c]; h0 += gc * F0[c]; h1 += gc * F1[c]; h2 += gc * F2[c]; }
			const float gd = st.w;
			const float ak = (cb[0] * h0 + cb[1] * h1 + cb[2] * h2 - gd) * invD;   // dL / dw_k
			float dz = -ak * w * s_inv;
			if (f == __float_as_int(st.z) && dcl && fsc == 1.0f) dz += gd * delta * s_inv * invD;   // the z_inv_max path (header comment)
			// distance: p = sigmoid(-sd / sigma), sd = -dist inside, +dist outside
			const float dsd = ak * e * (-p * (1.0f - p) * a.inv_sigma);
			const float gdist = fr.inside ? -dsd : dsd;
			{
				const bool e0 = fr.edge == 0, e2 = fr.edge == 2;
				const float ga = gdist * 2.0f * (1.0f - fr.t), gb = gdist * 2.0f * fr.t;
				const float wax = ga * fr.qx, way = ga * fr.qy, wbx = gb * fr.qx, wby = gb * fr.qy;
				g[0] += e2 ? 0.f : wax; g[1] += e2 ? 0.f : way;
				g[3] += e0 ? wbx : (e2 ? wax : 0.f); g[4] += e0 ? wby : (e2 ? way : 0.f);
				g[6] += e0 ? 0.f : wbx; g[7] += e0 ? 0.f : wby;
			}
			// depth z = sum c_i z_i and texel = sum c_i F_i: d c_i, then the clip c_i = max(w'_i, 0) / max(sum, 1e-5)
			const float zv[3] = {fb.z, fb.w, fc.x};
			const float hv[3] = {h0, h1, h2};
			const float wd = w * invD;
			float dc[3], dcs = 0.f;
#pragma unroll
			for (int i = 0; i < 3; ++i) {
				dc[i] = wd * hv[i] + dz * zv[i];
				g[3 * i + 2] += dz * cb[i];
				dcs += dc[i] * cb[i];
			}
			const bool sum_live = csum > 1e-5f;
			const float wv[3] = {fr.w0, fr.w1, fr.w2};
			float d_bw[3];
#pragma unroll
			for (int i = 0; i < 3; ++i) d_bw[i] = wv[i] >= 0.f ? (sum_live ? dc[i] - dcs : dc[i]) * isum : 0.f;
			bary_ndc_bwd(fa.x, fa.y, fb.z, fa.z, fa.w, fb.w, fb.x, fb.y, fc.x, px, py, d_bw, g);
		}
	}
#pragma unroll
	for (int d = 1; d < LPF; d <<= 1) {
		if constexpr (GEOM) {
#pragma unroll
			for (int k = 0; k < 9; ++k) g[k] += __shfl_xor(g[k], d, 64);
		}
		if constexpr (FEAT) {
#pragma unroll
			for (int v = 0; v < 3; ++v)
#pragma unroll
				for (int c = 0; c < FEAT_CC; ++c) dF[v][c] += __shfl_xor(dF[v][c], d, 64);
		}
	}
	if (!act || sub != 0) return;
	const int vv[3] = {v0, v1, v2};
	if constexpr (GEOM) {
		float* dv = d_vproj + (int64_t)img * a.V * 3;
#pragma unroll
		for (int k = 0; k < 3; ++k)
#pragma unroll
			for (int c = 0; c < 3; ++c)
				if (g[3 * k + c] != 0.f) atomicAdd(dv + 3 * vv[k] + c, g[3 * k + c]);
	}
	if constexpr (FEAT) {
#pragma unroll
		for (int k = 0; k < 3; ++k) {
			float* df = d_feat + ((int64_t)mesh * a.V + vv[k]) * C + c0;
#pragma unroll
			for (int c = 0; c < FEAT_CC; ++c)
				if (c < cn && dF[k][c] != 0.f) atomicAdd(df + c, dF[k][c]);
		}
	}
}

}  // namespace render
}  // namespace find
