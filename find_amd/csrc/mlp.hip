// C-ABI: find_mlp_fwd / find_mlp_bwd  -- launch sequences over the kernels in mlp_kernels.h: dims + workspaces, launches, forward,
// backward, entry points (the context, its streams and the fork / join of a call: mlp_ctx.h).
// Replaces NeuralDisplacementField.forward (reference src/model/model.py:393-453) and its autograd backward.
#include "mlp_dw2.h"
#include "mlp_dw4.h"
#include "mlp_dwpe.h"
#include "mlp_dwpe6.h"
#include "mlp_gemm5.h"
#include "mlp_gemm6.h"
#include "mlp_gemm7.h"
#include "mlp_dw3.h"
#include "mlp_dw6.h"
#include "mlp_gemm4.h"
#include "mlp_fused.h"
#include "mlp_fused6.h"
#include "mlp_ctx.h"

namespace find {
namespace mlp {

struct Dims {
	int64_t pos_batch, n_feet, V;
	bool shared;      // one set of positions evaluated for every foot: trunk computed once
	int64_t rows_t;   // trunk rows
	int64_t rows_h;   // head rows
	int64_t feet_t;   // grid.y of trunk launches
	int nchunk0;      // K chunks of trunk layer 0
	int nkt0;         // 256-wide k tiles of trunk layer 0 (dW)
};

static int make_dims(const find_mlp_params* p, int64_t pos_batch, int64_t n_feet, int64_t V, Dims* d) {
	FIND_REQUIRE(p != nullptr, "find_mlp: params is NULL");
	FIND_REQUIRE(p->width == W, "find_mlp: only width=256 is supported (got %d)", p->width);
	FIND_REQUIRE(p->in_dim == 3, "find_mlp: only in_dim=3 is supported (got %d)", p->in_dim);
	FIND_REQUIRE(p->pe_size >= 0 && p->pe_size <= 256 && p->pe_size % 32 == 0, "find_mlp: pe_size must be a multiple of 32 in [0,256] (got %d)", p->pe_size);
	FIND_REQUIRE(p->n_trunk >= 1 && p->n_trunk <= FIND_MAX_LAYERS, "find_mlp: n_trunk out of range (%d)", p->n_trunk);
	FIND_REQUIRE(p->n_disp >= 1 && p->n_disp < FIND_MAX_LAYERS, "find_mlp: n_disp out of range (%d)", p->n_disp);
	FIND_REQUIRE(p->n_col >= 1 && p->n_col < FIND_MAX_LAYERS, "find_mlp: n_col out of range (%d)", p->n_col);
	FIND_REQUIRE(p->lat_disp >= 0 && p->lat_col >= 0, "find_mlp: negative latent size");
	FIND_REQUIRE(n_feet >= 1 && V >= 1, "find_mlp: empty batch (n_feet=%lld, n_pts=%lld)", (long long)n_feet, (long long)V);
	FIND_REQUIRE(pos_batch == 1 || pos_batch == n_feet, "find_mlp: pos_batch must be 1 or n_feet (got %lld vs %lld)", (long long)pos_batch, (long long)n_feet);
	FIND_REQUIRE(V < (1ll << 31) / 256 && n_feet < (1 << 16), "find_mlp: batch too large for the launch grid");
	d->pos_batch = pos_batch; d->n_feet = n_feet; d->V = V;
	d->shared = (pos_batch == 1 && n_feet > 1);
	d->rows_t = pos_batch * V;
	d->rows_h = n_feet * V;
	d->feet_t = pos_batch;
	const int nsc = p->pe_size >> 4;
	d->nchunk0 = nsc + 1;
	d->nkt0 = (int)cdiv((nsc + 1) * 32, 256);
	return FIND_OK;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int check_weights(const find_mlp_params* p) {
	FIND_REQUIRE(p->pe_size == 0 || p->B != nullptr, "find_mlp: B is NULL");
	for (int i = 0; i < p->n_trunk; ++i) {
		FIND_REQUIRE(p->trunk_w[i] && p->trunk_b[i], "find_mlp: trunk layer %d weight/bias NULL", i);
		if (i > 0) FIND_REQUIRE(aligned16(p->trunk_w[i]), "find_mlp: trunk_w[%d] must be 16-byte aligned", i);
	}
	for (int i = 0; i <= p->n_disp; ++i) {
		FIND_REQUIRE(p->disp_w[i] && p->disp_b[i], "find_mlp: disp layer %d weight/bias NULL", i);
		if (i > 0) FIND_REQUIRE(aligned16(p->disp_w[i]), "find_mlp: disp_w[%d] must be 16-byte aligned", i);
	}
	for (int i = 0; i <= p->n_col; ++i) {
		FIND_REQUIRE(p->col_w[i] && p->col_b[i], "find_mlp: col layer %d weight/bias NULL", i);
		if (i > 0) FIND_REQUIRE(aligned16(p->col_w[i]), "find_mlp: col_w[%d] must be 16-byte aligned", i);
	}
	return FIND_OK;
}

// Forward workspace.  With save=false the hidden activations ping-pong between two buffers per stage.
// 16-k steps of the weight stream a chain of this model can need at most (forward: Fourier layer + trunk + both heads; backward: both
// heads + the two-operand trunk-output product + trunk), and the bytes of its fragment-ordered planes (mlp_fused6.h)
static int64_t chain_w6_bytes(const find_mlp_params* p) {
	const int64_t steps = 2 * (KP0 / KC + 1) + 16 * (int64_t)(p->n_trunk + p->n_disp + p->n_col + 4);
	return 8 * steps * F6_STEP_BYTES;
}

struct FwdWs {
	float* w0p;   // (256, KP0) layer-0 weight in padded PE order
	float* wd0;   // (256,256) main block of mlp_disp.0.weight
	float* wc0;   // (256,256) main block of mlp_col.0.weight
	float* fbd;   // (n_feet,256) per-foot bias of the disp head's first layer
	float* fbc;
	float* H[FIND_MAX_LAYERS];
	float* D[FIND_MAX_LAYERS];
	float* C[FIND_MAX_LAYERS];
	float* zd;    // (rows_h,3)
	float* zc;
	float* hp;    // shared template: (V,256) product of the trunk output with a head's first-layer weight (no bias), reused per head
	float* hp2;
	void* w6;     // fused6_kernel: the chain's weights as fragment-ordered bf16 planes (chain_w6_bytes)
	int64_t bytes;
};

static void carve_fwd(const find_mlp_params* p, const Dims& d, bool save, void* ws, FwdWs* o) {
	Carver c(ws);
	o->w0p = c.take<float>((int64_t)W * KP0);
	o->wd0 = c.take<float>((int64_t)W * W);
	o->wc0 = c.take<float>((int64_t)W * W);
	o->fbd = c.take<float>(d.n_feet * W);
	o->fbc = c.take<float>(d.n_feet * W);
	o->zd = c.take<float>(d.rows_h * 3);
	o->zc = c.take<float>(d.rows_h * 3);
	o->hp = (d.shared && d.n_feet > 1) ? c.take<float>(d.V * W) : nullptr;
	o->hp2 = (d.shared && d.n_feet > 1) ? c.take<float>(d.V * W) : nullptr;   // the colour head's copy: the heads run on two streams
	o->w6 = c.take<char>(chain_w6_bytes(p));
	float* pt[2] = {nullptr, nullptr};
	float* pd[2] = {nullptr, nullptr};
	float* pc[2] = {nullptr, nullptr};
	for (int i = 0; i < p->n_trunk; ++i) {
		if (save || !pt[i & 1]) pt[i & 1] = c.take<float>(d.rows_t * W);
		o->H[i] = pt[i & 1];
	}
	for (int i = 0; i < p->n_disp; ++i) {
		if (save || !pd[i & 1]) pd[i & 1] = c.take<float>(d.rows_h * W);
		o->D[i] = pd[i & 1];
	}
	for (int i = 0; i < p->n_col; ++i) {
		if (save || !pc[i & 1]) pc[i & 1] = c.take<float>(d.rows_h * W);
		o->C[i] = pc[i & 1];
	}
	o->bytes = c.off;
}

// row splits of a slab-producing launch: about `target` workgroups over all feet, cps 32-row chunks each
static void split_policy(int64_t n_feet, int64_t V, int* spf, int* cps, int64_t target = 128) {
	const int64_t cpf = cdiv(V, 32);
	int64_t s0 = std::max<int64_t>(1, std::min<int64_t>(cpf, cdiv(target, n_feet)));
	*cps = (int)cdiv(cpf, s0);
	*spf = (int)cdiv(cpf, *cps);
}

// Backward scratch.
struct BwdWs {
	float* Tt[FIND_MAX_LAYERS];  // transposed trunk weights (layers >= 1)
	float* Dt[FIND_MAX_LAYERS];  // transposed disp-head weights (layer 0: main block)
	float* Ct[FIND_MAX_LAYERS];
	float* dzD[FIND_MAX_LAYERS];  // one per head layer (as dzT)
	float* dzC[FIND_MAX_LAYERS];
	float* dzT[FIND_MAX_LAYERS];  // one per trunk layer: the dX chain never waits for the side stream's readers
	float* pw;    // dW partial slabs
	float* pb;    // bias partial slabs
	float* pw_t[4];  // slab sets: [0] aliases pw / pb (stream q), [1], [2] the trunk's side streams, [3] alternates with [0] on q
	float* pb_t[4];
	float* Sd;    // (n_feet,256) per-foot column sums of the disp head's first-layer dZ
	float* Sc;
	float* zsD;   // shared template: (V,256) sum over feet of the disp head's first-layer dZ
	float* zsC;
	float* fs1D;  // footsum_fold: the second partial sum of gemm7_kernel<.., FSUM> (the first lands in zsD / zsC)
	float* fs1C;
	float* pS;    // [nblk_fs][n_feet][256] partial per-foot column sums (disp head)
	float* pS2;   // same for the colour head: the reduces run on the side stream, so the heads cannot share one
	int nblk_fs;
	float* pwo[2];  // final-layer partials
	float* pbo[2];
	int nblk_out;
	int64_t max_split;
	float* grp_pw;   // small calls: slabs of the grouped weight-gradient launch, [job][slab][256][256], then the bias rows [job][slab][256]
	int64_t grp_slabs;  // slabs per job
	int grp_jobs;
	void* w6;        // fused6_kernel: the dX chain's weights as fragment-ordered bf16 planes
	int64_t bytes;
};

constexpr int64_t GROUP_MAX_UNITS = 1024;   // largest call (32-row tiles) that may take the fused / grouped small-call path
constexpr int GROUP_MIN_CPS = 8;            // 16-row chunks per workgroup of a grouped weight gradient, at least

static void carve_bwd(const find_mlp_params* p, const Dims& d, void* scratch, BwdWs* o) {
	Carver c(scratch);
	for (int i = 1; i < p->n_trunk; ++i) o->Tt[i] = c.take<float>((int64_t)W * W);
	for (int i = 0; i < p->n_disp; ++i) o->Dt[i] = c.take<float>((int64_t)W * W);
	for (int i = 0; i < p->n_col; ++i) o->Ct[i] = c.take<float>((int64_t)W * W);
	for (int i = 0; i < std::max(p->n_disp, 1); ++i) o->dzD[i] = c.take<float>(d.rows_h * W);
	for (int i = 0; i < std::max(p->n_col, 1); ++i) o->dzC[i] = c.take<float>(d.rows_h * W);
	for (int i = 0; i < std::max(p->n_trunk, 1); ++i) o->dzT[i] = c.take<float>(d.rows_t * W);
	int spf, cps;
	split_policy(d.n_feet, d.V, &spf, &cps);
	int64_t ms = d.n_feet * spf;
	split_policy(1, d.V, &spf, &cps);
	ms = std::max<int64_t>(ms, spf);
	o->max_split = ms;
	// dw2 policy: up to max(#CUs, feet) main slabs + one tail slab per foot, each 256x256
	const int64_t ms2 = std::max<int64_t>(512, d.n_feet) + d.n_feet + 16;
	o->pw = c.take<float>(std::max<int64_t>(ms * W * KP0, ms2 * W * W));
	o->pb = c.take<float>(std::max<int64_t>(ms, ms2) * W);
	o->pw_t[0] = o->pw; o->pb_t[0] = o->pb;
	for (int i = 1; i < 4; ++i) {  // trunk layers have matrix inputs (dw2 slabs) except layer 0, which always uses set 0
		o->pw_t[i] = c.take<float>(ms2 * W * W);
		o->pb_t[i] = c.take<float>(ms2 * W);
	}
	o->Sd = c.take<float>(d.n_feet * W);
	o->Sc = c.take<float>(d.n_feet * W);
	o->nblk_fs = (int)cdiv(d.V, FS_ROWS);
	if (d.shared) {
		o->zsD = c.take<float>(d.V * W);
		o->zsC = c.take<float>(d.V * W);
		o->fs1D = c.take<float>(d.V * W);
		o->fs1C = c.take<float>(d.V * W);
	} else {
		o->zsD = o->zsC = o->fs1D = o->fs1C = nullptr;
	}
	// (also without a shared template: the latents-only backward of a frozen network takes its per-foot column sums this way)
	o->pS = c.take<float>((int64_t)o->nblk_fs * d.n_feet * W);
	o->pS2 = c.take<float>((int64_t)o->nblk_fs * d.n_feet * W);
	o->w6 = c.take<char>(chain_w6_bytes(p));
	o->grp_pw = nullptr; o->grp_slabs = 0; o->grp_jobs = 0;
	if (cdiv(d.V, 32) * d.feet_t <= GROUP_MAX_UNITS) {
		// (a shared trunk groups its own layers only: the heads' layers there have n_feet times the rows and keep their own launches)
		// (round 6: ... and the heads' FIRST layers, whose foot-summed gradient has the trunk's V rows)
		o->grp_jobs = d.shared ? (p->n_trunk - 1) + 2 : (p->n_trunk - 1) + p->n_disp + p->n_col;
		o->grp_slabs = std::max<int64_t>(d.feet_t * (cdiv(d.V / 16, GROUP_MIN_CPS) + 1), std::min<int64_t>(d.feet_t * cdiv(d.V / 16, 2), 32));
		if (o->grp_jobs > 0) o->grp_pw = c.take<float>((int64_t)o->grp_jobs * o->grp_slabs * ((int64_t)W * W + W));
	}
	o->nblk_out = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(d.rows_h, 64), 512));
	for (int i = 0; i < 2; ++i) {
		o->pwo[i] = c.take<float>((int64_t)o->nblk_out * 3 * W);
		o->pbo[i] = c.take<float>((int64_t)o->nblk_out * 4);
	}
	o->bytes = c.off;
}

// ------------------------------------------------------------------------------------------- launches
// One tile launch of a Linear-shaped kernel: LDS attribute and size (prepare_kernel), the tile arithmetic every such kernel shares, the launch.
struct TileLaunch { int id; int lds; int rows; int grid; int block; };   // kernel id (attr_done), LDS bytes needed, rows per tile, launch geometry

static int ntiles_of(int64_t V, int rows, int64_t feet) { return (int)((int)cdiv(V, rows) * feet); }

template <typename K>
static int launch_tiles(find_ctx* c, K kernel, const TileLaunch& t, Gemm2Args a, int64_t feet, hipStream_t s) {
	int lds = 0;
	FIND_TRY(prepare_kernel(c, t.id, kernel, t.lds, &lds));
	a.tiles_per_foot = (int)cdiv(a.V, t.rows);
	a.ntiles = (int)(a.tiles_per_foot * feet);
	hipLaunchKernelGGL(kernel, dim3(t.grid), dim3(t.block), lds, s, a);
	return FIND_OK;
}

// the runtime epilogue as a compile-time constant: f(std::integral_constant<int, EPI>)
template <typename F>
static int with_epi(int epi, F&& f) {
	if (epi == EPI_BIAS_RELU) return f(std::integral_constant<int, EPI_BIAS_RELU>{});
	if (epi == EPI_MASK) return f(std::integral_constant<int, EPI_MASK>{});
	return f(std::integral_constant<int, EPI_NONE>{});
}
constexpr int epi_slot(int epi) { return epi == EPI_BIAS_RELU ? 0 : epi == EPI_MASK ? 1 : 2; }   // the kernel ids of a family: .._RELU, .._MASK, .._NONE

static int launch_gemm2_pe(find_ctx* c, const Gemm2Args& a, int64_t feet, hipStream_t s) {
	constexpr int BM = 64;
	const int grid = std::min(ntiles_of(a.V, BM, feet), c->num_cus);
	return launch_tiles(c, &gemm2_kernel<BM, AMODE_PE, EPI_BIAS_RELU>, TileLaunch{K_GEMM2_PE, gemm2_lds_bytes<BM>(), BM, grid, 256}, a, feet, s);
}

static int launch_gemm3(find_ctx* c, int epi, const Gemm2Args& a, int64_t feet, hipStream_t s) {
	return with_epi(epi, [&](auto E) -> int {
		constexpr int EPI = decltype(E)::value, BM = 64;
		const int grid = std::min(ntiles_of(a.V, BM, feet), c->num_cus);
		return launch_tiles(c, &gemm3_kernel<BM, EPI>, TileLaunch{K_GEMM3_RELU + epi_slot(EPI), gemm2_lds_bytes<BM>(), BM, grid, 256}, a, feet, s);
	});
}

template <int NI>
static int launch_gemm4(find_ctx* c, int epi, const Gemm2Args& a, int64_t feet, hipStream_t s) {
	return with_epi(epi, [&](auto E) -> int {
		constexpr int EPI = decltype(E)::value, NW = 8;
		constexpr int G = 8 * (8 / NI);  // the column groups of a row range sit 8 blocks apart (same XCD)
		const int grid = std::max(G, (c->num_cus / G) * G);
		const int id = (NI == 4 ? K_GEMM4_4_RELU : K_GEMM4_2_RELU) + epi_slot(EPI);
		return launch_tiles(c, &gemm4_kernel<EPI, NI, NW>, TileLaunch{id, NI * 32 * 1024, 32, grid, NW * 64}, a, feet, s);
	});
}

static int launch_gemm5(find_ctx* c, int epi, const Gemm2Args& a, int64_t feet, hipStream_t s, bool h16) {
	return with_epi(epi, [&](auto E) -> int {
		constexpr int EPI = decltype(E)::value;
		const int grid = (int)std::min<int64_t>(c->num_cus, cdiv(ntiles_of(a.V, 32, feet), GEMM5_NW));
		const int block = GEMM5_NW * 64;
		if constexpr (EPI != EPI_NONE) {   // fp16-stored A / y / mask (act16): the two epilogues the heads' hidden layers use
			if (h16 && (EPI == EPI_BIAS_RELU ? a.va_bias : a.vm_bias)) {   // (bcast_fold: mlp_gemm5.h)
				Gemm2Args v = a;
				v.tile_major = 1;   // the feet of a tile side by side: the shared product behind the virtual operand is read from HBM once
				return launch_tiles(c, &gemm5_kernel<EPI, true, true>, TileLaunch{EPI == EPI_BIAS_RELU ? K_GEMM5_RELU_V : K_GEMM5_MASK_V, GEMM5_LDS_VIRT, 32, grid, block}, v, feet, s);
			}
			if (h16) return launch_tiles(c, &gemm5_kernel<EPI, true>, TileLaunch{EPI == EPI_BIAS_RELU ? K_GEMM5_RELU_H : K_GEMM5_MASK_H, GEMM5_LDS, 32, grid, block}, a, feet, s);
		} else if (h16) {
			set_error("launch_gemm5: no fp16-stored variant of this epilogue");
			return FIND_EINVAL;
		}
		return launch_tiles(c, &gemm5_kernel<EPI>, TileLaunch{K_GEMM5_RELU + epi_slot(EPI), GEMM5_LDS, 32, grid, block}, a, feet, s);
	});
}

// workgroup pairs of the folded-foot-sum launch: the usual count, but never so many that a pair's unit range is shorter than a tile's run of
// feet (mlp_gemm7.h FSUM: a tile then has at most two partial sums); 0 = the shape does not qualify
static int gemm7_fsum_pairs(const find_ctx* c, int64_t V, int64_t feet) {
	const int64_t upf = cdiv(V, 32);
	const int def = std::max(16, (c->num_cus / 16) * 16) / 2;
	const int pairs = (int)std::min<int64_t>(def, (upf / 8) * 8);   // (the two column halves of a pair sit 8 blocks apart: pairs come in eights)
	return (feet >= 2 && feet <= 64 && pairs >= 8) ? pairs : 0;
}

static int launch_gemm7(find_ctx* c, int epi, const Gemm2Args& a, int64_t feet, hipStream_t s) {
	return with_epi(epi, [&](auto E) -> int {
		constexpr int EPI = decltype(E)::value;
		const int grid = std::max(16, (c->num_cus / 16) * 16);   // the two column halves of a row range sit 8 blocks apart (same XCD)
		const int block = GEMM7_NW * 64;
		if constexpr (EPI == EPI_MASK) {
			if (a.vm_bias && a.fs_out) {   // (footsum_fold: mlp_gemm7.h FSUM)
				const int pairs = gemm7_fsum_pairs(c, a.V, feet);
				FIND_REQUIRE(pairs > 0, "launch_gemm7: shape does not qualify (footsum_fold and the kernel selection disagree)");
				Gemm2Args f = a;
				f.tile_major = 1;
				return launch_tiles(c, &gemm7_kernel<EPI_MASK, 0, true, true>, TileLaunch{K_GEMM7_MASK_VF, GEMM7_LDS + 64 * 128 * 4, 32, 2 * pairs, block}, f, feet, s);
			}
		}
		if constexpr (EPI != EPI_NONE) {
			if (EPI == EPI_BIAS_RELU ? a.va_bias : a.vm_bias)   // (bcast_fold: mlp_gemm7.h VIRT)
				return launch_tiles(c, &gemm7_kernel<EPI, 0, true>, TileLaunch{EPI == EPI_BIAS_RELU ? K_GEMM7_RELU_V : K_GEMM7_MASK_V, GEMM7_LDS, 32, grid, block}, a, feet, s);
		}
		return launch_tiles(c, &gemm7_kernel<EPI>, TileLaunch{K_GEMM7_RELU + epi_slot(EPI), GEMM7_LDS, 32, grid, block}, a, feet, s);
	});
}

// Kernel choice for one Linear-shaped launch (all of them exact fp32 unless the call runs in the opt-in fp16 mode):
//   Fourier layer                                   gemm2<64, PE>   (sin / cos generated into the A tile)
//   fp16 mode, K = 256, >= gemm5_min_units units    gemm5           (W resident as fp16, HBM-bound)
//   K = 256, >= gemm4_min_units / 2 32-row units    gemm4<4>        (W half resident in LDS, matrix-pipe-bound)
//   K = 256, >= gemm4_small units                   gemm4<2>        (column quarters: the shared trunk's V rows)
//   anything else (two-segment K, tiny launches)    gemm3<64>       (LDS-DMA ring)
// h16 (host side only): a0, y and mask are fp16-STORED tensors (act16: gemm5_kernel<EPI, true>)
static int launch_gemm(find_ctx* c, int amode, int epi, Gemm2Args a, int64_t feet, hipStream_t s, bool h16 = false) {
	a.ablate = c->ablate;
	if (amode == AMODE_PE) return launch_gemm2_pe(c, a, feet, s);
	const int64_t units = cdiv(a.V, 32) * feet;
	const bool k256 = a.nseg == 1 && a.nchunk == 8;
	// (gemm5 keeps the whole W per workgroup, so 216 units occupy 27 CUs: 22 us against 13 us for gemm4 on column quarters)
	if (c->f16 && k256 && units >= c->gemm5_min_units) return launch_gemm5(c, epi, a, feet, s, h16);
	FIND_REQUIRE(!h16, "launch_gemm: an fp16-stored layer reached a kernel that reads fp32 (act16 and the kernel selection disagree)");
	if (c->x3 && k256 && units >= c->gemm6_min_units) return launch_gemm7(c, epi, a, feet, s);
	FIND_REQUIRE(!a.va_bias && !a.vm_bias && !a.fs_out, "launch_gemm: a virtual operand reached a kernel that cannot form it (bcast_fold / footsum_fold and the kernel selection disagree)");
	FIND_REQUIRE(!a.w_tr, "launch_gemm: an untransposed weight reached a kernel that cannot read it (gemm7_direct and the kernel selection disagree)");
	if (k256 && units * 2 >= c->gemm4_min_units) return launch_gemm4<4>(c, epi, a, feet, s);
	if (k256 && c->gemm4_small && units >= c->gemm4_small) return launch_gemm4<2>(c, epi, a, feet, s);
	return launch_gemm3(c, epi, a, feet, s);
}

// a K = 256, one-segment launch of this many rows per foot goes to gemm7 (launch_gemm's rule): its dX form then reads the model's weight
// itself (Gemm2Args::w_tr) instead of a transposed copy
static bool gemm7_direct(const find_ctx* c, int64_t V, int64_t feet) {
	const int64_t units = cdiv(V, 32) * feet;
	return c->x3 && !(c->f16 && units >= c->gemm5_min_units) && units >= c->gemm6_min_units;
}
// a fused chain of this call will run on fused6_kernel (chain_prepare's rule): split_w_kernel reads every weight once anyway, in whatever
// order the step asks for (FusedStep::wmode) -- no repack launch in front of the chain
static bool chain_direct(const find_ctx* c) { return c->x3 && c->fused6; }

// ---- fused chains (mlp_fused.h): one launch takes every 32-row tile through a list of layers
struct Chain {
	FusedArgs a;
	int nt = 1;             // 32-row blocks per tile (chain_prepare)
	bool x3 = false;        // runs on fused6_kernel: its weights have been split (chain_prepare)
	bool prepared = false;
	int in_dim = 3;         // of the Fourier layer (wmode 2)
	Chain() { memset(&a, 0, sizeof(a)); }
	FusedStep& add() { return a.step[a.n_steps++]; }
	bool full(int more) const { return a.n_steps + more > FUSED_MAX_STEPS; }
	// y = epi(x @ w^T): x from LDS (the previous step's result) unless src is given
	FusedStep& gemm(const float* w, int ldw, int nchunk, const float* src = nullptr) {
		FusedStep& s = add();
		s.kind = FS_GEMM; s.w = w; s.ldw = ldw; s.nchunk = nchunk;
		s.src = src; s.src_kind = src ? FS_SRC_GLOBAL : FS_SRC_LDS;
		return s;
	}
};

// A chain runs in two halves: chain_prepare fixes the tile geometry and -- bf16x3 -- launches split_w_kernel (it needs the weights only, so a
// caller may issue it long before the chain's inputs exist: the shared trunk's backward chain does, right behind the transposes, instead of
// between the large weight-gradient kernels, where this 5-us launch waited 90 us for a free CU on the step's critical path); chain_launch
// starts the chain itself.
static int chain_prepare(find_ctx* c, Chain& ch, int64_t V, int64_t feet, hipStream_t s, void* w6, int64_t w6_bytes) {
	// more 32-row blocks than CUs: 64-row tiles (one round of workgroups instead of two, half the weight staging per MFMA)
	ch.nt = (cdiv(V, 32) * feet > c->num_cus && !(c->ablate & 128)) ? 2 : 1;
	ch.a.V = (int)V;
	ch.a.tiles_per_foot = (int)cdiv(V, 32 * ch.nt);
	ch.a.ntiles = (int)(ch.a.tiles_per_foot * feet);
	ch.x3 = false;
	ch.prepared = true;
	if (c->x3 && c->fused6 && w6 != nullptr) {
		// bf16x3: the chain's weights as fragment-ordered bf16 planes (one small launch), then the chain on the bf16 matrix pipe
		SplitWArgs sa;
		memset(&sa, 0, sizeof(sa));
		int maxn = 0;
		for (int i = 0; i < ch.a.n_steps; ++i) {
			const FusedStep& st = ch.a.step[i];
			if (st.kind != FS_GEMM) continue;
			const int n = 2 * st.nchunk;
			sa.job[sa.njobs++] = SplitWJob{st.w, st.ldw, n, sa.total, st.wmode, ch.a.pe, ch.in_dim};
			sa.total += n;
			maxn = std::max(maxn, n);
		}
		if (sa.njobs > 0 && 8 * (int64_t)sa.total * F6_STEP_BYTES <= w6_bytes) {
			sa.dst = reinterpret_cast<u32x4*>(w6);
			hipLaunchKernelGGL(split_w_kernel, dim3((unsigned)cdiv(8 * maxn * 64, 256), (unsigned)sa.njobs), dim3(256), 0, s, sa);
			FIND_LAUNCH_CHECK("split_w_kernel");
			ch.a.w6 = w6;
			ch.a.total_steps = sa.total;
			ch.x3 = true;
		}
	}
	if (!ch.x3)
		for (int i = 0; i < ch.a.n_steps; ++i)
			FIND_REQUIRE(ch.a.step[i].kind != FS_GEMM || ch.a.step[i].wmode == 0, "find_mlp: a chain with weights in model order did not get its bf16x3 kernel (chain_direct and chain_prepare disagree)");
	return FIND_OK;
}

static int chain_launch(find_ctx* c, Chain& ch, hipStream_t s) {
	const int nt = ch.nt;
	int lds = 0;
	if (ch.x3) {
		if (nt == 2) FIND_TRY(prepare_kernel(c, K_FUSED6_2, &fused6_kernel<2>, fused6_lds(2), &lds, false));
		else FIND_TRY(prepare_kernel(c, K_FUSED6, &fused6_kernel<1>, fused6_lds(1), &lds, false));
		if (nt == 2) hipLaunchKernelGGL(fused6_kernel<2>, dim3(ch.a.ntiles), dim3(FUSED_NW * 64), lds, s, ch.a);   // (one tile per workgroup)
		else hipLaunchKernelGGL(fused6_kernel<1>, dim3(ch.a.ntiles), dim3(FUSED_NW * 64), lds, s, ch.a);
		FIND_LAUNCH_CHECK("fused6_kernel");
		return FIND_OK;
	}
	const int grid = std::min(ch.a.ntiles, c->num_cus);
	if (nt == 2) FIND_TRY(prepare_kernel(c, K_FUSED2, &fused_chain_kernel<2>, fused_lds(2), &lds, false));
	else FIND_TRY(prepare_kernel(c, K_FUSED, &fused_chain_kernel<1>, fused_lds(1), &lds, false));   // no LDS-DMA in this kernel: no reservation
	if (nt == 2) hipLaunchKernelGGL(fused_chain_kernel<2>, dim3(grid), dim3(FUSED_NW * 64), lds, s, ch.a);
	else hipLaunchKernelGGL(fused_chain_kernel<1>, dim3(grid), dim3(FUSED_NW * 64), lds, s, ch.a);
	FIND_LAUNCH_CHECK("fused_chain_kernel");
	return FIND_OK;
}

static int launch_chain(find_ctx* c, Chain& ch, int64_t V, int64_t feet, hipStream_t s, void* w6 = nullptr, int64_t w6_bytes = 0) {
	if (!ch.prepared) FIND_TRY(chain_prepare(c, ch, V, feet, s, w6, w6_bytes));
	return chain_launch(c, ch, s);
}

static bool use_fused(const find_ctx* c, int64_t V, int64_t feet) {
	const int64_t units = cdiv(V, 32) * feet;
	if (c->f16 && units >= c->gemm5_min_units) return false;   // the opt-in fp16 kernels take launches of this size (the chain is fp32)
	return c->fused_max_units > 0 && units <= c->fused_max_units;
}

static Gemm2Args gemm_args() {
	Gemm2Args a;
	memset(&a, 0, sizeof(a));
	a.nseg = 1;
	return a;
}

// Linear + ReLU forward:  y = relu(x @ w^T + bias[foot])  (launch_gemm with EPI_BIAS_RELU)
static Gemm2Args linear_args(const float* x, int64_t x_foot_stride, const float* w, int ldw, const float* bias, int64_t bias_foot_stride, float* y, int64_t V) {
	Gemm2Args a = gemm_args();
	a.a0 = x; a.a_foot_stride = x_foot_stride; a.lda = W;
	a.w0 = w; a.ldw = ldw; a.nchunk = W / KC;
	a.bias = bias; a.bias_foot_stride = bias_foot_stride;
	a.y = y; a.y_foot_stride = V * W; a.ldy = W; a.V = (int)V;
	return a;
}

// act16: the opt-in fp16 mode STORES the heads' hidden activations (w.D / w.C) and their gradients (b.dzD / b.dzC) as fp16 when every
// kernel that touches them is one of the HBM-bound large-shape kernels: a template shared by more than one foot (bias_relu_bcast ->
// gemm5 -> head_out forward; head_out_bwd -> dw3 / gemm5 / footsum backward) with enough rows for gemm5.  Forward and backward of a
// call agree on it through a note the forward leaves in the context (note_act16), so a knob turned in between cannot split them.
static bool use_act16(const find_ctx* c, bool f16, bool shared, int64_t n_feet, int64_t V) {
	return f16 && c->act16 && shared && n_feet > 1 && cdiv(V, 32) * n_feet >= c->gemm5_min_units;
}
// bcast_fold (round 6): inside act16 the output of a head's broadcast first layer, h1 = fp16(relu(P[v] + bias[foot])), is never stored: its
// three readers (the second layer's forward GEMM, the ReLU mask of that layer's dX GEMM, the x operand of its weight gradient) form it from the
// V x 256 product P (w.hp / w.hp2, kept until the backward) and the bias rows -- gemm5_kernel<.., VIRT>, dw3_h16v_kernel.  Needs a second hidden layer.
// The same in the default bf16x3 arithmetic (fp32-stored activations): gemm7_kernel<.., VIRT>, dw6v_kernel -- wherever the heads' hidden
// layers of a shared template go to gemm7 / dw6 (launch_gemm's and weight_grad's rule).
static bool use_fold(const find_ctx* c, bool a16, bool shared, int64_t n_feet, int64_t V, const find_mlp_params* p) {
	if (!c->bcast_fold || p->n_disp < 2 || p->n_col < 2) return false;
	if (a16) return true;
	const int64_t units = cdiv(V, 32) * n_feet;
	return c->x3 && !c->f16 && shared && n_feet > 1 && units >= c->gemm6_min_units;
}
static void note_act16(find_ctx* c, const void* ws, bool a16, bool fold) {
	for (auto& n : c->act16_notes) if (n.ws == ws) { n.a16 = a16; n.fold = fold; return; }
	c->act16_notes[c->act16_next] = find_ctx::Act16Note{ws, a16, fold};
	c->act16_next = (c->act16_next + 1) & 15;
}
static int noted_act16(const find_ctx* c, const void* ws, bool by_rule, bool fold_by_rule) {   // bit 0: act16, bit 1: bcast_fold
	for (const auto& n : c->act16_notes) if (n.ws == ws) return (n.a16 ? 1 : 0) | (n.fold ? 2 : 0);
	return (by_rule ? 1 : 0) | (fold_by_rule ? 2 : 0);
}

static bool call_f16(const find_ctx* c, const find_mlp_params* p) { return p->precision == 2 || (p->precision == 0 && c->mlp_f16 == 1); }
static bool call_x3(const find_ctx* c, const find_mlp_params* p) { return p->precision == 3 || (p->precision == 0 && c->mlp_f16 == 2); }

// ------------------------------------------------------------------------------------------- forward
// Everything a call holds once per head: heads[0] the displacement head, heads[1] the colour head (make_heads).  The forward fields are
// set by every call, the backward ones (from `gout` on) by find_mlp_bwd.
struct Head {
	bool colour;
	int nl;                    // hidden layers; layer nl is the 3-wide output layer
	const float* const* w;     // the model's weights (p->disp_w / p->col_w) and biases
	const float* const* b;
	int ld0;                   // leading dimension of w[0]: 256 + L
	int L;                     // latent width
	const float* lat;
	const float* w0; int ldw0; // the first layer's main block as the forward's kernels read it: the repacked copy, or w[0] itself (chain_direct)
	float* fb;                 // (n_feet,256) per-foot bias of the first layer (latents folded in)
	const float* bias0; int64_t bstride0;   // the first layer's bias rows: fb with latents, b[0] without
	float* const* act;         // saved activations of the hidden layers
	float* z;
	float* hp;                 // shared template: (V,256) product of the trunk output with w0 (no bias)
	float* out;                // forward: the head's output, NULL = not evaluated
	const float* gout;         // upstream gradient, NULL = nothing read this head
	float* const* gw; float* const* gb; float* glat;
	float* const* dz; int cur; // dZ buffers, one per layer, and the one the dX chain has reached
	float* const* wt;          // transposed weights (layer 0: main block)
	float* S; float* zs; float* fs1; float* pS;   // (BwdWs: Sd / Sc ...)
	int side;                  // side stream (and slab set) of the first layer's weight gradient: T1 / T2
};

static void make_heads(Head* heads, const find_mlp_params* p, const FwdWs& w, const float* lat_disp, const float* lat_col, const BwdWs* b, const find_mlp_grads* g) {
	memset(heads, 0, 2 * sizeof(Head));
	Head& d = heads[0];
	Head& c = heads[1];
	c.colour = true;
	d.nl = p->n_disp; c.nl = p->n_col;
	d.w = p->disp_w; c.w = p->col_w;
	d.b = p->disp_b; c.b = p->col_b;
	d.L = p->lat_disp; c.L = p->lat_col;
	d.lat = lat_disp; c.lat = lat_col;
	d.w0 = w.wd0; c.w0 = w.wc0;
	d.fb = w.fbd; c.fb = w.fbc;
	d.act = w.D; c.act = w.C;
	d.z = w.zd; c.z = w.zc;
	d.hp = w.hp; c.hp = w.hp2;   // (the forward may give the colour head w.hp: see there)
	for (int k = 0; k < 2; ++k) {
		Head& h = heads[k];
		h.ld0 = W + h.L;
		h.ldw0 = W;
		h.bias0 = h.L > 0 ? h.fb : h.b[0];
		h.bstride0 = h.L > 0 ? W : 0;
		h.side = 1 + k;
	}
	if (!b) return;
	d.gw = g->disp_w; c.gw = g->col_w;
	d.gb = g->disp_b; c.gb = g->col_b;
	d.glat = g->lat_disp; c.glat = g->lat_col;
	d.dz = b->dzD; c.dz = b->dzC;
	d.wt = b->Dt; c.wt = b->Ct;
	d.S = b->Sd; c.S = b->Sc;
	d.zs = b->zsD; c.zs = b->zsC;
	d.fs1 = b->fs1D; c.fs1 = b->fs1C;
	d.pS = b->pS; c.pS = b->pS2;
}

static int mlp_fwd_body(Fork& fk, const find_mlp_params* p, const Dims& d, const FwdWs& w, const float* pos, Head* heads) {
	find_ctx* c = fk.c;
	hipStream_t s = fk.s;
	const int64_t V = d.V, n_feet = d.n_feet;
	Head& hd = heads[0];
	Head& hc = heads[1];
	const bool a16 = use_act16(c, c->f16, d.shared, n_feet, V);
	const bool fold = use_fold(c, a16, d.shared, n_feet, V, p);
	note_act16(c, w.fbd, a16, fold);   // (every forward leaves its note, keyed by a buffer every workspace has: the backward follows it)

	// 1. repack: layer-0 weight into padded PE order; main blocks of the two head input layers.  Not for a bf16x3 chain that carries the
	// whole call (or everything up to the heads' broadcast first layers): its weight split reads the model's tensors directly (round 6: this
	// launch sat in front of both MLP passes of a training step, 8 - 20 us each on the critical path)
	const bool fused = use_fused(c, V, d.feet_t) && p->pe_size > 0;
	const bool direct = fused && chain_direct(c);
	if (!direct) {
		RepackArgs ra;
		memset(&ra, 0, sizeof(ra));
		ra.njobs = 3;
		ra.job[0] = RepackJob{p->trunk_w[0], w.w0p, W, KP0, p->in_dim + 2 * p->pe_size, 0, KP0, 2, p->pe_size, p->in_dim};
		ra.job[1] = RepackJob{hd.w[0], w.wd0, W, W, hd.ld0, 0, W, 0, 0, 0};
		ra.job[2] = RepackJob{hc.w[0], w.wc0, W, W, hc.ld0, 0, W, 0, 0, 0};
		hipLaunchKernelGGL(repack_kernel, dim3(96, ra.njobs), dim3(256), 0, s, ra);
		FIND_LAUNCH_CHECK("repack_kernel");
	} else {
		for (int k = 0; k < 2; ++k) { heads[k].w0 = heads[k].w[0]; heads[k].ldw0 = heads[k].ld0; }
	}
	// 2. per-foot latent bias (model.py:428-437 as a bias)
	// (only for the heads this call evaluates: the template pass of a 3-D-loss step leaves the colour head out, the texture pass the other one)
	for (int k = 0; k < 2; ++k) {
		const Head& h = heads[k];
		if (h.L > 0 && h.out != nullptr)
			hipLaunchKernelGGL(latent_bias_kernel, dim3(W / 4, (unsigned)n_feet), dim3(256), 0, s, h.w[0], h.ld0, h.b[0], h.lat, h.L, h.fb);
	}
	FIND_LAUNCH_CHECK("latent_bias_kernel");

	// The heads are independent after the trunk.  With both active, the colour head runs on a side stream: its bandwidth-bound
	// pieces (the bias + ReLU broadcast, the 3-wide output layer: no LDS, so they can share CUs with the W-resident GEMMs) then
	// overlap the other head's matrix-pipe-bound layers.  Forked from and joined back into the caller's stream (Fork::join).
	const bool forked = hd.out && hc.out && fk.on;
	// (bcast_fold: the products stay until the backward -- the colour head's is ALWAYS hp2, the other head's hp)
	if (!(fold || forked || (fused && hd.out))) hc.hp = w.hp;

	// 3 (+ 4, 5 for small calls). trunk (model.py:421-426); layer 0 generates the Fourier features on the fly
	const bool fused_heads = fused && !(d.shared && n_feet > 1);   // per-foot rows: the heads are as small as the trunk
	if (fused) {
		Chain ch;
		ch.a.pos = pos; ch.a.pos_foot_stride = V * 3; ch.a.Bm = p->B; ch.a.pe = p->pe_size; ch.in_dim = p->in_dim;
		{
			// even chunk counts (the padding columns of w0p are zeros; wmode 2 reads them as zeros)
			FusedStep& s0 = direct ? ch.gemm(p->trunk_w[0], p->in_dim + 2 * p->pe_size, (d.nchunk0 + 1) & ~1) : ch.gemm(w.w0p, KP0, (d.nchunk0 + 1) & ~1);
			s0.wmode = direct ? 2 : 0;
			s0.src_kind = FS_SRC_PE; s0.relu = 1; s0.bias = p->trunk_b[0]; s0.dst = w.H[0]; s0.to_lds = 1;
		}
		for (int i = 1; i < p->n_trunk; ++i) {
			FusedStep& st = ch.gemm(p->trunk_w[i], W, W / KC);
			st.relu = 1; st.bias = p->trunk_b[i]; st.dst = w.H[i]; st.to_lds = 1;
		}
		const float* hlast = w.H[p->n_trunk - 1];
		if (!fused_heads) {
			// shared template: the first layer of each head is H W0^T on the V template rows (bias + ReLU are broadcast per foot below)
			for (int k = 0; k < 2; ++k)
				if (heads[k].out) { FusedStep& st = ch.gemm(heads[k].w0, heads[k].ldw0, W / KC); st.dst = heads[k].hp; }
		} else {
			auto head = [&](const Head& h, bool reload) {
				FusedStep& f0 = ch.gemm(h.w0, h.ldw0, W / KC, reload ? hlast : nullptr);
				f0.relu = 1; f0.bias = h.bias0; f0.bias_foot_stride = (int)h.bstride0; f0.dst = h.act[0]; f0.to_lds = 1;
				for (int i = 1; i < h.nl; ++i) {
					FusedStep& st = ch.gemm(h.w[i], W, W / KC);
					st.relu = 1; st.bias = h.b[i]; st.dst = h.act[i]; st.to_lds = 1;
				}
				FusedStep& o = ch.add();
				o.kind = FS_OUT; o.w = h.w[h.nl]; o.bias = h.b[h.nl]; o.dst = h.out; o.dst2 = h.z; o.head = (unsigned char)h.colour;
				o.aux = h.colour ? p->avg_col : nullptr;
			};
			if (hd.out) head(hd, false);
			if (hc.out) head(hc, hd.out != nullptr);
		}
		FIND_TRY(launch_chain(c, ch, V, d.feet_t, s, w.w6, chain_w6_bytes(p)));
		if (fused_heads) return FIND_OK;
	} else {
		Gemm2Args a = gemm_args();
		a.pos = pos; a.pos_foot_stride = V * 3; a.Bm = p->B; a.pe = p->pe_size;
		a.w0 = w.w0p; a.ldw = KP0; a.nchunk = d.nchunk0;
		a.bias = p->trunk_b[0]; a.bias_foot_stride = 0;
		a.y = w.H[0]; a.y_foot_stride = V * W; a.ldy = W; a.V = (int)V;
		FIND_TRY(launch_gemm(c, AMODE_PE, EPI_BIAS_RELU, a, d.feet_t, s));
		for (int i = 1; i < p->n_trunk; ++i)
			FIND_TRY(launch_gemm(c, AMODE_MAT, EPI_BIAS_RELU, linear_args(w.H[i - 1], V * W, p->trunk_w[i], W, p->trunk_b[i], 0, w.H[i], V), d.feet_t, s));
		FIND_LAUNCH_CHECK("trunk gemm");
	}

	// 4. heads (model.py:439-440); the trunk rows are shared by every foot when d.shared
	const float* hl = w.H[p->n_trunk - 1];
	const int64_t hl_stride = d.shared ? 0 : V * W;
	// first layer of a head.  Shared template: every foot multiplies the SAME trunk rows, so  H W^T  is formed once on V rows
	// and each foot only adds its (latent-folded) bias and applies the ReLU -- a bandwidth-bound broadcast instead of a GEMM
	// over n_feet * V rows.  (The backward uses the same fact: footsum_kernel.)
	auto head_first = [&](const Head& h, hipStream_t st) -> int {
		if (h.hp) {
			if (!fused) {   // (the fused trunk launch has already formed the product)
				Gemm2Args a = gemm_args();
				a.a0 = hl; a.a_foot_stride = 0; a.lda = W;
				a.w0 = h.w0; a.ldw = W; a.nchunk = W / KC;
				a.y = h.hp; a.y_foot_stride = V * W; a.ldy = W; a.V = (int)V;
				FIND_TRY(launch_gemm(c, AMODE_MAT, EPI_NONE, a, 1, st));
			}
			if (fold) return FIND_OK;   // (the second layer reads hp and the bias rows itself)
			hipLaunchKernelGGL(bias_relu_bcast_kernel, dim3((unsigned)cdiv(V * (W / 4), 256), (unsigned)cdiv(n_feet, BCAST_FEET)), dim3(256), 0, st, h.hp, h.bias0,
							   h.bstride0, (int)n_feet, V, h.act[0], a16 ? 1 : 0);
			return FIND_OK;
		}
		FIND_REQUIRE(!a16, "find_mlp_fwd: act16 without a shared template");
		return launch_gemm(c, AMODE_MAT, EPI_BIAS_RELU, linear_args(hl, hl_stride, h.w0, W, h.bias0, h.bstride0, h.act[0], V), n_feet, st);
	};
	// 5. final 256->3 layers + tanh scalings (model.py:444-449), one launch per head
	auto head_out = [&](int head, hipStream_t st) {
		HeadOutArgs h;
		memset(&h, 0, sizeof(h));
		for (int k = 0; k < 2; ++k) {
			h.x[k] = heads[k].act[heads[k].nl - 1];
			h.w[k] = heads[k].w[heads[k].nl];
			h.b[k] = heads[k].b[heads[k].nl];
			h.z[k] = heads[k].z;
			h.out[k] = heads[k].out;
		}
		h.avg_col = p->avg_col;
		h.rows = d.rows_h;
		h.head0 = head;
		h.x_half = a16 ? 1 : 0;
		const unsigned gx = (unsigned)std::min<int64_t>(cdiv(d.rows_h, 32), 2048);
		if (a16) hipLaunchKernelGGL(head_out_fwd_h16_kernel, dim3(gx, 1), dim3(256), 0, st, h);   // (fp16-stored activations: on the fp16 matrix pipe)
		else hipLaunchKernelGGL(head_out_fwd_kernel, dim3(gx, 1), dim3(256), 0, st, h);
	};
	auto head = [&](const Head& h, hipStream_t st) -> int {
		FIND_TRY(head_first(h, st));
		for (int i = 1; i < h.nl; ++i) {
			Gemm2Args a = linear_args(h.act[i - 1], V * W, h.w[i], W, h.b[i], 0, h.act[i], V);
			if (i == 1 && fold) {   // (x is the shared fp32 product, the operand relu(hp[v] + bias0[foot]): bcast_fold)
				a.a0 = h.hp; a.a_foot_stride = 0;
				a.va_bias = h.bias0; a.va_bias_stride = h.bstride0;
			}
			FIND_TRY(launch_gemm(c, AMODE_MAT, EPI_BIAS_RELU, a, n_feet, st, a16));
		}
		head_out(h.colour, st);
		return FIND_OK;
	};
	hipStream_t sc = s;
	if (forked) {
		fk.fork_to(1);
		sc = fk.stream(1);
	}
	if (hd.out) FIND_TRY(head(hd, s));
	if (hc.out) FIND_TRY(head(hc, sc));
	FIND_LAUNCH_CHECK("head layers");
	return FIND_OK;
}

// ------------------------------------------------------------------------------------------- backward
// One weight-gradient job: dW / db of one Linear layer from dz (rows (foot, v)) and its input x (or, for the Fourier layer, the positions).
struct Wgrad {
	const float* dz = nullptr;
	const float* x = nullptr;        // the layer's input; x_foot_stride 0 = rows shared by all feet
	int64_t x_foot_stride = 0;
	const float* pos = nullptr;      // Fourier layer: the inputs are regenerated from the positions (x unused)
	int64_t pos_foot_stride = 0;
	int nkt = 1;                     // Fourier layer: 256-wide k tiles (Dims::nkt0)
	int64_t feet = 1, V = 0;
	float* dw = nullptr;
	int ld_out = W;
	int k_valid = W;
	int pe_map = 0;                  // Fourier layer: columns go back to the model's order
	float* db = nullptr;
	float* S = nullptr;              // per-foot column sums of dz (latent gradients)
	hipStream_t s = nullptr;         // the partial tiles go out on s; the slab reduce follows on s, or -- reduce_side >= 0 -- on that side
	int s_side = -1;                 // stream of the fork, ordered behind s (= side stream s_side)
	int reduce_side = -1;
	bool h16 = false;                // dz and x fp16-stored (act16)
	const float* vx_bias = nullptr;  // bcast_fold: x is the shared product P, the operand relu(P[v] + vx_bias[foot])
	int64_t vx_bias_stride = 0;
};

// partial slabs of one weight-gradient launch: dW tiles and bias rows
struct Slabs { float* pw; float* pb; };
static Slabs slabs(const BwdWs& b, int k) { return Slabs{b.pw_t[k], b.pb_t[k]}; }

// (diagnosis) dynamic LDS of the slab reduce: 0, or everything the CU has left beside its 16 KB of static LDS
static int reduce_lds(find_ctx* c) {
	if (c->reduce_exclusive != 1) return 0;
	const int dyn = c->lds_bytes - 16 * 1024 - 256;
	if (!c->attr_done[K_REDUCE]) {
		if (hipFuncSetAttribute(reinterpret_cast<const void*>(&reduce_w_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, dyn) != hipSuccess) return 0;
		c->attr_done[K_REDUCE] = true;
	}
	return dyn;
}

static int launch_reduce(find_ctx* c, const ReduceWArgs& r, hipStream_t s) {
	const unsigned grid = (unsigned)(r.nwblk + (r.pb ? r.n_feet + 1 : 0));
	if (c->reduce_exclusive == 2) hipLaunchKernelGGL(reduce_w_nolds_kernel, dim3(grid), dim3(1024), 0, s, r);
	else hipLaunchKernelGGL(reduce_w_kernel, dim3(grid), dim3(1024), reduce_lds(c), s, r);
	FIND_LAUNCH_CHECK("reduce_w_kernel");
	return FIND_OK;
}

static int weight_grad(find_ctx* c, Fork* fk, const find_mlp_params* p, const Wgrad& in, Slabs sl) {
	const int64_t feet = in.feet, V = in.V;
	hipStream_t s = in.s;
	FIND_REQUIRE(!in.vx_bias || (!in.pos && ((in.h16 && c->f16) || (!c->f16 && c->x3 && cdiv(V, 32) * feet >= c->gemm6_min_units))),
				 "weight_grad: a virtual operand reached a kernel that cannot form it (bcast_fold and the kernel selection disagree)");
	float* pbuf = (in.db || in.S) ? sl.pb : nullptr;
	const int cus = c->num_cus;
	int nsplit, spf, Kp = 256;
	if (!in.pos) {
		auto dw3_args = [&](int cpf, int cps) {
			Dw3Args a;
			memset(&a, 0, sizeof(a));
			a.dz = in.dz; a.dz_foot_stride = V * W; a.x = in.x; a.x_foot_stride = in.x_foot_stride;
			a.V = (int)V; a.chunks_per_foot = cpf; a.spf = spf; a.cps = cps; a.pw = sl.pw; a.pb = pbuf;
			a.xbias = in.vx_bias; a.xbias_stride = in.vx_bias_stride;
			return a;
		};
		if (c->f16) {
			// opt-in fp16 mode: 64-row chunks, rows past the end of a foot zero-filled by the kernel
			const int cpf64 = (int)cdiv(V, 64);
			const int want = (int)std::max<int64_t>(1, std::min<int64_t>(cpf64, cdiv(cus, feet)));
			const int cps3 = (int)std::max<int64_t>(cdiv(cpf64, want), std::min<int>(4, cpf64));  // at least 256 rows per slab (the small launches are slab-bound)
			spf = (int)cdiv(cpf64, cps3);
			nsplit = (int)(feet * spf);
			int lds = 0;
			if (in.vx_bias) FIND_TRY(prepare_kernel(c, K_DW3_V, &dw3_h16v_kernel, DW3_LDS, &lds));
			else if (in.h16) FIND_TRY(prepare_kernel(c, K_DW3_H, &dw3_h16_kernel, DW3_LDS, &lds));
			else FIND_TRY(prepare_kernel(c, K_DW3, &dw3_kernel, DW3_LDS, &lds));
			const Dw3Args d3 = dw3_args(cpf64, cps3);
			if (in.vx_bias) hipLaunchKernelGGL(dw3_h16v_kernel, dim3((unsigned)nsplit), dim3(256), lds, s, d3);   // (x formed from the shared product: bcast_fold)
			else if (in.h16) hipLaunchKernelGGL(dw3_h16_kernel, dim3((unsigned)nsplit), dim3(256), lds, s, d3);   // (dz and x fp16-stored: act16)
			else hipLaunchKernelGGL(dw3_kernel, dim3((unsigned)nsplit), dim3(256), lds, s, d3);
			FIND_LAUNCH_CHECK("dw3_kernel");
		} else if (c->x3 && cdiv(V, 32) * feet >= c->gemm6_min_units) {
			// bf16x3: 16-row chunks, rows past the end of a foot zero-filled by the kernel; few, long runs (slab traffic)
			const int cpf16 = (int)cdiv(V, 16);
			// Workgroups = slabs: one per CU when the launch has the chip to itself; HALF that inside a backward with side streams -- there it
			// runs beside the dX GEMMs of the next layer, which take the other CUs anyway, and half the slabs are half the reduce's traffic
			// (64 -> 32 MB per layer: headline step 1.76 -> 1.71 ms on one box; 96 and 64 workgroups are slower again)
			const int wgs6 = (fk && fk->on) ? std::max(1, c->num_cus / 2) : c->num_cus;
			const int want = (int)std::max<int64_t>(1, std::min<int64_t>(cpf16, cdiv(wgs6, feet)));
			const int cps6 = (int)std::max<int64_t>(cdiv(cpf16, want), std::min<int>(c->dw2_min_cps, cpf16));
			spf = (int)cdiv(cpf16, cps6);
			nsplit = (int)(feet * spf);
			int lds = 0;
			if (in.vx_bias) FIND_TRY(prepare_kernel(c, K_DW6_V, &dw6v_kernel, DW6_LDS, &lds));
			else FIND_TRY(prepare_kernel(c, K_DW6, &dw6_kernel, DW6_LDS, &lds));
			const Dw3Args d6 = dw3_args(cpf16, cps6);
			if (in.vx_bias) hipLaunchKernelGGL(dw6v_kernel, dim3((unsigned)nsplit), dim3(256), lds, s, d6);   // (x formed from the shared product: bcast_fold)
			else hipLaunchKernelGGL(dw6_kernel, dim3((unsigned)nsplit), dim3(256), lds, s, d6);
			FIND_LAUNCH_CHECK("dw6_kernel");
		} else {
			// LDS-DMA kernel: every foot's rows cut into spf contiguous runs of 16-row chunks, the <= 15 leftover rows
			// folded into the foot's last run
			const int cpf16 = (int)(V / 16);
			int cps2 = 1;
			spf = 1;
			if (cpf16 > 0) {
				const int want = (int)std::max<int64_t>(1, std::min<int64_t>(cpf16, cdiv(cus, feet)));
				// few, long runs (slab traffic) -- unless that leaves CUs without a workgroup: a launch of few rows (the head's first-layer gradient
				// over the foot-summed dZ of a shared template: 6890 rows = 54 runs of 8 chunks, 86 us) is bounded by its longest run, not by slabs
				const int floor_cps = (feet * cpf16 < (int64_t)c->dw2_min_cps * cus) ? std::min(2, c->dw2_min_cps) : c->dw2_min_cps;
				cps2 = (int)std::max<int64_t>(cdiv(cpf16, want), std::min<int>(floor_cps, cpf16));
				spf = (int)cdiv(cpf16, cps2);
			}
			nsplit = (int)(feet * spf);
			int lds = 0;
			if (c->dw_lds_free == 0) FIND_TRY(prepare_kernel(c, K_DW2, &dw2_kernel, DW2_LDS, &lds));
			Dw2Args d2;
			memset(&d2, 0, sizeof(d2));
			d2.dz = in.dz; d2.dz_foot_stride = V * W; d2.x = in.x; d2.x_foot_stride = in.x_foot_stride;
			d2.chunks_per_foot = cpf16; d2.tail_rows = (int)(V % 16); d2.spf = spf; d2.cps = cps2; d2.pw = sl.pw; d2.pb = pbuf;
			if (c->dw_lds_free == 1) hipLaunchKernelGGL(dw4_kernel, dim3((unsigned)nsplit), dim3(512), 0, s, d2);
			else hipLaunchKernelGGL(dw2_kernel, dim3((unsigned)nsplit), dim3(256), lds, s, d2);
			FIND_LAUNCH_CHECK("dw2_kernel");
		}
	} else {
		// Fourier layer: the inputs are regenerated from the positions.  dwpe_kernel (mlp_dwpe.h; pe >= 32): one k-tile of workgroups per 128
		// frequencies, slabs of 2 pe + 32 columns; dw_kernel<AMODE_PE> (round 1, LDS-staged; pe < 32): nkt k-tiles, slabs of 256 nkt columns.
		// Either way the launch stays within one round of workgroups over the chip (at most 256).
		const bool lds_free = p->pe_size >= 32;
		const int nkt_launch = lds_free ? (int)cdiv(p->pe_size, 128) : in.nkt;
		int cps;
		split_policy(feet, V, &spf, &cps, std::min<int64_t>(128, std::max<int64_t>(16, std::min(256, cus) / nkt_launch)));
		DwArgs a;
		memset(&a, 0, sizeof(a));
		a.dz = in.dz; a.dz_foot_stride = V * W;
		a.x = in.x; a.x_foot_stride = in.x_foot_stride; a.ldx = W;
		a.pos = in.pos; a.pos_foot_stride = in.pos_foot_stride; a.Bm = p->B; a.pe = p->pe_size;
		a.V = (int)V; a.spf = spf; a.cps = cps; a.Kp = lds_free ? 2 * p->pe_size + 32 : in.nkt * 256;
		a.pw = sl.pw; a.pb = pbuf;
		a.all_blocks = (c->ablate & 32) ? 1 : 0;
		nsplit = (int)(feet * spf);
		Kp = a.Kp;
		if (lds_free && (c->x3 || c->f16)) {   // bf16x3 calls (and the opt-in fp16 mode, whose Fourier layer keeps fp32-class arithmetic): the sin / cos columns on the bf16 matrix pipe, the x, y, z columns and the bias sums beside them
			hipLaunchKernelGGL(dwpe6_kernel, dim3((unsigned)nkt_launch, (unsigned)nsplit), dim3(512), 0, s, a);
			hipLaunchKernelGGL(dwxyz_kernel, dim3((unsigned)nsplit), dim3(1024), 0, s, a);
		}
		else if (lds_free) hipLaunchKernelGGL(dwpe_kernel, dim3((unsigned)nkt_launch, (unsigned)nsplit), dim3(512), 0, s, a);
		else hipLaunchKernelGGL((dw_kernel<AMODE_PE>), dim3((unsigned)in.nkt, (unsigned)nsplit), dim3(512), 0, s, a);
		FIND_LAUNCH_CHECK("dw_kernel");
	}
	ReduceWArgs r;
	memset(&r, 0, sizeof(r));
	r.pw = sl.pw; r.nsplit = nsplit; r.Kp = Kp; r.out = in.dw; r.ld_out = in.ld_out; r.K_valid = in.k_valid;
	if (in.pos) { r.pe_map = in.pe_map; r.pe = p->pe_size; r.in_dim = p->in_dim; }
	r.pb = pbuf; r.n_feet = (int)feet; r.spf = spf; r.db = in.db; r.S = in.S;
	r.nwblk = 256 * Kp / 4 / 64;
	hipStream_t rs = s;
	if (fk && fk->on && in.reduce_side >= 0 && in.s_side >= 0 && in.reduce_side != in.s_side) {
		fk->chain(in.s_side, in.reduce_side);
		rs = fk->stream(in.reduce_side);
	}
	return launch_reduce(c, r, rs);
}

// Grouped weight gradients of a small call: every 256 x 256 layer's dW / db (and per-foot column sums) in ONE dw2 launch + ONE slab reduce.
struct WgradGroup {
	Dw2Group d;
	Dw6Group d6;        // the same jobs for dw6_group_kernel (bf16x3 calls)
	bool x3 = false;
	ReduceWGroup r;
	int n = 0, nmain = 0;
	int live_jobs = 0;   // jobs this launch will really carry (a call that skips a head has fewer than the workspace reserves): what the geometry is sized for
	int64_t feet = 0;
	WgradGroup() { memset(&d, 0, sizeof(d)); memset(&d6, 0, sizeof(d6)); memset(&r, 0, sizeof(r)); }
};

// Splits per foot of a grouped weight gradient.  A workgroup owns a whole 256 x 256 tile over `cps` 16-row chunks (3.4 us of MFMA issue
// each at the fp32 peak) and writes a 256-KB slab that the grouped reduce reads back; one workgroup per CU (whole-LDS reservation), so the
// launch runs in ceil(workgroups / CUs) rounds.  Few long splits leave CUs idle or pay a whole round for a few leftover workgroups; many
// short ones pay the per-workgroup prologue + slab and make the reduce (~0.06 us per slab) the longer kernel: take the cheapest of
// the candidates under this model.
static void group_geometry(const find_ctx* c, int cpf16, int64_t feet, int jobs, int64_t max_slabs, int* spf_out, int* cps_out) {
	auto take = [&](int s) { *cps_out = (int)cdiv(cpf16, s); *spf_out = (int)cdiv(cpf16, *cps_out); };
	const int s_max = (int)std::max<int64_t>(1, std::min<int64_t>(cpf16, max_slabs / std::max<int64_t>(feet, 1)));
	double best = 1e30;
	take(1);
	for (int s = 1; s <= s_max; ++s) {
		const int cps = (int)cdiv(cpf16, s);
		if ((int)cdiv(cpf16, cps) != s || (cps < 2 && s > 1)) continue;   // (same geometry as a smaller s; single-chunk splits)
		const int64_t wgs = feet * s * std::max(jobs, 1);
		const double cost = (double)cdiv(wgs, c->num_cus) * (cps * 3.6 + 6.0) + wgs * 0.06;
		if (cost < best) { best = cost; take(s); }
	}
}

static int wgrad_group_add(find_ctx* c, WgradGroup& G, const BwdWs& b, const Wgrad& in) {
	FIND_REQUIRE(G.n < b.grp_jobs && G.n < DW2_MAX_JOBS && G.n < DW6_MAX_JOBS, "find_mlp_bwd: too many grouped weight gradients");
	const int64_t feet = in.feet, V = in.V;
	// bf16x3 calls: dw6_group_kernel (16-row chunks, rows past a foot's end zero-filled by the loads: ceil); the others dw4_group (tail rows folded)
	G.x3 = c->x3 && c->dw_lds_free == 1;
	const int cpf16 = G.x3 ? (int)cdiv(V, 16) : (int)(V / 16);
	int spf = 1, cps2 = 1;
	if (cpf16 > 0) group_geometry(c, cpf16, feet, G.live_jobs > 0 ? G.live_jobs : b.grp_jobs, b.grp_slabs, &spf, &cps2);
	const int nmain = (int)(feet * spf);
	FIND_REQUIRE(nmain <= b.grp_slabs, "find_mlp_bwd: grouped weight gradient needs %d slabs, %lld reserved", nmain, (long long)b.grp_slabs);
	float* pw = b.grp_pw + (int64_t)G.n * b.grp_slabs * W * W;
	float* pb = b.grp_pw + (int64_t)b.grp_jobs * b.grp_slabs * W * W + (int64_t)G.n * b.grp_slabs * W;
	Dw2Args& d2 = G.d.job[G.n];
	d2.dz = in.dz; d2.dz_foot_stride = V * W; d2.x = in.x; d2.x_foot_stride = in.x_foot_stride;
	d2.chunks_per_foot = cpf16; d2.tail_rows = (int)(V % 16); d2.spf = spf; d2.cps = cps2; d2.pw = pw; d2.pb = (in.db || in.S) ? pb : nullptr;
	Dw3Args& d6 = G.d6.job[G.n];
	d6.dz = in.dz; d6.dz_foot_stride = V * W; d6.x = in.x; d6.x_foot_stride = in.x_foot_stride;
	d6.V = (int)V; d6.chunks_per_foot = cpf16; d6.spf = spf; d6.cps = cps2; d6.pw = pw; d6.pb = d2.pb;
	ReduceWArgs& r = G.r.job[G.n];
	r.pw = pw; r.nsplit = nmain; r.Kp = 256; r.out = in.dw; r.ld_out = in.ld_out; r.K_valid = W;
	r.pb = d2.pb; r.n_feet = (int)feet; r.spf = spf; r.db = in.db; r.S = in.S;
	r.nwblk = 256 * 256 / 4 / 64;
	G.nmain = nmain; G.feet = feet;   // (every job of a group has the same geometry)
	G.n += 1;
	return FIND_OK;
}

static int wgrad_group_launch(find_ctx* c, WgradGroup& G, hipStream_t s) {
	if (G.n == 0) return FIND_OK;
	if (G.x3) {
		int lds = 0;
		FIND_TRY(prepare_kernel(c, K_DW6G, &dw6_group_kernel, DW6_LDS, &lds));
		hipLaunchKernelGGL(dw6_group_kernel, dim3((unsigned)G.nmain, (unsigned)G.n), dim3(256), lds, s, G.d6);
	} else if (c->dw_lds_free == 1) {
		hipLaunchKernelGGL(dw4_group_kernel, dim3((unsigned)G.nmain, (unsigned)G.n), dim3(512), 0, s, G.d);
	} else {
		int lds = 0;
		FIND_TRY(prepare_kernel(c, K_DW2G, &dw2_group_kernel, DW2_LDS, &lds));
		hipLaunchKernelGGL(dw2_group_kernel, dim3((unsigned)G.nmain, (unsigned)G.n), dim3(256), lds, s, G.d);
	}
	FIND_LAUNCH_CHECK("grouped weight-gradient kernel");
	hipLaunchKernelGGL(reduce_w_group_kernel, dim3((unsigned)(256 * 256 / 4 / 64 + (int)G.feet + 1), (unsigned)G.n), dim3(1024), 0, s, G.r);
	FIND_LAUNCH_CHECK("reduce_w_group_kernel");
	return FIND_OK;
}

static int mlp_bwd_body(Fork& fk, const find_mlp_params* p, const Dims& d, const FwdWs& w, const BwdWs& b, const float* pos, Head* heads, const find_mlp_grads* g) {
	find_ctx* c = fk.c;
	hipStream_t s = fk.s;
	const bool defer = fk.deferring;
	const int64_t V = d.V, n_feet = d.n_feet;
	const int K0 = p->in_dim + 2 * p->pe_size;
	Head& hd = heads[0];
	Head& hc = heads[1];
	const bool act_d = hd.gout != nullptr, act_c = hc.gout != nullptr;
	// no weight-gradient buffer at all: the network is frozen (requires_grad False on every weight -- stage 3 of train.py refines the
	// latent codes only, train.py:217-224) and the call returns the latent gradients alone
	const bool frozen = g->trunk_w[0] == nullptr;
	// side streams of the fork: Q carries the large head layers' weight gradients, T1 / T2 the first head layers (foot-summed, with
	// their column-sum reduce and latent gradients) and the trunk layers, R the slab reduces of the large head layers
	enum { Q = 0, T1 = 1, T2 = 2, R = 3 };

	// gradients of skipped parts are exact zeros: one launch for all of them (they were up to nine memsets in front of the texture pass's
	// backward, ~5 us each on the step's critical path)
	ZeroArgs za;
	memset(&za, 0, sizeof(za));
	int mrc = FIND_OK;
	auto zero = [&](float* ptr, int64_t n) {
		if (!ptr || n <= 0) return;
		if (za.njobs == ZERO_MAX_JOBS) { hipLaunchKernelGGL(zero_many_kernel, dim3(32, za.njobs), dim3(256), 0, s, za); za.njobs = 0; }
		za.p[za.njobs] = ptr; za.n[za.njobs] = n; za.njobs += 1;
	};
	auto zero_flush = [&]() {
		if (za.njobs > 0) hipLaunchKernelGGL(zero_many_kernel, dim3(32, za.njobs), dim3(256), 0, s, za);
		za.njobs = 0;
		if (hipGetLastError() != hipSuccess) { set_error("find_mlp_bwd: zero_many_kernel launch failed"); mrc = FIND_ELAUNCH; }
	};
	for (int k = 0; k < 2; ++k) {
		const Head& h = heads[k];
		if (h.gout) continue;
		zero(h.gw[0], (int64_t)W * h.ld0); zero(h.gb[0], W);
		for (int i = 1; i < h.nl; ++i) { zero(h.gw[i], (int64_t)W * W); zero(h.gb[i], W); }
		zero(h.gw[h.nl], 3 * W); zero(h.gb[h.nl], 3);
		if (h.L) zero(h.glat, n_feet * h.L);
	}
	if (!act_d && !act_c) {
		zero(g->trunk_w[0], (int64_t)W * K0); zero(g->trunk_b[0], W);
		for (int i = 1; i < p->n_trunk; ++i) { zero(g->trunk_w[i], (int64_t)W * W); zero(g->trunk_b[i], W); }
		zero_flush();
		return mrc;
	}
	zero_flush();
	if (mrc != FIND_OK) return mrc;

	// 1. transposed weights for the dX GEMMs (a frozen network's backward stops at the heads' first layers: only their later layers) --
	// where the kernel that will run the layer cannot read the model's weight itself: bf16x3 chains (split_w_kernel, FusedStep::wmode 1) and
	// gemm7 (Gemm2Args::w_tr) can, so a bf16x3 training step transposes nothing (round 6: this launch was 10 - 12 us in front of each of the
	// step's two MLP backward passes)
	const bool fused = use_fused(c, V, d.feet_t) && p->pe_size > 0;
	const bool small_chain = fused && !d.shared;                 // the whole dX chain is one fused launch (also the frozen network's head chains)
	const bool t_heads = !(small_chain ? chain_direct(c) : gemm7_direct(c, V, n_feet));                 // layers >= 1 of the heads
	const bool t_trunk = !(fused ? chain_direct(c) : gemm7_direct(c, V, d.feet_t));                     // trunk layers >= 1
	const bool t_first = !(fused && chain_direct(c));                                                    // the heads' first layers (two-operand sum: gemm3 outside a chain)
	struct WT { const float* w; int ld; int tr; };
	auto wt_of = [&](bool need_t, const float* orig, int ld_orig, const float* transposed) -> WT { return need_t ? WT{transposed, W, 0} : WT{orig, ld_orig, 1}; };
	auto wt_H = [&](const Head& h, int l) -> WT { return l == 0 ? wt_of(t_first, h.w[0], h.ld0, h.wt[0]) : wt_of(t_heads, h.w[l], W, h.wt[l]); };
	auto wt_T = [&](int l) -> WT { return wt_of(t_trunk, p->trunk_w[l], W, b.Tt[l]); };
	{
		RepackArgs ra;
		memset(&ra, 0, sizeof(ra));
		int n = 0;
		if (!frozen) {
			if (t_trunk) for (int i = 1; i < p->n_trunk; ++i) ra.job[n++] = RepackJob{p->trunk_w[i], b.Tt[i], W, W, W, 0, W, 1, 0, 0};
			if (t_first) for (int k = 0; k < 2; ++k) ra.job[n++] = RepackJob{heads[k].w[0], heads[k].wt[0], W, W, heads[k].ld0, 0, W, 1, 0, 0};
		}
		if (t_heads)
			for (int k = 0; k < 2; ++k)
				for (int i = 1; i < heads[k].nl; ++i) ra.job[n++] = RepackJob{heads[k].w[i], heads[k].wt[i], W, W, W, 0, W, 1, 0, 0};
		ra.njobs = n;
		if (n > 0) hipLaunchKernelGGL(repack_kernel, dim3(64, n), dim3(256), 0, s, ra);
		FIND_LAUNCH_CHECK("repack_kernel(T)");
	}

	// 2. final layers: dz of the last hidden layer of each head + dW/db of the 3-wide layers
	const bool a16_rule = use_act16(c, c->f16, d.shared, n_feet, V);
	const int note16 = noted_act16(c, w.fbd, a16_rule, use_fold(c, a16_rule, d.shared, n_feet, V, p));
	const bool a16 = (note16 & 1) != 0;   // (the forward stored w.D / w.C as fp16: b.dzD / b.dzC follow)
	const bool fold = (note16 & 2) != 0;  // (... and did not store w.D[0] / w.C[0] at all: their readers form them from w.hp / w.hp2 and the bias rows)
	struct Virt { const float* P; const float* bias; int64_t bstride; };
	auto virt = [&](const Head& h, int l) -> Virt {   // the input of head layer l (l >= 1): virtual for l == 1 under bcast_fold
		if (!fold || l != 1) return Virt{nullptr, nullptr, 0};
		return Virt{h.hp, h.bias0, h.bstride0};
	};
	{
		HeadOutBwdArgs h;
		memset(&h, 0, sizeof(h));
		HeadOutReduceArgs hr;
		memset(&hr, 0, sizeof(hr));
		for (int k = 0; k < 2; ++k) {
			const Head& hk = heads[k];
			h.y[k] = hk.act[hk.nl - 1];
			h.w[k] = hk.w[hk.nl];
			h.z[k] = hk.z;
			h.gout[k] = hk.gout;
			h.dy[k] = hk.dz[hk.cur];
			h.pw[k] = b.pwo[k]; h.pb[k] = b.pbo[k];
			hr.pw[k] = b.pwo[k]; hr.pb[k] = b.pbo[k];
			hr.dw[k] = hk.gout ? hk.gw[hk.nl] : nullptr; hr.db[k] = hk.gb[hk.nl];
		}
		h.rows = d.rows_h;
		h.half = a16 ? 1 : 0;
		hipLaunchKernelGGL(head_out_bwd_kernel, dim3((unsigned)b.nblk_out, 2), dim3(256), 0, s, h);
		hr.nblk = b.nblk_out;
		// (the 3-wide layers' dW / db feed nothing of the dX chain: their reduce goes to a side stream like every other weight gradient --
		// it used to sit between head_out_bwd and the first dX GEMM of both backward passes of a step, 10 - 14 us each)
		if (!frozen) {
			fk.fork_to(T2);
			hipLaunchKernelGGL(head_out_reduce_kernel, dim3(12, 2), dim3(1024), 0, fk.stream(T2), hr);
		}
		FIND_LAUNCH_CHECK("head_out_bwd");
	}

	const float* hl = w.H[p->n_trunk - 1];
	const int64_t hl_stride = d.shared ? 0 : V * W;

	// ---- pieces of the dX chain and of the gradients around it, shared by the paths below
	// a head's hidden layers, last down to the second, as steps of a fused chain
	auto head_chain = [&](Chain& ch, Head& h) {
		for (int l = h.nl - 1; l >= 1; --l) {
			const WT t = wt_H(h, l);
			FusedStep& st = ch.gemm(t.w, t.ld, W / KC, h.cur == 0 ? h.dz[0] : nullptr);
			st.wmode = (unsigned char)t.tr;
			st.mask = 1; st.aux = h.act[l - 1]; st.dst = h.dz[h.cur + 1]; st.to_lds = 1;
			h.cur += 1;
		}
	};
	// gradient wrt the trunk output: both heads summed in one accumulator (the displacement head's operand first), then masked by the
	// trunk's last activation
	auto trunk_out_steps = [&](Chain& ch, const float* dz_d, const float* dz_c) {
		const float* A[2]; WT Wt[2]; int nb = 0;
		if (act_d) { A[nb] = dz_d; Wt[nb] = wt_H(hd, 0); ++nb; }
		if (act_c) { A[nb] = dz_c; Wt[nb] = wt_H(hc, 0); ++nb; }
		for (int i = 0; i < nb; ++i) {
			FusedStep& st = ch.gemm(Wt[i].w, Wt[i].ld, W / KC, A[i]);
			st.wmode = (unsigned char)Wt[i].tr;
			st.accum = i > 0;
			if (i + 1 < nb) { st.keep = 1; continue; }
			st.mask = 1; st.aux = hl; st.dst = b.dzT[0]; st.to_lds = 1;
		}
	};
	auto trunk_steps = [&](Chain& ch) {
		for (int l = p->n_trunk - 1; l >= 1; --l) {
			const WT t = wt_T(l);
			FusedStep& st = ch.gemm(t.w, t.ld, W / KC);
			st.wmode = (unsigned char)t.tr;
			st.mask = 1; st.aux = w.H[l - 1]; st.dst = b.dzT[p->n_trunk - l]; st.to_lds = 1;
		}
	};
	// masked dX:  y = (dz @ W) * (mask > 0), with W given pre-transposed or -- t.tr -- as the model holds it
	// (v.bias: bcast_fold -- mask is the shared fp32 product P and the layer's output was relu(P[v] + v.bias[foot]))
	auto dx_args = [&](const float* dz, const WT& t, const float* mask, float* y, const Virt& v) {
		Gemm2Args a = gemm_args();
		a.a0 = dz; a.a_foot_stride = V * W; a.lda = W;
		a.w0 = t.w; a.ldw = t.ld; a.w_tr = t.tr; a.nchunk = W / KC;
		a.mask = mask; a.mask_foot_stride = v.bias ? 0 : V * W;
		a.vm_bias = v.bias; a.vm_bias_stride = v.bstride;
		a.y = y; a.y_foot_stride = V * W; a.ldy = W; a.V = (int)V;
		return a;
	};
	// weight gradient of a 256-wide layer (the caller adds what its path needs: stream, sums, virtual operand)
	auto layer_wgrad = [&](const float* dz, const float* x, int64_t x_foot_stride, int64_t feet, float* dw, float* db) {
		Wgrad wg;
		wg.dz = dz; wg.x = x; wg.x_foot_stride = x_foot_stride; wg.feet = feet; wg.V = V; wg.dw = dw; wg.db = db;
		return wg;
	};
	// the Fourier layer's weight gradient, on side stream `side` out of slab set `set`
	auto fourier_wgrad = [&](const float* dz, int side, int set) -> int {
		Wgrad wg;
		wg.dz = dz; wg.pos = pos; wg.pos_foot_stride = V * 3; wg.nkt = d.nkt0; wg.feet = d.feet_t; wg.V = V;
		wg.dw = g->trunk_w[0]; wg.ld_out = K0; wg.k_valid = 0; wg.pe_map = 1; wg.db = g->trunk_b[0];
		wg.s = fk.stream(side);
		return weight_grad(c, &fk, p, wg, slabs(b, set));
	};
	// per-foot column sums of a head's first-layer dZ (and, zs given, its sum over the feet): partial sums on the caller's stream, then
	// their reduce (of nblk blocks) on the stream of whoever reads S
	auto foot_partials = [&](const Head& h, float* zs) {
		hipLaunchKernelGGL(footsum_kernel, dim3((unsigned)b.nblk_fs * 4), dim3(256), 0, s, h.dz[h.cur], (int)n_feet, (int)V, zs, h.pS, a16 ? 1 : 0);
	};
	auto foot_reduce = [&](const Head& h, int nblk, hipStream_t st) {
		hipLaunchKernelGGL(footsum_reduce_kernel, dim3((unsigned)n_feet, 4), dim3(1024), 0, st, h.pS, nblk, (int)n_feet, h.S);
	};
	// d loss / d latent[foot] = S[foot] . W0[:, 256:]; with gw0 also the latent columns of the first layer's dW, with db_late its bias gradient
	auto latent_grad = [&](const Head& h, float* gw0, float* db_late, hipStream_t st) {
		hipLaunchKernelGGL(latent_grad_kernel, dim3((unsigned)(n_feet + (gw0 ? W : 0) + (db_late ? 1 : 0))), dim3(256), 0, st, h.w[0], h.ld0, h.lat, h.L, h.S, (int)n_feet,
						   h.glat, gw0, db_late);
	};

	// The trunk's dX chain of a call whose heads are large (the shared template of a batch: launched far below, behind the heads' GEMMs) is
	// put together HERE, so that its weights are split (chain_prepare) before the large kernels fill the chip.
	Chain tch;
	if (fused && !frozen && d.shared) {
		trunk_out_steps(tch, hd.zs, hc.zs);   // (the heads' foot-summed first-layer dZ)
		trunk_steps(tch);
		FIND_TRY(chain_prepare(c, tch, V, d.feet_t, s, b.w6, chain_w6_bytes(p)));
	}
	if (frozen) {
		// ---- latents only.  d loss / d latent[foot] = (sum_v dZ0[foot, v]) . W0[:, 256:]: the heads' dX chains down to their first layers,
		// per-foot column sums, one small product per head.  Nothing reaches the trunk, no weight gradient is formed: at the reference's
		// batch size this backward is 4 of the 9 layer-steps of the full chain and none of its thirteen weight-gradient jobs.
		auto want = [&](const Head& h) { return h.gout && h.L > 0 && h.glat != nullptr; };
		if (!want(hd) && !want(hc)) return FIND_OK;
		if (small_chain) {
			Chain ch;
			if (want(hc)) head_chain(ch, hc);
			if (want(hd)) head_chain(ch, hd);
			if (ch.a.n_steps > 0) FIND_TRY(launch_chain(c, ch, V, d.feet_t, s, b.w6, chain_w6_bytes(p)));
		} else {
			for (int k = 0; k < 2; ++k) {
				Head& h = heads[k];
				if (!want(h)) continue;
				for (int l = h.nl - 1; l >= 1; --l) {
					const Virt v = virt(h, l);
					FIND_TRY(launch_gemm(c, AMODE_MAT, EPI_MASK, dx_args(h.dz[h.cur], wt_H(h, l), v.P ? v.P : h.act[l - 1], h.dz[h.cur + 1], v), n_feet, s, a16));
					h.cur += 1;
				}
			}
		}
		for (int k = 0; k < 2; ++k) {
			const Head& h = heads[k];
			if (!want(h)) continue;
			foot_partials(h, nullptr);
			foot_reduce(h, b.nblk_fs, s);
			latent_grad(h, nullptr, nullptr, s);
			FIND_LAUNCH_CHECK("latent gradients of a frozen network");
		}
		return FIND_OK;
	}
	if (small_chain) {
		// ---- small call (every layer has few rows: the reference's batch 1, the texture samples): the whole dX chain of both heads and
		// the trunk is ONE fused launch (mlp_fused.h); every layer's dZ lands in its own buffer, and the weight gradients follow on the
		// side streams (round-robin, one slab set per stream)
		Chain ch;
		if (act_c) head_chain(ch, hc);   // (the colour head's layers first)
		if (act_d) head_chain(ch, hd);
		trunk_out_steps(ch, hd.dz[hd.cur], hc.dz[hc.cur]);
		trunk_steps(ch);
		FIND_TRY(launch_chain(c, ch, V, d.feet_t, s, b.w6, chain_w6_bytes(p)));
		// weight gradients: all inputs exist now.  fp32: every 256 x 256 layer in ONE grouped launch (+ one grouped slab reduce) on a side
		// stream, the Fourier layer on another; the opt-in fp16 mode keeps its per-layer dw3 launches.
		const bool grouped = !c->f16 && b.grp_pw != nullptr;
		WgradGroup G;
		G.live_jobs = (act_d ? p->n_disp : 0) + (act_c ? p->n_col : 0) + (p->n_trunk - 1);
		int rr = 0;
		auto one = [&](Wgrad wg) -> int {
			if (grouped) return wgrad_group_add(c, G, b, wg);
			const int k = fk.on ? 1 + rr % 2 : 0;
			rr += 1;
			fk.fork_to(k);
			wg.s = fk.stream(k);
			return weight_grad(c, &fk, p, wg, slabs(b, k));
		};
		const Head* lats[2]; int nlat = 0;
		auto head_wgrads = [&](const Head& h) -> int {
			for (int l = h.nl - 1; l >= 1; --l) FIND_TRY(one(layer_wgrad(h.dz[h.nl - 1 - l], h.act[l - 1], V * W, n_feet, h.gw[l], h.gb[l])));
			if (defer && h.L > 0) {
				// the weight gradients stay behind on the side streams: the latent gradients -- an OUTPUT autograd hands to whatever comes
				// next -- are formed on the caller's stream, from per-foot column sums of their own (no slab reduce to wait for)
				foot_partials(h, nullptr);
				foot_reduce(h, b.nblk_fs, s);
				latent_grad(h, h.gw[0], nullptr, s);
				FIND_LAUNCH_CHECK("latent gradients (deferred join)");
			}
			Wgrad wg = layer_wgrad(h.dz[h.cur], hl, hl_stride, n_feet, h.gw[0], h.gb[0]);
			wg.ld_out = h.ld0;
			wg.S = (h.L > 0 && !defer) ? h.S : nullptr;
			FIND_TRY(one(wg));
			if (h.L > 0 && !defer) lats[nlat++] = &h;
			return FIND_OK;
		};
		if (act_d) FIND_TRY(head_wgrads(hd));
		if (act_c) FIND_TRY(head_wgrads(hc));
		for (int l = p->n_trunk - 1; l >= 1; --l)
			FIND_TRY(one(layer_wgrad(b.dzT[p->n_trunk - 1 - l], w.H[l - 1], V * W, d.feet_t, g->trunk_w[l], g->trunk_b[l])));
		// the latent gradients read the per-foot column sums S (written by the slab reduce): same stream, behind it
		hipStream_t sl = s;
		if (grouped) {
			fk.fork_to(1);
			sl = fk.stream(1);
			FIND_TRY(wgrad_group_launch(c, G, sl));
		} else if (fk.on) {
			// (per-layer launches went to streams 1 / 2 round-robin: wait for both before the latent gradients on stream 1)
			fk.chain(2, 1);
			sl = fk.stream(1);
		}
		for (int i = 0; i < nlat; ++i) {
			latent_grad(*lats[i], lats[i]->gw[0], nullptr, sl);
			FIND_LAUNCH_CHECK("latent_grad_kernel");
		}
		{
			const int k = fk.on ? 2 : 0;
			fk.fork_to(k);
			FIND_TRY(fourier_wgrad(b.dzT[p->n_trunk - 1], k, 0));
		}
		FIND_LAUNCH_CHECK("find_mlp_bwd");
		return FIND_OK;
	}

	// 3. heads, last hidden layer down to the first.  Weight-gradient work (dW / db / latent gradients only feed the outputs, never
	// the dX chain) goes to the side streams; every layer's dZ has its own buffer, so the dX chain on the caller's stream never waits.
	int big_toggle = 0;
	hipEvent_t set_free[2] = {nullptr, nullptr};   // fires when the slab set's previous reduce (on R) has read it
	// The V-row weight gradients of a shared template's backward -- the trunk's layers and (round 6) the heads' first layers over the
	// foot-summed dZ, which used to be a 50-70-us fp32-MFMA launch of its own per head -- travel in ONE grouped launch behind the trunk's dX chain.
	WgradGroup G;
	const bool grouped_v = fused && d.shared && !c->f16 && b.grp_pw != nullptr;
	G.live_jobs = (p->n_trunk - 1) + (act_d ? 1 : 0) + (act_c ? 1 : 0);
	auto head_bwd = [&](Head& h) -> int {
		int fsum_pairs = 0;
		for (int l = h.nl - 1; l >= 1; --l) {
			const Virt v = virt(h, l);
			const float* const xin = v.P ? v.P : h.act[l - 1];
			fk.fork_to(Q);
			Wgrad wg = layer_wgrad(h.dz[h.cur], xin, v.P ? 0 : V * W, n_feet, h.gw[l], h.gb[l]);
			wg.s = fk.stream(Q); wg.h16 = a16; wg.vx_bias = v.bias; wg.vx_bias_stride = v.bstride;
			// the large layers alternate between two slab sets and hand their slab reduce to stream R: the reduce (LDS-using, so
			// it only gets a CU when a ring kernel's workgroup retires) no longer sits between two dw2 launches on Q
			// (Not under stream capture: there the streams only express dependencies and the graph executor schedules the branches;
			// hipStreamEndCapture of ROCm 7.0 / 7.2 faults on this R <-> Q event pattern, and captures cleanly without it.)
			if (fk.on && c->reduce_stream && !fk.capturing) {
				const int si = big_toggle & 1;
				big_toggle += 1;
				fk.wait(Q, set_free[si]);
				wg.s_side = Q; wg.reduce_side = R;
				FIND_TRY(weight_grad(c, &fk, p, wg, slabs(b, si ? 3 : 0)));
				set_free[si] = fk.mark(R);
			} else {
				FIND_TRY(weight_grad(c, &fk, p, wg, slabs(b, 0)));
			}
			// footsum_fold: this dX GEMM's output is the broadcast layer's dZ, of which only sums are read (below): formed inside the GEMM
			fsum_pairs = (l == 1 && v.P && !a16 && c->footsum_fold && h.zs != nullptr && gemm7_direct(c, V, n_feet)) ? gemm7_fsum_pairs(c, V, n_feet) : 0;
			Gemm2Args a = dx_args(h.dz[h.cur], wt_H(h, l), xin, h.dz[h.cur + 1], v);
			if (fsum_pairs > 0) { a.fs_out = h.zs; a.fs_slot_stride = h.fs1 - h.zs; a.cs_out = h.pS; }   // (y is then not written)
			FIND_TRY(launch_gemm(c, AMODE_MAT, EPI_MASK, a, n_feet, s, a16));
			h.cur += 1;
		}
		float* db_late = nullptr;
		hipStream_t q0;
		if (d.shared) {
			// every foot multiplies the same trunk rows: reduce dZ0 over feet first (one pass), then M = V GEMMs
			// (Measured and dropped: the foot sum on the head's side stream, the caller's stream going straight on to the other head's dX
			// chain and waiting for the sums in step 4 -- 3.49 against 3.38 ms per train_3d step: the HBM-bound pass beside the dX GEMMs
			// costs them more than the wait it removes.)
			// the foot-summed first layer is a small launch: its own side stream and slab set, so that it does not queue behind the
			// large weight-gradient launches on Q.  The per-foot column sums go there too: only the latent / bias gradients read them.
			if (fsum_pairs > 0) {
				// (footsum_fold: the two partial foot sums -> the foot sum; the per-foot column sums wait in pS, one block per workgroup pair of the GEMM)
				const int64_t n4 = V * W / 4;
				hipLaunchKernelGGL(add_inplace_kernel, dim3((unsigned)cdiv(n4, 256)), dim3(256), 0, s, h.zs, h.fs1, n4);
			} else {
				foot_partials(h, h.zs);
			}
			fk.fork_to(h.side);
			q0 = fk.stream(h.side);
			foot_reduce(h, fsum_pairs > 0 ? fsum_pairs : b.nblk_fs, q0);
			// (the bias gradient -- S summed over feet -- rides along with the latent-gradient launch when there is one)
			if (h.L > 0) db_late = h.gb[0];
			else hipLaunchKernelGGL(colsum_small_kernel, dim3(1), dim3(256), 0, q0, h.S, (int)n_feet, h.gb[0]);
			FIND_LAUNCH_CHECK("footsum");
			Wgrad wg = layer_wgrad(h.zs, hl, 0, 1, h.gw[0], nullptr);
			wg.ld_out = h.ld0;
			wg.s = q0;
			if (grouped_v) FIND_TRY(wgrad_group_add(c, G, b, wg));
			else FIND_TRY(weight_grad(c, &fk, p, wg, slabs(b, h.side)));
		} else {
			fk.fork_to(Q);
			q0 = fk.stream(Q);
			fk.wait(Q, set_free[0]);   // set 0 may still be read by a reduce on R
			Wgrad wg = layer_wgrad(h.dz[h.cur], hl, hl_stride, n_feet, h.gw[0], h.gb[0]);
			wg.ld_out = h.ld0;
			wg.S = (h.L > 0) ? h.S : nullptr;
			wg.s = q0;
			FIND_TRY(weight_grad(c, &fk, p, wg, slabs(b, 0)));
		}
		if (h.L > 0) {
			latent_grad(h, h.gw[0], db_late, q0);
			FIND_LAUNCH_CHECK("latent_grad_kernel");
		}
		return FIND_OK;
	};
	if (act_d) FIND_TRY(head_bwd(hd));
	if (act_c) FIND_TRY(head_bwd(hc));

	// 4 + 5.  gradient wrt the trunk output -- both heads (and, for a shared trunk, every foot) summed in the K loop -- and the trunk's
	// dX chain.  With few trunk rows (the shared template) all of it is one fused launch; the weight gradients follow on T1 / T2.
	// a trunk layer's weight gradient: into the grouped launch, or -- independent of each other, each filling a fraction of the chip --
	// alternating between T1 and T2 (own slab set each)
	auto trunk_wgrad = [&](int l, const float* dz) -> int {
		Wgrad wg = layer_wgrad(dz, w.H[l - 1], V * W, d.feet_t, g->trunk_w[l], g->trunk_b[l]);
		if (grouped_v) return wgrad_group_add(c, G, b, wg);
		const int k = fk.on ? 1 + (l & 1) : 0;
		fk.fork_to(k);
		wg.s = fk.stream(k);
		return weight_grad(c, &fk, p, wg, slabs(b, k));
	};
	int ct = 0;
	if (fused) {
		// (the chain was built, and its weights split, right behind the transposes: see there)
		FIND_TRY(launch_chain(c, tch, V, d.feet_t, s, b.w6, chain_w6_bytes(p)));
		// the trunk's weight gradients: all their inputs exist now -- one grouped launch + one grouped reduce (fp32), as in the small-call path
		for (int l = p->n_trunk - 1; l >= 1; --l, ++ct) FIND_TRY(trunk_wgrad(l, b.dzT[ct]));
		if (grouped_v) {
			fk.fork_to(T1);
			FIND_TRY(wgrad_group_launch(c, G, fk.stream(T1)));
		}
	} else {
		// 4. gradient wrt the trunk output: both heads (and, for a shared trunk, every foot) summed in the K loop
		{
			Gemm2Args a = gemm_args();
			const float* A[2]; const float* Wt[2]; int nb = 0;
			if (act_d) { A[nb] = d.shared ? hd.zs : hd.dz[hd.cur]; Wt[nb] = hd.wt[0]; ++nb; }
			if (act_c) { A[nb] = d.shared ? hc.zs : hc.dz[hc.cur]; Wt[nb] = hc.wt[0]; ++nb; }
			a.nseg = nb; a.a0 = A[0]; a.w0 = Wt[0];
			if (nb > 1) { a.a1 = A[1]; a.w1 = Wt[1]; }
			a.lda = W; a.ldw = W; a.nchunk = W / KC;
			a.a_foot_stride = d.shared ? 0 : V * W;  // shared: the foot-summed (V,256) matrices
			a.mask = hl; a.mask_foot_stride = V * W;
			a.y = b.dzT[ct]; a.y_foot_stride = V * W; a.ldy = W; a.V = (int)V;
			FIND_TRY(launch_gemm(c, AMODE_MAT, EPI_MASK, a, d.feet_t, s));
			FIND_LAUNCH_CHECK("trunk-out dX gemm");
		}
		// 5. trunk: the dX chain runs back to back on the caller's stream, the layers' weight gradients beside it; Q / set 0 keeps the Fourier layer
		for (int l = p->n_trunk - 1; l >= 1; --l, ++ct) {
			FIND_TRY(trunk_wgrad(l, b.dzT[ct]));
			FIND_TRY(launch_gemm(c, AMODE_MAT, EPI_MASK, dx_args(b.dzT[ct], wt_T(l), w.H[l - 1], b.dzT[ct + 1], Virt{nullptr, nullptr, 0}), d.feet_t, s));
		}
	}
	if (fused && d.shared && fk.on) {
		// (round 6: on Q the Fourier layer's weight gradient queued behind the last large layer's dw6 AND its slab reduce -- 60 us after the
		// trunk's dX chain had produced its input, at the very end of the step; T2 is idle by then, and its slab set is the Fourier layer's size)
		fk.fork_to(T2);
		FIND_TRY(fourier_wgrad(b.dzT[ct], T2, T2));
	} else {
		fk.fork_to(Q);
		fk.wait(Q, set_free[0]);
		FIND_TRY(fourier_wgrad(b.dzT[ct], Q, 0));
	}
	FIND_LAUNCH_CHECK("find_mlp_bwd");
	return FIND_OK;
}

}  // namespace mlp
}  // namespace find

// ------------------------------------------------------------------------------------------- entry points
extern "C" int64_t find_mlp_ws_bytes(const find_mlp_params* p, int64_t pos_batch, int64_t n_feet, int64_t n_pts, int save_for_bwd) {
	Dims d;
	if (make_dims(p, pos_batch, n_feet, n_pts, &d) != FIND_OK) return -1;
	FwdWs w;
	carve_fwd(p, d, save_for_bwd != 0, nullptr, &w);
	return w.bytes;
}

extern "C" int find_mlp_fwd(find_ctx* c, const find_mlp_params* p, const float* pos, int64_t pos_batch, int64_t n_feet, int64_t n_pts,
							const float* lat_disp, const float* lat_col, float* disp, float* col, void* ws,
							int64_t ws_bytes, int save_for_bwd, void* stream) {
	FIND_TRY(check_ctx(c, "find_mlp_fwd"));
	Dims d;
	FIND_TRY(make_dims(p, pos_batch, n_feet, n_pts, &d));
	FIND_TRY(check_weights(p));
	FIND_REQUIRE(pos && ws, "find_mlp_fwd: pos/ws is NULL");
	FIND_REQUIRE(disp || col, "find_mlp_fwd: both outputs NULL");
	// (the latents of a head the call does not evaluate may be NULL: nothing reads them)
	FIND_REQUIRE(p->lat_disp == 0 ? lat_disp == nullptr : (lat_disp != nullptr || disp == nullptr), "find_mlp_fwd: lat_disp pointer does not match params.lat_disp=%d", p->lat_disp);
	FIND_REQUIRE(p->lat_col == 0 ? lat_col == nullptr : (lat_col != nullptr || col == nullptr), "find_mlp_fwd: lat_col pointer does not match params.lat_col=%d", p->lat_col);
	FIND_REQUIRE(p->precision >= 0 && p->precision <= 3, "find_mlp_fwd: params.precision must be 0 (context default), 1 (fp32 MFMA), 2 (fp16) or 3 (bf16x3), got %d", p->precision);
	FwdWs w;
	carve_fwd(p, d, save_for_bwd != 0, ws, &w);
	if (ws_bytes < w.bytes) {
		set_error("find_mlp_fwd: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)w.bytes);
		return FIND_EWORKSPACE;
	}
	c->f16 = call_f16(c, p);
	c->x3 = call_x3(c, p);
	Fork fk(c, reinterpret_cast<hipStream_t>(stream), c->fwd_streams != 0);
	Head heads[2];
	make_heads(heads, p, w, lat_disp, lat_col, nullptr, nullptr);
	heads[0].out = disp; heads[1].out = col;
	const int rc = mlp_fwd_body(fk, p, d, w, pos, heads);
	const int rj = fk.join();   // on every path: the caller may free `ws` right after an error return
	return rc != FIND_OK ? rc : rj;
}

extern "C" int find_linear_relu_fwd(find_ctx* c, const float* x, const float* w, const float* b, int64_t n_feet, int64_t n_pts, float* y, void* stream) {
	FIND_TRY(check_ctx(c, "find_linear_relu_fwd"));
	FIND_REQUIRE(x && w && b && y, "find_linear_relu_fwd: NULL argument");
	FIND_REQUIRE(n_feet >= 1 && n_pts >= 1 && n_feet < (1 << 16), "find_linear_relu_fwd: bad sizes");
	FIND_REQUIRE(aligned16(w) && aligned16(x), "find_linear_relu_fwd: x and w must be 16-byte aligned");
	c->f16 = c->mlp_f16 == 1;
	c->x3 = c->mlp_f16 == 2;
	FIND_TRY(launch_gemm(c, AMODE_MAT, EPI_BIAS_RELU, linear_args(x, n_pts * W, w, W, b, 0, y, n_pts), n_feet, reinterpret_cast<hipStream_t>(stream)));
	FIND_LAUNCH_CHECK("find_linear_relu_fwd");
	return FIND_OK;
}

// Slabs of one weight-gradient launch: up to max(512, feet) + feet + 16 partial 256x256 tiles and as many 256-float bias rows.
static int64_t wgrad_slabs(int64_t n_feet) { return std::max<int64_t>(512, n_feet) + n_feet + 16; }

extern "C" int64_t find_linear_wgrad_scratch_bytes(int64_t n_feet) {
	if (n_feet < 1) return -1;
	return wgrad_slabs(n_feet) * ((int64_t)W * W + W) * (int64_t)sizeof(float);
}

extern "C" int find_linear_wgrad(find_ctx* c, const float* dz, const float* x, int64_t n_feet, int64_t n_pts, float* dw, float* db,
								 void* scratch, int64_t scratch_bytes, void* stream) {
	FIND_TRY(check_ctx(c, "find_linear_wgrad"));
	FIND_REQUIRE(dz && x && dw && scratch, "find_linear_wgrad: NULL argument");
	FIND_REQUIRE(n_feet >= 1 && n_pts >= 1 && n_feet < (1 << 16), "find_linear_wgrad: bad sizes");
	FIND_REQUIRE(aligned16(dz) && aligned16(x) && aligned16(scratch), "find_linear_wgrad: dz, x and scratch must be 16-byte aligned");
	if (scratch_bytes < find_linear_wgrad_scratch_bytes(n_feet)) {
		set_error("find_linear_wgrad: scratch too small (%lld < %lld)", (long long)scratch_bytes, (long long)find_linear_wgrad_scratch_bytes(n_feet));
		return FIND_EWORKSPACE;
	}
	float* const pw = static_cast<float*>(scratch);
	Wgrad wg;
	wg.dz = dz; wg.x = x; wg.x_foot_stride = n_pts * W; wg.feet = n_feet; wg.V = n_pts; wg.dw = dw; wg.db = db;
	wg.s = reinterpret_cast<hipStream_t>(stream);
	c->f16 = c->mlp_f16 == 1;
	c->x3 = c->mlp_f16 == 2;
	FIND_TRY(weight_grad(c, nullptr, nullptr, wg, Slabs{pw, pw + wgrad_slabs(n_feet) * W * W}));
	FIND_LAUNCH_CHECK("find_linear_wgrad");
	return FIND_OK;
}

extern "C" int64_t find_mlp_bwd_scratch_bytes(const find_mlp_params* p, int64_t pos_batch, int64_t n_feet, int64_t n_pts) {
	Dims d;
	if (make_dims(p, pos_batch, n_feet, n_pts, &d) != FIND_OK) return -1;
	BwdWs b;
	carve_bwd(p, d, nullptr, &b);
	return b.bytes;
}

extern "C" int find_mlp_bwd(find_ctx* c, const find_mlp_params* p, const float* pos, int64_t pos_batch, int64_t n_feet, int64_t n_pts,
							const float* lat_disp, const float* lat_col, const float* d_disp, const float* d_col,
							const void* ws, int64_t ws_bytes, void* scratch, int64_t scratch_bytes,
							const find_mlp_grads* g, void* stream) {
	FIND_TRY(check_ctx(c, "find_mlp_bwd"));
	Dims d;
	FIND_TRY(make_dims(p, pos_batch, n_feet, n_pts, &d));
	FIND_TRY(check_weights(p));
	FIND_REQUIRE(pos && ws && scratch && g, "find_mlp_bwd: NULL argument");
	FIND_REQUIRE(p->lat_disp == 0 ? lat_disp == nullptr : (lat_disp != nullptr || d_disp == nullptr), "find_mlp_bwd: lat_disp pointer does not match params");
	FIND_REQUIRE(p->lat_col == 0 ? lat_col == nullptr : (lat_col != nullptr || d_col == nullptr), "find_mlp_bwd: lat_col pointer does not match params");
	FIND_REQUIRE(p->precision >= 0 && p->precision <= 3, "find_mlp_bwd: params.precision must be 0, 1, 2 or 3 (got %d)", p->precision);
	{
		// weight-gradient buffers: all of them (a head without an upstream gradient may leave its own out: nothing is written for it), or
		// none at all (frozen network: latent gradients only)
		const bool frozen = g->trunk_w[0] == nullptr;
		bool ok = true;
		for (int i = 0; i < p->n_trunk; ++i) ok = ok && ((g->trunk_w[i] == nullptr) == frozen) && ((g->trunk_b[i] == nullptr) == frozen);
		for (int i = 0; i <= p->n_disp; ++i) ok = ok && (frozen ? !g->disp_w[i] && !g->disp_b[i] : (d_disp == nullptr || (g->disp_w[i] && g->disp_b[i])));
		for (int i = 0; i <= p->n_col; ++i) ok = ok && (frozen ? !g->col_w[i] && !g->col_b[i] : (d_col == nullptr || (g->col_w[i] && g->col_b[i])));
		FIND_REQUIRE(ok, "find_mlp_bwd: grads must name every weight-gradient buffer of the evaluated heads and the trunk, or none at all (frozen network)");
	}
	FwdWs w;
	carve_fwd(p, d, true, const_cast<void*>(ws), &w);
	if (ws_bytes < w.bytes) {
		set_error("find_mlp_bwd: forward workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)w.bytes);
		return FIND_EWORKSPACE;
	}
	BwdWs b;
	carve_bwd(p, d, scratch, &b);
	if (scratch_bytes < b.bytes) {
		set_error("find_mlp_bwd: scratch too small (%lld < %lld)", (long long)scratch_bytes, (long long)b.bytes);
		return FIND_EWORKSPACE;
	}
	c->f16 = call_f16(c, p);
	c->x3 = call_x3(c, p);
	Fork fk(c, reinterpret_cast<hipStream_t>(stream), c->bwd_streams != 0);
	// "defer_join" (one call: the knob is taken down here): the weight gradients of a small per-foot call -- the texture pass of a
	// train_3d step, 0.28 ms of grouped and Fourier-layer weight gradients that nothing reads until the main pass adds its own -- keep
	// running on the side streams while the caller's stream goes on; find_ctx_join (or the join of the next call) waits for them.
	// The caller keeps scratch, workspace and gradient buffers alive until then.  Not under stream capture, not for the large-call paths.
	const bool defer = c->defer_join != 0 && fk.on && !fk.capturing && !d.shared && use_fused(c, d.V, d.feet_t) && p->pe_size > 0 && g->trunk_w[0] != nullptr;
	c->defer_join = 0;
	fk.deferring = defer;
	Head heads[2];
	make_heads(heads, p, w, lat_disp, lat_col, &b, g);
	heads[0].gout = d_disp; heads[1].gout = d_col;
	const int rc = mlp_bwd_body(fk, p, d, w, b, pos, heads, g);
	// join on EVERY path: the caller's stream continues only after every side stream this call touched has finished, so scratch,
	// workspace and gradient buffers may be freed (stream-ordered) as soon as the call returns -- also after an error
	const int rj = (defer && rc == FIND_OK) ? fk.defer() : fk.join();
	return rc != FIND_OK ? rc : rj;
}

extern "C" int find_render_switches(int64_t bits) {
	FIND_REQUIRE(bits >= 0 && (bits & ~(int64_t)find::RASTER_SWITCHES) == 0, "find_render_switches: bits 0x%llx outside the result-preserving switches 0x%x", (unsigned long long)bits, find::RASTER_SWITCHES);
	find::g_raster_ablate = (int)bits;
	return FIND_OK;
}
