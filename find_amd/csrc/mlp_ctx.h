// Per-device state of the MLP entry points and what one call needs of it: the context (find_hip.h: find_ctx_create), kernel LDS
// attributes, fork / join onto the side streams, the hardware-queue probe.  Part of mlp.hip's translation unit.
#pragma once
#include "mlp_kernels.h"

// Per-device state of the MLP entry points (find_hip.h: find_ctx_create).  Nothing below is process-global.
enum { K_GEMM2_PE = 0, K_GEMM3_RELU, K_GEMM3_MASK, K_GEMM3_NONE, K_GEMM4_4_RELU, K_GEMM4_4_MASK, K_GEMM4_4_NONE, K_GEMM4_2_RELU, K_GEMM4_2_MASK,
	   K_GEMM4_2_NONE, K_GEMM5_RELU, K_GEMM5_MASK, K_GEMM5_NONE, K_GEMM7_RELU, K_GEMM7_MASK, K_GEMM7_NONE, K_DW2, K_DW3, K_DW6, K_DW6G, K_FUSED, K_FUSED2, K_FUSED6, K_FUSED6_2, K_DW2G, K_REDUCE, K_GEMM5_RELU_H, K_GEMM5_MASK_H, K_DW3_H, K_GEMM5_RELU_V, K_GEMM5_MASK_V, K_DW3_V, K_GEMM7_RELU_V, K_GEMM7_MASK_V, K_DW6_V, K_GEMM7_MASK_VF, K_COUNT };
constexpr int N_SIDE = 4;       // internal streams: 0 = q (large head layers' dW), 1 / 2 = first head layers + trunk layers, 3 = slab reduces
constexpr int N_EVENTS = 512;   // event ring: an MLP call with 3 x 8 layers uses ~170; checked per call

struct find_ctx {
	int device = 0;
	int num_cus = 256;
	int lds_bytes = 160 * 1024;   // largest dynamic LDS one workgroup may ask for on this device
	// knobs (find_hip.h: find_ctx_set)
	int ablate = 0;               // result-preserving switches (MLP_SWITCHES, common.h)
	int64_t gemm4_min_units = 1024;
	int gemm4_small = 64;         // column-quarter gemm4 for launches of at least this many 32-row units (0: never)
	int gemm5_min_units = 1024;
	int gemm6_min_units = 1024;
	int mlp_f16 = 0;              // default precision of calls that do not name one
	int fused_max_units = 512;    // chains of layers over at most this many 32-row tiles run as ONE fused_chain_kernel launch (0: never)
	int fused6 = 1;               // bf16x3 calls run their chains on fused6_kernel (0: the fp32-MFMA chain, as the other precisions)
	int dw2_min_cps = 8;          // at least this many 16-row chunks per dw2 workgroup (4: 2.257, 8: 2.243, 12: 2.266 ms/step at C2)
	int dw_lds_free = 1;          // 256 x 256 weight gradients: 1 = dw4_kernel (no LDS, <= 256 registers), 0 = dw2_kernel (LDS-DMA ring, whole register file claimed)
	int lds_exclusive = 0;        // 1 = the LDS-DMA ring kernels reserve the whole LDS of their CU: round 1's containment of the co-residence fault, which
	                              // round 2 showed to be about registers, not LDS (see "Co-residence" below); off by default now
	int reduce_exclusive = 0;     // diagnosis only: 1 = the slab reduce (16 KB of LDS) reserves its CU's whole LDS; 2 = LDS-free, slow reduce: the stress
	                              // configuration for the co-residence fault (long-lived foreign waves beside the weight-gradient kernels)
	int bwd_streams = 1;          // weight gradients on the side streams
	int fwd_streams = 1;          // colour head on a side stream beside the displacement head
	int reduce_stream = 0;        // 1 = slab reduces of the large head layers on their own stream R (two alternating slab sets): what the LDS-ring weight
	                              // gradient needed (its reduce only got a CU when a ring workgroup retired); with dw4_kernel the reduce behind its
	                              // launch on Q is 0.6 - 0.9 % faster (train_3d 3.245 -> 3.225 ms, C2 2.220 -> 2.199), so off by default
	int bind_streams = 1;         // 0 = keep the side streams as created
	int defer_join = 0;           // read by the next find_mlp_bwd: leave the weight-gradient side streams running behind the call (find_hip.h)
	int act16 = 1;                // in the opt-in fp16 mode the heads' hidden activations and their gradients are STORED as fp16 at the large
	                              // shared-template shapes (use_act16): those layers are HBM-bound, and the matrix pipe rounds them to fp16 anyway
	int bcast_fold = 1;           // inside act16 the broadcast first head layer's output is formed by its readers instead of stored (use_fold)
	int footsum_fold = 1;         // the foot sums of a shared template's first-layer dZ are formed inside the dX GEMM that produces it (mlp_gemm7.h FSUM)
	// internal streams / events
	hipStream_t side[N_SIDE] = {nullptr, nullptr, nullptr, nullptr};
	bool side_bound = false;      // the side streams have been chosen against the hardware queue of a caller's stream (bind_side_streams)
	hipEvent_t ev[N_EVENTS];
	int n_events = 0;
	int next = 0;
	int events_per_call_max = 0;
	hipEvent_t pend_ev[N_SIDE] = {nullptr, nullptr, nullptr, nullptr};   // end of the deferred work on each side stream
	bool pend[N_SIDE] = {};       // side stream k carries deferred work nobody has waited for yet
	bool attr_done[K_COUNT] = {};
	// how the last forward calls that saved a workspace stored the heads' activations (act16): the backward of a workspace follows its
	// forward's decision even if a knob was turned in between (ring of the last 16; a workspace not found falls back to the rule)
	struct Act16Note { const void* ws; bool a16; bool fold; };
	Act16Note act16_notes[16] = {};
	int act16_next = 0;
	// set per call
	bool f16 = false;
	bool x3 = false;              // this call runs its 256 -> 256 layers as bf16x3 (fp32-faithful on the bf16 matrix pipe, mlp_gemm6.h)
};

namespace find {
namespace mlp {

#define FIND_HIP_OK(expr, what)                                                                  \
	do {                                                                                         \
		hipError_t _e = (expr);                                                                  \
		if (_e != hipSuccess) {                                                                  \
			set_error("%s: %s", what, hipGetErrorString(_e));                                    \
			return FIND_ELAUNCH;                                                                 \
		}                                                                                        \
	} while (0)

#define FIND_TRY(expr)                    \
	do {                                  \
		const int _r = (expr);            \
		if (_r != FIND_OK) return _r;     \
	} while (0)

// Co-residence fault: what it was.
// Round 1: with a second workgroup of another stream resident on the same CU, dw2_kernel (weight gradient, both MFMA operands through
// an LDS-DMA ring, one wave per SIMD) produced rare wrong partial tiles -- a rank-1 error of ~1 % in a handful of dW elements, 3 % of the
// backward passes at 4 x 1002 rows, 13 % at 16 x 6890, every pass when the dX GEMMs ran on gemm3 beside it -- with every vmcnt / barrier of
// the ring in place.  Launching the LDS-DMA ring kernels with the WHOLE LDS of their CU made it disappear (0 of 500 passes) and was taken
// for the cure: "an LDS-using neighbour disturbs the ring".  It was a coincidence of which neighbours it kept out.
// Round 2 (tools/check_determinism.py with the knobs named; numbers = wrong tensors per 150 passes of a 16 x 6890 backward):
//   * a stress configuration reproduces it in EVERY pass: the slab reduce replaced by an LDS-free, slow one ("reduce_exclusive" = 2),
//     so that reduces of earlier layers stay resident beside the weight-gradient kernels of later ones: ~850 -- with the LDS reservation
//     on as well as off (it cannot keep an LDS-free kernel out).  The layers that break are exactly those whose weight-gradient launch
//     overlaps a running reduce; on one stream ("bwd_streams" = 0): 0.
//   * not the slabs (a private slab set per weight gradient: same rate); not the ring (every stage of every chunk equals HBM when it is
//     published AND after the wave has consumed it, 2.35 M stages per run); not barrier timing, DMA in flight, M0 hazards, operand-register
//     reuse, barrier flavour (each padded / changed: same rate).
//   * not LDS at all: a four-wave dw4 ("dw4 wide") -- no LDS, no DMA, no barrier, dw2's tile shape read straight from global memory -- breaks the
//     same way (663), while dw4_kernel, the same code with half the tile per wave, never does (0 in 1450 passes).
//   * what the victims share is their REGISTER SHAPE: dw2 312, dw2_group 300, dw4 wide 328 registers per lane -- all 256 accumulator
//     registers (the whole AGPR set) behind fewer than 256 architectural ones, one wave per SIMD.  Every kernel with at most 256 registers
//     was clean; so was the masked gemm3 when it still took 328 (200 architectural + 128 accumulator registers: 0 in 160 stress passes,
//     rebuilt with -DFIND_GEMM3_MIN_WGS=1), so the trigger is narrower than "more than 256".  And dw2 UNCHANGED except for its allocation
//     padded to all 512 registers of the SIMD (FIND_CLAIM_WHOLE_REGISTER_FILE: no foreign wave fits beside it any more): 0 in 600
//     passes, LDS reservation off.
// So: a wave that owns the full accumulator set within an allocation of fewer than 512 registers gets wrong register contents when
// waves of another kernel are allocated on its SIMD.
// The kernel descriptors are right (dw2: granulated VGPR count 38 = 312 registers, accum_offset 56); whether the silicon, the firmware's
// wave save / restore or the runtime mishandles such waves cannot be told from inside a kernel (a stand-alone two-kernel program with a
// 292-register victim ran clean: something else of the step's setting takes part).  The rule adopted, a superset of every shape that
// broke and enforced by tests/test_host_api.py on the compiler's output: a kernel either fits in 256 registers or claims the whole file.  dw4_kernel (<= 256,
// two waves per SIMD, no LDS) is the default weight gradient; dw2 / dw2_group / dw3 claim the file; gemm3 is capped at 256 through its
// launch bounds (the two reproducers -- round 1's dw2 and the wide dw4 -- have been removed since).  The whole-LDS reservation is
// off by default ("lds_exclusive"): the stress runs are clean without it, and what it really did was keep most neighbours away.
template <typename K>
static int prepare_kernel(find_ctx* c, int id, K kernel, int need_bytes, int* launch_bytes, bool reserve = true) {
	const int want = (reserve && c->lds_exclusive) ? c->lds_bytes : need_bytes;
	if (need_bytes > c->lds_bytes) {
		set_error("find_mlp: kernel needs %d bytes of LDS, device %d grants %d per workgroup", need_bytes, c->device, c->lds_bytes);
		return FIND_EINVAL;
	}
	if (!c->attr_done[id]) {
		FIND_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, c->lds_bytes),
					"hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
		c->attr_done[id] = true;
	}
	*launch_bytes = want;
	return FIND_OK;
}

// Fork / join of one entry-point call onto the context's side streams.  fork_to(k) makes side stream k wait for everything issued on
// the caller's stream so far; chain(a, b) orders side stream b behind a; join() -- called on EVERY exit path after the first fork,
// error returns included -- makes the caller's stream wait for every side stream this call touched, so that when the call returns
// the caller may free or reuse any buffer it passed in (stream-ordered).  Every HIP return code is kept: the first failure is
// reported by join().  Works under stream capture: a captured call forks and joins the same streams, so the capture stays closed.
static int bind_side_streams(find_ctx* c, hipStream_t caller);   // (below, with the probe)

struct Fork {
	find_ctx* c;
	hipStream_t s;
	bool on;              // side streams in use for this call
	bool capturing = false;   // the caller's stream is being captured into a HIP graph
	bool deferring = false;   // the call will end in defer() instead of join() (find_mlp_bwd: "defer_join")
	bool used[N_SIDE] = {};
	int n_ev = 0;
	int rc = FIND_OK;

	Fork(find_ctx* ctx, hipStream_t caller, bool enable) : c(ctx), s(caller), on(enable && ctx->side[0] != nullptr) {
		hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
		if (hipStreamIsCapturing(caller, &st) == hipSuccess) capturing = st != hipStreamCaptureStatusNone;
		if (on && !capturing && !ctx->side_bound && ctx->bind_streams) (void)bind_side_streams(ctx, caller);   // (a failed probe keeps the streams as created)
	}
	hipStream_t stream(int k) const { return on ? c->side[k] : s; }
	void fail(hipError_t e, const char* what) {
		if (e != hipSuccess && rc == FIND_OK) {
			set_error("%s: %s", what, hipGetErrorString(e));
			rc = FIND_ELAUNCH;
		}
	}
	hipEvent_t event() {
		hipEvent_t e = c->ev[c->next];
		c->next = (c->next + 1) % N_EVENTS;
		if (++n_ev > N_EVENTS && rc == FIND_OK) {
			set_error("find_mlp: more than %d events in one call", N_EVENTS);
			rc = FIND_ELAUNCH;
		}
		return e;
	}
	void order(hipStream_t from, hipStream_t to) {
		hipEvent_t e = event();
		fail(hipEventRecord(e, from), "hipEventRecord");
		fail(hipStreamWaitEvent(to, e, 0), "hipStreamWaitEvent");
	}
	void fork_to(int k) {
		if (!on) return;
		order(s, c->side[k]);
		used[k] = true;
	}
	// an event that fires when side stream k has run what was issued so far
	hipEvent_t mark(int k) {
		if (!on) return nullptr;
		hipEvent_t e = event();
		fail(hipEventRecord(e, c->side[k]), "hipEventRecord");
		return e;
	}
	void wait(int k, hipEvent_t e) {
		if (on && e) fail(hipStreamWaitEvent(c->side[k], e, 0), "hipStreamWaitEvent");
	}
	void chain(int from, int to) {
		if (!on || from == to) return;
		// a stream enters the call through a fork from the CALLER's stream first, never only through another side stream: under
		// stream capture, hipStreamEndCapture (ROCm 7.0 / 7.2) faults on a capture whose parallel stream was pulled in by a stream
		// that is itself a fork (nested fork); eagerly the extra wait is implied by the one on `from`
		if (!used[to]) fork_to(to);
		order(c->side[from], c->side[to]);
	}
	int join() {
		// (also what an earlier call left running there: find_ctx.pend -- streams are FIFO, waiting for this call's end covers it)
		for (int k = 0; k < N_SIDE; ++k)
			if ((on && used[k]) || (c->pend[k] && !capturing)) { order(c->side[k], s); used[k] = false; c->pend[k] = false; }
		c->events_per_call_max = std::max(c->events_per_call_max, n_ev);
		return rc;
	}
	// instead of join(): the side streams this call touched keep running behind it; whoever needs their results waits for pend_ev
	// (find_ctx_join, or the join() of a later call).  Only the caller may know that nothing reads them before that.
	int defer() {
		if (on)
			for (int k = 0; k < N_SIDE; ++k)
				if (used[k]) { fail(hipEventRecord(c->pend_ev[k], c->side[k]), "hipEventRecord"); c->pend[k] = true; used[k] = false; }
		c->events_per_call_max = std::max(c->events_per_call_max, n_ev);
		return rc;
	}
};

}  // namespace mlp
}  // namespace find

using namespace find;
using namespace find::mlp;

static int check_ctx(const find_ctx* c, const char* who) {
	FIND_REQUIRE(c != nullptr, "%s: ctx is NULL (find_ctx_create)", who);
	int dev = -1;
	if (hipGetDevice(&dev) != hipSuccess || dev != c->device) {
		set_error("%s: the context belongs to device %d, the calling thread's current device is %d", who, c->device, dev);
		return FIND_EINVAL;
	}
	return FIND_OK;
}

// Make `stream` wait for the side-stream work an earlier find_mlp_bwd left running ("defer_join").  Returns 1 if there was any, 0 if not.
extern "C" int find_ctx_join(find_ctx* c, void* stream) {
	FIND_TRY(check_ctx(c, "find_ctx_join"));
	int any = 0;
	for (int k = 0; k < N_SIDE; ++k)
		if (c->pend[k]) {
			FIND_HIP_OK(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), c->pend_ev[k], 0), "hipStreamWaitEvent");
			c->pend[k] = false;
			any = 1;
		}
	return any ? 1 : FIND_OK;
}

// ------------------------------------------------------------------------------------------- streams and hardware queues
// HIP multiplexes streams onto a few hardware queues (GPU_MAX_HW_QUEUES, four by default), in creation order; two streams on one queue
// run their launches in order.  Which of the context's side streams really run beside the caller's stream -- and beside each other --
// therefore depends on what the process created before: a probe launch tells.
namespace find {
namespace mlp {
__global__ void spin_kernel(long long ticks) {
	const long long t0 = wall_clock64();   // 100 MHz
	while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}
__global__ void nop_kernel() {}
}  // namespace mlp
}  // namespace find

// does a launch on b run while a is busy?  "Yes" cannot be wrong (on one queue b's launch cannot finish before a's spin); "no" can, when
// the host thread is held up between b's completion and the query for longer than the spin: a "no" is asked again, twice.
static int runs_beside(hipStream_t a, hipStream_t b, hipEvent_t ea, hipEvent_t eb, bool* beside) {
	*beside = false;
	for (int attempt = 0; attempt < 3 && !*beside; ++attempt) {
		FIND_HIP_OK(hipStreamSynchronize(a), "hipStreamSynchronize");
		FIND_HIP_OK(hipStreamSynchronize(b), "hipStreamSynchronize");
		hipLaunchKernelGGL(find::mlp::spin_kernel, dim3(1), dim3(64), 0, a, 30000ll << attempt);   // ~0.3 ms, then 0.6, 1.2
		FIND_HIP_OK(hipEventRecord(ea, a), "hipEventRecord");
		hipLaunchKernelGGL(find::mlp::nop_kernel, dim3(1), dim3(64), 0, b);
		FIND_HIP_OK(hipEventRecord(eb, b), "hipEventRecord");
		FIND_HIP_OK(hipEventSynchronize(eb), "hipEventSynchronize");
		*beside = hipEventQuery(ea) == hipErrorNotReady;
		FIND_HIP_OK(hipStreamSynchronize(a), "hipStreamSynchronize");
	}
	return FIND_OK;
}

// groups[0] = 0 for the caller's stream, groups[1 + k] for side stream k: streams with the same number share a hardware queue
static int stream_groups(hipStream_t const* st, int n, hipEvent_t ea, hipEvent_t eb, int* groups) {
	int ngroups = 0;
	int rep[16];
	for (int i = 0; i < n; ++i) {
		groups[i] = -1;
		for (int g = 0; g < ngroups && groups[i] < 0; ++g) {
			bool beside = false;
			FIND_TRY(runs_beside(st[rep[g]], st[i], ea, eb, &beside));
			if (!beside) groups[i] = g;
		}
		if (groups[i] < 0) {
			if (ngroups == 16) { groups[i] = 15; continue; }
			rep[ngroups] = i;
			groups[i] = ngroups++;
		}
	}
	return FIND_OK;
}

extern "C" int find_ctx_stream_groups(find_ctx* c, void* caller_stream, int32_t* groups) {
	FIND_TRY(check_ctx(c, "find_ctx_stream_groups"));
	FIND_REQUIRE(groups != nullptr, "find_ctx_stream_groups: groups is NULL");
	hipStream_t st[1 + N_SIDE];
	st[0] = reinterpret_cast<hipStream_t>(caller_stream);
	for (int k = 0; k < N_SIDE; ++k) st[1 + k] = c->side[k];
	int g[1 + N_SIDE];
	FIND_TRY(stream_groups(st, 1 + N_SIDE, c->ev[0], c->ev[1], g));
	for (int k = 0; k < 1 + N_SIDE; ++k) groups[k] = g[k];
	return FIND_OK;
}

namespace find { namespace mlp { static int bind_side_streams(find_ctx* c, hipStream_t caller); } }

// A caller's second stream that fits the context's layout: the first of `cands` that runs BESIDE caller_stream and shares the hardware queue
// of side stream `role` (0 = Q: the large head layers' weight gradients -- busy only during the main pass's backward).  With four hardware
// queues a fifth stream always shares one; which one decides what its work waits behind (find_hip.h).  *index = -1: none of them does.
extern "C" int find_ctx_stream_beside(find_ctx* c, void* caller_stream, void* const* cands, int32_t n, int32_t role, int32_t* index) {
	FIND_TRY(check_ctx(c, "find_ctx_stream_beside"));
	FIND_REQUIRE(cands != nullptr && index != nullptr && n >= 0 && role >= 0 && role < N_SIDE, "find_ctx_stream_beside: bad arguments (role 0..%d)", N_SIDE - 1);
	hipStream_t caller = reinterpret_cast<hipStream_t>(caller_stream);
	if (!c->side_bound && c->bind_streams) (void)find::mlp::bind_side_streams(c, caller);
	*index = -1;
	for (int i = 0; i < n; ++i) {
		hipStream_t s = reinterpret_cast<hipStream_t>(cands[i]);
		bool beside_caller = false, beside_role = true;
		FIND_TRY(runs_beside(caller, s, c->ev[0], c->ev[1], &beside_caller));
		if (!beside_caller) continue;
		FIND_TRY(runs_beside(c->side[role], s, c->ev[0], c->ev[1], &beside_role));
		if (!beside_role) { *index = i; break; }
	}
	return FIND_OK;
}

// The layout the step was tuned with (and gets in a process that creates nothing else first): the large weight gradients (Q) and the two
// small-launch streams (T1, T2) each on a queue of their own, none of them the caller's, and the slab reduces (R) behind T2's queue.
// After torch.distributed has created RCCL's streams the same four hipStreamCreate calls put R on the CALLER's queue -- the reduces then
// sit between the dX GEMMs: 3.47 instead of 3.25 ms per train_3d step on every rank of a multi-GPU run.  So the first call that forks
// chooses its side streams among a dozen candidates by probing (once per context, ~20 ms).
namespace find {
namespace mlp {
static int bind_side_streams(find_ctx* c, hipStream_t caller) {
	c->side_bound = true;   // (one attempt: a failure below keeps the streams as created)
	constexpr int N_CAND = 12;
	hipStream_t st[1 + N_CAND];
	st[0] = caller;
	int n = 1;
	for (int k = 0; k < N_SIDE; ++k) st[n++] = c->side[k];
	for (; n < 1 + N_CAND; ++n)
		if (hipStreamCreateWithFlags(&st[n], hipStreamNonBlocking) != hipSuccess) break;
	int g[1 + N_CAND];
	int rc = stream_groups(st, n, c->ev[0], c->ev[1], g);
	int pick[N_SIDE] = {-1, -1, -1, -1};
	if (rc == FIND_OK) {
		int ng = 0;
		for (int k = 0; k < 3; ++k)   // Q, T1, T2: first candidate on a queue that is neither the caller's nor an earlier pick's
			for (int i = 1; i < n && pick[k] < 0; ++i) {
				bool fresh = g[i] != 0;
				for (int j = 0; j < k; ++j) fresh = fresh && g[i] != g[pick[j]];
				if (fresh) { pick[k] = i; ++ng; }
			}
		if (ng == 3) {
			for (int i = 1; i < n && pick[3] < 0; ++i)   // R: another stream on T2's queue
				if (i != pick[0] && i != pick[1] && i != pick[2] && g[i] == g[pick[2]]) pick[3] = i;
			if (pick[3] < 0)   // (none: any stream that is not on the caller's queue and not a pick)
				for (int i = 1; i < n && pick[3] < 0; ++i)
					if (g[i] != 0 && i != pick[0] && i != pick[1] && i != pick[2]) pick[3] = i;
		}
	}
	const bool ok = rc == FIND_OK && pick[0] > 0 && pick[1] > 0 && pick[2] > 0 && pick[3] > 0;
	hipStream_t chosen[N_SIDE];
	for (int k = 0; k < N_SIDE; ++k) chosen[k] = ok ? st[pick[k]] : c->side[k];
	for (int i = 1; i < n; ++i) {
		bool keep = false;
		for (int k = 0; k < N_SIDE; ++k) keep = keep || st[i] == chosen[k];
		if (!keep) (void)hipStreamDestroy(st[i]);
	}
	for (int k = 0; k < N_SIDE; ++k) c->side[k] = chosen[k];
	return rc;
}
}  // namespace mlp
}  // namespace find

// ------------------------------------------------------------------------------------------- context
extern "C" int find_ctx_create(int device, find_ctx** out) {
	FIND_REQUIRE(out != nullptr, "find_ctx_create: out is NULL");
	*out = nullptr;
	int prev = 0, ndev = 0;
	FIND_HIP_OK(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
	FIND_REQUIRE(device >= 0 && device < ndev, "find_ctx_create: device %d out of range (%d visible)", device, ndev);
	FIND_HIP_OK(hipGetDevice(&prev), "hipGetDevice");
	FIND_HIP_OK(hipSetDevice(device), "hipSetDevice");
	find_ctx* c = new find_ctx();
	c->device = device;
	auto fail = [&](const char* what, hipError_t e) {
		set_error("find_ctx_create: %s: %s", what, hipGetErrorString(e));
		for (int i = 0; i < c->n_events; ++i) (void)hipEventDestroy(c->ev[i]);
		for (int i = 0; i < N_SIDE; ++i) if (c->side[i]) (void)hipStreamDestroy(c->side[i]);
		delete c;
		(void)hipSetDevice(prev);
		return FIND_ELAUNCH;
	};
	hipError_t e;
	int v = 0;
	if ((e = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device)) != hipSuccess) return fail("CU count", e);
	c->num_cus = v > 0 ? v : 256;
	if ((e = hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device)) != hipSuccess) return fail("LDS size", e);
	c->lds_bytes = v;
	for (int i = 0; i < N_SIDE; ++i)
		if ((e = hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreateWithFlags", e);
	for (c->n_events = 0; c->n_events < N_EVENTS; ++c->n_events)
		if ((e = hipEventCreateWithFlags(&c->ev[c->n_events], hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreateWithFlags", e);
	for (int i = 0; i < N_SIDE; ++i)
		if ((e = hipEventCreateWithFlags(&c->pend_ev[i], hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreateWithFlags", e);
	FIND_HIP_OK(hipSetDevice(prev), "hipSetDevice");
	*out = c;
	return FIND_OK;
}

extern "C" int find_ctx_destroy(find_ctx* c) {
	if (!c) return FIND_OK;
	int prev = 0;
	(void)hipGetDevice(&prev);
	(void)hipSetDevice(c->device);
	for (int i = 0; i < N_SIDE; ++i) if (c->side[i]) (void)hipStreamDestroy(c->side[i]);
	for (int i = 0; i < c->n_events; ++i) (void)hipEventDestroy(c->ev[i]);
	(void)hipSetDevice(prev);
	delete c;
	return FIND_OK;
}

namespace {
struct Knob { const char* key; int find_ctx::*field; int64_t lo, hi; };
const Knob KNOBS[] = {
	{"gemm4_small", &find_ctx::gemm4_small, 0, INT32_MAX},
	{"gemm5_min_units", &find_ctx::gemm5_min_units, 0, INT32_MAX},
	{"gemm6_min_units", &find_ctx::gemm6_min_units, 0, INT32_MAX},
	{"mlp_f16", &find_ctx::mlp_f16, 0, 2},
	{"fused_max_units", &find_ctx::fused_max_units, 0, 1024},
	{"fused6", &find_ctx::fused6, 0, 1},
	{"dw2_min_cps", &find_ctx::dw2_min_cps, 1, INT32_MAX},
	{"dw_lds_free", &find_ctx::dw_lds_free, 0, 1},
	{"lds_exclusive", &find_ctx::lds_exclusive, 0, 1},
	{"reduce_exclusive", &find_ctx::reduce_exclusive, 0, 2},
	{"bwd_streams", &find_ctx::bwd_streams, 0, 1},
	{"fwd_streams", &find_ctx::fwd_streams, 0, 1},
	{"reduce_stream", &find_ctx::reduce_stream, 0, 1},
	{"bind_streams", &find_ctx::bind_streams, 0, 1},
	{"defer_join", &find_ctx::defer_join, 0, 1},
	{"act16", &find_ctx::act16, 0, 1},
	{"bcast_fold", &find_ctx::bcast_fold, 0, 1},
	{"footsum_fold", &find_ctx::footsum_fold, 0, 1},
};
}  // namespace

extern "C" int find_ctx_set(find_ctx* c, const char* key, int64_t value) {
	FIND_REQUIRE(c != nullptr && key != nullptr, "find_ctx_set: NULL argument");
	if (strcmp(key, "ablate") == 0) {
		FIND_REQUIRE(value >= 0 && value <= INT32_MAX && (value & ~(int64_t)find::MLP_SWITCHES) == 0,
		             "find_ctx_set: ablate = %lld has bits outside the result-preserving switches 0x%x", (long long)value, find::MLP_SWITCHES);
		c->ablate = (int)value;
		return FIND_OK;
	}
	if (strcmp(key, "gemm4_min_units") == 0) {
		FIND_REQUIRE(value >= 0, "find_ctx_set: gemm4_min_units must be >= 0");
		c->gemm4_min_units = value;
		return FIND_OK;
	}
	for (const Knob& k : KNOBS)
		if (strcmp(key, k.key) == 0) {
			FIND_REQUIRE(value >= k.lo && value <= k.hi, "find_ctx_set: %s = %lld out of range [%lld, %lld]", key, (long long)value, (long long)k.lo, (long long)k.hi);
			c->*(k.field) = (int)value;
			return FIND_OK;
		}
	set_error("find_ctx_set: unknown key %s", key);
	return FIND_EINVAL;
}

extern "C" int find_ctx_get(const find_ctx* c, const char* key, int64_t* value) {
	FIND_REQUIRE(c != nullptr && key != nullptr && value != nullptr, "find_ctx_get: NULL argument");
	if (strcmp(key, "num_cus") == 0) { *value = c->num_cus; return FIND_OK; }
	if (strcmp(key, "pending") == 0) { *value = (c->pend[0] || c->pend[1] || c->pend[2] || c->pend[3]) ? 1 : 0; return FIND_OK; }
	if (strcmp(key, "lds_bytes") == 0) { *value = c->lds_bytes; return FIND_OK; }
	if (strcmp(key, "device") == 0) { *value = c->device; return FIND_OK; }
	if (strcmp(key, "events_per_call_max") == 0) { *value = c->events_per_call_max; return FIND_OK; }
	if (strcmp(key, "gemm4_min_units") == 0) { *value = c->gemm4_min_units; return FIND_OK; }
	if (strcmp(key, "ablate") == 0) { *value = c->ablate; return FIND_OK; }
	for (const Knob& k : KNOBS)
		if (strcmp(key, k.key) == 0) { *value = c->*(k.field); return FIND_OK; }
	set_error("find_ctx_get: unknown key %s", key);
	return FIND_EINVAL;
}
