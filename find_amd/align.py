"""Rigid and similarity alignment of point clouds on the HIP path (find_align_fit, find_icp_run, csrc/align.hip); not in the reference.
Stands in for pytorch3d.ops.corresponding_points_alignment and iterative_closest_point, under PyTorch3D's names and row-vector convention:
a SimilarityTransform (R, T, s) maps x to s * (x @ R) + T -- the convention of the model's registration (oracle/mlp_ref.py: registration),
so a result seeds `reg` directly (reg_from_transform, init_registration).  The ICP loop -- apply, nearest neighbour through the library's
own find_nn_fwd, trimming by an exact k-th smallest distance, the closed-form solve, the convergence rule -- is ONE C call that enqueues
every round and reads nothing back; the rules are in include/find_hip.h.  Every sum is taken in double in a fixed order: two runs agree bit
for bit and a cloud's row does not depend on the rest of the batch.  Nothing here is differentiable: results are detached.  GPU only."""
import math
from typing import NamedTuple

import torch

from . import _lib
from ._lib import check, current_stream, ptr
from .functional import _require_gpu

STATUS_MAX_ITERATIONS = 1   # find_hip.h: FIND_ALIGN_MAX_ITERATIONS
STATUS_DEGENERATE = 2       # FIND_ALIGN_DEGENERATE


class SimilarityTransform(NamedTuple):
	"""x -> s * (x @ R) + T: R (N, 3, 3), T (N, 3), s (N)."""
	R: torch.Tensor
	T: torch.Tensor
	s: torch.Tensor

	def apply(self, points):
		"""points (N, P, 3) -> s * (points @ R) + T, in the points' dtype (plain torch: not a hot path)."""
		R, T, s = (t.to(points.dtype) for t in self)
		return s[:, None, None] * torch.bmm(points, R) + T[:, None, :]


class ICPSolution(NamedTuple):
	"""converged (N) bool; rmse (N) of the used pairs under RTs; Xt (N, P1, 3) = RTs applied to X in fp32 (rows past x_len: zeros); RTs the
	SimilarityTransform; iterations (N) int32, the updates applied; status (N) int32: 0 converged, 1 stopped at max_iterations, 2 degenerate
	(fewer than 3 used pairs or a covariance of rank < 2: the transform of the round before is kept); idx (N, P1) int32 and dist (N, P1), the
	nearest neighbour in Y of every Xt and its squared distance (padding rows -1 / 0); tau (N), the trimming threshold on dist (+inf
	without trimming); used (N) int32, the pairs the rmse was taken over."""
	converged: torch.Tensor
	rmse: torch.Tensor
	Xt: torch.Tensor
	RTs: SimilarityTransform
	iterations: torch.Tensor
	status: torch.Tensor
	idx: torch.Tensor
	dist: torch.Tensor
	tau: torch.Tensor
	used: torch.Tensor


def _cloud(t, what, who):
	if not torch.is_tensor(t) or t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] < 1 or t.shape[1] < 1 or not t.is_floating_point():
		raise ValueError(f'find_amd.align.{who}: {what} (N, P, 3) floating point expected, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}')
	return t


def _lengths(t, n, p_max, what, who):
	if t is None:
		return None
	if not torch.is_tensor(t) or t.dim() != 1 or t.shape[0] != n or t.is_floating_point():
		raise ValueError(f'find_amd.align.{who}: {what} ({n}) integers expected, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}')
	return t


def _f32(t):
	return t.detach().to(torch.float32).contiguous()


def _i32(t, device, p_max):
	"""Lengths as the kernels want them, clamped to [0, p_max] on the device: a length is never an index past the tensor."""
	return None if t is None else t.detach().to(device=device, dtype=torch.int32).clamp(0, p_max).contiguous()


def _workspace(nbytes, what, device):
	if nbytes < 0:
		check(-1, what)
	return torch.empty(max(nbytes // 8, 1), device=device, dtype=torch.float64)


def corresponding_points_alignment(X, Y, weights=None, estimate_scale=False, allow_reflection=False, lengths=None, return_status=False):
	"""The SimilarityTransform that minimises sum_i w_i |s (X_i @ R) + T - Y_i|^2 per cloud (Umeyama / Kabsch; pytorch3d.ops'
	corresponding_points_alignment).  X, Y (N, P, 3) paired by row; weights (N, P) >= 0 or None; lengths (N) the valid pairs of a padded batch.
	estimate_scale False: s = 1.  allow_reflection False: det R = +1.  A cloud with fewer than 3 pairs of positive weight or a covariance of
	rank < 2 gets the identity (never NaN); return_status also returns the (N) int32 status, 2 for such a cloud.  Not differentiable: the
	result is detached."""
	who = 'corresponding_points_alignment'
	_cloud(X, 'X', who), _cloud(Y, 'Y', who)
	if X.shape != Y.shape:
		raise ValueError(f'find_amd.align.{who}: X and Y are paired by row: {tuple(X.shape)} / {tuple(Y.shape)}')
	N, P, _ = X.shape
	if weights is not None and (not torch.is_tensor(weights) or weights.shape != X.shape[:2] or not weights.is_floating_point()):
		raise ValueError(f'find_amd.align.{who}: weights ({N}, {P}) floating point expected, got {tuple(weights.shape) if torch.is_tensor(weights) else weights!r}')
	_lengths(lengths, N, P, 'lengths', who)
	_require_gpu(X, Y, weights)
	L = _lib.lib()
	dev = X.device
	x, y, w, ln = _f32(X), _f32(Y), None if weights is None else _f32(weights), _i32(lengths, dev, P)
	ws = _workspace(L.find_align_ws_bytes(N, P), 'find_align_ws_bytes', dev)
	R = torch.empty(N, 3, 3, device=dev, dtype=torch.float32)
	T = torch.empty(N, 3, device=dev, dtype=torch.float32)
	s = torch.empty(N, device=dev, dtype=torch.float32)
	status = torch.empty(N, device=dev, dtype=torch.int32)
	check(L.find_align_fit(ptr(x), ptr(y), ptr(ln), ptr(w), N, P, int(bool(estimate_scale)), int(bool(allow_reflection)), ptr(R), ptr(T), ptr(s),
						   ptr(status), ptr(ws), ws.numel() * 8, current_stream(dev)), 'find_align_fit')
	tr = SimilarityTransform(R, T, s)
	return (tr, status) if return_status else tr


def iterative_closest_point(X, Y, x_len=None, y_len=None, init_transform=None, max_iterations=50, relative_rmse_thr=1e-6, estimate_scale=False,
							trim=0.0, max_distance=None):
	"""Trimmed ICP from X (N, P1, 3) to Y (N, P2, 3) (pytorch3d.ops.iterative_closest_point): from init_transform (a SimilarityTransform;
	None: identity), rounds of  match every transformed X to its nearest Y  ->  keep the k = m - floor(trim m) closest of a cloud's m pairs
	(ties at the threshold all count; with max_distance also only pairs no farther than it)  ->  the closed-form transform of the ORIGINAL X
	onto its matches.  A cloud stops when its rmse changes by no more than relative_rmse_thr of itself; all of it runs on the device as one
	call, so a converged cloud costs its matches until max_iterations (nothing is read back to skip them).  x_len, y_len (N): the valid rows
	of padded batches.  Returns an ICPSolution whose Xt, idx, dist and rmse belong to the returned transform.  Not differentiable: the result
	is detached."""
	who = 'iterative_closest_point'
	_cloud(X, 'X', who), _cloud(Y, 'Y', who)
	if X.shape[0] != Y.shape[0]:
		raise ValueError(f'find_amd.align.{who}: {X.shape[0]} clouds X, {Y.shape[0]} clouds Y')
	N, P1, P2 = X.shape[0], X.shape[1], Y.shape[1]
	_lengths(x_len, N, P1, 'x_len', who), _lengths(y_len, N, P2, 'y_len', who)
	trim, thr, max_iterations = float(trim), float(relative_rmse_thr), int(max_iterations)
	if not 0. <= trim < 1.:
		raise ValueError(f'find_amd.align.{who}: trim in [0, 1) expected, got {trim}')
	if not thr >= 0. or not 0 <= max_iterations <= 10000:
		raise ValueError(f'find_amd.align.{who}: relative_rmse_thr >= 0 and 0 <= max_iterations <= 10000 expected, got {thr}, {max_iterations}')
	max_dist = math.inf if max_distance is None else float(max_distance)
	if not max_dist > 0.:
		raise ValueError(f'find_amd.align.{who}: max_distance > 0 or None expected, got {max_distance}')
	init = None
	if init_transform is not None:
		if len(init_transform) != 3 or not all(torch.is_tensor(t) for t in init_transform):
			raise ValueError(f'find_amd.align.{who}: init_transform must be a SimilarityTransform (R, T, s)')
		iR, iT, i_s = init_transform
		if iR.shape != (N, 3, 3) or iT.shape != (N, 3) or i_s.shape != (N,):
			raise ValueError(f'find_amd.align.{who}: init_transform of shapes ({N}, 3, 3), ({N}, 3), ({N}) expected, got {tuple(iR.shape)}, {tuple(iT.shape)}, {tuple(i_s.shape)}')
		init = (iR, iT, i_s)
	_require_gpu(X, Y, *(init or ()))
	L = _lib.lib()
	dev = X.device
	x, y, xl, yl = _f32(X), _f32(Y), _i32(x_len, dev, P1), _i32(y_len, dev, P2)
	iR, iT, i_s = (_f32(t) for t in init) if init is not None else (None, None, None)
	ws = _workspace(L.find_icp_ws_bytes(N, P1, P2), 'find_icp_ws_bytes', dev)
	R = torch.empty(N, 3, 3, device=dev, dtype=torch.float32)
	T = torch.empty(N, 3, device=dev, dtype=torch.float32)
	s = torch.empty(N, device=dev, dtype=torch.float32)
	rmse = torch.empty(N, device=dev, dtype=torch.float32)
	iterations = torch.empty(N, device=dev, dtype=torch.int32)
	status = torch.empty(N, device=dev, dtype=torch.int32)
	xt = torch.empty(N, P1, 3, device=dev, dtype=torch.float32)
	dist = torch.empty(N, P1, device=dev, dtype=torch.float32)
	idx = torch.empty(N, P1, device=dev, dtype=torch.int32)
	tau = torch.empty(N, device=dev, dtype=torch.float32)
	used = torch.empty(N, device=dev, dtype=torch.int32)
	check(L.find_icp_run(ptr(x), ptr(xl), ptr(y), ptr(yl), N, P1, P2, ptr(iR), ptr(iT), ptr(i_s), max_iterations, thr, int(bool(estimate_scale)), trim,
						 max_dist, ptr(R), ptr(T), ptr(s), ptr(rmse), ptr(iterations), ptr(status), ptr(xt), ptr(dist), ptr(idx), ptr(tau), ptr(used),
						 ptr(ws), ws.numel() * 8, current_stream(dev)), 'find_icp_run')
	return ICPSolution(status == 0, rmse, xt, SimilarityTransform(R, T, s), iterations, status, idx, dist, tau, used)


def align_meshes(src, dst, samples=10000, generator=None, **icp):
	"""ICP from `samples` surface samples of the Meshes src to as many of dst (losses.sample_points_from_meshes, src first, from `generator`);
	**icp: the keywords of iterative_closest_point.  Returns its ICPSolution: RTs moves src onto dst."""
	from .losses import sample_points_from_meshes
	with torch.no_grad():
		xs = sample_points_from_meshes(src, num_samples=samples, generator=generator)
		ys = sample_points_from_meshes(dst, num_samples=samples, generator=generator)
	return iterative_closest_point(xs, ys, **icp)


def reg_from_transform(tr):
	"""(N, 9) rows [t, euler XYZ, (s, s, s)] of the model's registration for a SimilarityTransform: R = Rx(e0) Ry(e1) Rz(e2), so
	e1 = asin(R[0,2]), e0 = atan2(-R[1,2], R[2,2]), e2 = atan2(-R[0,1], R[0,0]).  Valid for |e1| < pi/2: at |R[0,2]| = 1 (to fp32's
	resolution of the other entries) e0 and e2 are not determined, and a ValueError is raised."""
	R, T, s = tr
	if R.dim() != 3 or R.shape[1:] != (3, 3) or T.shape != (R.shape[0], 3) or s.shape != (R.shape[0],):
		raise ValueError(f'find_amd.align.reg_from_transform: R (N, 3, 3), T (N, 3), s (N) expected, got {tuple(R.shape)}, {tuple(T.shape)}, {tuple(s.shape)}')
	if bool((torch.hypot(R[:, 0, 0], R[:, 0, 1]) <= 1e-6).any()) or bool((R[:, 0, 2].abs() >= 1.).any()):
		raise ValueError('find_amd.align.reg_from_transform: a rotation with |e1| >= pi/2 (gimbal lock of the XYZ Euler angles) has no registration row')
	e1 = torch.asin(R[:, 0, 2])
	e0 = torch.atan2(-R[:, 1, 2], R[:, 2, 2])
	e2 = torch.atan2(-R[:, 0, 1], R[:, 0, 0])
	return torch.cat([T, torch.stack([e0, e1, e2], dim=1), s[:, None].expand(-1, 3)], dim=1)


def transform_from_reg(reg):
	"""The SimilarityTransform of registration rows (N, 9) [t, euler XYZ, S]; an anisotropic S is no similarity and raises ValueError."""
	if reg.dim() != 2 or reg.shape[1] != 9:
		raise ValueError(f'find_amd.align.transform_from_reg: reg (N, 9) expected, got {tuple(reg.shape)}')
	reg = reg.detach()
	S = reg[:, 6:9]
	if not bool((S == S[:, :1]).all()):
		raise ValueError('find_amd.align.transform_from_reg: anisotropic scale: a registration with S = (sx, sy, sz) not all equal is no similarity')
	c, s = torch.cos(reg[:, 3:6]), torch.sin(reg[:, 3:6])
	c0, c1, c2, s0, s1, s2 = c[:, 0], c[:, 1], c[:, 2], s[:, 0], s[:, 1], s[:, 2]
	R = torch.stack([c1 * c2, -c1 * s2, s1,
					 s0 * s1 * c2 + c0 * s2, c0 * c2 - s0 * s1 * s2, -s0 * c1,
					 s0 * s2 - c0 * s1 * c2, c0 * s1 * s2 + s0 * c2, c0 * c1], dim=1).reshape(-1, 3, 3)
	return SimilarityTransform(R, reg[:, :3].clone(), S[:, 0].clone())


def init_registration(model, batch_or_loader, val=False, trim=0.2, estimate_scale=True, samples=5000, generator=None, **icp):
	"""A closed-form start for the registration stage: trimmed ICP from the model's undeformed template (a NeuralDisplacementField's template
	mesh; a PCAModel's mean foot) to every scan of a batch (dict with 'mesh' and the keys its latent tables are addressed by) or of a loader
	of such batches, on `samples` surface samples of each, and the rows of model.reg (val: model.reg_val) overwritten with the result under
	no_grad.  A degenerate cloud (status 2) keeps its row.  Returns the ICPSolution (of all batches, concatenated).  Trainer does not call
	this: its default behaviour is unchanged."""
	from .structures import Meshes
	table = model.reg_val if val else model.reg
	batches = [batch_or_loader] if isinstance(batch_or_loader, dict) else batch_or_loader
	tv, tf = model.template_verts.data.detach(), model.template_faces.data[0]
	sols = []
	with torch.no_grad():
		for batch in batches:
			scans = batch['mesh']
			sel = batch[table.key] if table.labels is not None else batch['idx']
			rows = table.device_index(sel if not isinstance(sel, torch.Tensor) else sel.to(torch.int64))
			if rows is None:
				raise ValueError('find_amd.align.init_registration: the registration table must live on the GPU and be addressed by labels or an index vector')
			sol = align_meshes(Meshes(tv.expand(len(scans), -1, -1).contiguous(), tf), scans, samples=samples, generator=generator, trim=trim,
							   estimate_scale=estimate_scale, **icp)
			new = reg_from_transform(sol.RTs)
			keep = (sol.status & STATUS_DEGENERATE) != 0
			table.data[rows] = torch.where(keep[:, None], table.data[rows], new)
			sols.append(sol)
	if len(sols) == 1:
		return sols[0]
	cat = [torch.cat(f) if torch.is_tensor(f[0]) else SimilarityTransform(*(torch.cat(g) for g in zip(*f))) for f in zip(*sols)]
	return ICPSolution(*cat)
