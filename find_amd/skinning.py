"""The skinned foot model's decode: SMPL-family linear blend skinning with quaternion pose correctives (as STAR / SUPR publish it) as one HIP
call each way, find_skin_fwd / find_skin_bwd (csrc/skin.hip; the definition: include/find_hip.h).  find_amd.functional.linear_blend_skinning
is this module's function; model.SkinnedModel calls it.  CUDA(HIP) fp32 tensors only: there is no CPU or eager fallback.  Workspaces come
from functional._ws."""
import torch

from . import _lib
from . import functional as FN
from ._lib import check, current_stream, ptr

SKIN_CONSTS = ('v_template', 'dirs', 'J0', 'JS', 'weights', 'parent')


def _skin_consts(consts):
	"""The six model tensors of linear_blend_skinning from a mapping or an object with those attributes, shapes checked."""
	get = consts.__getitem__ if hasattr(consts, '__getitem__') else lambda k: getattr(consts, k)
	vt, dirs, J0, JS, w, parent = (get(k) for k in SKIN_CONSTS)
	V, J = w.shape if w.dim() == 2 else (-1, -1)
	B = JS.shape[1] if JS.dim() == 3 else -1
	ok = (vt.shape == (V, 3) and dirs.dim() == 3 and dirs.shape[0] == V and dirs.shape[2] == 3 and J0.shape == (J, 3) and JS.shape == (J, B, 3)
		  and parent.shape == (J,) and parent.dtype == torch.int32 and dirs.shape[1] - B in (4 * J, 4 * (J - 1)) and B >= 1)
	if not ok:
		raise RuntimeError('find_amd.linear_blend_skinning: bad model shapes ' + ', '.join(f'{k} {tuple(t.shape)}' for k, t in zip(SKIN_CONSTS, (vt, dirs, J0, JS, w, parent)))
						   + f' (parent {parent.dtype}); want v_template (V, 3), dirs (V, B+P, 3) with P = 4J or 4(J-1), J0 (J, 3), JS (J, B, 3), weights (V, J), parent (J) int32')
	return vt, dirs, J0, JS, w, parent


class _Skin(torch.autograd.Function):
	"""find_skin_fwd / find_skin_bwd: (pose, betas, trans) -> (verts (N, V, 3), posed joints (N, J, 3), the latter without gradient)."""

	@staticmethod
	def forward(ctx, pose, betas, trans, vt, dirs, J0, JS, w, parent):
		FN._require_gpu(pose, betas, trans, vt, dirs, J0, JS, w, parent)
		for k, t in zip(SKIN_CONSTS, (vt, dirs, J0, JS, w, parent)):
			if t.requires_grad:
				raise RuntimeError(f'find_amd.linear_blend_skinning: {k} is a constant of the model (requires_grad=False); only pose, betas and trans get a gradient')
			if t.device != pose.device:
				raise RuntimeError(f'find_amd.linear_blend_skinning: {k} on {t.device}, pose on {pose.device}')
		V, J = w.shape
		B, P = JS.shape[1], dirs.shape[1] - JS.shape[1]
		N = pose.shape[0]
		if pose.shape != (N, 3 * J) or betas.shape != (N, B) or trans.shape != (N, 3):
			raise RuntimeError(f'find_amd.linear_blend_skinning: bad shapes pose {tuple(pose.shape)} (want (N, {3 * J})) betas {tuple(betas.shape)} '
							   f'(want (N, {B})) trans {tuple(trans.shape)} (want (N, 3))')
		L = _lib.lib()
		pose, betas, trans = FN._c(pose), FN._c(betas), FN._c(trans)
		consts = tuple(FN._c(t) for t in (vt, dirs, J0, JS, w, parent))
		out = torch.empty(N, V, 3, dtype=torch.float32, device=pose.device)
		joints = torch.empty(N, J, 3, dtype=torch.float32, device=pose.device)
		ctx.mark_non_differentiable(joints)
		if N == 0:
			return out, joints
		ws = FN._ws(L.find_skin_fwd_ws_bytes(N, V, J, B, P), pose.device)
		check(L.find_skin_fwd(*(ptr(t) for t in consts), V, J, B, P, ptr(pose), ptr(betas), ptr(trans), N, ptr(out), ptr(joints), ptr(ws), ws.numel(),
							  current_stream(pose.device)), 'find_skin_fwd')
		ctx.save_for_backward(pose, betas, *consts)
		return out, joints

	@staticmethod
	def backward(ctx, g, _g_joints):
		L = _lib.lib()
		pose, betas, *consts = ctx.saved_tensors
		V, J = consts[4].shape
		B, P = consts[3].shape[1], consts[1].shape[1] - consts[3].shape[1]
		N = pose.shape[0]
		g = FN._c(g)
		d_pose, d_betas = torch.empty_like(pose), torch.empty_like(betas)
		d_trans = torch.empty(N, 3, dtype=torch.float32, device=g.device)
		ws = FN._ws(L.find_skin_bwd_ws_bytes(N, V, J, B, P), g.device)
		check(L.find_skin_bwd(*(ptr(t) for t in consts), V, J, B, P, ptr(pose), ptr(betas), ptr(g), N, ptr(d_pose), ptr(d_betas), ptr(d_trans), ptr(ws),
							  ws.numel(), current_stream(g.device)), 'find_skin_bwd')
		return (d_pose, d_betas, d_trans) + (None,) * 6


def linear_blend_skinning(consts, pose, betas, trans, return_joints=False):
	"""Vertices (N, V, 3) of a skinned model (SMPL-family linear blend skinning with quaternion pose correctives, as STAR / SUPR publish it;
	the definition: include/find_hip.h) from axis-angle poses (N, 3J), shape coefficients (N, B) and translations (N, 3); HIP forward and
	backward (find_skin_fwd / find_skin_bwd), gradients to those three only.  consts: a mapping (or object) with v_template (V, 3), dirs
	(V, B+P, 3) -- shape directions first, then pose directions; P = 4J or 4(J-1) --, J0 (J, 3), JS (J, B, 3), weights (V, J) and parent (J)
	int32, as SkinnedModel prepares them on load.  return_joints: also the posed joint positions (N, J, 3), detached."""
	verts, joints = _Skin.apply(pose, betas, trans, *_skin_consts(consts))
	return (verts, joints) if return_joints else verts
