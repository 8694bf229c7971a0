"""The skinned foot model's definition (include/find_hip.h: find_skin_fwd) restated in torch, in a chosen dtype, differentiable everywhere
-- at theta = 0 too -- and, beside it, a literal transcription of the form STAR / SUPR publish (v_shaped, the regressor on v_shaped,
quaternions turned into matrices, 4 x 4 transforms, the rest pose subtracted) from the raw arrays of a model file.  The tests run it on
the CPU; it follows the device of `pose` (tools/skin_cost.py times it on the GPU).

sin a / a and (1 - cos a) / a^2 as functions of x = a^2: below x = 1/4 the power series to x^8 (what is left out is under 1e-22), above it
sin(a) / a and 2 sin^2(a/2) / a^2, neither of which cancels.  The square root never sees an x below 1/4, so no branch of a torch.where
carries a NaN gradient."""
import math

import numpy as np
import torch


def exp_coefs(x):
	"""(sin a / a, (1 - cos a) / a^2) for x = a^2 >= 0."""
	small = x < 0.25
	xs = torch.where(small, x, torch.zeros_like(x))
	A_s, B_s = torch.zeros_like(x), torch.zeros_like(x)
	for n in range(8, -1, -1):
		A_s = A_s * xs + (-1.0) ** n / math.factorial(2 * n + 1)
		B_s = B_s * xs + (-1.0) ** n / math.factorial(2 * n + 2)
	a = torch.sqrt(torch.where(small, torch.ones_like(x), x))
	A_b = torch.sin(a) / a
	B_b = 2 * torch.sin(0.5 * a) ** 2 / (a * a)
	return torch.where(small, A_s, A_b), torch.where(small, B_s, B_b)


def skew(th):
	x, y, z = th.unbind(-1)
	o = torch.zeros_like(x)
	return torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(th.shape[:-1] + (3, 3))


def rotations(th):
	"""R = I + (sin a / a) K + ((1 - cos a) / a^2) K^2 for th (..., 3)."""
	x = (th * th).sum(-1)
	A, B = exp_coefs(x)
	K = skew(th)
	return torch.eye(3, dtype=th.dtype, device=th.device) + A[..., None, None] * K + B[..., None, None] * (K @ K)


def quaternions(th):
	"""q = ((sin(a/2) / a) th, cos(a/2) - 1) for th (..., 3)."""
	h2 = 0.25 * (th * th).sum(-1)
	A, B = exp_coefs(h2)
	return torch.cat([0.5 * A[..., None] * th, (-h2 * B)[..., None]], -1)


def skin(consts, pose, betas, trans, dtype=torch.float64, return_joints=False):
	"""out (N, V, 3) [, posed joints (N, J, 3)] from the prepared constants (v_template, dirs, J0, JS, weights, parent), all cast to dtype
	(and moved to pose's device)."""
	vt, dirs, J0, JS, w = (consts[k].detach().to(device=pose.device, dtype=dtype) for k in ('v_template', 'dirs', 'J0', 'JS', 'weights'))
	parent = [int(p) for p in consts['parent']]
	pose, betas, trans = pose.to(dtype), betas.to(dtype), trans.to(dtype)
	N, J, B = pose.shape[0], len(parent), JS.shape[1]
	P = dirs.shape[1] - B
	assert P in (4 * J, 4 * (J - 1))
	th = pose.reshape(N, J, 3)
	R = rotations(th)
	q = quaternions(th)
	feat = (q if P == 4 * J else q[:, 1:]).reshape(N, P)
	c = torch.cat([betas, feat], 1)
	vp = vt[None] + torch.einsum('vkc,nk->nvc', dirs, c)
	Jn = J0[None] + torch.einsum('jbc,nb->njc', JS, betas)
	GR, Gt = [None] * J, [None] * J
	for j, p in enumerate(parent):
		if p < 0:
			GR[j], Gt[j] = R[:, j], Jn[:, j]
		else:
			GR[j] = GR[p] @ R[:, j]
			Gt[j] = (GR[p] @ (Jn[:, j] - Jn[:, p])[..., None])[..., 0] + Gt[p]
	AR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)
	At = Gt - (AR @ Jn[..., None])[..., 0]
	MR = torch.einsum('vj,njrc->nvrc', w, AR)
	Mt = torch.einsum('vj,njr->nvr', w, At)
	out = (MR @ vp[..., None])[..., 0] + Mt + trans[:, None]
	return (out, Gt) if return_joints else out


def with_grads(consts, pose, betas, trans, d_out, dtype):
	"""(out, d_pose, d_betas, d_trans) of sum(out * d_out) in dtype, on the CPU."""
	p, b, t = (x.detach().cpu().to(dtype).requires_grad_(True) for x in (pose, betas, trans))
	out = skin(consts, p, b, t, dtype)
	gp, gb, gt = torch.autograd.grad(out, (p, b, t), d_out.detach().cpu().to(dtype))
	return out.detach(), gp, gb, gt


# ------------------------------------------------------------------------------------------------ the published form
def _quat2mat(q):
	"""Rotation matrix of a quaternion (x, y, z, w), normalised first: the published quat2mat."""
	q = q / np.linalg.norm(q)
	x, y, z, w = q
	return np.array([[w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z],
					 [2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x],
					 [2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z]])


def published(data, pose, betas, trans, num_betas):
	"""One foot, float64 numpy, from the raw arrays of a model file (v_template, shapedirs (V, 3, >= B), posedirs (V, 3, P), J_regressor
	(J, V), weights, kintree_table): v_shaped = v_template + shapedirs . betas;  J = J_regressor v_shaped;  per joint the quaternion
	(sin(a/2) th / a, cos(a/2)), its feature (.., cos(a/2) - 1) and its matrix;  v_posed = v_shaped + posedirs . features;  4 x 4 world
	transforms down the kinematic tree;  the rest pose subtracted (G_j [I | -J_j]);  T_v = sum_j w_vj A_j;  T_v [v_posed; 1] + trans.
	The angle is |th| (the published code's + 1e-8 is the recorded difference); a zero rotation gives the identity quaternion."""
	vt = np.asarray(data['v_template'], np.float64)
	sd = np.asarray(data['shapedirs'], np.float64)[:, :, :num_betas]
	pd = np.asarray(data['posedirs'], np.float64)
	jr = np.asarray(data['J_regressor'], np.float64)
	w = np.asarray(data['weights'], np.float64)
	J = w.shape[1]
	par = [int(p) if 0 <= int(p) < J else -1 for p in np.asarray(data['kintree_table'])[0]]
	pose, betas, trans = (np.asarray(a, np.float64) for a in (pose, betas, trans))
	v_shaped = vt + sd @ betas
	joints = jr @ v_shaped
	quats = []
	for j in range(J):
		th = pose[3 * j:3 * j + 3]
		a = np.linalg.norm(th)
		axis = th / a if a > 0 else np.zeros(3)
		quats.append(np.concatenate([np.sin(a / 2) * axis, [np.cos(a / 2)]]))
	feats = [q - np.array([0, 0, 0, 1.0]) for q in quats]
	feat = np.concatenate(feats if pd.shape[2] == 4 * J else feats[1:]) if pd.shape[2] else np.zeros(0)
	v_posed = v_shaped + pd @ feat
	G = [None] * J
	for j in range(J):
		local = np.eye(4)
		local[:3, :3] = _quat2mat(quats[j])
		local[:3, 3] = joints[j] - (joints[par[j]] if par[j] >= 0 else 0)
		G[j] = local if par[j] < 0 else G[par[j]] @ local
	A = []
	for j in range(J):
		rest = np.eye(4)
		rest[:3, 3] = -joints[j]
		A.append(G[j] @ rest)
	T = np.einsum('vj,jab->vab', w, np.stack(A))
	vh = np.concatenate([v_posed, np.ones((len(v_posed), 1))], 1)
	out = np.einsum('vab,vb->va', T, vh)[:, :3] + trans
	return out, np.stack([g[:3, 3] for g in G])
