"""Oracle (TEST INFRASTRUCTURE ONLY) for rows a1-a5: torch-CPU fp32, op-for-op what the reference executes.

PINNED for a1-a4 by tests/golden/mlp_main.npz + mlp_variants.npz (tests/test_oracle_mlp.py).
a5 (registration) follows PyTorch3D's euler_angles_to_matrix / Transform3d conventions: PARITY UNPINNED
(dependency absent), anchored by known-answer tests against scipy.spatial.transform.Rotation.

Weights are passed as a reference-format state_dict (SURVEY §8b key names).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def fourier_B(num_input_channels=3, mapping_size=256, scale=10.0):
	"""fourier_feature_transform.py:17-26.  Reseeds the *global* torch RNG to 1 (a reference quirk that makes
	every later nn.Linear init deterministic) and sorts the num_input_channels ROWS of B by L2 norm."""
	torch.manual_seed(1)
	B = torch.randn((num_input_channels, mapping_size)) * scale
	B_sort = sorted(B, key=lambda x: torch.norm(x, p=2))
	return torch.stack(B_sort)


def fourier_features(x, B):
	"""fourier_feature_transform.py:28-55:  [x, sin(2*pi*x@B), cos(2*pi*x@B)] on the last dim."""
	shp = x.shape
	x2 = x.reshape(-1, shp[-1])
	res = x2 @ B
	res = 2 * np.pi * res
	out = torch.cat([x2, torch.sin(res), torch.cos(res)], dim=1)
	return out.reshape(*shp[:-1], out.shape[-1])


def _seq(sd, prefix, x, final_linear, pre=None):
	"""nn.Sequential / ModuleList of Linear(+ReLU) stored at even indices (model.py:250-257, 351-371).
	pre: a list that receives every ReLU's input (detached), in layer order."""
	idxs = sorted({int(k.split('.')[1]) for k in sd if k.startswith(prefix + '.') and k.endswith('.weight')})
	for n, i in enumerate(idxs):
		x = F.linear(x, sd[f'{prefix}.{i}.weight'], sd[f'{prefix}.{i}.bias'])
		if not (final_linear and n == len(idxs) - 1):
			if pre is not None:
				pre.append(x.detach())
			x = torch.relu(x)
	return x


def relu_stats(pre):
	"""Per ReLU layer of one evaluation: each row's smallest |pre-activation| (..., L), and the layer's sum of squares and entry count (L,)
	-- what relu_margin needs; stats of several evaluations (row chunks, feet) combine by concatenating the first and adding the others."""
	rowmin = torch.stack([p.abs().amin(-1) for p in pre], -1)
	ss = torch.stack([(p.double() ** 2).sum() for p in pre])
	cnt = torch.tensor([float(p.numel()) for p in pre], dtype=torch.float64)
	return rowmin, ss, cnt


def relu_margin(rowmin, ss, cnt):
	"""A row's ReLU margin: min over the ReLU layers of (its smallest |pre-activation| in that layer) / rms(that layer's pre-activations).
	A row whose margin is ~ the relative rounding error of the arithmetic may see one of its ReLU masks flip between two evaluations
	that are both correct to that rounding: its gradient is then not a property of the arithmetic (a tie)."""
	rms = torch.sqrt(ss / cnt)
	return (rowmin.double() / rms).amin(-1)


def mlp_forward(sd, B, pos, shapevec=None, texvec=None, posevec=None, use_avg_colour=False, positional_encoding=True, margins=False):
	"""NeuralDisplacementField.forward, model.py:393-453.  Returns dict(disp, col, trunk); margins=True adds 'margin' (batch, npts):
	relu_margin over the 11 ReLU layers of both heads and the trunk, rms over every row of this call (a template shared by the feet is
	expanded first, so a trunk margin applies to that vertex in every foot), and 'relu_stats' (relu_stats of this call)."""
	batch, npts, _ = pos.shape
	if batch == 1 and shapevec is not None:  # model.py:404-406
		batch = shapevec.shape[0]
		pos = pos.expand(batch, -1, -1)
	if shapevec is not None:
		shapevec = shapevec.unsqueeze(1).expand(-1, npts, -1)
	if posevec is not None:
		posevec = posevec.unsqueeze(1).expand(-1, npts, -1)
	if texvec is not None:
		texvec = texvec.unsqueeze(1).expand(-1, npts, -1)

	pre = [] if margins else None
	x = fourier_features(pos, B) if positional_encoding else pos  # model.py:421-422
	x = _seq(sd, 'base', x, final_linear=False, pre=pre)  # model.py:424-426

	disp_input = x
	if shapevec is not None:
		disp_input = torch.cat([disp_input, shapevec], dim=-1)
	if posevec is not None:
		disp_input = torch.cat([disp_input, posevec], dim=-1)
	col_input = x
	if texvec is not None:
		col_input = torch.cat([col_input, texvec], dim=-1)

	disp = _seq(sd, 'mlp_disp', disp_input, final_linear=True, pre=pre)
	col = _seq(sd, 'mlp_col', col_input, final_linear=True, pre=pre)
	disp = 0.1 * torch.tanh(disp)  # model.py:444
	if use_avg_colour:
		col = sd['avg_col'][None, None, :] + 0.5 * (1 + torch.tanh(col))  # model.py:447
	else:
		col = 0.5 * (1 + torch.tanh(col))  # model.py:449
	out = dict(disp=disp, col=col, trunk=x)
	if margins:
		out['relu_stats'] = relu_stats(pre)
		out['margin'] = relu_margin(*out['relu_stats'])
	return out


def euler_angles_to_matrix_xyz(e):
	"""PyTorch3D euler_angles_to_matrix(e, 'XYZ') = Rx(e0) @ Ry(e1) @ Rz(e2) [P3D-recall; SURVEY A.1].
	e: (..., 3) radians -> (..., 3, 3)."""
	c, s = torch.cos(e), torch.sin(e)
	one, zero = torch.ones_like(c[..., 0]), torch.zeros_like(c[..., 0])

	def mat(rows):
		return torch.stack([torch.stack(r, dim=-1) for r in rows], dim=-2)

	Rx = mat([[one, zero, zero], [zero, c[..., 0], -s[..., 0]], [zero, s[..., 0], c[..., 0]]])
	Ry = mat([[c[..., 1], zero, s[..., 1]], [zero, one, zero], [-s[..., 1], zero, c[..., 1]]])
	Rz = mat([[c[..., 2], -s[..., 2], zero], [s[..., 2], c[..., 2], zero], [zero, zero, one]])
	return Rx @ Ry @ Rz


def registration(verts, disp, reg):
	"""get_meshes, model.py:481-491:  Transform3d().scale(S).rotate(R).translate(t).transform_points(v+disp).
	Row-vector convention: X = ((v + disp) * S) @ R + t   [P3D-recall; SURVEY A.1]."""
	if reg is None:
		return verts + disp
	S = reg[..., 6:9]
	t = reg[..., :3]
	R = euler_angles_to_matrix_xyz(reg[..., 3:6])
	p = (verts + disp) * S[:, None, :]
	return torch.bmm(p, R) + t[:, None, :]


def get_meshes_verts(sd, B, template_verts, shapevec, reg, texvec, posevec, use_avg_colour=False):
	"""get_meshes numeric core (model.py:455-504): returns dict(verts, disp, col)."""
	N = 0 if shapevec is None else shapevec.shape[0]
	verts = template_verts.expand(N, -1, -1)
	res = mlp_forward(sd, B, verts, shapevec, texvec, posevec, use_avg_colour)
	X = registration(verts, res['disp'], reg)
	return dict(verts=X, disp=res['disp'], col=res['col'])


# ------------------------------------------------------------------------------------------------ whole-model evaluation, foot by foot
TRAINABLE = ('base', 'mlp_disp', 'mlp_col')
LATENTS = ('shapevec', 'texvec', 'posevec', 'reg')


def _feet_rows(pos, n_feet, chunk):
	"""(foot, row slice) pieces of an evaluation: a batch-1 pos is a template every foot shares."""
	V = pos.shape[1]
	for f in range(n_feet):
		for r0 in range(0, V, chunk):
			yield f, slice(r0, min(V, r0 + chunk))


def _cast(sd, B, dtype, grad):
	p = {k: v.detach().to(dtype).clone().requires_grad_(grad and v.is_floating_point() and k.split('.')[0] in TRAINABLE) for k, v in sd.items()
		 if v.is_floating_point() and k.split('.')[0] in TRAINABLE + ('avg_col',)}
	return p, B.detach().to(dtype)


def model_margins(sd, B, pos, shapevec, texvec, posevec, dtype=torch.float64, chunk=8192):
	"""relu_margin of every output row (n_feet, V) of mlp_forward(sd, B, pos, ...) -- the rms of a layer over all n_feet x V rows, as one
	batched mlp_forward(margins=True) gives it -- evaluated foot by foot in row chunks (no autograd), so that any size fits in host memory.
	Inputs are cast exactly from what they are (fp32 parameters, positions, latents) to dtype."""
	p, Bd = _cast(sd, B, dtype, False)
	N = shapevec.shape[0]
	mins, ss, cnt = {}, 0, 0
	with torch.no_grad():
		for f, rs in _feet_rows(pos, N, chunk):
			pf = (pos[0] if pos.shape[0] == 1 else pos[f])[rs].to(dtype)[None]
			r = mlp_forward(p, Bd, pf, *(x[f:f + 1].to(dtype) for x in (shapevec, texvec, posevec)), margins=True)
			rowmin, s_, c_ = r['relu_stats']
			mins[(f, rs.start)] = rowmin[0]
			ss, cnt = ss + s_, cnt + c_
	rowmin = torch.stack([torch.cat([mins[k] for k in sorted(mins) if k[0] == f]) for f in range(N)])
	return relu_margin(rowmin, ss, cnt)


def model_eval(sd, B, pos, shapevec, texvec, posevec, reg=None, up=None, up_col=None, dtype=torch.float64, chunk=8192, use_avg_colour=False):
	"""The model's outputs and gradients, evaluated foot by foot in row chunks with every gradient summed over them: the whole-model oracle
	for any size (a 3 x 50 002-row call needs a few GB).  Inputs are cast exactly to dtype: float64 is the yardstick, float32 the reference's
	own arithmetic.
	pos (1 | N, V, 3): batch 1 is a template shared by the N feet.  reg (N, 9) given: the first output is the registered vertices
	(get_meshes_verts), else the displacement.  up / up_col (N, V, 3): upstream gradients of the two outputs (None: that output is not in
	the loss -- up None and up_col given is the colour-only pass; both None: forward only).
	Returns dict(out, col, grads): grads maps every trainable parameter (state_dict names) and 'shapevec' / 'texvec' / 'posevec' / 'reg' to
	its gradient in dtype -- those that receive none (a head outside the loss) are left out, as autograd leaves them None."""
	backward = up is not None or up_col is not None
	p, Bd = _cast(sd, B, dtype, backward)
	N, V = shapevec.shape[0], pos.shape[1]
	lat = {k: x.detach().to(dtype).clone().requires_grad_(backward) for k, x in zip(LATENTS, (shapevec, texvec, posevec, reg)) if x is not None}
	out = torch.empty(N, V, 3, dtype=dtype)
	col = torch.empty(N, V, 3, dtype=dtype)
	with torch.set_grad_enabled(backward):
		for f, rs in _feet_rows(pos, N, chunk):
			pf = (pos[0] if pos.shape[0] == 1 else pos[f])[rs].to(dtype)[None]
			sv, tv, pv = (lat[k][f:f + 1] for k in LATENTS[:3])
			if reg is not None:
				r = get_meshes_verts(p, Bd, pf, sv, lat['reg'][f:f + 1], tv, pv, use_avg_colour)
				o = r['verts']
			else:
				r = mlp_forward(p, Bd, pf, sv, tv, pv, use_avg_colour)
				o = r['disp']
			out[f, rs], col[f, rs] = o[0].detach(), r['col'][0].detach()
			if backward:
				loss = 0
				if up is not None:
					loss = loss + (o[0] * up[f, rs].to(dtype)).sum()
				if up_col is not None:
					loss = loss + (r['col'][0] * up_col[f, rs].to(dtype)).sum()
				loss.backward()
	grads = {k: v.grad for k, v in list(p.items()) + list(lat.items()) if v.grad is not None}
	return dict(out=out, col=col, grads=grads)
