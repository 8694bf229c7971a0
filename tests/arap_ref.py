"""The as-rigid-as-possible energy restated in torch on the CPU, in float64 or float32: the definition the HIP path (find_amd/csrc/arap.hip,
functional.arap_energy) is held to.

  weights  w_ij = w_ji: 'cotangent': 1/2 sum of cot of the angles opposite edge ij in the REST mesh (one or two faces), float64 on the host,
           clamped below at 0, rounded to fp32;  'uniform': 1.        W = sum over all directed edges of the fp32 weights, in float64.
  S_i = sum_j w_ij (q_i - q_j)(p_i - p_j)^T = U D V^T,   R_i = V diag(1, 1, det(V U^T)) U^T
  E   = (1 / W) sum_i sum_j w_ij |(p_i - p_j) - R_i (q_i - q_j)|^2
  dE/dp_i = (2 / W) sum_j w_ij [2 (p_i - p_j) - (R_i + R_j)(q_i - q_j)]          (rotations fixed)
  a cell with D_1 = 0 or D_2 <= RANK_TOL D_1 (no neighbours, collapsed or collinear ones): R_i = I, counted."""
import numpy as np
import torch

RANK_TOL = 1e-12   # of the definition


def directed_edges(faces):
	"""(ei, ej) int64 numpy: every edge of the faces in both directions, once each, sorted by (i, j)."""
	f = np.asarray(faces, np.int64).reshape(-1, 3)
	e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
	e = np.unique(np.concatenate([e, e[:, ::-1]], 0), axis=0)
	return e[:, 0].copy(), e[:, 1].copy()


def cotangent_by_face(rest, faces):
	"""{(i, j): 1/2 sum cot} in float64, UNCLAMPED, face by face (a plain loop: the direct evaluation)."""
	q = np.asarray(rest, np.float64).reshape(-1, 3)
	out = {}
	for tri in np.asarray(faces, np.int64).reshape(-1, 3):
		for c in range(3):
			o, a, b = int(tri[c]), int(tri[(c + 1) % 3]), int(tri[(c + 2) % 3])
			u, v = q[a] - q[o], q[b] - q[o]
			area2 = np.linalg.norm(np.cross(u, v))
			cot = float(u @ v) / area2 if area2 > 0 else 0.
			out[(a, b)] = out.get((a, b), 0.) + 0.5 * cot
			out[(b, a)] = out.get((b, a), 0.) + 0.5 * cot
	return out


def edge_weights(rest, faces, ei, ej, weights='cotangent'):
	"""fp32 numpy weights of the directed edges (ei, ej), and W."""
	if weights == 'uniform':
		w = np.ones(len(ei), np.float32)
	else:
		raw = cotangent_by_face(rest, faces)
		w = np.array([max(raw[(int(i), int(j))], 0.) for i, j in zip(ei, ej)], np.float64).astype(np.float32)
	return w, float(w.astype(np.float64).sum())


class Rest:
	def __init__(self, rest, faces, weights='cotangent'):
		self.q = torch.as_tensor(rest).detach().cpu().reshape(-1, 3).float()
		self.faces = torch.as_tensor(faces).detach().cpu().reshape(-1, 3).long()
		ei, ej = directed_edges(self.faces.numpy())
		w, self.W = edge_weights(self.q.numpy(), self.faces.numpy(), ei, ej, weights)
		self.ei, self.ej, self.w = torch.from_numpy(ei), torch.from_numpy(ej), torch.from_numpy(w)
		self.V = self.q.shape[0]


def rotations(p, rest, dtype=torch.float64):
	"""R (N, V, 3, 3), degenerate (N, V) bool, D (N, V, 3), S (N, V, 3, 3) from fp32 p (N, V, 3), all arithmetic in `dtype`.  Differentiable in p
	through torch.linalg.svd when p carries a graph."""
	p = p.to(dtype)
	q, w = rest.q.to(dtype), rest.w.to(dtype)
	eq = q[rest.ei] - q[rest.ej]                                     # (E, 3)
	ep = p[:, rest.ei] - p[:, rest.ej]                               # (N, E, 3)
	S = torch.zeros(p.shape[0], rest.V, 3, 3, dtype=dtype).index_add(1, rest.ei, (w[:, None] * eq)[None, :, :, None] * ep[:, :, None, :])
	U, D, Vh = torch.linalg.svd(S)
	Vm = Vh.transpose(-1, -2)
	sign = torch.where(torch.linalg.det(Vm @ U.transpose(-1, -2)) < 0, -1., 1.).to(dtype)
	flip = torch.stack([torch.ones_like(sign), torch.ones_like(sign), sign], -1)
	R = (Vm * flip[..., None, :]) @ U.transpose(-1, -2)
	degenerate = (D[..., 0] == 0) | (D[..., 1] <= RANK_TOL * D[..., 0])
	R = torch.where(degenerate[..., None, None], torch.eye(3, dtype=dtype).expand_as(R), R)
	return R, degenerate, D, S


def energy(p, rest, dtype=torch.float64, R=None):
	"""dict(E (N,), cell (N, V) -- already / W --, R, degenerate (N,) counts, D) in `dtype`.  R given: those rotations instead of fitted ones."""
	fitted, deg, D, _ = rotations(p, rest, dtype)
	R = fitted if R is None else R
	p = p.to(dtype)
	q, w = rest.q.to(dtype), rest.w.to(dtype)
	eq = q[rest.ei] - q[rest.ej]
	ep = p[:, rest.ei] - p[:, rest.ej]
	r = ep - torch.einsum('neab,eb->nea', R[:, rest.ei], eq)
	inv_w = 1. / rest.W if rest.W > 0 else 0.
	cell = torch.zeros(p.shape[0], rest.V, dtype=dtype).index_add(1, rest.ei, w * (r * r).sum(-1)) * inv_w
	return dict(E=cell.sum(1), cell=cell, R=R, degenerate=deg.sum(1).to(torch.int32), D=D)


def gradient(p, rest, g, dtype=torch.float64, R=None):
	"""sum_n g_n dE_n/dp (N, V, 3) by the fixed-rotation formula, in `dtype`."""
	if R is None:
		R = rotations(p, rest, dtype)[0]
	p = p.to(dtype)
	q, w = rest.q.to(dtype), rest.w.to(dtype)
	eq = q[rest.ei] - q[rest.ej]
	ep = p[:, rest.ei] - p[:, rest.ej]
	term = w[:, None] * (2 * ep - torch.einsum('neab,eb->nea', R[:, rest.ei] + R[:, rest.ej], eq))
	inv_w = 1. / rest.W if rest.W > 0 else 0.
	return torch.zeros_like(p).index_add(1, rest.ei, term) * (2 * inv_w) * g.to(dtype)[:, None, None]


def margins(D, mirrored):
	"""min over cells of (D_2 - D_3) / D_1 (mirrored) or (D_2 + D_3) / D_1: how far the worst cell is from having no unique rotation."""
	D = D.detach()
	m = (D[..., 1] - D[..., 2]) if mirrored else (D[..., 1] + D[..., 2])
	return float((m / D[..., 0]).min())


# ------------------------------------------------------------------ deformations of the GPU cases
def rotation_matrix(axis, angle):
	a = np.asarray(axis, np.float64)
	a = a / np.linalg.norm(a)
	K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
	return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def deform(q, kind, N, seed=0):
	"""fp32 (N, V, 3) from the fp32 rest vertices q (V, 3).  identity: bitwise q; bend: a rotation, a 3 mm sinusoidal bend and 0.5 mm noise;
	noise: 5 mm; mirror: q diag(1, 1, -1) plus 0.5 mm noise; scale: s q, s = 1.1 ... per mesh; collapsed: one point; line: q projected onto
	the x axis."""
	g = torch.Generator().manual_seed(seed)
	q = q.float()
	qn = q[None].expand(N, -1, -1)
	if kind == 'identity':
		return qn.clone()
	if kind == 'bend':
		out = []
		for n in range(N):
			R = torch.from_numpy(rotation_matrix([1., 0.3 + n, -0.5], 0.4 + 0.3 * n)).float()
			b = q.clone()
			b[:, 2] += 0.003 * torch.sin(q[:, 0] * (25. + n))
			out.append(b @ R.T + torch.tensor([0.01, -0.02, 0.005]))
		return torch.stack(out) + 0.0005 * torch.randn(N, *q.shape, generator=g)
	if kind == 'noise':
		return qn + 0.005 * torch.randn(N, *q.shape, generator=g)
	if kind == 'mirror':
		return qn * torch.tensor([1., 1., -1.]) + 0.0005 * torch.randn(N, *q.shape, generator=g)
	if kind == 'scale':
		return qn * (1.1 + 0.05 * torch.arange(N).float())[:, None, None]
	if kind == 'collapsed':
		return torch.full((N, *q.shape), 0.0125)
	if kind == 'line':
		return qn * torch.tensor([1., 0., 0.])
	raise ValueError(kind)
