"""A numpy restatement of the ray / triangle pair test as include/find_hip.h defines it (find_ray_fwd; csrc/raycast_math.h), parametrised by
dtype and in the same operation order, so its float32 flavour is the kernel's twin.  A helper of test_rays_host.py and test_gpu_rays.py, not a
test.

Per ray: kz = argmax |d| (the first of equals), kx, ky the next two axes in cyclic order, swapped if d[kz] < 0; e1 = axis(kx) - (d[kx] / d[kz])
axis(kz), e2 = axis(ky) - (d[ky] / d[kz]) axis(kz); dd = (d0 d0 + d1 d1) + d2 d2.  Per VERTEX (one value per (ray, vertex), whichever face
uses it): P = p - o, x = (P0 e1_0 + P1 e1_1) + P2 e1_2, y with e2, z = (P0 d0 + P1 d1) + P2 d2.  Per pair: U = cx by - cy bx, V = ax cy - ay cx,
W = bx ay - by ax, det = (U + V) + W; inside: all three >= 0 or all three <= 0, and det != 0; t = ((U za + V zb) + W zc) / (det dd); barycentrics
(U, V, W) / det; a hit: t_min < t <= t_max and t finite.  Never a hit: a -1 row, an index outside [0, V), a corner at the origin (P == 0), the
ray's skip face, a ray with a non-finite component or d == 0.  Ties in t: the smallest face.

naive=True is the negative control: the inside test by three scalar triple products U = d . (C x B), V = d . (A x C), W = d . (B x A) (the
Pluecker / Moeller-Trumbore family), the rest unchanged.  In float32 it leaks on rays aimed at vertices."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np


def frames(d, dtype):
	"""(e1, e2, dd) of directions d (R, 3), in dtype."""
	d = d.astype(dtype)
	n = np.arange(len(d))
	kz = np.abs(d).argmax(1)
	kx = (kz + 1) % 3
	ky = (kx + 1) % 3
	swap = d[n, kz] < 0
	kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
	e1, e2 = np.zeros((len(d), 3), dtype), np.zeros((len(d), 3), dtype)
	with np.errstate(all='ignore'):
		e1[n, kx], e1[n, kz] = 1, -(d[n, kx] / d[n, kz])
		e2[n, ky], e2[n, kz] = 1, -(d[n, ky] / d[n, kz])
		return e1, e2, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def dot(P, e):
	return (P[..., 0] * e[..., 0] + P[..., 1] * e[..., 1]) + P[..., 2] * e[..., 2]


def cross(A, B):
	return np.stack([A[..., 1] * B[..., 2] - A[..., 2] * B[..., 1], A[..., 2] * B[..., 0] - A[..., 0] * B[..., 2], A[..., 0] * B[..., 1] - A[..., 1] * B[..., 0]], -1)


def valid_faces(faces, n_verts):
	faces = np.asarray(faces)
	return ((faces >= 0) & (faces < n_verts)).all(-1)


def cast(origins, dirs, verts, faces, dtype=np.float64, skip=None, t_min=0., t_max=np.inf, naive=False, chunk=128, threads=8):
	"""The closest hit of rays origins, dirs (R, 3) on the mesh verts (V, 3), faces (F, 3) (integer; -1 rows and out-of-range rows never hit):
	(t (R,) in dtype, +inf for a miss; idx (R,) int64, -1 for a miss; bary (R, 3) in dtype, 0 for a miss).  `chunk` rays at a time, the
	chunks on `threads` threads (each writes rows of its own)."""
	dtype = np.dtype(dtype).type
	o, d, v = np.asarray(origins).astype(dtype), np.asarray(dirs).astype(dtype), np.asarray(verts).astype(dtype)
	faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
	R, F = len(o), len(faces)
	T, I, B = np.full(R, np.inf, dtype), np.full(R, -1, np.int64), np.zeros((R, 3), dtype)
	if R == 0 or F == 0 or len(v) == 0:
		return T, I, B
	ok = valid_faces(faces, len(v))
	f = np.where(ok[:, None], faces, 0)
	live = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
	e1, e2, dd = frames(d, dtype)
	t_min, t_max = dtype(t_min), dtype(t_max)

	def part(s):
		with np.errstate(all='ignore'):
			c = slice(s, s + chunk)
			r = np.arange(len(o[c]))
			P = v[None] - o[c, None]   # (r, V, 3): one value per (ray, vertex)
			z = dot(P, d[c, None])
			at_origin = (P == 0).all(-1)
			if naive:
				A, Bc, C = P[:, f[:, 0]], P[:, f[:, 1]], P[:, f[:, 2]]
				dc = d[c, None]
				U, Vv, W = dot(dc, cross(C, Bc)), dot(dc, cross(A, C)), dot(dc, cross(Bc, A))
			else:
				x, y = dot(P, e1[c, None]), dot(P, e2[c, None])
				ax, ay, bx, by, cx, cy = x[:, f[:, 0]], y[:, f[:, 0]], x[:, f[:, 1]], y[:, f[:, 1]], x[:, f[:, 2]], y[:, f[:, 2]]
				U, Vv, W = cx * by - cy * bx, ax * cy - ay * cx, bx * ay - by * ax
			det = (U + Vv) + W
			inside = (((U >= 0) & (Vv >= 0) & (W >= 0)) | ((U <= 0) & (Vv <= 0) & (W <= 0))) & (det != 0)
			t = ((U * z[:, f[:, 0]] + Vv * z[:, f[:, 1]]) + W * z[:, f[:, 2]]) / (det * dd[c, None])
			assert t.dtype == dtype
			hit = inside & (t > t_min) & (t <= t_max) & np.isfinite(t) & ok[None] & live[c, None]
			hit &= ~(at_origin[:, f[:, 0]] | at_origin[:, f[:, 1]] | at_origin[:, f[:, 2]])
			if skip is not None:
				hit &= np.arange(F)[None] != np.asarray(skip)[c, None]
			t = np.where(hit, t, dtype(np.inf))
			j = t.argmin(1)   # (the first of equals: the smallest face)
			T[c] = t[r, j]
			found = np.isfinite(T[c])
			I[c] = np.where(found, j, -1)
			B[c] = np.where(found[:, None], np.stack([U[r, j], Vv[r, j], W[r, j]], -1) / det[r, j, None], dtype(0))
	starts = range(0, R, chunk)
	if len(starts) > 1 and threads > 1:
		with ThreadPoolExecutor(max_workers=threads) as ex:
			list(ex.map(part, starts))
	else:
		for s in starts:
			part(s)
	return T, I, B


def aimed_rays(verts, faces, every=7):
	"""The watertightness inputs: from the float32 vertex mean at every vertex and at every `every`-th edge midpoint (the unique edges, sorted).
	Returns (origins, dirs) float32 with d = fl(target - o): the corner at the target equals d bit for bit."""
	v = np.asarray(verts, np.float32)
	f = np.asarray(faces)
	c = v.mean(0).astype(np.float32)
	e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
	mid = ((v[e[:, 0]] + v[e[:, 1]]) * np.float32(0.5))[::every]
	targets = np.concatenate([v, mid])
	o = np.broadcast_to(c, targets.shape).copy()
	return o, targets - o


def box_rays(verts, n, pad, seed):
	"""n rays from a point uniform in the box of verts grown by pad, aimed at a second such point: (origins, dirs) float32."""
	rng = np.random.RandomState(seed)
	lo, hi = verts.min(0) - pad, verts.max(0) + pad
	o = (lo + rng.rand(n, 3) * (hi - lo)).astype(np.float32)
	return o, (lo + rng.rand(n, 3) * (hi - lo)).astype(np.float32) - o


def visibility(verts, faces, centre, dtype=np.float64):
	"""The rule of find_amd.rays.vertex_visibility for one camera centre: bool (V,)."""
	v = np.asarray(verts, np.float32)
	o = np.broadcast_to(np.asarray(centre, np.float32), v.shape).copy()
	_, idx, _ = cast(o, v - o, v, faces, dtype)
	f = np.asarray(faces)
	return (idx < 0) | (f[np.maximum(idx, 0)] == np.arange(len(v))[:, None]).any(1)
