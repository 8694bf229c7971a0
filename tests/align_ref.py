"""The alignment rules of include/find_hip.h (find_align_fit, find_icp_run) restated in numpy, in a chosen dtype: float64 for the tests'
reference, float32 to measure what that format can reach on the same inputs.  Umeyama / Kabsch through np.linalg.svd, a brute-force nearest
neighbour (lowest index on ties), the trim rule as stated, the ICP loop with absolute solves.  One cloud at a time, row vectors:
x' = s (x @ R) + t.  Nothing here reads the code under test."""
import numpy as np

MAX_ITERATIONS, DEGENERATE = 1, 2   # status bits
RANK_TOL = 1e-12                    # second singular value <= RANK_TOL * first: rank < 2 (the header's rule)


def umeyama(x, y, w=None, estimate_scale=False, allow_reflection=False, dtype=np.float64):
	"""x, y (P, 3) paired rows, w (P) >= 0 or None -> (R (3, 3), t (3), s, status).  The minimiser of sum w |s (x @ R) + t - y|^2; identity
	and status DEGENERATE for fewer than 3 pairs of positive weight or a cross-covariance of rank < 2."""
	x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
	w = np.ones(len(x), dtype=dtype) if w is None else np.asarray(w, dtype=dtype)
	ident = (np.eye(3, dtype=dtype), np.zeros(3, dtype=dtype), dtype(1), DEGENERATE)
	keep = w > 0
	if keep.sum() < 3:
		return ident
	x, y, w = x[keep], y[keep], w[keep]
	sw = w.sum()
	mx, my = (w[:, None] * x).sum(0) / sw, (w[:, None] * y).sum(0) / sw
	xc, yc = x - mx, y - my
	H = (w[:, None] * xc).T @ yc
	U, D, Vt = np.linalg.svd(H)
	if not D[0] > 0 or not D[1] > RANK_TOL * D[0]:
		return ident
	E = np.ones(3, dtype=dtype)
	if not allow_reflection and np.linalg.det(U) * np.linalg.det(Vt) < 0:
		E[2] = -1
	R = (U * E) @ Vt
	s = dtype(1)
	if estimate_scale:
		var = (w * (xc * xc).sum(1)).sum()
		if not var > 0:
			return ident
		s = (D * E).sum() / var
	t = my - s * (mx @ R)
	return R.astype(dtype), t.astype(dtype), dtype(s), 0


def apply(x, R, t, s):
	return s * (x @ R) + t


def nearest(xt, y, chunk=1024, second=False):
	"""Brute force in the dtype of the inputs: (d2 (P1), idx (P1) the lowest index at the minimum[, the second smallest d2 (P1)])."""
	d2, idx, d2b = np.empty(len(xt), xt.dtype), np.empty(len(xt), np.int64), np.empty(len(xt), xt.dtype)
	for a in range(0, len(xt), chunk):
		q = xt[a:a + chunk]
		d = (q[:, None, 0] - y[None, :, 0]) ** 2
		d += (q[:, None, 1] - y[None, :, 1]) ** 2
		d += (q[:, None, 2] - y[None, :, 2]) ** 2
		j = d.argmin(1)
		idx[a:a + chunk], d2[a:a + chunk] = j, d[np.arange(len(q)), j]
		if second:
			d2b[a:a + chunk] = np.partition(d, 1, axis=1)[:, 1] if y.shape[0] > 1 else np.inf
	return (d2, idx, d2b) if second else (d2, idx)


def keep_count(m, trim):
	return m - int(np.floor(trim * m))


def trim_rule(d2, trim=0., max_dist=None):
	"""(tau, used (m) bool): tau the k-th smallest of the m values d2, k = m - floor(trim m) (+inf for trim == 0); a pair is used iff
	d2 <= tau, and with max_dist also d2 <= max_dist^2."""
	tau = d2.dtype.type(np.inf)
	if trim > 0 and len(d2):
		tau = np.sort(d2)[keep_count(len(d2), trim) - 1]
	used = d2 <= tau
	if max_dist is not None:
		used &= d2 <= d2.dtype.type(max_dist) ** 2
	return tau, used


def icp(x, y, init=None, max_iterations=50, rel_tol=1e-6, estimate_scale=False, trim=0., max_dist=None, dtype=np.float64):
	"""The loop of find_icp_run for one cloud x (P1, 3) -> y (P2, 3); init (R, t, s) or None.  dict(R, t, s, rmse, iterations, status, xt, d2, idx,
	tau, used): what is returned belongs to the returned transform."""
	x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
	R, t, s = (np.eye(3, dtype=dtype), np.zeros(3, dtype=dtype), dtype(1)) if init is None else (np.asarray(init[0], dtype=dtype),
																								   np.asarray(init[1], dtype=dtype), dtype(init[2]))
	prev, frozen, status, iterations = None, False, 0, 0
	for rnd in range(max_iterations + 1):
		xt = apply(x, R, t, s).astype(dtype)
		if len(y):
			d2, idx = nearest(xt, y)
		else:
			d2, idx = np.zeros(len(x), dtype), np.full(len(x), -1)
		tau, used = trim_rule(d2, trim, max_dist)
		used &= idx >= 0
		rmse = dtype(np.sqrt(d2[used].sum() / used.sum())) if used.any() else dtype(0)
		if frozen:
			break   # (nothing changes any more: this round's results are the last round's)
		if rnd > 0 and abs(prev - rmse) <= rel_tol * prev:
			break
		if rnd == max_iterations:
			status |= MAX_ITERATIONS
			break
		prev = rmse
		fit = umeyama(x[used], y[idx[used]], None, estimate_scale, False, dtype)
		if fit[3]:
			frozen, status = True, status | DEGENERATE
			continue
		R, t, s = fit[:3]
		iterations = rnd + 1
	return dict(R=R, t=t, s=s, rmse=rmse, iterations=iterations, status=status, xt=xt, d2=d2, idx=idx, tau=tau, used=used)


def rotation(axis, angle):
	"""Row-vector rotation matrix (3, 3) float64 about `axis` by `angle` radians (Rodrigues)."""
	a = np.asarray(axis, dtype=np.float64)
	a = a / np.linalg.norm(a)
	K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
	return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def rotation_error(R, R0):
	"""The angle (radians) of R^T R0."""
	c = (np.trace(np.asarray(R, np.float64).T @ np.asarray(R0, np.float64)) - 1) / 2
	return float(np.arccos(np.clip(c, -1, 1)))
