"""Reference of the UV atlas raster and of the dilate map (find_amd/csrc/bake.hip) in numpy, in the dtype asked for (float64: the truth;
float32: what the same formulas give in the kernel's precision, operation for operation).  A helper of test_bake_host.py and
test_gpu_bake.py, not a test.

Texel (i, j) of an H x W map has its centre at (u, v) = (j / (W - 1), 1 - i / (H - 1)).  The raster loops over the faces in index order and
lets the first face that holds a centre keep it.  A face is only evaluated on its bounding box grown by two texels: beyond it one of the
barycentrics is below -1 / (the face's extent in texels), far from the tie margins the tests look at (the largest face they use spans
three map widths of at most 512 texels)."""
import numpy as np


def centres(H, W, dtype=np.float64):
	"""(px (W,), py (H,)) of the texel centres."""
	dt = np.dtype(dtype).type
	return np.arange(W, dtype=dtype) / dt(W - 1), dt(1) - np.arange(H, dtype=dtype) / dt(H - 1)


def usable(verts_uvs, faces_uvs):
	"""(F,) bool, the rules' set of faces: indices in range, and a float32 signed area that is neither 0 nor NaN."""
	uv = np.asarray(verts_uvs, dtype=np.float32)
	faces = np.asarray(faces_uvs, dtype=np.int64).reshape(-1, 3)
	ok = ((faces >= 0) & (faces < uv.shape[0])).all(-1)
	t = uv[np.where(ok[:, None], faces, 0)] if uv.shape[0] else np.zeros((len(faces), 3, 2), np.float32)
	with np.errstate(invalid='ignore', over='ignore'):
		area = (t[:, 1, 0] - t[:, 0, 0]) * (t[:, 2, 1] - t[:, 0, 1]) - (t[:, 1, 1] - t[:, 0, 1]) * (t[:, 2, 0] - t[:, 0, 0])
	assert area.dtype == np.float32
	return ok & (area != 0) & ~np.isnan(area)


def raster(verts_uvs, faces_uvs, H, W, dtype=np.float64, strict=None):
	"""verts_uvs (Vt,2) float32 values, faces_uvs (F,3)  ->  face (H,W) int32 (-1: none), bary (H,W,3) in `dtype` (0 where none) and the
	margin m (H,W): the largest over the usable faces of the smallest barycentric of the centre (-inf where no face's box comes near).
	m > 0: strictly inside a face; m = 0: on an edge; m < 0: outside every face.
	strict: a fourth result, (H,W) int32: the smallest face that holds the centre with every barycentric above `strict` (-1: none)."""
	uv32 = np.asarray(verts_uvs, dtype=np.float32)
	uv = uv32.astype(dtype)
	faces = np.asarray(faces_uvs, dtype=np.int64).reshape(-1, 3)
	px, py = centres(H, W, dtype)
	face = np.full((H, W), -1, np.int32)
	clear = np.full((H, W), -1, np.int32)
	bary = np.zeros((H, W, 3), dtype)
	margin = np.full((H, W), -np.inf, np.float64)
	use = usable(uv32, faces)
	# the boxes in texels, grown by two (in float64 whatever the dtype; an infinite or huge UV is clamped)
	with np.errstate(invalid='ignore', over='ignore'):
		t64 = uv32.astype(np.float64)[np.where(use[:, None], faces, 0)] if len(faces) and uv32.shape[0] else np.zeros((len(faces), 3, 2))
		us, vs = t64[..., 0] * (W - 1), (1.0 - t64[..., 1]) * (H - 1)
		J0, J1 = np.clip(np.floor(us.min(-1)) - 2, 0, W).astype(np.int64), np.clip(np.ceil(us.max(-1)) + 2, -1, W - 1).astype(np.int64)
		I0, I1 = np.clip(np.floor(vs.min(-1)) - 2, 0, H).astype(np.int64), np.clip(np.ceil(vs.max(-1)) + 2, -1, H - 1).astype(np.int64)
	for f in np.nonzero(use & (J1 >= J0) & (I1 >= I0))[0]:
		tri = faces[f]
		(x0, y0), (x1, y1), (x2, y2) = uv[tri[0]], uv[tri[1]], uv[tri[2]]
		with np.errstate(invalid='ignore', over='ignore'):
			area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
			if area == 0 or np.isnan(area):
				continue
			box = (slice(I0[f], I1[f] + 1), slice(J0[f], J1[f] + 1))
			X, Y = px[None, box[1]], py[box[0], None]
			w = np.stack(np.broadcast_arrays((x2 - x1) * (Y - y1) - (y2 - y1) * (X - x1),
											 (x0 - x2) * (Y - y2) - (y0 - y2) * (X - x2),
											 (x1 - x0) * (Y - y0) - (y1 - y0) * (X - x0)), -1)
			b = w / area
			inside = (w >= 0).all(-1) if area > 0 else (w <= 0).all(-1)
		mn = np.where(np.isnan(b).any(-1), -np.inf, b.min(-1)).astype(np.float64)
		margin[box] = np.maximum(margin[box], mn)
		new = inside & (face[box] < 0)
		face[box][new] = f
		bary[box][new] = b[new]
		if strict is not None:
			clear[box][(mn > strict) & (clear[box] < 0)] = f
	return (face, bary, margin) if strict is None else (face, bary, margin, clear)


def contains(verts_uvs, tri, px, py):
	"""The smallest float64 barycentric of the points (px, py) in face `tri` (each (n,)): >= 0 means the closed triangle holds the point."""
	uv = np.asarray(verts_uvs, dtype=np.float32).astype(np.float64)
	x0, y0, x1, y1, x2, y2 = (uv[tri[:, k], c] for k in range(3) for c in range(2))
	area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
	w = np.stack([(x2 - x1) * (py - y1) - (y2 - y1) * (px - x1), (x0 - x2) * (py - y2) - (y0 - y2) * (px - x2), (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)], -1)
	return (w / area[:, None]).min(-1)


def dilate(face, pad):
	"""face (H,W)  ->  src (H,W) int32, the rule taken literally: a covered texel (face >= 0) maps to its own flat index i W + j; an
	uncovered one to the covered texel within Chebyshev distance `pad` with the smallest (di^2 + dj^2, flat index), -1 without one."""
	face = np.asarray(face)
	H, W = face.shape
	cov = face >= 0
	flat = np.arange(H * W, dtype=np.int64).reshape(H, W)
	none = np.iinfo(np.int64).max
	best = np.full((H, W), none, np.int64)   # the key (di^2 + dj^2) * H W + flat index of the source
	for di in range(-pad, pad + 1):
		for dj in range(-pad, pad + 1):
			# texels (i, j) whose neighbour (i + di, j + dj) is in the map
			ia, ib = max(0, -di), min(H, H - di)
			ja, jb = max(0, -dj), min(W, W - dj)
			if ia >= ib or ja >= jb:
				continue
			there = cov[ia + di:ib + di, ja + dj:jb + dj]
			key = np.where(there, (di * di + dj * dj) * (H * W) + flat[ia + di:ib + di, ja + dj:jb + dj], none)
			best[ia:ib, ja:jb] = np.minimum(best[ia:ib, ja:jb], key)
	src = np.where(best == none, -1, best % (H * W))
	return np.where(cov, flat, src).astype(np.int32)
