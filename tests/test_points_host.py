"""Keypoint splats without a GPU: a float64 restatement of PyTorch3D's point rasteriser + AlphaCompositor as FootRenderer uses them
(find_amd/csrc/points.hip, DESIGN.md 2 [P3D-recall]) checked on hand-computed cases, the argument checks that precede any device work,
the C-ABI's refusals and the kernel's resources in the gfx950 assembly.  tests/test_gpu_points.py holds the HIP kernel against it."""
import ctypes
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_SPLAT = 0.03


# ---------------------------------------------------------------------------------------------- float64 restatement
def project64(points, R, T, fov_deg=60.0):
	"""points (P,3) world, R (3,3), T (3,) row-vector convention -> (P,3) = (s x / z, s y / z, z) with x, y, z in view space."""
	v = np.asarray(points, np.float64) @ np.asarray(R, np.float64) + np.asarray(T, np.float64)
	s = 1.0 / math.tan(math.radians(fov_deg) / 2)
	with np.errstate(divide='ignore', invalid='ignore'):
		return np.stack([s * v[:, 0] / v[:, 2], s * v[:, 1] / v[:, 2], v[:, 2]], axis=1)


def pixel_centres(S):
	return 1.0 - (2.0 * np.arange(S) + 1.0) / S


def splat64(ndc, features, H, W, radius=R_SPLAT, K=10, rows=16):
	"""ndc (P,3) projected points, features (P,3) -> image (H,W,3), idx (H,W,K) int64, zbuf, dists (H,W,K) float64, and d2 (H,W,P) is
	not kept: every pixel's candidates are the points with z >= 0 and d^2 < r^2, sorted by (z, point index), the first K kept;
	w = 1 - d^2 / r^2, out = sum_k c_k w_k f_k with c_0 = 1, c_k+1 = c_k (1 - w_k)."""
	ndc = np.asarray(ndc, np.float64)
	features = np.asarray(features, np.float64)
	P = ndc.shape[0]
	r2 = radius * radius
	xc, yc = pixel_centres(W), pixel_centres(H)
	image = np.zeros((H, W, 3))
	idx = -np.ones((H, W, K), np.int64)
	zbuf = -np.ones((H, W, K))
	dists = -np.ones((H, W, K))
	front = ndc[:, 2] >= 0
	for y0 in range(0, H, rows):
		ys = yc[y0:y0 + rows]
		near = np.nonzero(front & (np.abs(ndc[:, 1] - ys.mean()) <= radius + np.ptp(ys) / 2 + 1e-9))[0]
		if near.size == 0:
			continue
		q = ndc[near]
		dx = xc[None, :, None] - q[None, None, :, 0]
		dy = ys[:, None, None] - q[None, None, :, 1]
		d2 = dx * dx + dy * dy                                   # (rows, W, n)
		key = np.where(d2 < r2, q[None, None, :, 2], np.inf)
		order = np.argsort(key, axis=-1, kind='stable')[..., :K]  # stable: equal z keeps the lower point index first
		kz = np.take_along_axis(key, order, -1)
		kd = np.take_along_axis(d2, order, -1)
		hit = np.isfinite(kz)
		n_k = order.shape[-1]
		sl = slice(y0, y0 + len(ys))
		idx[sl, :, :n_k] = np.where(hit, near[order], -1)
		zbuf[sl, :, :n_k] = np.where(hit, kz, -1.0)
		dists[sl, :, :n_k] = np.where(hit, kd, -1.0)
		w = np.where(hit, 1.0 - kd / r2, 0.0)
		cum = np.cumprod(np.concatenate([np.ones_like(w[..., :1]), 1.0 - w[..., :-1]], -1), -1)
		f = features[near][order] * hit[..., None]
		image[sl] = np.sum((cum * w)[..., None] * f, axis=-2)
	return image, idx, zbuf, dists


def render64(points, features, R, T, H, W, radius=R_SPLAT, K=10, fov_deg=60.0):
	"""Clouds (N,P,3) in views (M,3,3)/(M,3) -> the restatement's (image, idx, zbuf, dists) with image index n*M + m first."""
	points, features, R, T = (np.asarray(a, np.float64) for a in (points, features, R, T))
	outs = [splat64(project64(points[n], R[m], T[m], fov_deg), features[n], H, W, radius, K) for n in range(points.shape[0]) for m in range(R.shape[0])]
	return tuple(np.stack(o) for o in zip(*outs))


RED = np.array([[1.0, 0.0, 0.0]])


def _at_pixel(i, j, S, dx=0.0, dy=0.0, z=0.3):
	return np.array([[pixel_centres(S)[j] + dx, pixel_centres(S)[i] + dy, z]])


def test_point_on_a_pixel_centre_is_pure_red():
	img, idx, zb, d = splat64(_at_pixel(5, 7, 32), RED, 32, 32)
	assert np.array_equal(img[5, 7], [1.0, 0.0, 0.0])
	assert idx[5, 7, 0] == 0 and idx[5, 7, 1] == -1 and zb[5, 7, 0] == 0.3 and d[5, 7, 0] == 0.0
	assert zb[5, 7, 1] == -1 and d[5, 7, 1] == -1


def test_weight_at_a_known_offset():
	off = 0.01
	img, _, _, d = splat64(_at_pixel(5, 7, 32, dx=off), np.array([[0.2, 0.5, 1.0]]), 32, 32)
	w = 1 - off * off / R_SPLAT ** 2
	assert d[5, 7, 0] == pytest.approx(off * off, rel=1e-12)
	assert img[5, 7] == pytest.approx([0.2 * w, 0.5 * w, w], rel=1e-12)
	# a pixel 0.0625 NDC away is outside the radius: nothing there
	assert np.all(img[5, 5] == 0) and np.all(img[5, 9] == 0)


def test_two_stacked_points_composite_front_to_back():
	a = _at_pixel(3, 3, 16, dx=0.005, z=0.4)
	b = _at_pixel(3, 3, 16, dy=0.012, z=0.2)    # nearer: slot 0
	img, idx, zb, d = splat64(np.concatenate([a, b]), np.concatenate([RED, RED]), 16, 16)
	w0, w1 = 1 - 0.012 ** 2 / R_SPLAT ** 2, 1 - 0.005 ** 2 / R_SPLAT ** 2
	assert list(idx[3, 3, :3]) == [1, 0, -1]
	assert list(zb[3, 3, :2]) == [0.2, 0.4]
	assert img[3, 3, 0] == pytest.approx(w0 + (1 - w0) * w1, rel=1e-12)
	assert img[3, 3, 1] == 0 and img[3, 3, 2] == 0


def test_point_behind_the_camera_is_skipped():
	img, idx, _, _ = splat64(_at_pixel(4, 4, 16, z=-0.3), RED, 16, 16)
	assert np.all(img == 0) and np.all(idx == -1)
	# z = 0 is not behind (z < 0 is the rule)
	_, idx0, _, _ = splat64(_at_pixel(4, 4, 16, z=0.0), RED, 16, 16)
	assert idx0[4, 4, 0] == 0


def test_distance_equal_to_the_radius_is_excluded():
	# exactly representable: pixel centre 1 - 1/4 = 0.75 for S = 4, r = 0.25 and a point 0.25 to its side
	S, r = 4, 0.25
	ndc = np.array([[0.75 - r, 0.75, 0.5]])
	img, idx, _, _ = splat64(ndc, RED, S, S, radius=r)
	assert idx[0, 0, 0] == -1 and np.all(img[0, 0] == 0)
	ndc[0, 0] = np.nextafter(0.75 - r, 1.0)
	img, idx, _, _ = splat64(ndc, RED, S, S, radius=r)
	assert idx[0, 0, 0] == 0 and 0 < img[0, 0, 0] < 1e-12


def test_overflow_keeps_the_k_nearest_in_z():
	z = np.array([0.9, 0.3, 0.5, 0.1, 0.7, 0.3, 0.2])
	ndc = np.stack([np.full(7, pixel_centres(8)[2]), np.full(7, pixel_centres(8)[2]), z], 1)
	_, idx, zb, _ = splat64(ndc, np.repeat(RED, 7, 0), 8, 8, K=4)
	assert list(idx[2, 2]) == [3, 6, 1, 5]          # z 0.1, 0.2, then the tie 0.3 in point order
	assert list(zb[2, 2]) == [0.1, 0.2, 0.3, 0.3]
	_, idx, _, _ = splat64(ndc, np.repeat(RED, 7, 0), 8, 8, K=3)
	assert list(idx[2, 2]) == [3, 6, 1]              # the tie at the K-th place goes to the lower index


def test_projection_restatement_is_the_view_transform():
	R = np.eye(3)
	T = np.array([0.0, 0.0, 0.3])
	p = np.array([[0.03, -0.06, 0.0]])
	s = math.sqrt(3.0)
	assert project64(p, R, T)[0] == pytest.approx([s * 0.1, -s * 0.2, 0.3], rel=1e-12)


# ---------------------------------------------------------------------------------------------- argument checks (no device work)
def _cpu_mesh(n=1):
	from find_amd.structures import Meshes, TexturesVertex
	v = torch.tensor([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0], [0.0, 0.01, 0.0]]).expand(n, -1, -1)
	return Meshes(v, torch.tensor([[0, 1, 2]]), TexturesVertex(torch.ones(n, 3, 3)))


def test_keypoints_blend_without_images_raises_value_error():
	from find_amd.renderer import FootRenderer
	r = FootRenderer(image_size=16, device='cpu')
	R, T = r.view_from('topdown')
	with pytest.raises(ValueError, match='return_images'):
		r(_cpu_mesh(), R, T, return_images=False, return_mask=True, keypoints=torch.zeros(1, 2, 3), keypoints_blend=True)


def test_mismatched_keypoint_batch_raises_value_error():
	from find_amd.renderer import FootRenderer
	r = FootRenderer(image_size=16, device='cpu')
	R, T = r.view_from('topdown')
	with pytest.raises(ValueError, match='N = 2'):
		r(_cpu_mesh(2), R, T, keypoints=torch.zeros(3, 2, 3))
	with pytest.raises(ValueError):
		r(_cpu_mesh(2), R, T, keypoints=torch.zeros(2, 3))


def test_renderer_keeps_the_reference_point_settings():
	from find_amd.renderer import FootRenderer
	r = FootRenderer(image_size=16, device='cpu')
	assert (r.points_radius, r.points_per_pixel) == (0.03, 10)


def test_render_points_refuses_cpu_tensors_and_gradients():
	from find_amd import functional_render as FR
	pts, f = torch.zeros(1, 2, 3), torch.zeros(1, 2, 3)
	R, T = torch.eye(3)[None], torch.tensor([[0.0, 0.0, 0.3]])
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		FR.render_points(pts, f, R, T, 16)
	with pytest.raises(RuntimeError, match='no backward'):
		FR.render_points(pts.requires_grad_(True), f, R, T, 16)


def test_c_abi_struct_and_refusals():
	"""Argument validation precedes any launch: the refusals are reachable without a GPU (the pointers are never dereferenced)."""
	from find_amd import _lib
	assert ctypes.sizeof(_lib.PointsParams) == 5 * 4
	L = _lib.lib()
	fake = ctypes.c_void_p(0x1000)

	def call(K=10, radius=0.03, pts=fake, image=fake, n_clouds=1, n_views=1, P=4):
		p = _lib.PointsParams(16, 16, 60.0, radius, K)
		return L.find_points_render(ctypes.byref(p), pts, fake, fake, fake, n_clouds, n_views, P, image, None, None, None, None)
	assert call(K=0) == -1 and b'points_per_pixel 0' in L.find_last_error()
	assert call(K=33) == -1 and b'points_per_pixel 33' in L.find_last_error()
	assert call(radius=0.0) == -1 and b'radius' in L.find_last_error()
	assert call(radius=-0.03) == -1 and b'radius' in L.find_last_error()
	assert call(pts=None) == -1 and b'NULL' in L.find_last_error()
	assert call(image=None) == -1 and b'no output' in L.find_last_error()
	assert call(n_views=0) == -1 and b'bad sizes' in L.find_last_error()


def test_kernel_has_no_scratch_no_spills_and_fits_256_registers():
	"""The K-buffer is indexed statically only: the gfx950 code object of both instantiations (KMAX 16, 32) has no private segment."""
	hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
	if not os.path.exists(hipcc):
		pytest.skip('hipcc not available')
	csrc = os.path.join(ROOT, 'find_amd', 'csrc')
	with tempfile.TemporaryDirectory() as d:
		out = os.path.join(d, 'points.s')
		r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I' + os.path.join(ROOT, 'include'), '-I' + csrc, '-S',
							'--cuda-device-only', os.path.join(csrc, 'points.hip'), '-o', out], capture_output=True, text=True)
		assert r.returncode == 0, r.stderr[-2000:]
		asm = open(out).read()
	kernels = re.findall(r'\.amdhsa_kernel\s+(\S+)', asm)
	assert len(kernels) == 2 and all('points_render_kernel' in k for k in kernels), kernels
	assert [int(v) for v in re.findall(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', asm)] == [0, 0]
	assert all(int(v) <= 256 for v in re.findall(r'\.amdhsa_next_free_vgpr\s+(\d+)', asm))
	assert [int(v) for v in re.findall(r'\.vgpr_spill_count:\s+(\d+)', asm)] == [0, 0]
	assert [int(v) for v in re.findall(r'\.sgpr_spill_count:\s+(\d+)', asm)] == [0, 0]
