"""Keypoint splats on the GPU: find_points_render against the float64 restatement of tests/test_points_host.py (2 clouds x 3 views at 256^2,
1 / 26 / 5 000 points, points behind the camera, outside the image, on tile borders, crowded pixels, K 1 / 10 / 32), repeatability and
independence of the launch size, FootRenderer(keypoints=..., keypoints_blend=...), find_amd.evaluate.eval_3d end to end for a neural and a
PCA model, and the C-ABI's error codes."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.test_points_host import R_SPLAT, project64, splat64

pytestmark = pytest.mark.gpu

S = 256
TOL_D = 1e-8    # |d^2 - r^2| below this: the kernel's fp32 pixel centres and d^2 and float64 may disagree on the strict test (an edge tie)
TOL_Z = 0.0     # equal fp32 z: the tie rule decides (the projection is the kernel's to the bit, so no other depth tie exists)


def _views(n):
	from find_amd.renderer import FootRenderer
	R, T = FootRenderer(image_size=S, device='cuda').linspace_views(nviews=n, dist=0.3, elev_min=-40, elev_max=50, azim_min=10, azim_max=200)
	return R.float(), T.float()


def _unproject(ndc, R, T, fov_deg=60.0):
	"""(x_ndc, y_ndc, z_view) -> world points of view (R, T) (float64)."""
	s = 1.0 / math.tan(math.radians(fov_deg) / 2)
	v = np.stack([ndc[:, 0] * ndc[:, 2] / s, ndc[:, 1] * ndc[:, 2] / s, ndc[:, 2]], 1)
	return (v - T) @ R.T


def _clouds(P, R, T, seed):
	"""Two clouds: most points in a box around the origin (inside and outside the image), a tenth far out (behind the camera in some
	views), a few on tile borders of view 0 and a crowd of 40 on one pixel of view 0."""
	g = np.random.RandomState(seed)
	R0, T0 = R[0].double().cpu().numpy(), T[0].double().cpu().numpy()
	out = []
	for _ in range(2):
		p = g.uniform(-0.2, 0.2, (P, 3))
		if P >= 26:
			far = g.rand(P) < 0.1
			d = g.normal(size=(P, 3))
			p[far] = 0.6 * d[far] / np.linalg.norm(d[far], axis=1, keepdims=True)
			nb = max(2, P // 50)
			border = 1.0 - 2.0 * 16 * g.randint(1, S // 16, (nb, 2)) / S    # between pixel 16 k - 1 and 16 k
			border[: nb // 2, 1] = g.uniform(-0.9, 0.9, nb // 2)
			p[1:1 + nb] = _unproject(np.concatenate([border, g.uniform(0.2, 0.4, (nb, 1))], 1), R0, T0)
		if P >= 5000:
			c = 1.0 - (2.0 * np.array([100, 77]) + 1.0) / S
			crowd = np.concatenate([c + g.uniform(-0.01, 0.01, (40, 2)), g.uniform(0.2, 0.4, (40, 1))], 1)
			p[-40:] = _unproject(crowd, R0, T0)
		out.append(p)
	return torch.tensor(np.stack(out), dtype=torch.float32)


def _features(N, P, seed):
	return torch.tensor(np.random.RandomState(seed).uniform(0, 1, (N, P, 3)), dtype=torch.float32)


def project32(points, R, T, fov_deg=60.0):
	"""Step 1 as the kernel rounds it: fp32, one rounding per product and sum in the order of points.hip, s = 1 / tanf(...) as the host
	forms it.  (The splat weight 1 - d^2 / r^2 amplifies an NDC error by 2 / r = 67: a float64 projection of fp32 inputs differs from any
	fp32 one by more than the 1e-5 the images are held to, so steps 2-6 of the restatement are fed the projection the kernel computes.)"""
	f32 = np.float32
	libm = ctypes.CDLL('libm.so.6')
	libm.tanf.restype, libm.tanf.argtypes = ctypes.c_float, [ctypes.c_float]
	s = f32(1.0) / f32(libm.tanf(float(f32(f32(f32(fov_deg) * f32(math.pi)) / f32(180.0)) * f32(0.5))))
	p, R, T = np.asarray(points, f32), np.asarray(R, f32), np.asarray(T, f32)
	v = [((p[:, 0] * R[0, c] + p[:, 1] * R[1, c]) + p[:, 2] * R[2, c]) + T[c] for c in range(3)]
	with np.errstate(divide='ignore', invalid='ignore'):
		return np.stack([(s * v[0]) / v[2], (s * v[1]) / v[2], v[2]], 1).astype(np.float64)


def _render(points, features, R, T, H, W, K):
	"""The restatement with the kernel's projection: (image, idx, zbuf, dists), image index n*M + m."""
	outs = [splat64(project32(points[n], R[m], T[m]), features[n], H, W, R_SPLAT, K) for n in range(points.shape[0]) for m in range(R.shape[0])]
	return tuple(np.stack(o) for o in zip(*outs))


def _proj_of_image(points, R, T, img, M):
	n, m = divmod(img, M)
	return project32(points[n].numpy(), R[m].cpu().numpy(), T[m].cpu().numpy())


def _is_tie(ndc, i, j, radius=R_SPLAT):
	"""Pixel (i, j): some point sits on the radius within fp32 rounding, or two candidates' z are within rounding of each other."""
	yc, xc = 1.0 - (2.0 * i + 1.0) / S, 1.0 - (2.0 * j + 1.0) / S
	d2 = (xc - ndc[:, 0]) ** 2 + (yc - ndc[:, 1]) ** 2
	front = ndc[:, 2] >= 0
	if np.any(front & (np.abs(d2 - radius * radius) < TOL_D)):
		return True
	z = np.sort(ndc[front & (d2 < radius * radius + TOL_D), 2])
	return bool(np.any(np.diff(z) <= TOL_Z))


def _composite64(idx, dists, feats, radius=R_SPLAT):
	"""Image of the restatement's fragments (idx, dists (..., K)) with per-image features feats (n_img, P, 3)."""
	hit = idx >= 0
	w = np.where(hit, 1.0 - dists / radius ** 2, 0.0)
	cum = np.cumprod(np.concatenate([np.ones_like(w[..., :1]), 1.0 - w[..., :-1]], -1), -1)
	out = np.zeros(idx.shape[:-1] + (3,))
	for b in range(idx.shape[0]):
		f = feats[b][np.where(hit[b], idx[b], 0)] * hit[b][..., None]
		out[b] = np.sum((cum[b] * w[b])[..., None] * f, axis=-2)
	return out


@pytest.fixture(scope='module')
def scene():
	"""(R, T, {P: (points, features, restatement image / idx / zbuf / dists with K = 32)})"""
	R, T = _views(3)
	data = {}
	for P in (1, 26, 5000):
		pts, f = _clouds(P, R, T, seed=P), _features(2, P, seed=P + 1)
		data[P] = (pts, f) + _render(pts.numpy(), f.numpy(), R.cpu().numpy(), T.cpu().numpy(), S, S, K=32)
	return R, T, data


@pytest.mark.parametrize('K', [1, 10, 32])
@pytest.mark.parametrize('P', [1, 26, 5000])
def test_points_render_matches_float64(scene, P, K):
	from find_amd import functional_render as FR
	R, T, data = scene
	pts, f, _, idx64, zb64, d64 = data[P]
	idx64, zb64, d64 = idx64[..., :K], zb64[..., :K], d64[..., :K]
	M = R.shape[0]
	img, (idx, zb, d) = FR.render_points(pts.cuda(), f.cuda(), R.cuda(), T.cuda(), S, points_per_pixel=K, return_fragments=True)
	assert img.shape == (2, M, S, S, 3) and idx.shape == (2, M, S, S, K) and idx.dtype == torch.int32
	img, idx, zb, d = (t.reshape((2 * M,) + t.shape[2:]).cpu().numpy() for t in (img, idx, zb, d))
	feats = np.repeat(f.double().numpy(), M, axis=0)
	img64 = _composite64(idx64, d64, feats)
	bad = np.argwhere(np.any(idx != idx64, axis=-1))
	for b, i, j in bad:
		assert _is_tie(_proj_of_image(pts, R, T, b, M), i, j), (b, i, j, idx[b, i, j], idx64[b, i, j])
	assert len(bad) <= 2e-4 * idx.shape[0] * S * S, len(bad)
	ok = np.ones(idx.shape[:3], bool)
	ok[tuple(bad.T)] = False
	assert np.abs(zb - zb64)[ok].max() <= 1e-6
	assert np.abs(d - d64)[ok].max() <= 1e-6
	assert np.abs(img - img64)[ok].max() <= 1e-5
	# the cases the clouds were drawn for are there
	assert (idx64[..., 0] >= 0).any()
	if P >= 26:
		ndc = np.concatenate([_proj_of_image(pts, R, T, b, M) for b in range(2 * M)])
		assert (ndc[:, 2] < 0).any() and (np.abs(ndc[:, :2]) > 1.05).any()   # behind the camera, outside the image
	if P == 5000:
		assert (idx64[..., -1] >= 0).any()    # a pixel with K candidates or more (the crowd)


def test_repeats_are_bit_identical_and_launch_size_does_not_matter():
	from find_amd import functional_render as FR
	g = np.random.RandomState(5)
	R, T = torch.eye(3)[None].cuda(), torch.tensor([[0.0, 0.0, 0.3]]).cuda()
	few = g.uniform(-0.15, 0.15, (26, 3))
	many = g.uniform(-0.15, 0.15, (5000, 3))
	many[:, 2] = g.uniform(-0.9, -0.31, 5000)       # view z = world z + 0.3 < 0: behind the camera
	pos = np.sort(g.choice(5000, 26, replace=False))
	many[pos] = few
	f_few = g.uniform(0, 1, (26, 3))
	f_many = g.uniform(0, 1, (5000, 3))
	f_many[pos] = f_few
	t = lambda a: torch.tensor(a[None], dtype=torch.float32).cuda()
	a, (ia, za, da) = FR.render_points(t(few), t(f_few), R, T, S, return_fragments=True)
	b, (ib, zb, db) = FR.render_points(t(few), t(f_few), R, T, S, return_fragments=True)
	c, (ic, zc, dc) = FR.render_points(t(many), t(f_many), R, T, S, return_fragments=True)
	assert (a > 0).any()
	assert torch.equal(a, b) and torch.equal(ia, ib) and torch.equal(za, zb) and torch.equal(da, db)
	assert torch.equal(a, c) and torch.equal(za, zc) and torch.equal(da, dc)
	remap = torch.tensor(np.append(pos, -1), dtype=torch.int32).cuda()   # few's index -> many's index (-1 stays -1)
	assert torch.equal(remap[ia.long()], ic)


# ---------------------------------------------------------------------------------------------- FootRenderer
def _foot_meshes(N, seed=0, grad=False):
	"""N small curved sheets (~ foot-sized) with vertex colours."""
	from find_amd.structures import Meshes, TexturesVertex
	n = 12
	i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
	g = np.random.RandomState(seed)
	verts = []
	for k in range(N):
		x = (i - n / 2) * 0.02 + g.uniform(-0.005, 0.005)
		y = (j - n / 2) * 0.01
		z = 0.02 * np.cos(x * 10) + 0.01 * k
		verts.append(np.stack([x, y, z], -1).reshape(-1, 3))
	faces = []
	for a in range(n - 1):
		for b in range(n - 1):
			v = a * n + b
			faces += [[v, v + n, v + n + 1], [v, v + n + 1, v + 1]]
	V = torch.tensor(np.stack(verts), dtype=torch.float32).cuda()
	col = torch.tensor(g.uniform(0.2, 0.8, (N, n * n, 3)), dtype=torch.float32).cuda().requires_grad_(grad)
	return Meshes(V, torch.tensor(faces, dtype=torch.int64).cuda(), TexturesVertex(col)), col


def _red(kp):
	f = torch.zeros_like(kp)
	f[..., 0] = 1
	return f


def test_footrenderer_keypoints_equal_render_points_and_blend():
	from find_amd import functional_render as FR
	from find_amd.renderer import FootRenderer
	rdr = FootRenderer(image_size=128, device='cuda')
	meshes, _ = _foot_meshes(2)
	kp = meshes.verts_padded()[:, [5, 40, 77, 100, 131]]
	R, T = rdr.view_from('topdown')
	out = rdr(meshes, R, T, keypoints=kp, keypoints_blend=True)
	pcl = FR.render_points(kp, _red(kp), R.cuda().float(), T.cuda().float(), 128, radius=0.03, points_per_pixel=10)
	assert torch.equal(out['keypoints'], pcl)
	m = torch.any(pcl > 0, dim=-1, keepdim=True)
	assert torch.equal(out['keypoints_blend'], ~m * out['image'] + m * pcl)
	assert m.any() and (~m).any()
	# keypoints_blend without keypoints is ignored, as upstream
	plain = rdr(meshes, R, T, keypoints_blend=True)
	assert 'keypoints_blend' not in plain and 'keypoints' not in plain and torch.allclose(plain['image'], out['image'], atol=1e-6)
	# keypoints alone, without any mesh output
	assert torch.equal(rdr(meshes, R, T, return_images=False, keypoints=kp)['keypoints'], pcl)


def test_footrenderer_views_follow_image_index():
	from find_amd import functional_render as FR
	from find_amd.renderer import FootRenderer
	rdr = FootRenderer(image_size=96, device='cuda')
	meshes, _ = _foot_meshes(3, seed=1)
	kp = meshes.verts_padded()[:, ::9]
	# M = 1: equal to one launch per mesh
	R1, T1 = rdr.view_from('topdown')
	one = rdr(meshes, R1, T1, keypoints=kp)['keypoints']
	for n in range(3):
		assert torch.equal(one[n], rdr(meshes[n], R1, T1, keypoints=kp[n:n + 1])['keypoints'][0])
	# M > 1: image n*M + m is mesh n's keypoints in view m
	R, T = rdr.view_from(['topdown', '45', 'side1'])
	many = rdr(meshes, R, T, keypoints=kp)['keypoints']
	assert many.shape == (3, 3, 96, 96, 3)
	for n in range(3):
		for m in range(3):
			want = FR.render_points(kp[n:n + 1], _red(kp[n:n + 1]), R[m:m + 1].cuda().float(), T[m:m + 1].cuda().float(), 96)
			assert torch.equal(many[n, m], want[0, 0]), (n, m)
			assert (many[n, m] > 0).any()


def test_keypoint_on_a_vertex_lands_red_at_its_pixel():
	from find_amd.renderer import FootRenderer
	size = 128
	rdr = FootRenderer(image_size=size, device='cuda')
	meshes, _ = _foot_meshes(1, seed=2)
	v = 70
	kp = meshes.verts_padded()[:, [v]]
	R, T = rdr.view_from('topdown')
	out = rdr(meshes, R, T, keypoints=kp, keypoints_blend=True)
	ndc = project64(kp[0].double().cpu().numpy(), R[0].double().numpy(), T[0].double().numpy())[0]
	j = int(round(((1 - ndc[0]) * size - 1) / 2))
	i = int(round(((1 - ndc[1]) * size - 1) / 2))
	px = out['keypoints_blend'][0, 0, i, j]
	assert px[0] > 0.8 and px[1] == 0 and px[2] == 0, px
	assert not torch.equal(out['image'][0, 0, i, j], px)


def test_blend_keeps_the_image_gradient_where_no_keypoint_lands():
	from find_amd.renderer import FootRenderer
	rdr = FootRenderer(image_size=64, device='cuda')
	meshes, col = _foot_meshes(1, seed=3, grad=True)
	kp = meshes.verts_padded()[:, [20, 90]].detach()
	R, T = rdr.view_from('topdown')
	G = torch.rand(1, 1, 64, 64, 3, device='cuda')
	out = rdr(meshes, R, T, keypoints=kp, keypoints_blend=True)
	(g_blend,) = torch.autograd.grad((out['keypoints_blend'] * G).sum(), col)
	m = torch.any(out['keypoints'] > 0, dim=-1, keepdim=True)
	out2 = rdr(meshes, R, T)
	(g_img,) = torch.autograd.grad((out2['image'] * G * ~m).sum(), col)
	assert g_blend.abs().max() > 0
	assert torch.allclose(g_blend, g_img, rtol=1e-5, atol=1e-7)


def test_gradient_and_argument_errors():
	from find_amd import functional_render as FR
	from find_amd.renderer import FootRenderer
	rdr = FootRenderer(image_size=32, device='cuda')
	meshes, _ = _foot_meshes(2, seed=4)
	R, T = rdr.view_from('topdown')
	kp = meshes.verts_padded()[:, :3].clone().requires_grad_(True)
	with pytest.raises(RuntimeError, match='no backward'):
		rdr(meshes, R, T, keypoints=kp)
	with torch.no_grad():
		assert 'keypoints' in rdr(meshes, R, T, keypoints=kp)
	with pytest.raises(ValueError):
		rdr(meshes, R, T, return_images=False, return_mask=True, keypoints=kp.detach(), keypoints_blend=True)
	with pytest.raises(ValueError):
		rdr(meshes, R, T, keypoints=kp.detach()[:1])
	pts = kp.detach()
	Rc, Tc = R.cuda().float(), T.cuda().float()
	with pytest.raises(RuntimeError, match='points_per_pixel 33'):
		FR.render_points(pts, _red(pts), Rc, Tc, 32, points_per_pixel=33)
	with pytest.raises(RuntimeError, match='radius'):
		FR.render_points(pts, _red(pts), Rc, Tc, 32, radius=0.0)


# ---------------------------------------------------------------------------------------------- eval_3d
def _foot3d_val_kp(tmp_path, missing=None):
	"""Four scans with four keypoints each (`missing`: the index of one without)."""
	from tests.test_host_dataset import CFG_POSE, _write_scan
	from find_amd.dataset import Foot3DDataset
	root = str(tmp_path)
	mesh_dir = os.path.join(root, 'Meshes_sliced')
	data, val = [], []
	for k, fid in enumerate(['0021', '0022', '0023', '0024']):
		rel = f'{fid}/A/{fid}-A'
		n = 7 + k
		_write_scan(mesh_dir, rel + '.obj', rel + '.png', n, (0.0, 0.0, 0.0))
		kps = None if k == missing else [0, n + 1, 2 * n + 3, n * n - 1]
		data.append({'Foot ID': fid, 'Scan ID': 'A', 'footedness': 'Left', 'pose': ['T-Pose'], 'keypoints': kps, 'OBJ file': rel + '.obj',
					 'PNG file': rel + '.png'})
		val.append(fid)
	jpath = os.path.join(root, 'index.json')
	with open(jpath, 'w') as fh:
		json.dump({'keypoint_labels': ['a', 'b', 'c', 'd'], 'data': data}, fh)
	cfg = {'DATASET_FOLDER': root, 'DATASET_JSON': jpath, 'DATASET_NAME': 'Meshes_sliced', 'LOWPOLY_DATASET_NAME': 'x', 'VAL_FEET': val,
		   'TEMPLATE_FEET': [], 'POSE_VECTOR': CFG_POSE}
	return Foot3DDataset(cfg, device='cpu', is_train=False)


def _pca_model(n_val, tmp_path):
	from tests.test_gpu_pca import _write_mat
	from find_amd.model import PCAModel
	z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pca.npz'))
	m = PCAModel.load(_write_mat(z, tmp_path), device='cuda', train_size=1, val_size=n_val)
	g = torch.Generator().manual_seed(8)
	with torch.no_grad():
		m.shapevec_val.data.copy_(torch.randn(n_val, m.shapevec_val.data.shape[1], generator=g).cuda())
		m.reg_val.data[:, 3:6] = torch.randn(n_val, 3, generator=g).cuda() * 0.1
		m.reg_val.data[:, 6:9] = 1.0
	return m


@pytest.mark.parametrize('kind', ['neural', 'pca'])
def test_eval_3d_end_to_end(tmp_path, kind):
	from tests.test_gpu_eval2d import _model
	from find_amd import evaluate
	from find_amd.dataset import BatchCollator
	from find_amd.eval_metrics import eval_3d_metrics
	from find_amd.renderer import FootRenderer
	ds = _foot3d_val_kp(tmp_path)
	N = len(ds)
	model = _model(N) if kind == 'neural' else _pca_model(N, tmp_path)
	kp_idx = [3, 17, 40, 101]   # (a 128-vertex PCA template here: PCA_KEYPOINTS index a full-size one)
	S_ = 2000
	torch.manual_seed(11)
	resN, extraN = evaluate.eval_3d(model, ds, kp_idx, samples=S_, feet_per_call=N, render_correspondences=True, image_size=96, return_per_foot=True)
	torch.manual_seed(11)
	res1, extra1 = evaluate.eval_3d(model, ds, kp_idx, samples=S_, feet_per_call=1, return_per_foot=True)
	assert model.training
	key_cut = 'Chamf z-cutoff 0.07 (μm)'
	assert set(resN) == {'Keypoint (mm)', key_cut, 'Chamf (μm)'} and all(isinstance(v, float) for v in resN.values())
	assert torch.equal(extraN['keypoint_mm'], extra1['keypoint_mm']) and extraN['keypoint_mm'].shape == (N, 4)
	# the hand composition: every foot in one batch, eval_3d_metrics under the same seed
	collate = BatchCollator(device='cuda').collate_batches
	model.eval()
	torch.manual_seed(11)
	with torch.no_grad():
		batch = collate([ds[i] for i in range(N)])
		batch.update({vec.name: vec.data[batch['idx']] for vec in model.latent_vectors_val})
		res = model.get_meshes_from_batch(batch, is_train=False)
		gt_kps = torch.stack([v[k.long()] for v, k in zip(batch['mesh'].verts_list(), batch['kp_idxs'])])
		want = eval_3d_metrics(res['meshes'], batch['mesh'], pred_verts=res['verts'], template_kp_idxs=kp_idx, gt_kps=gt_kps, samples=S_)
		table = torch.norm(res['verts'][:, kp_idx] - gt_kps, dim=-1) * 1e3
	model.train()
	for k, v in want.items():
		assert resN[k] == pytest.approx(float(v), rel=1e-5), k
		assert res1[k] == pytest.approx(float(v), rel=1e-5), k
	assert torch.allclose(extraN['keypoint_mm'], table, rtol=1e-6, atol=1e-6)
	assert resN['Keypoint (mm)'] == pytest.approx(float(table.mean()), rel=1e-5)
	# the correspondence images: the top-down keypoint blends, red splats over the renders
	rdr = FootRenderer(image_size=96, device='cuda')
	R, T = rdr.view_from('topdown')
	for name, meshes, kp in (('gt', batch['mesh'], gt_kps), ('pred', res['meshes'], res['verts'][:, kp_idx].detach())):
		im = extraN[name]
		assert im.shape == (N, 1, 96, 96, 3)
		with torch.no_grad():
			ref = rdr(meshes, R, T, keypoints=kp, keypoints_blend=True)
		assert torch.allclose(im, ref['keypoints_blend'], atol=1e-6), name
		splat = (ref['keypoints'] > 0).any(-1)
		for n in range(N):
			assert splat[n].any(), (name, n)
			assert torch.equal(im[n][splat[n]], ref['keypoints'][n][splat[n]])


def test_eval_3d_refuses_a_foot_without_keypoints(tmp_path):
	from tests.test_gpu_eval2d import _model
	from find_amd import evaluate
	ds = _foot3d_val_kp(tmp_path, missing=2)
	with pytest.raises(ValueError, match='0023'):
		evaluate.eval_3d(_model(len(ds)), ds, [3, 17, 40, 101], samples=500, feet_per_call=2)


# ---------------------------------------------------------------------------------------------- C-ABI
def test_c_abi_error_codes():
	from find_amd import _lib
	L = _lib.lib()
	pts = torch.rand(1, 8, 3, device='cuda') * 0.1
	f = torch.ones(1, 8, 3, device='cuda')
	R, T = torch.eye(3, device='cuda')[None], torch.tensor([[0.0, 0.0, 0.3]], device='cuda')
	img = torch.empty(1, 16, 16, 3, device='cuda')
	P_ = _lib.ptr

	def call(K=10, radius=0.03, points=P_(pts)):
		p = _lib.PointsParams(16, 16, 60.0, radius, K)
		return L.find_points_render(ctypes.byref(p), points, P_(f), P_(R), P_(T), 1, 1, 8, P_(img), None, None, None, _lib.current_stream(pts.device))
	assert call(K=0) == -1 and b'points_per_pixel' in L.find_last_error()
	assert call(K=33) == -1 and b'points_per_pixel' in L.find_last_error()
	assert call(radius=0.0) == -1 and b'radius' in L.find_last_error()
	assert call(radius=-1.0) == -1
	assert call(points=None) == -1 and b'NULL' in L.find_last_error()
	assert call() == 0
	torch.cuda.synchronize()
	assert (img > 0).any()
