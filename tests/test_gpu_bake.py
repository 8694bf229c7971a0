"""find_amd.bake on the GPU: the atlas raster against the float64 reference of tests/bake_ref.py (coverage and winners outside the texels
whose centre lies within 1e-5 of an edge, values by the bound of DESIGN 7.4), the dilate map bit for bit, a bake of an affine field read back
through uv_sample, the colour head of a model baked in one and in several chunks, the callers (FootRenderer, vis.turntable, eval_3d) and
the poisoned allocations of the module.

Measured on an MI355X (-s prints one line per raster case): see DESIGN 7.7."""
import contextlib
import math
import os

import numpy as np
import pytest
import torch

import bake_ref
import poison
from find_amd import synthetic

pytestmark = pytest.mark.gpu

FREE = 1e-5            # a texel whose float64 margin is within this of 0 may fall either way
MAX_FREE = 0.01        # share of a case's texels that may
C_ERR, A_ERR = 4.0, 1e-7   # e_hip <= C_ERR * e_fp32 + A_ERR * scale

QUAD_UV = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
QUAD_FACES = np.array([[0, 1, 2], [0, 2, 3]])
TRIANGLE_UV = np.array([[0.13, 0.21], [0.91, 0.33], [0.37, 0.87]], np.float32)


# ------------------------------------------------------------------------------------------------ cases
def _atlas(n_faces):
	vu, fu = synthetic.face_atlas(n_faces)
	return vu.numpy(), fu.numpy()


def latlong_atlas(rings, segs):
	"""A lat-long chart of synthetic.ellipsoid_mesh(rings, segs), face for face: u along the segments with the seam column duplicated
	(Vt = rings (segs + 1) + 2 segs > V), v along the rings, a pole vertex per pole triangle; scaled into the map's inside and shifted by an
	irrational offset so that no chart edge runs along a row or column of texel centres."""
	def g(r, s):
		return r * (segs + 1) + s
	top, bot = rings * (segs + 1), rings * (segs + 1) + segs
	uv = [[s / segs, 1 - (r + 1) / (rings + 1)] for r in range(rings) for s in range(segs + 1)]
	uv += [[(s + 0.5) / segs, 1.0] for s in range(segs)] + [[(s + 0.5) / segs, 0.0] for s in range(segs)]
	faces = []
	for s in range(segs):
		faces.append([top + s, g(0, s), g(0, s + 1)])
		faces.append([bot + s, g(rings - 1, s + 1), g(rings - 1, s)])
	for r in range(rings - 1):
		for s in range(segs):
			a, b, c, d = g(r, s), g(r + 1, s), g(r + 1, s + 1), g(r, s + 1)
			faces += [[a, b, c], [a, c, d]]
	uv = 0.04 + 0.9 * np.asarray(uv) + np.array([math.sqrt(2) - 1, math.sqrt(3) - 1]) * 0.01
	return uv.astype(np.float32), np.asarray(faces)


def rules_case():
	"""Every row the rules name, each contributing what they say: faces 0 - 4 nothing, 5 and 6 overlap (5 wins), 7 covers the rest."""
	uv = np.array([[0.2, 0.2], [0.8, 0.25], [0.3, 0.8],            # 0 - 2: face 5
				   [0.4, 0.1], [0.9, 0.7], [0.35, 0.6],            # 3 - 5: face 6, overlapping face 5
				   [np.nan, 0.5],                                  # 6
				   [1.5, 1.5], [2.5, 1.5], [1.5, 2.5],             # 7 - 9: wholly outside
				   [-1.0, -1.0], [3.1, -1.0], [-1.0, 3.1]], np.float32)   # 10 - 12: larger than the whole map
	faces = np.array([[-1, -1, -1], [0, 1, 13], [0, 1, 1], [0, 1, 6], [7, 8, 9], [0, 1, 2], [3, 4, 5], [10, 11, 12]])
	return uv, faces


def _ellipsoid_atlas():
	v, f = synthetic.ellipsoid_mesh(12, 16)
	uv, fu = latlong_atlas(12, 16)
	assert fu.shape == tuple(f.shape) and uv.shape[0] > v.shape[0]
	return uv, fu


RASTER_CASES = {
	'quad-9x9': lambda: (QUAD_UV, QUAD_FACES, (9, 9)),
	'triangle-5x7': lambda: (TRIANGLE_UV, np.array([[0, 1, 2]]), (5, 7)),
	'triangle-64x48': lambda: (TRIANGLE_UV, np.array([[0, 2, 1]]), (64, 48)),   # (clockwise)
	'atlas384-64x48': lambda: _atlas(384) + ((64, 48),),
	'atlas384-257x255': lambda: _atlas(384) + ((257, 255),),
	'atlas13776-512x512': lambda: _atlas(13776) + ((512, 512),),
	'latlong-96x64': lambda: _ellipsoid_atlas() + ((96, 64),),
	'rules-40x56': lambda: rules_case() + ((40, 56),),
	'no-faces-17x9': lambda: (TRIANGLE_UV, np.zeros((0, 3), np.int64), (17, 9)),
}
_REF = {}


def reference(name):
	"""The case and its float64 / float32 / strict float64 references, computed once."""
	if name not in _REF:
		vu, fu, (H, W) = RASTER_CASES[name]()
		f64 = bake_ref.raster(vu, fu, H, W, np.float64, strict=FREE)
		_REF[name] = dict(vu=vu, fu=fu, size=(H, W), f64=f64[:3], strict=f64[3], f32=bake_ref.raster(vu, fu, H, W, np.float32))
	return _REF[name]


def value_errors(vu, fu, face, bary, size, keep):
	"""(|sum b - 1|, |sum b uv - centre|, max(0, -min b)), each the largest over the texels `keep` that `face` covers, in float64."""
	H, W = size
	sel = keep & (face >= 0)
	if not sel.any():
		return 0.0, 0.0, 0.0
	px, py = bake_ref.centres(H, W)
	cx, cy = np.broadcast_to(px[None, :], (H, W))[sel], np.broadcast_to(py[:, None], (H, W))[sel]
	b = bary[sel].astype(np.float64)
	corners = vu.astype(np.float64)[fu[face[sel]]]             # (n, 3, 2)
	at = (b[..., None] * corners).sum(1)
	return (float(np.abs(b.sum(-1) - 1).max()), float(max(np.abs(at[:, 0] - cx).max(), np.abs(at[:, 1] - cy).max())), float(np.maximum(0, -b.min(-1)).max()))


def _raster(vu, fu, size):
	from find_amd import bake
	face, bary = bake.uv_raster(torch.from_numpy(vu).cuda(), torch.from_numpy(fu).cuda(), size)
	return face, bary


# ------------------------------------------------------------------------------------------------ 1. raster
@pytest.mark.parametrize('name', list(RASTER_CASES))
def test_raster_against_float64(name):
	ref = reference(name)
	vu, fu, (H, W) = ref['vu'], ref['fu'], ref['size']
	face64, _, m = ref['f64']
	face32, bary32, _ = ref['f32']
	face_d, bary_d = _raster(vu, fu, (H, W))
	again = _raster(vu, fu, (H, W))
	assert face_d.shape == (H, W) and face_d.dtype == torch.int32 and bary_d.shape == (H, W, 3) and bary_d.dtype == torch.float32
	assert torch.equal(face_d, again[0]) and torch.equal(bary_d, again[1])   # bit-identical from run to run
	face, bary = face_d.cpu().numpy(), bary_d.cpu().numpy()
	free = np.abs(m) < FREE
	keep = ~free
	assert np.isfinite(bary).all() and ((face >= -1) & (face < max(len(fu), 1))).all()
	assert not bary[face < 0].any()
	if name == 'quad-9x9':   # every product exact: no texel is left to rounding
		assert np.array_equal(face, face64) and np.array_equal(bary, ref['f64'][1].astype(np.float32))
		keep = np.ones_like(free)
	else:
		assert free.mean() <= MAX_FREE, free.mean()
	if name == 'no-faces-17x9':
		assert (face == -1).all() and not bary.any()
		return
	# coverage is float64's; the winner holds the centre in float64, and no earlier face holds it by more than the margin
	assert np.array_equal((face >= 0)[keep], (face64 >= 0)[keep])
	sel = keep & (face >= 0)
	px, py = bake_ref.centres(H, W)
	cx, cy = np.broadcast_to(px[None, :], (H, W))[sel], np.broadcast_to(py[:, None], (H, W))[sel]
	assert (bake_ref.contains(vu, fu[face[sel]], cx, cy) >= 0).all()
	strict = ref['strict']
	assert (face[sel & (strict >= 0)] <= strict[sel & (strict >= 0)]).all()
	# values
	e_hip, e_32 = value_errors(vu, fu, face, bary, (H, W), keep), value_errors(vu, fu, face32, bary32, (H, W), keep)
	bounds = [C_ERR * e + A_ERR for e in e_32]
	print(f'\n[bake] {name}: {int((face >= 0).sum())} of {H * W} texels covered, {int(free.sum())} free, {int((face != face64)[sel].sum())} other winners; '
		  + '; '.join(f'{k} e_hip {a:.2e} e_fp32 {b:.2e} bound {c:.2e}' for k, a, b, c in zip(('sum', 'uv', 'neg'), e_hip, e_32, bounds)))
	for k, a, c in zip(('sum', 'uv', 'neg'), e_hip, bounds):
		assert a <= c, (k, a, c)
	if name == 'rules-40x56':   # what each row contributes
		assert set(np.unique(face)) == {5, 6, 7} and (face == 7).sum() > H * W / 2


# ------------------------------------------------------------------------------------------------ 2. dilate map
@pytest.fixture(scope='module')
def face_maps():
	maps = {k: _raster(*(reference(k)[x] for x in ('vu', 'fu', 'size')))[0] for k in ('atlas384-64x48', 'triangle-5x7', 'triangle-64x48', 'atlas384-257x255')}
	maps['uncovered-33x21'] = torch.full((33, 21), -1, dtype=torch.int32, device='cuda')
	return maps


@pytest.mark.parametrize('pad', [0, 1, 4, 16])
@pytest.mark.parametrize('which', ['atlas384-64x48', 'triangle-5x7', 'triangle-64x48', 'atlas384-257x255', 'uncovered-33x21'])
def test_dilate_map_is_exact(face_maps, which, pad):
	from find_amd import bake
	face = face_maps[which]
	src = bake.dilate_map(face, pad)
	assert src.dtype == torch.int32 and src.shape == face.shape
	want = bake_ref.dilate(face.cpu().numpy(), pad)
	assert np.array_equal(src.cpu().numpy(), want)
	if which == 'uncovered-33x21':
		assert (src == -1).all()
	elif pad > 0:
		assert ((src >= 0) & (face < 0)).any()


# ------------------------------------------------------------------------------------------------ 3. a bake is exact on an affine field
# (u, v) = UV_C + UV_M @ (x, y); the offset keeps every texel centre of the 64 x 64 map at least 4e-4 (in barycentrics) from an edge
UV_C, UV_M = np.array([0.5 + 3 / 1024, 0.5 + 5 / 1024]), np.array([[8.0, 2.0], [-2.0, 8.0]])


def _flat_grid():
	"""A 6 x 6 grid in the plane z = 0.01, its UVs an affine image of (x, y) inside [0.1, 0.9]^2.  x and y are multiples of 1 / 128, so the
	UVs (multiples of 1 / 1024) are exact in float32: the map of an affine field is one affine function of (u, v) across all faces."""
	k = (np.arange(6) - 2.5) / 64
	x, y = np.meshgrid(k, k, indexing='xy')
	verts = np.stack([x, y, np.full_like(x, 0.01)], -1).reshape(-1, 3).astype(np.float32)
	faces = []
	for r in range(5):
		for c in range(5):
			a, b, cc, d = r * 6 + c, r * 6 + c + 1, (r + 1) * 6 + c + 1, (r + 1) * 6 + c
			faces += [[a, b, cc], [a, cc, d]]
	uv64 = UV_C + verts.astype(np.float64)[:, :2] @ UV_M.T
	uv = uv64.astype(np.float32)
	assert uv.min() >= 0.1 and uv.max() <= 0.9 and np.array_equal(uv.astype(np.float64), uv64)
	return verts, np.asarray(faces), uv


def _bilinear(maps, u, v, dtype):
	"""uv_sample's read in numpy: maps (H,W,C) at (u, v), align_corners=True on the flipped map, border padding."""
	H, W, _ = maps.shape
	dt = np.dtype(dtype).type
	x, y = u.astype(dtype) * dt(W - 1), (dt(1) - v.astype(dtype)) * dt(H - 1)
	x, y = np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)
	j0, i0 = np.minimum(np.floor(x).astype(np.int64), W - 2), np.minimum(np.floor(y).astype(np.int64), H - 2)
	fx, fy = (x - j0.astype(dtype))[:, None], (y - i0.astype(dtype))[:, None]
	m = maps.astype(dtype)
	top = m[i0, j0] * (dt(1) - fx) + m[i0, j0 + 1] * fx
	low = m[i0 + 1, j0] * (dt(1) - fx) + m[i0 + 1, j0 + 1] * fx
	return top * (dt(1) - fy) + low * fy, (i0, j0)


@pytest.mark.parametrize('C', [3, 5])
def test_bake_reproduces_an_affine_field(C):
	from find_amd import bake
	from find_amd import functional_render as FR
	verts, faces, uv = _flat_grid()
	H = W = 64
	rng = np.random.RandomState(C)
	A, b0 = rng.randn(3, C) * 10, rng.randn(C)
	A32, b32 = A.astype(np.float32), b0.astype(np.float32)
	A, b0 = A32.astype(np.float64), b32.astype(np.float64)
	At, bt = torch.from_numpy(A32).cuda(), torch.from_numpy(b32).cuda()
	vd, fd, ud = torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda(), torch.from_numpy(uv).cuda()
	plan = bake.plan(ud, fd, (H, W), pad=2)
	maps = bake.bake(lambda pos: pos @ At + bt, plan, vd[None], fd, texels_per_call=700)
	assert maps.shape == (1, H, W, C)
	# the references: the same bake in numpy, float64 and float32
	face64, bary64, m = bake_ref.raster(uv, faces, H, W, np.float64)
	face32, bary32, _ = bake_ref.raster(uv, faces, H, W, np.float32)
	assert not (np.abs(m) < FREE).any()
	assert np.array_equal(plan.face.cpu().numpy() >= 0, face64 >= 0)

	def ref_maps(face, bary, dtype):
		pts = (bary[..., None] * verts.astype(dtype)[faces[np.maximum(face, 0)]]).sum(-2)
		return pts @ A.astype(dtype) + b0.astype(dtype)
	# 500 surface points, given as (face, barycentrics); the point uv_sample reads is the one with the UV sum_k w_k uv_k
	fi = rng.randint(0, len(faces), 500)
	w = rng.dirichlet(np.ones(3), 500).astype(np.float32)
	corners = uv[faces[fi]]                                                       # (500, 3, 2) float32
	at = (w.astype(np.float64)[..., None] * corners.astype(np.float64)).sum(1)
	at32 = (w[..., None] * corners).sum(1)
	assert at32.dtype == np.float32
	pos = np.concatenate([(at - UV_C) @ np.linalg.inv(UV_M).T, np.full((500, 1), float(verts[0, 2]))], -1)
	truth = pos @ A + b0
	scale = float(np.abs(truth).max())
	read64, (i0, j0) = _bilinear(ref_maps(face64, bary64, np.float64), at[:, 0], at[:, 1], np.float64)
	cov = face64 >= 0
	ok = cov[i0, j0] & cov[i0, j0 + 1] & cov[i0 + 1, j0] & cov[i0 + 1, j0 + 1]
	assert ok.sum() > 300
	read32, _ = _bilinear(ref_maps(face32, bary32, np.float32), at32[:, 0], at32[:, 1], np.float32)
	assert np.abs(read64 - truth)[ok].max() <= 1e-12 * scale   # bilinear reads reproduce an affine function
	e32 = float(np.abs(read32.astype(np.float64) - truth)[ok].max())
	fi_d, w_d = torch.from_numpy(fi.astype(np.int32)).cuda()[None], torch.from_numpy(w).cuda()[None]

	def read(c):   # (uv_sample reads three channels)
		return FR.uv_sample(maps[..., c:c + 3].contiguous(), ud[None], fd[None], fi_d, w_d)[0]
	got = read(0) if C == 3 else torch.cat([read(0), read(C - 3)[:, 6 - C:]], -1)
	assert got.shape == (500, C)
	e_hip = float(np.abs(got.cpu().numpy().astype(np.float64) - truth)[ok].max())
	bound = C_ERR * e32 + A_ERR * scale
	print(f'\n[bake] affine field C = {C}: {int(ok.sum())} of 500 samples on covered texels, e_hip {e_hip:.2e}, e_fp32 {e32:.2e}, bound {bound:.2e}, scale {scale:.2f}')
	assert e_hip <= bound, (e_hip, e32, bound)
	# the rest of the map: the gutter copies its source, what is farther is `fill`
	flat = maps.reshape(H * W, C)
	T = plan.idx.numel()
	src = torch.from_numpy(bake_ref.dilate(plan.face.cpu().numpy(), 2).reshape(-1)).cuda().long()
	unc = (plan.face.reshape(-1) < 0)
	near, far = unc & (src >= 0), unc & (src < 0)
	assert near.any() and far.any()
	assert torch.equal(plan.lookup[far], torch.full_like(plan.lookup[far], T)) and (flat[far] == 1.0).all()
	assert torch.equal(plan.idx[plan.lookup[near]], src[near]) and torch.equal(flat[near], flat[src[near]])
	assert torch.equal(plan.idx[plan.lookup[~unc]], torch.arange(H * W, device='cuda')[~unc])


# ------------------------------------------------------------------------------------------------ 4. the model's colour head
@pytest.fixture(scope='module')
def model_bake():
	from find_amd import bake
	model = synthetic.make_model(n_verts=1002, train_size=3, val_size=1, device='cuda')
	lat = synthetic.latents(3, seed=3, device='cuda')
	F = model.template_faces.shape[1]
	vu, fu = synthetic.face_atlas(F)
	vu, fu = vu.cuda(), fu.cuda()
	plan = bake.plan(vu, fu, 128, pad=4)
	return model, lat, vu, fu, plan


def test_bake_colours_is_the_colour_head(model_bake):
	import test_gpu_mlp_f64 as M64
	from oracle import mlp_ref
	from find_amd import bake
	from find_amd.structures import TexturesUV
	model, lat, vu, fu, plan = model_bake
	T = plan.idx.numel()
	assert T > 3000
	with torch.no_grad():
		pos = plan.points(model.template_verts.data, model.template_faces.data[0])
		assert pos.shape == (1, T, 3)
		direct = model(pos, texvec=lat['texvec'], want=('col',))['col']
	# the float64 yardstick of tests/test_gpu_mlp_f64.py at these positions: its tie margin and its bound for the colour output
	sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
	B = model.encoder[0]._B.detach().cpu()
	cpu = {k: v.cpu() for k, v in lat.items()}
	margin = mlp_ref.model_margins(sd, B, pos.cpu(), cpu['shapevec'], cpu['texvec'], cpu['posevec'])
	keep = margin >= M64.KAPPA
	assert 1.0 - keep.double().mean().item() <= M64.MAX_EXCLUDED
	o64 = mlp_ref.model_eval(sd, B, pos.cpu(), cpu['shapevec'], cpu['texvec'], cpu['posevec'], dtype=torch.float64)['col']
	o32 = mlp_ref.model_eval(sd, B, pos.cpu(), cpu['shapevec'], cpu['texvec'], cpu['posevec'], dtype=torch.float32)['col']
	bound = M64._bound('output.col', (o32.double() - o64)[keep].abs().max().item())
	assert (direct.cpu().double() - o64)[keep].abs().max().item() <= bound
	for tpc in (T, 1000):
		tex = bake.bake_colours(model, plan, shapevec=lat['shapevec'], texvec=lat['texvec'], posevec=lat['posevec'], texels_per_call=tpc)
		assert isinstance(tex, TexturesUV) and tex.maps_padded().shape == (3, 128, 128, 3) and tex.faces_uvs_padded().shape == (3,) + tuple(fu.shape)
		baked = tex.maps_padded().reshape(3, -1, 3)[:, plan.idx]
		err = (baked.cpu().double() - direct.cpu().double())[keep].abs().max().item()
		print(f'\n[bake] colour head, {tpc} texels per call of {T}: |baked - one call| {err:.2e}, bound {bound:.2e}')
		assert err <= bound, (tpc, err, bound)
		assert (baked.cpu().double() - o64)[keep].abs().max().item() <= bound


def _batch(lat):
	return {f'{k}_val': v for k, v in lat.items()}


def test_textured_meshes_render_and_spin(model_bake):
	from find_amd import bake, vis
	from find_amd.renderer import FootRenderer
	from find_amd.structures import TexturesUV
	model, lat, vu, fu, plan = model_bake
	batch = _batch(lat)
	textured = bake.textured_meshes(model, plan, vu, fu, batch, is_train=False)
	with torch.no_grad():
		plain = model.get_meshes_from_batch(batch, is_train=False)['meshes']
	assert len(textured) == 3 and isinstance(textured.textures, TexturesUV) and torch.equal(textured.verts_padded(), plain.verts_padded())
	renderer = FootRenderer(64, device='cuda')
	R, T = renderer.linspace_views(nviews=2, dist=0.3, elev_min=-60, elev_max=60)
	with torch.no_grad():
		a = renderer(textured, R, T, return_mask=True)
		b = renderer(plain, R, T, return_mask=True)
	assert torch.equal(a['mask'], b['mask']) and a['mask'].max() > 0.5
	assert a['image'].shape == (3, 2, 64, 64, 3) and torch.isfinite(a['image']).all()
	assert (a['image'] - b['image']).abs().mean() < 0.1   # the same field, read two ways
	frames = vis.turntable(textured[1], None, image_size=64, nframes=4, azim=70, dist=0.35, silent=True)
	assert frames.dtype == torch.uint8 and frames.shape == (4, 64, 64, 3) and (frames < 255).any()


def test_eval_3d_writes_textured_meshes(tmp_path):
	from tests.test_gpu_eval2d import _model
	from tests.test_gpu_vis import _foot3d_val2
	from find_amd import evaluate
	from find_amd.dataset import load_obj, load_texture_png
	ds = _foot3d_val2(str(tmp_path / 'data'))
	model = _model(2)
	kp_idx = [3, 17, 40, 101]
	uvs = synthetic.face_atlas(model.template_faces.shape[1])
	torch.manual_seed(21)
	res0, extra0 = evaluate.eval_3d(model, ds, kp_idx, samples=2000, export_meshes=True, out_dir=str(tmp_path / 'plain'))
	torch.manual_seed(21)
	res1, extra1 = evaluate.eval_3d(model, ds, kp_idx, samples=2000, export_meshes=True, out_dir=str(tmp_path / 'tex'), template_uvs=uvs, texture_size=96,
									texture_pad=2)
	today = ['00_gt_mesh.obj', '00_pred_mesh.obj', '01_gt_mesh.obj', '01_pred_mesh.obj']
	more = [f'{n:02d}_pred_textured.{e}' for n in range(2) for e in ('mtl', 'obj', 'png')]
	assert res0 == res1
	assert sorted(os.listdir(tmp_path / 'plain' / 'meshes')) == today and sorted(os.path.basename(f) for f in extra0['files']) == today
	assert sorted(os.listdir(tmp_path / 'tex' / 'meshes')) == sorted(today + more) and sorted(os.path.basename(f) for f in extra1['files']) == sorted(today + more)
	for f in today:
		assert open(tmp_path / 'plain' / 'meshes' / f).read() == open(tmp_path / 'tex' / 'meshes' / f).read()
	for n in range(2):
		v, f, props = load_obj(str(tmp_path / 'tex' / 'meshes' / f'{n:02d}_pred_textured.obj'))
		v0, f0, _ = load_obj(str(tmp_path / 'tex' / 'meshes' / f'{n:02d}_pred_mesh.obj'))
		assert torch.equal(v, v0) and torch.equal(f.verts_idx, f0.verts_idx) and torch.equal(f.textures_idx, uvs[1]) and torch.equal(props.verts_uvs, uvs[0])
		png = load_texture_png(str(tmp_path / 'tex' / 'meshes' / f'{n:02d}_pred_textured.png'))
		assert png.shape == (96, 96, 3) and 0.01 < (png < 1).float().mean() < 1


# ------------------------------------------------------------------------------------------------ 5. poison
@contextlib.contextmanager
def poisoned_bake(byte):
	"""tests/poison.py's proxy on find_amd.bake: every torch.empty / torch.empty_like of the module comes back filled with `byte`."""
	from find_amd import bake
	if byte not in poison.PATTERNS:
		raise ValueError(byte)
	assert bake.torch is torch
	proxy = poison._TorchProxy(byte)
	try:
		bake.torch = proxy
		yield proxy
	finally:
		bake.torch = torch


def test_no_op_reads_or_leaves_unwritten_memory():
	from test_poison_host import allocating_ops
	from find_amd import bake
	vu, fu = (torch.from_numpy(x).cuda() for x in _atlas(384))
	tv, tf, tuv = (torch.from_numpy(x).cuda() for x in _flat_grid())
	A = torch.linspace(-3, 3, 15, device='cuda').reshape(3, 5)
	ran = set()

	def run():
		out = {}
		out['face'], out['bary'] = bake.uv_raster(vu, fu, (64, 48))
		out['face_none'], out['bary_none'] = bake.uv_raster(vu, fu[:0], (17, 9))
		out['face_rules'], out['bary_rules'] = bake.uv_raster(*(torch.from_numpy(x).cuda() for x in rules_case()), (40, 56))
		for pad in (0, 4, 16):
			out[f'src{pad}'] = bake.dilate_map(out['face'], pad)
		out['src_none'] = bake.dilate_map(out['face_none'], 3)
		plan = bake.plan(tuv, tf, 40, pad=2)
		out['lookup'], out['idx'] = plan.lookup, plan.idx
		out['maps'] = bake.bake(lambda pos: pos @ A + 0.25, plan, tv[None], tf, texels_per_call=300)
		ran.update(('uv_raster', 'dilate_map', 'bake'))
		torch.cuda.synchronize()
		return {k: v.clone() for k, v in out.items()}
	runs = []
	for byte in (None, 0xFF, 0x00):
		run()   # (what a forgotten region would hold: the right values of this call)
		with (poisoned_bake(byte) if byte is not None else contextlib.nullcontext()) as proxy:
			runs.append(run())
			assert byte is None or proxy.calls >= 12
	assert bake.torch is torch
	rules = {k: poison.Rule(irange=(0, 384)) for k in ('face',)}
	bad = poison.compare('bake', *runs, rules)
	assert not bad, '\n'.join(bad)
	assert (runs[0]['face_none'] == -1).all() and not runs[0]['bary_none'].any() and (runs[0]['src_none'] == -1).all()
	ops = allocating_ops(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'find_amd', 'bake.py'))
	assert sorted(ops) == ['bake', 'dilate_map', 'uv_raster'] and set(ops) <= ran
