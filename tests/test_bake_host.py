"""find_amd.bake without a GPU: the two entry points are declared, bound and exported and refuse bad arguments before any HIP call, the
wrappers have no CPU fallback, the numpy reference (tests/bake_ref.py) gives the answers worked out by hand, a textured OBJ reads back
bit for bit, and synthetic.face_atlas is what it says."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bake_ref
from find_amd import bake, synthetic

HERE = os.path.dirname(os.path.abspath(__file__))
SYMBOLS = ('find_uv_raster', 'find_uv_dilate_map')

QUAD_UV = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
QUAD_FACES = np.array([[0, 1, 2], [0, 2, 3]])


def test_header_and_bindings_declare_the_symbols():
	from find_amd import _lib
	hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'find_hip.h')).read()
	for name in SYMBOLS:
		assert re.search(r'\bint ' + name + r'\(', hdr), name
		assert name in _lib.PROTOTYPES and hasattr(_lib.lib(), name), name
	assert len(_lib.PROTOTYPES['find_uv_raster'][1]) == 9 and len(_lib.PROTOTYPES['find_uv_dilate_map'][1]) == 6


def test_bad_arguments_are_refused_before_any_hip_call():
	"""Host memory stands in for the device pointers: a call that got as far as HIP would fail another way (or not at all)."""
	from find_amd import _lib
	L = _lib.lib()
	buf = ctypes.create_string_buffer(4096)
	p = ctypes.c_void_p(ctypes.addressof(buf))

	def refused(rc, word):
		msg = L.find_last_error()
		assert rc == -1 and msg and word in msg, (rc, msg)

	refused(L.find_uv_raster(p, 4, p, 2, 8, 8, None, p, None), b'NULL')
	refused(L.find_uv_raster(p, 4, p, 2, 8, 8, p, None, None), b'NULL')
	refused(L.find_uv_raster(None, 4, p, 2, 8, 8, p, p, None), b'NULL')
	refused(L.find_uv_raster(p, 4, None, 2, 8, 8, p, p, None), b'NULL')
	refused(L.find_uv_raster(p, 4, p, 2, 1, 8, p, p, None), b'map size')
	refused(L.find_uv_raster(p, 4, p, 2, 8, 4097, p, p, None), b'map size')
	refused(L.find_uv_raster(p, 4, p, -1, 8, 8, p, p, None), b'bad sizes')
	refused(L.find_uv_dilate_map(None, 8, 8, 4, p, None), b'NULL')
	refused(L.find_uv_dilate_map(p, 8, 8, 4, None, None), b'NULL')
	refused(L.find_uv_dilate_map(p, 1, 8, 4, p, None), b'map size')
	refused(L.find_uv_dilate_map(p, 8, 4097, 4, p, None), b'map size')
	refused(L.find_uv_dilate_map(p, 8, 8, 17, p, None), b'pad')
	refused(L.find_uv_dilate_map(p, 8, 8, -1, p, None), b'pad')


def test_ops_have_no_cpu_fallback():
	vu, fu = torch.from_numpy(QUAD_UV), torch.from_numpy(QUAD_FACES)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		bake.uv_raster(vu, fu, 9)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		bake.dilate_map(torch.zeros(4, 4, dtype=torch.int32), 2)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		bake.plan(vu, fu, (9, 9))


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_reference_on_the_unit_quad(dtype):
	"""9 x 9 over the unit square split along its diagonal: every centre is k / 8, every product exact.  Row 0 is v = 1; texel (i, j) has
	u = j / 8, v = 1 - i / 8.  Face 0 = (0,0), (1,0), (1,1) holds u >= v: the diagonal (by the smallest index) and the lower right."""
	face, bary, m = bake_ref.raster(QUAD_UV, QUAD_FACES, 9, 9, dtype)
	i, j = np.meshgrid(np.arange(9), np.arange(9), indexing='ij')
	assert np.array_equal(face, np.where(j >= 8 - i, 0, 1))
	assert face[0, 0] == 1 and face[8, 8] == 0 and face[0, 8] == 0 and face[8, 0] == 0 and face[1, 0] == 1 and face[8, 7] == 0
	u, v = j / 8.0, 1 - i / 8.0
	# face 0: b0 = 1 - u, b1 = u - v, b2 = v; face 1 = (0,0), (1,1), (0,1): b0 = 1 - v, b1 = u, b2 = v - u
	want = np.where((face == 0)[..., None], np.stack([1 - u, u - v, v], -1), np.stack([1 - v, u, v - u], -1))
	assert bary.dtype == dtype and np.array_equal(bary, want.astype(dtype))
	assert np.array_equal(m == 0, (i == 0) | (j == 0) | (i == 8) | (j == 8) | (i + j == 8)) and (m >= 0).all()


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_reference_on_a_hand_worked_triangle(dtype):
	"""H = 5 rows, W = 7 columns; the triangle (0,0), (1,0), (0,1) in UV: u + v <= 1.  u = j / 6, v = 1 - i / 4: covered where
	j / 6 <= i / 4, i.e. 2 j <= 3 i -- row 0 (the top, v = 1) holds column 0 only, row 4 (v = 0) all seven.  Swapping u and v, or H and W,
	gives another picture."""
	uv = np.array([[0, 0], [1, 0], [0, 1]], np.float32)
	face, bary, m = bake_ref.raster(uv, [[0, 1, 2]], 5, 7, dtype)
	want = np.array([[1, 0, 0, 0, 0, 0, 0],
					 [1, 1, 0, 0, 0, 0, 0],
					 [1, 1, 1, 1, 0, 0, 0],
					 [1, 1, 1, 1, 1, 0, 0],
					 [1, 1, 1, 1, 1, 1, 1]])
	assert face.shape == (5, 7) and np.array_equal(face >= 0, want == 1) and np.array_equal(face[face >= 0], np.zeros(want.sum()))
	# texel (2, 3): u = v = 0.5, on the hypotenuse: (0, 0.5, 0.5); texel (4, 6): the corner (1, 0); texel (3, 1): u = 1/6, v = 1/4
	assert np.allclose(bary[2, 3], [0, 0.5, 0.5], atol=1e-7) and np.allclose(bary[4, 6], [0, 1, 0], atol=1e-7)
	assert np.allclose(bary[3, 1], [1 - 1 / 6 - 1 / 4, 1 / 6, 1 / 4], atol=1e-7)
	assert not bary[face < 0].any() and m[0, 1] < -0.1 and m[4, 3] == 0 and m[3, 1] > 0.1
	# the rules' skipped faces: an index out of range, a repeated vertex, a NaN
	bad = np.array([[0, 0], [1, 0], [0, 1], [np.nan, 0.5]], np.float32)
	f2, _, _ = bake_ref.raster(bad, [[0, 1, 4], [-1, 1, 2], [0, 1, 1], [0, 1, 3], [0, 1, 2]], 5, 7, dtype)
	assert np.array_equal(f2 >= 0, want == 1) and (f2[f2 >= 0] == 4).all()


def test_reference_dilate_on_known_answers():
	face = np.full((5, 6), -1, np.int32)
	face[2, 2] = 7
	face[2, 4] = 0
	assert np.array_equal(bake_ref.dilate(face, 0), np.where(face >= 0, np.arange(30).reshape(5, 6), -1))
	src = bake_ref.dilate(face, 1)
	a, b = 2 * 6 + 2, 2 * 6 + 4
	want = np.array([[-1, -1, -1, -1, -1, -1],
					 [-1, a, a, a, b, b],      # (1, 3): both at distance 2 -- the smaller flat index
					 [-1, a, a, a, b, b],      # (2, 3): both at distance 1
					 [-1, a, a, a, b, b],
					 [-1, -1, -1, -1, -1, -1]])
	assert np.array_equal(src, want)
	far = bake_ref.dilate(face, 2)
	assert far[0, 0] == a and far[4, 5] == b and far[0, 5] == b and far[2, 0] == a
	assert (bake_ref.dilate(np.full((4, 4), -1), 16) == -1).all()


def test_textured_obj_reads_back(tmp_path):
	from find_amd.dataset import load_obj, load_texture_png
	from find_amd.structures import Meshes, TexturesUV
	g = torch.Generator().manual_seed(5)
	verts = torch.randn(2, 6, 3, generator=g)
	faces = torch.tensor([[0, 1, 2], [0, 2, 3], [3, 4, 5], [1, 4, 5]])
	verts_uvs = torch.rand(2, 9, 2, generator=g)
	faces_uvs = torch.tensor([[0, 1, 2], [3, 4, 5], [-1, -1, -1], [6, 7, 8]])[None].expand(2, -1, -1)
	maps = torch.rand(2, 5, 7, 3, generator=g)
	maps[1, 0, 0] = torch.tensor([0.0, 1.0, 200 / 255])
	maps[1, 0, 1] = torch.tensor([1.5, -0.5, float('nan')])
	mesh = Meshes(verts, faces, TexturesUV(maps, faces_uvs, verts_uvs))
	loc = str(tmp_path / 'foot.obj')
	files = bake.export_textured_obj(mesh, loc, idx=1)
	assert files == [loc, str(tmp_path / 'foot.mtl'), str(tmp_path / 'foot.png')] and all(os.path.exists(f) for f in files)
	text = open(loc).read().split('\n')
	assert text[0] == 'mtllib foot.mtl' and text[1] == 'usemtl material_0' and 'f 4 5 6' in text and 'f 1/1 2/2 3/3' in text
	assert open(files[1]).read().split('\n')[0] == 'newmtl material_0' and 'map_Kd foot.png' in open(files[1]).read()
	v, f, props = load_obj(loc)
	assert torch.equal(v, verts[1]) and torch.equal(f.verts_idx, faces) and torch.equal(f.textures_idx, faces_uvs[1])
	assert torch.equal(props.verts_uvs, verts_uvs[1])
	png = load_texture_png(files[2])
	x = maps[1].numpy()
	with np.errstate(invalid='ignore'):
		want = np.where(np.isnan(x), np.float32(0), np.clip(np.float32(255) * x, 0, 255)).astype(np.uint8)
	assert want[0, 0].tolist() == [0, 255, 200] and want[0, 1].tolist() == [255, 0, 0]
	assert png.shape == (5, 7, 3) and np.array_equal((png.numpy() * 255).round().astype(np.uint8), want)
	with pytest.raises(ValueError, match='TexturesUV'):
		bake.export_textured_obj(Meshes(verts, faces), loc)


@pytest.mark.parametrize('n_faces', [1, 2, 7, 384])
def test_face_atlas(n_faces):
	vu, fu = synthetic.face_atlas(n_faces)
	assert vu.shape == (3 * n_faces, 2) and vu.dtype == torch.float32 and fu.shape == (n_faces, 3) and fu.dtype == torch.int64
	assert torch.equal(fu.flatten(), torch.arange(3 * n_faces))
	assert vu.min() >= 0 and vu.max() <= 1
	t = vu.double()[fu]                                    # (F, 3, 2)
	e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
	area = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
	g = max(1, int(np.ceil(np.sqrt((n_faces + 1) // 2))))
	assert (area > 0.2 / g ** 2).all()                     # counter-clockwise, legs of 0.7 cells
	# pairwise disjoint: for every pair a separating axis among the six edge normals
	n = torch.stack([t[:, (k + 1) % 3] - t[:, k] for k in range(3)], 1)
	n = torch.stack([-n[..., 1], n[..., 0]], -1)           # (F, 3, 2)
	proj = torch.einsum('fkc,gvc->fkgv', n, t)             # edge normal k of face f on corner v of face g
	own = torch.einsum('fkc,fvc->fkv', n, t)
	sep = (proj.max(-1).values < own.min(-1).values[:, :, None]) | (proj.min(-1).values > own.max(-1).values[:, :, None])   # (F, 3, G): f's axis k separates g
	sep = sep.any(1)
	apart = sep | sep.T
	apart.fill_diagonal_(True)
	assert apart.all()
	with pytest.raises(ValueError):
		synthetic.face_atlas(4, inset=0.4)
