"""find_amd.vis on the host: the camera algebra of a spin (rotating the camera about world z == rotating the mesh, reference
src/vis/mesh_turntable.py:41-55), the OBJ round trip of export_obj / read_obj_colours, the refusals of turntable and the new C-ABI symbol.
The oracle's pieces: look_at_view_transform from oracle/camera_ref.py, Rz(theta) = euler_angles_to_matrix([0, 0, theta], 'XYZ') from
oracle/mlp_ref.py (the registration's restatement of it)."""
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import camera_ref, mlp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_rz(theta64):
	e = torch.zeros(theta64.shape[0], 3, dtype=torch.float64)
	e[:, 2] = theta64
	return mlp_ref.euler_angles_to_matrix_xyz(e).numpy()


@pytest.mark.parametrize('nframes', [2, 5, 250])
def test_turntable_views_rotate_the_camera_as_upstream_rotates_the_mesh(nframes):
	from find_amd import vis
	from find_amd.renderer import FootRenderer
	R, T = vis.turntable_views(FootRenderer(image_size=64, device='cpu'), nframes=nframes, azim=70, dist=0.35)
	assert R.shape == (nframes, 3, 3) and T.shape == (nframes, 3) and R.dtype == torch.float32 and T.dtype == torch.float32
	R0, T0 = camera_ref.look_at_view_transform(dist=0.35, elev=0.0, azim=70.0, up=((1, 0, 0),))
	R0, T0 = R0[0].astype(np.float64), T0[0].astype(np.float64)
	theta = torch.linspace(0, 2 * math.pi, nframes, dtype=torch.float32).double()   # (upstream's float32 angles, both ends included)
	Rz = _oracle_rz(theta)
	p = np.random.RandomState(nframes).uniform(-0.15, 0.15, (50, 3))
	R64, T64 = R.double().numpy(), T.double().numpy()
	for i in range(nframes):
		got = p @ R64[i] + T64[i]
		want = (p @ Rz[i]) @ R0 + T0
		assert np.abs(got - want).max() < 1e-6, (i, np.abs(got - want).max())
		assert np.abs(R64[i].T @ R64[i] - np.eye(3)).max() < 1e-6, i
	assert np.abs(R64[0] - R64[-1]).max() < 1e-6
	if nframes > 2:
		assert np.abs(R64[0] - R64[nframes // 2]).max() > 0.5   # (and the frames between do turn)


def _coloured_meshes():
	from find_amd.structures import Meshes, TexturesVertex
	verts = torch.tensor([[[1e-7, -0.123456789, 1 / 3], [0.25, 1e-7, -1 / 3], [-0.123456789, 0.5, 1e-7], [1 / 3, 1 / 3, 0.1]],
						  [[0.7, -0.2, 1e-7], [1 / 3, 0.123456789, 0.9], [-1e-7, 0.3, 0.4], [0.6, -1 / 3, 0.2]]], dtype=torch.float32)
	faces = torch.tensor([[0, 1, 2], [0, 2, 3], [3, 1, 0]])
	cols = torch.rand(2, 4, 3, generator=torch.Generator().manual_seed(0))
	cols[0, 0] = torch.tensor([1 / 3, 1e-7, 0.123456789])
	return Meshes(verts, faces, TexturesVertex(cols)), verts, faces, cols


def test_obj_round_trip_is_bit_exact(tmp_path):
	from find_amd import vis
	from find_amd.structures import Meshes, TexturesUV
	meshes, verts, faces, cols = _coloured_meshes()
	for idx in (0, 1):
		loc = vis.export_obj(meshes, str(tmp_path / f'm{idx}.obj'), idx=idx)
		v, c, f = vis.read_obj_colours(loc)
		assert v.dtype == torch.float32 and c.dtype == torch.float32 and f.dtype == torch.int64
		assert torch.equal(v, verts[idx]) and torch.equal(c, cols[idx]) and torch.equal(f, faces)
	assert not torch.equal(verts[0], verts[1])   # (idx does select)
	# the layout: `v x y z r g b` lines, then 1-based `f a b c`
	lines = open(str(tmp_path / 'm0.obj')).read().splitlines()
	assert len(lines) == 4 + 3 and all(len(l.split()) == 7 and l.startswith('v ') for l in lines[:4])
	assert lines[4:] == ['f 1 2 3', 'f 1 3 4', 'f 4 2 1']
	# geometry only: on request, and for a UV-textured mesh
	v, c, f = vis.read_obj_colours(vis.export_obj(meshes, str(tmp_path / 'plain.obj'), idx=1, include_colour=False))
	assert c is None and torch.equal(v, verts[1]) and torch.equal(f, faces)
	uv = TexturesUV(torch.rand(1, 4, 4, 3), faces[None], torch.rand(1, 4, 2))
	v, c, f = vis.read_obj_colours(vis.export_obj(Meshes(verts[:1], faces, uv), str(tmp_path / 'uv.obj')))
	assert c is None and torch.equal(v, verts[0]) and torch.equal(f, faces)
	# a ragged batch writes each mesh's own vertices and faces, not the padding
	ragged = Meshes([verts[0], verts[1][:3]], [faces, faces[:1]])
	v, c, f = vis.read_obj_colours(vis.export_obj(ragged, str(tmp_path / 'ragged.obj'), idx=1))
	assert c is None and torch.equal(v, verts[1][:3]) and torch.equal(f, faces[:1])


def test_turntable_refuses_a_cpu_mesh_and_an_unwritable_format(tmp_path):
	from find_amd import vis
	meshes = _coloured_meshes()[0]
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		vis.turntable(meshes[0], None, image_size=32, nframes=2, azim=70, dist=0.35)
	with pytest.raises(RuntimeError, match=r'\.gif'):
		vis.turntable(meshes[0], str(tmp_path / 'x.avi'), image_size=32, nframes=2)
	try:
		import imageio  # noqa: F401
	except ImportError:
		with pytest.raises(RuntimeError, match=r'imageio.*\.gif'):
			vis.turntable(meshes[0], str(tmp_path / 'x.mp4'), image_size=32, nframes=2)
	assert os.listdir(str(tmp_path)) == []


def test_error_colours_on_the_host():
	from find_amd import vis
	err = torch.tensor([[0.0, 15e-6, 30e-6, 31e-6, 1.0]])
	col = vis.error_colours(err)
	assert col.shape == (1, 5, 3) and torch.equal(col[..., 1:], torch.zeros(1, 5, 2))
	assert col[0, 0, 0] == 0 and col[0, 1, 0] == pytest.approx(0.5, rel=1e-6) and torch.equal(col[0, 2:, 0], torch.ones(3))


def test_frames_u8_symbol_is_declared_bound_and_exported():
	from find_amd import _lib
	assert 'find_frames_u8' in _lib.PROTOTYPES
	hdr = open(os.path.join(ROOT, 'include', 'find_hip.h')).read()
	hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
	assert re.search(r'\bint\s+find_frames_u8\s*\(', hdr)
	L = _lib.lib()
	assert hasattr(L, 'find_frames_u8')
	# argument checks come before any launch: they run without a GPU
	assert L.find_frames_u8(None, 1, 1, 1, 3, 1, None, None) == -1 and b'NULL' in L.find_last_error()
	import ctypes
	buf = ctypes.create_string_buffer(64)   # (a non-NULL host address: the sizes are refused before it is read)
	p = ctypes.addressof(buf)
	for n, h, w, c in ((0, 1, 1, 3), (1, 0, 1, 3), (1, 1, 1, 0), (1, 1, 1, 17), (1 << 20, 1 << 12, 1 << 12, 3)):
		assert L.find_frames_u8(p, n, h, w, c, 0, p, None) == -1 and b'bad sizes' in L.find_last_error(), (n, h, w, c)
