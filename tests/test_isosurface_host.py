"""Surface nets on the host: the properties of the numpy restatement (tests/isosurface_ref.py) on fields made from formulas, the host build of
the per-cell and per-sample arithmetic, the C interface before any launch, and what the wrappers of find_amd.isosurface say on the CPU.

The fields: a sphere of radius 0.04 in the box +-0.06 at 8^3, 16^3 and 32^3 (sample (i, j, k) at -0.06 + (i + 0.5) 0.12 / n, the convention of
inside.grid_points), an ellipsoid (0.02, 0.04, 0.1) on (9, 17, 33) over its semi-axes + 0.02, a torus (R 0.035, r 0.012) on (32, 32, 16), two
spheres of radius 0.02 at x = +-0.03 on 24^3, one inside sample in 3^3, one cell, a plane and the checkerboard pair.  Status bit 1 is
conservative -- an active cell in the outermost cell LAYER: the 8^3 sphere, whose second sample layer is inside, sets it and is closed all
the same; the other smooth cases leave it clear.

Caps, none a constant of the code under test: the extracted sphere's volume is second order in the spacing -- within 20 %, 6 %, 1.5 % of
4/3 pi r^3 at 8^3, 16^3, 32^3 (14.6 %, 4.0 %, 1.0 % were measured) and each at most 0.3 of the one before; its radius at 32^3 is within half a
spacing (1.3e-4 was measured for a spacing of 3.75e-3); float32 vertices are within 1e-5 grid units of float64 (1e-6 was measured)."""
import inspect
import math
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import isosurface_ref as ref   # noqa: E402


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('name', list(ref.SMOOTH))
def test_smooth_shapes_are_watertight_and_oriented(name):
	r = ref.result(name)
	chi = ref.euler(r.faces)
	print(f'{name} {ref.field(name).shape}: {len(r.g)} vertices, {len(r.faces)} faces, chi {chi}, status {r.status}, {r.ambiguous} ambiguous lattice faces')
	assert r.ambiguous == 0 and ref.watertight(r.faces) and chi == ref.SMOOTH[name]
	assert r.status == (ref.BOUNDARY if name == 'sphere8' else 0)
	assert len(np.unique(r.faces)) == len(r.g) and r.faces.min() == 0 and r.faces.max() == len(r.g) - 1
	assert ref.exact_volume(r.g, r.faces) > 0   # normals from inside to outside
	r32 = ref.result(name, np.float32)
	assert r32.g.dtype == np.float32 and np.array_equal(r32.faces, r.faces) and np.array_equal(r32.cellmap, r.cellmap)
	e32 = np.abs(r32.g - r.g).max()
	print(f'{name}: float32 against float64 {e32:.3e} grid units')
	assert e32 <= 1e-5
	# vertices in flat cell order, each in its own cell
	cells = np.argwhere(r.cellmap >= 0)
	assert np.array_equal(r.cellmap[r.cellmap >= 0], np.arange(len(r.g))) and (r.g >= cells).all() and (r.g <= cells + 1).all()


def test_sphere_volume_is_second_order_and_radius():
	want = 4 / 3 * math.pi * 0.04 ** 3
	off = []
	for n, cap in ((8, 0.20), (16, 0.06), (32, 0.015)):
		r = ref.result(f'sphere{n}')
		spacing = 0.12 / n
		verts = -0.06 + (r.g + 0.5) * spacing
		off.append(ref.exact_volume(verts, r.faces) / want - 1)
		print(f'sphere at {n}^3: volume {100 * off[-1]:.2f} % off')
		assert -cap <= off[-1] < 0
	assert off[1] / off[0] <= 0.3 and off[2] / off[1] <= 0.3
	radius = np.sqrt((verts ** 2).sum(1))
	print(f'sphere at 32^3: worst radius error {np.abs(radius - 0.04).max():.3e}, spacing {spacing:.3e}')
	assert np.abs(radius - 0.04).max() <= 0.5 * spacing


def test_one_sample_one_cell_plane_and_checkerboard():
	r = ref.result('one_sample')   # a cube of side 1/3 cell about the sample
	assert len(r.g) == 8 and len(r.faces) == 12 and ref.watertight(r.faces) and ref.euler(r.faces) == 2
	assert np.allclose(np.sort(np.unique(r.g)), [5 / 6, 7 / 6], atol=1e-15) and abs(ref.exact_volume(r.g, r.faces) - 1 / 27) <= 1e-15
	r = ref.result('one_cell')
	assert len(r.g) == 1 and r.faces.shape == (0, 3) and r.status == ref.BOUNDARY
	assert np.allclose(r.g, [[1 / 9, 1 / 9, 1 / 9]], atol=1e-15)   # three crossing edges at t = 1/3: (t, 0, 0), (0, t, 0), (0, 0, t)
	r = ref.result('plane')
	assert r.status == ref.BOUNDARY and len(r.faces) > 0 and not ref.closed(r.faces) and r.ambiguous == 0
	assert (ref.undirected_edge_counts(r.faces) <= 2).all() and (ref.directed_edge_counts(r.faces) == 1).all()
	r = ref.result('checkerboard')   # closed, not manifold: held against the restatement only
	u = ref.undirected_edge_counts(r.faces)
	print(f'checkerboard: {len(r.g)} vertices, {len(r.faces)} faces, {r.ambiguous} ambiguous lattice face(s), edge multiplicities {np.unique(u).tolist()}')
	assert r.ambiguous == 1 and ref.closed(r.faces) and u.max() == 4 and not ref.watertight(r.faces)


def test_sides_are_exact_and_non_finite_samples_are_outside():
	v = ref.field('sphere8').copy()
	iso = v[3, 3, 2]   # a sample exactly at iso is outside; one ulp above iso it is inside
	assert not ref.sides(v, iso)[3, 3, 2] and ref.sides(v, np.nextafter(iso, np.float32(1)))[3, 3, 2]
	base = ref.extract(v, iso)
	assert base.status & ref.NON_FINITE == 0
	for bad in (np.nan, np.inf, -np.inf):
		w = v.copy()
		w[3, 3, 3] = bad   # (inside the sphere)
		r = ref.extract(w, iso)
		assert r.status & ref.NON_FINITE and not ref.sides(w, iso)[3, 3, 3] and np.isfinite(r.g).all() and ref.closed(r.faces)
		assert not np.array_equal(r.g, base.g)   # the sample left the inside
		assert np.isfinite(ref.extract(w, iso, np.float32).g).all()


def test_transposed_grids_give_transposed_meshes():
	"""The strides: the (5, 9, 17) ellipsoid with its axes permuted has the same vertex set, permuted."""
	v = ref._ellipsoid((5, 9, 17))
	r = ref.extract(v)
	assert len(r.g) > 50 and ref.closed(r.faces)
	for perm in ((1, 2, 0), (2, 1, 0)):
		q = ref.extract(np.ascontiguousarray(v.transpose(perm)))
		assert len(q.g) == len(r.g) and len(q.faces) == len(r.faces)
		order = lambda a: a[np.lexsort(np.round(a, 6).T[::-1])]   # noqa: E731 (the sum over the edges runs in another order: equal to rounding)
		assert np.abs(order(r.g[:, perm]) - order(q.g)).max() <= 1e-12


def test_torch_vertices_with_fixed_topology():
	for name in ('sphere16', 'plane'):
		v = torch.from_numpy(ref.field(name)).double().requires_grad_(True)
		iso = torch.tensor(0., dtype=torch.float64, requires_grad=True)
		g = ref.g_torch(v, iso)
		assert np.abs(g.detach().numpy() - ref.result(name).g).max() <= 1e-14
		gv, gi = torch.autograd.grad(g.sum(), (v, iso))
		assert torch.isfinite(gv).all() and torch.isfinite(gi) and gv.abs().max() > 0


# ------------------------------------------------------------------ arguments, on the CPU
def test_cpu_tensors_and_bad_arguments_raise_with_the_functions_name():
	from find_amd import isosurface, synthetic
	v, f = synthetic.template(1002)
	field = torch.zeros(1, 4, 4, 4)
	o, s = torch.zeros(3), torch.ones(3)
	for name, call in (('extract_surface', lambda: isosurface.extract_surface(field, o, s)), ('field_grid', lambda: isosurface.field_grid(v[None], f, 8)),
					   ('field_grid', lambda: isosurface.remesh(v[None], f, 8))):
		with pytest.raises(RuntimeError, match=f'find_amd.isosurface.{name}.*no CPU fallback'):
			call()
	for call in (lambda: isosurface.extract_surface(field[0], o, s), lambda: isosurface.extract_surface(torch.zeros(1, 1, 4, 4), o, s),
				 lambda: isosurface.extract_surface(torch.zeros(1, 4, 4, 1025), o, s), lambda: isosurface.field_grid(v, f, 8),
				 lambda: isosurface.field_grid(v[None], f[:, :2], 8)):
		with pytest.raises(RuntimeError, match='find_amd.isosurface.*expected'):
			call()


def test_signatures():
	from find_amd import isosurface
	sig = inspect.signature(isosurface.extract_surface).parameters
	assert list(sig) == ['values', 'origin', 'spacing', 'iso', 'max_verts', 'max_faces']
	assert (sig['iso'].default, sig['max_verts'].default, sig['max_faces'].default) == (0.0, None, None)
	assert 'READ BACK' in isosurface.extract_surface.__doc__
	sig = inspect.signature(isosurface.field_grid).parameters
	assert list(sig) == ['verts', 'faces', 'res', 'offset', 'pad', 'level'] and [sig[k].default for k in list(sig)[2:]] == [64, 0.0, 0.005, 0.5]
	sig = inspect.signature(isosurface.remesh).parameters
	assert list(sig) == ['verts', 'faces', 'res', 'offset', 'pad', 'level', 'as_meshes'] and sig['as_meshes'].default is False
	assert (isosurface.BOUNDARY, isosurface.VERTS_OVERFLOW, isosurface.FACES_OVERFLOW, isosurface.NON_FINITE) == (1, 2, 4, 8)


def test_the_wrappers_live_in_a_module_of_their_own():
	"""The poison census of tests/test_poison_host.py walks four modules; find_amd.isosurface allocates and is none of them
	(tests/test_gpu_isosurface.py poisons its allocations itself)."""
	from poison import MODULES
	from test_poison_host import allocating_ops
	assert 'find_amd.isosurface' not in MODULES
	ops = allocating_ops(os.path.join(ROOT, 'find_amd', 'isosurface.py'))
	assert '_SurfaceNets' in ops and 'field_grid' in ops


# ------------------------------------------------------------------ the C side, before any launch
def test_host_build_of_the_cell_arithmetic():
	"""csrc/surface_nets_math.h -- the sides, the vertex of a cell for all 254 mixed corner masks and the per-sample backward term against
	central differences: the functions surface_nets.hip compiles for the device -- built for the host and run by
	tools/surface_nets_host_check.cpp."""
	cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++') if c and os.path.exists(c)), None)
	assert cxx is not None, 'no host C++ compiler'
	with tempfile.TemporaryDirectory() as tmp:
		exe = os.path.join(tmp, 'surface_nets_host_check')
		subprocess.run([cxx, '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'find_amd', 'csrc'), os.path.join(ROOT, 'tools', 'surface_nets_host_check.cpp'), '-o', exe],
					   check=True, capture_output=True)
		r = subprocess.run([exe], capture_output=True, text=True)
	assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:]


def _ws_bytes(n, nx, ny, nz, block=256):
	"""The layout find_hip.h describes: the cell -> vertex map, three int32 and two int64 per block of 256 samples, each carve 256-byte aligned."""
	up = lambda x: (x + 255) // 256 * 256   # noqa: E731
	nb = -(-nx * ny * nz // block)
	return up(4 * n * (nx - 1) * (ny - 1) * (nz - 1)) + 3 * up(4 * n * nb) + 2 * up(8 * n * nb)


def test_header_binding_workspace_and_refusals():
	from find_amd import _lib, isosurface
	hdr = open(os.path.join(ROOT, 'include', 'find_hip.h')).read()
	assert '#define FIND_SURFACE_NETS_BLOCK 256' in hdr and isosurface.BLOCK_CELLS == 256
	names = ('find_surface_nets_ws_bytes', 'find_surface_nets_bwd_ws_bytes', 'find_surface_nets_count', 'find_surface_nets_emit', 'find_surface_nets_bwd')
	for name in names:
		assert name in _lib.PROTOTYPES and f'{name}(' in hdr
		assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
	L = _lib.lib()
	assert L.find_surface_nets_ws_bytes(1, 2, 2, 2) == 1536 == _ws_bytes(1, 2, 2, 2)
	assert L.find_surface_nets_ws_bytes(2, 64, 64, 64) == 2057728 == _ws_bytes(2, 64, 64, 64)
	for dims in ((3, 5, 9, 17), (16, 128, 128, 128), (1, 1024, 2, 2), (1, 2, 2, 257)):
		assert L.find_surface_nets_ws_bytes(*dims) == _ws_bytes(*dims), dims
	assert L.find_surface_nets_ws_bytes(0, 4, 4, 4) == 256 and L.find_surface_nets_bwd_ws_bytes(0, 4, 4, 4) == 256
	assert L.find_surface_nets_bwd_ws_bytes(1, 2, 2, 2) == 256 and L.find_surface_nets_bwd_ws_bytes(16, 128, 128, 128) == 16 * 8192 * 8
	for q in (L.find_surface_nets_ws_bytes, L.find_surface_nets_bwd_ws_bytes):
		assert q(1 << 16, 4, 4, 4) == -1 and q(-1, 4, 4, 4) == -1 and q(1, 1, 4, 4) == -1 and q(1, 4, 1025, 4) == -1 and q(1, 4, 4, 0) == -1
	one = torch.zeros(4096)   # (host memory: every call below is refused before it would be read)
	p = _lib.ptr(one)
	big = 1 << 20
	assert L.find_surface_nets_count(p, 0., 1, 4, 4, 1, p, p, p, p, big, None) == -1 and b'bad sizes' in L.find_last_error()
	assert L.find_surface_nets_count(None, 0., 1, 4, 4, 4, p, p, p, p, big, None) == -1 and b'NULL' in L.find_last_error()
	assert L.find_surface_nets_count(p, 0., 1, 4, 4, 4, p, p, None, p, big, None) == -1 and b'NULL' in L.find_last_error()
	assert L.find_surface_nets_count(p, 0., 1, 4, 4, 4, p, p, p, p, 1535, None) == -2 and b'workspace' in L.find_last_error()
	assert L.find_surface_nets_count(None, 0., 0, 4, 4, 4, None, None, None, None, 0, None) == 0   # no mesh: nothing to do
	assert L.find_surface_nets_emit(p, 0., 1, 4, 4, 1025, p, p, 8, 8, p, p, p, p, big, None) == -1 and b'bad sizes' in L.find_last_error()
	assert L.find_surface_nets_emit(p, 0., 1, 4, 4, 4, p, p, -1, 8, p, p, p, p, big, None) == -1 and b'capacities' in L.find_last_error()
	assert L.find_surface_nets_emit(p, 0., 1, 4, 4, 4, p, p, 8, 1 << 33, p, p, p, p, big, None) == -1 and b'capacities' in L.find_last_error()
	assert L.find_surface_nets_emit(p, 0., 1, 4, 4, 4, p, p, 8, 8, None, p, p, p, big, None) == -1 and b'NULL' in L.find_last_error()
	assert L.find_surface_nets_emit(p, 0., 1, 4, 4, 4, p, None, 8, 8, p, p, p, p, big, None) == -1 and b'NULL' in L.find_last_error()
	assert L.find_surface_nets_emit(p, 0., 1, 4, 4, 4, p, p, 8, 8, p, p, p, p, 256, None) == -2 and b'workspace' in L.find_last_error()
	assert L.find_surface_nets_emit(None, 0., 0, 4, 4, 4, None, None, 0, 0, None, None, None, None, 0, None) == 0
	assert L.find_surface_nets_bwd(p, 0., 1, 4, 1, 4, p, p, 8, p, p, p, big, None) == -1 and b'bad sizes' in L.find_last_error()
	assert L.find_surface_nets_bwd(p, 0., 1, 4, 4, 4, p, p, 1 << 30, p, p, p, big, None) == -1 and b'capacities' in L.find_last_error()
	assert L.find_surface_nets_bwd(p, 0., 1, 4, 4, 4, None, p, 8, p, p, p, big, None) == -1 and b'NULL' in L.find_last_error()
	assert L.find_surface_nets_bwd(p, 0., 1, 4, 4, 4, p, None, 8, p, p, p, big, None) == -1 and b'NULL' in L.find_last_error()
	assert L.find_surface_nets_bwd(p, 0., 1, 4, 4, 4, p, p, 8, p, p, p, 255, None) == -2 and b'workspace' in L.find_last_error()
	assert L.find_surface_nets_bwd(None, 0., 0, 4, 4, 4, None, None, 0, None, None, None, 0, None) == 0
