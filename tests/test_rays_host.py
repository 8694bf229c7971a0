"""Ray casting on the host: the numpy restatement of the pair test (tests/rays_ref.py) against closed forms, its watertightness on the closed
template with the triple-product flavour as the negative control, the visibility rule on an ellipsoid, the host build of csrc/raycast_math.h
against the float32 restatement bit for bit, the C interface before any launch, and what the wrappers of find_amd.rays say on the CPU.

Bounds, none a constant of the code under test: the closed forms are exact (every quantity is a small dyadic number); watertightness is a
count, 0 misses (0 of 9 842 was measured in float32 and float64; the triple-product flavour missed 186 in float32, at least 1 is asked); the
visibility margin is derived from the mesh in test_visibility_rule_on_an_ellipsoid."""
import inspect
import math
import os
import re
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
import inside_ref   # noqa: E402
import rays_ref as ref   # noqa: E402

CUBE_V, CUBE_F = inside_ref.CUBE_VERTS, inside_ref.CUBE_FACES   # vertex 4 x + 2 y + z; the side z = 0 is faces 8 (0, 2, 6) and 9 (0, 6, 4)
DTYPES = (np.float64, np.float32)


def _one(o, d, dt, verts=CUBE_V, faces=CUBE_F, **kw):
	t, idx, bary = ref.cast(np.array([o], float), np.array([d], float), verts, faces, dt, **kw)
	assert t.dtype == dt and bary.dtype == dt
	return float(t[0]), int(idx[0]), bary[0].tolist()


# ------------------------------------------------------------------ closed forms
@pytest.mark.parametrize('dt', DTYPES)
def test_axis_rays_against_the_unit_cube(dt):
	# (0.25, 0.5) on the side z = 0 is 0.5 v0 + 0.25 v2 + 0.25 v6; d has length 2, so t = 1 / 2
	assert _one([0.25, 0.5, -1], [0, 0, 2], dt) == (0.5, 8, [0.5, 0.25, 0.25])
	assert _one([0.25, 0.5, -1], [0, 0, -2], dt) == (math.inf, -1, [0, 0, 0])
	# on the side's diagonal both faces hold the point: the smallest face wins
	t, idx, bary = _one([0.5, 0.5, -1], [0, 0, 2], dt)
	assert (t, idx, bary) == (0.5, 8, [0.5, 0, 0.5])
	# negative directions along each axis: the far side at t = 2 (the origin is 2 beyond it)
	for k in range(3):
		o, d = [0.3, 0.6, 0.7], [0, 0, 0]
		o[k], d[k] = 3., -1.
		t, idx, bary = _one(o, d, dt)
		assert t == 2 and CUBE_V[CUBE_F[idx]][:, k].tolist() == [1, 1, 1] and abs(sum(bary) - 1) <= 1e-6 and min(bary) >= 0
	# the hit point is o + t d, and sum bary_i v_i
	rng = np.random.RandomState(1)
	o, d = rng.uniform(0.1, 0.9, (50, 3)), rng.uniform(-1, 1, (50, 3))
	t, idx, bary = ref.cast(o, d, CUBE_V, CUBE_F, dt)
	assert (idx >= 0).all() and (t > 0).all()
	hit = o + t[:, None].astype(float) * d
	assert np.abs(hit - (bary[:, :, None] * CUBE_V[CUBE_F[idx]]).sum(1)).max() <= (1e-12 if dt is np.float64 else 1e-5)
	assert np.abs(np.abs(hit - 0.5).max(1) - 0.5).max() <= (1e-12 if dt is np.float64 else 1e-5)


@pytest.mark.parametrize('dt', DTYPES)
def test_rules_of_the_pair_test(dt):
	inf = math.inf
	# a ray in the plane of a side misses its two faces (det == 0) ...
	assert _one([-1, 0.5, 0], [1, 0, 0], dt, faces=CUBE_F[8:10]) == (inf, -1, [0, 0, 0])
	# ... from a corner the faces at that corner are never hit: along the diagonal the first hit is at the far corner, t = 1
	t, idx, _ = _one([0, 0, 0], [1, 1, 1], dt)
	assert t == 1 and 0 not in CUBE_F[idx] and 7 in CUBE_F[idx]
	assert _one([0, 0, 0], [1, 0.5, 0.25], dt)[:2] == (1., 2)
	at_corner = (CUBE_F == 0).any(1)
	assert _one([0, 0, 0], [1, 0.5, 0.25], dt, faces=CUBE_F[at_corner]) == (inf, -1, [0, 0, 0])
	# skip: the named face is never hit; the other face of the diagonal takes over, the next side otherwise
	assert _one([0.5, 0.5, -1], [0, 0, 2], dt, skip=np.array([8]))[:2] == (0.5, 9)
	assert _one([0.25, 0.5, -1], [0, 0, 2], dt, skip=np.array([8]))[:2] == (1., 11)
	assert _one([0.25, 0.5, -1], [0, 0, 2], dt, skip=np.array([-1]))[:2] == (0.5, 8)
	# the interval is open below and closed above
	assert _one([0.25, 0.5, -1], [0, 0, 2], dt, t_min=0.5)[:2] == (1., 11)
	assert _one([0.25, 0.5, -1], [0, 0, 2], dt, t_max=0.5)[:2] == (0.5, 8)
	assert _one([0.25, 0.5, -1], [0, 0, 2], dt, t_max=0.4999999)[:2] == (inf, -1)
	assert _one([0.25, 0.5, -1], [0, 0, 2], dt, t_min=0.5, t_max=0.75)[:2] == (inf, -1)
	# -1 rows and indices out of range never hit
	padded = np.concatenate([[[-1, -1, -1], [0, 2, 8], [0, -1, 6]], CUBE_F[8:10], [[0, 6, 1 << 30]]])
	assert _one([0.25, 0.5, -1], [0, 0, 2], dt, faces=padded)[:2] == (0.5, 3)
	assert _one([0.25, 0.5, -1], [0, 0, 2], dt, faces=padded[[0, 1, 2, 5]]) == (inf, -1, [0, 0, 0])
	assert ref.cast(np.zeros((2, 3)), np.ones((2, 3)), CUBE_V, CUBE_F[:0], dt)[1].tolist() == [-1, -1] and ref.cast(np.zeros((0, 3)), np.zeros((0, 3)), CUBE_V, CUBE_F, dt)[0].shape == (0,)
	# zero and non-finite rays miss
	c = [0.5, 0.5, 0.5]
	for o, d in ((c, [0, 0, 0]), (c, [math.nan, 1, 0]), (c, [inf, 0, 0]), ([math.nan, 0.5, 0.5], [1, 0, 0]), ([0.5, -inf, 0.5], [1, 0, 0])):
		assert _one(o, d, dt) == (inf, -1, [0, 0, 0]), (o, d)
	assert _one(c, [1, 0, 0], dt)[:2] == (0.5, 2)


# ------------------------------------------------------------------ watertightness
def _template(n):
	from find_amd import synthetic
	v, f = synthetic.template(n)
	return v.numpy().astype(np.float32), f.numpy()


def test_watertight_on_the_closed_template_and_the_triple_products_leak():
	v, f = _template(6890)
	o, d = ref.aimed_rays(v, f)
	assert len(o) == 9842 and np.array_equal(d[:6890], v - o[:6890])   # (the corner at the target equals d bit for bit)
	misses = {}
	for name, dt, naive in (('float32', np.float32, False), ('float64', np.float64, False), ('float32 triple products', np.float32, True)):
		t, idx, bary = ref.cast(o, d, v, f, dt, naive=naive)
		misses[name] = int((~np.isfinite(t)).sum())
		hit = np.isfinite(t)
		assert (np.abs(t[hit] - 1) <= 1e-5).all() and (idx[hit] >= 0).all() and (idx[~hit] == -1).all()
		if not naive:   # the face that is hit holds the target vertex
			assert (f[idx[:6890]] == np.arange(6890)[:, None]).any(1).all()
	print('rays that miss the closed template(6890), of 9842:', misses)
	assert misses['float32'] == 0 and misses['float64'] == 0
	assert misses['float32 triple products'] >= 1   # the inputs have teeth


# ------------------------------------------------------------------ visibility
def ellipsoid_case(rings=25, segs=40, centre=(0.5, 0., 0.)):
	"""(verts, faces, centre, h, margin) of an ellipsoid seen from `centre` (+x by default).  h = n . (C - v) with n the ANALYTIC unit normal of the ellipsoid at the vertex:
	the height of the camera over the tangent plane.  The mesh is the convex hull of points on the ellipsoid, so vertex v is seen iff C - v
	leaves the cone of the faces at v, i.e. iff n_f . (C - v) > 0 for one of them, and n_f . (C - v) = h + (n_f - n) . (C - v).  With
	delta_v the largest |n_f - n| over the faces at v -- the angle between a face and the tangent plane at its corner, 4 sagitta / edge for
	a chord of a circle -- a vertex with h > margin_v = delta_v |C - v| is seen and one with h < -margin_v is not.  margin is per vertex."""
	from find_amd import synthetic
	v, f = synthetic.ellipsoid_mesh(rings, segs)
	v, f = v.numpy().astype(np.float32), f.numpy()
	axes = np.array([0.12, 0.045, 0.04])
	n = v.astype(np.float64) / axes ** 2
	n /= np.linalg.norm(n, axis=1, keepdims=True)
	tri = v[f].astype(np.float64)
	nf = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
	nf /= np.linalg.norm(nf, axis=1, keepdims=True)
	delta = np.zeros(len(v))
	np.maximum.at(delta, f.ravel(), np.linalg.norm(nf[:, None] - n[f], axis=-1).ravel())
	C = np.array(centre, np.float32)
	return v, f, C, (n * (C - v)).sum(1), delta * np.linalg.norm(C - v, axis=1)


def test_visibility_rule_on_an_ellipsoid():
	v, f, C, h, margin = ellipsoid_case()
	seen_side, far_side = h > margin, h < -margin
	print(f'ellipsoid (25, 40) from +x: margins {margin.min():.4f} .. {margin.max():.4f} m, {seen_side.sum()} vertices above theirs, {far_side.sum()} below, {len(v)} in all')
	assert seen_side.sum() >= 0.2 * len(v) and far_side.sum() >= 0.3 * len(v)   # (a condition on the inputs: the margins leave most vertices decided)
	for dt in DTYPES:
		vis = ref.visibility(v, f, C, dt)
		assert vis[seen_side].all() and not vis[far_side].any(), dt
	# the library's camera convention: p_view = p_world @ R + T, so C = -T @ R^T (pure torch, no device needed)
	from find_amd import rays
	g = torch.Generator().manual_seed(0)
	R = torch.linalg.qr(torch.randn(4, 3, 3, generator=g, dtype=torch.float64))[0]
	T = torch.randn(4, 3, generator=g, dtype=torch.float64)
	centres = rays.camera_centres(R, T)
	assert centres.shape == (4, 3) and ((centres[:, None, :] @ R)[:, 0] + T).abs().max() <= 1e-12


def test_hemisphere_directions_and_frames():
	from find_amd import rays
	for n in (1, 16, 64):
		d = rays.hemisphere_directions(n)
		assert d.shape == (n, 3) and d.dtype == torch.float32 and torch.equal(d, rays.hemisphere_directions(n))
		assert ((d.norm(dim=1) - 1).abs() <= 1e-6).all() and (d[:, 2] > 0).all()
	# cosine-distributed: the mean of cos(theta) is 2 / 3, the mean direction is the pole
	d = rays.hemisphere_directions(4096).double()
	assert abs(d[:, 2].mean().item() - 2 / 3) <= 1e-3 and d[:, :2].mean(0).abs().max().item() <= 1e-3
	g = torch.Generator().manual_seed(3)
	nrm = torch.randn(100, 3, generator=g) * 3
	nrm[:3] = torch.eye(3)
	t1, t2, n = rays.normal_frames(nrm)
	for a, b in ((t1, t2), (t1, n), (t2, n)):
		assert ((a * b).sum(-1).abs() <= 1e-6).all()
	assert all(((x.norm(dim=-1) - 1).abs() <= 1e-6).all() for x in (t1, t2, n)) and ((torch.linalg.cross(t1, t2) - n).abs() <= 1e-6).all()
	assert ((n * nrm).sum(-1) > 0).all()


# ------------------------------------------------------------------ the C side, before any launch
def _pairs():
	"""A few hundred (ray, face) pairs on template(1002): rays aimed at vertices and edge midpoints against the faces at the target and the
	face the restatement hits, box rays against the face they hit and its neighbours in the list, and the rules' corner cases."""
	v, f = _template(1002)
	rows = []
	o, d = ref.aimed_rays(v, f, every=40)
	pick = np.r_[0:len(v):37, len(v):len(o)]
	_, hit, _ = ref.cast(o[pick], d[pick], v, f, np.float32)
	for r, h in zip(pick, hit):
		at = np.nonzero((f == r).any(1))[0] if r < len(v) else np.array([], int)
		for j in set(at.tolist()) | {int(h), (int(h) + 1) % len(f), (7 * int(r)) % len(f)}:
			rows.append(np.concatenate([o[r], d[r], v[f[j]].ravel(), [0, np.inf]]))
	o, d = ref.box_rays(v, 60, 0.02, 5)
	t, hit, _ = ref.cast(o, d, v, f, np.float32)
	for r in range(len(o)):
		for j in {max(int(hit[r]), 0), (max(int(hit[r]), 0) + 1) % len(f)}:
			for t_min, t_max in ((0, np.inf), (0, t[r] if np.isfinite(t[r]) else 1), (t[r] if np.isfinite(t[r]) else 0, np.inf), (0, np.float32(0.5) * min(t[r], 1))):
				rows.append(np.concatenate([o[r], d[r], v[f[j]].ravel(), [t_min, t_max]]))
	tri = v[f[10]].ravel()
	for o_, d_ in ((v[f[10, 0]], [0, 0, 1]), ([0, 0, 0], [0, 0, 0]), ([0, 0, 0], [np.nan, 1, 0]), ([np.inf, 0, 0], [1, 0, 0]), (v[f[10, 1]] - [0, 0, 1], [0, 0, 1]),
				   (v[f[10]].mean(0) - [0, 0, 1], [0, 0, 1]), (v[f[10]].mean(0) + [0, 0, 1], [0, 0, -3]), (v[f[10, 0]], v[f[10, 1]] - v[f[10, 0]])):
		rows.append(np.concatenate([o_, d_, tri, [0, np.inf]]))
	return np.array(rows, np.float32)


def test_host_build_of_the_pair_arithmetic():
	"""csrc/raycast_math.h -- the functions raycast.hip compiles for the device -- built for the host and run by tools/raycast_host_check.cpp: its
	own closed forms, and the pairs of _pairs() bit for bit against the float32 restatement."""
	cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++') if c and os.path.exists(c)), None)
	assert cxx is not None, 'no host C++ compiler'
	pairs = _pairs()
	assert pairs.shape[1] == 17 and len(pairs) >= 300
	with tempfile.TemporaryDirectory() as tmp:
		exe = os.path.join(tmp, 'raycast_host_check')
		subprocess.run([cxx, '-std=c++17', '-O1', '-ffp-contract=off', '-I', os.path.join(ROOT, 'find_amd', 'csrc'), os.path.join(ROOT, 'tools', 'raycast_host_check.cpp'),
						'-o', exe], check=True, capture_output=True)
		r = subprocess.run([exe], capture_output=True, text=True)
		assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:]
		pairs.tofile(os.path.join(tmp, 'in.bin'))
		r = subprocess.run([exe, 'pairs', os.path.join(tmp, 'in.bin'), os.path.join(tmp, 'out.bin')], capture_output=True, text=True)
		assert r.returncode == 0, r.stdout[-2000:]
		got = np.fromfile(os.path.join(tmp, 'out.bin'), np.float32).reshape(-1, 5)
	assert len(got) == len(pairs)
	want = np.zeros_like(got)
	for i, p in enumerate(pairs):
		t, idx, bary = ref.cast(p[None, 0:3], p[None, 3:6], p[6:15].reshape(3, 3), np.array([[0, 1, 2]]), np.float32, t_min=p[15], t_max=p[16])
		if idx[0] == 0:
			want[i] = [1, t[0], *bary[0]]
	print(f'{len(pairs)} pairs, {int(want[:, 0].sum())} hits')
	assert 100 <= want[:, 0].sum() <= len(pairs) - 100
	assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0][:10]


def test_header_binding_workspace_and_refusals():
	from find_amd import _lib
	hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'find_hip.h')).read(), flags=re.S)
	for name, n_args in (('find_ray_ws_bytes', 3), ('find_ray_fwd', 21), ('find_ray_bwd', 17)):
		assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args
		decl = re.search(r'\b' + name + r'\(([^;]*)\);', hdr)
		assert decl and len(decl.group(1).split(',')) == n_args, name
	L = _lib.lib()
	# one 64-bit key per ray, whatever the face count
	assert L.find_ray_ws_bytes(16, 5000, 13776) == 16 * 5000 * 8 and L.find_ray_ws_bytes(1, 1, 0) == 256 and L.find_ray_ws_bytes(0, 0, 0) == 256
	assert L.find_ray_ws_bytes(3, 100, 5) == 2560 and L.find_ray_ws_bytes(3, 100, 1 << 20) == 2560
	assert L.find_ray_ws_bytes(1 << 16, 1, 1) == -1 and L.find_ray_ws_bytes(1, 1 << 30, 1) == -1 and L.find_ray_ws_bytes(1, 1, -1) == -1
	one = torch.zeros(64)   # (host memory: every call below is refused before it would be read)
	p = _lib.ptr(one)
	inf = math.inf

	def fwd(origins=p, dirs=p, r_len=None, skip=None, verts=p, faces=p, fb=1, N=1, R=1, V=1, F=1, t_min=0., t_max=inf, any_hit=0, t=p, idx=p, bary=p, hit=None, ws=p,
			ws_bytes=256):
		return L.find_ray_fwd(origins, dirs, r_len, skip, verts, faces, fb, N, R, V, F, t_min, t_max, any_hit, t, idx, bary, hit, ws, ws_bytes, None)
	for kw, word in ((dict(origins=None), b'NULL'), (dict(dirs=None), b'NULL'), (dict(ws=None), b'NULL'), (dict(t=None), b'NULL'), (dict(idx=None), b'NULL'),
					 (dict(bary=None), b'NULL'), (dict(any_hit=1), b'NULL'), (dict(verts=None), b'NULL'), (dict(faces=None), b'NULL'), (dict(fb=2, N=3), b'faces_batch'),
					 (dict(V=0), b'without vertices'), (dict(R=1 << 30), b'bad sizes'), (dict(N=1 << 16), b'bad sizes'), (dict(F=-1), b'bad sizes'),
					 (dict(t_min=-1e-9), b't_min'), (dict(t_min=math.nan), b't_min'), (dict(t_max=math.nan), b't_max'), (dict(any_hit=2), b'any_hit')):
		assert fwd(**kw) == -1 and word in L.find_last_error(), (kw, L.find_last_error())
	assert fwd(N=2, R=5000, V=4, F=13776) == -2 and b'workspace' in L.find_last_error()
	assert fwd(origins=None, dirs=None, verts=None, faces=None, N=0, R=5, V=0, F=0, t=None, idx=None, bary=None, ws=None, ws_bytes=0) == 0   # no mesh: nothing to do
	assert fwd(origins=None, dirs=None, N=3, R=0, t=None, idx=None, bary=None, ws=None, ws_bytes=0) == 0   # no ray

	def bwd(origins=p, dirs=p, verts=p, faces=p, fb=1, idx=p, bary=p, t=p, d_t=p, N=1, R=1, V=1, F=1, d_o=p, d_d=p, d_v=p):
		return L.find_ray_bwd(origins, dirs, verts, faces, fb, idx, bary, t, d_t, N, R, V, F, d_o, d_d, d_v, None)
	for kw, word in ((dict(origins=None), b'NULL'), (dict(dirs=None), b'NULL'), (dict(idx=None), b'NULL'), (dict(bary=None), b'NULL'), (dict(t=None), b'NULL'),
					 (dict(d_t=None), b'NULL'), (dict(verts=None), b'NULL'), (dict(faces=None), b'NULL'), (dict(d_o=None, d_d=None, d_v=None), b'gradient output'),
					 (dict(fb=2, N=3), b'faces_batch'), (dict(R=1 << 30), b'bad sizes'), (dict(V=-1), b'bad sizes')):
		assert bwd(**kw) == -1 and word in L.find_last_error(), (kw, L.find_last_error())
	assert bwd(origins=None, dirs=None, verts=None, faces=None, idx=None, bary=None, t=None, d_t=None, N=0) == 0


def test_cpu_tensors_and_bad_shapes_raise_with_the_functions_name():
	from find_amd import rays
	v, f = (torch.from_numpy(x) for x in _template(1002))
	v, o = v[None], torch.zeros(1, 5, 3)
	d = torch.ones(1, 5, 3)
	R, T = torch.eye(3)[None], torch.tensor([[0., 0., 0.5]])
	calls = (('ray_mesh_intersect', lambda: rays.ray_mesh_intersect(o, d, v, f)), ('ray_occluded', lambda: rays.ray_occluded(o, d, v, f)),
			 ('vertex_visibility', lambda: rays.vertex_visibility(v, f, R, T)), ('ambient_occlusion', lambda: rays.ambient_occlusion(o, d, v, f)),
			 ('vertex_ambient_occlusion', lambda: rays.vertex_ambient_occlusion(v, f)))
	for name, call in calls:
		with pytest.raises(RuntimeError, match=f'find_amd.rays.{name}: .*no CPU fallback'):
			call()
	bad = (('ray_mesh_intersect', lambda: rays.ray_mesh_intersect(o[0], d[0], v, f)), ('ray_mesh_intersect', lambda: rays.ray_mesh_intersect(o, d[:, :4], v, f)),
		   ('ray_mesh_intersect', lambda: rays.ray_mesh_intersect(o, d, v.expand(2, -1, -1), f)), ('ray_occluded', lambda: rays.ray_occluded(o, d, v, f[:, :2])),
		   ('ray_occluded', lambda: rays.ray_occluded(o, d, v, f.float())), ('ray_occluded', lambda: rays.ray_occluded(o, d, v, f[None].expand(3, -1, -1))),
		   ('vertex_visibility', lambda: rays.vertex_visibility(v[0], f, R, T)), ('vertex_visibility', lambda: rays.vertex_visibility(v, f, R, T[0])),
		   ('ambient_occlusion', lambda: rays.ambient_occlusion(o, d[:, :4], v, f)), ('vertex_ambient_occlusion', lambda: rays.vertex_ambient_occlusion(v[0], f)))
	for name, call in bad:
		with pytest.raises(RuntimeError, match=f'find_amd.rays.{name}: .*expected'):
			call()


def test_signatures_and_the_module_of_its_own():
	from find_amd import bake, rays
	for fn in (rays.ray_mesh_intersect, rays.ray_occluded):
		sig = inspect.signature(fn).parameters
		assert list(sig) == ['origins', 'dirs', 'verts', 'faces', 'r_len', 'skip', 't_min', 't_max']
		assert (sig['r_len'].default, sig['skip'].default, sig['t_min'].default, sig['t_max'].default) == (None, None, 0.0, math.inf)
	assert list(inspect.signature(rays.vertex_visibility).parameters) == ['verts', 'faces', 'R', 'T']
	sig = inspect.signature(rays.ambient_occlusion).parameters
	assert list(sig) == ['points', 'normals', 'verts', 'faces', 'n_dirs', 'max_dist', 'skip', 'rays_per_call']
	assert (sig['n_dirs'].default, sig['max_dist'].default, sig['skip'].default, sig['rays_per_call'].default) == (64, None, None, 1 << 20)
	assert list(inspect.signature(rays.vertex_ambient_occlusion).parameters)[:2] == ['verts', 'faces']
	sig = inspect.signature(bake.bake_ambient_occlusion).parameters
	assert list(sig) == ['plan', 'verts', 'faces', 'n_dirs', 'max_dist', 'fill'] and (sig['n_dirs'].default, sig['max_dist'].default, sig['fill'].default) == (64, None, 1.0)
	# the poison census of tests/test_poison_host.py walks four modules; find_amd.rays allocates and is none of them (tests/test_gpu_rays.py
	# poisons its allocations itself)
	from poison import MODULES
	from test_poison_host import allocating_ops
	assert 'find_amd.rays' not in MODULES and '_cast' in allocating_ops(os.path.join(ROOT, 'find_amd', 'rays.py'))
