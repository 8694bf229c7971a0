"""The mesh BVH on the host: the header, the binding and the built library agree on the new symbols; find_bvh_bytes; what every entry point
refuses before a launch; and tools/bvh_host_check.cpp -- the tree of csrc/bvh.hip built on the host from csrc/bvh_math.h and walked with
csrc/raycast_math.h's pair test -- against brute force over the same faces.

There is no tolerance in this file: the walk must give brute force's (t bits, face) on every ray, the any_hit walk must give "something was
hit", and every pair that brute force accepts must pass box_hit for every box above its face with t_hi lowered to the pair's own t.  The
counts asked are 0."""
import math
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import inside_ref   # noqa: E402
import rays_ref as ref   # noqa: E402


# ------------------------------------------------------------------ the C side, before any launch
def test_header_binding_and_library_agree():
	from find_amd import _lib, rays
	hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'find_hip.h')).read(), flags=re.S)
	L = _lib.lib()
	for name, n_args in (('find_bvh_bytes', 2), ('find_bvh_keys', 10), ('find_bvh_build', 10), ('find_bvh_refit', 9), ('find_ray_bvh_fwd', 23)):
		assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
		decl = re.search(r'\b' + name + r'\(([^;]*)\);', hdr)
		assert decl and len(decl.group(1).split(',')) == n_args, name
		assert hasattr(L, name)
	# find_ray_bvh_fwd is find_ray_fwd with the structure and its size in front of the workspace
	a, b = _lib.PROTOTYPES['find_ray_fwd'][1], _lib.PROTOTYPES['find_ray_bvh_fwd'][1]
	assert b[:18] == a[:18] and b[20:] == a[18:]
	leaf, arity = (int(re.search(r'#define\s+' + n + r'\s+(\d+)', hdr).group(1)) for n in ('FIND_BVH_LEAF', 'FIND_BVH_ARITY'))
	assert (rays.BVH_LEAF, rays.BVH_ARITY) == (leaf, arity) and leaf >= 1 and arity >= 2


def test_bvh_bytes():
	from find_amd import _lib, rays
	L = _lib.lib()
	assert L.find_bvh_bytes(1 << 16, 1) == -1 and L.find_bvh_bytes(1, 1 << 30) == -1 and L.find_bvh_bytes(-1, 1) == -1 and L.find_bvh_bytes(1, -1) == -1
	sizes = [L.find_bvh_bytes(1, F) for F in range(0, 3000)]
	assert all(b >= a > 0 for a, b in zip(sizes, sizes[1:])) and sizes == [L.find_bvh_bytes(1, F) for F in range(0, 3000)]
	assert L.find_bvh_bytes(0, 0) > 0 and L.find_bvh_bytes(3, 13776) == 3 * L.find_bvh_bytes(1, 13776) and L.find_bvh_bytes(1, (1 << 30) - 1) > L.find_bvh_bytes(1, 1 << 20)
	# the order (int32 per face) and a box (32 bytes) per leaf at least
	for F in (1, 100, 13776, 100000):
		assert L.find_bvh_bytes(1, F) >= 4 * F + 32 * math.ceil(F / rays.BVH_LEAF)
	# the size changes only where the padded leaf count does
	A, Lf = rays.BVH_ARITY, rays.BVH_LEAF
	for k in (1, 2, 3):
		assert L.find_bvh_bytes(1, Lf * A ** k) == L.find_bvh_bytes(1, Lf * A ** (k - 1) + 1) < L.find_bvh_bytes(1, Lf * A ** k + 1)


def test_refusals_before_any_launch():
	from find_amd import _lib
	L = _lib.lib()
	one = torch.zeros(64)   # (host memory: every call below is refused before it would be read)
	p = _lib.ptr(one)
	inf = math.inf
	big = L.find_bvh_bytes(3, 13776)

	def keys(verts=p, faces=p, fb=1, N=1, V=1, F=1, keys=p, bvh=p, nbytes=big):
		return L.find_bvh_keys(verts, faces, fb, N, V, F, keys, bvh, nbytes, None)

	def build(verts=p, faces=p, fb=1, N=1, V=1, F=1, keys=p, bvh=p, nbytes=big):
		return L.find_bvh_build(verts, faces, fb, N, V, F, keys, bvh, nbytes, None)

	def refit(verts=p, faces=p, fb=1, N=1, V=1, F=1, keys=None, bvh=p, nbytes=big):
		return L.find_bvh_refit(verts, faces, fb, N, V, F, bvh, nbytes, None)
	for fn, name in ((keys, b'find_bvh_keys'), (build, b'find_bvh_build'), (refit, b'find_bvh_refit')):
		cases = [(dict(verts=None), b'NULL'), (dict(faces=None), b'NULL'), (dict(bvh=None), b'NULL'), (dict(fb=2, N=3), b'faces_batch'), (dict(fb=0), b'faces_batch'),
				 (dict(V=0), b'without vertices'), (dict(N=1 << 16), b'bad sizes'), (dict(F=1 << 30), b'bad sizes'), (dict(F=-1), b'bad sizes'), (dict(V=-1), b'bad sizes')]
		if fn is not refit:
			cases.append((dict(keys=None), b'NULL'))
		for kw, word in cases:
			assert fn(**kw) == -1 and word in L.find_last_error() and name in L.find_last_error(), (name, kw, L.find_last_error())
		assert fn(N=3, V=4, F=13776, nbytes=big - 1) == -2 and b'too small' in L.find_last_error() and name in L.find_last_error()
		assert fn(verts=None, faces=None, keys=None, bvh=None, N=0, V=0, F=0, nbytes=0) == 0   # no mesh: nothing to do

	def fwd(origins=p, dirs=p, r_len=None, skip=None, verts=p, faces=p, fb=1, N=1, R=1, V=1, F=1, t_min=0., t_max=inf, any_hit=0, t=p, idx=p, bary=p, hit=None, bvh=p,
			nbytes=big, ws=p, ws_bytes=256):
		return L.find_ray_bvh_fwd(origins, dirs, r_len, skip, verts, faces, fb, N, R, V, F, t_min, t_max, any_hit, t, idx, bary, hit, bvh, nbytes, ws, ws_bytes, None)
	for kw, word in ((dict(origins=None), b'NULL'), (dict(dirs=None), b'NULL'), (dict(ws=None), b'NULL'), (dict(t=None), b'NULL'), (dict(idx=None), b'NULL'),
					 (dict(bary=None), b'NULL'), (dict(any_hit=1), b'NULL'), (dict(verts=None), b'NULL'), (dict(faces=None), b'NULL'), (dict(bvh=None), b'NULL'),
					 (dict(fb=2, N=3), b'faces_batch'), (dict(V=0), b'without vertices'), (dict(R=1 << 30), b'bad sizes'), (dict(N=1 << 16), b'bad sizes'),
					 (dict(F=-1), b'bad sizes'), (dict(t_min=-1e-9), b't_min'), (dict(t_min=math.nan), b't_min'), (dict(t_max=math.nan), b't_max'), (dict(any_hit=2), b'any_hit')):
		assert fwd(**kw) == -1 and word in L.find_last_error() and b'find_ray_bvh_fwd' in L.find_last_error(), (kw, L.find_last_error())
	assert fwd(N=2, R=5000, V=4, F=13776) == -2 and b'workspace' in L.find_last_error()
	assert fwd(N=3, V=4, F=13776, nbytes=big - 1, ws_bytes=1 << 20) == -2 and b'structure' in L.find_last_error()
	assert fwd(origins=None, dirs=None, verts=None, faces=None, bvh=None, N=0, R=5, V=0, F=0, t=None, idx=None, bary=None, ws=None, ws_bytes=0, nbytes=0) == 0
	assert fwd(origins=None, dirs=None, N=3, R=0, t=None, idx=None, bary=None, ws=None, ws_bytes=0) == 0


def test_cpu_tensors_and_a_structure_of_other_shapes_raise():
	import pytest
	from find_amd import bake, rays   # noqa: F401
	v = torch.rand(1, 8, 3)
	f = torch.tensor([[0, 1, 2], [2, 3, 4]])
	o, d = torch.zeros(1, 5, 3), torch.ones(1, 5, 3)
	with pytest.raises(RuntimeError, match='find_amd.rays.build_bvh: .*no CPU fallback'):
		rays.build_bvh(v, f)
	for name, call in (('ray_mesh_intersect', lambda: rays.ray_mesh_intersect(o, d, v, f, accel='bvh')), ('ray_occluded', lambda: rays.ray_occluded(o, d, v, f, accel='bvh')),
					   ('vertex_visibility', lambda: rays.vertex_visibility(v, f, torch.eye(3)[None], torch.zeros(1, 3), accel='bvh')),
					   ('ambient_occlusion', lambda: rays.ambient_occlusion(o, d, v, f, accel='bvh')),
					   ('vertex_ambient_occlusion', lambda: rays.vertex_ambient_occlusion(v, f, accel='bvh'))):
		with pytest.raises(RuntimeError, match=f'find_amd.rays.{name}: .*no CPU fallback'):
			call()
	with pytest.raises(RuntimeError, match="accel"):
		rays.ray_mesh_intersect(o, d, v, f, accel='grid')
	with pytest.raises(RuntimeError, match='expected'):
		rays.build_bvh(v[0], f)


# ------------------------------------------------------------------ the host checker
def _snap(o, lo, hi, rng):
	"""Every origin gets one coordinate moved onto a plane of the box [lo, hi]."""
	o = o.copy()
	k = rng.randint(0, 3, len(o))
	o[np.arange(len(o)), k] = np.where(rng.rand(len(o)) < 0.5, lo[k], hi[k])
	return o


def _case(v, f, n_box, seed, every=1):
	"""(verts, faces, rays (R, 8), skip (R)) of one mesh: box rays; rays from the vertex mean at every vertex and every `every`-th edge
	midpoint; from outside the box at the same targets; axis-parallel rays (two zero components) and rays with one zero component, half of
	them starting ON a plane of the mesh's box (and so lying in it when the zero component is that axis); the first rays again with t_max,
	and with t_min, set to the float32 restatement's t of their hit; and again with the face they hit skipped."""
	v, f = np.ascontiguousarray(v, np.float32), np.asarray(f, np.int64)
	rng = np.random.RandomState(seed)
	used = v[np.unique(f[ref.valid_faces(f, len(v))])]
	used = used[np.isfinite(used).all(1)]
	lo, hi = used.min(0), used.max(0)
	o0, d0 = ref.box_rays(used, n_box, 0.02, seed)
	fv = f[ref.valid_faces(f, len(v)) & np.isfinite(v[np.clip(f, 0, len(v) - 1)]).all((1, 2))]
	o1, d1 = ref.aimed_rays(np.where(np.isfinite(v), v, 0).astype(np.float32), fv, every=every)
	outside = (lo - np.float32(0.03) - (hi - lo) * np.float32(0.1)).astype(np.float32)
	o2 = np.broadcast_to(outside, o1.shape).copy()
	d2 = (o1 + d1) - o2
	n_ax = max(n_box // 2, 60)
	o3 = (lo + rng.rand(n_ax, 3) * (hi - lo)).astype(np.float32)
	o3[n_ax // 2:] = _snap(o3[n_ax // 2:], lo, hi, rng)
	d3 = np.zeros((n_ax, 3), np.float32)
	d3[np.arange(n_ax), rng.randint(0, 3, n_ax)] = rng.choice([-1., 0.5, 2.], n_ax)
	o3[::2] -= d3[::2] * np.float32(3)   # half of them from outside, along the axis
	o4 = (lo - 0.02 + rng.rand(n_ax, 3) * (hi - lo + 0.04)).astype(np.float32)
	o4[n_ax // 2:] = _snap(o4[n_ax // 2:], lo, hi, rng)
	d4 = ((lo + rng.rand(n_ax, 3) * (hi - lo)).astype(np.float32) - o4)
	d4[np.arange(n_ax), rng.randint(0, 3, n_ax)] = 0
	o, d = np.concatenate([o0, o1, o2, o3, o4]), np.concatenate([d0, d1, d2, d3, d4])
	t_min, t_max, skip = np.zeros(len(o), np.float32), np.full(len(o), np.inf, np.float32), np.full(len(o), -1, np.int32)
	# the interval's ends and the skip face, on a sample of every group
	pick = np.unique(np.concatenate([np.arange(0, len(o), max(len(o) // 300, 1)), np.arange(len(o0), len(o0) + min(len(o1), 60))]))
	t, idx, _ = ref.cast(o[pick], d[pick], np.where(np.isfinite(v), v, 0).astype(np.float32), fv, np.float32)
	hit = np.isfinite(t)
	assert hit.sum() >= 20, hit.sum()
	oh, dh, th = o[pick][hit], d[pick][hit], t[hit]
	# (fv's indices are not f's where invalid rows were dropped: the skip group is added only when they are the same list)
	groups = [(oh, dh, np.zeros_like(th), th, np.full(len(th), -1)), (oh, dh, th, np.full_like(th, np.inf), np.full(len(th), -1)),
			  (oh, dh, np.zeros_like(th), np.nextafter(th, np.float32(0)), np.full(len(th), -1))]
	if len(fv) == len(f):
		groups.append((oh, dh, np.zeros_like(th), np.full_like(th, np.inf), idx[hit]))
	for go, gd, ga, gb, gs in groups:
		o, d, t_min, t_max, skip = np.concatenate([o, go]), np.concatenate([d, gd]), np.concatenate([t_min, ga]), np.concatenate([t_max, gb]), np.concatenate([skip, gs.astype(np.int32)])
	rays_ = np.concatenate([o, d, t_min[:, None], t_max[:, None]], 1).astype(np.float32)
	return v, f.astype(np.int32), rays_, skip.astype(np.int32)


def _cases():
	from find_amd import synthetic
	out = {}
	tv, tf = (x.numpy() for x in synthetic.template(1002))
	out['template(1002)'] = _case(tv, tf, 1500, 1)
	out['cube'] = _case(inside_ref.CUBE_VERTS, inside_ref.CUBE_FACES, 400, 2)
	v2 = np.array([[0.04, -0.03, 0.01], [-0.04, 0.03, 0.02], [0.03, 0.04, -0.02], [-0.03, -0.04, -0.01]])
	out['two'] = _case(v2, np.array([[0, 1, 2], [1, 0, 3]]), 400, 3)
	n = 9   # a planar grid in z = 0: no extent on one axis
	gx, gy = np.meshgrid(np.arange(n) * 0.01, np.arange(n) * 0.0125, indexing='ij')
	gv = np.stack([gx.ravel(), gy.ravel(), np.zeros(n * n)], 1)
	q = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None]).ravel()
	gf = np.concatenate([np.stack([q, q + n, q + n + 1], 1), np.stack([q, q + n + 1, q + 1], 1)])
	out['grid in z = 0'] = _case(gv, gf, 400, 4)
	# every fifth face of an ellipsoid a second time at the end of the list: equal t on two indices, the smaller must win
	ev, ef = (x.numpy() for x in synthetic.ellipsoid_mesh(8, 12))
	out['duplicated faces'] = _case(ev, np.concatenate([ef, ef[::5]]), 400, 5)
	# -1 rows, indices out of range and a vertex that is not finite: invalid faces sort last and are in no box
	bv, bf = ev.copy(), np.concatenate([ef[:40], [[-1, -1, -1], [0, 1, len(ev)], [-3, 2, 1]], ef[40:], [[-1, -1, -1]]])
	bv[7] = np.nan
	out['invalid faces'] = _case(bv, bf, 400, 6)
	out['one face'] = _case(v2, np.array([[0, 1, 2]]), 200, 7)
	return out


def test_host_walk_equals_brute_force():
	"""tools/bvh_host_check.cpp: its closed forms, then the cases of _cases(): 0 differences of the walk from brute force, 0 of the any_hit walk,
	0 accepted pairs behind a box that box_hit refuses."""
	cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++') if c and os.path.exists(c)), None)
	assert cxx is not None, 'no host C++ compiler'
	cases = _cases()
	with tempfile.TemporaryDirectory() as tmp:
		exe = os.path.join(tmp, 'bvh_host_check')
		subprocess.run([cxx, '-std=c++17', '-O1', '-ffp-contract=off', '-I', os.path.join(ROOT, 'find_amd', 'csrc'), os.path.join(ROOT, 'tools', 'bvh_host_check.cpp'),
						'-o', exe], check=True, capture_output=True)
		r = subprocess.run([exe], capture_output=True, text=True)
		assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:]
		with open(os.path.join(tmp, 'in.bin'), 'wb') as fh:
			fh.write(np.int32(len(cases)).tobytes())
			for v, f, rays_, skip in cases.values():
				fh.write(np.array([len(v), len(f), len(rays_)], np.int32).tobytes())
				for x in (v, f, rays_, skip):
					fh.write(np.ascontiguousarray(x).tobytes())
		r = subprocess.run([exe, 'cases', os.path.join(tmp, 'in.bin')], capture_output=True, text=True)
	print(r.stdout)
	lines = [ln for ln in r.stdout.splitlines() if ln.startswith('case ')]
	assert r.returncode == 0 and r.stdout.strip().endswith('ok') and len(lines) == len(cases), r.stdout[-3000:]
	for name, ln in zip(cases, lines):
		m = re.search(r'(\d+) rays, (\d+) hit, (\d+) accepted pairs; differences (\d+), any_hit (\d+), pairs behind a refused box (\d+)', ln)
		n_rays, hit, pairs, diff, diff_any, unreached = (int(x) for x in m.groups())
		assert n_rays == len(cases[name][2]) and (diff, diff_any, unreached) == (0, 0, 0), (name, ln)
		assert hit >= 0.2 * n_rays and hit < n_rays and pairs >= hit, (name, ln)   # (a condition on the inputs)
