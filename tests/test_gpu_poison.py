"""No HIP op may read memory it did not write: every op's public wrapper, forward and backward, run clean and with every torch.empty /
torch.empty_like / _ws of the wrappers returning memory filled with 0xFF (NaN, -1, ~0) and with 0x00 (tests/poison.py).

Per case: a discarded clean warm-up call in front of each of the three runs (same inputs, same switch bits), then
  * no poison survives: floats finite wherever the clean run's are, integers -1 or inside their op's range;
  * deterministic quantities equal the clean run's bit for bit (every forward but the shaded image, Chamfer keys and loss, smoothness,
    normal / depth / part / contrastive losses, PCA, registration, latents, optimiser, the MLP, and the fused surface-Chamfer backward
    while a cloud's targets fit one wave -- see _SURF_THREE for what happens past that);
  * float-atomic sums agree within the bound the suite already holds two correct runs of that op to (the `rel` / `abs` rules, each with
    its source), or, where the suite has none, within (n_row + 3) * 2^-24 * sum |addend| per row from a float64 restatement of the
    addends (poison.atomic_bound).  No tolerance is taken from the clean run.
Each case names (`ref`) the existing test that holds its clean result to a reference at or around its shape.

CASES is read on the CPU by tests/test_poison_host.py (the census: every allocating op of functional.py / functional_render.py is in
some case's `covers`), so this module imports without a device and builds its inputs lazily."""
import contextlib
import math
import os

import numpy as np
import pytest
import torch

from poison import BITS, Rule, atomic_bound, compare, poisoned

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')

# bounds the suite already holds two correct runs of an op to
CHAMFER_BWD = Rule(bits=False, rel=3e-5, floor=1e-12)     # test_gpu_chamfer_tiles.py: 3e-5 of the largest entry
IMAGE = Rule(bits=False, abs=1e-5)                        # test_gpu_render_features.py:338 / test_gpu_render.py: float-atomic vertex normals
FEAT_D_FEATURES = Rule(bits=False, rel=1e-5)              # test_gpu_render_features.py::test_rasterisers_and_list_switches_agree
FEAT_D_VERTS = Rule(bits=False, rel=5e-4)                 # the same test
SPLIT_BWD = Rule(bits=False, rel=1e-5)                    # test_gpu_render_zclip.py::test_split_mode_forward_is_bit_reproducible_and_backward_within_atomics_order
RENDER_BWD = Rule(bits=False, rel=1e-4)                   # test_gpu_render.py::test_early_exit_and_list_order_change_nothing: two runs of the backward, 1e-4 of the largest entry
# The whole step's parameter gradients: the suite holds no two runs of a step to each other, and a derived bound would have to follow every
# float atomic of the step through the MLP's backward.  BORROWED, not derived: the 1e-4 * max(1e-3, largest entry) that test_gpu_pipeline.py
# holds each run to the oracle with -- wider than two runs differ, far below what a poisoned buffer does (NaN, or a whole addend).
STEP_GRAD = Rule(bits=False, rel=1e-4, floor=1e-3)


class Case:
	"""name; covers: the allocating ops (autograd.Function classes and module-level functions) the case runs; build() -> inputs, called
	once; run(inputs) -> dict of outputs and gradients, through the public wrapper, forward plus backward; kind: 'bits' or 'atomics';
	bits: the profiling switch for all three runs; rules(inputs) -> {quantity: Rule} for what is not simply bit-equal; ref: the existing
	test that holds the clean result to a reference; check(inputs, r0): that comparison, done here, where the case's shape has none."""

	def __init__(self, name, covers, build, run, kind='bits', bits=0, rules=None, ref='', check=None):
		self.name, self.covers, self.build, self.run, self.kind, self.bits, self.rules, self.ref, self.check = name, tuple(covers), build, run, kind, bits, rules, ref, check
		self._inputs = None

	def inputs(self):
		if self._inputs is None:
			self._inputs = self.build()
		return self._inputs


CASES = []


def case(name, covers, build, run, **kw):
	CASES.append(Case(name, covers, build, run, **kw))


def _gen(seed):
	return torch.Generator().manual_seed(seed)


def _out(**kw):
	return {k: (None if v is None else v.detach().clone()) for k, v in kw.items()}


def _row_stats(rows, index, addend):
	"""(n_row, sum |addend|) of a scatter: index (..., K) rows of a (rows, 3) gradient, addend (..., K, 3) float64."""
	idx = index.reshape(-1).long()
	ok = idx >= 0
	a = addend.reshape(-1, 3).abs()[ok]
	n = torch.zeros(rows, dtype=torch.float64).index_add_(0, idx[ok], torch.ones(int(ok.sum()), dtype=torch.float64))
	s = torch.zeros(rows, 3, dtype=torch.float64).index_add_(0, idx[ok], a)
	return n, s


def _sample_bound(faces, face_idx, uv, g, n_verts):
	"""Bound of find_sample_points_bwd's d_verts: vertex faces[face_idx[s], c] receives w_c(uv_s) * g_s (geom.hip: bary_weights)."""
	N = face_idx.shape[0]
	out = []
	for m in range(N):
		f = (faces if faces.dim() == 2 else faces[m]).long()[face_idx[m].long()]
		us = uv[m, :, 0].double().sqrt()
		w = torch.stack([1 - us, us * (1 - uv[m, :, 1].double()), us * uv[m, :, 1].double()], dim=-1)
		n, s = _row_stats(n_verts, f, w[..., None] * g[m].double()[:, None, :])
		out.append(atomic_bound(n[:, None], s))
	return torch.stack(out)


# ================================================================================================ geometry and losses
def _geom_mesh(n=3, seed=0):
	from test_gpu_geom import _mesh
	return _mesh(1002, n=n, seed=seed)


# ---- face_areas, 7 padded faces (ref: test_gpu_geom.py::test_face_areas_and_sampling_vs_oracle, the same mesh and padding)
def _b_face_areas():
	verts, faces = _geom_mesh()
	fpad = torch.cat([faces, torch.full((7, 3), -1, dtype=faces.dtype)])[None].expand(3, -1, -1).contiguous()
	return verts.cuda(), fpad.cuda()


def _r_face_areas(i):
	from find_amd import functional as FN
	return _out(areas=FN.face_areas(*i))


case('face_areas, 7 padded faces', ['face_areas'], _b_face_areas, _r_face_areas, ref='test_gpu_geom.py::test_face_areas_and_sampling_vs_oracle')


# ---- sample_points forward + backward with attr, N = 2, S = 300 (ref: the same test, at S = 5000)
def _b_sample_points():
	verts, faces = _geom_mesh(n=2, seed=1)
	g = _gen(2)
	F = faces.shape[0]
	fi = torch.randint(0, F, (2, 300), generator=g)
	uv = torch.rand(2, 300, 2, generator=g)
	attr = torch.rand(verts.shape, generator=g)
	w1, w2 = torch.randn(2, 300, 3, generator=g), torch.randn(2, 300, 3, generator=g)
	return dict(verts=verts, faces=faces, fi=fi, uv=uv, attr=attr, w1=w1, w2=w2)


def _r_sample_points(i):
	from find_amd import functional as FN
	v, a = i['verts'].cuda().requires_grad_(True), i['attr'].cuda().requires_grad_(True)
	pts, cs = FN.sample_points(v, i['faces'].cuda(), i['fi'].cuda(), i['uv'].cuda(), a)
	((pts * i['w1'].cuda()).sum() + (cs * i['w2'].cuda()).sum()).backward()
	return _out(points=pts, attr=cs, d_verts=v.grad, d_attr=a.grad)


def _rules_sample_points(i):
	V = i['verts'].shape[1]
	return dict(d_verts=Rule(bits=False, bound=_sample_bound(i['faces'], i['fi'], i['uv'], i['w1'], V)),
				d_attr=Rule(bits=False, bound=_sample_bound(i['faces'], i['fi'], i['uv'], i['w2'], V)))


def _check_sample_points(i, r0):
	"""The oracle at this sample count, to that test's tolerances."""
	from oracle import geom_ref as G
	vr, ar = i['verts'].clone().requires_grad_(True), i['attr'].clone().requires_grad_(True)
	rp, rc = G.sample_points(vr, i['faces'], i['fi'], i['uv'], attr=ar)
	((rp * i['w1']).sum() + (rc * i['w2']).sum()).backward()
	assert (r0['points'] - rp.detach()).abs().max().item() < 1e-6 and (r0['attr'] - rc.detach()).abs().max().item() < 1e-6
	assert (r0['d_verts'] - vr.grad).abs().max().item() < 1e-4 * max(1.0, vr.grad.abs().max().item())
	assert (r0['d_attr'] - ar.grad).abs().max().item() < 1e-4 * max(1.0, ar.grad.abs().max().item())


case('sample_points with attr, 2 x 300', ['_SamplePoints'], _b_sample_points, _r_sample_points, kind='atomics', rules=_rules_sample_points,
	 ref='test_gpu_geom.py::test_face_areas_and_sampling_vs_oracle', check=_check_sample_points)


# ---- sample_surface / find_sample_surface_again, N = 3, S = 300, one mesh whose faces are all padding (forward: the mesh carries no gradient)
# (ref: test_gpu_geom.py::test_sample_surface_faces_follow_the_area_distribution, at S = 5000 with 5 padded faces)
def _b_sample_surface():
	verts, faces = _geom_mesh(n=3, seed=12)
	g = _gen(14)
	fp = torch.cat([faces, torch.full((5, 3), -1, dtype=faces.dtype)])[None].expand(3, -1, -1).contiguous().clone()
	fp[2] = -1   # a mesh without a face: total area 0, every draw falls back to face 0 and reads vertex max(-1, 0)
	return dict(verts=verts.cuda(), faces=fp.cuda(), rnd=torch.rand(3, 300, 3, generator=g).cuda(), attr=torch.rand(verts.shape, generator=g).cuda(), F=fp.shape[1])


def _r_sample_surface(i, again=False):
	from find_amd import functional as FN
	FN._AREA_SUMS.clear()
	FN._AREA_SUM_OWNERS.clear()
	for _ in range(2 if again else 1):   # (the second call of a mesh without gradient samples from the kept area sums)
		pts, cs, fi, uv = FN.sample_surface(i['verts'], i['faces'], i['rnd'], i['attr'])
	assert len(FN._AREA_SUMS) == 1
	return _out(points=pts, attr=cs, face_idx=fi, uv=uv)


def _rules_sample_surface(i):
	return dict(face_idx=Rule(irange=(0, i['F'])))


case('sample_surface, a mesh of padding only', ['_SampleSurface'], _b_sample_surface, _r_sample_surface, rules=_rules_sample_surface,
	 ref='test_gpu_geom.py::test_sample_surface_faces_follow_the_area_distribution')
case('sample_surface again, from the kept area sums', ['_SampleSurface'], _b_sample_surface, lambda i: _r_sample_surface(i, True), rules=_rules_sample_surface,
	 ref='test_gpu_geom.py::test_sample_surface_keeps_the_area_sums_of_meshes_without_gradient')


# ---- sample_surface on a mesh that takes a gradient (the autograd path), 5 padded faces, backward through find_sample_points_bwd
def _b_sample_surface_grad(empty_mesh=False):
	verts, faces = _geom_mesh(n=3, seed=12)
	g = _gen(15)
	fp = torch.cat([faces, torch.full((5, 3), -1, dtype=faces.dtype)])[None].expand(3, -1, -1).contiguous().clone()
	if empty_mesh:
		fp[2] = -1   # every draw of this mesh falls back to face 0, a -1 row: find_sample_points_bwd must skip it (its gradient: exactly zero)
	rnd = torch.rand(3, 300, 3, generator=g)
	# The face of every draw, in float64 (the first face whose running area sum exceeds draw * total; face 0 on a mesh without area), and
	# every face draw moved to the MIDDLE of its face's interval: half a face's share (2.5e-4 of the total) from either neighbour, where the
	# kernel's fp32 running sum (within 2e-6 of the total: test_sample_surface_faces_follow_the_area_distribution) selects the same face.
	# The bound below restates the addends from this selection: nothing of it comes from a run.
	v64, f = verts.double(), fp.clamp(min=0).long()
	tri = torch.stack([v64[m][f[m]] for m in range(3)])                                                  # (3, F, 3, 3)
	area = 0.5 * torch.linalg.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0]).norm(dim=-1) * (fp >= 0).all(-1)
	cdf = area.cumsum(1)
	total = cdf[:, -1:]
	fi = torch.searchsorted(cdf, rnd[..., 0].double() * total, right=True).clamp(max=fp.shape[1] - 1)
	mid = (torch.gather(cdf, 1, fi) - 0.5 * torch.gather(area, 1, fi)) / total.clamp(min=1e-300)
	has_area = (total > 0).expand_as(fi)
	rnd[..., 0] = torch.where(has_area, mid, rnd[..., 0].double()).float()
	fi = torch.where(has_area, fi, torch.zeros_like(fi))
	assert (torch.gather(area, 1, fi)[has_area] > 0).all()
	return dict(verts=verts, faces=fp, rnd=rnd, w=torch.randn(3, 300, 3, generator=g), F=fp.shape[1], fi=fi, empty_mesh=empty_mesh)


def _r_sample_surface_grad(i):
	from find_amd import functional as FN
	v = i['verts'].cuda().requires_grad_(True)
	pts, _, fi, uv = FN.sample_surface(v, i['faces'].cuda(), i['rnd'].cuda())
	(pts * i['w'].cuda()).sum().backward()
	return _out(points=pts, face_idx=fi, uv=uv, d_verts=v.grad)


def _rules_sample_surface_grad(i):
	return dict(face_idx=Rule(irange=(0, i['F'])),
				d_verts=Rule(bits=False, bound=_sample_bound(i['faces'], i['fi'], i['rnd'][..., 1:], i['w'], i['verts'].shape[1])))


def _check_sample_surface_grad(i, r0):
	assert torch.equal(r0['face_idx'].long(), i['fi']), 'the kernel chose other faces than the float64 running sum'
	if i['empty_mesh']:
		assert (r0['d_verts'][2] == 0).all(), 'a mesh without faces got a gradient'


case('sample_surface with gradient, 3 x 300', ['_SampleSurface'], _b_sample_surface_grad, _r_sample_surface_grad, kind='atomics', rules=_rules_sample_surface_grad,
	 ref='test_gpu_geom.py::test_sample_surface_faces_follow_the_area_distribution', check=_check_sample_surface_grad)
case('sample_surface with gradient, a mesh of padding only', ['_SampleSurface'], lambda: _b_sample_surface_grad(True), _r_sample_surface_grad, kind='atomics',
	 rules=_rules_sample_surface_grad, ref='test_gpu_geom.py::test_sample_surface_faces_follow_the_area_distribution', check=_check_sample_surface_grad)


# ---- knn1 forward + backward (ref: test_gpu_geom.py::test_nn_ragged_and_ties for the forward, ::test_knn1_backward_against_float64 for the backward)
def _b_knn1(name):
	def build():
		from oracle import geom_ref as G
		from test_gpu_geom import KNN1_BWD_CASES, knn1_bwd_reference
		x, y, xl, yl = KNN1_BWD_CASES[name]
		w = torch.randn(x.shape[:2], generator=_gen(6))
		_, idx = G.knn1(x, y, xl, yl)
		b_y = knn1_bwd_reference(x, y, idx, w)[3]
		return dict(x=x, y=y, xl=xl, yl=yl, w=w, b_y=b_y)
	return build


def _r_knn1(i):
	from find_amd import functional as FN
	x, y = i['x'].cuda().requires_grad_(True), i['y'].cuda().requires_grad_(True)
	d, idx = FN.knn1(x, y, i['xl'].cuda(), i['yl'].cuda())
	(d * i['w'].cuda()).sum().backward()
	return _out(dist=d, idx=idx, d_x=x.grad, d_y=y.grad)


def _rules_knn1(i):
	return dict(idx=Rule(irange=(0, i['y'].shape[1])), d_y=Rule(bits=False, bound=i['b_y']))


case('knn1 ragged, 3 x 300 x 200', ['_NN'], _b_knn1('ragged'), _r_knn1, kind='atomics', rules=_rules_knn1, ref='test_gpu_geom.py::test_knn1_backward_against_float64')
case('knn1 with a length of 0 on either side', ['_NN'], _b_knn1('no query, no target'), _r_knn1, kind='atomics', rules=_rules_knn1,
	 ref='test_gpu_geom.py::test_knn1_backward_against_float64')


# ---- chamfer_distance under each of its four routes (ref: test_gpu_chamfer_tiles.py::test_tile_path_equals_all_pairs_bit_for_bit[ragged] and
# test_gpu_geom.py::test_chamfer_with_an_empty_cloud / ::test_chamfer_fused_vs_oracle[(1, 777, 5000)])
def _b_chamfer_ragged():
	from test_gpu_chamfer_tiles import CASES as TILE_CASES
	x, y, xl, yl = TILE_CASES['ragged']
	return dict(x=x, y=y, xl=xl, yl=yl)


def _b_chamfer_split():
	n, p1, p2 = 1, 777, 5000   # batch 1: the targets are split over blocks, merged by 64-bit atomic minima into keys preset to 0xff
	g = _gen(p1 * 7 + p2 + n)
	return dict(x=torch.randn(n, p1, 3, generator=g) * 0.05, y=torch.randn(n, p2, 3, generator=g) * 0.05, xl=None, yl=None)


def _r_chamfer(i):
	from find_amd import functional as FN
	from test_gpu_chamfer_tiles import _keys
	x, y = i['x'].cuda().requires_grad_(True), i['y'].cuda().requires_grad_(True)
	xl, yl = (None if t is None else t.cuda() for t in (i['xl'], i['yl']))
	loss, _ = FN.chamfer_distance(x, y, xl, yl)
	n, p1, p2 = x.shape[0], x.shape[1], y.shape[1]
	kx, ky = _keys(loss.grad_fn.saved_tensors[2], n, p1, p2)   # (the forward's workspace: kx, then ky)
	kx, ky = kx.view(n, p1), ky.view(n, p2)
	if xl is not None:   # rows at or past a cloud's length belong to nobody
		kx = torch.where(torch.arange(p1, device='cuda')[None] < xl[:, None], kx, torch.zeros_like(kx))
		ky = torch.where(torch.arange(p2, device='cuda')[None] < yl[:, None], ky, torch.zeros_like(ky))
	(loss * 1.5).backward()
	return _out(loss=loss, kx=kx, ky=ky, d_x=x.grad, d_y=y.grad)


_CHAMFER_RULES = lambda i: dict(d_x=CHAMFER_BWD, d_y=CHAMFER_BWD)
for _bits, _what in ((512, 'all pairs'), (1024, 'grid'), (16384, 'tiles')):
	case(f'chamfer_distance ragged, {_what}', ['_Chamfer'], _b_chamfer_ragged, _r_chamfer, kind='atomics', bits=_bits, rules=_CHAMFER_RULES,
		 ref='test_gpu_chamfer_tiles.py::test_tile_path_equals_all_pairs_bit_for_bit[ragged]')
case('chamfer_distance 1 x 777 x 5000, target splits', ['_Chamfer'], _b_chamfer_split, _r_chamfer, kind='atomics', rules=_CHAMFER_RULES,
	 ref='test_gpu_geom.py::test_chamfer_fused_vs_oracle[shape1]')


# ---- surface_chamfer_distance (ref: test_gpu_surface_chamfer_bwd.py::test_fused_backward_is_as_close_to_float64_as_the_pair_it_replaces, the same entries)
def _b_surface_chamfer(key):
	def build():
		from test_gpu_surface_chamfer_bwd import _inputs
		return _inputs(*key, seed=sum(key))
	return build


def _r_surface_chamfer(i):
	from find_amd import functional as FN
	verts, faces, rnd, y, yl = i
	v = verts.clone().requires_grad_(True)
	loss, samples = FN.surface_chamfer(v, faces, rnd, y, yl)
	(loss * 0.7).backward()
	return _out(loss=loss, samples=samples, d_verts=v.grad)


def _slice_bits(k):
	from test_gpu_surface_chamfer_bwd import _slices
	return _slices(k)


_SURF_SMALL = (1, 7, 5, 63, 40, True, True)   # the smallest ragged entry of test_gpu_surface_chamfer_bwd.CASES: 39 targets, one wave of them
for _k in (1, 8):
	case(f'surface_chamfer_distance n1 V7 F5 63 x 40 ragged, {_k} slice(s)', ['_SurfaceChamfer', '_SampleSurface'], _b_surface_chamfer(_SURF_SMALL),
		 _r_surface_chamfer, bits=_slice_bits(_k), ref='test_gpu_surface_chamfer_bwd.py::test_fused_backward_is_as_close_to_float64_as_the_pair_it_replaces')


# The next entry of that table: three meshes with faces of their own, 70 / 0 / 35 targets -- a cloud without targets, and one with more
# targets than a wave has lanes.  There the fused backward is NOT reproducible to the bit, poison or not: its LDS adds are compare-and-swaps
# that land in whatever order the lanes of two waves meet on a word (geom.hip, lds_add_cas; measured on an MI355X: 6 to 10 of 11 repeats of
# the clean call differ from the first, by one unit in the last place, 2e-8 of the largest entry).  So d_verts is held to the derived bound
# of a sum in another order, restated in float64 from the draws: d_x[s] = c0 (x_s - y_j) + sum_k -c1 (y_k - x_s) (n_s addends, A_s their
# absolute sum), d_verts[v] = sum w_c d_x[s] over the n_v corners at v:
#     (n_v + 3) 2^-24 sum w_c A_s  +  sum w_c (n_s + 3) 2^-24 A_s.
# The samples come from sample_points on given draws (the other way into surface_chamfer_distance), so the restatement needs nothing of a run.
_SURF_THREE = (3, 7, 5, 63, 70, False, True)
G_SURF = 0.7


def _b_surface_chamfer_three():
	from oracle import geom_ref as G
	from test_gpu_surface_chamfer_bwd import _inputs
	n, V, F, S, P2 = _SURF_THREE[:5]
	verts, faces, rnd, y, yl = _inputs(*_SURF_THREE, seed=sum(_SURF_THREE))
	g = _gen(17)
	fi = torch.randint(0, F, (n, S), generator=g).to(torch.int32)
	uv = torch.rand(n, S, 2, generator=g)
	v64, y64, f, lens = verts.double().cpu(), y.double().cpu(), faces.cpu().long(), yl.cpu().long()
	us = uv[..., 0].double().sqrt()
	w = torch.stack([1 - us, us * (1 - uv[..., 1].double()), us * uv[..., 1].double()], dim=-1)          # (n, S, 3)
	corners = torch.stack([f[m][fi[m].long()] for m in range(n)])                                       # (n, S, 3)
	x64 = (w[..., None] * torch.stack([v64[m][corners[m]] for m in range(n)])).sum(2)                    # (n, S, 3)
	_, ix = G.knn1(x64, y64, None, lens)
	_, iy = G.knn1(y64, x64, lens, None)
	bound = torch.zeros(n, V, 3, dtype=torch.float64)
	u = 2.0 ** -24
	for m in range(n):
		c0, c1 = 2 * G_SURF / (n * S), 2 * G_SURF / (n * max(int(lens[m]), 1))
		ok = ix[m] >= 0
		A = (c0 * (x64[m] - y64[m][ix[m].clamp(min=0)]).abs()) * ok[:, None]
		n_s = ok.double()
		k = (iy[m] >= 0).nonzero()[:, 0]
		A.index_add_(0, iy[m][k], c1 * (y64[m][k] - x64[m][iy[m][k]]).abs())
		n_s.index_add_(0, iy[m][k], torch.ones(len(k), dtype=torch.float64))
		e_s = (n_s[:, None] + 3) * u * A
		n_v, s_v = _row_stats(V, corners[m], w[m][..., None] * A[:, None, :])
		_, e_v = _row_stats(V, corners[m], w[m][..., None] * e_s[:, None, :])
		bound[m] = (n_v[:, None] + 3) * u * s_v + e_v
	return dict(verts=verts, faces=faces, fi=fi.cuda(), uv=uv.cuda(), y=y, yl=yl, bound=bound)


def _r_surface_chamfer_three(i):
	from find_amd import functional as FN
	v = i['verts'].clone().requires_grad_(True)
	samples = FN.sample_points(v, i['faces'], i['fi'], i['uv'])
	loss = FN.surface_chamfer_distance(samples, i['y'], i['yl'])
	(loss * G_SURF).backward()
	return _out(loss=loss, samples=samples, d_verts=v.grad)


for _k in (1, 8):
	case(f'surface_chamfer_distance n3 V7 F5 63 x 70 ragged, own faces, {_k} slice(s)', ['_SurfaceChamfer', '_SamplePoints'], _b_surface_chamfer_three,
		 _r_surface_chamfer_three, kind='atomics', bits=_slice_bits(_k), rules=lambda i: dict(d_verts=Rule(bits=False, bound=i['bound'])),
		 ref='test_gpu_surface_chamfer_bwd.py::test_fused_backward_is_as_close_to_float64_as_the_pair_it_replaces')


# ---- point_face_distance: p_len with a 0, padded faces, a mesh without faces; split and unsplit (bit 8192)
# (ref: test_gpu_surface.py::test_against_float64 holds the op at 3 x 1500 points on 2001 faces; this scene of 200 points is held here, in _check_point_face)
def _face_splits(blocks, n_faces, bits):
	"""surface.hip: face_splits, restated (PF_TILE = 512 faces per tile): the blocks that share the face range of one launch.  More than one:
	the keys are preset to 0xff by a memset and merged with 64-bit atomic minima; one: plain stores, no preset."""
	splits = 1
	if bits & 8192:
		return splits
	while blocks * splits < 512 and splits < 16 and n_faces // (splits * 2) >= 512:
		splits *= 2
	return splits


def _b_point_face():
	import surface_ref as SR
	from find_amd import synthetic
	from test_gpu_surface import _deformed, _off_the_medial_axis, _queries
	v, f = synthetic.template(1002)     # 2000 faces: with the padding, two tiles of 512 for each of two splits
	g = _gen(4)
	verts = _deformed(v, 3, g)
	P, F = 200, f.shape[0]
	pts = torch.stack([_queries(verts[m], f, F, P, g) for m in range(3)])
	faces = torch.cat([f, torch.full((9, 3), -1, dtype=f.dtype)])[None].expand(3, -1, -1).contiguous().clone()
	faces[2] = -1                       # a mesh without faces
	blocks = 3 * -(-P // (64 * 2))      # (surface.hip: a block owns 64 * PF_NQ = 128 queries)
	assert _face_splits(blocks, faces.shape[1], 0) == 2 and _face_splits(blocks, faces.shape[1], 8192) == 1   # the two cases below do take two routes
	p_len = torch.tensor([P, 0, 150])
	gout = torch.randn(3, P, generator=g)
	r = SR.point_face(pts[0].double(), verts[0].double(), f, far=1e-4)
	gout[0] *= _off_the_medial_axis(r)   # (there the last bit decides the face, and with it the gradient: test_against_float64 leaves those queries out too)
	# float64 restatement of d_verts' addends: -2 g bary_k (p - c) at the corners of the nearest face (surface_ref.gradients)
	bound = torch.zeros(3, v.shape[0], 3, dtype=torch.float64)
	c = (r['bary'][..., None] * verts[0].double()[f[r['idx']].long()]).sum(1)
	addend = -2 * gout[0].double()[:, None, None] * r['bary'][..., None] * (pts[0].double() - c)[:, None, :]
	n, s = _row_stats(v.shape[0], f[r['idx']], addend)
	bound[0] = atomic_bound(n[:, None], s)   # (meshes 1 and 2 have no valid row, or no face: exactly zero)
	return dict(pts=pts, verts=verts, faces=faces, p_len=p_len, gout=gout, bound=bound, F=faces.shape[1], r64=r, r32=SR.point_face(pts[0], verts[0], f), f=f)


def _r_point_face(i):
	from find_amd import functional as FN
	p, v = i['pts'].cuda().requires_grad_(True), i['verts'].cuda().requires_grad_(True)
	dist2, idx, bary = FN.point_face_distance(p, v, i['faces'].cuda(), i['p_len'])
	(dist2 * i['gout'].cuda()).sum().backward()
	return _out(dist2=dist2, idx=idx, bary=bary, d_points=p.grad, d_verts=v.grad)


def _rules_point_face(i):
	return dict(idx=Rule(irange=(0, i['F'])), d_verts=Rule(bits=False, bound=i['bound']))


def _check_point_face(i, r0):
	"""Mesh 0 against the float64 brute force, by test_gpu_surface.py's criterion (e_hip <= 4 e32 + 1e-7 scale: _held); the documented values
	of rows at or past p_len and of a mesh without faces."""
	import surface_ref as SR
	from test_gpu_surface import _held
	r64, r32 = i['r64'], i['r32']
	_held('point_face small scene: dist2', r0['dist2'][0], r64['dist2'], r32['dist2'])
	gp64, gv64 = SR.gradients(i['pts'][0].double(), i['verts'][0].double(), i['f'], r64['idx'], r64['bary'], i['gout'][0].double())
	gp32, gv32 = SR.gradients(i['pts'][0], i['verts'][0], i['f'], r32['idx'], r32['bary'], i['gout'][0])
	_held('point_face small scene: d verts', r0['d_verts'][0], gv64, gv32)
	for m, n in enumerate(i['p_len'].tolist()):
		for k in ('dist2', 'bary', 'd_points'):
			assert (r0[k][m, n:] == 0).all(), (k, m)
		assert (r0['idx'][m, n:] == -1).all()
	assert (r0['idx'][2] == -1).all() and (r0['dist2'][2] == 0).all() and (r0['d_verts'][1:] == 0).all()


for _bits, _what in ((0, 'split'), (8192, 'unsplit')):
	case(f'point_face_distance with an empty cloud and a mesh without faces, {_what}', ['_PointFace'], _b_point_face, _r_point_face, kind='atomics', bits=_bits,
		 rules=_rules_point_face, ref='test_gpu_surface.py::test_against_float64', check=_check_point_face)


# ---- masked_mse (ref: test_gpu_geom.py::test_masked_mse_vs_torch, the same sizes and the same shift)
def _b_masked_mse(n_pts, shift):
	def build():
		g = _gen(41 + n_pts)
		pred = torch.rand(n_pts + shift, 3, generator=g)
		gt = torch.rand(n_pts + shift, 3, generator=g) * 1.3
		gt[::7] = 1.25
		return pred.cuda(), gt.cuda(), shift
	return build


def _r_masked_mse(i):
	from find_amd import functional as FN
	pred, gt, shift = i
	buf = pred.clone().requires_grad_(True)
	loss = FN.masked_mse(buf[shift:][None], gt[shift:][None])
	(loss * 2.5).backward()
	return _out(loss=loss, d_pred=buf.grad)


case('masked_mse 1003 points', ['_MaskedMSE'], _b_masked_mse(1003, 0), _r_masked_mse, ref='test_gpu_geom.py::test_masked_mse_vs_torch')
case('masked_mse 1001 points off a 16-byte boundary', ['_MaskedMSE'], _b_masked_mse(1001, 1), _r_masked_mse, ref='test_gpu_geom.py::test_masked_mse_vs_torch')


# ---- image_mse (ref: test_gpu_geom.py::test_image_mse_vs_torch, the same shapes)
def _b_image_mse(shape):
	def build():
		g = _gen(sum(shape))
		img, gimg = torch.rand(*shape, 3, generator=g), torch.rand(*shape, 3, generator=g)
		m, gm = torch.rand(*shape, generator=g), (torch.rand(*shape, generator=g) > 0.4).float()
		return img.cuda(), gimg.cuda(), m.cuda(), gm.cuda()
	return build


def _r_image_mse(i):
	from find_amd import functional as FN
	img, gimg, m, gm = i
	a, am = img.clone().requires_grad_(True), m.clone().requires_grad_(True)
	loss = FN.image_mse(a, gimg, am, gm)
	(loss * 3.0).backward()
	return _out(loss=loss, d_a=a.grad, d_am=am.grad)


def _r_image_mse_plain(i):
	from find_amd import functional as FN
	_, _, m, gm = i
	s = m.clone().requires_grad_(True)
	loss = FN.image_mse(s, gm)   # silhouettes: one channel, no masks
	loss.backward()
	return _out(loss=loss, d_a=s.grad)


case('image_mse (2, 3, 40, 40), 16-byte loads', ['_ImageMSE'], _b_image_mse((2, 3, 40, 40)), _r_image_mse, ref='test_gpu_geom.py::test_image_mse_vs_torch')
case('image_mse (1, 1, 7, 5), scalar', ['_ImageMSE'], _b_image_mse((1, 1, 7, 5)), _r_image_mse, ref='test_gpu_geom.py::test_image_mse_vs_torch')
case('image_mse one channel, no masks', ['_ImageMSE'], _b_image_mse((2, 3, 40, 40)), _r_image_mse_plain, ref='test_gpu_geom.py::test_image_mse_vs_torch')


# ---- image_metric_sums (ref: test_gpu_eval2d.py::test_sums_match_float64[3-(37, 29)-1])
def _b_metric_sums():
	from test_gpu_eval2d import _inputs
	return _inputs(3, (37, 29), 1, seed=301)


def _r_metric_sums(i):
	from find_amd import functional as FN
	return _out(sums=FN.image_metric_sums(*i))


case('image_metric_sums (3, 37 x 29, 1) with hide', ['image_metric_sums'], _b_metric_sums, _r_metric_sums, ref='test_gpu_eval2d.py::test_sums_match_float64')


# ---- frames_u8 (ref: test_gpu_vis.py::test_frames_u8_is_exact)
def _r_frames(i):
	from find_amd import functional as FN
	return _out(plain=FN.frames_u8(i, rot180=False), turned=FN.frames_u8(i, rot180=True))


case('frames_u8 (3, 17, 33, 3)', ['frames_u8'], lambda: (torch.rand(3, 17, 33, 3, generator=_gen(8)) * 1.2 - 0.1).cuda(), _r_frames,
	 ref='test_gpu_vis.py::test_frames_u8_is_exact')


# ---- smoothness (ref: test_gpu_geom.py::test_smoothness_forward_backward_vs_oracle / ::test_smoothness_loss_scalar_vs_oracle, the same mesh)
def _b_smooth():
	verts, faces = _geom_mesh(n=3, seed=4)
	return verts.cuda(), faces.cuda()


def _r_smooth(i):
	from find_amd import functional as FN
	verts, faces = i
	topo = FN.MeshTopology.get(faces, verts.shape[1])
	v = verts.clone().requires_grad_(True)
	e, l = FN.mesh_edge_and_laplacian(v, topo)
	(0.1 * l + 10 * e).backward()
	return _out(edge=e, lap=l, d_verts=v.grad)


def _r_smooth_loss(i):
	from find_amd import functional as FN
	verts, faces = i
	topo = FN.MeshTopology.get(faces, verts.shape[1])
	v = verts.clone().requires_grad_(True)
	loss = FN.mesh_smoothness_loss(v, topo, w_edge=10.0, w_lap=0.1)
	(loss * 1000.0).backward()
	return _out(loss=loss, d_verts=v.grad)


case('mesh_edge_and_laplacian 3 x 1002', ['_Smooth'], _b_smooth, _r_smooth, ref='test_gpu_geom.py::test_smoothness_forward_backward_vs_oracle')
case('mesh_smoothness_loss 3 x 1002', ['_SmoothLoss'], _b_smooth, _r_smooth_loss, ref='test_gpu_geom.py::test_smoothness_loss_scalar_vs_oracle')


# ---- vertex_normals (ref: test_gpu_normals.py::test_vertex_normals_shared_topology_against_float64 / ::test_vertex_normals_per_mesh_faces)
def _b_vnormals_shared():
	verts, faces = _geom_mesh(n=3, seed=4)
	return verts.cuda(), faces.cuda(), torch.randn(verts.shape, generator=_gen(5)).cuda()


def _b_vnormals_per_mesh():
	from find_amd import synthetic
	(v1, f1), (v2, f2) = synthetic.ellipsoid_mesh(4, 9), synthetic.ellipsoid_mesh(10, 10)
	verts = torch.zeros(2, 102, 3)
	verts[0, :38], verts[1] = v1, v2
	faces = torch.full((2, 200, 3), -1, dtype=torch.int64)
	faces[0, :f1.shape[0]], faces[1] = f1, f2
	return verts.cuda(), faces.cuda(), torch.randn(verts.shape, generator=_gen(6)).cuda()


def _r_vnormals(i):
	from find_amd import functional as FN
	verts, faces, proj = i
	v = verts.clone().requires_grad_(True)
	n = FN.vertex_normals(v, faces)
	n.backward(proj)
	return _out(normals=n, d_verts=v.grad)


case('vertex_normals, shared faces', ['_VertexNormals'], _b_vnormals_shared, _r_vnormals, ref='test_gpu_normals.py::test_vertex_normals_shared_topology_against_float64')
case('vertex_normals, per-mesh padded faces', ['_VertexNormals'], _b_vnormals_per_mesh, _r_vnormals, ref='test_gpu_normals.py::test_vertex_normals_per_mesh_faces')


# ---- normal_map in both spaces (ref: test_gpu_normals.py::test_normal_map_against_float64, the same inputs)
def _b_normal_map():
	from test_gpu_normals import _rotations
	N, M, H, W = 2, 3, 16, 16
	g = _gen(7)
	raw = torch.randn(N, M, H, W, 3, generator=g) * torch.rand(N, M, H, W, 1, generator=g) * 3
	raw[torch.rand(N, M, H, W, generator=g) < 0.2] = 0
	return raw.cuda(), _rotations(M, 1).float().cuda(), torch.randn(N, M, H, W, 3, generator=g).cuda()


def _r_normal_map(space):
	def run(i):
		from find_amd import functional as FN
		raw, R, proj = i
		x = raw.clone().requires_grad_(True)
		out = FN.normal_map(x, None if space == 'world' else R, space=space)
		out.backward(proj)
		return _out(out=out, d_raw=x.grad)
	return run


for _space in ('view', 'world'):
	case(f'normal_map, {_space} space', ['_NormalMap'], _b_normal_map, _r_normal_map(_space), ref='test_gpu_normals.py::test_normal_map_against_float64')


# ---- normal_loss (ref: test_gpu_normals.py::test_normal_loss_against_float64[(3, 37, 29)] / ::test_normal_loss_with_all_weights_zero)
def _b_normal_loss(zero):
	def build():
		from test_gpu_normals import _loss_inputs
		p, t, w = _loss_inputs((3, 37, 29), 1 if zero else 69)
		return p.cuda(), t.cuda(), (torch.zeros_like(w) if zero else w).cuda()
	return build


def _r_normal_loss(i):
	from find_amd import functional as FN
	p, t, w = i
	x = p.clone().requires_grad_(True)
	loss = FN.normal_loss(x, t, w)
	(loss * 1.7).backward()
	return _out(loss=loss, d_pred=x.grad)


case('normal_loss (3, 37, 29)', ['_NormalLoss'], _b_normal_loss(False), _r_normal_loss, ref='test_gpu_normals.py::test_normal_loss_against_float64')
case('normal_loss, all weights zero', ['_NormalLoss'], _b_normal_loss(True), _r_normal_loss, ref='test_gpu_normals.py::test_normal_loss_with_all_weights_zero')


# ---- depth_map with ragged faces at 24 x 40 (ref: test_gpu_depth.py::test_depth_gradient_ragged_faces / ::test_depth_gradient_rectangular_image)
def _depth_bound(verts, faces, R, T, p2f, g, H, W, fov_deg=60.0):
	"""Bound of find_depth_bwd's d_verts from the float64 restatement of its addends (test_depth_host.depth_closed_form's formula, the
	addends kept apart): pixel p adds g_p b_k / (n . d) * n @ R^T at corner k of its face."""
	verts, R, T, g = verts.double(), R.double(), T.double(), g.double()
	N, V, _ = verts.shape
	M = R.shape[0]
	F = faces.shape[-2]
	p2f = p2f.reshape(N * M, H, W).long()
	g = g.reshape(N * M, H, W)
	s = 1.0 / math.tan(math.radians(fov_deg) / 2)
	img, yi, xi = torch.nonzero(p2f >= 0, as_tuple=True)
	f = p2f[img, yi, xi] - img * F
	mesh, view = img // M, img % M
	fv = faces.long()[f] if faces.dim() == 2 else faces.long()[mesh, f]
	p = torch.einsum('pki,pij->pkj', verts[mesh[:, None], fv], R[view]) + T[view][:, None, :]
	d = torch.stack([(1 - (2 * xi.double() + 1) / W) / s, (1 - (2 * yi.double() + 1) / H) / s, torch.ones(len(img), dtype=torch.float64)], dim=1)
	n = torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1)
	nd = (n * d).sum(1)
	X = ((n * p[:, 0]).sum(1) / nd)[:, None] * d
	rows, adds = [], []
	for k in range(3):
		b = (torch.linalg.cross(p[:, (k + 1) % 3] - X, p[:, (k + 2) % 3] - X, dim=1) * n).sum(1) / (n * n).sum(1)
		dp = (g[img, yi, xi] * b / nd)[:, None] * n
		rows.append(mesh * V + fv[:, k])
		adds.append(torch.einsum('pj,pij->pi', dp, R[view]))
	cnt, sm = _row_stats(N * V, torch.stack(rows, 1), torch.stack(adds, 1))
	return atomic_bound(cnt[:, None], sm).view(N, V, 3)


def _b_depth_map():
	from find_amd import functional_render as FR
	from find_amd import synthetic
	from test_gpu_depth import _upstream, _views
	(v1, f1), (v2, f2) = synthetic.ellipsoid_mesh(4, 9), synthetic.ellipsoid_mesh(10, 10)
	verts = torch.zeros(2, 102, 3)
	verts[0, :38], verts[1] = v1, v2
	faces = torch.full((2, 200, 3), -1, dtype=torch.int32)
	faces[0, :f1.shape[0]], faces[1] = f1.to(torch.int32), f2.to(torch.int32)
	R, T = _views([0.3, 0.28], [10., -60.], [0., 40.])
	params = FR.make_params((24, 40))
	_, _, p2f, zbuf = FR.render(verts.cuda(), None, faces.cuda(), R.cuda(), T.cuda(), params, want_mask=False, want_image=False, want_frags=True)
	torch.cuda.synchronize()
	up = _upstream(p2f, 2)
	bound = _depth_bound(verts, faces.clamp(min=0), R, T, p2f.cpu(), up, 24, 40)
	return dict(verts=verts.cuda(), faces=faces.cuda(), R=R.cuda(), T=T.cuda(), params=params, p2f=p2f, zbuf=zbuf, up=up.cuda(), bound=bound)


def _r_depth_map(i):
	from find_amd import functional as FN
	x = i['verts'].clone().requires_grad_(True)
	depth = FN.depth_map(x, i['faces'], i['R'], i['T'], i['params'], i['p2f'], i['zbuf'])
	depth.backward(i['up'])
	return _out(depth=depth, d_verts=x.grad)


def _check_depth_map(i, r0):
	"""The two existing tests have ragged faces at 32^2 and shared faces at 24 x 40; this combination against the oracle by their criterion."""
	from test_gpu_depth import _against_oracle
	assert torch.equal(r0['depth'], i['zbuf'].cpu())
	_against_oracle('ragged faces at 24 x 40', i['verts'].cpu(), i['faces'].cpu().clamp(min=0), i['R'].cpu(), i['T'].cpu(), i['p2f'], i['up'].cpu(), r0['depth'], r0['d_verts'])
	assert (r0['d_verts'][0, 38:] == 0).all()


case('depth_map, ragged faces at 24 x 40', ['_DepthMap'], _b_depth_map, _r_depth_map, kind='atomics', rules=lambda i: dict(d_verts=Rule(bits=False, bound=i['bound'])),
	 ref='test_gpu_depth.py::test_depth_gradient_ragged_faces', check=_check_depth_map)


# ---- depth_loss (ref: test_gpu_depth.py::test_depth_loss_against_float64[(3, 1073)] / ::test_depth_loss_without_a_valid_pixel)
def _b_depth_loss(valid):
	def build():
		from test_gpu_depth import _loss_inputs
		p, t, w = _loss_inputs(3, 37 * 29, 1 if not valid else 3 + 37 * 29)
		return (p if valid else -p.abs()).cuda(), t.cuda(), w.cuda()
	return build


def _r_depth_loss(kind, per_image):
	def run(i):
		from find_amd import functional as FN
		p, t, w = i
		x = p.clone().requires_grad_(True)
		r = FN.depth_loss(x, t, w, kind=kind, delta=0.01, trunc=0.02, return_per_image=per_image)
		loss, per = r if per_image else (r, None)
		(loss * 1.7).backward()
		return _out(loss=loss, per_image=per, d_pred=x.grad)
	return run


for _kind in ('l1', 'l2', 'huber'):
	case(f'depth_loss {_kind} (3, 37 x 29)', ['_DepthLoss'], _b_depth_loss(True), _r_depth_loss(_kind, False), ref='test_gpu_depth.py::test_depth_loss_against_float64')
	case(f'depth_loss {_kind} with the per-image sums', ['_DepthLoss'], _b_depth_loss(True), _r_depth_loss(_kind, True), ref='test_gpu_depth.py::test_depth_loss_against_float64')
	case(f'depth_loss {_kind} without a valid pixel', ['_DepthLoss'], _b_depth_loss(False), _r_depth_loss(_kind, True), ref='test_gpu_depth.py::test_depth_loss_without_a_valid_pixel')


# ---- register_points (ref: test_gpu_mlp.py::test_registration_forward_backward_vs_oracle[(3, 3, 257)], and (1, 3, 1500) for the shared template)
def _b_register(vb):
	def build():
		gen = _gen(9 + vb)
		N, V = 3, 257
		verts = torch.randn(vb, V, 3, generator=gen) * 0.1
		disp = torch.randn(N, V, 3, generator=gen) * 0.01
		reg = torch.cat([torch.rand(N, 3, generator=gen) * 0.02 - 0.01, torch.rand(N, 3, generator=gen) * 0.6 - 0.3, torch.rand(N, 3, generator=gen) * 0.2 + 0.9], dim=1)
		return verts.cuda(), disp.cuda(), reg.cuda(), torch.randn(N, V, 3, generator=gen).cuda()
	return build


def _r_register(i):
	from find_amd import functional as FN
	verts, disp, reg, gout = i
	d, r = disp.clone().requires_grad_(True), reg.clone().requires_grad_(True)
	out = FN.register_points(verts, d, r)
	out.backward(gout)
	return _out(out=out, d_disp=d.grad, d_reg=r.grad)


for _vb in (1, 3):
	case(f'register_points (3, 257), verts batch {_vb}', ['_Register'], _b_register(_vb), _r_register, ref='test_gpu_mlp.py::test_registration_forward_backward_vs_oracle')


# ---- pca_offsets (ref: test_gpu_pca.py::test_decode_matches_float64 at (1, 98, 1) and (3, 6890, 7))
def _r_pca(i):
	from find_amd import functional as FN
	coefs, sv, dout = i
	s = sv.detach().clone().requires_grad_(True)
	off = FN.pca_offsets(coefs, s)
	off.backward(dout)
	return _out(offsets=off, d_shapevec=s.grad)


def _b_pca():
	from test_gpu_pca import _decode_inputs
	return _decode_inputs(3, 98, 7, seed=108)


def _check_pca(i, r0):
	"""float64 at this shape, to that test's tolerances."""
	coefs, sv, dout = (t.detach().double().cpu() for t in i)
	off64, d64 = torch.einsum('vbc,nb->nvc', coefs, sv), torch.einsum('nvc,vbc->nb', dout, coefs)
	assert (r0['offsets'].double() - off64).abs().max().item() / off64.abs().max().item() < 1e-5
	assert (r0['d_shapevec'].double() - d64).abs().max().item() / d64.abs().max().item() < 1e-4


case('pca_offsets (3, 98, 7)', ['_PCAOffsets'], _b_pca, _r_pca, ref='test_gpu_pca.py::test_decode_matches_float64', check=_check_pca)


# ---- latents (ref: test_gpu_mlp.py::test_latent_gather_matches_indexing_and_scatters_deterministically / ::test_latent_gather_many_and_weighted_terms)
def _b_latent_gather():
	g = _gen(3)
	return torch.randn(37, 100, generator=g).cuda(), torch.tensor([5, 0, 36, 5, -1, 17, 5, 0]).cuda(), torch.randn(8, 100, generator=g).cuda()


def _r_latent_gather(i):
	from find_amd import functional as FN
	table, idx, w = i
	t = table.clone().requires_grad_(True)
	out = FN.latent_gather(t, idx)
	(out * w).sum().backward()
	return _out(rows=out, d_table=t.grad)


def _b_latent_many():
	g = _gen(8)
	tables = [torch.randn(n, d, generator=g).cuda() for n, d in [(5, 100), (9, 100), (5, 100), (9, 9)]]
	idxs = [torch.tensor(i).cuda() for i in ([0, 4, 4], [8, 2, 2], [1, 1, 1], [-1, 3, 0])]
	return tables, idxs, [torch.randn(3, t.shape[1], generator=g).cuda() for t in tables]


def _r_latent_many(i):
	from find_amd import functional as FN
	tables, idxs, w = i
	ts = [t.clone().requires_grad_(True) for t in tables]
	outs = FN.latent_gather_many(ts, idxs)
	sum((o * x).sum() for o, x in zip(outs, w)).backward()
	r = {f'rows{k}': o for k, o in enumerate(outs)}
	r.update({f'd_table{k}': t.grad for k, t in enumerate(ts)})
	return _out(**r)


def _r_weighted_terms(i):
	from find_amd import functional as FN
	raws = [torch.tensor(v, device='cuda', requires_grad=True) for v in i]
	total, scaled = FN.weighted_terms(raws, [10000.0, 1000.0, 1.0])
	(total * 2.0 + scaled[2]).backward()
	return _out(total=total, scaled=torch.stack(scaled), d_terms=torch.stack([r.grad for r in raws]))


case('latent_gather, duplicate and -1 indices', ['_LatentGather', '_grad_for'], _b_latent_gather, _r_latent_gather,
	 ref='test_gpu_mlp.py::test_latent_gather_matches_indexing_and_scatters_deterministically')
case('latent_gather_many, four tables', ['_LatentGatherMany', '_grad_for'], _b_latent_many, _r_latent_many, ref='test_gpu_mlp.py::test_latent_gather_many_and_weighted_terms')
case('weighted_terms, three terms', ['_WeightedTerms'], lambda: (0.25, 3.0, 1e-3), _r_weighted_terms, ref='test_gpu_mlp.py::test_latent_gather_many_and_weighted_terms')


# ---- contrastive_pose (ref: test_gpu_contrastive.py::test_loss_and_gradient_equal_the_reference, the fixture's cases)
def _b_contrastive(name):
	def build():
		z = np.load(os.path.join(GOLD, 'contrastive.npz'))
		return (torch.from_numpy(z[f'case/{name}/vecs']).cuda(), torch.from_numpy(z[f'case/{name}/codes']).float().cuda(), torch.from_numpy(z[f'case/{name}/pairs']).cuda())
	return build


def _r_contrastive(i):
	from find_amd import functional as FN
	vecs, codes, pairs = i
	v = vecs.clone().requires_grad_(True)
	loss = FN.contrastive_pose(v, codes, pairs)
	loss.backward()
	return _out(loss=loss, d_vecs=v.grad)


for _name in ('n16_k256', 'n24_k3_chunked'):
	case(f'contrastive_pose {_name}', ['_ContrastivePose'], _b_contrastive(_name), _r_contrastive, ref='test_gpu_contrastive.py::test_loss_and_gradient_equal_the_reference')


# ---- part_labels, part_cross_entropy in both forms (ref: test_gpu_part_loss.py::test_loss_and_gradients_equal_the_reference / ::test_labels_equal_the_reference)
def _b_part():
	z = np.load(os.path.join(GOLD, 'part_loss.npz'))
	name = str(z['ce_cases'][0])
	C = z[f'ce/{name}/logits'].shape[-1]
	return dict(logits=torch.from_numpy(z[f'ce/{name}/logits']).cuda(), labels=torch.from_numpy(z[f'ce/{name}/gt_labels']).cuda(), mask=torch.from_numpy(z[f'ce/{name}/mask']).cuda(),
				gt_logits=torch.from_numpy(z[f'ce/{name}/gt_logits']).cuda(), C=C)


def _r_part_labels(i):
	from find_amd import functional as FN
	return _out(labels=FN.part_labels(i['gt_logits'], i['mask'].shape[1:]))


def _r_part_ce(form):
	def run(i):
		from find_amd import functional as FN
		x, m = i['logits'].clone().requires_grad_(True), i['mask'].clone().requires_grad_(True)
		loss, ce = FN.part_cross_entropy(x, i['labels'], m, return_ce=True, form=form)
		loss.backward()
		return _out(loss=loss, ce=ce, d_logits=x.grad, d_mask=m.grad)
	return run


case('part_labels', ['part_labels'], _b_part, _r_part_labels, rules=lambda i: dict(labels=Rule(irange=(0, i['gt_logits'].shape[1]))),
	 ref='test_gpu_part_loss.py::test_labels_equal_the_reference')
for _form in ('direct', 'staged'):
	case(f'part_cross_entropy, {_form}', ['_PartCrossEntropy'], _b_part, _r_part_ce(_form), ref='test_gpu_part_loss.py::test_loss_and_gradients_equal_the_reference')


# ---- the MLP, forward and backward (ref: test_gpu_mlp_f64.py::test_model_against_float64 / ::test_model_against_float64_every_size hold the model to float64
# at 31 .. 6890 points per foot in every arithmetic; test_gpu_mlp.py::test_backward_is_bit_reproducible_* documents the backward as deterministic)
def _mlp_case(n_feet, V, want):
	from test_gpu_mlp_f64 import Case as MlpCase
	return MlpCase(n_feet, V, False, col_only=want == ('col',))


def _b_mlp(n_feet, V, want):
	def build():
		from test_gpu_mlp_f64 import _model, _oracle
		c = _mlp_case(n_feet, V, want)
		o = _oracle(c)   # (its inputs are the case's: latents, free points in the foot box, upstream weights that leave out rows at a ReLU tie)
		return dict(m=_model(c), lat={k: v.cuda() for k, v in o['lat'].items()}, pos=o['pos'].cuda(), up=o['up'].cuda(), o=o)
	return build


def _r_mlp(precision, want):
	def run(i):
		from find_amd import functional as FN
		m = i['m']
		prev = FN.set_mlp_precision(precision)
		try:
			m.set_mlp_precision(None)   # follow the process default set above
			lv = {k: i['lat'][k].clone().requires_grad_(True) for k in (('texvec',) if want == ('col',) else ('shapevec', 'texvec', 'posevec'))}
			m.zero_grad(set_to_none=True)
			res = m(i['pos'], want=want, **lv)
			sum((res[k] * i['up']).sum() for k in want).backward()
			torch.cuda.synchronize()
			r = {k: res[k] for k in want}
			r.update({'d_' + n: p.grad for n, p in m.named_parameters() if p.grad is not None})
			r.update({'d_' + k: v.grad for k, v in lv.items() if v.grad is not None})
			assert len(r) > len(want) + len(lv)   # (weight gradients are there)
			return _out(**r)
		finally:
			FN.set_mlp_precision(prev)
			m.zero_grad(set_to_none=True)
	return run


def _check_mlp(precision):
	def check(i, r0):
		"""The clean run against the float64 evaluation of the model (oracle.mlp_ref through test_gpu_mlp_f64._oracle), by that module's
		criteria: e_hip <= C e_fp32 + A per tensor for fp32 and bf16x3 (_errors / _over), F16_OUT / F16_REL for fp16 operands."""
		import test_gpu_mlp_f64 as M
		o = i['o']
		assert o['excluded'] < M.MAX_EXCLUDED
		from oracle import mlp_ref
		mine = lambda n: n.split('.')[0] in mlp_ref.TRAINABLE or n in ('shapevec', 'texvec', 'posevec')   # (as test_gpu_mlp_f64._hip gathers them)
		h = dict(out=r0.get('disp'), col=r0['col'], grads={k[2:]: v for k, v in r0.items() if k.startswith('d_') and mine(k[2:])})
		if precision == 'fp16':
			o64 = o['o64']
			assert set(h['grads']) == set(o64['grads'])
			worst = max((h['grads'][k].double() - g).abs().max().item() / g.abs().max().item() for k, g in o64['grads'].items())
			d = max((h[k].double() - o64[k]).abs().max().item() for k in ('out', 'col') if h[k] is not None)
			assert d < M.F16_OUT and worst < M.F16_REL, (d, worst)
		else:
			err = M._errors(h, o)
			assert not M._over(err), {k: err[k] for k in M._over(err)}
	return check


for _n, _V in ((3, 1000), (1, 70)):
	for _prec in ('fp32', 'bf16x3', 'fp16'):
		for _want in (('disp', 'col'), ('col',)):
			case(f'mlp {_n} x {_V} {_prec} want={"+".join(_want)}', ['_MLP', '_fill_rest', '_ws'], _b_mlp(_n, _V, _want), _r_mlp(_prec, _want), check=_check_mlp(_prec),
				 ref='test_gpu_mlp_f64.py::test_model_against_float64_every_size')


# ================================================================================================ rendering
def _raster(i):
	"""(run helper) p2f range of a render: packed ids image * F + face."""
	return Rule(irange=(0, i['n_img'] * i['F']))


# ---- render on blend_scene.npz at 32^2 under both rasterisers (ref: test_gpu_pins.py holds the scene's flat-shaded forward to the reference's blend; the
# Phong image and the gradients are held to the oracle here, in _check_render_blend)
def _b_render_blend():
	from test_gpu_render_features import _blend_scene
	verts, faces, R, T = _blend_scene()
	g = _gen(3)
	cols = torch.rand(verts.shape, generator=g)
	N, M = verts.shape[0], R.shape[0]
	return dict(verts=verts.cuda(), cols=cols.cuda(), faces=faces.cuda(), R=R.cuda(), T=T.cuda(), wm=torch.rand(N, M, 32, 32, generator=g).cuda(),
				wi=torch.rand(N, M, 32, 32, 3, generator=g).cuda(), n_img=N * M, F=faces.shape[-2], size=32, clip=False)


def _r_render(i):
	from find_amd import functional_render as FR
	params = FR.make_params(i['size'], clip_faces=i['clip'])
	v, c = i['verts'].clone().requires_grad_(True), i['cols'].clone().requires_grad_(True)
	mask, image, p2f, zbuf = FR.render(v, c, i['faces'], i['R'], i['T'], params, want_mask=True, want_image=True, want_frags=True)
	((mask * i['wm']).sum() + (image * i['wi']).sum()).backward()
	return _out(mask=mask, image=image, p2f=p2f, zbuf=zbuf, d_verts=v.grad, d_cols=c.grad)


def _check_render_blend(i, r0):
	"""This scene with Phong shading and both gradients is in no other test (test_gpu_pins.py holds its flat-shaded forward to the
	reference's blend): the oracle here, by test_gpu_render.py's criteria -- mask, image and z-buffer within TOL = 1e-4 / 1e-5 where the same
	face is in front (all but 0.2 % of the pixels, test_gpu_pins.py's share of centres on an edge), the gradients within GRAD_TOL = 1e-4 of
	the largest entry of autograd through the oracle's restatement (mask: the oracle's K nearest; image: the face in front)."""
	from oracle import render_ref
	size, M = i['size'], i['R'].shape[0]
	verts, cols, faces, R, T = (i[k].cpu() for k in ('verts', 'cols', 'faces', 'R', 'T'))
	ref = render_ref.render(verts.numpy(), faces.numpy(), cols.numpy(), R.numpy(), T.numpy(), image_size=size)
	same = r0['p2f'].numpy() == ref['pix_to_face']
	assert same.mean() > 0.998, same.mean()
	assert np.abs(r0['mask'].numpy() - ref['mask']).max() < 1e-4
	assert np.abs(r0['image'].numpy() - ref['image'])[same].max() < 1e-4 and np.abs(r0['zbuf'].numpy() - ref['zbuf'])[same].max() < 1e-5
	rp = render_ref.default_params(size)
	vproj = render_ref.project(rp, verts.numpy(), R.numpy(), T.numpy())
	p2f_k, _, _, _ = render_ref.rasterize(vproj, faces.numpy(), M, size, size, 100, rp.sil_blur_radius)
	vr, cr = verts.clone().requires_grad_(True), cols.clone().requires_grad_(True)
	rm = render_ref.torch_mask(rp, vr, faces.long(), R, T, torch.from_numpy(p2f_k).long(), M)
	ri = render_ref.torch_phong_image(rp, vr, cr, faces.long(), R, T, r0['p2f'].long().reshape(-1, size, size, 1), M)
	((rm.reshape(r0['mask'].shape) * i['wm'].cpu()).sum() + (ri.reshape(r0['image'].shape) * i['wi'].cpu()).sum()).backward()
	for got, want, what in ((r0['d_verts'], vr.grad, 'd_verts'), (r0['d_cols'], cr.grad, 'd_cols')):
		scale, err = want.abs().max().item(), (got - want).abs().max().item()
		print(f'blend_scene {what}: max err {err:.3e} of scale {scale:.3e}')
		assert scale > 0 and err < 1e-4 * scale, (what, err, scale)


_RENDER_RULES = lambda i: dict(image=IMAGE, p2f=_raster(i), d_verts=RENDER_BWD, d_cols=RENDER_BWD)
for _bits, _what in ((2048, 'band'), (4096, 'list')):
	case(f'render blend_scene at 32^2, {_what} rasteriser', ['_Render'], _b_render_blend, _r_render, kind='atomics', bits=_bits, rules=_RENDER_RULES,
		 ref='test_gpu_pins.py::test_render_of_a_scene_equals_the_reference_blend_of_its_fragments', check=_check_render_blend)


# ---- a clip_faces=True crossing view at 48^2 (ref: test_gpu_render_zclip.py holds split mode to the clipped oracle at 64^2 .. 128^2 on this camera set)
def _b_render_clip():
	from find_amd import synthetic
	from test_gpu_render_zclip import _views
	v, f = synthetic.template(1002)
	g = _gen(9)
	cols = torch.rand(1, v.shape[0], 3, generator=g)
	R, T = _views([0.02, 0.3, 0.046], [0.0, 45.0, 0.0], [0.0, 20.0, 0.0])   # (test_split_mode_forward_is_bit_reproducible_...: a camera inside the mesh)
	return dict(verts=v[None].clone().cuda(), cols=cols.cuda(), faces=f.cuda(), R=R.cuda(), T=T.cuda(), wm=torch.rand(1, 3, 48, 48, generator=g).cuda(),
				wi=torch.rand(1, 3, 48, 48, 3, generator=g).cuda(), n_img=3, F=f.shape[0], size=48, clip=True)


case('render clip_faces=True, a crossing view at 48^2', ['_Render'], _b_render_clip, _r_render, kind='atomics',
	 rules=lambda i: dict(image=SPLIT_BWD, p2f=_raster(i), d_verts=SPLIT_BWD, d_cols=SPLIT_BWD),
	 ref='test_gpu_render_zclip.py::test_split_mode_forward_is_bit_reproducible_and_backward_within_atomics_order')


# ---- the feature render: the K = 4 overflow scene, and C = 5 on blend_scene (ref: test_gpu_render_features.py::test_k_overflow_and_ties_vs_oracle, the same
# scene, K and C; ::test_forward_vs_float64_oracle / ::test_gradients_features_only_vs_oracle)
def _b_features(layers):
	def build():
		from test_gpu_render_features import _blend_scene, _features, _layers
		verts, faces, R, T = _layers() if layers else _blend_scene()
		C = 5
		feats = _features(verts.shape[0], verts.shape[1], C, seed=3)
		gt = torch.randn(verts.shape[0], R.shape[0], 32, 32, C, generator=_gen(1))
		return dict(verts=verts.cuda(), feats=feats.cuda(), faces=faces.cuda(), R=R.float().cuda(), T=T.float().cuda(), gt=gt.cuda(), K=4 if layers else 100)
	return build


def _r_features(i):
	from find_amd import functional_render as FR
	params = FR.make_params(32, faces_per_pixel=i['K'])
	v, f = i['verts'].clone().requires_grad_(True), i['feats'].clone().requires_grad_(True)
	mask, _, _, _, feat = FR.render(v, None, i['faces'], i['R'], i['T'], params, want_mask=True, want_image=False, features=f)
	(feat * i['gt']).sum().backward()
	return _out(mask=mask, feat=feat, d_verts=v.grad, d_features=f.grad)


_FEATURE_RULES = lambda i: dict(d_verts=FEAT_D_VERTS, d_features=FEAT_D_FEATURES)
for _bits in (2048, 4096):
	case(f'feature render, the K = 4 overflow scene, bits {_bits}', ['_RenderFeatures'], _b_features(True), _r_features, kind='atomics', bits=_bits, rules=_FEATURE_RULES,
		 ref='test_gpu_render_features.py::test_k_overflow_and_ties_vs_oracle')
case('feature render, C = 5 on blend_scene', ['_RenderFeatures'], _b_features(False), _r_features, kind='atomics', rules=_FEATURE_RULES,
	 ref='test_gpu_render_features.py::test_forward_vs_float64_oracle')


# ---- render_points, P = 26, K = 10 (ref: test_gpu_points.py holds the splats to float64 at 1 / 26 / 5000 points and K 1 / 10 / 32)
def _b_points():
	from test_gpu_points import _clouds, _features, _views
	R, T = _views(3)
	return dict(points=_clouds(26, R, T, 5).cuda(), feats=_features(2, 26, 6).cuda(), R=R.cuda(), T=T.cuda())


def _r_points(i):
	from find_amd import functional_render as FR
	with torch.no_grad():
		image, (idx, zbuf, dists) = FR.render_points(i['points'], i['feats'], i['R'], i['T'], 256, points_per_pixel=10, return_fragments=True)
	return _out(image=image, idx=idx, zbuf=zbuf, dists=dists)


case('render_points, P = 26, K = 10', ['render_points'], _b_points, _r_points, rules=lambda i: dict(idx=Rule(irange=(0, 26))), ref='test_gpu_points.py')


# ---- uv_sample and the UV-textured render (ref: test_gpu_texture.py::test_uv_sample_matches_oracle, the same scene, and
# ::test_uv_textured_render_equals_vertex_colour_render_on_a_linear_map_and_masks_faces, the same meshes and views)
def _b_uv_sample():
	from test_oracle_texture import _scene
	return tuple(torch.from_numpy(a).cuda() for a in _scene(seed=3, Nm=3, H=37, W=29, Vt=40, F=25, P=700))


def _r_uv_sample(i):
	from find_amd import functional_render as FR
	return _out(texels=FR.uv_sample(*i))


def _b_uv_render():
	from oracle import camera_ref
	from test_gpu_texture import _uv_mesh
	verts, f, tuv, _, Meshes, _ = _uv_mesh()
	rng = np.random.RandomState(5)
	R, T = camera_ref.look_at_view_transform(dist=np.full(3, 0.3), elev=rng.uniform(-60, 60, 3), azim=rng.uniform(-90, 90, 3), up=((1, 0, 0),))
	return dict(mesh=Meshes(verts.cuda(), f.cuda(), tuv.to('cuda')), R=torch.from_numpy(R).cuda(), T=torch.from_numpy(T).cuda())


def _r_uv_render(i):
	from find_amd.renderer import FootRenderer
	rdr = i.setdefault('rdr', FootRenderer(image_size=96, device='cuda'))
	out = rdr(i['mesh'], i['R'], i['T'], return_mask=True)
	return _out(mask=out['mask'], image=out['image'])


case('uv_sample 3 maps x 700 points', ['uv_sample'], _b_uv_sample, _r_uv_sample, ref='test_gpu_texture.py::test_uv_sample_matches_oracle')
case('UV-textured render at 96^2', ['render_uv', 'render_frags', 'uv_sample', '_Render'], _b_uv_render, _r_uv_render, kind='atomics', rules=lambda i: dict(image=IMAGE),
	 ref='test_gpu_texture.py::test_uv_textured_render_equals_vertex_colour_render_on_a_linear_map_and_masks_faces')


# ---- vis.turntable: its frame buffer is torch.empty, filled slice by slice (ref: test_gpu_vis.py::test_spin_equals_the_oracle_on_rotated_vertices, the same mesh
# and camera at 64^2 and 9 frames).  A frame is (255 * image) truncated: two images within the suite's 1e-5 of each other (float-atomic vertex
# normals) are at most one level apart.
def _b_spin():
	from test_gpu_vis import _mesh
	return _mesh()[0]


def _r_spin(i):
	from find_amd import vis
	from test_gpu_vis import AZIM, DIST
	return _out(frames=vis.turntable(i, None, image_size=32, nframes=5, azim=AZIM, dist=DIST, silent=True, views_per_call=2))   # (calls of 2, 2 and 1 views)


case('vis.turntable, 5 frames at 32^2 in calls of 2', ['turntable', 'frames_u8', '_Render'], _b_spin, _r_spin, kind='atomics', rules=lambda i: dict(frames=Rule(bits=False, abs=1.0)),
	 ref='test_gpu_vis.py::test_spin_equals_the_oracle_on_rotated_vertices')


# ================================================================================================ optimiser
# (ref: test_gpu_optim.py::test_fused_step_matches_golden_trajectory holds SGD with momentum to torch's trajectory)
def _b_sgd():
	g = _gen(12)
	shapes = [(257, 3), (100,), (9, 9)]
	return [torch.randn(s, generator=g).cuda() for s in shapes], [[torch.randn(s, generator=g).cuda() for s in shapes] for _ in range(2)]


def _r_sgd(i):
	from find_amd import optim
	params0, grads = i
	ps = [p.clone().requires_grad_(True) for p in params0]
	opt = optim.SGD(ps, lr=1e-2, momentum=0.9)
	r = {}
	for step in range(2):   # the first step's momentum buffer is torch.empty_like
		for p, g in zip(ps, grads[step]):
			p.grad = g.clone()
		opt.step()
		for k, p in enumerate(ps):
			r[f'step{step + 1}/param{k}'] = p
			r[f'step{step + 1}/momentum{k}'] = opt.state[p]['momentum_buffer']
	return _out(**r)


case('optim.SGD(momentum=0.9), first and second step', ['SGD'], _b_sgd, _r_sgd, ref='test_gpu_optim.py::test_fused_step_matches_golden_trajectory')


# ================================================================================================ whole step, eager
# (ref: test_gpu_pipeline.py::test_train_3d_loss_set_matches_oracle and ::test_render_losses_match_oracle hold this setup's terms and gradients to the oracle)
def _b_step():
	from test_gpu_pipeline import _setup
	mwl, opts, batch, _ = _setup(n_feet=2, seed=3)
	mwl.rdr = type(mwl.rdr)(image_size=32, device='cuda')
	np.random.seed(11)
	R, T = mwl.rdr.sample_views(nviews=2, dist_mean=0.3, dist_std=0, elev_min=-90, elev_max=90, azim_min=-90, azim_max=90)
	return dict(mwl=mwl, opts=opts, batch=batch, views=(R, T))


def _r_step(i):
	from find_amd.train_utils import sample_latent_vectors
	mwl = i['mwl']
	mwl.zero_grad(set_to_none=True)
	batch = dict(i['batch'])
	batch.update(sample_latent_vectors(batch, mwl.model.latent_vectors_train))   # (the latent lookup is part of the step's graph: anew per run)
	torch.manual_seed(5)   # (the sampler's draws come from torch's device generator: the same in every run)
	loss, losses = mwl(batch, 0, i['opts'], chamf=True, smooth=True, texture=True, sil=True, pix=True, normal=True, p2s=True, depth=True, render_foot=True,
					   views=i['views'])
	assert set(losses) == {'loss_chamf', 'loss_smooth', 'loss_tex', 'loss_sil', 'loss_pix', 'loss_normal', 'loss_p2s', 'loss_depth'}
	loss.backward()
	torch.cuda.synchronize()
	r = {'loss': loss}
	r.update(losses)
	r.update({'d_' + n: p.grad for n, p in mwl.named_parameters() if p.grad is not None})
	assert sum(k.startswith('d_') for k in r) > 20
	i['grads'] = [k for k in r if k.startswith('d_')]
	return _out(**r)


def _rules_step(i):
	# the losses are forwards: bit for bit, but for the pixel term, which reads the shaded image (float-atomic vertex normals), and with it the total
	r = {k: STEP_GRAD for k in i['grads']}
	# loss_pix = 1.0 * mean((image * mask - gt image * gt mask)^2) with every factor in [0, 1]: two images within the suite's 1e-5 of each other move it
	# by at most 2 * 1e-5; the total adds that to bit-equal terms and rounds (a few ulp of the total: 1e-6 of it)
	r['loss_pix'] = Rule(bits=False, abs=2e-5)
	r['loss'] = Rule(bits=False, rel=1e-6, floor=20.0)
	return r


# Every term this setup can feed: the eight below.  Left out: cont_pose (needs pose codes in the batch: test_gpu_contrastive.py's composition) and
# restyle_perc_cluster (needs an encoder network of the caller's: test_gpu_part_loss.py's stub); their ops have cases of their own above.
# (Eight was also the most terms weighted_terms took; it takes 16 now, and test_gpu_all_terms.py holds the step with all ten terms to its parts.)
case('ModelWithLoss step, chamf + smooth + texture + sil + pix + normal + p2s + depth',
	 ['_MLP', '_Render', '_RenderFeatures', '_Chamfer', '_SmoothLoss', '_MaskedMSE', '_ImageMSE', '_Register', '_LatentGatherMany', '_WeightedTerms', '_PointFace', '_DepthMap',
	  '_DepthLoss', '_NormalLoss', '_VertexNormals'],
	 _b_step, _r_step, kind='atomics', rules=_rules_step, ref='test_gpu_pipeline.py::test_train_3d_loss_set_matches_oracle')


# ================================================================================================ the test
@contextlib.contextmanager
def _switch(bits):
	from find_amd import _lib
	_lib.set_tuning('raster_ablate', bits)
	try:
		yield
	finally:
		_lib.set_tuning('raster_ablate', 0)


def run_three(c):
	"""(r0, r1, r2): clean, under poisoned(0xFF), under poisoned(0x00); one discarded clean call of the same case before each."""
	inputs = c.inputs()
	out = []
	for byte in (None, 0xFF, 0x00):
		with _switch(c.bits):
			c.run(inputs)
			torch.cuda.synchronize()
			with (poisoned(byte) if byte is not None else contextlib.nullcontext()) as proxy:
				r = c.run(inputs)
				torch.cuda.synchronize()
			if proxy is not None:
				assert proxy.calls > 0, 'the case allocated nothing through the wrappers'
		out.append({k: (None if v is None else v.cpu()) for k, v in r.items()})
	return inputs, out


@pytest.mark.parametrize('c', CASES, ids=[c.name for c in CASES])
def test_no_poison_survives_and_nothing_changes(c):
	inputs, (r0, r1, r2) = run_three(c)
	assert r0 and any(v is not None and v.numel() for v in r0.values())
	for k, v in r0.items():   # the clean run is finite: a case whose own result is NaN shows nothing
		if v is not None and v.is_floating_point():
			assert torch.isfinite(v).all(), (c.name, k)
	if c.check is not None:
		c.check(inputs, r0)
	rules = c.rules(inputs) if c.rules is not None else {}
	assert set(rules) <= set(r0), (set(rules) - set(r0))
	bad = compare(c.name, r0, r1, r2, rules)
	assert not bad, '\n'.join(bad)


# ================================================================================================ whole step, captured
def test_captured_step_replays_the_same_with_poisoned_private_buffers():
	"""GraphedStep (capturable Adam, warmup=1, the smallest model of test_gpu_trainloop.py) captured once clean and once with warm-up and
	capture inside poisoned(0xFF): the fills are kernels, so they are captured and every replay poisons the graph's private buffers again.
	Three replays of each on the same scans and draws: the same loss terms (forwards: bit for bit) and the same parameters, by the rule
	test_gpu_train3d.py::test_graphed_step_equals_eager_steps holds a graph to the eager loop with (float atomics in the sampling backward
	under Adam's scale-free update: all but a thousandth of the elements within a tenth of one step, none further than a few such flips).
	Only the FIRST replay's terms are compared bit for bit, which is less than "the eager case's rules" for every replay: replays two and
	three start from parameters an Adam step has moved, and that step's gradients hold float-atomic sums, so two correct captures no longer
	evaluate the same forward; their terms are held to the 1e-4 * max(1, |term|) of that same test instead."""
	from find_amd.graph import GraphedStep
	from test_gpu_train3d import FixedDraws
	from test_gpu_trainloop import _draws, _setup
	lr, order = 5e-4, (0, 3, 1)
	draws = _draws(1002, 1002)
	runs = []
	for byte in (None, 0xFF):
		mwl, opts, batch_of, _, opt = _setup(1002, 1002, capturable=True)
		with FixedDraws(draws):
			with (poisoned(byte) if byte is not None else contextlib.nullcontext()):
				gs = GraphedStep(mwl, opts, [opt], warmup=1, **opts.net_train_kwargs())
				first = gs(batch_of(order[0]))   # warm-up and capture happen in the first call
			terms = [first] + [gs(batch_of(k)) for k in order[1:]]
			terms = [(loss.detach().clone(), {k: v.detach().clone() for k, v in losses.items()}) for loss, losses in terms]
		torch.cuda.synchronize()
		assert len(gs._graphs) == 1
		runs.append((terms, {n: p.detach().clone() for n, p in mwl.model.named_parameters()}))
	(t0, p0), (t1, p1) = runs
	# the first replay starts from identical parameters: its terms are forwards of identical inputs
	assert torch.equal(t0[0][0], t1[0][0]) and all(torch.equal(t0[0][1][k], t1[0][1][k]) for k in t0[0][1])
	for (la, ta), (lb, tb) in zip(t0, t1):
		assert torch.isfinite(lb) and set(ta) == set(tb)
		for k in ta:
			assert torch.isfinite(tb[k]) and abs(ta[k].item() - tb[k].item()) <= 1e-4 * max(1.0, abs(ta[k].item())), (k, ta[k].item(), tb[k].item())
	for n, p in p0.items():
		assert torch.isfinite(p1[n]).all(), n
		d = (p1[n] - p).abs()
		assert (d > 0.1 * lr).float().mean().item() < 1e-3, (n, (d > 0.1 * lr).float().mean().item())
		assert d.max().item() < 0.1 * lr * len(order), (n, d.max().item())
