"""The Chamfer term's fused backward (chamfer_surface_bwd_kernel, find_amd/csrc/geom.hip: neighbours -> d_verts in one workgroup's LDS)
against a float64 sum over the neighbours the GPU forward chose, held to the error of the pair it replaces (find_chamfer_bwd +
find_sample_points_bwd): e_new <= 4 e_old + 1e-7 max|d_verts|.  Shapes: the smallest at which the kernel can go
wrong -- one item, either side of a wave and of a 1024-thread round, a gradient image whose length is no multiple of 4 floats, one face
(every add on the same three rows), ragged and empty target clouds, every slice count the size rule can choose."""
import pytest
import torch

pytestmark = pytest.mark.gpu

G_LOSS = 0.7


def _slices(k):
	"""The switch field that forces k slices per foot (find_render_switches, bits 0x70000); 0 leaves the size rule alone."""
	return 0 if k == 0 else (k.bit_length() << 16)


def _keys(ws, n, p1, p2):
	off = (n * p1 * 8 + 255) // 256 * 256   # the workspace is carved in 256-byte steps: kx, then ky
	return ws[:n * p1 * 8].view(torch.int64).view(n, p1).cpu(), ws[off:off + n * p2 * 8].view(torch.int64).view(n, p2).cpu()


def _forward(verts, faces, rnd, y, yl):
	"""The sampler and the Chamfer forward as surface_chamfer issues them -> x, face_idx, uv, the Chamfer workspace."""
	from find_amd import _lib
	from find_amd import functional as FN
	from find_amd._lib import check, current_stream, ptr
	L = _lib.lib()
	x, _, face_idx, uv = FN.sample_surface(verts, faces, rnd)
	n, p1, _ = x.shape
	p2 = y.shape[1]
	ws = torch.zeros(L.find_chamfer_ws_bytes(n, p1, p2), dtype=torch.uint8, device=x.device)
	loss = torch.zeros((), device=x.device)
	check(L.find_chamfer_fwd(ptr(x), None, ptr(y), ptr(yl), n, p1, p2, ptr(loss), ptr(ws), ws.numel(), current_stream(x.device)), 'find_chamfer_fwd')
	torch.cuda.synchronize()
	return x, face_idx, uv, ws


def _reference(x, y, yl, faces, face_idx, uv, ws, n_verts):
	"""d_verts in float64 on the CPU from the forward's own neighbours, samples and draws."""
	n, p1, _ = x.shape
	p2 = y.shape[1]
	kx, ky = _keys(ws, n, p1, p2)
	x64, y64, uv64 = x.double().cpu(), y.double().cpu(), uv.double().cpu()
	faces, face_idx = faces.cpu().long(), face_idx.cpu().long()
	lens = [p2] * n if yl is None else yl.cpu().tolist()
	d_verts = torch.zeros(n, n_verts, 3, dtype=torch.float64)
	for m in range(n):
		d_x = torch.zeros(p1, 3, dtype=torch.float64)
		ok = kx[m] != -1
		j = (kx[m][ok] & 0xffffffff).long()
		d_x[ok] += 2.0 * G_LOSS / (n * max(p1, 1)) * (x64[m][ok] - y64[m][j])
		k = torch.arange(p2) < lens[m]
		k &= ky[m] != -1
		j = (ky[m][k] & 0xffffffff).long()
		d_x.index_add_(0, j, -2.0 * G_LOSS / (n * max(lens[m], 1)) * (y64[m][k] - x64[m][j]))
		us = uv64[m, :, 0].sqrt()
		w = torch.stack([1.0 - us, us * (1.0 - uv64[m, :, 1]), us * uv64[m, :, 1]], dim=-1)
		f = (faces if faces.dim() == 2 else faces[m])[face_idx[m]]
		for c in range(3):
			d_verts[m].index_add_(0, f[:, c], w[:, c:c + 1] * d_x)
	return d_verts


def _old_pair(x, y, yl, faces, face_idx, uv, ws, n_verts):
	from find_amd import _lib
	from find_amd._lib import check, current_stream, ptr
	L = _lib.lib()
	n, p1, _ = x.shape
	p2 = y.shape[1]
	g = torch.full((), G_LOSS, device=x.device)
	d_x = torch.zeros_like(x)
	d_verts = torch.zeros(n, n_verts, 3, device=x.device)
	s = current_stream(x.device)
	check(L.find_chamfer_bwd(ptr(x), None, ptr(y), ptr(yl), n, p1, p2, ptr(g), ptr(ws), ws.numel(), ptr(d_x), None, s), 'find_chamfer_bwd')
	fb = 1 if faces.dim() == 2 else faces.shape[0]
	check(L.find_sample_points_bwd(ptr(faces), fb, ptr(face_idx), ptr(uv), ptr(d_x), n, n_verts, faces.shape[-2], p1, ptr(d_verts), s), 'find_sample_points_bwd')
	torch.cuda.synchronize()
	return d_verts.double().cpu()


def _fused(x, y, yl, faces, face_idx, uv, ws, n_verts, slices):
	from find_amd import _lib
	from find_amd._lib import check, current_stream, ptr
	L = _lib.lib()
	n, p1, _ = x.shape
	p2 = y.shape[1]
	g = torch.full((), G_LOSS, device=x.device)
	d_verts = torch.full((n, n_verts, 3), float('nan'), device=x.device)   # the kernel overwrites: nothing of this may survive
	fb = 1 if faces.dim() == 2 else faces.shape[0]
	_lib.set_tuning('raster_ablate', _slices(slices))
	try:
		nbytes = L.find_chamfer_surface_bwd_ws_bytes(n, n_verts, p1)
		assert nbytes >= 0
		bws = torch.full((max(nbytes, 256),), 0xff, dtype=torch.uint8, device=x.device)   # (NaN slabs: every slab element is written before it is read)
		check(L.find_chamfer_surface_bwd(ptr(x), ptr(y), ptr(yl), n, p1, p2, ptr(g), ptr(ws), ws.numel(), ptr(faces), fb, ptr(face_idx), ptr(uv), n_verts,
										 faces.shape[-2], ptr(d_verts), ptr(bws), bws.numel(), current_stream(x.device)), 'find_chamfer_surface_bwd')
		torch.cuda.synchronize()
	finally:
		_lib.set_tuning('raster_ablate', 0)
	return d_verts.double().cpu()


def _inputs(n, V, F, p1, p2, shared, ragged, seed):
	g = torch.Generator().manual_seed(seed)
	verts = (torch.rand(n, V, 3, generator=g) * 0.2).cuda()
	# three different corners per face (the sampler never picks a face without area, and F = 1 needs its only face)
	shape = (F, 3) if shared else (n, F, 3)
	faces = torch.stack([torch.randperm(V, generator=g)[:3] for _ in range(F if shared else n * F)]).to(torch.int32).view(shape).cuda()
	rnd = torch.rand(n, p1, 3, generator=g).cuda()
	y = (torch.rand(n, p2, 3, generator=g) * 0.2 + 0.05).cuda()
	yl = None
	if ragged:
		lens = [p2, 0, max(p2 // 2, 1)][:n] if n > 1 else [max(p2 - 1, 1)]
		yl = torch.tensor(lens, dtype=torch.int32).cuda()
	return verts, faces, rnd, y, yl


_CACHE = {}


def _case(key):
	"""Forward, float64 reference and the old pair's gradient of a case: computed once, shared by the slice counts."""
	if key not in _CACHE:
		n, V, F, p1, p2, shared, ragged = key
		verts, faces, rnd, y, yl = _inputs(*key, seed=sum(key))
		x, face_idx, uv, ws = _forward(verts, faces, rnd, y, yl)
		args = (x, y, yl, faces, face_idx, uv, ws, V)
		_CACHE[key] = (args, _reference(*args), _old_pair(*args))
	return _CACHE[key]


def _holds(new, old, ref):
	scale = ref.abs().max().item()
	e_new, e_old = (new - ref).abs().max().item(), (old - ref).abs().max().item()
	print(f'scale {scale:.3e}  e_old {e_old:.3e}  e_new {e_new:.3e}')
	assert torch.isfinite(new).all()
	assert e_new <= 4 * e_old + 1e-7 * scale, (e_new, e_old, scale)
	return scale


#        n  V    F    p1    p2    shared ragged
CASES = [(1, 3, 1, 1, 2, True, False),
		 (1, 7, 5, 63, 40, True, True),
		 (3, 7, 5, 63, 70, False, True),
		 (3, 257, 500, 1025, 700, True, True),
		 (1, 257, 500, 1025, 1100, False, False),
		 (3, 3, 1, 1025, 63, True, True),
		 (1, 257, 1, 63, 1025, True, False)]


@pytest.mark.parametrize('slices', [0, 1, 2, 4, 8])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'n{}-V{}-F{}-p{}x{}-{}{}'.format(*c[:5], 'shared' if c[5] else 'own', '-ragged' if c[6] else ''))
def test_fused_backward_is_as_close_to_float64_as_the_pair_it_replaces(case, slices):
	args, ref, old = _case(case)
	new = _fused(*args, slices)
	scale = _holds(new, old, ref)
	assert scale > 0
	yl = args[2]
	if yl is not None:
		for m, length in enumerate(yl.cpu().tolist()):
			if length == 0:   # no target: direction 1 has no item, direction 0 only ~0 keys -- exact zeros, not what the buffer held
				assert (new[m] == 0).all() and (old[m] == 0).all()


def _largest_fitting_verts():
	from find_amd import _lib
	L = _lib.lib()
	lo, hi = 1, 1 << 20   # fits, does not fit
	assert L.find_chamfer_surface_bwd_ws_bytes(1, lo, 64) >= 0 and L.find_chamfer_surface_bwd_ws_bytes(1, hi, 64) < 0
	while hi - lo > 1:
		mid = (lo + hi) // 2
		lo, hi = (mid, hi) if L.find_chamfer_surface_bwd_ws_bytes(1, mid, 64) >= 0 else (lo, mid)
	return lo


@pytest.mark.parametrize('slices', [1, 2])
def test_largest_gradient_image_that_fits_the_lds(slices):
	V = _largest_fitting_verts()
	assert 160 * 1024 - 32 < V * 12 + 64 * 12 <= 160 * 1024   # the image and d_x of the 64 samples: all of a CU's LDS but the alignment slack
	args, ref, old = _case((2, V, 8, 64, 50, True, False))
	_holds(_fused(*args, slices), old, ref)


class _Meshes:
	"""What DisplacementLoss reads of a Meshes."""

	def __init__(self, verts, faces):
		self.v, self.f = verts, faces

	def verts_padded(self):
		return self.v

	def faces_shared(self):
		return self.f if self.f.dim() == 2 else None

	def faces_padded(self):
		return self.f


_ORIGINALS = {}


def _displacement(monkeypatch, fused, verts, faces, gt, seed, gt_z_cutoff, graph=False):
	"""DisplacementLoss on one seed -> (loss, the predicted samples it drew, verts.grad)."""
	from find_amd import functional as FN
	from find_amd import losses
	seen, fused_calls = [], []
	sample_surface, surface_chamfer_distance = _ORIGINALS.setdefault('fn', (FN.sample_surface, FN.surface_chamfer_distance))   # (not an earlier call's spies)

	def spy_sample(*a, **k):
		r = sample_surface(*a, **k)
		seen.append(r[0])
		return r

	def spy_fused(*a, **k):
		fused_calls.append(1)
		return surface_chamfer_distance(*a, **k)
	monkeypatch.setattr(FN, 'sample_surface', spy_sample)
	monkeypatch.setattr(FN, 'surface_chamfer_distance', spy_fused)
	monkeypatch.setattr(losses, 'FUSED_CHAMFER_BWD', 2 if fused else 0)   # (2: also below the size rule)
	v = verts.clone().requires_grad_(True)

	def run():
		loss = losses.DisplacementLoss()(None, dict(meshes=_Meshes(v, faces)), {}, 0, num_samples=gt.shape[1], gt_z_cutoff=gt_z_cutoff, gt_samples=gt)['loss']
		return loss, torch.autograd.grad(loss * G_LOSS, v)[0]
	if graph:
		g = torch.cuda.CUDAGraph()
		torch.cuda.synchronize()
		with torch.cuda.graph(g):
			loss, grad = run()
		torch.manual_seed(seed)
		g.replay()
	else:
		torch.manual_seed(seed)
		loss, grad = run()
	torch.cuda.synchronize()
	assert len(seen) == 1 and len(fused_calls) == (1 if fused else 0)
	return loss.clone(), seen[0].clone(), grad.clone()


@pytest.mark.parametrize('gt_z_cutoff', [None, 0.1])
def test_displacement_loss_fused_against_forced_old(monkeypatch, gt_z_cutoff):
	"""Eagerly and inside a captured graph: the same samples and loss bit for bit, verts.grad within the criterion."""
	from find_amd import losses
	n, V, F, S = 3, 257, 500, 1025
	verts, faces, _, gt, _ = _inputs(n, V, F, S, S, True, False, seed=11)
	for graph in (False, True):
		l1, x1, g1 = _displacement(monkeypatch, True, verts, faces, gt, 5, gt_z_cutoff, graph)
		l0, x0, g0 = _displacement(monkeypatch, False, verts, faces, gt, 5, gt_z_cutoff, graph)
		assert torch.equal(l1, l0) and torch.equal(x1, x0) and float(l1) > 0
		# the float64 sum from the same draw
		torch.manual_seed(5)
		rnd = torch.rand(n, S, 3, device=verts.device)
		y, yl = (gt, None) if gt_z_cutoff is None else losses._compact_by_mask(gt, gt[..., 2] <= gt_z_cutoff)
		x, face_idx, uv, ws = _forward(verts, faces, rnd, y.contiguous(), yl)
		assert torch.equal(x, x1)
		ref = _reference(x, y, yl, faces, face_idx, uv, ws, V)
		_holds(g1.double().cpu(), g0.double().cpu(), ref)


def test_one_vertex_too_many_keeps_the_old_path(monkeypatch):
	from find_amd import _lib
	from find_amd import functional as FN
	L = _lib.lib()
	V = _largest_fitting_verts() + 1
	assert L.find_chamfer_surface_bwd_ws_bytes(2, V, 64) < 0 and not FN.surface_chamfer_fits(2, V, 64)
	verts, faces, _, gt, _ = _inputs(2, V, 8, 64, 64, True, False, seed=3)
	with pytest.raises(RuntimeError, match='do not fit'):
		FN.surface_chamfer(verts.clone().requires_grad_(True), faces, torch.rand(2, 64, 3, device='cuda'), gt)
	monkeypatch.setattr(FN, 'surface_chamfer_distance', lambda *a, **k: pytest.fail('fused path taken'))   # whatever the switch says
	from find_amd import losses
	out = []
	for on in (2, 0):
		monkeypatch.setattr(losses, 'FUSED_CHAMFER_BWD', on)
		v = verts.clone().requires_grad_(True)
		torch.manual_seed(9)
		loss = losses.DisplacementLoss()(None, dict(meshes=_Meshes(v, faces)), {}, 0, num_samples=64, gt_samples=gt)['loss']
		out.append((loss.clone(), torch.autograd.grad(loss, v)[0]))
	assert torch.equal(out[0][0], out[1][0]) and float(out[0][0]) > 0
	# the same kernels on the same inputs: float atomics may still land in another order
	scale = out[1][1].abs().max().item()
	assert scale > 0 and (out[0][1] - out[1][1]).abs().max().item() <= 1e-5 * scale
