"""The surface sampler (find_sample_surface_fwd / _again: face_areas_kernel -> area_scan_kernel -> sample_surface_kernel) against float64,
at scan sizes: one round of area_scan_kernel is 1024 threads x CDF_PER 16 = 16 384 faces, and F runs from 1 to 100 003 (F % 4 != 0 takes the
scalar path), with zero-area faces at face 0, at thread starts, at round starts and at the last face, and ragged batches that pad each
mesh with its own number of -1 faces (padding starting on a 16-face boundary, inside a thread's run, on a round boundary).

The running sum is read back from a workspace the test owns (include/find_hip.h: it stays in `ws` for find_sample_surface_again).

The bound on the running sum.  The float64 reference is the cumulative sum of the kernel's own float32 areas (find_face_areas; the areas
themselves are held to the float64 oracle in test_gpu_geom), so only the scan's float32 additions are measured.  Every partial sum the
scan forms is a sum of non-negative areas, so by the standard bound for a summation tree (each input is multiplied by at most one
(1 + delta), |delta| <= u = 2^-24, per addition on its path to the result) a partial sum is within gamma_D * S of the exact one, with
gamma_D = D u / (1 - D u), D the depth of that path and S the exact sum of the inputs.  The path of an area in round r:
   15 in-thread additions + 6 levels of the wave's shuffle scan            (to the wave total)
 + 16 additions per earlier round (carry += the 16 wave totals)
 + 15 additions of the wave totals into the thread's base
 + 1 (inc - a[15]) + 1 (base + that) + 1 (off + a[k])                      ->  D(r) = 38 + 16 (r + 1)   (round 0 included, generously)
The subtraction inc - a[15] removes the thread's own total a second time: its rounding in inc (<= 6 levels) is left behind, at most
gamma_6 * S more.  So a stored value may be off by BOUND(f) = 2 gamma_D(r) * S_end(f), S_end the exact sum through the end of f's thread
(the thread has read those areas).  The stored value is the running max of such partial sums over positive-area faces, so it inherits the
same bound against the (non-decreasing) exact cumulative sum."""
import numpy as np
import pytest
import torch

from oracle import geom_ref as G

pytestmark = pytest.mark.gpu

ROUND = 1024 * 16
U32 = 2.0 ** -24
C_OUT, A_OUT = 4.0, 1e-7   # the bar of test_gpu_mlp_f64 (outputs: absolute; gradients: relative to the largest float64 entry)
C_REL, A_REL = 4.0, 2e-7

F_SIZES = [1, 15, 16, 17, 16383, 16384, 16385, 20000, 100000, 100003]


def _gamma(d):
	return d * U32 / (1.0 - d * U32)


def scan_bound(s64):
	"""BOUND(f) of the module docstring for a float64 cumulative sum s64 (F,) of one mesh's float32 areas."""
	F = s64.shape[0]
	f = np.arange(F)
	end = np.minimum((f // 16) * 16 + 15, F - 1)
	depth = 38 + 16 * (f // ROUND + 1)
	return 2.0 * _gamma(depth) * s64[end]


def sampler_case(F, N, ragged, seed):
	"""Verts (N, V, 3) float32 (random irregular triangles: areas over two orders of magnitude), faces (F, 3) or (N, F, 3) int32 with -1
	padding, n_real (N,) = the rows before the padding.  Zero-area faces (a repeated vertex) at face 0, the thread starts 16, 32, the round
	starts and the last real face, where those exist."""
	g = np.random.default_rng(seed)
	V = max(3, min(F + 2, 60000))
	verts = (g.standard_normal((N, V, 3)) * 0.05).astype(np.float32)
	scale = np.exp(g.uniform(-2.5, 2.5, (N, V, 1))).astype(np.float32)   # irregular sizes
	verts = verts * scale
	f0, o1, o2 = g.integers(0, V, F), g.integers(1, V, F), g.integers(1, V - 1, F)
	faces = np.stack([f0, (f0 + o1) % V, (f0 + o2 + (o2 >= o1)) % V], 1)   # three distinct vertices

	def zero(fs, i):
		fs[i, 1] = fs[i, 0]

	for i in [0, 16, 32, 33] + list(range(ROUND, F, ROUND)) + list(range(ROUND - 1, F, ROUND)):
		if F > 1 and i < F - 1:
			zero(faces, i)
	n_real = np.full(N, F)
	if not ragged:
		if F > 2:
			zero(faces, F - 1)
		return verts, faces.astype(np.int32), n_real
	fb = np.repeat(faces[None], N, 0)
	starts = [F, (F // 16) * 16, (F // 16) * 16 - 9, (F // ROUND) * ROUND, F - 1, F - 40, F // 2]
	for n in range(N):
		s = starts[n % len(starts)] - (n // len(starts)) * 16
		s = int(min(F, max(1 if F < 3 else 2, s)))
		fb[n, s:] = -1
		n_real[n] = s
		if s > 2 and n % 2 == 0:
			zero(fb[n], s - 1)      # a zero-area last real face just before the padding
	return verts, fb.astype(np.int32), n_real


def run_sampler(verts, faces, rnd, attr=None, again_ws=None):
	"""find_sample_surface_fwd (or _again on a given workspace) through _lib: (face_idx, uv, out, attr_out, ws)."""
	from find_amd import _lib
	L = _lib.lib()
	N, V, _ = verts.shape
	F = faces.shape[-2]
	S = rnd.shape[1]
	fb = 1 if faces.dim() == 2 else N
	dev = verts.device
	face_idx = torch.empty(N, S, device=dev, dtype=torch.int32)
	uv = torch.empty(N, S, 2, device=dev)
	out = torch.empty(N, S, 3, device=dev)
	aout = torch.empty(N, S, 3, device=dev) if attr is not None else None
	if again_ws is None:
		nb = L.find_sample_surface_ws_bytes(N, F)
		ws = torch.full((nb // 4,), float('nan'), device=dev)
		_lib.check(L.find_sample_surface_fwd(_lib.ptr(verts), _lib.ptr(faces), fb, _lib.ptr(rnd), N, V, F, S, _lib.ptr(face_idx), _lib.ptr(uv),
											 _lib.ptr(out), _lib.ptr(attr), _lib.ptr(aout), _lib.ptr(ws), nb, _lib.current_stream(dev)),
				   'find_sample_surface_fwd')
	else:
		ws = again_ws
		_lib.check(L.find_sample_surface_again(_lib.ptr(verts), _lib.ptr(faces), fb, _lib.ptr(rnd), N, V, F, S, _lib.ptr(face_idx), _lib.ptr(uv),
											   _lib.ptr(out), _lib.ptr(attr), _lib.ptr(aout), _lib.ptr(ws), ws.numel() * 4,
											   _lib.current_stream(dev)), 'find_sample_surface_again')
	torch.cuda.synchronize()
	return face_idx, uv, out, aout, ws


def check_running_sum(c, a32):
	"""c (F,) the stored running sum, a32 (F,) the float32 areas of one mesh.  Returns (max |c - s64| / bound, s64, bound)."""
	c64 = c.astype(np.float64)
	s64 = np.cumsum(a32.astype(np.float64))
	bound = scan_bound(s64)
	F = c.shape[0]
	d = np.diff(c64)
	down = np.nonzero(d < 0)[0]
	assert down.size == 0, f'running sum decreases at {down.size} faces, first {down[:5] + 1}: {d[down[:5]]}'
	zero = np.nonzero(a32 == 0)[0]
	zi = zero[zero > 0]
	steps = c64[zi] - c64[zi - 1]
	assert (steps == 0).all(), f'{int((steps != 0).sum())} zero-area faces with a non-zero step, first {zi[steps != 0][:5]}'
	if a32[0] == 0:
		assert c64[0] == 0.0, c64[0]
	pos = np.nonzero(a32 > 0)[0]
	if pos.size:
		last = pos[-1]
		assert c[F - 1] == c[last], f'total {c[F - 1]!r} != running sum at the last positive face {last}: {c[last]!r}'
	err = np.abs(c64 - s64)
	ratio = float((err / np.maximum(bound, 1e-300)).max()) if F else 0.0
	assert (err <= bound).all(), f'running sum off float64 by {err.max():.3e} (> bound at {int((err > bound).sum())} faces), ratio {ratio:.2f}'
	return ratio, s64, bound


def adversarial_draws(c, s64, a32, n_rand, g):
	"""Draws in [0,1): 0, 1e-9, 1 - 2^-24; every float64 boundary s64[f] / total and its two float32 neighbours; a draw aimed into every
	interval that the stored sum c gives a zero-area face; then n_rand uniform ones."""
	tot = s64[-1]
	b = (s64 / tot).astype(np.float32)
	bnd = np.concatenate([b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(2))])
	zi = np.nonzero(a32 == 0)[0]
	ctot = np.float64(c[-1])
	aims = []
	if ctot > 0 and zi.size:
		lo = np.where(zi > 0, c[np.maximum(zi - 1, 0)], 0.0).astype(np.float64)
		hi = c[zi].astype(np.float64)
		aims = [((lo + hi) / 2 / ctot).astype(np.float32), (hi / ctot).astype(np.float32), np.nextafter((hi / ctot).astype(np.float32), np.float32(0))]
	d = np.concatenate([np.array([0.0, 1e-9, 1.0 - 2.0 ** -24], np.float32), bnd] + aims + [g.random(n_rand, dtype=np.float32)])
	return np.clip(d, 0.0, np.float32(1.0 - 2.0 ** -24)).astype(np.float32)


def check_choice(got, draws, s64, bound, a64, n_real):
	"""The face of every draw against searchsorted on the float64 sum.  Returns the number of draws that differ (all within rounding)."""
	F = s64.shape[0]
	assert got.min() >= 0 and got.max() < n_real, f'a padding row was chosen: max face {got.max()}, real faces {n_real}'
	assert (a64[got] > 0).all(), f'zero-area faces chosen: {np.unique(got[a64[got] <= 0])[:10]}'
	tot = s64[-1]
	r64 = draws.astype(np.float64) * tot
	want = np.minimum(np.searchsorted(s64, r64, side='right'), F - 1)
	bad = np.nonzero(got != want)[0]
	if bad.size:
		lo = np.minimum(got[bad], want[bad])
		hi = np.maximum(got[bad], want[bad])
		# tolerance: the stored sum's bound at the far face, the stored total's own bound (the draw is scaled by it), and the rounding of
		# fl(rnd * total) and of the clamp below the total (one u each, relative to the total)
		t = bound[hi] + bound[-1] + 2 * U32 * tot
		near = (np.abs(s64[lo] - r64[bad]) <= t) & (np.abs(s64[hi - 1] - r64[bad]) <= t)
		assert near.all(), (f'{int((~near).sum())} draws choose a face beyond rounding: draw {draws[bad][~near][:5]}, '
							f'got {got[bad][~near][:5]}, want {want[bad][~near][:5]}')
		# only faces of zero or rounding-level area between the two
		between = s64[hi - 1] - s64[lo]
		assert (between <= 2 * t).all(), between.max()
	return int(bad.size)


@pytest.mark.parametrize('F', F_SIZES)
@pytest.mark.parametrize('N,ragged', [(1, False), (3, False), (3, True), (16, True)])
def test_sampler_running_sum_and_face_choice_vs_float64(F, N, ragged):
	from find_amd import functional as FN
	verts, faces, n_real = sampler_case(F, N, ragged, seed=F * 7 + N * 3 + ragged)
	v = torch.from_numpy(verts).cuda()
	fc = torch.from_numpy(faces).cuda()
	a32 = FN.face_areas(v, fc).cpu().numpy()
	fl = faces if faces.ndim == 3 else np.repeat(faces[None], N, 0)
	a64 = G.face_areas(torch.from_numpy(verts).double(), torch.from_numpy(np.maximum(fl, 0)).long()).numpy()
	a64[fl[..., 0] < 0] = 0.0
	assert ((a32 == 0) == (a64 == 0)).all()
	# pass 1: uniform draws only, to read the running sum
	g = np.random.default_rng(F + N)
	rnd0 = torch.rand(N, 64, 3, generator=torch.Generator().manual_seed(F)).cuda()
	_, _, _, _, ws = run_sampler(v, fc, rnd0)
	c = ws[:N * F].view(N, F).cpu().numpy()
	draws, ratios, sums = [], [], []
	for n in range(N):
		ratio, s64, bound = check_running_sum(c[n], a32[n])
		ratios.append(ratio)
		sums.append((s64, bound))
		draws.append(adversarial_draws(c[n], s64, a32[n], 2048, g))
	S = max(d.shape[0] for d in draws)
	rnd = np.random.default_rng(F * 3 + N).random((N, S, 3), dtype=np.float32)
	for n in range(N):
		rnd[n, :draws[n].shape[0], 0] = draws[n]
	rnd_t = torch.from_numpy(rnd).cuda()
	fi, uv, out, _, ws1 = run_sampler(v, fc, rnd_t)
	assert torch.equal(ws1[:N * F].view(N, F).cpu(), torch.from_numpy(c)), 'the running sum differs between two runs'
	got = fi.cpu().numpy().astype(np.int64)
	nbad = 0
	for n in range(N):
		nbad += check_choice(got[n], rnd[n, :, 0], sums[n][0], sums[n][1], a64[n], n_real[n])
	# _again on the kept sum: bit for bit; and a repeat of the whole call: bit for bit
	fi2, uv2, out2, _, _ = run_sampler(v, fc, rnd_t, again_ws=ws1)
	fi3, uv3, out3, _, _ = run_sampler(v, fc, rnd_t)
	for x, y in [(fi, fi2), (uv, uv2), (out, out2), (fi, fi3), (uv, uv3), (out, out3)]:
		assert torch.equal(x, y)
	print(f'[sampler F={F} N={N} ragged={ragged}] running sum err / bound max {max(ratios):.3e}; {N * S} draws, '
		  f'{nbad} differ from float64 searchsorted (all within rounding)')


def _points_case(V, N, seed):
	from find_amd import synthetic
	v, f = synthetic.template(V)
	g = torch.Generator().manual_seed(seed)
	verts = v[None] + 0.003 * torch.randn(N, v.shape[0], 3, generator=g)
	col = torch.rand(verts.shape, generator=g)
	return verts, f, col


@pytest.mark.parametrize('V,N', [(6890, 16), (50002, 3)])
def test_sampler_points_colours_and_backward_vs_float64(V, N):
	"""Points, colours and the scatter backward (float atomics) of FN.sample_surface against float64 for the faces HIP chose:
	e_hip <= C * e_fp32 + A, e_fp32 the float32 restatement's own error against float64."""
	from find_amd import functional as FN
	verts, faces, col = _points_case(V, N, seed=V + N)
	S = 5000
	rnd = torch.rand(N, S, 3, generator=torch.Generator().manual_seed(V))
	vg = verts.clone().cuda().requires_grad_(True)
	cg = col.clone().cuda().requires_grad_(True)
	pts, cs, fi, uv = FN.sample_surface(vg, faces.cuda(), rnd.cuda(), cg)
	w1 = torch.randn(N, S, 3, generator=torch.Generator().manual_seed(1))
	w2 = torch.randn(N, S, 3, generator=torch.Generator().manual_seed(2))
	((pts * w1.cuda()).sum() + (cs * w2.cuda()).sum()).backward()
	got = fi.cpu().long()
	a64 = G.face_areas(verts.double(), faces)
	assert (a64.gather(1, got) > 0).all()
	res = {}
	for dt in (torch.float64, torch.float32):
		vr = verts.to(dt).requires_grad_(True)
		cr = col.to(dt).requires_grad_(True)
		rp, rc = G.sample_points(vr, faces, got, uv.cpu().to(dt), attr=cr)
		((rp * w1.to(dt)).sum() + (rc * w2.to(dt)).sum()).backward()
		res[dt] = (rp.detach().double(), rc.detach().double(), vr.grad.double(), cr.grad.double())
	hip = (pts.detach().cpu().double(), cs.detach().cpu().double(), vg.grad.cpu().double(), cg.grad.cpu().double())
	for k, name in enumerate(['points', 'colours', 'd_verts', 'd_colours']):
		ref = res[torch.float64][k]
		e_hip = (hip[k] - ref).abs().max().item()
		e32 = (res[torch.float32][k] - ref).abs().max().item()
		if k < 2:
			bar = C_OUT * e32 + A_OUT
		else:
			s = ref.abs().max().item()
			e_hip, e32 = e_hip / s, e32 / s
			bar = C_REL * e32 + A_REL
		print(f'[sampler points V={V} N={N}] {name}: e_hip {e_hip:.3e}  e_fp32 {e32:.3e}  bar {bar:.3e}')
		assert e_hip <= bar, (name, e_hip, e32, bar)
