"""The Chamfer search through balanced tiles (nn_tile_build_kernel / nn_tile_query_kernel, find_amd/csrc/geom.hip) against all pairs
(nn_kernel): the same 64-bit keys (distance bits << 32 | lowest index) and the same loss, bit for bit, on the smallest shapes at which
the tiling or the culling can go wrong, and at the build's capacity (8192 points, 8 per thread, 128 tiles).  Bit 16384 of the profiling switch forces the tile path from 64 points per cloud on, bit 512
forces all pairs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TILES, BRUTE = 16384, 512


def _sphere(g, n, p, r=0.1, noise=1e-3):
	v = torch.randn(n, p, 3, generator=g)
	return v / v.norm(dim=-1, keepdim=True) * r + noise * torch.randn(n, p, 3, generator=g)


def _fwd(x, y, xl, yl, bits):
	"""find_chamfer_fwd with a workspace of the test's own -> (kx, ky, loss, ws)."""
	from find_amd import _lib
	from find_amd._lib import check, current_stream, ptr
	L = _lib.lib()
	n, p1, _ = x.shape
	p2 = y.shape[1]
	nbytes = L.find_chamfer_ws_bytes(n, p1, p2)
	assert nbytes > 0
	ws = torch.zeros(nbytes, dtype=torch.uint8, device=x.device)
	loss = torch.zeros((), device=x.device)
	_lib.set_tuning('raster_ablate', bits)
	try:
		check(L.find_chamfer_fwd(ptr(x), ptr(xl), ptr(y), ptr(yl), n, p1, p2, ptr(loss), ptr(ws), ws.numel(), current_stream(x.device)), 'find_chamfer_fwd')
		torch.cuda.synchronize()
	finally:
		_lib.set_tuning('raster_ablate', 0)
	return (*_keys(ws, n, p1, p2), loss.clone(), ws)


def _keys(ws, n, p1, p2):
	off = (n * p1 * 8 + 255) // 256 * 256   # the workspace is carved in 256-byte steps: kx, then ky
	return ws[:n * p1 * 8].view(torch.int64).clone(), ws[off:off + n * p2 * 8].view(torch.int64).clone()


def _bwd(x, y, xl, yl, ws):
	from find_amd import _lib
	from find_amd._lib import check, current_stream, ptr
	L = _lib.lib()
	n, p1, _ = x.shape
	p2 = y.shape[1]
	g = torch.ones((), device=x.device)
	dx, dy = torch.zeros_like(x), torch.zeros_like(y)
	check(L.find_chamfer_bwd(ptr(x), ptr(xl), ptr(y), ptr(yl), n, p1, p2, ptr(g), ptr(ws), ws.numel(), ptr(dx), ptr(dy), current_stream(x.device)), 'find_chamfer_bwd')
	torch.cuda.synchronize()
	return dx, dy


def _cases():
	g = torch.Generator().manual_seed(4242)
	i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
	c = {}
	c['surface'] = (_sphere(g, 3, 1000), _sphere(g, 3, 777), None, None)
	c['blob'] = (torch.randn(2, 500, 3, generator=g) * 0.05, torch.randn(2, 500, 3, generator=g) * 0.05, None, None)
	# clouds of exactly 1, 63, 64, 65 and 129 points on either side (lengths), and whole tensors of 64, 65 and 129
	c['tile edges'] = (_sphere(g, 5, 129), _sphere(g, 5, 129), i32(1, 63, 64, 65, 129), i32(129, 65, 64, 63, 1))
	c['tile edges 64'] = (_sphere(g, 1, 64), _sphere(g, 1, 65), None, None)
	c['tile edges 129'] = (_sphere(g, 1, 129), _sphere(g, 1, 64), None, None)
	c['ragged'] = (_sphere(g, 3, 400), _sphere(g, 3, 300), i32(400, 0, 250), i32(300, 100, 0))
	xd, yd = _sphere(g, 1, 600), _sphere(g, 1, 600)
	yd[0, 100:200] = yd[0, 0:100]          # duplicated targets
	yd[0, 599] = yd[0, 3]                  # ... far apart in index
	xd[0, :50] = yd[0, 100:150]            # queries exactly on duplicated targets (distance 0 to two indices: the lowest must win)
	xd[0, 50] = yd[0, 599]
	c['duplicates'] = (xd, yd, None, None)
	yc = _sphere(g, 1, 500)
	yc[0, 100:400] = yc[0, 100].clone()    # 300 coincident targets
	c['coincident'] = (_sphere(g, 1, 500), yc, None, None)
	c['all coincident'] = (_sphere(g, 1, 200), torch.full((1, 200, 3), 0.25), None, None)
	line = torch.linspace(-1, 1, 300)[None, :, None] * torch.tensor([0.3, -0.2, 0.1])
	c['collinear'] = (line + 0.0, _sphere(g, 1, 300), None, None)
	plane = _sphere(g, 1, 400) * torch.tensor([1.0, 1.0, 0.0])
	c['coplanar'] = (plane, _sphere(g, 1, 400) * torch.tensor([1.0, 0.0, 1.0]), None, None)
	xo = _sphere(g, 1, 700)
	xo[0, :64] = xo[0, :64] * 50.0 + 3.0   # queries far outside the targets' box
	c['outliers'] = (xo, _sphere(g, 1, 700), None, None)
	off = torch.tensor([50.0, -120.0, 7.0])
	c['far from the origin'] = (_sphere(g, 2, 900) + off, _sphere(g, 2, 900, noise=2e-3) + off, None, None)
	flat = torch.tensor([1.0, 1.0, 0.01])
	c['far from the origin, flat'] = (_sphere(g, 1, 800, r=0.02) * flat + 300.0, _sphere(g, 1, 800, r=0.02) * flat + 300.0, None, None)
	c['many feet'] = (_sphere(g, 16, 320), _sphere(g, 16, 320), None, None)
	c['training shape'] = (_sphere(g, 2, 5000), _sphere(g, 2, 5000, noise=2e-3), None, None)
	# the build at its capacity: 8 points per thread (kmax = (p + 1023) >> 10) and 128 tiles; the default route sends clouds of up to 8191
	# points here.  8192 on both sides: every tile full, all 128 rows of the tile table in use.
	c['capacity'] = (_sphere(g, 1, 8192), _sphere(g, 1, 8192, noise=2e-3), None, None)
	# every kmax from 2 to 8, tile counts 17, 33, 49, 65, 97, 113 and 128, different on the two sides of a pair
	per_thread = (1025, 2049, 3073, 4097, 6145, 7169, 8191)
	c['points per thread'] = (_sphere(g, 7, 8192), _sphere(g, 7, 8192, noise=2e-3), i32(*per_thread), i32(*reversed(per_thread)))
	c['lopsided'] = (_sphere(g, 1, 64), _sphere(g, 1, 8192), None, None)
	c['lopsided, reversed'] = (_sphere(g, 1, 8192), _sphere(g, 1, 64), None, None)
	return c


CASES = _cases()


@pytest.mark.parametrize('name', list(CASES))
def test_tile_path_equals_all_pairs_bit_for_bit(name):
	"""Keys and loss are equal to the bit; both gradients agree within the bound of a float sum in another order (the backward scatters
	with float atomics: 3e-5 of the largest entry, as test_chamfer_through_the_grid_equals_brute_force_bit_for_bit explains)."""
	from find_amd import _lib
	from find_amd import functional as FN
	x, y, xl, yl = (None if t is None else t.cuda() for t in CASES[name])
	kx0, ky0, l0, _ = _fwd(x, y, xl, yl, TILES)
	kx1, ky1, l1, _ = _fwd(x, y, xl, yl, BRUTE)
	assert torch.equal(kx0, kx1), (name, int((kx0 != kx1).sum()))
	assert torch.equal(ky0, ky1), (name, int((ky0 != ky1).sum()))
	assert torch.equal(l0, l1) and torch.isfinite(l0), (name, l0.item(), l1.item())
	out = []
	for bits in (TILES, BRUTE):
		_lib.set_tuning('raster_ablate', bits)
		try:
			xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
			loss, _ = FN.chamfer_distance(xg, yg, xl, yl)
			loss.backward()
			torch.cuda.synchronize()
			out.append((loss.detach().clone(), xg.grad.clone(), yg.grad.clone()))
		finally:
			_lib.set_tuning('raster_ablate', 0)
	(la, gxa, gya), (lb, gxb, gyb) = out
	assert torch.equal(la, lb) and torch.equal(la, l0)
	assert (gxa - gxb).abs().max().item() <= 3e-5 * max(gxb.abs().max().item(), 1e-12), name
	assert (gya - gyb).abs().max().item() <= 3e-5 * max(gyb.abs().max().item(), 1e-12), name


def test_ties_go_to_the_lowest_original_index():
	"""Tile order is not index order: a query that sits exactly on duplicated targets must still report the lowest of their indices."""
	x, y, _, _ = (None if t is None else t.cuda() for t in CASES['duplicates'])
	kx, _, _, _ = _fwd(x, y, None, None, TILES)
	idx = (kx & 0xffffffff).cpu()
	assert idx[:50].tolist() == list(range(50)) and int(idx[50]) == 3
	assert int((kx[:51] >> 32).abs().max()) == 0   # distance 0


def test_tile_path_is_the_same_from_run_to_run():
	"""The build's LDS atomics decide which points of a cut bin go left and the order inside a tile: the tiling differs between runs, the
	keys and the loss must not.  The gradients of the two key sets come from the unchanged backward kernel, whose float-atomic scatter adds
	a row's addends in any order: rows with at most two addends (own term + one scattered) are order-independent and must be identical,
	the others agree within the summation-order bound."""
	x, y = CASES['surface'][0].cuda(), CASES['surface'][1].cuda()
	kx0, ky0, l0, ws0 = _fwd(x, y, None, None, TILES)
	kx1, ky1, l1, ws1 = _fwd(x, y, None, None, TILES)
	assert torch.equal(kx0, kx1) and torch.equal(ky0, ky1) and torch.equal(l0, l1)
	dx0, dy0 = _bwd(x, y, None, None, ws0)
	dx1, dy1 = _bwd(x, y, None, None, ws1)
	n, p1, p2 = x.shape[0], x.shape[1], y.shape[1]
	for d0, d1, kother, p in ((dx0, dx1, ky0, p1), (dy0, dy1, kx0, p2)):
		hits = torch.zeros(n, p, dtype=torch.int64, device=x.device)
		hits.scatter_add_(1, (kother & 0xffffffff).view(n, -1), torch.ones(n, kother.numel() // n, dtype=torch.int64, device=x.device))
		few = (hits <= 1)[..., None].expand_as(d0)
		assert torch.equal(d0[few], d1[few])
		assert (d0 - d1).abs().max().item() <= 3e-5 * d0.abs().max().item()


def test_tile_path_replays_in_a_graph():
	"""One forward + backward at 2 x 600 captured in a HIP graph (no host synchronisation, no allocation in the path): three replays give
	the eager run's keys."""
	from find_amd import _lib
	from find_amd._lib import check, current_stream, ptr
	L = _lib.lib()
	g = torch.Generator().manual_seed(99)
	x, y = _sphere(g, 2, 600).cuda(), _sphere(g, 2, 600).cuda()
	n, p1, p2 = 2, 600, 600
	kx0, ky0, l0, _ = _fwd(x, y, None, None, TILES)
	ws = torch.zeros(L.find_chamfer_ws_bytes(n, p1, p2), dtype=torch.uint8, device=x.device)
	loss, one = torch.zeros((), device=x.device), torch.ones((), device=x.device)
	dx, dy = torch.zeros_like(x), torch.zeros_like(y)
	graph = torch.cuda.CUDAGraph()
	_lib.set_tuning('raster_ablate', TILES)
	try:
		torch.cuda.synchronize()
		with torch.cuda.graph(graph):
			s = current_stream(x.device)
			check(L.find_chamfer_fwd(ptr(x), None, ptr(y), None, n, p1, p2, ptr(loss), ptr(ws), ws.numel(), s), 'find_chamfer_fwd')
			check(L.find_chamfer_bwd(ptr(x), None, ptr(y), None, n, p1, p2, ptr(one), ptr(ws), ws.numel(), ptr(dx), ptr(dy), s), 'find_chamfer_bwd')
	finally:
		_lib.set_tuning('raster_ablate', 0)
	for _ in range(3):
		ws.zero_()
		graph.replay()
		torch.cuda.synchronize()
		kx, ky = _keys(ws, n, p1, p2)
		assert torch.equal(kx, kx0) and torch.equal(ky, ky0) and torch.equal(loss, l0)
	assert torch.isfinite(dx).all() and float(dx.abs().max()) > 0
