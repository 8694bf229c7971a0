"""The as-rigid-as-possible energy on the HIP path: the autograd binding of find_arap_fwd / find_arap_bwd (csrc/arap.hip).  The public names
are functional.ArapRest (the rest mesh: topology, weights, W) and functional.arap_energy, which calls in here; losses.ARAPLoss is the mean
over the batch.  There is no CPU or eager fallback: CPU tensors raise.  The workspace comes from functional._ws; the rotations, outputs and
the gradient are torch.empty / torch.empty_like, which the kernels write in full (tests/test_gpu_arap.py runs them over poisoned memory)."""
import torch

from . import _lib
from . import functional as FN
from ._lib import check, current_stream, ptr


class _Arap(torch.autograd.Function):
	@staticmethod
	def forward(ctx, verts, rest):
		FN._require_gpu(verts)
		L = _lib.lib()
		if verts.dim() != 3 or verts.shape[1] != rest.n_verts or verts.shape[2] != 3:
			raise RuntimeError(f'find_amd.arap: verts (N, {rest.n_verts}, 3) expected -- the rest mesh has {rest.n_verts} vertices --, got {tuple(verts.shape)}')
		if verts.device != rest.rest.device:
			raise RuntimeError(f'find_amd.arap: verts on {verts.device}, the rest mesh on {rest.rest.device}')
		verts = verts.detach().contiguous()
		N, V, _ = verts.shape
		dev, topo = verts.device, rest.topo
		ws = FN._ws(L.find_arap_ws_bytes(N, V), dev)
		R = torch.empty(N, V, 3, 3, device=dev, dtype=torch.float64)   # this node's own: the backward reads it, nothing else writes it
		cell = torch.empty(N, V, device=dev, dtype=torch.float32)
		energy = torch.empty(N, device=dev, dtype=torch.float32)
		degenerate = torch.empty(N, device=dev, dtype=torch.int32)
		check(L.find_arap_fwd(ptr(verts), ptr(rest.rest), ptr(topo.nbr_off), ptr(topo.nbr_idx), ptr(rest.nbr_w), N, V, rest.n_nbr, rest.W, ptr(R), ptr(cell),
							  ptr(energy), ptr(degenerate), ptr(ws), ws.numel(), current_stream(dev)), 'find_arap_fwd')
		ctx.rest = rest
		ctx.save_for_backward(verts, R)
		ctx.mark_non_differentiable(cell, R, degenerate)
		return energy, cell, R, degenerate

	@staticmethod
	def backward(ctx, g, *_):
		L = _lib.lib()
		verts, R = ctx.saved_tensors
		rest, topo = ctx.rest, ctx.rest.topo
		N, V, _ = verts.shape
		d = torch.empty_like(verts)
		g = g.contiguous()
		check(L.find_arap_bwd(ptr(verts), ptr(rest.rest), ptr(topo.nbr_off), ptr(topo.nbr_idx), ptr(rest.nbr_w), N, V, rest.n_nbr, rest.W, ptr(R), ptr(g),
							  ptr(d), current_stream(verts.device)), 'find_arap_bwd')
		return d, None


def arap_energy(verts, rest, return_per_vertex=False, return_rotations=False):
	"""functional.arap_energy (documented there).  The rotations the backward reads stay in double with the autograd node; a caller who asks
	for them gets an fp32 copy."""
	energy, cell, R, degenerate = _Arap.apply(verts, rest)
	out = (energy,)
	if return_per_vertex:
		out += (cell,)
	if return_rotations:
		out += ((R.float(), degenerate),)
	return out[0] if len(out) == 1 else out
