"""functional.sample_points with given draws that name a -1 row of a ragged batch's padded faces, or a face with a vertex index past the
mesh: the corner adds nothing, forward and backward, and nothing is read or written through it.  (The forward used to read the three floats in front of the mesh's vertices -- zeros in
fresh memory, anything in a re-used block: eval_3d_metrics on a ragged batch then depended on what ran before it.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_a_padding_face_adds_nothing_and_reads_nothing():
	from find_amd import functional as FN
	g = torch.Generator().manual_seed(0)
	N, V, F, S = 2, 7, 5, 64
	# the vertices of both meshes sit behind a block of NaN: what an out-of-range read of mesh 0 would meet
	block = torch.full((N + 1, V, 3), float('nan'), device='cuda')
	block[1:] = torch.rand(N, V, 3, generator=g).cuda()
	block.requires_grad_()
	verts = block[1:]
	assert verts.is_contiguous()
	faces = torch.randint(0, V, (N, F, 3), generator=g).cuda()
	faces[0, 3:] = -1                      # mesh 0 has three faces, two rows of padding
	faces[1, 4, 1] = V                     # and mesh 1 one index past its vertices
	face_idx = torch.randint(0, F, (N, S), generator=g, dtype=torch.int32).cuda()
	face_idx[0, :2] = torch.tensor([3, 4], dtype=torch.int32)
	face_idx[1, 0] = 4
	uv = torch.rand(N, S, 2, generator=g).cuda()
	attr = torch.rand(N, V, 3, generator=g).cuda()
	pts, cols = FN.sample_points(verts, faces, face_idx, uv, attr)
	su = uv[..., 0].double().sqrt()
	w = torch.stack([1 - su, su * (1 - uv[..., 1].double()), su * uv[..., 1].double()], -1)   # (N, S, 3)
	corners = torch.stack([faces[n][face_idx[n].long()] for n in range(N)])                    # (N, S, 3)
	ok = (corners >= 0) & (corners < V)
	for got, src in ((pts.detach(), verts.detach()), (cols, attr)):
		v = torch.stack([src[n].double()[corners[n].clamp(0, V - 1)] for n in range(N)])       # (N, S, 3 corners, 3)
		want = (w[..., None] * v * ok[..., None]).sum(2)
		assert torch.isfinite(got).all()
		assert (got.double() - want).abs().max().item() < 1e-6
	assert (pts[0, :2] == 0).all() and (cols[0, :2] == 0).all() and not ok[1, 0].all()
	# backward: d_verts[n, corner] += w * g for the corners that exist; the index V of the last mesh would land behind the gradient's end
	gout = torch.rand(N, S, 3, generator=g).cuda()
	(pts * gout).sum().backward()
	torch.cuda.synchronize()
	want = torch.zeros(N, V, 3, dtype=torch.float64, device='cuda')
	for n in range(N):
		for c in range(3):
			keep = ok[n, :, c]
			want[n].index_add_(0, corners[n, keep, c], w[n, keep, c, None] * gout[n, keep].double())
	assert torch.isfinite(block.grad).all() and not block.grad[0].any()
	assert (block.grad[1:].double() - want).abs().max().item() < 1e-5
