"""Baking the colour field into UV textures: the writing half of structures.TexturesUV (not in the reference, which only ever reads scan
textures).  The texture loss trains the colour head as a continuous field; everything else the library shows evaluates it at the template's
vertices and interpolates.  Here an atlas is rastered into texels once (find_uv_raster: which face owns a texel's centre, and its
barycentrics there), the field is evaluated at each covered texel's surface point, the chart borders are padded from the nearest covered
texel (find_uv_dilate_map) so that functional_render.uv_sample's bilinear reads near a border mix in no background, and the maps come back
as a TexturesUV that FootRenderer, vis.turntable and export_textured_obj take.

Texel (i, j) of an H x W map has its centre at (u, v) = (j / (W - 1), 1 - i / (H - 1)), row 0 the top of the image: uv_sample's convention
(grid_sample with align_corners=True on the vertically flipped map).  An output path: nothing here carries a gradient.  GPU only."""
import os

import numpy as np
import torch

from . import _lib
from . import functional as FN
from ._lib import check, current_stream, ptr
from .functional import _c, _faces_i32, _require_gpu
from .rays import _accel_keyword
from .structures import TexturesUV


def _size(size):
	if isinstance(size, (tuple, list)):
		return int(size[0]), int(size[1])
	return int(size), int(size)


def uv_raster(verts_uvs, faces_uvs, size):
	"""verts_uvs (Vt,2), faces_uvs (F,3), size an int or (H, W)  ->  (face (H,W) int32, bary (H,W,3)): per texel the smallest face whose
	closed UV triangle holds the texel's centre (-1: none) and the centre's barycentrics in it (0 where none).  Faces with an index outside
	[0, Vt) or of zero / NaN area cover nothing; UVs outside [0, 1] are legal and do not wrap.  Bit-identical from call to call."""
	_require_gpu(verts_uvs, faces_uvs)
	if verts_uvs.dim() != 2 or verts_uvs.shape[-1] != 2 or faces_uvs.dim() != 2 or faces_uvs.shape[-1] != 3:
		raise ValueError(f'find_amd.bake.uv_raster: verts_uvs (Vt,2) and faces_uvs (F,3) expected, got {tuple(verts_uvs.shape)} / {tuple(faces_uvs.shape)}')
	H, W = _size(size)
	vu, fu = _c(verts_uvs.detach()), _faces_i32(faces_uvs)
	face = torch.empty(H, W, device=vu.device, dtype=torch.int32)
	bary = torch.empty(H, W, 3, device=vu.device, dtype=torch.float32)
	check(_lib.lib().find_uv_raster(ptr(vu), vu.shape[0], ptr(fu), fu.shape[0], H, W, ptr(face), ptr(bary), current_stream(vu.device)), 'find_uv_raster')
	return face, bary


def dilate_map(face, pad):
	"""face (H,W) int32 of uv_raster  ->  src (H,W) int32: the flat index i * W + j of the texel each texel takes its value from -- a
	covered one itself, an uncovered one the covered texel within Chebyshev distance `pad` (0 .. 16) that is nearest in di^2 + dj^2 (ties:
	the smallest flat index), -1 without one."""
	_require_gpu(face)
	if face.dim() != 2 or face.dtype != torch.int32:
		raise ValueError(f'find_amd.bake.dilate_map: face (H,W) int32 expected, got {tuple(face.shape)} {face.dtype}')
	face = _c(face)
	src = torch.empty_like(face)
	check(_lib.lib().find_uv_dilate_map(ptr(face), face.shape[0], face.shape[1], int(pad), ptr(src), current_stream(face.device)), 'find_uv_dilate_map')
	return src


class BakePlan:
	"""What an atlas and a map size decide, made once (plan) and used for every bake:
	face (H,W) int32, bary (H,W,3)   uv_raster's;
	idx (T,) int64                   flat indices of the covered texels, row-major;
	lookup (H*W,) int64              per texel the compact index in [0, T) of the texel it copies (a covered one its own), or T: fill;
	verts_uvs (Vt,2), faces_uvs (F,3), pad   the atlas and the gutter it was made with."""

	def __init__(self, face, bary, idx, lookup, verts_uvs, faces_uvs, pad):
		self.face, self.bary, self.idx, self.lookup, self.verts_uvs, self.faces_uvs, self.pad = face, bary, idx, lookup, verts_uvs, faces_uvs, pad
		self._face_idx = face.reshape(-1)[idx].long()   # the owning face and the barycentrics of the covered texels
		self._bary_idx = bary.reshape(-1, 3)[idx]

	@property
	def size(self):
		return tuple(self.face.shape)

	def points(self, verts, faces):
		"""The covered texels' surface points (N|1, T, 3) on verts (N|1,V,3) with the mesh's faces (F,3) (or (1,F,3)), face for face the
		atlas's faces_uvs: sum_k bary_k * verts[:, faces[face[idx], k]]."""
		if faces.dim() == 3:
			faces = faces[0]
		corners = faces.long()[self._face_idx]   # (T, 3)
		b = self._bary_idx
		return sum(b[None, :, k, None] * verts[:, corners[:, k]] for k in range(3))

	def assemble(self, cols, fill=1.0):
		"""cols (N,T,C), the values of the covered texels  ->  maps (N,H,W,C); texels with no covered texel within the gutter get `fill`
		(the renderer's white background)."""
		H, W = self.size
		N, T, C = cols.shape
		if T != self.idx.numel():
			raise ValueError(f'find_amd.bake.BakePlan.assemble: cols (N,{self.idx.numel()},C) expected, got {tuple(cols.shape)}')
		table = torch.cat([cols, cols.new_full((N, 1, C), fill)], dim=1)
		return table.index_select(1, self.lookup).reshape(N, H, W, C)


def plan(verts_uvs, faces_uvs, size, pad=4):
	"""The BakePlan of an atlas (verts_uvs (Vt,2), faces_uvs (F,3), on the GPU) at a map size (int or (H, W)) with a gutter of `pad` texels.
	Depends on the atlas alone: make it once.  (It reads the number of covered texels back: one host synchronisation.)"""
	face, bary = uv_raster(verts_uvs, faces_uvs, size)
	src = dilate_map(face, pad).reshape(-1).long()
	covered = face.reshape(-1) >= 0
	idx = covered.nonzero().flatten()
	T = idx.numel()
	compact = torch.cumsum(covered, 0) - 1   # the compact index of a covered texel
	lookup = torch.where(src >= 0, compact[src.clamp(min=0)], torch.full_like(src, T))
	return BakePlan(face, bary, idx, lookup, verts_uvs.detach(), faces_uvs, int(pad))


def bake(field, plan, verts, faces, texels_per_call=65536, fill=1.0):
	"""Maps (N,H,W,C) of `field`, any callable (n,P,3) -> (n|N,P,C), evaluated under no_grad at the surface points of the plan's covered
	texels on verts (N|1,V,3) / faces (F,3), `texels_per_call` of them at a time; the gutter and the rest of the map as BakePlan.assemble."""
	if texels_per_call < 1:
		raise ValueError(f'find_amd.bake.bake: texels_per_call >= 1 expected, got {texels_per_call}')
	T = plan.idx.numel()
	if T == 0:
		raise ValueError('find_amd.bake.bake: the atlas covers no texel of the map')
	with torch.no_grad():
		pts = plan.points(verts, faces)
		cols = None
		for a in range(0, T, texels_per_call):
			c = field(pts[:, a:a + texels_per_call].contiguous())
			if cols is None:
				cols = torch.empty(c.shape[0], T, c.shape[-1], device=c.device, dtype=c.dtype)
			cols[:, a:a + c.shape[1]] = c
		return plan.assemble(cols, fill)


def bake_colours(model, plan, shapevec=None, texvec=None, posevec=None, texels_per_call=65536, fill=1.0, verts_uvs=None, faces_uvs=None):
	"""The colour head of a NeuralDisplacementField as TexturesUV, a map per row of the codes: model(pos, ..., want=('col',))['col'] at
	the template positions of the covered texels -- on model.template_verts (centred, what the field is trained on) with
	model.template_faces, whose faces the atlas's faces_uvs follow one for one.  The batch-1 positions share the trunk across the feet.
	verts_uvs / faces_uvs: the atlas to hand back, the plan's own by default."""
	def field(pos):
		return model(pos, shapevec=shapevec, texvec=texvec, posevec=posevec, want=('col',))['col'][..., :3]
	maps = bake(field, plan, model.template_verts.data, model.template_faces.data[0], texels_per_call=texels_per_call, fill=fill)
	vu = plan.verts_uvs if verts_uvs is None else verts_uvs
	fu = plan.faces_uvs if faces_uvs is None else faces_uvs
	N = maps.shape[0]
	return TexturesUV(maps, fu.to(maps.device)[None].expand(N, -1, -1), vu.to(maps.device)[None].expand(N, -1, -1))


def texel_normals(plan, verts, faces):
	"""The covered texels' shading normals (N, T, 3): the barycentric blend of functional.vertex_normals at the texel's face, as
	BakePlan.points blends the positions (not renormalised; rays.ambient_occlusion normalises what it is given)."""
	vn = FN.vertex_normals(verts, faces)
	if faces.dim() == 3:
		faces = faces[0]
	corners = faces.long()[plan._face_idx]
	b = plan._bary_idx
	return sum(b[None, :, k, None] * vn[:, corners[:, k]] for k in range(3))


@_accel_keyword
def bake_ambient_occlusion(plan, verts, faces, n_dirs=64, max_dist=None, fill=1.0):
	"""An ambient-occlusion map per mesh, (N, H, W, 1) in [0, 1] (1 = open sky): rays.ambient_occlusion at the covered texels' surface points
	(plan.points) about texel_normals, each texel's rays never hitting the face that owns it (skip); the gutter and the rest of the map as
	BakePlan.assemble.  verts (N, V, 3), faces (F, 3) (or (1, F, 3)), face for face the atlas's faces_uvs.  Multiply a baked colour map by
	it to shade: maps * ao.  Keyword accel (added by rays._accel_keyword): None, 'bvh' or a rays.MeshBVH of (verts, faces (F, 3)), as in
	rays.ray_mesh_intersect: the same bits, found through a bounding-volume hierarchy instead of against every face.  No gradient."""
	from . import rays
	if plan.idx.numel() == 0:
		raise ValueError('find_amd.bake.bake_ambient_occlusion: the atlas covers no texel of the map')
	with torch.no_grad():
		f = faces[0] if faces.dim() == 3 else faces
		pts = plan.points(verts, f).contiguous()
		N = pts.shape[0]
		skip = plan._face_idx.to(torch.int32)[None].expand(N, -1)
		ao = rays.ambient_occlusion(pts, texel_normals(plan, verts, f).contiguous(), verts, f, n_dirs=n_dirs, max_dist=max_dist, skip=skip)
		return plan.assemble(ao[..., None], fill)


def textured_meshes(model, plan, verts_uvs, faces_uvs, batch, is_train=False):
	"""model.get_meshes_from_batch(batch, is_train)['meshes'] with the baked TexturesUV in place of the vertex colours (which are not
	evaluated).  FootRenderer and vis.turntable take the result; no gradient."""
	sfx = 'train' if is_train else 'val'
	with torch.no_grad():
		meshes = model.get_meshes_from_batch(batch, is_train=is_train, lazy_colours=True)['meshes']
		tex = bake_colours(model, plan, shapevec=batch.get(f'shapevec_{sfx}', None), texvec=batch.get(f'texvec_{sfx}', None),
						   posevec=batch.get(f'posevec_{sfx}', None), verts_uvs=verts_uvs, faces_uvs=faces_uvs)
	meshes = meshes.update_padded(meshes.verts_padded().detach())
	meshes.textures = tex
	return meshes


def _map_u8(img):
	"""(255 * x) truncated, clamped to [0, 255], NaN -> 0: functional.frames_u8 on the GPU, the same in numpy for a CPU map."""
	if img.is_cuda:
		return FN.frames_u8(img.detach().float()[None], rot180=False)[0].cpu().numpy()
	x = img.detach().numpy().astype(np.float32)
	with np.errstate(invalid='ignore'):
		return np.where(np.isnan(x), np.float32(0), np.clip(np.float32(255) * x, 0, 255)).astype(np.uint8)


def export_textured_obj(mesh, loc, idx=0):
	"""Mesh `idx` of a TexturesUV mesh as three files any viewer opens: `loc` (mtllib, usemtl material_0, `v`, `vt`, `f a/ta b/tb c/tc`,
	1-based, every float %.9g as vis.export_obj: float32 reads back bit for bit; a face with a -1 UV corner is written `f a b c`),
	<stem>.mtl (newmtl material_0, map_Kd <stem>.png) and <stem>.png, the map as bytes ((255 * x) truncated).  dataset.load_obj and
	dataset.load_texture_png read them back.  Returns [loc, mtl, png]."""
	from PIL import Image
	tex = mesh.textures
	if not isinstance(tex, TexturesUV):
		raise ValueError(f'find_amd.bake.export_textured_obj: a mesh with TexturesUV expected, got {type(tex).__name__}')
	stem = os.path.splitext(loc)[0]
	name = os.path.basename(stem)
	n = mesh._num_verts[idx]
	verts = mesh.verts_padded()[idx, :n].detach().cpu().numpy().astype(np.float32)
	faces = mesh.faces_list()[idx].detach().cpu().numpy().astype(np.int64)
	uvs = tex.verts_uvs_padded()[idx].detach().cpu().numpy().astype(np.float32)
	fuv = tex.faces_uvs_padded()[idx].detach().cpu().numpy().astype(np.int64)[:faces.shape[0]]
	if fuv.shape[0] != faces.shape[0]:
		raise ValueError(f'find_amd.bake.export_textured_obj: {faces.shape[0]} faces but {fuv.shape[0]} rows of faces_uvs')
	lines = [f'mtllib {name}.mtl', 'usemtl material_0']
	lines += ['v ' + ' '.join('%.9g' % x for x in row) for row in verts.tolist()]
	lines += ['vt ' + ' '.join('%.9g' % x for x in row) for row in uvs.tolist()]
	for f, t in zip((faces + 1).tolist(), (fuv + 1).tolist()):
		lines.append('f %d %d %d' % tuple(f) if min(t) < 1 else 'f %d/%d %d/%d %d/%d' % (f[0], t[0], f[1], t[1], f[2], t[2]))
	with open(loc, 'w') as fh:
		fh.write('\n'.join(lines) + '\n')
	with open(stem + '.mtl', 'w') as fh:
		fh.write(f'newmtl material_0\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nmap_Kd {name}.png\n')
	Image.fromarray(_map_u8(tex.maps_padded()[idx])).save(stem + '.png')
	return [loc, stem + '.mtl', stem + '.png']
