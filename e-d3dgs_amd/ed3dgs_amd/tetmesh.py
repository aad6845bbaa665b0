"""Marching tetrahedra on the GPU through the C ABI (csrc/tetmesh.hip): utils/tetmesh.py's `marching_tetrahedra` with the
same signature, batch convention and return structure.

marching_tetrahedra(vertices [B,N,3], tets [T,4] int32/int64, sdf [B,N], scales [B,N] or [B,N,1]) returns
list(zip(*per_batch)), per batch entry ((endpoints [E,2,3], endpoint sdf [E,2,1]), endpoint scales [E,2,1],
faces [F,3] int64, edge ids [E,2] int64), equal to the reference's arrays bit for bit up to 32 Mi tets.  Above that the
reference emits faces chunk by chunk; here the order stays unchunked (same vertices, same triangles, another face order).
Two host synchronisations per batch entry: the crossing-edge count sizes the edge sort, the vertex count the outputs."""
import ctypes as C

import torch

from . import _lib


class _Buf:
    def __init__(self, device):
        self.device, self.t = device, None

    def _alloc(self, _user, nbytes):
        self.t = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self.t.data_ptr()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


@torch.no_grad()
def _unbatched(vertices, tets, sdf, scales):
    dev = vertices.device
    L = _lib.lib()
    N, T = sdf.shape[0], tets.shape[0]
    v = vertices.detach().float().contiguous()
    s = sdf.detach().float().contiguous().reshape(-1)
    sc = scales.detach().float().contiguous().reshape(-1)
    if v.shape != (N, 3) or sc.shape[0] != N:
        raise ValueError("marching_tetrahedra: vertices [N,3], sdf [N] and scales [N(,1)] must agree")
    t = tets.detach().contiguous() if tets.dtype in (torch.int32, torch.int64) else tets.detach().long().contiguous()
    is64 = t.dtype == torch.int64
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    tb = L.ed3dgs_tetmesh_tet_bytes(C.c_int(T))
    tet_ws = torch.empty(tb, dtype=torch.uint8, device=dev)
    edge = _Buf(dev)
    cb = _lib.ALLOC_FN(edge._alloc)
    counts = (C.c_longlong * 4)()
    rc = L.ed3dgs_tetmesh_count(C.c_int(N), C.c_int(T), _ptr(t), C.c_int(int(is64)), _ptr(s), _ptr(tet_ws), C.c_size_t(tb),
                                cb, None, counts, stream)
    if rc < 0:
        raise RuntimeError(_lib.last_error())
    E, n1, n2, S = (int(x) for x in counts)
    f32 = dict(dtype=torch.float32, device=dev)
    ends = torch.empty((E, 2, 3), **f32)
    end_sdf = torch.empty((E, 2, 1), **f32)
    end_scales = torch.empty((E, 2, 1), **f32)
    faces = torch.empty((n1 + 2 * n2, 3), dtype=torch.int64, device=dev)
    ids = torch.empty((E, 2), dtype=torch.int64, device=dev)
    if S > 0:
        rc = L.ed3dgs_tetmesh_emit(C.c_int(N), C.c_int(T), _ptr(t), C.c_int(int(is64)), _ptr(v), _ptr(s), _ptr(sc), _ptr(tet_ws),
                                   _ptr(edge.t), counts, _ptr(ends), _ptr(end_sdf), _ptr(end_scales), _ptr(faces), _ptr(ids),
                                   stream)
        if rc < 0:
            raise RuntimeError(_lib.last_error())
    return (ends, end_sdf), end_scales, faces, ids


def marching_tetrahedra(vertices, tets, sdf, scales):
    if not (vertices.is_cuda and tets.is_cuda and sdf.is_cuda and scales.is_cuda):
        raise RuntimeError("marching_tetrahedra: inputs must be GPU tensors (the MI355X path has no CPU fallback)")
    return list(zip(*[_unbatched(vertices[b], tets, sdf[b], scales[b]) for b in range(vertices.shape[0])]))
