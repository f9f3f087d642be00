"""The closest points between query triangles held in PyTorch device tensors and the triangles of a scene, and the contact test (no reference
counterpart; include/tirt.h, "Triangle distance": the definition, bit for bit; csrc/tirt_triangle_query.hip: the walk over the scene's 4-wide nodes).

    q = TriangleQuery(scene, stack_size=64, flags=0)      # scene after setup_data_gpu() (Example.build_scene)
    h = q.closest(triangles, max_distance=None, points=False)      # TriangleClosest(d2 [n] f32, prim [n] i32, code [n] i32, point_query, point_scene [n, 3] or None)
    m = q.collides(triangles)                             # [n] bool: closest(triangles, max_distance=0.0).prim >= 0
    h, counts = q.closest_counts(triangles, max_distance=None)      # counts [n, 2] int32: N_box, N_leaf of a COUNT_NODES walk
    p = q.pairs(triangles, max_distance=0.0, points=False, capacity=None, ordered=True)      # TrianglePairs(row_start [n + 1] i64, prim, d2, code, point_query, point_scene): CSR rows; p.query() = the query index per pair
    c = q.count_within(triangles, max_distance)           # [n] int32: the scene triangles within max_distance of each query triangle

``triangles`` is a float32 tensor ``[n, 3, 3]`` (triangle, vertex, xyz) on the scene context's device whose last two dimensions are contiguous (strides
``(s, 3, 1)`` with any ``s >= 9``: a slice of a wider buffer is handed over without a copy; any other layout is copied once), or a pair
``(vertices [m, 3] float32, faces [n, 3] integer)`` that is gathered in torch.  ``max_distance``: None (no bound), a float for every query, or an ``[n]``
float32 tensor on the same device (any positive stride); a negative or NaN bound finds nothing.  The unit of the query is a triangle: the distance between
two triangles is attained vertex-to-face or edge-to-edge, and crossing triangles have an edge of one through the other -- ``code`` says which of the 21
candidates of the definition answered (0..2 a query vertex, 3..5 a scene vertex, 6..14 edge against edge, 15..17 a query edge through the scene triangle,
18..20 a scene edge through the query triangle).  Nothing found: ``prim = -1``, ``d2 = inf``, ``code = -1``, both points 0.  Analytic spheres, spot and laser
shapes take no part; alpha cut-outs are ignored.  The outputs come from ``torch.empty`` and the work is queued on ``torch.cuda.current_stream(device)``:
nothing waits for it on the host.  A query triangle deep inside a dense part of the scene tests every leaf whose box meets its box (ties at distance 0
go to the smallest primitive id, so the walk cannot stop at the first contact).
"""
import collections

from . import _native
from .PointQuery import PointQuery, _Pairs, _pairs_front

TriangleClosest = collections.namedtuple("TriangleClosest", ["d2", "prim", "code", "point_query", "point_scene"])


class TrianglePairs(_Pairs, collections.namedtuple("TrianglePairs", ["row_start", "prim", "d2", "code", "point_query", "point_scene"])):
    __slots__ = ()


class TriangleQuery:
    def __init__(self, scene, stack_size=64, flags=0):
        try:
            self._point = PointQuery(scene, stack_size, flags)      # its checks of stack_size and flags, its device rule and its bound check
        except ValueError as exc:
            raise ValueError(str(exc).replace("PointQuery", "TriangleQuery")) from None
        self.torch = self._point.torch
        self.scene, self.stack_size, self.flags = scene, self._point.stack_size, self._point.flags

    def _check_triangles(self, triangles, what):
        """(device, n, row stride in floats, the tensor that is handed over: it has to outlive the call that queues the work)"""
        torch = self.torch
        if isinstance(triangles, (tuple, list)):
            if len(triangles) != 2 or not all(isinstance(x, torch.Tensor) for x in triangles):
                raise TypeError("TriangleQuery.%s: triangles must be a tensor [n, 3, 3] or a pair (vertices [m, 3], faces [n, 3]) of tensors" % what)
            vertices, faces = triangles
            if vertices.dtype != torch.float32:
                raise TypeError("TriangleQuery.%s: vertices must be float32, got %s" % (what, vertices.dtype))
            if faces.dtype not in (torch.int32, torch.int64):
                raise TypeError("TriangleQuery.%s: faces must be int32 or int64, got %s" % (what, faces.dtype))
            if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
                raise ValueError("TriangleQuery.%s: vertices must be [m, 3] and faces [n, 3], got %s and %s" % (what, tuple(vertices.shape), tuple(faces.shape)))
            if vertices.device != faces.device:
                raise ValueError("TriangleQuery.%s: vertices are on %s, faces on %s" % (what, vertices.device, faces.device))
            if vertices.device.type != "cuda":
                raise TypeError("TriangleQuery.%s: vertices must be on the GPU, got a %s tensor" % (what, vertices.device.type))
            triangles = vertices[faces.long()]               # [n, 3, 3], contiguous (an index out of range is torch's error)
        if not isinstance(triangles, torch.Tensor):
            raise TypeError("TriangleQuery.%s: triangles must be a torch.Tensor, got %s" % (what, type(triangles).__name__))
        if triangles.dtype != torch.float32:
            raise TypeError("TriangleQuery.%s: triangles must be float32, got %s" % (what, triangles.dtype))
        if triangles.dim() != 3 or tuple(triangles.shape[1:]) != (3, 3):
            raise ValueError("TriangleQuery.%s: triangles must be [n, 3, 3], got shape %s" % (what, tuple(triangles.shape)))
        if triangles.device.type != "cuda":
            raise TypeError("TriangleQuery.%s: triangles must be on the GPU, got a %s tensor" % (what, triangles.device.type))
        dev = self._point._device()
        if triangles.device != dev:
            raise ValueError("TriangleQuery.%s: triangles are on %s, the scene's context on %s" % (what, triangles.device, dev))
        n = triangles.shape[0]
        if n and (triangles.stride(1) != 3 or triangles.stride(2) != 1 or (n > 1 and triangles.stride(0) < 9)):
            triangles = triangles.contiguous()
        return dev, n, (triangles.stride(0) if n > 1 else 9), triangles

    def _run(self, triangles, max_distance, points, flags, counts, what):
        torch = self.torch
        dev, n, stride, tris = self._check_triangles(triangles, what)
        dptr, dstride, dall = self._check_bound(max_distance, dev, n, what)
        d2 = torch.empty(n, dtype=torch.float32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        code = torch.empty(n, dtype=torch.int32, device=dev)
        pq = torch.empty((n, 2, 3), dtype=torch.float32, device=dev) if points else None
        cnt = torch.empty((n, 2), dtype=torch.int32, device=dev) if counts else None
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            self.scene.ctx.query_mesh_distance(tris.data_ptr(), n, stride, self.stack_size, flags, dmax=dptr, dmax_stride=dstride, dmax_all=dall,
                                               out_d2=d2.data_ptr(), out_prim=prim.data_ptr(), out_code=code.data_ptr(),
                                               out_points=pq.data_ptr() if points else 0, counts=cnt.data_ptr() if counts else 0, stream=stream)
            # (a gathered or copied input was allocated on this stream, and the stream is ordered after the walk: the allocator can only reuse it afterwards)
        return TriangleClosest(d2, prim, code, pq[:, 0] if points else None, pq[:, 1] if points else None), cnt

    def _check_bound(self, max_distance, dev, n, what):
        try:
            return self._point._check_bound(max_distance, dev, n, what)
        except (TypeError, ValueError) as exc:
            raise type(exc)(str(exc).replace("PointQuery", "TriangleQuery").replace("the points on", "the triangles on")) from None

    def closest(self, triangles, max_distance=None, points=False):
        """The closest pair of points between every query triangle and the scene's triangles, bit for bit Context.mesh_distance's: d2 (inf where nothing
        is found), prim (-1), code (-1) and, with points=True, the point on the query triangle and the point on the scene.  Asynchronous on the current stream."""
        return self._run(triangles, max_distance, points, self.flags, False, "closest")[0]

    def collides(self, triangles):
        """[n] bool: the query triangle touches or crosses some scene triangle by the definition's arithmetic -- closest(triangles, max_distance=0.0).prim >= 0"""
        return self.closest(triangles, max_distance=0.0).prim >= 0

    def pairs(self, triangles, max_distance=0.0, points=False, capacity=None, ordered=True):
        """EVERY scene triangle within max_distance of every query triangle -- with the default 0.0 the contact pair list: all that touch or cross it --
        as CSR rows (include/tirt.h, "Triangle pairs"): TrianglePairs(row_start [n + 1] int64, prim [total] i32, d2 [total] f32, code [total] i32,
        point_query, point_scene [total, 3] or None).  Row i is the slice row_start[i] : row_start[i + 1]; inside a row d2 ascends and ties go to the
        smaller primitive id, so its element 0 is closest()'s answer and a row is non-empty at 0.0 exactly where collides() is true; ordered=False skips
        that pass.  capacity=None sizes the result exactly: a counting call, ONE HOST WAIT to read the total, then the filling call.  capacity=c runs
        both in one call with no host wait: only the rows that fit entirely (row_start[i + 1] <= c) are written, row_start is complete, and
        row_start[-1] > c says the result was cut."""
        return _pairs_front(self, "pairs", True, triangles, max_distance, points, capacity, ordered)

    def count_within(self, triangles, max_distance):
        """[n] int32: how many scene triangles lie within max_distance (a float or an [n] float32 tensor; required) of every query triangle: the lengths
        of pairs()'s rows, from the counting call alone.  Asynchronous on the current stream."""
        if max_distance is None:
            raise TypeError("TriangleQuery.count_within: max_distance is required (without a bound every triangle counts)")
        row_start = _pairs_front(self, "count_within", True, triangles, max_distance, False, None, True, count_only=True)
        return (row_start[1:] - row_start[:-1]).to(self.torch.int32)

    def closest_counts(self, triangles, max_distance=None):
        """closest() with the per-query N_box / N_leaf counts ([n, 2] int32) of a COUNT_NODES walk: (TriangleClosest, counts)"""
        return self._run(triangles, max_distance, False, self.flags | _native.COUNT_NODES, True, "closest_counts")
