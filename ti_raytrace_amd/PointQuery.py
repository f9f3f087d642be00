"""The nearest surface point of a scene to query points held in PyTorch device tensors (no reference counterpart; include/tirt.h,
"Closest point": the definition, bit for bit; csrc/tirt_closest_point.hip: the walk over the scene's 4-wide nodes).

    q = PointQuery(scene, stack_size=64, flags=0)         # scene after setup_data_gpu() (Example.build_scene)
    h = q.closest(points, max_distance=None, attributes=False)      # PointHits(dist2 [N] f32, prim [N] i32, point [N, 3] or None, uv [N, 2] or None)
    s = q.signed_distance(points, max_distance=None, attributes=False)      # SignedHits(dist [N] f32, prim, point, uv): dist < 0 inside
    m = q.inside(points, method="pseudonormal")           # [N] bool; method="winding": winding_number(points) > 0.5
    wn = q.winding_number(points, beta=2.0)               # [N] f32: the generalized winding number (1 inside, 0 outside, in between near holes)
    nn = q.nearest(points, k, max_distance=None, attributes=False, count=False)      # PointNearest(dist2 [N, k], prim [N, k], point, uv, count [N] or None)
    c = q.count_within(points, max_distance)              # [N] int32: the primitives within max_distance of each point
    w = q.within(points, max_distance, attributes=False, capacity=None, ordered=True)      # PointPairs(row_start [N + 1] i64, prim, dist2, point, uv): CSR rows; w.query() = the query index per pair
    r = q.mesh_report()                                   # {"boundary_edges", "nonmanifold_edges", "flipped_edges", "invalid_triangles", "primitives", "closed"}

``points`` is a float32 tensor ``[N, C >= 3]`` on the scene context's device with ``stride(1) == 1`` and any row stride (an ``[N, 8]``
tensor's ``[:, :3]`` view works).  ``max_distance``: None (no bound), a float for every query, or an ``[N]`` float32 tensor on the same
device (any positive stride); a negative or NaN bound finds nothing.  Nothing found: ``prim = -1``, ``dist2 = inf``, point and uv 0.
``uv`` is the hit record's convention (``point = a + u (b - a) + v (c - a)``).  The outputs come from ``torch.empty`` and the work is
queued on ``torch.cuda.current_stream(device)``: nothing waits for it on the host.

``nearest`` returns the ``k`` (0 .. 64) nearest primitives of every query in order -- ``dist2`` ascending, at equal bits the smaller primitive id first;
column 0 is ``closest``'s answer bit for bit -- padded with ``(inf, -1, 0, 0)`` where fewer than ``k`` lie within the bound, and with ``count=True`` the number
of ALL primitives within the bound, which may exceed ``k`` (include/tirt.h, "K nearest primitives").  With the count the walk cannot cull by the k-th distance:
give a bound with it.  ``count_within`` is the count alone.

``signed_distance`` is ``closest`` with the sign of the angle-weighted pseudo-normal of the closest face, edge or vertex (include/tirt.h, "Signed
distance"): ``dist = -sqrt(dist2)`` inside a closed, consistently oriented mesh or an analytic sphere, ``+sqrt(dist2)`` outside and on the surface,
``inf`` where nothing is found.  The first signed call after the geometry changed builds the table of pseudo-normals on the device, on the same stream
(no host sync); ``mesh_report()`` builds it at once, waits, and says whether the meshes are closed -- on an open mesh the sign is "which side of the sheet".

``winding_number`` is the generalized winding number (include/tirt.h, "Winding number"): the sum of the signed solid angles of all triangles over 4 pi --
1 inside a closed mesh, 0 outside, fractional near a hole, 2 inside two overlapping shells -- with far clusters of triangles replaced by two terms from
their moments where the cluster is more than ``beta`` of its radii away (``beta >= 1``; ``float("inf")``: the exact sum).  ``w > 0.5`` is the inside test
for meshes that ``mesh_report()`` calls open: ``inside(points, method="winding")``.  The first winding call after the geometry changed builds the moment
table on the device, on the same stream (no host sync).
"""
import collections
import operator
import os

from . import _native

PointHits = collections.namedtuple("PointHits", ["dist2", "prim", "point", "uv"])
SignedHits = collections.namedtuple("SignedHits", ["dist", "prim", "point", "uv"])
PointNearest = collections.namedtuple("PointNearest", ["dist2", "prim", "point", "uv", "count"])


class _Pairs:
    """what the two CSR results share: query() expands row_start to the query index of every pair"""
    __slots__ = ()

    def query(self):
        """[total] int64: the index of the query each pair belongs to (pairs of rows that were cut by a capacity are not among them)"""
        import torch
        lengths = self.row_start[1:] - self.row_start[:-1]
        fits = self.row_start[1:] <= self.prim.shape[0]
        return torch.repeat_interleave(torch.arange(lengths.shape[0], device=lengths.device), lengths * fits)


class PointPairs(_Pairs, collections.namedtuple("PointPairs", ["row_start", "prim", "dist2", "point", "uv"])):
    __slots__ = ()


def _pairs_front(q, what, tri, queries, max_distance, attributes, capacity, ordered, count_only=False):
    """PointQuery.within / TriangleQuery.pairs / .count_within: the checks of the sibling calls, then COUNT, the one host wait and FILL (capacity None),
    or BOTH.  -> (row_start, prim, d2, code, attributes) as tensors"""
    torch = q.torch
    if tri:
        dev, n, stride, queries = q._check_triangles(queries, what)
    else:
        dev, n, stride = q._check_points(queries, what)
    dptr, dstride, dall = q._check_bound(max_distance, dev, n, what)
    if capacity is not None:
        capacity = operator.index(capacity)
        if capacity < 0:
            raise ValueError("%s.%s: capacity must be >= 0, got %d" % (type(q).__name__, what, capacity))
    flags = q.flags | (0 if ordered else _native.PAIRS_UNORDERED)
    stream = torch.cuda.current_stream(dev).cuda_stream
    row_start = torch.empty(n + 1, dtype=torch.int64, device=dev)
    run = q.scene.ctx.query_mesh_pairs if tri else q.scene.ctx.query_point_pairs

    def call(mode, cap, **out):
        run(queries.data_ptr() if n else 0, n, stride, mode, row_start.data_ptr(), capacity=cap, stack_size=q.stack_size, flags=flags, dmax=dptr,
            dmax_stride=dstride, dmax_all=dall, stream=stream, **out)
    mode = _native.PAIRS_BOTH
    if capacity is None or count_only:
        call(_native.PAIRS_COUNT, 0)
        if count_only:
            return row_start
        capacity, mode = int(row_start[-1].item()), _native.PAIRS_FILL      # the one host wait of this path
    prim = torch.empty(capacity, dtype=torch.int32, device=dev)
    d2 = torch.empty(capacity, dtype=torch.float32, device=dev)
    code = torch.empty(capacity, dtype=torch.int32, device=dev) if tri else None
    out = dict(out_d2=d2.data_ptr(), out_prim=prim.data_ptr())
    a0 = a1 = None
    if tri:
        out["out_code"] = code.data_ptr()
        if attributes:
            a0 = torch.empty((capacity, 2, 3), dtype=torch.float32, device=dev)
            out["out_points"] = a0.data_ptr()
    elif attributes:
        a0 = torch.empty((capacity, 3), dtype=torch.float32, device=dev)
        a1 = torch.empty((capacity, 2), dtype=torch.float32, device=dev)
        out["out_point"], out["out_uv"] = a0.data_ptr(), a1.data_ptr()
    if n or mode == _native.PAIRS_BOTH:
        call(mode, capacity, **out)
    if tri:
        from .TriangleQuery import TrianglePairs
        return TrianglePairs(row_start, prim, d2, code, a0[:, 0] if attributes else None, a0[:, 1] if attributes else None)
    return PointPairs(row_start, prim, d2, a0, a1)


def _torch():
    try:
        import torch
    except ImportError as exc:
        raise ImportError("ti_raytrace_amd.PointQuery needs PyTorch (ROCm build); the C-ABI tirt_query_closest_point "
                          "(include/tirt.h) works without it") from exc
    return torch


class PointQuery:
    def __init__(self, scene, stack_size=64, flags=0):
        self.torch = _torch()
        if not 1 <= int(stack_size) <= 4096:
            raise ValueError("PointQuery: stack_size must be 1..4096, got %r" % (stack_size,))
        if int(flags) & ~(_native.TRAVERSE_EXHAUSTIVE | _native.COUNT_NODES):
            raise ValueError("PointQuery: flags are TRAVERSE_EXHAUSTIVE and COUNT_NODES, got %r" % (flags,))
        self.scene = scene
        self.stack_size = int(stack_size)
        self.flags = int(flags)

    def _device(self):
        """the scene context's device, without creating the context"""
        ctx = getattr(self.scene, "_ctx", None)
        if ctx is not None:
            dev = ctx.device_id
        else:
            dev = getattr(self.scene, "_device_id", None)
            if dev is None:
                dev = int(os.environ.get("LOCAL_RANK", "0"))           # what Scene.ctx will pick
        return self.torch.device("cuda", int(dev))

    def _check_points(self, points, what):
        torch = self.torch
        if not isinstance(points, torch.Tensor):
            raise TypeError("PointQuery.%s: points must be a torch.Tensor, got %s" % (what, type(points).__name__))
        if points.dtype != torch.float32:
            raise TypeError("PointQuery.%s: points must be float32, got %s" % (what, points.dtype))
        # (type and layout first: these checks need no device)
        if points.dim() != 2 or points.shape[1] < 3:
            raise ValueError("PointQuery.%s: points must be [N, C >= 3], got shape %s" % (what, tuple(points.shape)))
        n = points.shape[0]
        if n > 1 and points.stride(0) < 3:
            raise ValueError("PointQuery.%s: rows of points overlap (stride(0) = %d < 3)" % (what, points.stride(0)))
        if n > 0 and points.stride(1) != 1:
            raise ValueError("PointQuery.%s: the last dimension of points must have stride 1, got %d" % (what, points.stride(1)))
        if points.device.type != "cuda":
            raise TypeError("PointQuery.%s: points must be on the GPU, got a %s tensor" % (what, points.device.type))
        dev = self._device()
        if points.device != dev:
            raise ValueError("PointQuery.%s: points are on %s, the scene's context on %s" % (what, points.device, dev))
        return dev, n, (points.stride(0) if n > 1 else max(points.shape[1], 3))

    def _check_bound(self, max_distance, dev, n, what):
        """(device address or 0, stride, the bound of every query when the address is 0)"""
        torch = self.torch
        if max_distance is None:
            return 0, 1, float("inf")
        if isinstance(max_distance, torch.Tensor):
            if max_distance.dtype != torch.float32:
                raise TypeError("PointQuery.%s: max_distance must be float32, got %s" % (what, max_distance.dtype))
            if max_distance.device != dev:
                raise ValueError("PointQuery.%s: max_distance is on %s, the points on %s" % (what, max_distance.device, dev))
            if max_distance.dim() != 1 or max_distance.shape[0] != n:
                raise ValueError("PointQuery.%s: max_distance must be [N] = [%d], got shape %s" % (what, n, tuple(max_distance.shape)))
            if n > 1 and max_distance.stride(0) < 1:
                raise ValueError("PointQuery.%s: max_distance must have a positive stride, got %d" % (what, max_distance.stride(0)))
            if n:
                return max_distance.data_ptr(), (max_distance.stride(0) if n > 1 else 1), float("inf")
            return 0, 1, float("inf")
        if isinstance(max_distance, (int, float)):
            return 0, 1, float(max_distance)
        raise TypeError("PointQuery.%s: max_distance must be None, a float or a float32 tensor, got %s" % (what, type(max_distance).__name__))

    def closest(self, points, max_distance=None, attributes=False):
        """The nearest surface point of every query, bit for bit Context.closest_point's: dist2 (inf where nothing is found), prim (-1) and, with
        attributes=True, the point and its (u, v).  Asynchronous on the current stream."""
        torch = self.torch
        dev, n, stride = self._check_points(points, "closest")
        dptr, dstride, dall = self._check_bound(max_distance, dev, n, "closest")
        d2 = torch.empty(n, dtype=torch.float32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        point = torch.empty((n, 3), dtype=torch.float32, device=dev) if attributes else None
        uv = torch.empty((n, 2), dtype=torch.float32, device=dev) if attributes else None
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            self.scene.ctx.query_closest_point(points.data_ptr(), n, stride, self.stack_size, self.flags, dmax=dptr, dmax_stride=dstride, dmax_all=dall,
                                               out_d2=d2.data_ptr(), out_prim=prim.data_ptr(), out_point=point.data_ptr() if attributes else 0,
                                               out_uv=uv.data_ptr() if attributes else 0, stream=stream)
        return PointHits(d2, prim, point, uv)

    def signed_distance(self, points, max_distance=None, attributes=False):
        """The signed distance to the nearest surface point of every query, bit for bit Context.signed_distance's: dist (inf where nothing is found; negative
        inside), prim (-1) and, with attributes=True, the point and its (u, v) -- those three are closest()'s.  Asynchronous on the current stream."""
        torch = self.torch
        dev, n, stride = self._check_points(points, "signed_distance")
        dptr, dstride, dall = self._check_bound(max_distance, dev, n, "signed_distance")
        sd = torch.empty(n, dtype=torch.float32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        point = torch.empty((n, 3), dtype=torch.float32, device=dev) if attributes else None
        uv = torch.empty((n, 2), dtype=torch.float32, device=dev) if attributes else None
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            self.scene.ctx.query_signed_distance(points.data_ptr(), n, stride, sd.data_ptr(), self.stack_size, self.flags, dmax=dptr, dmax_stride=dstride,
                                                 dmax_all=dall, out_prim=prim.data_ptr(), out_point=point.data_ptr() if attributes else 0,
                                                 out_uv=uv.data_ptr() if attributes else 0, stream=stream)
        return SignedHits(sd, prim, point, uv)

    def nearest(self, points, k, max_distance=None, attributes=False, count=False):
        """The k nearest primitives of every query in the order of include/tirt.h, "K nearest primitives": dist2 [N, k] (inf where fewer are within the
        bound), prim [N, k] (-1), with attributes=True the points [N, k, 3] and their (u, v) [N, k, 2], with count=True the number of all primitives
        within the bound [N] int32.  Asynchronous on the current stream."""
        torch = self.torch
        try:
            k = operator.index(k)
        except TypeError:
            raise TypeError("PointQuery.nearest: k must be an int, got %s" % type(k).__name__) from None
        if not 0 <= k <= _native.NEAREST_MAX:
            raise ValueError("PointQuery.nearest: k must be 0..%d, got %d" % (_native.NEAREST_MAX, k))
        if k == 0 and not count:
            raise ValueError("PointQuery.nearest: k == 0 without count=True returns nothing")
        dev, n, stride = self._check_points(points, "nearest")
        dptr, dstride, dall = self._check_bound(max_distance, dev, n, "nearest")
        d2 = torch.empty((n, k), dtype=torch.float32, device=dev)
        prim = torch.empty((n, k), dtype=torch.int32, device=dev)
        point = torch.empty((n, k, 3), dtype=torch.float32, device=dev) if attributes else None
        uv = torch.empty((n, k, 2), dtype=torch.float32, device=dev) if attributes else None
        cnt = torch.empty(n, dtype=torch.int32, device=dev) if count else None
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            self.scene.ctx.query_nearest(points.data_ptr(), n, stride, k, self.stack_size, self.flags, dmax=dptr, dmax_stride=dstride, dmax_all=dall,
                                         out_d2=d2.data_ptr() if k else 0, out_prim=prim.data_ptr() if k else 0,
                                         out_point=point.data_ptr() if attributes and k else 0, out_uv=uv.data_ptr() if attributes and k else 0,
                                         out_count=cnt.data_ptr() if count else 0, stream=stream)
        return PointNearest(d2, prim, point, uv, cnt)

    def count_within(self, points, max_distance):
        """[N] int32: how many primitives lie within max_distance (a float or an [N] float32 tensor; required) of every query -- nearest(k=0, count=True)"""
        if max_distance is None:
            raise TypeError("PointQuery.count_within: max_distance is required (without a bound every primitive counts)")
        return self.nearest(points, 0, max_distance, count=True).count

    def within(self, points, max_distance, attributes=False, capacity=None, ordered=True):
        """EVERY primitive within max_distance (a float or an [N] float32 tensor; None = no bound: every primitive of the scene for every query) of every
        query, as CSR rows (include/tirt.h, "Point pairs"): PointPairs(row_start [N + 1] int64, prim [total] i32, dist2 [total] f32, point [total, 3], uv
        [total, 2] or None).  Row i is the slice row_start[i] : row_start[i + 1]; inside a row dist2 ascends and ties go to the smaller primitive id, so
        its element 0 is closest()'s answer and its first k elements are nearest(k)'s; ordered=False skips that pass (the order is then unspecified).
        capacity=None sizes the result exactly: a counting call, ONE HOST WAIT to read the total (row_start[-1].item()), then the filling call.
        capacity=c runs both in one call with no host wait, into arrays of c pairs: only the rows that fit entirely (row_start[i + 1] <= c) are
        written, row_start is complete, and row_start[-1] > c says the result was cut (what lies behind the last row that fits is uninitialised)."""
        return _pairs_front(self, "within", False, points, max_distance, attributes, capacity, ordered)

    def inside(self, points, method="pseudonormal"):
        """[N] bool: signed_distance(points).dist < 0, or with method="winding": winding_number(points) > 0.5 (open, flipped or intersecting meshes)"""
        if method == "pseudonormal":
            return self.signed_distance(points).dist < 0
        if method == "winding":
            return self.winding_number(points) > 0.5
        raise ValueError('PointQuery.inside: method is "pseudonormal" or "winding", got %r' % (method,))

    def _winding(self, points, beta, what, count):
        torch = self.torch
        try:
            beta = float(beta)
        except (TypeError, ValueError):
            raise TypeError("PointQuery.%s: beta must be a float, got %s" % (what, type(beta).__name__)) from None
        if not beta >= 1.0:
            raise ValueError("PointQuery.%s: beta must be >= 1 or inf, got %r" % (what, beta))
        dev, n, stride = self._check_points(points, what)
        w = torch.empty(n, dtype=torch.float32, device=dev)
        counts = torch.empty((n, 2), dtype=torch.int32, device=dev) if count else None
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            self.scene.ctx.query_winding_number(points.data_ptr(), n, stride, w.data_ptr(), beta=beta, stack_size=self.stack_size,
                                                flags=self.flags | (_native.COUNT_NODES if count else 0), counts=counts.data_ptr() if count else 0,
                                                stream=stream)
        return w, counts

    def winding_number(self, points, beta=2.0):
        """[N] float32: the generalized winding number of every query, bit for bit Context.winding_number's (NaN for a query with a NaN or infinite
        coordinate, or one that ran out of traversal stack).  Asynchronous on the current stream."""
        return self._winding(points, beta, "winding_number", False)[0]

    def winding_counts(self, points, beta=2.0):
        """winding_number() with the per-query counts ([N, 2] int32: child slots examined, leaves evaluated) of a COUNT_NODES walk: (w, counts)"""
        return self._winding(points, beta, "winding_counts", True)

    def mesh_report(self):
        """Builds the pseudo-normal table now and waits for it: the counts of triangle edges that are boundary, non-manifold and flipped, of invalid
        (zero-area or non-finite) triangles and of primitives, and closed = the first four are zero (the sign means inside / outside everywhere)"""
        return self.scene.ctx.signed_distance_prepare()

    def closest_counts(self, points, max_distance=None):
        """closest() with the per-query N_box / N_leaf counts ([N, 2] int32) of a COUNT_NODES walk: (PointHits, counts)"""
        torch = self.torch
        dev, n, stride = self._check_points(points, "closest_counts")
        dptr, dstride, dall = self._check_bound(max_distance, dev, n, "closest_counts")
        d2 = torch.empty(n, dtype=torch.float32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        counts = torch.empty((n, 2), dtype=torch.int32, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            self.scene.ctx.query_closest_point(points.data_ptr(), n, stride, self.stack_size, self.flags | _native.COUNT_NODES, dmax=dptr,
                                               dmax_stride=dstride, dmax_all=dall, out_d2=d2.data_ptr(), out_prim=prim.data_ptr(),
                                               counts=counts.data_ptr(), stream=stream)
        return PointHits(d2, prim, None, None), counts
