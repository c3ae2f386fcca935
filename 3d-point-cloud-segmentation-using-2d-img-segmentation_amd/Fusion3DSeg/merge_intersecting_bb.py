"""Drop-in for the reference's Fusion3DSeg/merge_intersecting_bb.py::merge_bb.

The reference decides that two instances overlap when their oriented boxes share at least one cloud point and
does so with O(B^2) full-cloud scans plus Python list intersections (reference :64-91).  Here every scan of one
outer iteration is ONE kernel launch (f3d_points_in_obb*: all points x {box of id1, boxes of its candidates},
membership bitset in LDS, box-pair co-occurrence matrix); the control flow -- including the list-index-as-id
and delete-while-iterating quirks (Q6/Q7) and the early return at :83-84 -- stays on the host so ids match.

Oriented boxes: the fit itself (Open3D's ``OrientedBoundingBox.create_from_points``: convex hull -> PCA of the hull
vertices -> extents in that frame) runs on the GPU for all instances of a cloud in one launch (``f3d_obb_candidates_dev`` +
``f3d_obb_fit_dev``: hull vertex set with certified orientation signs, Jacobi eigen-solve).  An instance the kernel cannot
certify (coplanar / duplicate points ...) is DEFERRED to the host fit ``obb_from_points`` below -- Open3D when it is installed,
otherwise the same recipe on scipy's Qhull.  The recipe is unpinned against Open3D itself (absent from the image).
"""
import json
import os
import time
from pathlib import Path

import numpy as np

import f3d
from f3d import sharding


def obb_from_points(pts):
    """(center [3], R [3,3] columns = axes, extent [3]) of the PCA-aligned box of the convex hull."""
    try:
        import open3d as o3d
        b = o3d.geometry.OrientedBoundingBox.create_from_points(o3d.utility.Vector3dVector(pts))
        return np.asarray(b.center), np.asarray(b.R), np.asarray(b.extent)
    except ImportError:
        pass
    from scipy.spatial import ConvexHull
    pts = np.asarray(pts, np.float64)
    hp = pts[np.sort(ConvexHull(pts).vertices)]
    mean = hp.mean(0)
    evals, evecs = np.linalg.eigh(np.cov((hp - mean).T, bias=True))
    R = evecs[:, np.argsort(-evals, kind='stable')]
    R[:, 2] = np.cross(R[:, 0], R[:, 1])
    loc = (hp - mean) @ R
    lo, hi = loc.min(0), loc.max(0)
    return mean + R @ ((lo + hi) / 2), R, hi - lo


def obb_corners(center, R, extent):
    x, y, z = (R[:, i] * extent[i] / 2 for i in range(3))
    c = np.asarray(center)
    return np.array([c - x - y - z, c + x - y - z, c - x + y - z, c - x - y + z,
                     c + x + y + z, c - x + y + z, c + x - y + z, c + x + y - z])


def _pack(boxes):
    return np.array([np.concatenate([c, np.asarray(R).reshape(-1), e]) for c, R, e in boxes], np.float64).reshape(-1, 15)


def cal_min_max(id, id_info_per_point, pcd_points, box_fn=None):
    """Dead code of the reference (:15-42), kept for importers: the extents of instance `id`'s oriented-box corners along
    the world axes.  The reference projects the 8 corners on the three axis lines with skspatial's ``Line.project_point``
    (= the corner with the other two coordinates zeroed), takes the column-wise min / max and then drops the ZERO entries
    (:24-25 -- a bug: an extent that is exactly 0 disappears as well); each of the six results is therefore an array of
    0 or 1 elements.  skspatial and Open3D are absent from the image: restated, parity unpinned."""
    pts = np.asarray(pcd_points)[np.where(id_info_per_point == id)]
    corners = obb_corners(*(box_fn or obb_from_points)(pts))
    out = []
    for axis in range(3):
        proj = np.zeros((8, 3))
        proj[:, axis] = corners[:, axis]
        mn, mx = proj.min(axis=0), proj.max(axis=0)
        out += [mn[np.nonzero(mn)], mx[np.nonzero(mx)]]
    return tuple(out)


def check_intersection(id1, id_list, id_info_per_point, pcd_points, info_sem, box_fn=None):
    """Dead code of the reference (:44-56): axis-interval overlap of the boxes of id1 and every id2 of the same
    ``category_id``.  Quirks kept: the result list is re-created inside the loop (:48), so only the LAST id2 can be
    reported; instance ids are looked up through ``id_list`` here (unlike check_intersection_open3d)."""
    min_x1, max_x1, min_y1, max_y1, min_z1, max_z1 = cal_min_max(id_list[id1], id_info_per_point, pcd_points, box_fn)
    intersecting_id = []
    for id2 in range(1, len(id_list)):
        if id1 != id2:
            intersecting_id = []
            if info_sem[id1]["category_id"] == info_sem[id2]["category_id"]:
                min_x2, max_x2, min_y2, max_y2, min_z2, max_z2 = cal_min_max(id_list[id2], id_info_per_point, pcd_points, box_fn)
                if (((min_x1 <= min_x2 and min_x2 <= max_x1) or (min_x2 <= min_x1 and min_x1 <= max_x2)) and
                        ((min_y1 <= min_y2 and min_y2 <= max_y1) or (min_y2 <= min_y1 and min_y1 <= max_y2)) and
                        ((min_z1 <= min_z2 and min_z2 <= max_z1) or (min_z2 <= min_z1 and min_z1 <= max_z2))):
                    intersecting_id.append(id2)
    return intersecting_id


def intersection_point_bb(lst1, lst2):
    s = set(lst2)
    return [v for v in lst1 if v in s]


def update_id_info(id1, int_bb, info_sem, id_info_per_point):
    """Relabel instance int_bb as id1 and add its area (reference :58-62); arrays mutated in place."""
    info_sem[id1]["area"] += info_sem[int_bb]["area"]
    id_info_per_point[id_info_per_point == int_bb] = id1
    return info_sem, id_info_per_point


class HipCloud:
    """The cloud resident on the GPU for one merge: grouping by instance id, hull candidates and point-in-box scans through
    libf3d_hip (f3d_group_by_id*, f3d_obb_extremes*, f3d_obb_hull_filter*, f3d_points_in_obb*).  With torch the arrays stay on
    the device across the calls; without it the host-pointer entry points upload what they need (the context keeps the cloud
    between the three grouping calls).  `point_range` = the [lo, hi) share of the points this process scans (sharded merge)."""

    def __init__(self, pts, point_range=None):
        self.n = len(pts)
        self.lo, self.hi = (0, self.n) if point_range is None else point_range
        self.ctx = f3d.default_context()
        self.torch = None
        self._host = None
        try:
            import torch
            if torch.cuda.is_available():
                self.torch = torch
                self.device = torch.device('cuda', self.ctx.device)
                self.stream = torch.cuda.Stream(self.device)
                if torch.is_tensor(pts):                               # a cloud that is already resident (merge_bb_dev): used where it lies
                    if not (pts.is_cuda and pts.dtype == torch.float64 and pts.is_contiguous() and pts.dim() == 2 and pts.shape[1] == 3):
                        raise ValueError('a device cloud must be a contiguous float64 CUDA tensor [N, 3]')
                    self.stream.wait_stream(torch.cuda.current_stream(self.device))
                    self.dev = pts
                else:
                    self._host = pts
                    with torch.cuda.stream(self.stream):
                        self.dev = torch.from_numpy(pts).to(self.device)
                    self.stream.synchronize()
        except ImportError:
            pass
        if self.torch is None:
            self._host = pts

    @property
    def pts(self):
        """The cloud on the host (downloaded on first use when the caller handed over a device tensor: only the host fallbacks need it)."""
        if self._host is None:
            self._host = self.dev.cpu().numpy()
        return self._host

    def group(self, ids, nids):
        """(order int32 [n], starts int64 [nids + 2]) -- members of every id in ascending point index."""
        if self.torch is None:
            return self.ctx.group_by_id(ids, nids)
        torch = self.torch
        resident = torch.is_tensor(ids)
        if resident:
            self._resident_ids(ids)
        with torch.cuda.stream(self.stream):
            dids = ids if resident else torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(self.device)
            self.d_order = torch.empty(self.n, dtype=torch.int32, device=self.device)
            self.d_keys = torch.empty(self.n, dtype=torch.int32, device=self.device)
            self.d_starts = torch.empty(nids + 2, dtype=torch.int64, device=self.device)
            self.ctx.group_by_id_dev(dids.data_ptr(), self.n, nids, self.d_order.data_ptr(), self.d_keys.data_ptr(), self.d_starts.data_ptr(),
                                     self.stream.cuda_stream)
            self.stream.synchronize()
            self.nids = nids
            # resident ids: the member lists stay on the device (nobody relabels a host array); only the segment bounds come back
            return (None if resident else self.d_order.cpu().numpy()), self.d_starts.cpu().numpy()

    def _resident_ids(self, ids):
        """Resident ids are read, and relabelled, where they lie: through their data pointer."""
        if not (self.torch.is_tensor(ids) and ids.is_cuda and ids.dtype == self.torch.int64 and ids.dim() == 1 and len(ids) == self.n and ids.is_contiguous()):
            raise ValueError(f'resident ids must be a contiguous int64 CUDA tensor [{self.n}]')

    def relabel(self, ids, src, dst):
        """ids[ids == src] = dst on the device tensor `ids` (update_id_info, merge_intersecting_bb.py:59-61)."""
        self._resident_ids(ids)
        with self.torch.cuda.stream(self.stream):
            self.ctx.relabel_dev(ids.data_ptr(), self.n, int(src), int(dst), None, self.stream.cuda_stream)

    def fit_indices(self, index_sets):
        """Boxes of a few instances given as point-index arrays (refits after a merge), gathered and fitted on the device:
        (boxes [k, 15], status [k])."""
        torch = self.torch
        start = np.zeros(len(index_sets) + 1, np.int64)
        start[1:] = np.cumsum([len(a) for a in index_sets])
        total = int(start[-1])
        flat = np.ascontiguousarray(np.concatenate(index_sets), dtype=np.int32) if total else np.zeros(0, np.int32)
        with torch.cuda.stream(self.stream):
            didx = torch.from_numpy(flat).to(self.device)
            dstart = torch.from_numpy(start).to(self.device)
            cpts = torch.empty((max(total, 1), 3), dtype=torch.float64, device=self.device)
            boxes = torch.empty((len(index_sets), f3d.OBB_DOUBLES), dtype=torch.float64, device=self.device)
            status = torch.empty(len(index_sets), dtype=torch.int32, device=self.device)
            isvert = torch.empty(max(total, 1), dtype=torch.uint8, device=self.device)
            self.ctx.gather_points_dev(self.dev.data_ptr(), f3d.F64, didx.data_ptr(), total, cpts.data_ptr(), self.stream.cuda_stream)
            self.ctx.obb_fit_dev(cpts.data_ptr(), dstart.data_ptr(), len(index_sets), total, boxes.data_ptr(), status.data_ptr(), isvert.data_ptr(), None,
                                 self.stream.cuda_stream)
            self.stream.synchronize()
            return boxes.cpu().numpy(), status.cpu().numpy()

    def extremes(self):
        if self.torch is None:
            return self.ctx.obb_extremes(self.pts)
        torch = self.torch
        with torch.cuda.stream(self.stream):
            out = torch.empty((self.nids, 26), dtype=torch.int32, device=self.device)
            self.ctx.obb_extremes_dev(self.dev.data_ptr(), f3d.F64, self.n, self.d_order.data_ptr(), self.d_keys.data_ptr(), self.nids,
                                      out.data_ptr(), self.stream.cuda_stream)
            self.stream.synchronize()
            return out.cpu().numpy()

    def hull_filter(self, fstart, facets, margin):
        if self.torch is None:
            return self.ctx.obb_hull_filter(fstart, facets, margin)
        torch = self.torch
        with torch.cuda.stream(self.stream):
            dfs = torch.from_numpy(np.ascontiguousarray(fstart, dtype=np.int32)).to(self.device)
            deq = torch.from_numpy(np.ascontiguousarray(facets, dtype=np.float64).reshape(-1, 4)).to(self.device)
            dmg = torch.from_numpy(np.ascontiguousarray(margin, dtype=np.float64)).to(self.device)
            cand = torch.empty(max(self.n, 1), dtype=torch.int32, device=self.device)
            cnt = torch.empty(max(self.nids, 1), dtype=torch.int32, device=self.device)
            self.ctx.obb_hull_filter_dev(self.dev.data_ptr(), f3d.F64, self.n, self.d_order.data_ptr(), self.d_keys.data_ptr(),
                                         self.d_starts.data_ptr(), self.nids, dfs.data_ptr(), deq.data_ptr() if len(deq) else None, dmg.data_ptr(),
                                         cand.data_ptr(), cnt.data_ptr(), self.stream.cuda_stream)
            self.stream.synchronize()
            return cand.cpu().numpy()[:self.n], cnt.cpu().numpy()[:self.nids]

    def candidates_and_boxes(self, min_members):
        """All-device box fits (follows group()): hull candidates of every id in ascending point index (cand int32, cand_start int64
        [nids + 1]), boxes float64 [nids, 15] and status int32 [nids] (f3d.OBB_OK / OBB_FEW / OBB_DEFERRED).  None without torch."""
        if self.torch is None:
            return None
        torch = self.torch
        t0 = time.perf_counter()
        with torch.cuda.stream(self.stream):
            cand = torch.empty(max(self.n, 1), dtype=torch.int32, device=self.device)
            cstart = torch.empty(self.nids + 1, dtype=torch.int64, device=self.device)
            self.ctx.obb_candidates_dev(self.dev.data_ptr(), f3d.F64, self.n, self.d_order.data_ptr(), self.d_keys.data_ptr(), self.d_starts.data_ptr(),
                                        self.nids, min_members, cand.data_ptr(), cstart.data_ptr(), self.stream.cuda_stream)
            self.stream.synchronize()
            cs = cstart.cpu().numpy()
            total = int(cs[-1])
            self.t_candidates = time.perf_counter() - t0
            t0 = time.perf_counter()
            cpts = torch.empty((max(total, 1), 3), dtype=torch.float64, device=self.device)
            boxes = torch.empty((self.nids, f3d.OBB_DOUBLES), dtype=torch.float64, device=self.device)
            status = torch.empty(self.nids, dtype=torch.int32, device=self.device)
            isvert = torch.empty(max(total, 1), dtype=torch.uint8, device=self.device)
            self.ctx.gather_points_dev(self.dev.data_ptr(), f3d.F64, cand.data_ptr(), total, cpts.data_ptr(), self.stream.cuda_stream)
            self.ctx.obb_fit_dev(cpts.data_ptr(), cstart.data_ptr(), self.nids, total, boxes.data_ptr(), status.data_ptr(), isvert.data_ptr(), None,
                                 self.stream.cuda_stream)
            self.stream.synchronize()
            out = cand[:total].cpu().numpy(), cs, boxes.cpu().numpy(), status.cpu().numpy()
            self.t_fit = time.perf_counter() - t0
            return out

    def fit(self, point_sets):
        """Boxes of a few point sets (refits after a merge): (boxes [k, 15], status [k])."""
        return self.ctx.obb_fit(point_sets)

    def cooccurrence(self, packed):
        """uint8 [B, B]: some point of this process's share lies in both boxes (rows of `packed`, float64 [B, 15])."""
        B = len(packed)
        if self.hi <= self.lo:
            return np.zeros((B, B), np.uint8)
        if self.torch is None:
            _, cooc = self.ctx.points_in_obb(self.pts[self.lo:self.hi], packed, want_bits=False, want_cooc=True)
            return cooc.astype(np.uint8)
        torch = self.torch
        with torch.cuda.stream(self.stream):
            cd = torch.empty((B, B), dtype=torch.uint8, device=self.device)
            self.ctx.points_in_obb_dev(self.dev.data_ptr() + 24 * self.lo, f3d.F64, self.hi - self.lo, packed, None, cd.data_ptr(),
                                       self.stream.cuda_stream)
            self.stream.synchronize()
            return cd.cpu().numpy()


def _all_gather_rows(dist, mine):
    """Every rank's float64 array `mine` (same shape everywhere) -> list of all of them, bit for bit."""
    import torch
    dev = 'cuda' if dist.get_backend() == 'nccl' else 'cpu'
    t = torch.from_numpy(np.ascontiguousarray(mine)).to(dev)
    parts = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, t)
    return [x.cpu().numpy() for x in parts]


class _MergeState:
    """Book-keeping that turns the reference's O(B^2) full-cloud rescans and refits into exact incremental updates:
    * the points of every id in ascending point order (one GPU sort, not a 50M-entry host argsort), so that a box is fitted on
      exactly the array ``pcd_points[ids == id]`` the reference would build -- minus the members that provably lie strictly
      inside the hull of the instance's 26 directional extremes (dropped by a GPU pass): hull, hull vertices and box are the
      same, Qhull sees a few hundred points instead of ~10^4;
    * cached boxes with their axis-aligned bounds, refitted only after a merge (on the union of the two candidate lists);
    * the cloud resident on the GPU for the whole merge.
    Sharded (``dist`` = an initialised torch.distributed module): every rank holds the arrays, scans only its contiguous share
    of the points and combines every co-occurrence answer with one all_reduce(MAX); the initial box fits are dealt out by
    instance (id mod world) and exchanged with one all_gather.  The control flow runs identically on every rank."""

    PREFILTER_MIN = 256                                   # instances smaller than this are fitted on all of their points

    def __init__(self, pts, ids, box_fn, dist=None, backend=None, prefilter='auto'):
        # box_fn None = the built-in fit: on the GPU, instances the kernel defers on the host (obb_from_points).  A caller-supplied
        # box_fn gets exactly pcd_points[ids == id] unless it opts into the hull-candidate prefilter (exact for hull-based fits only).
        self.gpu_fit = box_fn is None
        self._pts, self.ids, self.box_fn, self.dist = pts, ids, (box_fn or obb_from_points), dist
        self.use_prefilter = self.gpu_fit if prefilter == 'auto' else bool(prefilter)
        self.prof = {'group': 0.0, 'prefilter': 0.0, 'fit': 0.0, 'nfit': 0, 'nfit_gpu': 0, 'nfit_deferred': 0, 'scan': 0.0, 'nscan': 0, 'absorb': 0.0,
                     'upload': 0.0, 'exchange': 0.0}
        n = len(pts)
        self.rank, self.world = (dist.get_rank(), dist.get_world_size()) if dist is not None else (0, 1)
        share = (n * self.rank // self.world, n * (self.rank + 1) // self.world)
        t0 = time.perf_counter()
        self.cloud = backend(pts, share) if backend is not None else HipCloud(pts, share)
        self.prof['upload'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        self.resident = not isinstance(ids, np.ndarray)  # merge_bb_dev: ids (and the cloud) are device tensors, relabelled in place on the device
        ids_ok = n > 0 and int(ids.min()) >= 0 and int(ids.max()) < 2 ** 30
        if self.resident and not ids_ok:
            raise ValueError('merge_bb_dev: instance ids must lie in [0, 2^30)')
        self.nids = int(ids.max()) + 1 if ids_ok else 0
        self.members = None
        if ids_ok:
            order, starts = self.cloud.group(ids, self.nids)
            if order is not None:
                self.members = {k: [order[starts[k]:starts[k + 1]]] for k in range(self.nids) if starts[k + 1] > starts[k]}
            self.counts = {k: int(starts[k + 1] - starts[k]) for k in range(self.nids) if starts[k + 1] > starts[k]}
        else:                                             # negative or huge ids: plain NumPy grouping (no prefilter either)
            order = np.argsort(ids, kind='stable')
            uniq, start = np.unique(ids[order], return_index=True)
            bounds = np.append(start, n)
            self.members = {int(u): [order[bounds[k]:bounds[k + 1]]] for k, u in enumerate(uniq)}
            self.counts = {k: len(v[0]) for k, v in self.members.items()}
        # hull candidates: ascending point indices, a superset of the hull's vertices
        self.cands = {k: v[0] for k, v in self.members.items()} if self.members is not None else {}
        self.prof['group'] = time.perf_counter() - t0
        self.boxes, self.failed = {}, {}
        self.parents = None                               # merge_bb's mirror of [e["parent_id"] for e in info_sem] (vectorised partner search)
        self.cnt = self.lo = self.hi = self.have = None
        done = False
        if ids_ok and self.gpu_fit and hasattr(self.cloud, 'candidates_and_boxes'):
            t0 = time.perf_counter()
            done = self._fit_all_device()
            spent = time.perf_counter() - t0
            self.prof['prefilter'] = getattr(self.cloud, 't_candidates', 0.0)          # extremes, inner hulls, filter, compaction: all on the device
            self.prof['fit'] += spent - self.prof['prefilter']
        if ids_ok and self.use_prefilter and not done:
            t0 = time.perf_counter()
            self._prefilter(starts)
            self.prof['prefilter'] = time.perf_counter() - t0
        if dist is not None and not done:
            self._fit_all_sharded()

    def _fit_all_device(self):
        """Candidates and boxes of every instance on the GPU (every rank of a sharded merge computes all of them: the kernels are
        deterministic, so no exchange is needed).  Deferred instances keep their candidates and are fitted lazily on the host."""
        res = self.cloud.candidates_and_boxes(self.PREFILTER_MIN)
        if res is None:
            return False
        cand, cs, boxes, status = res
        ok = np.flatnonzero(status == f3d.OBB_OK)
        for k in self.counts:
            self.cands[k] = cand[cs[k]:cs[k + 1]]
        if len(ok):
            c, R, e = boxes[ok, 0:3], boxes[ok, 3:12].reshape(-1, 3, 3), boxes[ok, 12:15]
            half = R * (e / 2)[:, None, :]                                          # [k, 3 (xyz), 3 (axis)]
            signs = np.array([[-1, -1, -1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1], [1, 1, 1], [-1, 1, 1], [1, -1, 1], [1, 1, -1]], np.float64)
            corners = c[:, None, :] + np.einsum('ja,kxa->kjx', signs, half)         # obb_corners for every box
            pad = 1e-9 * (np.abs(corners).max(axis=(1, 2)) + np.abs(e).max(axis=1) + 1.0)
            lo, hi = corners.min(1) - pad[:, None], corners.max(1) + pad[:, None]
            for j, k in enumerate(ok):
                if int(k) in self.counts:
                    self.boxes[int(k)] = (c[j].copy(), R[j].copy(), e[j].copy(), lo[j], hi[j])
        self.prof['nfit'] += len(ok); self.prof['nfit_gpu'] += len(ok)
        return True

    def _prefilter(self, starts):
        """Drop, per instance, the members strictly inside the hull of its directional extremes (exact: see HipCloud / f3d.h)."""
        from scipy.spatial import ConvexHull, QhullError
        big = [k for k, c in self.counts.items() if c >= self.PREFILTER_MIN]
        if not big or not hasattr(self.cloud, 'extremes'):
            return
        ext = self.cloud.extremes()
        fstart = np.zeros(self.nids + 1, np.int32)
        margin = np.zeros(self.nids)
        eqs, nf = [], np.zeros(self.nids, np.int64)
        for k in big:
            e = np.unique(ext[k][ext[k] >= 0])
            if len(e) < 4:
                continue
            p = self.pts[e]
            try:
                eq = ConvexHull(p).equations                              # n . x + o <= 0 inside, |n| = 1
            except (QhullError, ValueError):
                continue                                                  # flat / degenerate / non-finite extremes: keep every member
            eqs.append(eq); nf[k] = len(eq)
            margin[k] = 1e-9 * (np.abs(p).max() + 1.0)
        fstart[1:] = np.cumsum(nf)
        if not eqs:
            return
        facets = np.concatenate(eqs)
        cand, cnt = self.cloud.hull_filter(fstart, facets, margin)
        for k in big:
            if nf[k]:
                self.cands[k] = np.sort(cand[starts[k]:starts[k] + cnt[k]])

    @property
    def pts(self):
        """The cloud on the host (a resident cloud is downloaded on first use: only host fallbacks ask for it)."""
        return self._pts if isinstance(self._pts, np.ndarray) else self.cloud.pts

    def count(self, i):
        return self.counts.get(int(i), 0)

    def mirror(self, info_sem, nlist):
        """Array form of what check_intersection_open3d's partner loop reads per id2 (parent_id of the CURRENT list entry, member count,
        bounds of the fitted box): merge_bb keeps it in step with its deletions and relabels, so that the loop over id2 becomes array
        operations.  The loop's decisions (order, the early return at a small instance, the list-index quirks) are unchanged."""
        size = max(nlist, (max(self.counts) + 1) if self.counts else 0, 1)
        try:
            self.parents = np.array([e["parent_id"] for e in info_sem])
        except Exception:                                 # (ragged / unhashable parent ids: the literal loop handles whatever == means for them)
            self.parents = None
        if self.parents is None or self.parents.ndim != 1 or len(self.parents) != len(info_sem):
            self.parents = None
            return
        self.cnt = np.zeros(size, np.int64)
        for k, c in self.counts.items():
            if 0 <= k < size:
                self.cnt[k] = c
        self.lo, self.hi = np.zeros((size, 3)), np.zeros((size, 3))
        self.have = np.zeros(size, bool)

    def drop_info(self, b):
        if self.parents is not None:
            self.parents = np.delete(self.parents, b)

    def _fit(self, i):
        t0 = time.perf_counter()
        fitted = None
        if self.gpu_fit and hasattr(self.cloud, 'fit_indices') and getattr(self.cloud, 'torch', None) is not None and len(self.cands[i]) >= 4:
            boxes, status = self.cloud.fit_indices([self.cands[i]])            # gathered and fitted on the device
            if status[0] == f3d.OBB_OK:
                fitted = (boxes[0, 0:3].copy(), boxes[0, 3:12].reshape(3, 3).copy(), boxes[0, 12:15].copy())
                self.prof['nfit_gpu'] += 1
            else:
                self.prof['nfit_deferred'] += 1
        if fitted is None:
            hull_only = self.use_prefilter or self.gpu_fit                      # a caller's box_fn gets pcd_points[ids == id] unless it opted in
            src = self.pts[self.cands[i]] if hull_only else self.pts[np.sort(np.concatenate(self.members[i]))]
            if self.gpu_fit and hasattr(self.cloud, 'fit') and getattr(self.cloud, 'torch', 0) is None and len(src) >= 4:
                boxes, status = self.cloud.fit([src])                          # host-pointer entry (no torch in the process)
                if status[0] == f3d.OBB_OK:
                    fitted = (boxes[0, 0:3].copy(), boxes[0, 3:12].reshape(3, 3).copy(), boxes[0, 12:15].copy())
                    self.prof['nfit_gpu'] += 1
        c, R, e = fitted if fitted is not None else self.box_fn(src)
        corners = obb_corners(c, R, e)
        pad = 1e-9 * (np.abs(corners).max() + np.abs(e).max() + 1.0)           # the in-box test rounds; never prune a touching pair
        self.prof['fit'] += time.perf_counter() - t0; self.prof['nfit'] += 1
        return (np.asarray(c, np.float64), np.asarray(R, np.float64), np.asarray(e, np.float64), corners.min(0) - pad, corners.max(0) + pad)

    def _fit_all_sharded(self):
        """Initial boxes of all instances with >= 4 points, dealt out by id mod world, exchanged bit for bit."""
        t0 = time.perf_counter()
        ids = sorted(k for k, c in self.counts.items() if c >= 4)
        mine = np.zeros((len(ids), 22))                                        # c 3, R 9, e 3, lo 3, hi 3, ok 1
        for j, k in enumerate(ids):
            if j % self.world == self.rank:
                try:
                    c, R, e, lo, hi = self._fit(k)
                    mine[j] = np.concatenate([c, R.reshape(-1), e, lo, hi, [1.0]])
                except Exception as exc:                                       # raised again if (and when) the flow asks for this box
                    self.failed[k] = exc
                    mine[j, 21] = -1.0
        parts = _all_gather_rows(self.dist, mine)
        for j, k in enumerate(ids):
            row = parts[j % self.world][j]
            if row[21] > 0:
                self.boxes[k] = (row[0:3].copy(), row[3:12].reshape(3, 3).copy(), row[12:15].copy(), row[15:18].copy(), row[18:21].copy())
            elif row[21] < 0 and k not in self.failed:
                self.failed[k] = RuntimeError(f'the box fit of instance {k} failed on rank {j % self.world}')
        self.prof['exchange'] += time.perf_counter() - t0

    def box(self, i):
        """(center, R, extent, aabb_lo, aabb_hi) of instance i, refitted only after its membership changed."""
        i = int(i)
        if i in self.failed:
            raise self.failed[i]
        if i not in self.boxes:
            self.boxes[i] = self._fit(i)
        return self.boxes[i]

    def absorb(self, dst, src):
        """update_id_info's relabel (reference :59-61) on the incremental state."""
        dst, src = int(dst), int(src)
        t0 = time.perf_counter()
        if self.members is None:                                               # resident ids: one relabel pass on the device
            if src not in self.counts:
                return
            self.cloud.relabel(self.ids, src, dst)
        else:
            moved = self.members.pop(src, None)
            if not moved:
                return
            for part in moved:
                self.ids[part] = dst
            self.members.setdefault(dst, []).extend(moved)
        self.counts[dst] = self.counts.get(dst, 0) + self.counts.pop(src, 0)
        if self.cnt is not None:
            if 0 <= dst < len(self.cnt):
                self.cnt[dst] = self.counts[dst]; self.have[dst] = False
            if 0 <= src < len(self.cnt):
                self.cnt[src] = 0; self.have[src] = False
        cs = self.cands.pop(src)
        self.cands[dst] = np.sort(np.concatenate([self.cands[dst], cs])) if dst in self.cands else cs   # hull(A u B) has its vertices among both lists
        self.boxes.pop(dst, None); self.boxes.pop(src, None)
        self.failed.pop(dst, None); self.failed.pop(src, None)
        self.prof['absorb'] += time.perf_counter() - t0

    def shares_point(self, box1, others):
        """For each box in `others`: does some cloud point lie in both it and box1?  One launch over (this rank's share of) the cloud,
        one all_reduce(MAX) of the answers when sharded."""
        hits = np.zeros(len(others), np.uint8)
        t0 = time.perf_counter()
        for s in range(0, len(others), f3d.MAX_OBB - 1):
            part = [box1] + others[s:s + f3d.MAX_OBB - 1]
            cooc = self.cloud.cooccurrence(_pack([(b[0], b[1], b[2]) for b in part]))
            hits[s:s + len(part) - 1] = cooc[0, 1:]
        if self.dist is not None:
            t1 = time.perf_counter()
            hits = sharding.sharded_cooccurrence(self.dist, hits)
            self.prof['exchange'] += time.perf_counter() - t1
        self.prof['scan'] += time.perf_counter() - t0; self.prof['nscan'] += 1
        return hits.astype(bool)


def check_intersection_open3d(id1, id_list, id_info_per_point, pcd_points, pcd, info_sem, box_fn=None, state=None):
    """Ids (list indices) whose box shares a cloud point with the box of id1 (reference :68-91).

    Same decisions as the reference, fewer scans: a partner whose box's axis-aligned bounds do not touch those of
    id1's box cannot share a point with it, so only the touching partners are tested on the GPU (exact pruning)."""
    st = state if state is not None else _MergeState(pcd_points, id_info_per_point, box_fn)
    if st.count(id1) < 4:
        return []
    box1 = st.box(id1)
    cand = []
    if st.parents is not None and len(st.parents) == len(info_sem) and len(id_list) <= len(st.cnt):
        # the loop below on arrays (merge_bb's mirror): same-parent partners in ascending order, cut at the first small one
        L = len(info_sem)
        if id1 < L - 1:
            hi = min(len(id_list), L - 1)
            same = np.flatnonzero(st.parents[1:hi] == st.parents[id1]) + 1
            same = same[same != id1]
            small = np.flatnonzero(st.cnt[same] < 4)
            if small.size:
                same = same[:small[0]]                     # the reference returns what it has so far (:83-84)
            for id2 in same[~st.have[same]].tolist():      # boxes fitted (or refitted after a merge) since they were last looked at
                b2 = st.box(id2)
                st.lo[id2], st.hi[id2], st.have[id2] = b2[3], b2[4], True
            with np.errstate(invalid='ignore'):
                touch = (box1[3] <= st.hi[same]).all(axis=1) & (st.lo[same] <= box1[4]).all(axis=1)
            cand = same[touch].tolist()
    else:
        for id2 in range(1, len(id_list)):
            if id1 != id2 and id2 < len(info_sem) - 1 and id1 < len(info_sem) - 1:
                if info_sem[id1]["parent_id"] == info_sem[id2]["parent_id"]:
                    if st.count(id2) < 4:
                        break                              # the reference returns what it has so far (:83-84)
                    b2 = st.box(id2)
                    if (box1[3] <= b2[4]).all() and (b2[3] <= box1[4]).all():
                        cand.append(id2)
    if not cand:
        return []
    hit = st.shares_point(box1, [st.box(c) for c in cand])
    return [c for c, h in zip(cand, hit) if h]


def merge_bb(dir_name, info_sem, id_info_per_point, pcd, box_fn=None, dist=None, backend=None, prefilter='auto'):
    """Merge same-parent instances whose boxes share a point; writes final_info.json and ids.npy (reference :103-137).
    ``dist``: an initialised ``torch.distributed`` module -- every rank calls merge_bb with the same arguments, scans its share of
    the points and gets the same result (rank 0 writes the files).  ``backend``: the object that groups and scans the cloud
    (default: the HIP library; the CPU tests of the sharded control flow inject a NumPy one).  ``box_fn`` None = the built-in fit
    (GPU, host for the instances the kernel defers); a caller-supplied ``box_fn`` is called on ``pcd_points[ids == id]`` like the
    reference's, or -- ``prefilter=True``, exact for hull-based fits only -- on the instance's hull candidates."""
    n0 = len(info_sem)
    resident = not isinstance(id_info_per_point, np.ndarray) and hasattr(id_info_per_point, 'is_cuda')
    pts = pcd if resident else np.ascontiguousarray(np.asarray(pcd.points if hasattr(pcd, 'points') else pcd), dtype=np.float64)
    t0 = time.perf_counter()
    id_list = [info_sem[i]["id"] for i in range(len(info_sem))]
    st = _MergeState(pts, id_info_per_point, box_fn, dist, backend, prefilter)
    st.mirror(info_sem, len(id_list))
    for id1 in range(1, len(id_list)):
        hits = check_intersection_open3d(id1, id_list, id_info_per_point, pts, pcd, info_sem, box_fn, st)
        if hits:
            for b in hits:
                info_sem[id1]["area"] += info_sem[b]["area"]       # update_id_info (:58-62)
                st.absorb(id1, b)
            for b in hits:
                if b < len(info_sem):
                    del info_sem[b]
                    st.drop_info(b)
    ks, bx = [], []
    for k in range(1, len(info_sem)):
        i = info_sem[k]["id"]
        if st.count(i) > 4:
            ks.append(k); bx.append(st.box(i)[:3])
    if ks:                                                 # obb_corners for all of them at once (the same operations in the same order per element)
        C = np.array([b[0] for b in bx], np.float64)
        Rm = np.array([np.asarray(b[1], np.float64) for b in bx]).reshape(-1, 3, 3)
        E = np.array([b[2] for b in bx], np.float64)
        x, y, z = (Rm[:, :, a] * E[:, a:a + 1] / 2 for a in range(3))
        corners = np.stack([C - x - y - z, C + x - y - z, C - x + y - z, C - x - y + z,
                            C + x + y + z, C - x + y + z, C + x - y + z, C + x + y - z], axis=1)
        for k, cs in zip(ks, corners.tolist()):
            info_sem[k]["bbox"] = cs
    print(f'Time taken for merging {n0} to {len(info_sem)} Bounding boxes = {time.perf_counter() - t0} seconds')
    if os.environ.get('F3D_MERGE_PROFILE'):
        print('merge_bb breakdown [s]: ' + ', '.join(f'{k}={v:.3f}' if isinstance(v, float) else f'{k}={v}' for k, v in st.prof.items()))
    if dir_name is not None and (dist is None or dist.get_rank() == 0):
        out = Path(dir_name) / "panoptic_segmentation"
        out.mkdir(parents=True, exist_ok=True)
        with open(out / "final_info.json", 'w') as fp:
            json.dump(info_sem, fp, indent=4)
        with open(out / "ids.npy", 'wb') as fi:
            np.save(fi, id_info_per_point.cpu().numpy() if resident else id_info_per_point)
    return info_sem, id_info_per_point


def merge_bb_dev(info_sem, ids, points, dir_name=None, dist=None):
    """merge_bb on a RESIDENT cloud: ``points`` float64 CUDA tensor [N, 3], ``ids`` int64 CUDA tensor [N] (relabelled in place on
    the device, like the reference mutates its array).  Nothing of the cloud crosses PCIe: grouping, hull candidates, box fits,
    scans and relabels run on the tensors where they lie; the host sees the segment bounds, the candidates' indices and the boxes.
    Same result as merge_bb on the host copies (tests/test_mirror_gpu.py)."""
    import torch
    if not (torch.is_tensor(ids) and ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous() and ids.dim() == 1):
        raise ValueError('merge_bb_dev: ids must be a contiguous int64 CUDA tensor [N]')
    if not (torch.is_tensor(points) and points.is_cuda and len(points) == len(ids)):
        raise ValueError('merge_bb_dev: points must be a CUDA tensor [N, 3] of the same length as ids')
    return merge_bb(dir_name, info_sem, ids, points, dist=dist)
