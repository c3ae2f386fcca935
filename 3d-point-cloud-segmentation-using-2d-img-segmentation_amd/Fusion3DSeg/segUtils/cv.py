"""``split_into_instances`` and ``CVSegmentation`` of the reference's Fusion3DSeg/segUtils/cv.py on the GPU.

The reference flood-fills, class by class, from the lowest remaining point index through same-class neighbours
(a Python list queue).  Here the flood fill is one GPU pass (f3d_components_same_class: lock-free union-find over the
CSR adjacency, every component rooted at its smallest index); the numbering that follows -- classes in the given
order, components by ascending seed, small clusters folded into one "unclassified" bucket created on first use -- is
reproduced with array operations, so ids, info records and updated classes are identical to the reference's
(pinned by tests/golden/split_instances.npz).

``CVSegmentation`` (:7-399) also returns every cluster in the reference's flood (pop) order and its boundary, and grows
colour regions (``color_segment``).  Its floods are f3d_flood_order (all clusters at once, level by level, in the
reference's order) and f3d_color_segment (one GPU workgroup for the whole seed list); the numbering and the final fold of
category-0 records (``merge_instances_by_classes``) are host bookkeeping over the per-cluster pieces.  Pinned by
tests/golden/cvseg.npz.  The private ``_floodfill_*`` helpers and ``_get_clusters`` (which cannot run in the reference) are
not ported.  Stated difference: colours must be float64 or float32 (TypeError otherwise; uint8 colours wrap in the reference).

One stated difference: the adjacency is used as an undirected graph.  The reference follows neighbour lists as
directed edges; the two coincide for symmetric lists, which is what ``KDTree.query_radius`` (the only producer,
fusion.py:369-377) returns.
"""
from collections.abc import Sequence

import numpy as np

import f3d
from f3d.tensors import CSR_ADJACENCY, device_csr, dtype_code, host_csr, on_device, work_stream


def adjacency_to_csr(adj, n):
    """list / object array of neighbour index arrays -> (offsets int64 [n+1], neighbours int32 [E]); a CSR pair
    (as ``fusion.radius_adjacency(..., as_csr=True)`` returns it) passes through."""
    if isinstance(adj, tuple) and len(adj) == 2:
        offs, nbrs = np.ascontiguousarray(adj[0], np.int64), np.ascontiguousarray(adj[1], np.int32)
        if len(offs) != n + 1:
            raise ValueError('CSR adjacency: offsets must have n + 1 entries')
        return offs, nbrs
    lens = np.fromiter((len(a) for a in adj), dtype=np.int64, count=n)
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    if n == 0 or offs[-1] == 0:
        return offs, np.zeros(0, np.int32)
    return offs, np.concatenate([np.asarray(a).reshape(-1) for a in adj]).astype(np.int32)


def split_into_instances(classes, adj, nclasses=133, instance_classes=None, minimum_points=1, verbose=False):
    """-> (instance ids [M], point ids [N], info list, updated classes [N]); see the reference docstring (:402-424)."""
    n = len(classes)
    classes = np.array(classes).copy()
    offs, nbrs = adjacency_to_csr(adj, n)
    ctx = f3d.default_context()
    allclasses = np.unique(classes)
    ids = np.zeros_like(classes)
    info, small_id = [], None
    if instance_classes is None:
        instance_classes, semantic_classes, ninst = allclasses, [], 0
        if (instance_classes == nclasses).any():
            instance_classes = instance_classes[instance_classes != nclasses]
            semantic_classes, ninst = [nclasses], 1
    else:
        instance_classes = np.array(instance_classes)
        semantic_classes = np.setdiff1d(allclasses, instance_classes)
        ninst = len(semantic_classes)
    for k in range(ninst if len(semantic_classes) else 0):
        c = semantic_classes[k]
        m = classes == c
        ids[m] = k
        if c == nclasses:
            small_id = k
        info.append({'id': k, 'isthing': False, 'category_id': int(c), 'area': int(m.sum())})

    root = ctx.components_same_class(classes, offs, nbrs) if n else np.zeros(0, np.int64)
    relabelled = False                                           # some cluster's class was rewritten since `root` was computed
    for c in instance_classes:
        if verbose:
            print('splitting class:', c)
        if relabelled and c == nclasses:                         # folded clusters now belong to this class: flood again
            root = ctx.components_same_class(classes, offs, nbrs)
            relabelled = False
        pts = np.nonzero(classes == c)[0]
        if not len(pts):
            continue
        seeds, inv, sizes = np.unique(root[pts], return_inverse=True, return_counts=True)      # ascending seed = visit order
        big = sizes >= minimum_points
        rank = np.cumsum(big) - 1                                # running index among the kept clusters
        comp_id = ninst + rank
        nbig = int(big.sum())
        if not big.all():
            first_small = int(np.argmax(~big))
            if small_id is None:                                 # the bucket takes the next id at its first use (:483-487)
                small_id = ninst + int(big[:first_small].sum())
                comp_id = comp_id + (np.arange(len(seeds)) > first_small)
                new_small = True
            else:
                new_small = False
            comp_id = np.where(big, comp_id, small_id)
        else:
            new_small = False
        # info records in id order: kept clusters, with the bucket's record spliced in where it was created
        recs = [{'id': int(i), 'isthing': True, 'category_id': int(c), 'area': int(a)} for i, a in zip(comp_id[big], sizes[big])]
        if new_small:
            pos = int(small_id - ninst)
            recs.insert(pos, {'id': int(small_id), 'isthing': True, 'category_id': int(nclasses), 'area': 0})
        info.extend(recs)
        if not big.all():
            info[small_id]['area'] += int(sizes[~big].sum())
            classes[pts[~big[inv]]] = nclasses                   # folded clusters become "unclassified" (:482,499)
            relabelled = True
        ids[pts] = comp_id[inv]
        ninst += nbig + (1 if new_small else 0)
    return np.arange(ninst), ids, info, classes


# ------------------------------------------------------------------------------------------------ CVSegmentation
class _Flood:
    """One f3d_flood_order pass: the compact form (order, offsets, flags, root) plus, on the host, each cluster's class."""

    def __init__(self, ctx, classes, adj, inst):
        n = len(classes)
        if on_device(classes):
            import torch
            offs, nbrs = adj
            dev = classes.device
            self.root = torch.empty(n, dtype=torch.int64, device=dev)
            order = torch.empty(n, dtype=torch.int64, device=dev)
            coffs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            flags = torch.zeros(n, dtype=torch.uint8, device=dev)
            with work_stream(dev) as work:                     # the call itself drains `work` (frontier readbacks)
                self.stats = ctx.flood_order_dev(classes.data_ptr(), n, offs.data_ptr(), nbrs.data_ptr(), inst, self.root.data_ptr(),
                                                 order.data_ptr(), coffs.data_ptr(), flags.data_ptr(), work.cuda_stream)
            m, L = self.stats['clusters'], self.stats['points']
            self.order, self.flags = order[:L], flags.bool()
            self.offsets = coffs[:m + 1]
            self.coffs = self.offsets.cpu().numpy()
            self.seed_class = classes[self.order[self.offsets[:-1]]].cpu().numpy() if m else np.zeros(0, np.int64)
        else:
            offs, nbrs = adj
            self.root, self.order, self.offsets, self.flags, self.stats = ctx.flood_order(classes, offs, nbrs, inst)
            self.coffs = self.offsets
            self.seed_class = classes[self.order[self.coffs[:-1]]]
        # clusters of one class are consecutive (numbered by class rank, then seed)
        self.ranges = {}
        sc = self.seed_class
        if len(sc):
            cut = np.flatnonzero(np.r_[True, sc[1:] != sc[:-1], True])
            for a, b in zip(cut[:-1], cut[1:]):
                self.ranges[int(sc[a])] = (int(a), int(b))

    def boundary(self, k, n):
        """length-n bool boundary of cluster k"""
        pts = self.order[self.coffs[k]:self.coffs[k + 1]]
        if on_device(self.order):
            import torch
            out = torch.zeros(n, dtype=torch.bool, device=self.order.device)
        else:
            out = np.zeros(n, bool)
        out[pts] = self.flags[pts]
        return out


class Boundaries(Sequence):
    """The boundaries instance_seperate returns, built when read: entry i is np.hstack of its records' length-N boundaries
    (None for a semantic record), exactly as merge_instances_by_classes stacks them; M * N bools are never held at once."""

    def __init__(self, groups, n):
        self._groups, self._n = groups, n

    def __len__(self):
        return len(self._groups)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        parts = [None if p is None else p[0].boundary(p[1], self._n) for p in self._groups[i]]
        if any(on_device(p) for p in parts) and all(p is not None for p in parts):
            import torch
            return torch.cat(parts)
        return np.hstack([p if p is None or not on_device(p) else p.cpu().numpy() for p in parts])


def _merge_plan(ids, idinfo, classes):
    """merge_instances_by_classes without the stacking: -> (ninstances, new id of every record id, out info, groups of record
    indices).  Records of a category in `classes` fold into that category's first record (areas summed in its dict)."""
    firsts = [None] * len(classes)
    out_info, groups, new_of = [], [], {}
    for k, rec in enumerate(idinfo):
        j = next((j for j, c in enumerate(classes) if rec['category_id'] == c), None)
        if j is not None and firsts[j] is not None:
            slot = firsts[j]
            out_info[slot]['area'] += rec['area']
            groups[slot].append(k)
        else:
            slot = len(out_info)
            if j is not None:
                firsts[j] = slot
            out_info.append(rec)
            groups.append([k])
        new_of[rec['id']] = slot
    return len(out_info), new_of, out_info, groups


def _remap(ids, new_of):
    """outids[ids == old] = new for every (old, new), on the original ids (ids without a record keep theirs)"""
    if not new_of:
        return ids.clone() if on_device(ids) else ids.copy()
    old = np.fromiter(new_of.keys(), np.int64, len(new_of))
    new = np.fromiter(new_of.values(), np.int64, len(new_of))
    if on_device(ids):
        import torch
        o = torch.as_tensor(old, device=ids.device)
        srt, perm = torch.sort(o)
        pos = torch.searchsorted(srt, ids).clamp_(max=len(old) - 1)
        hit = srt[pos] == ids
        return torch.where(hit, torch.as_tensor(new, device=ids.device)[perm[pos]].to(ids.dtype), ids)
    srt = np.argsort(old, kind='stable')
    pos = np.minimum(np.searchsorted(old[srt], ids), len(old) - 1)
    hit = old[srt][pos] == ids
    out = ids.copy()
    out[hit] = new[srt][pos][hit].astype(ids.dtype)
    return out


class CVSegmentation:
    def __init__(self, classes, adj):
        """classic segmentation algorithms on the GPU: classes [N] point classes (NumPy, or a device tensor with a device CSR
        adjacency), adj the neighbour lists (list of arrays, or a CSR pair as ``radius_adjacency(..., as_csr=True)`` returns)."""
        self.classes = classes
        self.adj = adj
        self.floods = []            # compact form of the last instance_seperate: one _Flood per flood pass

    def _csr(self, n):
        """(offsets int64 [n + 1], neighbours int32 [offsets[n]]), checked: the kernels read every row the offsets name."""
        if on_device(self.classes):
            return device_csr(self.adj, n, self.classes.device, 'CVSegmentation: device classes')
        return host_csr(*adjacency_to_csr(self.adj, n), n, CSR_ADJACENCY)

    @staticmethod
    def merge_classes(classes, source, destination):
        for fcls, tcls in zip(source, destination):           # sequential: chains apply
            classes[classes == fcls] = tcls
        return classes

    @staticmethod
    def get_semantic_object_ids(idinfo):
        semanticids = [d['id'] for d in idinfo if not d['isthing']]
        objectids = [d['id'] for d in idinfo if d['isthing']]
        return semanticids, objectids

    @staticmethod
    def get_objects(ids, objectids):
        if on_device(ids):
            import torch
            return torch.isin(ids, torch.as_tensor(list(objectids), dtype=ids.dtype, device=ids.device))
        return np.isin(ids, np.asarray(list(objectids), dtype=ids.dtype if len(objectids) else None))

    @staticmethod
    def get_classes(ids, idinfo):
        classes = ids.clone().zero_() if on_device(ids) else np.zeros_like(ids)
        for info in idinfo:                                      # the last matching record wins
            classes[ids == info['id']] = info['category_id']
        return classes

    @staticmethod
    def get_ids_by_classes(idinfo, classes):
        classids = [[] for _ in classes]
        for info in idinfo:
            for i, category in enumerate(classes):
                if category == info['category_id']:
                    classids[i].append(info['id'])
        return classids

    @staticmethod
    def merge_instances_by_classes(ids, idinfo, classes, clusters=None, boundaries=None):
        ninst, new_of, out_info, groups = _merge_plan(ids, idinfo, classes)
        outids = _remap(ids, new_of)
        outclusters = [np.hstack([clusters[k] for k in g]) for g in groups]
        outboundaries = [np.hstack([boundaries[k] for k in g]) for g in groups]
        return ninst + 1, outids, out_info, outclusters, outboundaries

    def instance_seperate(self, instance_classes=None, minimum_points=1):
        """-> (arange(M + 1), ids [N], info, clusters (pop order), boundaries); see the reference docstring (:309-324).
        self.classes is rewritten in place (small clusters become class 0), as in the reference.  The fifth value is a
        read-only sequence (``Boundaries``) rather than a list: entry i is built when it is read (indexing, slicing,
        iteration and len() work as on the reference's list; use list(...) for a mutable copy)."""
        dev = on_device(self.classes)
        classes = self.classes
        n = len(classes)
        adj = self._csr(n)
        ctx = f3d.default_context(classes.device.index) if dev else f3d.default_context()
        if dev:
            import torch
            if classes.dtype != torch.int64 or not classes.is_contiguous():
                raise TypeError('instance_seperate: device classes must be a contiguous int64 tensor (rewritten in place)')
            xp_cat = lambda a: torch.as_tensor(a, device=classes.device)                    # noqa: E731
            present = torch.unique(classes).cpu().numpy()
            ids = torch.zeros_like(classes)
        else:
            xp_cat = lambda a: a                                                           # noqa: E731
            present = np.unique(classes)
            ids = np.zeros_like(classes)
        info, clusters, parts = [], [], []
        if instance_classes is None:
            order, nid = present, 0
        else:
            order = np.array(instance_classes)
            for k, c in enumerate(np.setdiff1d(present, order)):
                mask = classes == int(c)
                ids[mask] = k
                pts = torch.nonzero(mask).reshape(-1) if dev else np.nonzero(mask)[0]
                info.append({'id': k, 'isthing': False, 'category_id': int(c), 'area': int(len(pts))})
                clusters.append(pts)
                parts.append(None)
            nid = len(info)
        self.floods = []
        seg, relabelled = None, False
        for pos, c in enumerate(order):
            c = int(c)
            if seg is None or (c == 0 and relabelled):          # clusters of class 0 grew by the relabelled ones: flood again
                seg = _Flood(ctx, classes, adj, np.asarray(order[pos:], np.int64))
                self.floods.append(seg)
                relabelled = False
            k0, k1 = seg.ranges.get(c, (0, 0))
            if k0 == k1:
                continue
            ks = np.arange(k0, k1)
            seeds = seg.order[xp_cat(seg.coffs[k0:k1])]
            now = classes[seeds]
            now = now.cpu().numpy() if dev else now
            ks = ks[now == c]                                   # a repeated class: clusters relabelled by its first turn are gone
            if not len(ks):
                continue
            sizes = seg.coffs[ks + 1] - seg.coffs[ks]
            new_ids = nid + np.arange(len(ks))
            small = sizes < minimum_points
            for k, i_, a, sm in zip(ks, new_ids, sizes, small):
                info.append({'id': int(i_), 'isthing': True, 'category_id': 0 if sm else c, 'area': int(a)})
                clusters.append(seg.order[int(seg.coffs[k]):int(seg.coffs[k + 1])])
                parts.append((seg, int(k)))
            nid += len(ks)
            # ids and the relabelling, over the class's clusters at once (they are consecutive in `order`)
            lo, hi = int(seg.coffs[k0]), int(seg.coffs[k1])
            all_sizes = seg.coffs[k0 + 1:k1 + 1] - seg.coffs[k0:k1]
            keep = np.zeros(k1 - k0, np.int64) - 1
            keep[ks - k0] = new_ids
            per_pt = np.repeat(keep, all_sizes)
            sm_pt = np.repeat(np.isin(np.arange(k0, k1), ks[small]), all_sizes)
            pts = seg.order[lo:hi]
            sel = per_pt >= 0
            ids[pts[xp_cat(sel)]] = xp_cat(per_pt[sel]).to(ids.dtype) if dev else per_pt[sel].astype(ids.dtype)
            if small.any() and c != 0:
                classes[pts[xp_cat(sm_pt)]] = 0
                relabelled = True
        ninst, new_of, out_info, groups = _merge_plan(ids, info, (0,))
        outids = _remap(ids, new_of)
        outclusters = []
        for g in groups:
            if len(g) == 1:
                outclusters.append(clusters[g[0]])
            elif dev:
                import torch
                outclusters.append(torch.cat([clusters[k] for k in g]))
            else:
                outclusters.append(np.hstack([clusters[k] for k in g]))
        bnd = Boundaries([[parts[k] for k in g] for g in groups], n)
        rng = np.arange(ninst + 1)
        return rng, outids, out_info, outclusters, bnd

    def color_segment(self, colors, ids, seeds, threshold, neutral_ids=(0, ), max_level=10):
        """-> ids, updated in place; see the reference docstring (:367-386).  Colours float64 or float32."""
        n = len(ids)
        if on_device(ids):
            import torch
            if colors.dtype not in (torch.float64, torch.float32):
                raise TypeError(f'color_segment: colours must be float64 or float32, got {colors.dtype}')
            if ids.dtype != torch.int64 or not ids.is_contiguous():
                raise TypeError('color_segment: device ids must be a contiguous int64 tensor (updated in place)')
            if not on_device(colors) or colors.device != ids.device or tuple(colors.shape) != (n, 3):
                raise ValueError(f'color_segment: colours must be a [{n}, 3] tensor on {ids.device}')
            offs, nbrs = self._csr(n)
            sd = torch.as_tensor(seeds, dtype=torch.int64, device=ids.device).reshape(-1)
            sd = torch.where(sd < 0, sd + n, sd).contiguous()  # NumPy's negative indices; the kernel rejects the rest (IndexError)
            clr = colors.contiguous()
            ctx = f3d.default_context(ids.device.index)
            with work_stream(ids.device) as work:
                ctx.color_segment_dev(clr.data_ptr(), dtype_code(clr), n, offs.data_ptr(),
                                      nbrs.data_ptr(), ids.data_ptr(), sd.data_ptr(), len(sd), threshold, neutral_ids, max_level, None,
                                      work.cuda_stream)
                ctx.take_device_error(work.cuda_stream)
            return ids
        clr = np.asarray(colors)
        if clr.dtype not in (np.float64, np.float32):
            raise TypeError(f'color_segment: colours must be float64 or float32, got {clr.dtype}')
        offs, nbrs = self._csr(n)
        sd = np.asarray(seeds, dtype=np.int64).reshape(-1)
        sd = np.where(sd < 0, sd + n, sd)                       # NumPy's negative indices
        if len(sd) and (sd.min() < 0 or sd.max() >= n):
            raise IndexError(f'color_segment: seed index out of bounds for {n} points')
        work = ids if (ids.dtype == np.int64 and ids.flags.c_contiguous) else np.ascontiguousarray(ids, dtype=np.int64)
        f3d.default_context().color_segment(clr, offs, nbrs, work, sd, threshold, neutral_ids, max_level)
        if work is not ids:
            ids[...] = work
        return ids
