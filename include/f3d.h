/*
 * f3d.h -- C-ABI of libf3d_hip.so: the MI355X (gfx950) implementation of the Fusion3DSeg hot
 * path (per-point pinhole projection + frustum visibility, multi-view mask sampling and label
 * voting/argmax, oriented-box membership/merge support).
 *
 * The reference is pure Python/NumPy and has no FFI; the boundary is its Python call surface
 * (SURVEY.md 8(b)).  Each entry point below names the reference function (file:line, relative
 * to the reference repository) whose arithmetic it replaces; INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add at each call site.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / numpy types.
 *   - every function returns F3D_OK (0) or a negative f3d_status; the text of the last error
 *     of a context is available from f3d_last_error().
 *   - functions without a "_dev" suffix take HOST pointers: inputs are copied to the device
 *     through the context's staging buffers, the kernels run on the context's stream, outputs are
 *     copied back, and the call returns after the stream has drained (NumPy drop-in).  Staging is
 *     separate from the scratch of the _dev functions and holds nothing once a call has returned.
 *     Four host-pointer sequences keep data on the device between their calls, in buffers of their
 *     own: f3d_radius_graph_count -> _fill, f3d_radius_query_count -> _fill, f3d_tsdf_extract_count -> _fill
 *     and f3d_group_by_id -> f3d_obb_extremes -> f3d_obb_hull_filter.  Any other call on the context may come in between;
 *     a sequence ends where its first call is made again.  Staging and these buffers grow on first
 *     use like scratch (and a strict context refuses that); f3d_ctx_reserve*() does not size them.
 *   - "_dev" functions take DEVICE pointers and a hipStream_t (as void*; NULL = the context's
 *     own stream).  They only enqueue work and never synchronise.  Scratch (sort keys, coded masks,
 *     the deferred-point list, the vote table) lives in the context and GROWS ON FIRST USE of a larger
 *     problem (hipMalloc, not capturable); size it beforehand with f3d_ctx_reserve() (and its
 *     f3d_ctx_reserve_*() kin: they cover the scratch of _dev calls only) and a _dev call
 *     of that or a smaller size performs no allocation at all (hipGraph-safe).  With
 *     f3d_ctx_set_strict(ctx, 1) a call that would have to grow scratch fails with F3D_ERR_NOMEM instead.
 *   - the caller owns every buffer; the library keeps no caller pointer after a call returns
 *     (host variants) / after the enqueued work has completed (_dev variants).
 *   - a context is not thread-safe; use one per thread.  There is no global state.
 *   - quaternions are (w, x, y, z) float64 and are NOT assumed to be normalised (quirk Q4).
 *   - the library has no CPU fallback: without a HIP device every compute entry point fails
 *     with F3D_ERR_HIP.
 */
#ifndef F3D_H
#define F3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define F3D_VERSION 100           /* 0.1.0 */
#define F3D_MAX_FILTER 512        /* longest filter_classes list accepted */
#define F3D_NPLANES 5             /* 4 frustum side planes + far plane (fusion.py:254-258) */

typedef enum f3d_status {
    F3D_OK = 0,
    F3D_ERR_INVALID = -1,         /* bad argument (NULL, negative size, unsupported combination)  */
    F3D_ERR_HIP = -2,             /* HIP runtime error / no device / extension not usable         */
    F3D_ERR_INDEX = -3,           /* reference raises IndexError (voting.py:98): label or point id
                                     out of range                                                 */
    F3D_ERR_ZERO_QUAT = -4,       /* reference raises ZeroDivisionError (pyquaternion inverse)    */
    F3D_ERR_NOMEM = -5
} f3d_status;

typedef enum f3d_dtype {
    F3D_F64 = 0,                  /* xyz stored as float64 [N,3] row-major (the reference layout) */
    F3D_F32 = 1                   /* xyz stored as float32 [N,3]; widened to f64 in registers     */
} f3d_dtype;

/* One camera view, in the form the kernels consume (8-byte aligned, 704 bytes = 88 doubles).
 * Built on the host by f3d_views_build(); the fused kernel reads it through scalar loads and
 * stages the float32 cull planes in LDS.
 *   exact data (the reference's arithmetic uses exactly these):  K, qinv, t, plane_pt, plane_n
 *   accelerators (never decide a result on their own, see DESIGN.md "fast paths"):
 *     M, mnorm      : M = K * Rot(qinv) rounded once from extended precision; mnorm[k] bounds the
 *                     row-k operand magnitudes.  The fast projection h = M (p - t) is accepted only
 *                     when its floor provably equals the canonical path's; otherwise the canonical
 *                     arithmetic (camera_utils.py:21-25 order) is evaluated.
 *     cull_*32      : float32 copy of the planes, a = n32 . p32 - off32; a point (or a whole tile's
 *                     bounding box) is accepted/rejected without the exact plane test only when |a|
 *                     exceeds rel32 * (|x|+|y|+|z|) + abs32.
 *     M32           : (float)M, the operator of the float32 "centre + offset" projection: one lane per view
 *                     projects the centre c of a wavefront's bounding box with M in float64, every lane then
 *                     only needs the float32 offset term M32 (p - c); accepted when farther than a rigorous
 *                     bound from a pixel border, otherwise the point goes to the exact kernel. */
typedef struct f3d_view {
    /* hot (128 B = two scalar-cache lines): everything the fast projection reads */
    double M[9];                  /* K * Rot(qinv), row-major                                     */
    double t[3];                  /* camera translation       (camera_utils.py:21)                */
    double mnorm[3];              /* ||K row k||_1 * |qinv|^2, rounded up                          */
    double pad0;
    /* warm (128 B): float32 planes of the pre-culls */
    float  cull_n32[F3D_NPLANES][3];
    float  cull_off32[F3D_NPLANES];
    float  cull_rel32;
    float  cull_abs32;
    float  img_w;                 /* the image the frustum planes were built for (f3d_views_build's w, h)         */
    float  img_h;
    double cull_rel64;            /* float64 refinement of the point cull (middle tier):                          */
    double cull_abs64;            /* a = n . p - plane_off in FMAs; |a| <= rel64 * |p|_1 + abs64 -> exact kernel   */
    float  pad1[4];
    float  M32[9];                /* (float)M[k]                                                                  */
    float  pad2[7];
    /* exact data: what the reference's arithmetic uses */
    double K[9];                  /* intrinsics, row-major (camera_utils.py:23)                   */
    double qinv[4];               /* conj(q)/|q|^2 (w,x,y,z)  (camera_utils.py:22)                */
    double plane_pt[F3D_NPLANES][3];   /* fusion.py:254-257                                       */
    double plane_n[F3D_NPLANES][3];    /* inward normals, fusion.py:256-258                       */
    double plane_off[F3D_NPLANES];     /* n . plane_pt (only for the float64 cull refinement)      */
} f3d_view;

/* An oriented box as open3d's OrientedBoundingBox exposes it (center, R columns = axes, extent);
 * merge_intersecting_bb.py:75-76. */
typedef struct f3d_obb {
    double center[3];
    double R[9];                  /* row-major 3x3, column i = axis i                             */
    double extent[3];
} f3d_obb;

typedef struct f3d_ctx f3d_ctx;

/* ---- context ---------------------------------------------------------------------------- */
int         f3d_version(void);
f3d_ctx*    f3d_ctx_create(int device);            /* NULL on failure (no device, HIP error)      */
void        f3d_ctx_destroy(f3d_ctx* ctx);
const char* f3d_last_error(const f3d_ctx* ctx);    /* ctx may be NULL: last creation error        */
int         f3d_ctx_synchronize(f3d_ctx* ctx);
void*       f3d_ctx_stream(f3d_ctx* ctx);          /* the context's hipStream_t                   */
/* Sizes the context's scratch for f3d_project_vote_argmax_dev / f3d_cloud_sort_cells_dev on up to n points, nviews
 * masks of h x w pixels, and for f3d_vote_uv2pt_dev frames of h*w pixels (any argument may be 0 to skip its part). */
int         f3d_ctx_reserve(f3d_ctx* ctx, int64_t n, int nviews, int h, int w);
/* strict = 1: scratch never grows inside a call; a too-small buffer is F3D_ERR_NOMEM (reserve first). */
int         f3d_ctx_set_strict(f3d_ctx* ctx, int strict);
/* Number of device allocations this context has made so far (diagnostic: unchanged across an allocation-free call). */
long long   f3d_ctx_alloc_count(const f3d_ctx* ctx);

/* ---- host-side geometry (tiny, per view; no device needed) ------------------------------ */
/* pyquaternion Quaternion(q).inverse.elements at camera_utils.py:22 */
int f3d_quat_inverse(const double q_wxyz[4], double qinv_wxyz[4]);
/* Fusion._get_frustum_data (fusion.py:119-132; camera_utils.py:60-171), frame_ids = all.
 * eyes [V,3], lookats [V,3], face_normals [V,4,3]; any output may be NULL. */
int f3d_frustum_data(const double K[9], double w, double h, const double* q_wxyz /*[V,4]*/,
                     const double* t /*[V,3]*/, int nviews,
                     double* eyes, double* lookats, double* face_normals);
/* The packed per-view records: K, inverse pose, and the 5 planes Fusion.fuse builds per frame
 * (fusion.py:254-258) with far plane at eye + max_depth * lookat. */
int f3d_views_build(const double K[9], double w, double h, const double* q_wxyz, const double* t,
                    int nviews, double max_depth, f3d_view* out /*[V]*/);

/* ---- a1: SpatQuadranion.rotate (RTAB_utils/spatQuad.py:7-28) ----------------------------- */
int f3d_rotate_f64(f3d_ctx* ctx, const double* xyz, int64_t n, const double q_wxyz[4], double* out);
/* device pointers (out may not alias xyz), enqueue only; the quaternion is read on the host at call time */
int f3d_rotate_f64_dev(f3d_ctx* ctx, const double* xyz, int64_t n, const double q_wxyz[4], double* out, void* stream);

/* ---- a2: points2pixel (Fusion3DSeg/camera_utils.py:9-26) -> int32 uv[2*n], row 0 = u ------ */
int f3d_points2pixel_f64(f3d_ctx* ctx, const double* xyz, int64_t n, const double K[9],
                         const double q_wxyz[4], const double t[3], int32_t* uv);
int f3d_points2pixel_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n,
                         const double K[9], const double q_wxyz[4], const double t[3],
                         int32_t* uv, void* stream);

/* ---- a4: point_inside_polyhedra (Fusion3DSeg/intersections.py:146-164) -> uint8 inside[n] - */
int f3d_inside_polyhedra_f64(f3d_ctx* ctx, const double* xyz, int64_t n, const double* plane_pts,
                             const double* normals, int m, uint8_t* inside);
int f3d_inside_polyhedra_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n,
                             const double* plane_pts /*host [m,3]*/, const double* normals /*host*/,
                             int m, uint8_t* inside, void* stream);

/* ---- a2+a4 fused for one view: the per-frame body of Fusion.fuse (fusion.py:254-266) ------ */
/* uv is written for every point (like points2pixel), inside as a4. */
int f3d_project_view_f64(f3d_ctx* ctx, const double* xyz, int64_t n, const f3d_view* view /*host*/,
                         int32_t* uv, uint8_t* inside);
int f3d_project_view_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n,
                         const f3d_view* view /*host*/, int32_t* uv, uint8_t* inside, void* stream);

/* ---- fused multi-view path: project -> sample -> vote -> segment ------------------------- */
/* For every point and view: inside (a4) -> uv (a2) -> drop u not in [0,W) or v not in [0,H) ->
 * label = masks[v][row][col] -> one vote; then VotingSegmentation.segment (voting.py:106-137)
 * with `nclasses`, `threshold`, optional `filter` (NULL / 0 = none).
 * classes: int64 [n].  votes_u16 (optional, may be NULL): uint16 [n, nclasses+1] vote counts,
 * equal to the reference's float64 votes matrix on this path.
 * Labels > nclasses make the reference raise IndexError -> F3D_ERR_INDEX (host variant; the
 * _dev variant records it, fetch with f3d_take_device_error after synchronising). */
int f3d_project_vote_argmax(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n,
                            const f3d_view* views, int nviews,
                            const uint8_t* masks /*[V,H,W]*/, int h, int w,
                            int nclasses, const int32_t* filter, int nfilter, double threshold,
                            int64_t* classes, uint16_t* votes_u16);
/* flags for the device variant (results never depend on them):
 *   F3D_FUSE_SORT     the cloud is in arbitrary order: cell-sort it inside the call (into context
 *                     scratch, ~4 HBM passes over xyz) so that a wavefront's 64 points are spatial
 *                     neighbours and culled waves skip the projection; labels are written back in the
 *                     caller's order.  `perm` must be NULL.
 *   F3D_FUSE_GATHER   with `perm`: xyz is still the caller-order cloud and the kernel reads point
 *                     perm[i] (what F3D_FUSE_SORT does internally; lets a caller time / reuse the sort).
 * Every call first finds the labels that occur in the masks and copies the masks into context scratch as 8x8-pixel
 * tiles (one cache line each) of vote-bin codes -- two passes over V*H*W bytes; the 1-byte gathers of neighbouring
 * points then share lines in both image directions, and a thread's vote histogram only has bins for labels that
 * exist.  With nclasses > 253 (no byte left for the "no sample" and "rejected label" codes) the accelerated kernel
 * is skipped and the reference-arithmetic kernel labels every point.
 * perm (device, may be NULL): perm[i] is the caller-order index of the i-th point in cell order
 * (from f3d_cloud_sort_cells_dev); without F3D_FUSE_GATHER xyz must be the sorted copy.
 * classes/votes are always written at caller-order indices. */
#define F3D_FUSE_SORT    2u
#define F3D_FUSE_GATHER  4u
int f3d_project_vote_argmax_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n,
                                const f3d_view* views_dev /*device [V]*/, int nviews,
                                const uint8_t* masks, int h, int w,
                                int nclasses, const int32_t* filter /*host*/, int nfilter,
                                double threshold, int64_t* classes, uint16_t* votes_u16,
                                unsigned flags, const int32_t* perm, void* stream);
/* The same path with the views arriving in CHUNKS (with the masks sharded by view over the ranks, the
 * all-gather of view chunk c+1 is in flight while chunk c votes).  Same results as one f3d_project_vote_argmax_dev call
 * over all views (votes are a sum over views: order-free), at most 255 views in total, no vote output.
 *   f3d_mask_presence_dev      labels that occur in `nviews` masks -> present256 (device, 256 bytes of 0 / 1).  Ranks
 *                              combine theirs with an all-reduce MAX (the vote-bin code book must be the same on every
 *                              rank and for every chunk, before any mask of another rank has arrived).
 *   f3d_fuse_chunked_begin_dev builds the code book from the combined presence (NULL: every label 0..nclasses gets a
 *                              bin -- no exchange, larger histograms) or from `filter`, and sizes ALL scratch of the
 *                              chunk calls (coded masks of nviews views, the deferred lists, and the per-point vote
 *                              state between chunks: f3d "carry", 4 * ceil((nclasses + 3) / 4) bytes per point, 8-bit
 *                              bins in context scratch in HBM).
 *   f3d_fuse_chunk_dev         views [v_begin, v_end): codes those planes of `masks` and lets every point vote on them.
 *                              Chunks must follow each other without gaps from 0 to nviews, with the same xyz / n /
 *                              views_dev / masks base pointer / h / w / nclasses / filter / threshold; flags and perm
 *                              are taken from the first chunk.  masks[v] must be complete for the chunk's views when the
 *                              call is enqueued on `stream` and for ALL views at the last chunk (the float64 tier and the
 *                              reference-arithmetic kernel run there, over every view).  classes is written by the last
 *                              chunk only.  F3D_ERR_INVALID for a chunk out of sequence. */
int f3d_mask_presence_dev(f3d_ctx* ctx, const uint8_t* masks, int nviews, int h, int w, uint8_t* present256, void* stream);
int f3d_fuse_chunked_begin_dev(f3d_ctx* ctx, const uint8_t* present256, int64_t n, int nviews, int h, int w, int nclasses,
                               const int32_t* filter /*host*/, int nfilter, void* stream);
int f3d_fuse_chunk_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views_dev, int nviews,
                       int v_begin, int v_end, const uint8_t* masks /*[nviews,H,W]*/, int h, int w, int nclasses,
                       const int32_t* filter /*host*/, int nfilter, double threshold, int64_t* classes,
                       unsigned flags, const int32_t* perm, void* stream);
/* The same with the mask CODING sharded as well: a rank codes only the masks it produced -- with the book of
 * f3d_fuse_chunked_begin_dev, identical on every rank -- and the ranks all-gather CODED planes (f3d_coded_plane_bytes(h, w) each:
 * 8 x 8-pixel tiles of vote-bin codes with a one-tile border; ~3 % more bytes than the raw plane).
 *   f3d_code_planes_dev        `nplanes` raw masks -> `coded` (nplanes x f3d_coded_plane_bytes, 8-byte aligned), enqueue only.
 *   f3d_fuse_chunk_coded_dev   like f3d_fuse_chunk_dev, but `coded` = the gather buffer of coded planes, [nviews] planes in the
 *                              order of views_dev, read where they lie.  No raw mask ever reaches this rank, so the last
 *                              tier runs the reference's arithmetic on the coded planes. */
size_t f3d_coded_plane_bytes(int h, int w);
int f3d_code_planes_dev(f3d_ctx* ctx, const uint8_t* masks, int nplanes, int h, int w, uint8_t* coded, void* stream);
int f3d_fuse_chunk_coded_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views_dev, int nviews,
                             int v_begin, int v_end, const uint8_t* coded /*[nviews] coded planes*/, int h, int w,
                             int nclasses, const int32_t* filter /*host*/, int nfilter, double threshold, int64_t* classes,
                             unsigned flags, const int32_t* perm, void* stream);
/* Test hook: cell-sorts the cloud and evaluates, for every (point, view) pair, the accelerated decisions of the
 * fused kernel (wave-box and per-point float32 culls, centre + offset projection for a w x h image) next to the exact
 * arithmetic.  stats[0] = pairs inside the frustum, stats[1] = pairs the offset projection leaves to the exact
 * kernel, stats[2] = decided pairs whose pixel differs from the canonical path (must be 0), stats[3] = float32 cull
 * decisions the exact plane test contradicts (must be 0).  Host pointers. */
int f3d_debug_fastpath_audit(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n,
                             const f3d_view* views, int nviews, int w, int h, uint64_t stats[4]);
/* Diagnostic: how many points of the last fused call of this context the float32 kernel handed to the float64 middle
 * tier (counts[0]) and how many of those needed the reference's own arithmetic for at least one view (counts[1]).
 * Synchronises `stream`. */
int f3d_debug_fuse_deferred(f3d_ctx* ctx, void* stream, uint32_t counts[2]);
/* Diagnostic: how many wave-tiles (128 points) of the last fused call of this context left their view loops early because
 * every point of the tile was already decided "unlabelled".  Synchronises `stream`. */
int f3d_debug_fuse_decided(f3d_ctx* ctx, void* stream, uint32_t* count);
/* Sort of the cloud by coarse grid cell: perm (int32 [n], caller-order index of sorted point i)
 * and, unless NULL, sorted_xyz (same dtype/size as xyz); device buffers owned by the caller. */
int f3d_cloud_sort_cells_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n,
                             void* sorted_xyz, int32_t* perm, void* stream);
/* Returns and clears the sticky error recorded by _dev kernels of this context (F3D_OK or F3D_ERR_INDEX; the
 * message names the operation that recorded it: each operation owns one bit of the word, and the host-pointer
 * variants consume only their own).  Synchronises `stream`. */
int f3d_take_device_error(f3d_ctx* ctx, void* stream);

/* ---- a7: one frame of VotingSegmentation.vote (voting.py:94-98) --------------------------- */
/* votes[uv2pt[i], mask[i]] += 1 for uv2pt[i] != -1, each distinct (point,label) pair of the
 * frame counted once (quirk Q1).  votes: float64 [npts, ncols], updated in place. */
int f3d_vote_uv2pt(f3d_ctx* ctx, const int32_t* uv2pt, const uint8_t* mask, int64_t hw,
                   double* votes, int64_t npts, int ncols);
int f3d_vote_uv2pt_dev(f3d_ctx* ctx, const int32_t* uv2pt, const uint8_t* mask, int64_t hw,
                       double* votes, int64_t npts, int ncols, void* stream);

/* The whole loop of VotingSegmentation.vote (voting.py:88-98) for F frames of h x w pixels in one call: luts int32 [F, h*w],
 * masks uint8 [F, h*w] (already at the lookup's resolution).  Same result as F calls of f3d_vote_uv2pt in frame order, incl.
 * the IndexError semantics: the frames before the first offending one are applied, it and the later ones are not
 * (F3D_ERR_INDEX from the host variant; the _dev variant records it for f3d_take_device_error).  One launch pair per 2^25
 * lookups; duplicates die in an LDS set per 32 x 32 tile, the global set is generation-stamped and never cleared. */
int f3d_vote_uv2pt_batch(f3d_ctx* ctx, const int32_t* luts, const uint8_t* masks, int64_t nframes, int h, int w,
                         double* votes, int64_t npts, int ncols);
int f3d_vote_uv2pt_batch_dev(f3d_ctx* ctx, const int32_t* luts, const uint8_t* masks, int64_t nframes, int h, int w,
                             double* votes, int64_t npts, int ncols, void* stream);

/* ---- a8: VotingSegmentation.segment (voting.py:106-137) ----------------------------------- */
int f3d_segment_votes(f3d_ctx* ctx, const double* votes, int64_t npts, int ncols, int nclasses,
                      double threshold, const int32_t* filter, int nfilter, int64_t* classes);
int f3d_segment_votes_dev(f3d_ctx* ctx, const double* votes, int64_t npts, int ncols, int nclasses,
                          double threshold, const int32_t* filter /*host*/, int nfilter,
                          int64_t* classes, void* stream);

/* ---- PointVotingSegmentation.segment (voting.py:267-299) ---------------------------------- */
/* As f3d_segment_votes (first-maximum argmax, `nclasses` for no votes / max/total < threshold / a zero maximum, the sequential
 * index -> class remap with its aliasing), with the two differences of that class: the total of a row is its LAST COLUMN, not
 * its sum, and without a filter the candidates are the columns before the last one.  A negative filter entry reads the column
 * NumPy's index wraps to and is written to `classes` as given (the reference stores the list's value).  ncols == 1 without a filter ->
 * F3D_ERR_INVALID (NumPy: argmax of an empty sequence). */
int f3d_segment_votes_lastcol(f3d_ctx* ctx, const double* votes, int64_t npts, int ncols, int nclasses,
                              double threshold, const int32_t* filter, int nfilter, int64_t* classes);
int f3d_segment_votes_lastcol_dev(f3d_ctx* ctx, const double* votes, int64_t npts, int ncols, int nclasses,
                                  double threshold, const int32_t* filter /*host*/, int nfilter,
                                  int64_t* classes, void* stream);

/* ---- a9: mask post-processing of SegmentImage (get2DSeg.py:110-118) ----------------------- */
/* sem: float32 [c, hw] logits -> uint8 mask[hw]: argmax over c; softmax max < conf -> `low`. */
int f3d_sem_logits_to_mask(f3d_ctx* ctx, const float* sem, int c, int64_t hw, float conf_threshold,
                           int low_label, uint8_t* mask);
int f3d_sem_logits_to_mask_dev(f3d_ctx* ctx, const float* sem, int c, int64_t hw,
                               float conf_threshold, int low_label, uint8_t* mask, void* stream);
/* The device-resident 2D -> 3D hand-off (SegmentImage's loop, get2DSeg.py:106-126, without the PNG round trip): `nimg` images of
 * logits, float32 [nimg, c, hw], become `nimg` consecutive planes of the caller's uint8 [V, H, W] mask tensor (masks = its base
 * + first_plane * hw) -- the tensor f3d_project_vote_argmax_dev reads.  One launch, enqueued on `stream`; no synchronisation and
 * no copy to the host. */
int f3d_sem_logits_to_masks_dev(f3d_ctx* ctx, const float* sem, int nimg, int c, int64_t hw,
                                float conf_threshold, int low_label, uint8_t* masks, void* stream);

/* ---- a10/a11: oriented-box membership for merge_bb (merge_intersecting_bb.py:64-91) ------- */
/* inside_bits: uint32 [n, ceil(b/32)] -- bit k of word j of point i set iff point i lies in box
 * 32*j+k (|Rt(p-c)|_a <= extent_a/2, a = 0..2).  cooc (optional): uint8 [b,b], cooc[i][j] = 1 iff
 * some point lies in both boxes i and j ("index lists share an element", :64-66,88-90). */
int f3d_points_in_obb(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n,
                      const f3d_obb* boxes, int b, uint32_t* inside_bits, uint8_t* cooc);
int f3d_points_in_obb_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n,
                          const f3d_obb* boxes /*host*/, int b, uint32_t* inside_bits,
                          uint8_t* cooc /*device, zeroed by the call*/, void* stream);
/* update_id_info's relabel (merge_intersecting_bb.py:59-61): ids[ids == from] = to; returns the
 * number of relabelled points through *count (may be NULL). */
int f3d_relabel(f3d_ctx* ctx, int64_t* ids, int64_t n, int64_t from, int64_t to, int64_t* count);
int f3d_relabel_dev(f3d_ctx* ctx, int64_t* ids, int64_t n, int64_t from, int64_t to,
                    int64_t* count_dev, void* stream);

/* ---- a10/a11: per-instance point lists and hull candidates for the oriented-box fits of merge_bb -------- */
/* The reference builds points[ids == id] for every instance (merge_intersecting_bb.py:72-74,81-82,124-125; get3DSeg.py:434)
 * and fits a box on it (Open3D: convex hull -> PCA of the hull vertices).
 * f3d_group_by_id: stable grouping of the point indices by id.  order int32 [n] lists the members of id 0, then id 1, ...
 * (ids outside [0, nids) last), each in ascending point index; starts int64 [nids + 2]: id k owns
 * order[starts[k] .. starts[k + 1]), starts[nids + 1] = n.  sorted_ids (device variant) uint32 [n] = the id of every position.
 * f3d_obb_extremes: extremes int32 [nids, 26] = for every id the member that is extreme along +-x, +-y, +-z and the 10 face /
 * body diagonals (float32 dot products; -1 for an id without members).
 * f3d_obb_hull_filter: with the facets (n . p + o <= 0 inside; double [F, 4], facet_start int32 [nids + 1] per id) of a convex
 * polytope spanned by MEMBERS of the id (e.g. the hull of its <= 26 extremes), drops every member strictly inside it by more
 * than margin[id]: such a point is interior to the hull of all members, so hull and box of the survivors are those of the
 * whole instance.  cand int32 [n]: the survivors of id k at cand[starts[k] ..], cand_count[k] of them, in no particular order.
 * The host-pointer variants form a sequence (group -> extremes -> hull_filter); the grouping and the cloud stay in the context. */
int f3d_group_by_id(f3d_ctx* ctx, const int64_t* ids, int64_t n, int64_t nids, int32_t* order, int64_t* starts);
int f3d_obb_extremes(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, int32_t* extremes);
int f3d_obb_hull_filter(f3d_ctx* ctx, int64_t n, const int32_t* facet_start, const double* facets, const double* margin,
                        int32_t* cand, int32_t* cand_count);
int f3d_group_by_id_dev(f3d_ctx* ctx, const int64_t* ids, int64_t n, int64_t nids, int32_t* order, uint32_t* sorted_ids,
                        int64_t* starts, void* stream);
int f3d_obb_extremes_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const int32_t* order,
                         const uint32_t* sorted_ids, int64_t nids, int32_t* extremes, void* stream);
int f3d_obb_hull_filter_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const int32_t* order,
                            const uint32_t* sorted_ids, const int64_t* starts, int64_t nids, const int32_t* facet_start,
                            const double* facets, const double* margin, int32_t* cand, int32_t* cand_count, void* stream);

/* ---- a11: the oriented-box fit itself (Open3D's OrientedBoundingBox.create_from_points at merge_intersecting_bb.py:75,86,126 and
 * get3DSeg.py:434-435): convex hull -> mean / covariance of the hull vertices -> eigenvectors by descending eigenvalue, third axis =
 * first x second -> extents of the hull vertices in that frame.  One wavefront per instance: hull vertex set by gift wrapping with
 * CERTIFIED orientation signs (float64 + static error bound), cyclic Jacobi for the 3 x 3 eigen-problem.
 * pts: float64 [total, 3], the instances' points back to back (a superset of each hull's vertices is enough: f3d_obb_candidates_dev);
 * start int64 [nfit + 1]: instance k owns pts[start[k] .. start[k + 1]).  boxes: f3d_obb [nfit] (center, R row-major with the axes
 * as columns, extent).  status int32 [nfit]: F3D_OBB_OK; F3D_OBB_FEW = fewer than 4 points; F3D_OBB_DEFERRED = a sign could not be
 * certified (coplanar / duplicate points, non-finite coordinates, a facet with more than 3 vertices) or the frontier outgrew its
 * LDS table -- nothing is guessed, the caller fits that instance on the host (Qhull raises for the truly flat ones, like Open3D).
 * isvert (optional) uint8 [total]: 1 for the hull vertices.  nvert (optional) int32 [nfit].
 * Axis signs: the largest component of the first two axes is positive (the box as a point set does not depend on them; LAPACK /
 * Eigen do not specify theirs).  Open3D itself is absent from the build image: parity with it is unpinned. */
#define F3D_OBB_OK 0
#define F3D_OBB_FEW 1
#define F3D_OBB_DEFERRED 2
int f3d_obb_fit(f3d_ctx* ctx, const double* pts, const int64_t* start, int nfit, double* boxes, int32_t* status,
                uint8_t* isvert, int32_t* nvert);
int f3d_obb_fit_dev(f3d_ctx* ctx, const double* pts, const int64_t* start, int nfit, int64_t total /* = start[nfit] */,
                    double* boxes, int32_t* status, uint8_t* isvert /*device, required*/, int32_t* nvert, void* stream);
/* Hull candidates of EVERY instance in device passes (follows f3d_group_by_id_dev of the same cloud): directional extremes ->
 * hulls of the <= 26 extremes on the device (the same certified wave code) -> members strictly inside that inner polytope are
 * dropped -> the survivors compacted in ascending point index.  cand int32 [n] (capacity): the candidates of id 0, id 1, ... back to
 * back; cand_start int64 [nids + 1].  Instances with fewer than min_members members, or whose inner hull cannot be certified, keep
 * every member.  The hull -- hence the box -- of an instance's candidates is that of all of its members. */
int f3d_obb_candidates_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const int32_t* order,
                           const uint32_t* sorted_ids, const int64_t* starts, int64_t nids, int min_members,
                           int32_t* cand, int64_t* cand_start, void* stream);
/* out[j] = (double) xyz[idx[j]], j < count: the compact point array f3d_obb_fit_dev reads */
int f3d_gather_points_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, const int32_t* idx, int64_t count, double* out,
                          void* stream);

/* ---- a12 / (f)#4: the other primitives of Fusion3DSeg/intersections.py (host pointers) ---- */
/* ray_x_lines (:6-38): points [n,3], within uint8 [n] */
int f3d_ray_x_lines(f3d_ctx* ctx, const double origin[3], const double direction[3], const double* starts,
                    const double* ends, int64_t n, double* points, uint8_t* within);
/* rays_x_plane (:41-63): points [n,3], valid uint8 [n] */
int f3d_rays_x_plane(f3d_ctx* ctx, const double plane_point[3], const double plane_normal[3], const double* origins,
                     const double* directions, int64_t n, double* points, uint8_t* valid);
/* lines_x_planes (:66-94): points [n,m,3], valid uint8 [n,m].  The reference subtracts [n,3] from [n,m,3] without
 * a new axis (:89-90): it only broadcasts for n == 1 or n == m (then the segment test uses line m); any other
 * shape is F3D_ERR_INVALID, where NumPy raises ValueError. */
int f3d_lines_x_planes(f3d_ctx* ctx, const double* line_origins, const double* line_ends, int64_t n,
                       const double* plane_points, const double* plane_normals, int m, double* points, uint8_t* valid);
/* point_inside_polygon (:97-119): inside uint8 [n], within uint8 [m,n] */
int f3d_point_inside_polygon(f3d_ctx* ctx, const double* points, int64_t n, const double* vertices, int m,
                             uint8_t* inside, uint8_t* within);
/* points_plane_projection (:167-180): out [n,3] */
int f3d_points_plane_projection(f3d_ctx* ctx, const double* points, int64_t n, const double plane_point[3],
                                const double normal[3], double* out);
/* lines_plane_projection (:183-204): start / end projections and unit directions, each [n,3] */
int f3d_lines_plane_projection(f3d_ctx* ctx, const double* starts, const double* ends, int64_t n,
                               const double plane_point[3], const double normal[3], double* start_proj,
                               double* end_proj, double* directions);

/* ---- (f)#1: flood fill of split_into_instances (Fusion3DSeg/segUtils/cv.py:425-440) ------ */
/* Connected components of the adjacency (CSR: offsets int64 [n+1], neighbours int32 [offsets[n]]) restricted to
 * edges whose end points have the same class; root[i] = smallest point index of i's component (= the seed the
 * reference's "lowest remaining index" rule picks).  The adjacency must be symmetric, as KDTree.query_radius
 * (fusion.py:369-377) produces it.  A neighbour index outside [0, n) -> F3D_ERR_INDEX. */
int f3d_components_same_class(f3d_ctx* ctx, const int64_t* classes, int64_t n, const int64_t* offsets,
                              const int32_t* neighbours, int64_t* root);
int f3d_components_same_class_dev(f3d_ctx* ctx, const int64_t* classes, int64_t n, const int64_t* offsets,
                                  const int32_t* neighbours, int32_t* parent_scratch /*int32 [n]*/, int64_t* root,
                                  void* stream);

/* ---- CVSegmentation.instance_seperate: ordered same-class flood (Fusion3DSeg/segUtils/cv.py:52-89, 309-365) ---- */
/* The clusters (same-class connected components) of the classes inst[0..ninst) (HOST array, processing order; a repeated
 * class counts at its first position), numbered by the rank of their class in that list, then by ascending seed (= smallest
 * index), are concatenated in the reference's FIFO pop order:
 *   root    int64 [n]    : smallest index of the point's component (as f3d_components_same_class)
 *   order   int64 [n]    : order[coffs[c] .. coffs[c+1]) = cluster c in pop order; entries past stats[1] are -1
 *   coffs   int64 [n+1]  : cluster offsets, stats[0] + 1 of them used
 *   flags   uint8 [n]    : 1 = boundary point of its cluster (the reference's boundary[parents[q]] for a popped
 *                          different-class neighbour q); a cluster's boundary is flags restricted to its points
 *   stats   int64 [4]    : HOST, {clusters, points in clusters, BFS levels, frontier readbacks}
 * Preconditions: symmetric rows without duplicate entries, which is what KDTree.query_radius and f3d_radius_graph produce
 * (the reference follows rows as directed edges and enqueues a duplicate twice).  A neighbour index outside [0, n) ->
 * F3D_ERR_INDEX.  n < 2^31.  The _dev twin takes device pointers (inst stays on the host), enqueues on `stream` and
 * synchronises it: the frontier length is read back every few levels.  Scratch: f3d_ctx_reserve_cvseg(). */
int f3d_flood_order(f3d_ctx* ctx, const int64_t* classes, int64_t n, const int64_t* offsets, const int32_t* neighbours,
                    const int64_t* inst, int ninst, int64_t* root, int64_t* order, int64_t* coffs, uint8_t* flags, int64_t stats[4]);
int f3d_flood_order_dev(f3d_ctx* ctx, const int64_t* classes, int64_t n, const int64_t* offsets, const int32_t* neighbours,
                        const int64_t* inst, int ninst, int64_t* root, int64_t* order, int64_t* coffs, uint8_t* flags,
                        int64_t stats[4], void* stream);

/* ---- CVSegmentation.color_segment: running-mean colour growing (cv.py:92-142, 367-399) ---------------------------- */
/* For every seed in order: FIFO flood from the seed (level 1) through neighbours whose id is neutral (ids in
 * neutral_ids at the start, minus points taken by earlier seeds); a popped point at level == max_level, or with
 * |sma - colour| > threshold in any channel, is skipped; otherwise npts += 1, sma = sma + (colour - sma) / npts in the
 * colours' dtype (F3D_F64 or F3D_F32), ids[point] = the seed's id (read when the seed starts) and its neighbours are
 * enqueued.  ids int64 [n] is updated in place.  threshold: HOST double [3]; neutral_ids: HOST, at most
 * F3D_COLOR_MAX_NEUTRAL; max_level <= 0 = no limit.  One workgroup runs the whole seed list.  Same adjacency
 * preconditions as f3d_flood_order.  A seed or neighbour index outside [0, n) -> F3D_ERR_INDEX (the host entry
 * then leaves ids as they were).
 * accepted (HOST, may be NULL): points accepted over all seeds.  The _dev twin: colors, offsets, neighbours, ids and seeds
 * on the device; enqueues on `stream`; accepted_dev (device int64, may be NULL) is incremented. */
#define F3D_COLOR_MAX_NEUTRAL 64
int f3d_color_segment(f3d_ctx* ctx, const void* colors, f3d_dtype dtype, int64_t n, const int64_t* offsets, const int32_t* neighbours,
                      int64_t* ids, const int64_t* seeds, int64_t nseeds, const double threshold[3], const int64_t* neutral_ids,
                      int nneutral, int max_level, int64_t* accepted);
int f3d_color_segment_dev(f3d_ctx* ctx, const void* colors, f3d_dtype dtype, int64_t n, const int64_t* offsets,
                          const int32_t* neighbours, int64_t* ids, const int64_t* seeds, int64_t nseeds, const double threshold[3],
                          const int64_t* neutral_ids, int nneutral, int max_level, int64_t* accepted_dev, void* stream);
/* Sizes the scratch of both for clouds of up to n points: later _dev calls of a strict context do not allocate. */
int f3d_ctx_reserve_cvseg(f3d_ctx* ctx, int64_t n);

/* ---- segUtils/refinement.py: region growing of a picked instance (refinement.py:70-400) ------------------------------ */
/* One FIFO flood over the adjacency with a running mean `sma` carried over the whole flood.  The first queue is
 * seeds[0..nseeds) in the given order (level 1), distinct.  A popped entry at level == max_level (max_level <= 0 = no
 * limit), or with |sma - value| > threshold in any channel (compared in float64), is skipped.  Any other entry expands:
 * its neighbours that were never enqueued are enqueued in row order at level + 1.  It is also accepted, unless
 * seeds_given != 0 and it is one of the seeds: npts += 1, sma = sma + (value - sma) / npts in the values' dtype, and the
 * point is appended to `cluster`.  sma starts as sma0 (HOST double [nchan], exactly representable in the values' dtype)
 * and npts as npts0.  This covers the reference's four floods:
 *   floodfill_depth_points / floodfill_color_points : seeds = the instance, sma0 = their average, npts0 = nseeds, given
 *   floodfill_depth_point                           : seeds = the picked list, sma0 = their average, npts0 = nseeds
 *   floodfill_color_point                           : one seed, sma0 = its colour, npts0 = 0
 * values: [n, nchan], nchan = 1 (F3D_F64) or 3 (F3D_F64 or F3D_F32); threshold: HOST double [nchan]; adjacency as for
 * f3d_flood_order (rows without duplicate entries).  cluster: int64 [n], the accepted points in acceptance order;
 * *count their number.  A seed or neighbour index outside [0, n), or a seed listed twice -> F3D_ERR_INDEX (count = 0).
 * n <= 2^31 - 2049.  The _dev twin: values, offsets, neighbours, seeds, cluster and count_dev (device int64) on the device;
 * enqueues on `stream`; an error is recorded for f3d_take_device_error.  Scratch: f3d_ctx_reserve_refine(). */
int f3d_region_grow(f3d_ctx* ctx, const void* values, f3d_dtype dtype, int nchan, int64_t n, const int64_t* offsets,
                    const int32_t* neighbours, const int64_t* seeds, int64_t nseeds, const double* sma0, int64_t npts0,
                    int seeds_given, const double* threshold, int max_level, int64_t* cluster, int64_t* count);
int f3d_region_grow_dev(f3d_ctx* ctx, const void* values, f3d_dtype dtype, int nchan, int64_t n, const int64_t* offsets,
                        const int32_t* neighbours, const int64_t* seeds, int64_t nseeds, const double* sma0, int64_t npts0,
                        int seeds_given, const double* threshold, int max_level, int64_t* cluster, int64_t* count_dev,
                        void* stream);
/* out[i] = |((x - px) * nx + (y - py) * ny) + (z - pz) * nz|: distance of float64 points [n, 3] to the plane through
 * plane_point with unit normal `normal` (both HOST double [3]); no contraction.  The reference's einsum
 * (refinement.py:155-157) sums in another order, so the two agree to rounding, not bit for bit. */
int f3d_plane_distance(f3d_ctx* ctx, const double* points, int64_t n, const double plane_point[3], const double normal[3],
                       double* out);
int f3d_plane_distance_dev(f3d_ctx* ctx, const double* points, int64_t n, const double plane_point[3], const double normal[3],
                           double* out, void* stream);
/* Sizes the scratch of f3d_region_grow_dev for clouds of up to n points: later calls of a strict context do not allocate. */
int f3d_ctx_reserve_refine(f3d_ctx* ctx, int64_t n);

/* ---- door_window_bbox.generate_mesh: door / window quads on the mesh (segUtils/door_window_bbox.py:65-150) ---------- */
/* For every wanted instance id inst[s], box_pts = points[ids == inst[s]] in ascending point index, and against the triangles
 * tris int64 [nt, 3] of verts float64 [nv, 3] (a negative vertex index counts from the end, as in NumPy):
 *   normal[t]  = cross(v1 - v0, v2 - v0) / sqrt((x*x + y*y) + z*z), left as it is when that squared norm is 0, and (0, 0, 1)
 *                when its x is NaN (Open3D compute_triangle_normals, restated);
 *   perp[m, t] = ((p - v0)_x n_x + (p - v0)_z n_z) + (p - v0)_y n_y;  tri_dist[t] = sum over m of |perp[m, t]|, in point order;
 *   candidates = the t with tri_dist[t] < min + 0.05 * min, in triangle order (none when the minimum is 0, infinite or NaN);
 *   per candidate the members projected onto its plane (p - n * perp) that pass _point_in_triangle (:26-47); the first
 *   candidate with the most of them is chosen;
 *   the instance is skipped when cos(10 deg) < n_z; else its quad [4, 3] is built from _get_perpendicular_vectors(n) and the
 *   extents of the projected members around the first one (:119-131).
 * np.dot / np.linalg.norm are the fma chains fma(x2, y2, fma(x1, y1, x0 * y0)); every other product and sum is rounded alone.
 * Outputs: quads float64 [k, 4, 3] (NaN unless the status is F3D_QUAD_OK), status int32 [k], tri int32 [k] (the chosen
 * triangle, -1 without candidates), normals float64 [nt, 3] (may be NULL).  inst holds distinct ids (a repeated id owns no
 * points: F3D_QUAD_NO_CANDIDATE); k <= F3D_QUADS_MAX_INST.  A vertex index outside [-nv, nv) -> F3D_ERR_INDEX.  Scratch
 * grows with n + k * nt (f3d_ctx_reserve_quads).
 * The _dev twin takes device pointers (inst too), enqueues on `stream` and records an index error for f3d_take_device_error;
 * the host entry reads everything back once at the end. */
#define F3D_QUAD_OK 0
#define F3D_QUAD_HORIZONTAL 1              /* skipped: the chosen triangle faces up (:117) */
#define F3D_QUAD_NO_CANDIDATE 2            /* the reference raises ValueError (argmax of an empty sequence) */
#define F3D_QUADS_MAX_INST 65535
int f3d_door_window_quads(f3d_ctx* ctx, const double* points, int64_t n, const int64_t* ids, const int64_t* inst, int k,
                          const double* verts, int64_t nv, const int64_t* tris, int64_t nt, double* quads, int32_t* status,
                          int32_t* tri, double* normals);
int f3d_door_window_quads_dev(f3d_ctx* ctx, const double* points, int64_t n, const int64_t* ids, const int64_t* inst, int k,
                              const double* verts, int64_t nv, const int64_t* tris, int64_t nt, double* quads, int32_t* status,
                              int32_t* tri, double* normals, void* stream);
int f3d_ctx_reserve_quads(f3d_ctx* ctx, int64_t n, int k, int64_t nt);

/* ---- segUtils/meshUtils.py: face filtering, vertex maps, triangle clusters (reference :235-333, :360-375) ------------ */
/* Common to the mesh entries below. tris: [nt, 3] vertex indices, C-contiguous, int64 (F3D_I64) or int32 (F3D_I32); face
 * outputs have the same type.  verts: [nv, 3] of F3D_F64 or F3D_F32; vertex outputs have the same type.  Masks and flags are
 * bytes (0 / not 0 in, 0 / 1 out).  nv < 2^31 and 3 * nt < 2^31.  The slot of a triangle corner is s = 3 * f + j.
 * Outputs whose length depends on the data are sized by the caller for the largest case given below; counts (int64 [4])
 * receives {first length, second length, 1 when a vertex index is outside [0, nv), 0}.
 * A vertex index outside [0, nv) -> F3D_ERR_INDEX and no output is written (the reference's NumPy / list indexing wraps a
 * negative index instead: a stated deviation).  The host entries return it; the _dev twins take device pointers (counts
 * too), enqueue on `stream`, write counts = {0, 0, 1, 0} alone and record the error in a bit of its own for
 * f3d_take_device_error.
 * Scratch grows with nv + nt (f3d_ctx_reserve_mesh). */
typedef enum f3d_itype {
    F3D_I64 = 0,
    F3D_I32 = 1
} f3d_itype;

/* vertex_triangle_mapping (:235-259) as a CSR: one stable radix sort of (vertex, slot) pairs.  offsets int64 [nv + 1];
 * tri int32 [3 nt] and pos int8 [3 nt]: row v = offsets[v] .. offsets[v + 1] lists the faces that hold v and the corner
 * they hold it at, in ascending slot order (the reference's append order; a face (v, v, w) is listed twice in row v). */
int f3d_mesh_vertex_map(f3d_ctx* ctx, const void* tris, int itype, int64_t nt, int64_t nv, int64_t* offsets, int32_t* tri,
                        int8_t* pos, int64_t* counts);
int f3d_mesh_vertex_map_dev(f3d_ctx* ctx, const void* tris, int itype, int64_t nt, int64_t nv, int64_t* offsets, int32_t* tri,
                            int8_t* pos, int64_t* counts, void* stream);

/* remove_faces_by_vertices (:262-301).  mask [nv]: the vertices to remove.  not_removed [nt] = no corner of the face is
 * masked; old2new int64 [nv] = the exclusive scan of !mask at the kept vertices, 0 at the removed ones; remaining
 * [counts[0], 3] (room for nt rows) = old2new[tris[not_removed]], face order kept. */
int f3d_mesh_remove_faces(f3d_ctx* ctx, const void* tris, int itype, int64_t nt, int64_t nv, const uint8_t* mask,
                          uint8_t* not_removed, void* remaining, int64_t* old2new, int64_t* counts);
int f3d_mesh_remove_faces_dev(f3d_ctx* ctx, const void* tris, int itype, int64_t nt, int64_t nv, const uint8_t* mask,
                              uint8_t* not_removed, void* remaining, int64_t* old2new, int64_t* counts, void* stream);

/* keep_faces_by_vertices (:304-333).  mask [nv]: a face is kept when any corner is masked.  The vertices of the kept faces
 * are renumbered in order of first appearance (faces in order, corners 0, 1, 2): out_verts [counts[0], 3] (room for
 * min(3 nt, nv) rows), out_tris [counts[1], 3] (room for nt rows).  The result does not depend on thread timing. */
int f3d_mesh_keep_faces(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                        const uint8_t* mask, void* out_verts, void* out_tris, int64_t* counts);
int f3d_mesh_keep_faces_dev(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                            const uint8_t* mask, void* out_verts, void* out_tris, int64_t* counts, void* stream);

/* get_triangle_clusters (:360-375; Open3D's cluster_connected_triangles restated, parity with Open3D unpinned).  Two
 * triangles are adjacent iff they share an ordered edge (min(a, b), max(a, b)) among (0,1), (0,2), (1,2); clusters are
 * numbered in ascending order of their lowest triangle.  clusters int32 [nt]; cluster_n int64 and cluster_area float64
 * [counts[0]] (room for nt entries); tri_area float64 [nt] (may be NULL) = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz) with
 * c = cross(p0 - p1, p0 - p2), every product and difference rounded alone.  A cluster's area is a fixed-shape float64 sum
 * of its members in ascending triangle index (chunks of 4096 members; in a chunk item i goes to lane i mod 64, a lane adds
 * left to right, the lanes meet in an xor butterfly 32, 16, .., 1; the chunk sums are summed the same way): the same bits
 * on every call. */
int f3d_mesh_triangle_clusters(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                               int32_t* clusters, int64_t* cluster_n, double* cluster_area, double* tri_area, int64_t* counts);
int f3d_mesh_triangle_clusters_dev(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype,
                                   int64_t nt, int32_t* clusters, int64_t* cluster_n, double* cluster_area, double* tri_area,
                                   int64_t* counts, void* stream);

/* clean_mesh (no reference counterpart): drop the faces that touch a vertex of remove_mask [nv] (may be NULL), cluster the
 * survivors, drop the clusters with fewer than min_triangles faces or an area below min_area, drop the vertices no face
 * references (vertex order kept) and renumber.  kept_v [nv], kept_t [nt]; new_verts [counts[1], 3] (room for nv rows),
 * new_tris [counts[0], 3] (room for nt rows).  Equal, bit for bit, to the composition of the entries above. */
int f3d_mesh_clean(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                   const uint8_t* remove_mask, int64_t min_triangles, double min_area, void* new_verts, void* new_tris,
                   uint8_t* kept_v, uint8_t* kept_t, int64_t* counts);
int f3d_mesh_clean_dev(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                       const uint8_t* remove_mask, int64_t min_triangles, double min_area, void* new_verts, void* new_tris,
                       uint8_t* kept_v, uint8_t* kept_t, int64_t* counts, void* stream);

/* Face frames (no reference counterpart): normals float64 [nt, 3], centroids float64 [nt, 3] (may be NULL), areas float64 [nt]
 * (may be NULL).  float32 vertices are widened exactly; every product, sum and difference is rounded alone:
 *   c = cross(p0 - p1, p0 - p2), len = sqrt((cx*cx + cy*cy) + cz*cz), area = 0.5 * len (tri_area of f3d_mesh_triangle_clusters,
 *   bit for bit), normal = c / len per component when len is finite and > 0 and (0, 0, 0) otherwise (a degenerate face, a
 *   non-finite vertex, a cross product whose length underflows to 0 or overflows), centroid = ((p0 + p1) + p2) / 3.0.
 * counts = {0, 0, bad-index flag, 0}.  No scratch. */
int f3d_mesh_face_frames(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                         double* normals, double* centroids, double* areas, int64_t* counts);
int f3d_mesh_face_frames_dev(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                             double* normals, double* centroids, double* areas, int64_t* counts, void* stream);

/* The face graph (no reference counterpart): the adjacency of the faces over shared edges as a CSR, offsets int64 [nt + 1] and
 * neighbours int32 [cap], the pair that f3d_smooth_votes, f3d_smooth_segment, f3d_components_same_class, f3d_extract_planes and
 * split_into_instances take.  A face's edges are the unordered pairs (min, max) of its corners (0,1), (0,2), (1,2), the edges of
 * f3d_mesh_triangle_clusters: (v, v) is an edge like any other, and an edge held by k faces connects all k.  Row f lists every
 * face g != f that shares at least one edge with f through which the pair passes, in strictly ascending g: no duplicates, never
 * f itself.  offsets is the exclusive scan of the row lengths, offsets[nt] = counts[0] = nnz.
 *   gate == 0: every shared edge passes; verts may be NULL (nv still bounds the indices).
 *   gate != 0: the pair passes through edge e iff s * ((nf0*ng0 + nf1*ng1) + nf2*ng2) >= cos_crease, n the normals of
 *     f3d_mesh_face_frames, s = +1 when the two faces run through e in opposite directions of their windings v0 -> v1 -> v2 -> v0
 *     (consistently oriented neighbours) and -1 when they run through it the same way; a face that holds e twice (degenerate,
 *     normal 0) counts by its first occurrence.  So the test is the dihedral one whatever the winding of either face: a flat sheet
 *     with randomly flipped faces stays connected, a sheet folded back on itself is cut.  A NaN makes the comparison false.
 * The relation is symmetric by construction (the test reads the same from f and from g), which is what split_into_instances and
 * f3d_components_same_class require of their adjacency.
 * counts = {nnz, distinct edges held by more than two half-edges (non-manifold), bad-index flag, distinct edges held by exactly one
 * half-edge (boundary)}.  When nnz > cap, offsets and counts are written, neighbours is left untouched (it may be NULL when cap
 * is 0) and the call succeeds: call again with room.  cap = 3 nt suffices when no edge has more than two faces.
 * Cost: one radix sort of the 3 nt edge keys, then per face a merge of the runs of its three keys; a run of k faces costs O(k) per
 * member, so k faces fanned around one edge cost (and produce) O(k^2).
 * Scratch grows with nt alone (f3d_ctx_reserve_mesh sizes it). */
int f3d_mesh_face_graph(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt, int gate,
                        double cos_crease, int64_t* offsets, int32_t* neighbours, int64_t cap, int64_t* counts);
int f3d_mesh_face_graph_dev(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt, int gate,
                            double cos_crease, int64_t* offsets, int32_t* neighbours, int64_t cap, int64_t* counts, void* stream);
/* Sizes the scratch of the f3d_mesh_*_dev entries for meshes of up to nv vertices and nt triangles. */
int f3d_ctx_reserve_mesh(f3d_ctx* ctx, int64_t nv, int64_t nt);

/* ---- extract_planes: the plane table of a cloud over its adjacency (no reference counterpart) ------------------------------ */
/* refinement.py's depth_floodfill_dl / depth_floodfill_point / door_floor_align take a plane table (PlaneswithPoints, BoundingPoints)
 * that the reference got from a binary it does not ship (planeUtils.run_connected_executable).  This entry produces it: a
 * deterministic plane segmentation of a cloud over its adjacency.  tests/planes_ref.py restates the contract in NumPy.
 *
 * Inputs.  xyz [n, 3] of `dtype` (float32 is widened exactly); offsets int64 [n + 1] / neighbours int32: a symmetric CSR adjacency
 * without duplicate entries, as f3d_radius_graph_* produces it (the preconditions of f3d_flood_order; a row may or may not list its
 * own point).  normals float64 [n, 3], optional: unit vectors, used as given.  dot(a, b) below is (a0*b0 + a1*b1) + a2*b2; every
 * product, sum and difference is rounded alone.  jacobi3 is the cyclic Jacobi solver of csrc/f3d_eigen.h; of its eigenvalues w[0..3)
 * lambda0 is the smallest (ties: the lowest index), lambda2 the largest of the other two (ties: the lowest index), lambda1 the third.
 *   1 core     The others of point i are the entries of its row that differ from i, in row order.
 *              normals given: i is core iff n_i's three components are finite and i has at least 2 others.
 *              normals NULL : with at least 2 others, over the sequence i, others (m points): mean = (sum added in that order) / m;
 *              the 6 centred second moments xx xy xz yy yz zz, each the sum of the products of (p - mean) added in that order;
 *              jacobi3; tr = (lambda0 + lambda1) + lambda2; i is core iff tr > 0 and lambda0 / tr <= max_variation; n_i = lambda0's
 *              eigenvector as jacobi3 returns it.  normals_out (optional, this mode only) receives n_i, 0 for a point with fewer
 *              than 2 others.
 *   2 edges    For adjacent core points i and j, d = p_j - p_i: the edge holds iff |dot(n_i, n_j)| >= cos_angle and
 *              max(|dot(d, n_i)|, |dot(d, n_j)|) <= offset.  Both tests give the same bits from either end, so the relation is
 *              symmetric on a symmetric adjacency.  Its components are found by union-find; a component's root is its lowest index.
 *   3 planes   A component with at least min_points (>= 3) core members is a plane; planes are numbered by ascending root.
 *              centroid c_P = S(p) / count and then the centred moments S((p - c_P)(p - c_P)^T), where S is a fixed-shape sum over
 *              the members in ascending index: chunks of 4096 members; in a chunk item i goes to lane i mod 64, a lane adds left to
 *              right from 0.0, the lanes meet in an xor butterfly 32, 16, .., 1; the chunk sums are summed the same way.  No float
 *              atomics.  jacobi3 of the moment sums: n_P = lambda0's vector, u_P = lambda2's vector, v_P = n_P x u_P.  Signs: with
 *              normals given n_P is negated when dot(n_P, n_root) < 0; without, when its component of largest magnitude (ties: the
 *              lowest axis) is negative.  u_P follows the largest-component rule in both modes.
 *   4 inliers  A member with |dot(p - c_P, n_P)| > dist becomes -1.  The plane is not refitted.
 *   5 attach   Synchronous rounds.  In round t every point that held -1 at the end of round t - 1 (points that are not core and
 *              dropped members included) looks along its row at the planes its neighbours held at the end of round t - 1 and takes
 *              the lowest P with |dot(p - c_P, n_P)| <= dist.  The rounds end with the first round that changes nothing (it
 *              counts), or after max_rounds; max_rounds = 0: no attaching.  The result depends on the rounds, not on thread timing.
 *   6 quads    a = dot(p - c_P, u_P), b = dot(p - c_P, v_P) over the final members; their extents through order-preserving 64-bit
 *              integer atomicMin / atomicMax.  Corner = (c_P + a u_P) + b v_P for (a, b) = (min, min), (max, min), (max, max),
 *              (min, max).  The quad's area is the product of the two extents.
 * Outputs.  labels int32 [n] (-1: no plane); planes float64 [max_planes, 8] = n_P, -dot(n_P, c_P), c_P, the rms residual
 * sqrt(S(dot(p - c_P, n_P)^2) / count) over the final members; corners float64 [max_planes, 4, 3]; counts int64 [4] = {planes
 * written, qualifying components, attach rounds run, labelled points}.  When more than max_planes components qualify the first
 * max_planes by root are written and the members of the others stay -1 (counts[1] tells); rows past the planes written are zero.  A
 * plane whose members were all dropped in step 4 and that attaches nothing keeps its number; its rms and corners are NaN.
 * Errors.  A neighbour index outside [0, n) -> F3D_ERR_INDEX and no output is written: the host entry returns it; the _dev twin
 * records it in a bit of its own for f3d_take_device_error, and every later kernel of the call returns at once.  n >= 2^31,
 * min_points < 3, max_rounds < 0, max_planes < 0 -> F3D_ERR_INVALID.  n == 0: counts = 0.
 * Two calls return identical bits.  Limits: two parallel layers closer than `offset` are one plane; with normals == NULL two layers
 * closer than the graph's radius share their rows, so they are one plane while their spread passes max_variation and hold no core
 * point otherwise; pass a finer graph, or normals.
 * The _dev twin takes device pointers (counts too), enqueues on `stream` and synchronises it every few attach rounds (the changed
 * flag stays on the device; {done, rounds} are read back).  Scratch: f3d_ctx_reserve_planes(n), for any max_planes. */
int f3d_extract_planes(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const int64_t* offsets, const int32_t* neighbours,
                       const double* normals, double cos_angle, double offset, double dist, double max_variation, int64_t min_points,
                       int64_t max_rounds, int64_t max_planes, int32_t* labels, double* planes, double* corners, int64_t* counts,
                       double* normals_out);
int f3d_extract_planes_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const int64_t* offsets, const int32_t* neighbours,
                           const double* normals, double cos_angle, double offset, double dist, double max_variation, int64_t min_points,
                           int64_t max_rounds, int64_t max_planes, int32_t* labels, double* planes, double* corners, int64_t* counts,
                           double* normals_out, void* stream);
int f3d_ctx_reserve_planes(f3d_ctx* ctx, int64_t n);

/* ---- smooth_votes / smooth_segment: neighbour-summed vote rows over an adjacency (no reference counterpart) ---------------- */
/* Every voter labels a point from its own vote row alone; these entries put a spatial prior between the vote and
 * split_into_instances: a point's row becomes the sum of its own row and of its neighbours' rows, optionally only of the neighbours
 * on the same surface (normals gate) or of similar colour (colour gate).  tests/smooth_ref.py restates the contract in NumPy.
 *
 * Inputs.  votes [n, ncols]: float64 (F3D_VOTES_F64) or the uint16 matrix f3d_project_vote_argmax writes (F3D_VOTES_U16, widened
 * exactly); 1 <= ncols <= 256.  offsets int64 [n + 1] / neighbours int32: ANY CSR -- rows need not be symmetric, may or may not list
 * their own point, and a duplicate entry counts twice.  normals float64 [n, 3] with cos_angle: optional (NULL = no gate).  colors
 * [n, 3] of `cdtype` (float32 is widened exactly) with max_color_dist >= 0: optional (NULL = no gate).  self_weight: finite, >= 0.
 * iterations >= 1.
 * One iteration.  The others of point i are the entries j != i of its row, in row order.  Such a j contributes iff every gate that
 * was given holds:
 *   normals  |dot(n_i, n_j)| >= cos_angle, dot(a, b) = (a0*b0 + a1*b1) + a2*b2   (the rule of f3d_extract_planes);
 *   colours  (dr*dr + dg*dg) + db*db <= max_color_dist*max_color_dist, d = c_j - c_i.
 * Every product, sum and difference is rounded alone; a NaN makes a comparison false.  Then per column c
 *   out[i, c] = (..((self_weight * v[i, c]) + v[j1, c]) + v[j2, c] ..)   over the contributing others in row order.
 * A column's sum has one fixed order, so the result is bit-reproducible for any input, not only for integer counts.  Iteration
 * t + 1 reads the complete output of iteration t (synchronous, two buffers); nothing is atomic.
 * f3d_smooth_votes writes votes_out float64 [n, ncols] (for odd and for even `iterations` the last one lands there); votes_out
 * overlapping votes -> F3D_ERR_INVALID.
 * f3d_smooth_segment produces classes int64 [n] and never writes the last iteration's matrix: its epilogue applies the rules of
 * f3d_segment_votes (lastcol != 0: of f3d_segment_votes_lastcol) to the smoothed row held by the wave -- nclasses, threshold, the
 * filter list with its sequential remap.  When all vote values and self_weight are integers and the row totals stay below 2^53 it
 * equals f3d_segment_votes(_lastcol) on the matrix f3d_smooth_votes would have written, bit for bit (every voter of this library
 * meets that condition).  Outside it, its own order defines it: the row total is summed lane-wise -- lane l adds columns l, l + 64,
 * l + 128, l + 192 to 0.0 in ascending order, the 64 lanes meet in an xor butterfly 32, 16, .., 1 -- where f3d_segment_votes uses
 * 16 lanes; the argmax (first maximum) and the comparisons do not depend on an order.
 * Errors.  A neighbour index outside [0, n), or offsets that do not ascend from a value >= 0 -> F3D_ERR_INDEX and no output is
 * written: a check kernel runs first, and under its flag every later kernel of the call returns at once, so nothing is read out of
 * bounds.  The host entry returns it; the _dev twin records it in a bit of its own for f3d_take_device_error.  ncols > 256 (never
 * truncated), n >= 2^31, iterations < 1, self_weight negative or not finite, a NaN cos_angle with normals, a negative or NaN
 * max_color_dist with colors, lastcol with one column and no filter -> F3D_ERR_INVALID; a filter column outside the matrix ->
 * F3D_ERR_INDEX.  n == 0: nothing to do.
 * Limits.  Unit neighbour weights only: no distance or confidence weights.
 * The host entries wrap the _dev twins, which take device pointers (the filter list stays on the host) and enqueue on `stream`.
 * Scratch: one iteration needs none; more ping-pong through one n * ncols * 8 byte matrix of the context (two for
 * f3d_smooth_segment from 3 iterations on): f3d_ctx_reserve_smooth(n, ncols, iterations) sizes it for both entries. */
typedef enum f3d_vtype {
    F3D_VOTES_F64 = 0,
    F3D_VOTES_U16 = 1
} f3d_vtype;
int f3d_smooth_votes(f3d_ctx* ctx, const void* votes, int vtype, int64_t n, int ncols, const int64_t* offsets, const int32_t* neighbours,
                     const double* normals, double cos_angle, const void* colors, f3d_dtype cdtype, double max_color_dist,
                     double self_weight, int iterations, double* votes_out);
int f3d_smooth_votes_dev(f3d_ctx* ctx, const void* votes, int vtype, int64_t n, int ncols, const int64_t* offsets,
                         const int32_t* neighbours, const double* normals, double cos_angle, const void* colors, f3d_dtype cdtype,
                         double max_color_dist, double self_weight, int iterations, double* votes_out, void* stream);
int f3d_smooth_segment(f3d_ctx* ctx, const void* votes, int vtype, int64_t n, int ncols, const int64_t* offsets,
                       const int32_t* neighbours, const double* normals, double cos_angle, const void* colors, f3d_dtype cdtype,
                       double max_color_dist, double self_weight, int iterations, int nclasses, double threshold,
                       const int32_t* filter, int nfilter, int lastcol, int64_t* classes);
int f3d_smooth_segment_dev(f3d_ctx* ctx, const void* votes, int vtype, int64_t n, int ncols, const int64_t* offsets,
                           const int32_t* neighbours, const double* normals, double cos_angle, const void* colors, f3d_dtype cdtype,
                           double max_color_dist, double self_weight, int iterations, int nclasses, double threshold,
                           const int32_t* filter, int nfilter, int lastcol, int64_t* classes, void* stream);
int f3d_ctx_reserve_smooth(f3d_ctx* ctx, int64_t n, int ncols, int iterations);

/* ---- lift_overlaps / lift_instances: 3D instances from per-frame 2D instance ids (no reference counterpart) ---------------- */
/* The 2D network separates two chairs that touch in every frame, but its instance ids are local to a frame, so they cannot be voted
 * the way classes are.  These entries turn them into ids that are consistent over the cloud ("mask lifting"): integer set arithmetic
 * over the pixel-to-point lookups (uv2pt of Fusion.fuse, f3d_render_lookups, f3d_render_mesh_lookups).  tests/lift_ref.py restates
 * the contract in NumPy.
 *
 * Inputs.  luts int32 [F, HW]: pixel -> cloud point, negative = none.  inst uint16 [F, HW]: the pixel's instance id within its frame,
 * 0 = none.  npoints N >= 1, max_ids K with 1 <= K <= 65535, F >= 1, HW >= 1, F * K < 2^31, F * HW < 2^31.  The segment of (frame f,
 * id k) has index g = f * K + (k - 1); there are S = F * K segments.
 * 1. Incidence.  The set of distinct pairs (point, g) over all pixels with lut >= 0 and inst > 0: several pixels of a frame that hit
 *    one point with one id count once, and a point may lie in two segments of one frame.  row(p) = the segments of p in ascending g;
 *    seen[p] = |row(p)| saturated at 65535 (uint16 [N]); sizes[g] = the number of distinct points of g (int32 [S]).
 * 2. Overlaps.  overlap(a, b), a < b, = the number of points whose row holds both.  f3d_lift_overlaps lists the P pairs with
 *    overlap > 0 in ascending (a, b): pairs int32 [cap, 2], counts int32 [cap].  They are written only when P <= cap (cap >= 0 entries
 *    of room; stats[0] = P in any case: the caller repeats the call with room).
 * 3. Merge.  a and b are linked iff overlap >= min_overlap, (double)overlap >= ratio * (double)min(sizes[a], sizes[b]) (one double
 *    multiply, not contracted; a NaN ratio links nothing) and, when seg_classes (int32 [S], may be NULL) is given, seg_classes[a] ==
 *    seg_classes[b].  Links are transitive.  A component's root is its smallest index; the non-empty segments' components are
 *    numbered 1 .. I in ascending root.  seg2inst[g] (int32 [S]) = that number, 0 for an empty segment.
 * 4. Vote.  count(i) = |{g in row(p) : seg2inst[g] = i}|; ids[p] (int32 [N]) = the instance with the largest count, a tie going to the
 *    smaller id, 0 for an empty row; support[p] (uint16 [N]) = the winning count, saturated at 65535.
 * 5. Small instances.  An instance that won fewer than min_points points is dropped: its points get ids 0 and support 0 (not the
 *    runner-up).  The survivors are renumbered 1 .. I' in ascending old id and seg2inst follows.  inst_points int64 [S + 1]: entry i
 *    <= I' = the points of i, entry 0 the unlabelled points; the entries past I' are not written.
 * Everything but the comparison of step 3 is integer, so every output is bit-reproducible.
 * stats (host int64 [6]) = {P, I', I, incidences, sum over the points of seen * (seen - 1) / 2, runs of the pair table}.
 * Errors.  A pixel with inst > K or lut >= N (whatever the other array says) -> F3D_ERR_INDEX and no output is written: the first
 * kernel raises a flag under which every later kernel returns at once.  Both the host entries and the _dev twins return it: they read
 * the flag back with the counts.  Arguments outside the limits above -> F3D_ERR_INVALID.
 * Cost and limits.  The pairs of a row are counted in an open-addressing table of 64-bit keys, so work grows with the sum of
 * seen^2, not with S^2.  The table starts at 2 * min(S (S - 1) / 2, max(F * HW / 4, 32768)) slots, rounded up to a power of two >= 1024 (or
 * at what f3d_ctx_reserve_lift set aside, when that is more); a probe sequence that finds no slot raises a flag, nothing is dropped,
 * and the table stage runs again with 2 * min(sum of seen * (seen - 1) / 2, S (S - 1) / 2) slots, which holds every pair (a strict
 * context returns F3D_ERR_NOMEM instead).  A row longer than 64 segments is handled by a whole wave.
 * The host entries wrap the _dev twins, which take device pointers (stats stays on the host), enqueue on `stream` and synchronise it
 * for ONE blocking readback of the counts.  Scratch: about 24 bytes per pixel + 20 per segment + 8 per point, and the table (12 bytes
 * per slot, + 24 per entry of cap); f3d_ctx_reserve_lift(F, HW, N, K, max_pairs) sizes both for up to max_pairs distinct pairs. */
int f3d_lift_overlaps(f3d_ctx* ctx, const int32_t* luts, const uint16_t* inst, int nframes, int64_t hw, int64_t npoints, int max_ids,
                      int32_t* sizes, int32_t* pairs, int32_t* counts, int64_t cap, int64_t* stats);
int f3d_lift_overlaps_dev(f3d_ctx* ctx, const int32_t* luts, const uint16_t* inst, int nframes, int64_t hw, int64_t npoints, int max_ids,
                          int32_t* sizes, int32_t* pairs, int32_t* counts, int64_t cap, int64_t* stats, void* stream);
int f3d_lift_instances(f3d_ctx* ctx, const int32_t* luts, const uint16_t* inst, int nframes, int64_t hw, int64_t npoints, int max_ids,
                       double ratio, int64_t min_overlap, const int32_t* seg_classes, int64_t min_points, int32_t* ids, uint16_t* support,
                       uint16_t* seen, int32_t* seg2inst, int64_t* inst_points, int64_t* stats);
int f3d_lift_instances_dev(f3d_ctx* ctx, const int32_t* luts, const uint16_t* inst, int nframes, int64_t hw, int64_t npoints, int max_ids,
                           double ratio, int64_t min_overlap, const int32_t* seg_classes, int64_t min_points, int32_t* ids,
                           uint16_t* support, uint16_t* seen, int32_t* seg2inst, int64_t* inst_points, int64_t* stats, void* stream);
int f3d_ctx_reserve_lift(f3d_ctx* ctx, int nframes, int64_t hw, int64_t npoints, int max_ids, int64_t max_pairs);

/* ---- (f)#1: the adjacency itself, Fusion.save_data (Fusion3DSeg/fusion.py:374-375) -------- */
/* tree = KDTree(points); adj = tree.query_radius(points, r=2*ds_radius): for every point the indices of all points
 * (itself included) whose float64 squared distance ((dx*dx + dy*dy) + dz*dz, sklearn's euclidean_rdist order) is
 * <= r*r.  Returned as CSR in two passes because the size is data dependent:
 *   count: offsets int64 [n+1] (exclusive scan, offsets[n] = *nnz); the grid stays in the context,
 *   fill : neighbours int32 [*nnz], row i = offsets[i] .. offsets[i+1]; must follow the count pass of the same cloud.
 * Order inside a row: by grid cell, then ascending index (sklearn's tree-traversal order is unspecified as well;
 * split_into_instances, the only consumer, does not depend on it).  NaN / infinite coordinates -> F3D_ERR_INVALID
 * (sklearn raises ValueError).  The result is symmetric and feeds f3d_components_same_class directly. */
int f3d_radius_graph_count(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, double radius,
                           int64_t* offsets /*[n+1]*/, int64_t* nnz);
int f3d_radius_graph_fill(f3d_ctx* ctx, int64_t n, int32_t* neighbours /*[nnz]*/);
int f3d_radius_graph_count_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, double radius,
                               int64_t* offsets /*device [n+1]*/, int64_t* nnz /*host*/, void* stream);
int f3d_radius_graph_fill_dev(f3d_ctx* ctx, int64_t n, const int64_t* offsets /*device*/,
                              int32_t* neighbours /*device [nnz]*/, void* stream);

/* ---- the bipartite form: PointCorrespondance.get_merge_maps (segUtils/correspondance.py:234-242) ------ */
/* tree = KDTree(dense, leaf_size=2); nb = tree.query_radius(sparse, r) inverted: row q (one per QUERY point, the dense pixels)
 * lists every DATA index i (the sparse cloud) with float64 squared distance ((dx*dx + dy*dy) + dz*dz, sklearn's euclidean_rdist
 * order) <= r*r, INCLUSIVE, in ASCENDING i (the order the reference's inversion loop appends them in).  float32 inputs are widened
 * exactly; data and queries have a dtype each.  CSR in two passes, like f3d_radius_graph_*:
 *   count: offsets int64 [n+1] (exclusive scan, offsets[n] = *nnz); the data's grid stays in the context, in state of its own
 *          (other entries may run between the two passes),
 *   fill : neighbours int32 [*nnz], row q = offsets[q] .. offsets[q+1]; must follow the count pass of the same queries (the _dev
 *          fill takes the same query pointer and dtype again, and the queries must hold the same values).
 * Errors (sklearn raises ValueError, here F3D_ERR_INVALID): m == 0, NaN / infinity in the data or in the queries, radius = +inf
 * (sklearn would return every pair; so does any radius >= 1e300 here).  radius < 0 or NaN: every row is empty, no error.  n == 0:
 * nothing to do.  One blocking readback per count pass (nnz and the non-finite flag together). */
int f3d_radius_query_count(f3d_ctx* ctx, const void* data, f3d_dtype data_dtype, int64_t m, const void* queries,
                           f3d_dtype query_dtype, int64_t n, double radius, int64_t* offsets /*[n+1]*/, int64_t* nnz);
int f3d_radius_query_fill(f3d_ctx* ctx, int64_t n, int32_t* neighbours /*[nnz]*/);
int f3d_radius_query_count_dev(f3d_ctx* ctx, const void* data, f3d_dtype data_dtype, int64_t m, const void* queries,
                               f3d_dtype query_dtype, int64_t n, double radius, int64_t* offsets /*device [n+1]*/,
                               int64_t* nnz /*host*/, void* stream);
int f3d_radius_query_fill_dev(f3d_ctx* ctx, const void* queries /*device, as counted*/, f3d_dtype query_dtype, int64_t n,
                              const int64_t* offsets /*device*/, int32_t* neighbours /*device [nnz]*/, void* stream);

/* ---- hybrid k-nearest search and label transfer between point sets (no reference counterpart) ------ */
/* "At most k nearest within the radius" (Open3D's KDTreeSearchParamHybrid; sklearn's KDTree.query cut at a radius), from n QUERY
 * points into m DATA points, and a label transfer built on it that carries one int64 per data point (class ids, panoptic ids, 0/1
 * bits, negative values, values above 2^32) to every query point.  data [m, 3] and queries [n, 3] have a dtype each; float32 inputs
 * are widened exactly.
 *
 * f3d_knn_query.  Let C_q be the data indices i with float64 d2(q, i) = (dx*dx + dy*dy) + dz*dz <= radius*radius, INCLUSIVE: the
 * predicate of f3d_radius_query_*, so C_q is that entry's row q.  Row q of the result holds the c = min(k, |C_q|) members of C_q that
 * are smallest under the lexicographic order (d2, i), in that order: ties in distance go to the lower index, and the result depends
 * on neither thread timing, launch shape nor cell order.  idx int32 [n, k], dist2 float64 [n, k] (the d2 above, bit for bit), counts
 * int32 [n] = c; the slots c .. k-1 hold idx = -1 and dist2 = +inf.  dist2 and counts may be NULL.
 *
 * f3d_transfer_labels.  The kept set of query q is the row above.  out[q] is the label with the most occurrences in it; among labels
 * with the same count the one whose first occurrence comes earliest in the row wins (so k = 1 gives the nearest point's label, and
 * an all-distinct row gives it too).  support[q] int32 = the winner's count (may be NULL).  An empty row gives out = fill,
 * support = 0.  labels int64 [m] are read only at the kept indices: never for a query without a neighbour.  Nothing of size [n, k]
 * is kept in memory.
 *
 * Ranges and errors, as for f3d_radius_query_*: 1 <= k <= 32, else F3D_ERR_INVALID; m == 0, NaN / infinity in the data or in the
 * queries, radius >= 1e300: F3D_ERR_INVALID, nothing written.  radius < 0 or NaN: every row is empty, no error.  n == 0: nothing to
 * do.  The search is radius-bounded by construction -- the grid's cell edge is the radius -- so an unbounded k-NN is not offered,
 * and a radius far above the point spacing degrades towards brute force (every query then visits most of the cloud).
 * Cost: one blocking readback per call (the cloud's box and the queries' non-finite flag together); the rest is enqueued.  The data's
 * grid is built per call in context state of its own: a call between the count and fill passes of f3d_radius_query_* or
 * f3d_radius_graph_* disturbs neither.  Scratch, independent of n and k: the grid, 40*m + 8*cells bytes + the sort's temporary
 * storage (cells <= 2^24), and a 64-byte flag word.  f3d_ctx_reserve_knn(m) sizes it for any radius (cells = 2^24), so that a strict
 * context does not allocate. */
int f3d_knn_query(f3d_ctx* ctx, const void* data, f3d_dtype data_dtype, int64_t m, const void* queries, f3d_dtype query_dtype,
                  int64_t n, int k, double radius, int32_t* idx /*[n,k]*/, double* dist2 /*[n,k]*/, int32_t* counts /*[n]*/);
int f3d_knn_query_dev(f3d_ctx* ctx, const void* data, f3d_dtype data_dtype, int64_t m, const void* queries, f3d_dtype query_dtype,
                      int64_t n, int k, double radius, int32_t* idx /*device [n,k]*/, double* dist2 /*device [n,k]*/,
                      int32_t* counts /*device [n]*/, void* stream);
int f3d_transfer_labels(f3d_ctx* ctx, const void* data, f3d_dtype data_dtype, int64_t m, const int64_t* labels /*[m]*/,
                        const void* queries, f3d_dtype query_dtype, int64_t n, int k, double radius, int64_t fill,
                        int64_t* out /*[n]*/, int32_t* support /*[n]*/);
int f3d_transfer_labels_dev(f3d_ctx* ctx, const void* data, f3d_dtype data_dtype, int64_t m, const int64_t* labels /*device [m]*/,
                            const void* queries, f3d_dtype query_dtype, int64_t n, int k, double radius, int64_t fill,
                            int64_t* out /*device [n]*/, int32_t* support /*device [n]*/, void* stream);
int f3d_ctx_reserve_knn(f3d_ctx* ctx, int64_t m);

/* ---- PointVotingSegmentation.vote: radius search fused with the frame vote (segUtils/voting.py:224-265) ------ */
/* The loop body of the reference for F frames in one call.  cloud [m, 3] (`cloud_dtype`), queries [F, hw, 3] (`query_dtype`: the
 * frames' world-space depth points), masks uint8 [F, hw] (already at the depth resolution), votes float64 [m, ncols] updated IN
 * PLACE, ncols = nclasses + 1.  Per frame, in frame order:
 *     nns = KDTree(cloud).query_radius(queries[f], radius)     pixel q pairs with every cloud index i whose float64 squared distance
 *                                                              ((dx*dx + dy*dy) + dz*dz) is <= radius*radius, INCLUSIVE (the
 *                                                              predicate of f3d_radius_query_*; float32 inputs are widened exactly)
 *     votes[i, masks[f, q]] += 1 ; votes[i, ncols - 1] += 1    over all pairs, with NumPy's buffered fancy-index rule: every DISTINCT
 *                                                              cell gets +1 per frame however many pairs hit it
 * so a point may receive several labels from one frame, and the last column counts the FRAMES that saw the point.  A label equal to
 * ncols - 1 is a legal index that lands on the last column: that cell then gets +2 from the frame.  No pixel is skipped (a dropout
 * pixel sits at its camera centre and votes like any other).  The result is bit-reproducible (integer counts, exact float64 adds).
 * Errors, as the reference raises them:
 *   - a label >= ncols on a pixel that HAS a neighbour is an IndexError at that frame (a pixel without one drops its label);
 *   - NaN / infinity in the queries is sklearn's ValueError at that frame (F3D_ERR_INVALID);
 *   the frames before the first offending frame are applied, it and the later ones are not; if one frame has both, the ValueError
 *   wins (the search precedes the vote).  The host variant returns F3D_ERR_INDEX / F3D_ERR_INVALID after copying the votes back.
 *   The _dev variant returns F3D_ERR_INVALID at once for the ValueError, and records the IndexError in a bit of its own of the
 *   device error word, for f3d_take_device_error; while that bit is pending, further calls write nothing.
 *   - m == 0, NaN / infinity in the cloud, radius >= 1e300: F3D_ERR_INVALID, nothing applied.  radius < 0 or NaN: no pair, no error.
 * One blocking readback per call (the cloud's box and a streaming pre-pass over masks and queries together); the search that looks
 * for an offending label's neighbours runs only when the pre-pass saw such a label.  The cloud's grid is built once per call, in
 * context state of its own (other entries may run between calls).
 * Scratch, independent of the number of pairs: the grid, 40*m + 8*cells bytes + the sort's temporary storage (cells <= 2^24), and
 * the per-frame key sets, G * m * W * 4 bytes with W = ceil((min(ncols, 256) + 1) / 32) words per point and
 * G = clamp(256 MiB / (m * W * 4), 1, 64) frames per launch.  f3d_ctx_reserve_point_vote sizes both for any radius, so that a strict
 * context does not allocate. */
int f3d_point_vote_frames(f3d_ctx* ctx, const void* cloud, f3d_dtype cloud_dtype, int64_t m, const void* queries,
                          f3d_dtype query_dtype, const uint8_t* masks, int64_t nframes, int64_t hw, double radius,
                          double* votes /*[m, ncols], in place*/, int ncols);
int f3d_point_vote_frames_dev(f3d_ctx* ctx, const void* cloud, f3d_dtype cloud_dtype, int64_t m, const void* queries,
                              f3d_dtype query_dtype, const uint8_t* masks, int64_t nframes, int64_t hw, double radius,
                              double* votes /*device [m, ncols], in place*/, int ncols, void* stream);
int f3d_ctx_reserve_point_vote(f3d_ctx* ctx, int64_t m, int ncols);

/* ---- occlusion-aware forward voting: point-splat z-buffer renders of the cloud (no reference counterpart) ------------------ */
/* The forward path (f3d_project_vote_argmax) lets a point vote in every view whose frustum holds it, also through a wall; the
 * reference's votes go through uv2pt, the pixel -> point table Fusion.fuse builds from depth frames (fusion.py:105-111, :326-327),
 * so only the surface a camera saw gets its label.  These entries render the cloud itself into per-view depth buffers and give
 * (1) uv2pt-style lookups for any posed cloud, which feed f3d_vote_uv2pt_batch, and (2) the forward vote with a visibility test.
 * View j is views[j] from f3d_views_build; point i is the caller-order index, n < 2^31; float32 clouds are widened exactly.
 *   sample   (h0, h1, h2) = f3d_project_h(p), u = floor(h0 / h2), v = floor(h1 / h2), z32 = (float)h2 rounded to nearest even: the
 *            arithmetic of f3d_project_view.  Point i has a sample in view j iff it is inside the view's 5 planes (a4),
 *            0 <= u < w, 0 <= v < h and FLT_MIN <= z32 < +inf (the bits of z32 are then a monotone unsigned key; NaN, zero,
 *            negative and subnormal depths have no sample).
 *   key      key(i, j) = (uint64)bits(z32) << 32 | (uint32)i.  Cell (j, r, c) of zkey [V, h, w] is the minimum key over all samples
 *            (i, j) and offsets |du|, |dv| <= splat with r = v + dv, c = u + du inside the image; all ones when there is none.  The
 *            nearest point by float32 depth wins, ties go to the lowest index; the result does not depend on thread timing, launch
 *            shape or the pass size.  splat is an integer in [0, 8]: a point owns the (2 splat + 1)^2 pixel patch around its pixel.
 *   lookups  depth float32 [V, h, w] = the winning z32, +inf for an empty cell; uv2pt int32 [V, h * w] = the winning index, -1 for
 *            an empty cell (pixel index v * w + u).  Either may be NULL.
 *   visible  sample (i, j) is visible iff (double)z32 <= (double)zmin32 + depth_tol, zmin32 = the depth of cell (j, v, u) (never
 *            empty: the sample covers it; f3d_vote_visible_mesh tests against a mesh instead).  depth_tol >= 0, +inf allowed (every sample is visible: the votes of
 *            f3d_project_vote_argmax).
 *   vote     votes[i, masks[j, v, u]] += 1 for every visible sample; votes float64 [n, ncols], IN PLACE (the layout of
 *            VotingSegmentation: f3d_segment_votes finishes the job).  A label >= ncols on a visible sample is the reference's
 *            IndexError: F3D_ERR_INDEX from the host variant, a bit of its own for f3d_take_device_error from the _dev variant;
 *            the outputs are then unspecified.  Labels of invisible samples are never read.
 * The keys live in context scratch and the views are processed in passes (render, then unpack or vote) of views_per_pass views;
 * 0 = as many as fit 256 MiB of keys, at least 1.  Votes are sums over views, so the pass size never changes a result.
 * F3D_ERR_INVALID: n >= 2^31, splat outside [0, 8], depth_tol negative or NaN, views_per_pass < 0.
 * f3d_ctx_reserve_render sizes the keys of an automatic pass over nviews views of h x w pixels, the only scratch of the _dev entries:
 * a strict context then allocates nothing in them with views_per_pass = 0 (or any smaller pass).  The keys do not grow with n, which
 * is only checked against the limit above. */
int f3d_render_lookups(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views, int nviews, int h, int w,
                       int splat, float* depth, int32_t* uv2pt);
int f3d_render_lookups_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views_dev /*device [V]*/,
                           int nviews, int h, int w, int splat, float* depth, int32_t* uv2pt, void* stream);
int f3d_vote_visible(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views, int nviews,
                     const uint8_t* masks /*[V,H,W]*/, int h, int w, int splat, double depth_tol, double* votes /*[n, ncols], in place*/,
                     int ncols, int views_per_pass);
int f3d_vote_visible_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views_dev /*device [V]*/,
                         int nviews, const uint8_t* masks, int h, int w, int splat, double depth_tol, double* votes, int ncols,
                         int views_per_pass, void* stream);
int f3d_ctx_reserve_render(f3d_ctx* ctx, int64_t n, int nviews, int h, int w);
/* Diagnostic: renders the views like f3d_render_lookups_dev with a counting build of the splat kernel.  counts[0] = samples,
 * counts[1] = cells they cover, counts[2] = atomics issued (a cell that already held a smaller key is skipped; this count depends on
 * thread timing, the rendered keys do not).  ms (may be NULL): device-event times of the key fill and of the splat, summed over the
 * passes.  Device pointers; synchronises `stream` once per pass. */
int f3d_debug_render_counts(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views_dev, int nviews,
                            int h, int w, int splat, uint64_t counts[3], double ms[2], void* stream);

/* ---- triangle-mesh z-buffer renders: face voting and mesh occlusion (no reference counterpart) ---------------------------- */
/* The same depth keys, filled from a triangle mesh instead of a point splat: a watertight occluder for the forward vote, and the
 * pixel -> triangle lookups that let the masks vote for faces directly.  All arithmetic is float64 without contraction, every product
 * and sum as written.  View j is views[j] from f3d_views_build; triangle t is the caller-order index, nt < 2^31; tris [nt, 3] int64
 * (F3D_I64) or int32 (F3D_I32), verts [nv, 3] float64 or float32 (widened exactly), as the meshUtils entries take them; h * w <= 2^30.
 *   vertex    (h0, h1, h2) = f3d_project_h(K, qinv, t, p), x = h0 / h2, y = h1 / h2, iz = 1.0 / h2, z32 = (float)h2.  Eligible in the view
 *             iff FLT_MIN <= z32 < +inf, |x| <= 2^30 and |y| <= 2^30 (NaN fails).  The 5 frustum planes play no part.
 *   pixel     (u, v) covers [u, u+1) x [v, v+1), the floor of the point path; its sample is (sx, sy) = (u + 0.5, v + 0.5).
 *   triangle  (a, b, c) is rasterised in a view iff its three vertices are eligible, its three indices are distinct and
 *             A = (x_b - x_a)*(y_c - y_a) - (y_b - y_a)*(x_c - x_a) is finite and non-zero.  Both windings are drawn (no culling).
 *             There is NO near-plane clipping: a triangle with both an eligible and an ineligible vertex is skipped and counted in
 *             straddling[j].  What is lost that way lies nearer to the camera plane than the triangle's longest edge: nothing a
 *             camera sees of a scan mesh (centimetre edges); a coarse mesh (a wall of two triangles) must be subdivided by the caller.
 *   edges     per edge between vertex indices i and j, lo = min(i, j), hi = max(i, j):
 *                 e = (x_hi - x_lo)*(sy - y_lo) - (y_hi - y_lo)*(sx - x_lo)
 *             the value of the directed edge i -> j is e if i < j, else -e.  E01, E12, E20 = the directed values of a->b, b->c, c->a,
 *             each negated when A < 0.  The sample is covered iff E01 >= 0 && E12 >= 0 && E20 >= 0.  Two triangles sharing an edge
 *             evaluate bit-identical e with opposite sign requirements, so a sample inside a closed fan is never dropped; a sample
 *             exactly on a shared edge belongs to both, and the key decides.
 *   depth     s = (E12 + E20) + E01, z = s / ((E12*iz_a + E20*iz_b) + E01*iz_c), z32 = (float)z (perspective-correct).  The fragment
 *             exists iff the sample is covered, s > 0, FLT_MIN <= z32 < +inf and z <= z_far (+inf allowed).
 *   pixels    the candidates of a triangle are u in [floor(min x) - 1, floor(max x) + 1], v likewise, clamped to the image; only the
 *             coverage test decides among them.  (Every covered sample lies inside that box but for rounding on slivers thinner than
 *             2^-20 px; fixing the box makes the result exact there too.)
 *   key       key = (uint64)bits(z32) << 32 | (uint32)t; cell (j, r, c) of zkey [V, h, w] holds the minimum key over the fragments of
 *             view j at that pixel, all ones when there is none: the layout and sentinel of f3d_render_lookups.  The nearest float32
 *             depth wins, ties go to the lowest triangle index; the result does not depend on thread timing, launch shape, work
 *             distribution or pass size.
 * f3d_render_mesh_lookups: depth float32 [V, h, w] (+inf = empty), uv2tri int32 [V, h * w] (-1 = empty), straddling int64 [V]; any of
 *   the three may be NULL.
 * f3d_vote_faces: the reference's voting direction (the pixel votes for what it sees) with one row per triangle: per view,
 *   votes[uv2tri[j], masks[j]] += 1 over the non-empty cells, float64 [nt, ncols] IN PLACE, the layout of VotingSegmentation
 *   (f3d_segment_votes finishes the job).  Per pass this IS raster -> unpack -> the launches of f3d_vote_uv2pt_batch, so its rules hold:
 *   ncols <= 256, and the reference's fancy-index "+=" (voting.py:98) gives a (triangle, label) pair ONE vote per view however many of
 *   the view's pixels carry it.  A label >= ncols on a non-empty cell is the reference's IndexError.
 * f3d_vote_visible_mesh: the forward vote of a POINT CLOUD xyz [n, 3] with the mesh as the occluder.  The points' samples are exactly
 *   those of f3d_vote_visible; a sample is visible iff (double)z32 <= (double)zmin32 + depth_tol, zmin32 = the mesh depth of its pixel,
 *   an EMPTY cell counting as +inf (nothing is in front of it).  depth_tol = +inf: the votes of f3d_project_vote_argmax.
 * Views go in passes of views_per_pass (0 = as many as fit 256 MiB of keys, and for f3d_vote_faces one launch of the batched vote);
 * the keys live in the scratch of f3d_render_lookups.  f3d_ctx_reserve_mesh_render sizes all scratch of the _dev entries (keys, the
 * rasteriser's list, the lookups and the vote table of f3d_vote_faces) for automatic passes: a strict context then allocates nothing.
 * Errors: a vertex index outside [0, nv) -> F3D_ERR_INDEX and nothing is written (a pre-pass; in the _dev twins a device-error bit of
 * its own for f3d_take_device_error); the IndexErrors above likewise (host: nothing written back; _dev: outputs unspecified).
 * nt >= 2^31, depth_tol negative or NaN, z_far NaN, views_per_pass < 0 -> F3D_ERR_INVALID.  Non-finite vertices are no error: their
 * triangles are ineligible.  nt == 0: empty buffers, no votes. */
int f3d_render_mesh_lookups(f3d_ctx* ctx, const void* verts, f3d_dtype vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                            const f3d_view* views, int nviews, int h, int w, double z_far, float* depth, int32_t* uv2tri,
                            int64_t* straddling);
int f3d_render_mesh_lookups_dev(f3d_ctx* ctx, const void* verts, f3d_dtype vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                                const f3d_view* views_dev /*device [V]*/, int nviews, int h, int w, double z_far, float* depth,
                                int32_t* uv2tri, int64_t* straddling, void* stream);
int f3d_vote_faces(f3d_ctx* ctx, const void* verts, f3d_dtype vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                   const f3d_view* views, int nviews, const uint8_t* masks /*[V,H,W]*/, int h, int w, double z_far,
                   double* votes /*[nt, ncols], in place*/, int ncols, int views_per_pass);
int f3d_vote_faces_dev(f3d_ctx* ctx, const void* verts, f3d_dtype vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                       const f3d_view* views_dev, int nviews, const uint8_t* masks, int h, int w, double z_far, double* votes, int ncols,
                       int views_per_pass, void* stream);
int f3d_vote_visible_mesh(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const void* verts, f3d_dtype vdtype, int64_t nv,
                          const void* tris, int itype, int64_t nt, const f3d_view* views, int nviews, const uint8_t* masks, int h, int w,
                          double z_far, double depth_tol, double* votes /*[n, ncols], in place*/, int ncols, int views_per_pass);
int f3d_vote_visible_mesh_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const void* verts, f3d_dtype vdtype, int64_t nv,
                              const void* tris, int itype, int64_t nt, const f3d_view* views_dev, int nviews, const uint8_t* masks,
                              int h, int w, double z_far, double depth_tol, double* votes, int ncols, int views_per_pass, void* stream);
int f3d_ctx_reserve_mesh_render(f3d_ctx* ctx, int nviews, int h, int w);
/* Diagnostic: renders the views like f3d_render_mesh_lookups_dev (depth, uv2tri: device, may be NULL) with a counting build of the
 * rasteriser.  The work is split over three tiers by the size of a triangle's candidate box, which no result depends on:
 * counts[0..3] = (triangle, view) pairs walked by one lane (small), by their wave (medium), deferred to the list of the tile kernel
 * (huge), and huge pairs that found the list full and were walked by their wave instead (overflow).  list_capacity: 0 = the
 * library's, else a smaller capacity for this call (a test forces the overflow path with a handful of triangles).  ms (may be NULL):
 * device-event times of the key fill and of the raster (both kernels), summed over the passes.  Synchronises `stream` once per pass. */
int f3d_debug_raster_counts(f3d_ctx* ctx, const void* verts, f3d_dtype vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                            const f3d_view* views_dev, int nviews, int h, int w, double z_far, int64_t list_capacity, float* depth,
                            int32_t* uv2tri, uint64_t counts[4], double ms[2], void* stream);

/* ---- a5: patch matching of Fusion.fuse (Fusion3DSeg/fusion.py:269-298) ------------------- */
/* The loop over the in-frustum points ("seeds", in index order) of one frame: seed k takes the still-free depth pixels of
 * the (2*half+1)^2 window around its projection uv[:,k] that lie within `radius` of it and whose normals satisfy
 * dot > min_cosine, judged with the seed's position / normal from before the frame.  Equivalent, and what is computed:
 * owner[p] = the lowest k whose window covers free pixel p and whose test accepts it, -1 if none (or not free).
 * uv int32 [2,m] (row 0 = u, row 1 = v, as points2pixel returns it), seeds [m,3], frame points / normals [h*w,3],
 * free uint8 [h*w] (non_merged), owner int32 [h*w].  The test reproduces NumPy's evaluation order (norm(axis=-1),
 * einsum 'ij,j->i') and the window the reference's slice arithmetic, negative stops included. */
int f3d_patch_owner(f3d_ctx* ctx, const int32_t* uv, int64_t m, int h, int w, int half, double radius, double min_cosine,
                    const double* seed_pts, const double* seed_normals, const double* frame_pts,
                    const double* frame_normals, const uint8_t* free_px, int32_t* owner);
int f3d_patch_owner_dev(f3d_ctx* ctx, const int32_t* uv, int64_t m, int h, int w, int half, double radius,
                        double min_cosine, const double* seed_pts, const double* seed_normals, const double* frame_pts,
                        const double* frame_normals, const uint8_t* free_px, int32_t* owner, void* stream);

/* Fusion.patch_downsample (fusion.py:172-208): the pixels are visited in a shuffled order (prio[p] = position of pixel p); a
 * pixel that is still free becomes a seed and takes the free pixels of its window that pass the same test.  owner[p] = the
 * pixel index of the seed that takes p (a seed owns itself), -1 for pixels nobody takes; seeds are the pixels with
 * owner[p] == p, in ascending prio.  Resolved in data-parallel rounds (*rounds, diagnostic).
 *
 * The matching (f3d_patch_owner) and this seed selection with the ORDERED SUMS of what every seed takes (fusion.py:195-201,
 * 289-298: np.mean over the accepted pixels stacked in window order): one thread per seed adds the rows of its pixels in ascending
 * pixel index, the order NumPy adds them in, so the fused points / normals / colours stay bit-identical.  sums double [.., 9] =
 * rows of frame_pts, frame_normals, frame_colors (colours may be NULL -> zeros), counts int32 = pixels taken.  f3d_patch_match:
 * per seed (m rows); f3d_patch_seeds_sums: per pixel (h*w rows, meaningful where owner[p] == p).  The frame is uploaded once per
 * call. */
int f3d_patch_match(f3d_ctx* ctx, const int32_t* uv, int64_t m, int h, int w, int half, double radius, double min_cosine,
                    const double* seed_pts, const double* seed_normals, const double* frame_pts, const double* frame_normals,
                    const double* frame_colors, const uint8_t* free_px, int32_t* owner, double* sums, int32_t* counts);
int f3d_patch_seeds_sums(f3d_ctx* ctx, const double* frame_pts, const double* frame_normals, const double* frame_colors,
                         const int32_t* prio, const uint8_t* free_px, int h, int w, int half, double radius, double min_cosine,
                         int32_t* owner, double* sums, int32_t* counts, int32_t* rounds);
/* The same two calls on DEVICE pointers (frame, seeds, free mask, outputs), enqueued on `stream`.  f3d_patch_seeds_sums_dev still
 * reads back one counter per round of the seed resolution (the round loop is data dependent); *rounds is a host int (may be NULL). */
int f3d_patch_match_dev(f3d_ctx* ctx, const int32_t* uv, int64_t m, int h, int w, int half, double radius, double min_cosine,
                        const double* seed_pts, const double* seed_normals, const double* frame_pts, const double* frame_normals,
                        const double* frame_colors, const uint8_t* free_px, int32_t* owner, double* sums, int32_t* counts,
                        void* stream);
int f3d_patch_seeds_sums_dev(f3d_ctx* ctx, const double* frame_pts, const double* frame_normals, const double* frame_colors,
                             const int32_t* prio, const uint8_t* free_px, int h, int w, int half, double radius,
                             double min_cosine, int32_t* owner, double* sums, int32_t* counts, int32_t* rounds, void* stream);

/* ---- a5 on a device-resident cloud: the per-frame steps of Fusion.fuse_device --------------------------- */
/* The cloud is rows [0, *count) of caller-owned device arrays points / normals / colours float64 [cap,3], nmerges int64 [cap],
 * occurences uint32 [cap]; *count is an int64 on the device that f3d_fusion_new_seeds_dev advances.  Normals are normalised as
 * nsum / sqrt(nsum.dot(nsum)), the dot in the order `norm_mode` names: F3D_NORM_PLAIN ((x*x + y*y) + z*z), F3D_NORM_FMA
 * (fma(z,z, fma(y,y, x*x)), what an FMA BLAS ddot gives) or F3D_NORM_HOST (left unnormalised: the caller normalises). */
#define F3D_NORM_PLAIN 0
#define F3D_NORM_FMA 1
#define F3D_NORM_HOST 2

/* Order-preserving compaction of project_view's inside flags over n rows (rows >= *count ignored): the hits k = 0..m-1 in ascending
 * row, ids int32 [m], uv int32 [2,m] (row stride m; uv_all is [2,n]), hit_pts / hit_normals [m,3] (copies of the cloud rows).  Room
 * for m = n in every output.  stats int64 [3] (device) = {m, valid pixels of the frame (valid uint8 [npx], nonzero = valid), *count}:
 * the one small readback before the matching. */
int f3d_fusion_hits_dev(f3d_ctx* ctx, const uint8_t* inside, const int32_t* uv_all, int64_t n, const int64_t* count,
                        const double* points, const double* normals, const uint8_t* valid, int64_t npx, int32_t* ids,
                        int32_t* uv, double* hit_pts, double* hit_normals, int64_t* stats, void* stream);
/* The matches of a frame (f3d_patch_match_dev's sums / counts over the m hits) applied in place to the rows ids[k] with counts[k] > 0:
 * (sum + row) / (n + 1) for points, colours and normals, the normal normalised, nmerges += n, occurences += 1. */
int f3d_fusion_seed_update_dev(f3d_ctx* ctx, const int32_t* ids, int64_t m, const double* sums, const int32_t* counts, int norm_mode,
                               double* points, double* normals, double* colors, int64_t* nmerges, uint32_t* occurences,
                               void* stream);
/* uv2pt int32 [npx] = ids[owner[p]] (-1 where owner[p] < 0); free_px[p] = 0 for every taken pixel. */
int f3d_fusion_lookup_dev(f3d_ctx* ctx, const int32_t* owner, const int32_t* ids, int64_t npx, int32_t* uv2pt, uint8_t* free_px,
                          void* stream);
/* patch_downsample's guard on a frame: stats int64 [2] (device) = {free pixels, 1 if the frame takes the sequential path}: radius <= 0,
 * or a free pixel whose own normal test fails (normals.normals <= min_cosine) or whose point is not finite. */
int f3d_fusion_frame_check_dev(f3d_ctx* ctx, const uint8_t* free_px, const double* frame_pts, const double* frame_normals, int64_t npx,
                               double radius, double min_cosine, int64_t* stats, void* stream);
/* prio int32 [npx] = the inverse of the visiting order: prio[order[i]] = i (order int64 [npx], a permutation of 0..npx-1). */
int f3d_fusion_prio_dev(f3d_ctx* ctx, const int64_t* order, int64_t npx, int32_t* prio, void* stream);
/* patch_downsample's new seeds (f3d_patch_seeds_sums_dev's owner / sums / counts) appended to the cloud in visiting order: the seed of
 * rank r goes to row *count + r (mean = sum / n, normal normalised, nmerges = n, occurences = 1), uv2pt[p] = *count + rank of
 * owner[p] and free_px[p] = 0 for every taken pixel, then *count += seeds.  The caller guarantees cap >= *count + npx. */
int f3d_fusion_new_seeds_dev(f3d_ctx* ctx, const int32_t* owner, const int32_t* prio, const double* sums, const int32_t* counts,
                             int64_t npx, int norm_mode, int64_t* count, int64_t cap, double* points, double* normals, double* colors,
                             int64_t* nmerges, uint32_t* occurences, int32_t* uv2pt, uint8_t* free_px, void* stream);

/* ---- (f)#3: depth frame -> world points (RTAB_utils/ios_rtab.py) -------------------------- */
/* RTAB2Cache.__getRGBP3d (:171-173): x = (px - cx) * (d / fx), y = (py - cy) * (d / fy), z = d with the scaled
 * intrinsics K and the integer pixel grid; __getModP3d: divided by depth_scale (1000: mm -> m, :187), rotated by the
 * frame's camera->world quaternion (w,x,y,z; the pose file stores x,y,z,w, :190) with SpatQuadranion.rotate and
 * translated (:191-192).  depth [h,w] row-major -> xyz float64 [h*w,3], pixel order = row-major, every operation in
 * the reference's order (float64, IEEE division). */
#define F3D_DEPTH_U16 2          /* 16-bit PNG depth as PIL loads it */
#define F3D_DEPTH_F32 1
#define F3D_DEPTH_F64 0
int f3d_unproject_depth(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9],
                        double depth_scale, const double q_wxyz[4], const double t[3], double* xyz /*[h*w*3]*/);
int f3d_unproject_depth_dev(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9],
                            double depth_scale, const double q_wxyz[4], const double t[3], double* xyz, void* stream);
/* F frames per launch (a single 1024 x 1024 frame is launch-bound): depth [F, h, w], q_wxyz host [F, 4], t host [F, 3] ->
 * xyz float64 [F, h*w, 3].  The poses travel in the kernel argument block, 64 frames per launch: enqueue only, no staging. */
int f3d_unproject_depth_batch_dev(f3d_ctx* ctx, const void* depth, int depth_type, int nframes, int h, int w,
                                  const double K[9], double depth_scale, const double* q_wxyz, const double* t,
                                  double* xyz, void* stream);


/* ---- surface normals of depth frames: RTAB2Cache.surface_normal_estimation (RTAB_utils/ios_rtab.py:236-248) ---- */
/* Open3D's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) restated, then the flip towards the camera.  Per point i
 * of a frame, in float64 (parity with Open3D itself is unpinned):
 *   neighbours: the points j of the SAME frame (i included) with d2 = (dx*dx + dy*dy) + dz*dz < radius*radius (strict), the
 *               max_nn smallest in (d2, j) order (ties to the lower index);
 *   normal    : (0, 0, 1) when fewer than 3 are kept, when all kept points are bit-identical (the zero-depth cluster) or when
 *               the covariance vanishes; else the unit eigenvector of the smallest eigenvalue of C = E[p p^T] - E[p] E[p]^T
 *               over the kept set (deterministic: no float atomics);
 *   orient    : flipped when dot(n, (p - c) / |p - c|) > 0, c = the frame's camera centre; a point p == c gives NaN and is not
 *               flipped, as in the reference.  orient = 0 returns the unoriented normals.
 * Non-finite coordinates, radius <= 0 (or not finite), max_nn outside [1, F3D_NORMALS_MAX_NN] -> F3D_ERR_INVALID, nothing written.
 * F * n < 2^31.  F == 0 or n == 0 is a no-op. */
#define F3D_NORMALS_MAX_NN 64
/* One frame, host pointers: xyz [n, 3] -> normals [n, 3]; counts [n] int32 (kept neighbours) and neighbours [n, max_nn] int32
 * (-1 padded, (d2, j) order) may be NULL; cam_centre may be NULL when orient == 0. */
int f3d_estimate_normals(f3d_ctx* ctx, const double* xyz, int64_t n, const double cam_centre[3], double radius, int max_nn,
                         int orient, double* normals, int32_t* counts, int32_t* neighbours);
/* F frames at once: xyz device [F, n, 3], cam_centres HOST [F, 3] (may be NULL when orient == 0) -> normals device [F, n, 3];
 * counts device [F*n] and neighbours device [F*n, max_nn] optional (NULL).  One blocking readback per call (the bounding box
 * of the batch, which sizes the grid and rejects non-finite input), none per frame; the rest is enqueued on `stream`. */
int f3d_estimate_normals_batch_dev(f3d_ctx* ctx, const double* xyz, int nframes, int64_t n, const double* cam_centres,
                                   double radius, int max_nn, int orient, double* normals, int32_t* counts, int32_t* neighbours,
                                   void* stream);

/* ---- TSDF reconstruction: a triangle mesh from posed depth frames (no reference counterpart) ------------------------------ */
/* The reference takes its mesh from an external exporter; a capture of posed depth frames has none.  These entries integrate the
 * frames into a truncated signed distance volume and extract a triangle mesh from it by surface nets (no lookup table).  All
 * arithmetic is float64 without contraction, every product, sum and division as written; storage is float32.
 *   volume     dims (nx, ny, nz), each >= 1, nx * ny * nz < 2^31; origin lo[3] (float64), voxel edge vs > 0.  Linear index
 *              lin = (k * ny + j) * nx + i (x fastest); voxel centre c_a = lo[a] + ((double)idx_a + 0.5) * vs.  The state is two
 *              caller-owned arrays, tsdf float32 [nz, ny, nx] and weight float32 [nz, ny, nx]; a fresh volume is all zeros.  The
 *              library keeps no pointer to the state between calls.
 *   integrate  nframes depth images [F, h, w] of type F3D_DEPTH_U16 / F32 / F64 with the depth_scale of f3d_unproject_depth; view f
 *              is views[f] from f3d_views_build.  Per voxel the frames are applied in ascending f (the running average depends on
 *              the order).  For each frame:
 *                1. (h0, h1, h2) = f3d_project_h(K, qinv, t, c); skip unless h2 > 0.
 *                2. x = h0 / h2, y = h1 / h2; skip unless x >= 0 && x < w && y >= 0 && y < h (NaN fails); u = (int)floor(x),
 *                   v = (int)floor(y): the floor pixel of points2pixel, no interpolation.
 *                3. d = (double)raw[v, u] / depth_scale; skip unless d > 0 && d <= max_depth (NaN and inf fail).
 *                4. sdf = d - h2; skip if sdf < -trunc.  val = sdf / trunc, and val = 1.0 if val > 1.0.
 *                5. T = (float)(((double)T_old * (double)w_old + val) / ((double)w_old + 1.0)).
 *                6. w = (float)min((double)w_old + 1.0, (double)max_weight).
 *              The five frustum planes of the view play no part in the result.  trunc > 0; max_weight in [1, 2^24].
 *   colour     f3d_tsdf_integrate_color: the same with a third caller-owned state array, color float32 [nz, ny, nx, 4], channels
 *              (r, g, b, wc) on a 0..255 scale, wc the colour's own weight; a fresh volume is all zeros; 16 bytes per voxel, 16-byte
 *              aligned (the _dev form refuses another pointer).  Colour images rgb uint8 [F, hc, wc_img, 3], one per depth frame;
 *              hc, wc_img > 0 are independent of h, w, hc * wc_img < 2^31.  The colour pixel of depth pixel (u, v) is
 *              uc = (int64)u * wc_img / w, vc = (int64)v * hc / h (the integer rule of f3d_fuse_features).  Steps 1 - 6 are those above;
 *              for a frame that has passed step 4, with val as computed there before the clamp:
 *                7. the voxel is in band iff !(val > 1.0).  If it is, for each channel with pix = rgb[f, vc, uc, channel]:
 *                   C = (float)(((double)C_old * (double)wc_old + (double)pix) / ((double)wc_old + 1.0)); then
 *                   wc = (float)min((double)wc_old + 1.0, (double)max_weight).
 *              Frames apply in ascending f.  tsdf and weight come out bit-identical to f3d_tsdf_integrate on the same inputs.  A voxel
 *              that is never in band keeps its 16 bytes unread and unwritten.  The colour has a weight of its own because a voxel just
 *              in front of a silhouette is updated, with the clamped 1.0, by every frame that sees the background far behind it
 *              through the same pixel: those frames must not give it the background's colour.
 *   extract   a voxel is observed iff weight >= min_weight (min_weight >= 1) and inside iff it is observed and tsdf < 0 (+0.0 and
 *              -0.0 are outside).  Cell (i, j, k), 0 <= idx_a <= n_a - 2, has the 8 voxels idx + {0, 1}^3 as corners and is active
 *              iff all 8 are observed and they are not all on one side.
 *   vertex     of an active cell.  For an axis a let (b, c) be the next two axes cyclically (x -> (y, z), y -> (z, x), z -> (x, y)).
 *              Cell edge e = 4 a + 2 oc + ob (ob, oc in {0, 1}) runs from the corner with local coordinates L[a] = 0, L[b] = ob,
 *              L[c] = oc to the one with L[a] = 1; it crosses iff the insideness of its ends differs, at L with
 *              L[a] = s0 / (s0 - s1), s0 and s1 the float32 samples at the two ends widened to double.  Each component is summed
 *              over the crossing edges in ascending e, starting from 0.0; local = sum / (double)count;
 *              vert_a = lo[a] + (((double)cell_a + 0.5) + local_a) * vs.  Vertex ids are the ranks of the active cells in ascending
 *              linear cell index (the voxel formula).
 *   faces      for every voxel p = (i, j, k) and axis a with p_a <= n_a - 2: both ends of the grid edge p -> p + e_a observed, their
 *              insideness different, and the four cells around the edge in range and active: A = p - e_b - e_c, B = p - e_c, C = p,
 *              D = p - e_b.  Each such edge gives one quad, (A, B, C, D) when p is inside (the normal points along +a, from inside to
 *              outside), else (A, D, C, B); it splits into the triangles (q0, q1, q2) and (q0, q2, q3).  The quads come in
 *              ascending 3 * lin(p) + a, the two triangles of a quad are consecutive.
 *   vertex colours  f3d_tsdf_extract_colors, a third member of the count -> fill sequence (before, after or without the fill): for an
 *              active cell, walk its crossing edges in ascending e with L[a] = s0 / (s0 - s1) exactly as the vertex rule does; c0, c1
 *              the colour state at the edge's two ends.  Both ends with wc > 0: the edge adds col = c0 + L[a] * (c1 - c0) per channel
 *              (float64, as written); one end: that end's colour; neither: nothing.  sum starts at 0.0 per channel,
 *              m = sum / (double)count over the contributing edges, rgb uint8 [nv, 3] = (uint8)floor(min(max(m, 0), 255) + 0.5)
 *              (a NaN m gives 0); the optional colored uint8 [nv] is 1 where count > 0, else 0 with rgb = 0.  Vertex ids are those of
 *              the fill.  It needs no scratch beyond the count's.
 * Outputs: verts float64 [nv, 3], tris int32 [nt, 3] of vertex ids; nv, nt < 2^31, otherwise F3D_ERR_INVALID.  The result depends on
 * nothing but the state, min_weight, lo and vs: not on the launch shape, timing or the scan's tiling (tiles of F3D_TSDF_SCAN_TILE counts,
 * scanned by blocks of 256).
 * f3d_tsdf_extract_count -> f3d_tsdf_extract_fill is a sequence (see the preamble): the cell ranks and the quad offsets stay in
 * context scratch, the host-pointer count also keeps its copy of tsdf; the sequence ends where count is called again.  The totals come
 * back like those of f3d_radius_graph_count_dev: through host pointers, after one synchronisation of the stream.  The _dev fill takes
 * the same tsdf and dims again, and so does f3d_tsdf_extract_colors_dev.  Either output of fill may be NULL.
 * F3D_ERR_INVALID, with nothing written (but for the one case named last): NULLs; non-positive dims or a product >= 2^31; vs, trunc, depth_scale or max_depth not finite
 * and positive; max_weight outside [1, 2^24]; min_weight < 1 (or NaN); an unknown depth type; h, w <= 0 or nframes < 0; a fill without
 * its count, or with other dims; a count that finds 2^30 quads or more (known only after the passes have run: *nv and *nt are then 0 and
 * the sequence is ended).  Non-finite depths or poses are no error: they contribute nothing.  nframes == 0 is a no-op; a volume
 * without an active cell gives nv = nt = 0.  The colour entries add: a NULL color or rgb; hc or wc_img <= 0 or hc * wc_img >= 2^31; a
 * device color that is not 16-byte aligned; f3d_tsdf_extract_colors without its count or with other dims.  nv == 0 is a no-op there.
 * Scratch: 11 bytes per voxel + 4 per scan tile; f3d_ctx_reserve_tsdf(nvoxels) sizes it, and a strict context then allocates nothing in
 * the three _dev entries.  Reserving may move the scratch, so it ends a counted sequence: count again before the fill.
 * f3d_debug_tsdf_grid_cap (test hook): blocks > 0 caps the grid of every grid-stride TSDF launch of the context at that many blocks, so that
 * a small volume takes many passes per block; 0 = the library's launch shapes.  No result depends on it.
 * f3d_debug_grid_cap (test hook): the same for every other grid-stride launch of the library, and for the TSDF and raycast launches as
 * well (they take the smaller of the two caps).  The state belongs to the PROCESS, not to ctx: it holds for every context and every
 * thread until it is set back to 0.  It only ever lowers a grid, never below one block.  f3d_debug_grid_cap_stats reads and resets two
 * process-wide counters: out[0] = grids sized while the cap was on, out[1] = those the cap made smaller.  No result depends on either.
 * f3d_debug_poison (test hook): drains the context's stream, fills every allocated scratch, staging and kept buffer of ctx over its whole
 * capacity with `byte` (0..255), and with them the members that hold nothing between calls (the filter list, the relabel counter, the
 * batched vote's first-bad word, the point vote's words, the vote set, which the next batched vote then clears), and drains the stream
 * again; out[0] = buffers filled, out[1] = bytes filled.  The sticky device error word and the code book keep their contents.  It ends
 * every counted sequence of the context (radius graph, radius query, group -> extremes -> hull filter, TSDF extract): their fill passes
 * then ask for the count pass, as after any other interruption.  F3D_ERR_INVALID: a byte outside [0, 255], out == NULL, or a
 * view-chunked fused call in progress (nothing is filled).  It reads no environment variable and no entry looks at it: no result of a
 * later call may depend on the byte. */
#define F3D_TSDF_SCAN_TILE 2048
#define F3D_TSDF_MAX_WEIGHT 16777216.0f
int f3d_tsdf_integrate(f3d_ctx* ctx, float* tsdf, float* weight, int nx, int ny, int nz, const double lo[3], double vs, double trunc,
                       float max_weight, const void* depth, int depth_type, int nframes, int h, int w, double depth_scale,
                       double max_depth, const f3d_view* views);
int f3d_tsdf_integrate_dev(f3d_ctx* ctx, float* tsdf, float* weight, int nx, int ny, int nz, const double lo[3] /*host*/, double vs,
                           double trunc, float max_weight, const void* depth, int depth_type, int nframes, int h, int w,
                           double depth_scale, double max_depth, const f3d_view* views_dev /*device [F]*/, void* stream);
int f3d_tsdf_extract_count(f3d_ctx* ctx, const float* tsdf, const float* weight, int nx, int ny, int nz, float min_weight, int64_t* nv,
                           int64_t* nt);
int f3d_tsdf_extract_fill(f3d_ctx* ctx, int nx, int ny, int nz, const double lo[3], double vs, double* verts /*[nv,3]*/,
                          int32_t* tris /*[nt,3]*/);
int f3d_tsdf_extract_count_dev(f3d_ctx* ctx, const float* tsdf, const float* weight, int nx, int ny, int nz, float min_weight,
                               int64_t* nv /*host*/, int64_t* nt /*host*/, void* stream);
int f3d_tsdf_extract_fill_dev(f3d_ctx* ctx, const float* tsdf, int nx, int ny, int nz, const double lo[3] /*host*/, double vs,
                              double* verts, int32_t* tris, void* stream);
int f3d_tsdf_integrate_color(f3d_ctx* ctx, float* tsdf, float* weight, float* color /*[nz,ny,nx,4]*/, int nx, int ny, int nz,
                             const double lo[3], double vs, double trunc, float max_weight, const void* depth, int depth_type,
                             const uint8_t* rgb /*[F,hc,wc_img,3]*/, int nframes, int h, int w, int hc, int wc_img, double depth_scale,
                             double max_depth, const f3d_view* views);
int f3d_tsdf_integrate_color_dev(f3d_ctx* ctx, float* tsdf, float* weight, float* color, int nx, int ny, int nz,
                                 const double lo[3] /*host*/, double vs, double trunc, float max_weight, const void* depth, int depth_type,
                                 const uint8_t* rgb, int nframes, int h, int w, int hc, int wc_img, double depth_scale, double max_depth,
                                 const f3d_view* views_dev /*device [F]*/, void* stream);
int f3d_tsdf_extract_colors(f3d_ctx* ctx, const float* color, int nx, int ny, int nz, uint8_t* rgb /*[nv,3]*/,
                            uint8_t* colored /*[nv] or NULL*/);
int f3d_tsdf_extract_colors_dev(f3d_ctx* ctx, const float* tsdf, const float* color, int nx, int ny, int nz, uint8_t* rgb,
                                uint8_t* colored, void* stream);
int f3d_ctx_reserve_tsdf(f3d_ctx* ctx, int64_t nvoxels);
int f3d_debug_tsdf_grid_cap(f3d_ctx* ctx, int blocks);
int f3d_debug_grid_cap(f3d_ctx* ctx, int blocks);
int f3d_debug_grid_cap_stats(f3d_ctx* ctx, int64_t out[2]);
int f3d_debug_poison(f3d_ctx* ctx, int byte, int64_t out[2]);

/* ---- feature fusion: per-point pooling of per-pixel feature maps over views (no reference counterpart) -------------------- */
/* Every other 2D -> 3D entry moves one byte per pixel (a class or an instance id).  These move a vector: the [C] logits or
 * probabilities of the 2D network (soft votes), or a per-pixel embedding that is compared with text embeddings afterwards.  The
 * geometry is that of the occlusion-aware forward vote above: the same samples, the same keys, the same visibility rule.
 *   inputs     xyz [n, 3] F3D_F64 or F3D_F32, n < 2^31; views [V] from f3d_views_build; h, w > 0: the image size at which the samples
 *              and the z-buffer are taken; feats [V, hf, wf, d], channel-last and C-contiguous, of type ftype (F3D_FEAT_F16: IEEE
 *              binary16, F3D_FEAT_F32); hf, wf >= 1 are independent of h, w, hf * wf < 2^31; 1 <= d <= 4096; splat in [0, 8];
 *              depth_tol >= 0, +inf allowed; sums float32 [n, d] and counts int32 [n], both updated IN PLACE (a fresh
 *              accumulation starts from zeros: the caller zeroes them); views_per_pass >= 0 as in f3d_vote_visible.
 *   sample     the sample (u, v, z32) of (point i, view j) is exactly that of f3d_vote_visible.  It is visible iff
 *              (double)z32 <= (double)zmin32 + depth_tol, zmin32 = the depth of cell (j, v, u) of the splat z-buffer of this very
 *              cloud.  With depth_tol = +inf every sample is visible and the z-buffer passes are skipped.
 *   pixel      the feature pixel of a sample is uf = (int64)u * wf / w, vf = (int64)v * hf / h (the nearest rule of
 *              segUtils/voting.py resize_nearest); it is in range by construction.
 *   sum        for the views of the call in ascending j, for every visible sample (i, j):
 *                sums[i, c] = (float)(sums[i, c] + (float)feats[j, vf, uf, c]) for every c (one float32 add; the binary16 -> float32
 *                conversion is exact), counts[i] += 1.
 *              No float atomics: a point's adds happen in ascending view order whatever the launch shape, so nothing in the result
 *              depends on thread timing, on views_per_pass or on how the caller splits the views over calls: two calls over views
 *              [0, a) and [a, V) equal one call over [0, V) bit for bit.  A point without a visible sample keeps its row.
 *   finalize   f3d_features_finalize(sums, counts, n, d, normalize, out): m_c = sums[i, c] / (float)counts[i], the correctly rounded
 *              float32 quotient; a row of zeros when counts[i] <= 0.  With normalize != 0: s = sum_c (double)m_c * (double)m_c in
 *              float64 (in any order), out[i, c] = (float)((double)m_c / sqrt(s)), zeros when s == 0.  out float32 [n, d]; out == sums
 *              is allowed.
 * Scratch: only the depth keys of a pass, so f3d_ctx_reserve_render(n, nviews, h, w) sizes it and a strict context then allocates
 * nothing in f3d_fuse_features_dev with views_per_pass = 0 (or any smaller pass); f3d_features_finalize_dev needs none.
 * F3D_ERR_INVALID: the bad arguments of f3d_vote_visible, hf or wf < 1, hf * wf >= 2^31, d outside [1, 4096], an unknown ftype, a
 * NULL array that is needed.  There is no device error: nothing is indexed by data.  n == 0 or V == 0 is a no-op. */
typedef enum f3d_ftype {
    F3D_FEAT_F16 = 0,             /* IEEE binary16 feature maps                                   */
    F3D_FEAT_F32 = 1              /* float32 feature maps                                         */
} f3d_ftype;
int f3d_fuse_features(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views, int nviews, int h, int w,
                      const void* feats /*[V,hf,wf,d]*/, f3d_ftype ftype, int hf, int wf, int d, int splat, double depth_tol,
                      float* sums /*[n,d], in place*/, int32_t* counts /*[n], in place*/, int views_per_pass);
int f3d_fuse_features_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views_dev /*device [V]*/, int nviews,
                          int h, int w, const void* feats, f3d_ftype ftype, int hf, int wf, int d, int splat, double depth_tol,
                          float* sums, int32_t* counts, int views_per_pass, void* stream);
int f3d_features_finalize(f3d_ctx* ctx, const float* sums, const int32_t* counts, int64_t n, int d, int normalize, float* out);
int f3d_features_finalize_dev(f3d_ctx* ctx, const float* sums, const int32_t* counts, int64_t n, int d, int normalize, float* out,
                              void* stream);

/* ---- registration: TSDF raycast and point-to-plane ICP pose refinement (no reference counterpart) -------------------------- */
/* Every other entry takes its camera poses as given.  These produce one: ray-cast the TSDF volume from a pose into a vertex map and a
 * normal map (the model), align a depth frame to the maps by projective point-to-plane ICP, integrate the frame at the refined pose:
 * frame-to-model tracking.  All arithmetic is float64 without contraction, every product, sum, division and sqrt as written; there is
 * no sin, cos or atan in the contract.  dot(a, b) = (a0*b0 + a1*b1) + a2*b2; cross(a, b) = (a1*b2 - a2*b1, a2*b0 - a0*b2,
 * a0*b1 - a1*b0); rotate is f3d_rotate_f64's q p conj(q), project_h the homogeneous pixel of f3d_tsdf_integrate's step 1.
 *   pixels     the convention of the TSDF, not that of f3d_unproject_depth: f3d_tsdf_integrate gives the depth of pixel (u, v) to
 *              everything that projects into [u, u+1) x [v, v+1), so a pixel stands for the ray through (u + 0.5, v + 0.5).  With
 *              fx = K[0], cx = K[2], fy = K[4], cy = K[5] (the other entries of K are not read) the camera-frame ray of a pixel is
 *              dc = (((double)u + 0.5 - cx) / fx, ((double)v + 0.5 - cy) / fy, 1.0).  f3d_unproject_depth keeps the reference's
 *              integer grid (the ray through (u, v)).
 *   quaternion a camera->world q (w, x, y, z) is normalised as qn = q / sqrt(((q0*q0 + q1*q1) + q2*q2) + q3*q3), by component
 *              division; a zero or non-finite quaternion is F3D_ERR_INVALID.
 * f3d_tsdf_raycast: model maps of the volume (tsdf, weight, dims, lo, vs, min_weight >= 1 as for extract) from the pose (q_wxyz, t)
 * for an h x w image; znear >= 0, step > 0, nsteps >= 1.  Outputs, each may be NULL: vertex float64 [h*w, 3] (world), normal
 * float64 [h*w, 3] (unit, world), depth float64 [h*w] (camera z).  A pixel without a hit gets NaN rows and depth 0.
 *   ray        dw = rotate(qn, dc); the point at parameter s is P_a(s) = t[a] + s * dw_a; dc.z = 1, so s is the camera-z depth.
 *   F(P)       g_a = (P_a - lo[a]) / vs - 0.5, i_a = floor(g_a).  The sample is valid iff 0 <= i_a <= n_a - 2 on all axes (NaN
 *              fails) and all 8 corner weights are >= min_weight.  f_a = g_a - (double)i_a.  With the corner samples T_ijk
 *              (offsets i, j, k in {0, 1} along x, y, z) widened to double: c_jk = T0jk + f_x * (T1jk - T0jk);
 *              c_k = c_0k + f_y * (c_1k - c_0k); F = c_0 + f_z * (c_1 - c_0).
 *   march      s_k = znear + (double)k * step, k = 0 .. nsteps-1 (no running sum).  The ray ends at the first valid sample with
 *              F_k < 0 (+0.0 and -0.0 are outside, as in extract).  It is a hit iff k >= 1 and sample k-1 was valid with
 *              F_{k-1} >= 0; then s* = s_{k-1} + step * (F_{k-1} / (F_{k-1} - F_k)).  Otherwise (the ray entered the surface from
 *              behind or from unobserved space, or never ended) it is no hit.
 *   normal     V = P(s*); G_a = F(V + vs e_a) - F(V - vs e_a), e_a the unit axis vector (the other two coordinates are V's own).  Any of
 *              the six samples invalid: no hit.  len = sqrt((G0*G0 + G1*G1) + G2*G2); len == 0 or not finite: no hit.
 *              normal = G / len: the stored TSDF is positive in front of the surface, so the normal points out of it, towards where
 *              the cameras were.  vertex = V, depth = s*.
 * The kernel skips samples that the index rule above calls invalid (a slab test of the ray against the volume with a wide margin);
 * no bit of the output depends on that, on the launch shape or on f3d_debug_tsdf_grid_cap, which caps this launch too.
 * f3d_icp_sums: one linearisation of the alignment of a source depth frame (depth, depth_type, h, w, K, depth_scale, max_depth as in
 * f3d_tsdf_integrate, one frame) at the source pose (q_wxyz, t) to the model maps model_vertex, model_normal float64 [hm*wm, 3]
 * (world frame, NaN = missing; usually from f3d_tsdf_raycast, or from another frame through f3d_unproject_depth and
 * f3d_estimate_normals) seen by the model camera model_view (one record of f3d_views_build for an hm x wm image; its planes play no
 * part).  max_dist > 0.  Per source pixel i = v*w + u; a pixel that fails a step contributes 0.0 to every sum:
 *   1. d = (double)raw / depth_scale; d > 0 && d <= max_depth.
 *   2. c = (((double)u + 0.5 - cx) * (d / fx), ((double)v + 0.5 - cy) * (d / fy), d); pr = rotate(qn, c); p = pr + t.
 *   3. (h0, h1, h2) = project_h(Km, qinv_m, t_m, p); h2 > 0; x = h0 / h2, y = h1 / h2; 0 <= x < wm and 0 <= y < hm;
 *      um = (int)floor(x), vm = (int)floor(y).
 *   4. V, N = the model rows at vm*wm + um; all six values finite.
 *   5. e = p - V; (e0*e0 + e1*e1) + e2*e2 <= max_dist * max_dist.
 *   6. r = dot(N, e); J = (cross(pr, N), N): the increment rotates about the current camera centre, which keeps the system well
 *      conditioned for clouds far from the origin.
 *   7. the F3D_ICP_NSUMS = 29 terms: the 21 products J_a * J_b, a <= b, row-major; the 6 products J_a * r; r * r; 1.0.
 * Each of the 29 sums runs over the pixel indices 0 .. h*w-1 in chunks of F3D_ICP_CHUNK pixels.  A chunk sum: lane l of 64 adds the
 * chunk's items l, l + 64, .. left to right from 0.0, then the 64 lane sums meet in an xor butterfly 32, 16, .., 1
 * (acc = acc + acc[lane ^ off]).  The total is the same sum of all the chunk sums.  Output: sums float64 [29].
 * f3d_icp: iterations >= 1 rounds of that on the device, with no host synchronisation in the _dev entry; min_pairs >= 6.  Each round,
 * at the current pose (q, t):
 *   totals     as above; count = the last total.  count < min_pairs: the status becomes F3D_ICP_LOST.
 *   solve      A = the symmetric 6 x 6 matrix of the 21 sums, b_a = -(sum J_a r), maxd = the largest A_aa.  Cholesky A = L L^T, column by
 *              column: for j = 0 .. 5: s = A_jj; s = s - L_jk * L_jk for k = 0 .. j-1; the pivot s must be finite and
 *              > F3D_ICP_PIVOT_EPS * maxd, otherwise the status becomes F3D_ICP_LOST; L_jj = sqrt(s); for i = j+1 .. 5: e = A_ij;
 *              e = e - L_ik * L_jk for k = 0 .. j-1; L_ij = e / L_jj.  Forward: for i = 0 .. 5: s = b_i; s = s - L_ik * y_k for
 *              k = 0 .. i-1; y_i = s / L_ii.  Back: for i = 5 .. 0: s = y_i; s = s - L_ki * x_k for k = i+1 .. 5; x_i = s / L_ii.
 *              x = (omega, v).  F3D_ICP_PIVOT_EPS guards against a degenerate scene; it is not a tuning value.
 *   update     dq = (1, omega0 / 2, omega1 / 2, omega2 / 2); q' = dq (x) qn, the Hamilton product, each component left to right:
 *              w = ((a0*b0 - a1*b1) - a2*b2) - a3*b3, x = ((a0*b1 + a1*b0) + a2*b3) - a3*b2, y = ((a0*b2 - a1*b3) + a2*b0) + a3*b1,
 *              z = ((a0*b3 + a1*b2) - a2*b1) + a3*b0 with a = dq, b = qn; q' is normalised as above; t' = t + v.
 *   once lost  the pose stays as it was at the start of that round and the remaining rounds do nothing.
 * Outputs: pose float64 [7] = q', t'; stats float64 [iterations, 3] = {count, sum r*r, status} per round, measured before that
 * round's update; rows after a lost round are {0, 0, 1}; status = the final F3D_ICP_OK / F3D_ICP_LOST (int32; a device word in the _dev
 * entry, may be NULL there).
 * Scratch: the chunk sums [nchunks, 29], the pose and the lost flag (the 29 totals of a round stay in LDS);
 * f3d_ctx_reserve_icp(npixels) sizes it, and a strict context then allocates nothing in the _dev entries.  The raycast needs none.
 * F3D_ERR_INVALID, with nothing written: NULLs (but for the optional outputs); non-positive sizes; h*w or hm*wm >= 2^31; the bad volume
 * arguments of extract; vs, step, depth_scale, max_depth or max_dist not finite and positive; znear negative or not finite;
 * nsteps < 1; iterations < 1; min_pairs < 6; a non-finite K, t or lo; a zero or non-finite quaternion; an unknown depth type. */
#define F3D_ICP_CHUNK 256
#define F3D_ICP_NSUMS 29
#define F3D_ICP_PIVOT_EPS 1e-10
#define F3D_ICP_OK 0
#define F3D_ICP_LOST 1
int f3d_tsdf_raycast(f3d_ctx* ctx, const float* tsdf, const float* weight, int nx, int ny, int nz, const double lo[3], double vs,
                     float min_weight, const double K[9], const double q_wxyz[4], const double t[3], int h, int w, double znear,
                     double step, int nsteps, double* vertex /*[h*w,3]*/, double* normal /*[h*w,3]*/, double* depth /*[h*w]*/);
int f3d_tsdf_raycast_dev(f3d_ctx* ctx, const float* tsdf, const float* weight, int nx, int ny, int nz, const double lo[3] /*host*/,
                         double vs, float min_weight, const double K[9] /*host*/, const double q_wxyz[4] /*host*/,
                         const double t[3] /*host*/, int h, int w, double znear, double step, int nsteps, double* vertex,
                         double* normal, double* depth, void* stream);
int f3d_icp_sums(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9], double depth_scale, double max_depth,
                 const double q_wxyz[4], const double t[3], const double* model_vertex, const double* model_normal, int hm, int wm,
                 const f3d_view* model_view, double max_dist, double* sums /*[29]*/);
int f3d_icp_sums_dev(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9] /*host*/, double depth_scale,
                     double max_depth, const double q_wxyz[4] /*host*/, const double t[3] /*host*/, const double* model_vertex,
                     const double* model_normal, int hm, int wm, const f3d_view* model_view /*device*/, double max_dist,
                     double* sums, void* stream);
int f3d_icp(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9], double depth_scale, double max_depth,
            const double q_wxyz[4], const double t[3], const double* model_vertex, const double* model_normal, int hm, int wm,
            const f3d_view* model_view, double max_dist, int iterations, int min_pairs, double* pose /*[7]*/,
            double* stats /*[iterations,3]*/, int32_t* status);
int f3d_icp_dev(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9] /*host*/, double depth_scale,
                double max_depth, const double q_wxyz[4] /*host*/, const double t[3] /*host*/, const double* model_vertex,
                const double* model_normal, int hm, int wm, const f3d_view* model_view /*device*/, double max_dist, int iterations,
                int min_pairs, double* pose, double* stats, int32_t* status /*device, may be NULL*/, void* stream);
int f3d_ctx_reserve_icp(f3d_ctx* ctx, int64_t npixels);

/* Colour in registration: the volume's colour rendered along with its maps, and a photometric term in the ICP.  Depth cannot see a
 * motion that maps the geometry onto itself (along a wall, about the axis of a round object); the colour images can.  Everything
 * above holds: float64 without contraction, every product, sum and division as written.
 * f3d_tsdf_raycast_color: the arguments of f3d_tsdf_raycast plus color float32 [nz, ny, nx, 4], the state of
 * f3d_tsdf_integrate_color (a device pointer must be 16-byte aligned), and two more optional outputs: rgb float64 [h*w, 3] on the
 * 0..255 scale and intensity float64 [h*w].  vertex, normal and depth are f3d_tsdf_raycast's, bit for bit.
 *   colour     for a hit at V: g, i, f as in F(P) at P = V.  The colour sample is valid iff the index rule of F(P) holds at V and all 8
 *              corners have wc > 0 (their TSDF weights play no part).  Per channel, with the corner values C_ijk widened to double:
 *              c_jk = C0jk + f_x * (C1jk - C0jk); c_k = c_0k + f_y * (c_1k - c_0k); value = c_0 + f_z * (c_1 - c_0).
 *   intensity  ((0.299 * R + 0.587 * G) + 0.114 * B) / 255.0.
 *   missing    a hit whose colour sample is invalid keeps its vertex, normal and depth and gets NaN in rgb and intensity; so does a
 *              pixel without a hit.
 * f3d_icp_color_sums: the arguments of f3d_icp_sums plus model_intensity float64 [hm*wm] (NaN = missing; f3d_tsdf_raycast_color's),
 * the source colour image rgb uint8 [hc, wc_img, 3] (hc, wc_img > 0 with a product < 2^31, of any size) and color_weight, finite and
 * >= 0 (read by f3d_icp_color only).  Steps 1 to 7 are unchanged and give the first 29 sums.  A pixel that passed step 5 contributes
 * a photometric pair as well iff all of this holds:
 *   source     uc = (int64)u * wc_img / w, vc = (int64)v * hc / h (the colour pixel of f3d_tsdf_integrate_color); Is = the intensity
 *              of that pixel's three bytes.
 *   model      a = x - 0.5, b = y - 0.5 with (x, y) of step 3; i0 = floor(a), j0 = floor(b); 0 <= i0 <= wm - 2 and 0 <= j0 <= hm - 2;
 *              fa = a - i0, fb = b - j0; the taps I00 = I[j0, i0], I10 = I[j0, i0+1], I01 = I[j0+1, i0], I11 = I[j0+1, i0+1] all
 *              finite.  top = I00 + fa * (I10 - I00); bot = I01 + fa * (I11 - I01); Im = top + fb * (bot - top); dx0 = I10 - I00,
 *              dx1 = I11 - I01; gx = dx0 + fb * (dx1 - dx0); gy = bot - top.
 *   residual   rc = Im - Is.
 *   gradient   with the rows K0, K1, K2 of the model view's K and h2 of step 3, for k = 0, 1, 2:
 *              gc_k = (gx * (K0k - x * K2k) + gy * (K1k - y * K2k)) / h2; gw = rotate(conj(qinv_m), gc), conj(q) = (q0, -q1, -q2, -q3).
 *   Jc         (cross(pr, gw), gw): the shape of J with gw in place of N.
 * The pair adds a second set of 29 terms after the first: the 21 products Jc_a * Jc_b, the 6 products Jc_a * rc, rc * rc, 1.0;
 * F3D_ICP_NSUMS_COLOR = 58 sums, each of the shape above.  Output: sums float64 [58].
 * f3d_icp_color: the rounds of f3d_icp with A = A_g + color_weight * A_c (entry by entry) and b_a = -(bg_a + color_weight * bc_a); the
 * lost rule uses the geometric count; Cholesky, the pivot rule, the update and "once lost" are f3d_icp's.  stats float64
 * [iterations, 5] = {count, sum r*r, status, colour count, sum rc*rc}; rows after a lost round are {0, 0, 1, 0, 0}.
 * Scratch: the chunk sums [nchunks, 58], the pose and the lost flag; f3d_ctx_reserve_icp_color(npixels) sizes it (and covers the
 * 29-sum entries), a strict context then allocates nothing in the _dev entries.  F3D_ERR_INVALID, with nothing written: the bad
 * arguments of f3d_tsdf_raycast / f3d_icp_sums / f3d_icp; a NULL color, model_intensity or rgb; a device color that is not 16-byte
 * aligned; hc or wc_img < 1 or hc * wc_img >= 2^31; a negative or non-finite color_weight.
 * Out of scope: robust weights, an intensity-difference gate, pyramids of the colour image, exposure compensation, colour from
 * anything but the volume. */
#define F3D_ICP_NSUMS_COLOR 58
int f3d_tsdf_raycast_color(f3d_ctx* ctx, const float* tsdf, const float* weight, const float* color /*[nz,ny,nx,4]*/, int nx, int ny, int nz,
                           const double lo[3], double vs, float min_weight, const double K[9], const double q_wxyz[4], const double t[3],
                           int h, int w, double znear, double step, int nsteps, double* vertex /*[h*w,3]*/, double* normal /*[h*w,3]*/,
                           double* depth /*[h*w]*/, double* rgb /*[h*w,3]*/, double* intensity /*[h*w]*/);
int f3d_tsdf_raycast_color_dev(f3d_ctx* ctx, const float* tsdf, const float* weight, const float* color, int nx, int ny, int nz,
                               const double lo[3] /*host*/, double vs, float min_weight, const double K[9] /*host*/,
                               const double q_wxyz[4] /*host*/, const double t[3] /*host*/, int h, int w, double znear, double step,
                               int nsteps, double* vertex, double* normal, double* depth, double* rgb, double* intensity, void* stream);
int f3d_icp_color_sums(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9], double depth_scale,
                       double max_depth, const double q_wxyz[4], const double t[3], const double* model_vertex, const double* model_normal,
                       int hm, int wm, const f3d_view* model_view, double max_dist, const double* model_intensity /*[hm*wm]*/,
                       const uint8_t* rgb /*[hc,wc_img,3]*/, int hc, int wc_img, double color_weight, double* sums /*[58]*/);
int f3d_icp_color_sums_dev(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9] /*host*/, double depth_scale,
                           double max_depth, const double q_wxyz[4] /*host*/, const double t[3] /*host*/, const double* model_vertex,
                           const double* model_normal, int hm, int wm, const f3d_view* model_view /*device*/, double max_dist,
                           const double* model_intensity, const uint8_t* rgb, int hc, int wc_img, double color_weight, double* sums,
                           void* stream);
int f3d_icp_color(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9], double depth_scale, double max_depth,
                  const double q_wxyz[4], const double t[3], const double* model_vertex, const double* model_normal, int hm, int wm,
                  const f3d_view* model_view, double max_dist, const double* model_intensity, const uint8_t* rgb, int hc, int wc_img,
                  double color_weight, int iterations, int min_pairs, double* pose /*[7]*/, double* stats /*[iterations,5]*/,
                  int32_t* status);
int f3d_icp_color_dev(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9] /*host*/, double depth_scale,
                      double max_depth, const double q_wxyz[4] /*host*/, const double t[3] /*host*/, const double* model_vertex,
                      const double* model_normal, int hm, int wm, const f3d_view* model_view /*device*/, double max_dist,
                      const double* model_intensity, const uint8_t* rgb, int hc, int wc_img, double color_weight, int iterations,
                      int min_pairs, double* pose, double* stats, int32_t* status /*device, may be NULL*/, void* stream);
int f3d_ctx_reserve_icp_color(f3d_ctx* ctx, int64_t npixels);

/* Coarse-to-fine registration: pyramids of the depth frame and of the model maps, and the rounds above run level after level.  At
 * full resolution, projective ICP on a surface with structure near the pixel scale (bricks, slats, shelves) slides into the
 * neighbouring period of that structure and still reports F3D_ICP_OK; a few rounds on half- and quarter-size averages put the pose
 * within the basin of the right one first.  Everything above holds: float64 without contraction, every sum, division and sqrt as written.
 * Both half-samplings give output pixel (u, v) of an h2 x w2 = (h / 2) x (w / 2) image (integer division: an odd last row or column is
 * dropped) from the four input pixels (2v, 2u), (2v, 2u+1), (2v+1, 2u), (2v+1, 2u+1), "the four" below, always in that order.
 *   intrinsics a pixel stands for the ray through (u + 0.5, v + 0.5), and the block of output pixel u covers [2u, 2u + 2) with its
 *              centre at 2(u + 0.5): input coordinate x is output coordinate x / 2, exactly, with no half-pixel term.  So the output's
 *              intrinsics are K' = (fx / 2, fy / 2, cx / 2, cy / 2): the first two rows of K divided by 2 (a division by 2 is exact),
 *              and ((u + 0.5) - cx') / fx' is the mean of the two input columns' ((u_in + 0.5) - cx) / fx up to rounding.
 * f3d_depth_half: depth, depth_type, h, w, depth_scale, max_depth as in f3d_icp_sums; gate > 0; h, w >= 2.  out float64 [h2*w2], metres.
 *   1. d = (double)raw / depth_scale for each of the four; a sample is valid iff d > 0 && d <= max_depth.
 *   2. dmin = the smallest valid d.
 *   3. a sample is used iff it is valid and d - dmin <= gate: at a silhouette the foreground wins and no depth is invented between
 *      two surfaces.
 *   4. out = sum / (double)count, the sum left to right from 0.0 over the used samples; no valid sample: out = 0.0.
 * The output is a depth frame of type F3D_DEPTH_F64 with depth_scale 1, for the next step and for the ICP.
 * f3d_maps_half: model_vertex, model_normal float64 [hm*wm, 3], model_intensity float64 [hm*wm] or NULL, model_view (one f3d_view for
 * the hm x wm image, as f3d_icp_sums takes it), gate > 0; hm, wm >= 2.  Outputs vertex_out, normal_out float64 [hm2*wm2, 3] and, iff
 * model_intensity is given, intensity_out float64 [hm2*wm2].
 *   1. a row of the four is usable iff its six values are finite and z = project_h(Km, qinv_m, t_m, V).h2 > 0.
 *   2. zmin = the smallest z of the usable rows.
 *   3. a row is used iff it is usable and z - zmin <= gate.
 *   4. vertex = S / (double)count per component, S the sum of the used vertices, left to right from 0.0.
 *   5. G = the sum of the used normals, likewise; len = sqrt((G0*G0 + G1*G1) + G2*G2); len == 0 or not finite: the vertex and normal rows
 *      are NaN; otherwise normal = G / len.
 *   6. intensity = the sum of the finite intensities of the used rows, left to right from 0.0, over their count; none: NaN (also where
 *      step 5 gave NaN rows).
 *   7. no usable row: every output is NaN.
 * The averages are why this is a step of its own: ray-casting the volume again at the coarse size point-samples the surface, which
 * aliases the very structure a coarse level is meant to smooth.  The output's model view is f3d_views_build of K' for hm2 x wm2.
 * f3d_icp_levels: the rounds of f3d_icp (rgb NULL) or f3d_icp_color (rgb given) over nlevels in [1, F3D_ICP_MAX_LEVELS] records, in
 * array order; the caller lists the coarsest first.  A record holds the source frame (depth, depth_type, h, w, K, depth_scale), the
 * model (model_vertex, model_normal, model_intensity or NULL, hm, wm, model_view) and max_dist, iterations >= 1, min_pairs >= 6 of
 * its level; max_depth, the start pose, the colour image (rgb, hc, wc_img: every level samples the full image by the pixel rule of
 * f3d_icp_color_sums) and color_weight belong to the call.  Either every level has a model_intensity and rgb is given, or none has
 * and rgb is NULL.  The records live on the host; in the _dev entry their pointers are device pointers.
 *   rounds     each round is exactly a round of f3d_icp / f3d_icp_color on its level's frame at the pose the round before left, across a
 *              level boundary too: there is no new arithmetic.
 *   once lost  covers the whole call: the pose stays as it was at the start of the lost round, every later round of every level writes
 *              {0, 0, 1} (five columns with colour: {0, 0, 1, 0, 0}).
 * Hence: nlevels = 1 equals f3d_icp / f3d_icp_color bit for bit; nlevels = n equals n calls of f3d_icp, each started from the pose the
 * call before returned, their stats rows concatenated, for as long as no call is lost.
 * Outputs: pose float64 [7]; stats float64 [sum of iterations, 3 or 5]; status as f3d_icp's.  Scratch: that of the level with the
 * most source pixels; f3d_ctx_reserve_icp(that count), or f3d_ctx_reserve_icp_color with colour, covers it and a strict context then
 * allocates nothing in the _dev entry.  The half-samplings need none.
 * F3D_ERR_INVALID, with nothing written: NULLs (but for model_intensity, intensity_out, rgb and the _dev status); h, w, hm or wm < 2 in
 * a half-sampling; gate not finite and positive; nlevels outside [1, F3D_ICP_MAX_LEVELS]; a level that f3d_icp would refuse; levels
 * with and without model_intensity in one call, or a mismatch between them and rgb; with rgb, the bad colour arguments of f3d_icp_color.
 * Out of scope: filters with more than the four taps, pyramids of the colour image, robust weights, damping. */
#define F3D_ICP_MAX_LEVELS 6
typedef struct f3d_icp_level {
    const void* depth;              /* the source frame of this level */
    int depth_type, h, w;
    double K[9];
    double depth_scale;
    const double* model_vertex;     /* [hm*wm, 3] */
    const double* model_normal;     /* [hm*wm, 3] */
    const double* model_intensity;  /* [hm*wm], or NULL in a call without colour */
    int hm, wm;
    const f3d_view* model_view;
    double max_dist;
    int iterations, min_pairs;
} f3d_icp_level;
int f3d_depth_half(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, double depth_scale, double max_depth, double gate,
                   double* out /*[(h/2)*(w/2)]*/);
int f3d_depth_half_dev(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, double depth_scale, double max_depth, double gate,
                       double* out, void* stream);
int f3d_maps_half(f3d_ctx* ctx, const double* model_vertex, const double* model_normal, const double* model_intensity /*may be NULL*/,
                  int hm, int wm, const f3d_view* model_view, double gate, double* vertex_out /*[(hm/2)*(wm/2),3]*/,
                  double* normal_out /*[(hm/2)*(wm/2),3]*/, double* intensity_out /*[(hm/2)*(wm/2)], NULL iff model_intensity is*/);
int f3d_maps_half_dev(f3d_ctx* ctx, const double* model_vertex, const double* model_normal, const double* model_intensity, int hm, int wm,
                      const f3d_view* model_view /*device*/, double gate, double* vertex_out, double* normal_out, double* intensity_out,
                      void* stream);
int f3d_icp_levels(f3d_ctx* ctx, const f3d_icp_level* levels /*host pointers inside*/, int nlevels, double max_depth,
                   const double q_wxyz[4], const double t[3], const uint8_t* rgb /*[hc,wc_img,3] or NULL*/, int hc, int wc_img,
                   double color_weight, double* pose /*[7]*/, double* stats /*[sum of iterations, 3 or 5]*/, int32_t* status);
int f3d_icp_levels_dev(f3d_ctx* ctx, const f3d_icp_level* levels /*host records, device pointers inside*/, int nlevels, double max_depth,
                       const double q_wxyz[4] /*host*/, const double t[3] /*host*/, const uint8_t* rgb, int hc, int wc_img,
                       double color_weight, double* pose, double* stats, int32_t* status /*device, may be NULL*/, void* stream);

/* Cloud-to-cloud ICP: the alignment of an unordered source cloud to an unordered target cloud in another frame.  f3d_icp pairs a
 * depth frame with model maps through a camera projection; here the partner of a source point is its nearest target point, found in
 * the target's radius grid (the grid and the exact walk of f3d_knn_query).  The pose (q_wxyz, t) maps source coordinates into the
 * target's frame.  All arithmetic is float64 without contraction, every operation rounded alone; dot, cross, rotate and the
 * quaternion normalisation are those of f3d_icp; float32 inputs are widened exactly.
 * f3d_cloud_icp_sums: one linearisation.  source [n, 3] of source_dtype, target [m, 3] of target_dtype, target_normals float64 [m, 3]
 * (F3D_CLOUD_ICP_PLANE; not read and may be NULL in F3D_CLOUD_ICP_POINT), max_dist > 0.  Per source point i; a point that fails a step
 * contributes 0.0 to every sum:
 *   1. pr = rotate(qn, s_i); p = pr + t.
 *   2. j = the target index that minimises (d2, j) lexicographically over the targets with d2 <= max_dist * max_dist, where
 *      e = p - T_j and d2 = (e0*e0 + e1*e1) + e2*e2: the predicate, the bits and the tie rule (the lower index wins) of f3d_knn_query
 *      with k = 1.  No such target: no pair.  pairs[i] = j or -1; it is written whenever a neighbour exists, also when step 3 then
 *      rejects the pair.
 *   3. F3D_CLOUD_ICP_PLANE: N = target_normals[j]; its three components must be finite, else no pair (the second nearest target is
 *      not tried).  r = dot(N, e); J = (cross(pr, N), N); the 29 terms of f3d_icp step 7.
 *   4. F3D_CLOUD_ICP_POINT: for a = 0, 1, 2 in that order N = the unit axis e_a, r = e[a], J = (cross(pr, e_a), e_a), and the 27
 *      products of each a are added to the accumulators in that order; 1.0 is added to the count once per pair.  (The terms that are
 *      +-0.0 by construction may be left out: no accumulator is ever -0.0.)
 * The sums run over the source indices 0 .. n-1 in chunks of F3D_ICP_CHUNK with the lane, butterfly and chunk layout of f3d_icp_sums;
 * no result depends on the launch shape, the cell order or thread timing.  Outputs: sums float64 [29]; pairs int32 [n] (may be NULL).
 * f3d_cloud_icp: iterations >= 1 rounds of that with the solve, the update, the lost rule, the stats rows and the status of f3d_icp,
 * unchanged; min_pairs >= 6 in both modes.  The increment rotates about t: a caller whose source lies far from its origin subtracts
 * the source's mean first and folds it back into t.  The target's grid (cell edge a hair above max_dist) is built once per call, and
 * there is one blocking readback per call (the target's box with the non-finite flag of the source); everything after it is
 * enqueued, in the _dev entries with no further host synchronisation.  n == 0: zero sums, and every round of f3d_cloud_icp is lost.
 * Scratch: the target's grid (as for f3d_knn_query), the chunk sums [ceil(n / 256), 29], the pose and the lost flag;
 * f3d_ctx_reserve_cloud_icp(m, n) sizes it for any radius, and a strict context then allocates nothing in the _dev entries.
 * F3D_ERR_INVALID, with nothing written: NULLs other than the optional outputs (source may be NULL when n == 0); PLANE mode without
 * normals; an unknown mode or dtype; m == 0; n or m >= 2^31; NaN or infinity in the source or the target; max_dist not finite and
 * positive, or >= 1e300; iterations < 1; min_pairs < 6; a zero or non-finite quaternion; a non-finite t. */
#define F3D_CLOUD_ICP_PLANE 0
#define F3D_CLOUD_ICP_POINT 1
int f3d_cloud_icp_sums(f3d_ctx* ctx, const void* source, f3d_dtype source_dtype, int64_t n, const void* target, f3d_dtype target_dtype,
                       int64_t m, const double* target_normals /*[m,3] or NULL*/, int mode, const double q_wxyz[4], const double t[3],
                       double max_dist, double* sums /*[29]*/, int32_t* pairs /*[n] or NULL*/);
int f3d_cloud_icp_sums_dev(f3d_ctx* ctx, const void* source, f3d_dtype source_dtype, int64_t n, const void* target,
                           f3d_dtype target_dtype, int64_t m, const double* target_normals, int mode, const double q_wxyz[4] /*host*/,
                           const double t[3] /*host*/, double max_dist, double* sums, int32_t* pairs, void* stream);
int f3d_cloud_icp(f3d_ctx* ctx, const void* source, f3d_dtype source_dtype, int64_t n, const void* target, f3d_dtype target_dtype,
                  int64_t m, const double* target_normals /*[m,3] or NULL*/, int mode, const double q_wxyz[4], const double t[3],
                  double max_dist, int iterations, int min_pairs, double* pose /*[7]*/, double* stats /*[iterations,3]*/,
                  int32_t* status);
int f3d_cloud_icp_dev(f3d_ctx* ctx, const void* source, f3d_dtype source_dtype, int64_t n, const void* target, f3d_dtype target_dtype,
                      int64_t m, const double* target_normals, int mode, const double q_wxyz[4] /*host*/, const double t[3] /*host*/,
                      double max_dist, int iterations, int min_pairs, double* pose, double* stats,
                      int32_t* status /*device, may be NULL*/, void* stream);
int f3d_ctx_reserve_cloud_icp(f3d_ctx* ctx, int64_t m, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* F3D_H */
