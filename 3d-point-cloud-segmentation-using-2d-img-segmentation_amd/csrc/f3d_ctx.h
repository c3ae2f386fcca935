// What every file of the C-ABI layer (f3d_ctx.cpp, f3d_capi.cpp) shares: the context, its scratch, staging and kept arenas, and
// the helpers with users in more than one of those files.  Internal: everything declared here has C++ linkage and hidden
// visibility; the exported names are those of include/f3d.h alone.
#pragma once
#include <hip/hip_runtime.h>
#include <initializer_list>
#include <vector>
#include <cstddef>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "f3d.h"
#include "f3d_kernels.h"
#include "f3d_math.h"

static_assert(sizeof(f3d_view) == 704, "f3d_view is 88 doubles");
static_assert(offsetof(f3d_view, t) == 72 && offsetof(f3d_view, mnorm) == 96, "the kernels stage M, t, mnorm as the record's first 15 doubles");
static_assert(offsetof(f3d_view, img_h) == offsetof(f3d_view, cull_n32) + 23 * 4, "cull planes, margins and image size: 24 consecutive floats");

#pragma clang fp contract(off)

// Device memory of a context, three kinds of buffer with a type each, so that a name of one kind does not compile where another
// is expected.  All grow on first use of a larger problem (grow()) and are refused growth by a strict context.
//   scratch_slot: the work area of a _dev entry (grids, sort buffers, coded masks, ...), one name per area; only _dev entries
//                 ensure() them, and f3d_ctx_reserve* sizes them.  Some hold state between two _dev calls (the grid between a count
//                 and its fill pass, the coded masks and the todo list of a view-chunked fused call).
//   staging:      the device copies of a host-pointer entry's arguments.  They have no names: the k-th buffer a call asks for
//                 is ctx->stage[k] (struct staging), and nothing in them outlives the call.
//   kept_slot:    what a host-pointer SEQUENCE leaves on the device for its next call, owned by that sequence alone
//                 (f3d_ctx::graph_kept, qry_kept, grp_cloud say whether they hold it).
enum scratch_slot { SLOT_OBB_BOXES = 0, SLOT_SORT_PERM, SLOT_SORT_SCRATCH, SLOT_TILED_MASKS, SLOT_TODO, SLOT_GRAPH, SLOT_GRAPH_BBOX,
                    SLOT_PATCH, SLOT_GRP_SCRATCH, SLOT_OBB_TABLE, SLOT_OBB_FACETS, SLOT_OBB_CAND, SLOT_FUSE_TABLES, SLOT_FUSE_CARRY,
                    SLOT_FUSE_XYZ, SLOT_FUSION, SLOT_PATCH_STATUS, SLOT_NRM, SLOT_NRM_CAMS, SLOT_QRY, SLOT_FLOOD, SLOT_COLOR,
                    SLOT_CVS_INST, SLOT_CVS_STATS, SLOT_QUADS, SLOT_GROW, SLOT_PVOTE, SLOT_PVOTE_BITS, SLOT_MESH, SLOT_ZKEY,
                    SLOT_ZCOUNTS, SLOT_KNN, SLOT_KNN_FLAG, SLOT_PLANES, SLOT_RASTER, SLOT_ZLUT, SLOT_SMOOTH, SLOT_FACE_GRAPH, SLOT_LIFT, SLOT_LIFT_TABLE,
                    SLOT_TSDF, SLOT_ICP, SLOT_COUNT };
enum kept_slot { KEPT_GRAPH_OFFS = 0,                                      // f3d_radius_graph_count -> _fill: the offsets
                 KEPT_QRY_IN, KEPT_QRY_OFFS,                               // f3d_radius_query_count -> _fill: the queries, the offsets
                 KEPT_GRP_ORDER, KEPT_GRP_KEYS, KEPT_GRP_STARTS,           // f3d_group_by_id -> f3d_obb_extremes -> f3d_obb_hull_filter
                 KEPT_GRP_XYZ,                                             //   ... and, from the extremes call on, the cloud
                 KEPT_TSDF,                                                // f3d_tsdf_extract_count -> _fill: the samples
                 KEPT_COUNT };
enum { STAGE_MAX = 9,                                                      // staging buffers of one call: f3d_patch_match and f3d_door_window_quads take 9
       BACK_MAX = 5 };                                                     // outputs one call copies back: f3d_mesh_clean has 5

struct devbuf { void* p; size_t cap; };

struct f3d_ctx {
    int device;
    hipStream_t stream;
    char err[512];
    devbuf scratch[SLOT_COUNT];
    devbuf stage[STAGE_MAX];
    devbuf kept[KEPT_COUNT];
    int* dev_err;                       // sticky device error word: one bit per operation (F3D_DEVERR_*)
    int strict;                         // 1: a scratch buffer that would have to grow is F3D_ERR_NOMEM (allocation-free _dev calls)
    long long allocs;                   // device allocations made by this context so far (f3d_ctx_alloc_count)
    unsigned long long* table;          // open-addressing set of the uv2pt vote
    size_t table_slots;
    unsigned vote_gen;                  // generation stamp of the batched vote's set entries (the set is cleared when it wraps)
    bool table_stamped;                 // the table holds generation-stamped entries only (else: clear before a batched call)
    int* first_bad;                     // device int: first frame of the current batched call with an out-of-range index
    int* filter_dev;                    // filter_classes of the call being enqueued (device copy)
    int32_t filter_host[F3D_MAX_FILTER];  // its staging copy: must outlive the asynchronous upload
    unsigned long long* count_dev;
    f3d_codebook* codebook;             // vote-bin code book of the fused path (device)
    f3d_fuse_occupancy fuse_occ;        // blocks per CU of the k_fuse instances launched so far (asked of the runtime once each)
    // radius graph: the search of the last count pass (the fill pass must follow it for the same cloud); graph_kept: that pass was
    // f3d_radius_graph_count, whose offsets KEPT_GRAPH_OFFS holds
    f3d_gridsearch graph;
    int64_t graph_n;
    bool graph_kept;
    // radius query: the search of the last count pass, its grid in SLOT_QRY, for the fill pass of the same queries; qry_kept: that
    // pass was f3d_radius_query_count, whose queries and offsets KEPT_QRY_IN / KEPT_QRY_OFFS hold
    f3d_gridsearch qry;
    int64_t qry_m, qry_n;
    int qry_qdtype;
    const void* qry_queries;
    bool qry_kept;
    // point vote: device int[4] of the call being enqueued (f3d_kernels.h); pv_partial: the last call stopped at a frame with
    // non-finite queries after applying the frames before it (the host-pointer entry still copies the votes back)
    int* pv_words;
    int pv_partial;
    // instance grouping of the last f3d_group_by_id call (host-pointer sequence group -> extremes -> hull filter), in KEPT_GRP_*;
    // grp_cloud: f3d_obb_extremes has run for this grouping and left its cloud (of grp_dtype) in KEPT_GRP_XYZ
    int64_t grp_n, grp_nids;
    int grp_dtype;
    bool grp_cloud;
    // TSDF extract: dims and totals of the last count pass (tsdf_n = -1: none), its codes, ranks and offsets in SLOT_TSDF; tsdf_kept: that
    // pass was f3d_tsdf_extract_count, whose samples KEPT_TSDF holds
    int64_t tsdf_n, tsdf_nv, tsdf_nq;
    int tsdf_dims[3];
    bool tsdf_kept;
    unsigned long long tsdf_counts[2];  // readback target of the count pass
    int tsdf_grid_cap;                  // f3d_debug_tsdf_grid_cap (0 = the library's launch shapes)
    // view-chunked fused call in progress (f3d_fuse_chunked_begin_dev .. the chunk with v_end == nviews)
    struct { int active, next, nviews, h, w, nclasses, gather; int64_t n; const int32_t* perm; const void* xyz; f3d_fuse_todo lay; } chunk;
};

#pragma GCC visibility push(hidden)

int fail(f3d_ctx* ctx, int code, const char* fmt, ...);

#define F3D_HIP(ctx, call)                                                                               \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess) return fail(ctx, e_ == hipErrorOutOfMemory ? F3D_ERR_NOMEM : F3D_ERR_HIP,  \
                                          "%s: %s", #call, hipGetErrorString(e_));                       \
    } while (0)

// One buffer of the context with room for `bytes`: it grows (with 1/8 of headroom) when it is too small, which a strict context refuses.
int grow(f3d_ctx* ctx, devbuf* b, size_t bytes, const char* kind, int index, void** out);

inline int ensure(f3d_ctx* ctx, scratch_slot s, size_t bytes, void** out) { return grow(ctx, &ctx->scratch[s], bytes, "scratch", s, out); }

inline bool dtype_ok(int dt) { return dt == F3D_F64 || dt == F3D_F32; }

inline hipStream_t pick(f3d_ctx* ctx, void* stream) { return stream ? (hipStream_t)stream : ctx->stream; }

int enter(f3d_ctx* ctx);

inline size_t xyz_bytes(f3d_dtype dt, int64_t n) { return (size_t)n * 3 * (dt == F3D_F64 ? 8 : 4); }

int make_filter(f3d_ctx* ctx, const int32_t* filter, int nfilter, int ncols, bool cols_must_exist, hipStream_t s,
                f3d_filter_args* fa);

// Reads the sticky device error word and consumes the bits in `mask` (each operation owns one bit, so that an error
// recorded by one operation is never blamed on, or silently skips, another one that shares the context).
int take_error(f3d_ctx* ctx, hipStream_t s, int mask = F3D_DEVERR_ALL);
// the message take_error reports for `bits` (F3D_DEVERR_*): that of the first of them in its table, NULL for none
const char* device_error_message(int bits);

// One call of an entry without "_dev" (include/f3d.h): inputs are copied into the context's staging buffers as they are staged, on
// the context's stream; outputs are copied back by finish(), which returns after the stream has drained, so no two calls' staging
// is alive at once and the k-th buffer a call asks for is simply ctx->stage[k].  The first failed allocation or copy stays in `rc`
// and turns every later step into a no-op.  A NULL host pointer is not copied: a NULL output is not wanted (its buffer is passed
// over, NULL device pointer), a NULL input (an optional one) leaves its buffer uninitialised.
struct staging {
    f3d_ctx* ctx;
    int rc = F3D_OK;
    struct { void* host; const void* dev; size_t bytes; } back_[BACK_MAX];
    int nback = 0, next = 0;

    explicit staging(f3d_ctx* c) : ctx(c) {}
    void* slot(size_t bytes) {
        void* p = nullptr;
        if (!rc && next >= STAGE_MAX) rc = fail(ctx, F3D_ERR_INVALID, "staging: more than %d buffers", STAGE_MAX);
        if (!rc) { rc = grow(ctx, &ctx->stage[next], bytes, "staging", next, &p); ++next; }
        return p;
    }
    // what a host-pointer sequence leaves for its next call: a buffer of the sequence's own instead of a staging buffer
    void* keep(kept_slot k, size_t bytes) {
        void* p = nullptr;
        if (!rc) rc = grow(ctx, &ctx->kept[k], bytes, "kept", k, &p);
        return p;
    }
    void put(void* dev, const void* host, size_t bytes) { if (!rc && host && bytes) rc = h2d(dev, host, bytes); }
    void back(void* host, const void* dev, size_t bytes) {
        if (!host || !bytes || rc) return;
        if (nback == BACK_MAX) { rc = fail(ctx, F3D_ERR_INVALID, "staging: more than %d outputs", BACK_MAX); return; }
        back_[nback++] = {host, dev, bytes};
    }
    template <class T> T* in(const T* host, size_t bytes) {
        void* p = slot(bytes);
        put(p, host, bytes);
        return (T*)p;
    }
    template <class T> T* out(T* host, size_t bytes) {
        if (!host) { ++next; return nullptr; }                 // (a call's buffers keep their positions whatever it leaves out)
        T* p = (T*)slot(bytes);
        back(host, p, bytes);
        return p;
    }
    template <class T> T* inout(T* host, size_t bytes) {
        T* p = in(host, bytes);
        back(host, p, bytes);
        return p;
    }
    // Consumes the device-error bits in `mask` before the copies back (an IndexError writes nothing), or after them with
    // `keep_partial` (what was applied before the error stays applied, as NumPy leaves it).
    int finish(int mask = 0, bool keep_partial = false) {
        if (rc) return rc;
        hipStream_t s = ctx->stream;
        if (mask && !keep_partial && (rc = take_error(ctx, s, mask))) return rc;
        for (int k = 0; k < nback; ++k) F3D_HIP(ctx, hipMemcpyAsync(back_[k].host, back_[k].dev, back_[k].bytes, hipMemcpyDeviceToHost, s));
        F3D_HIP(ctx, hipStreamSynchronize(s));
        return mask && keep_partial ? take_error(ctx, s, mask) : F3D_OK;
    }

  private:
    int h2d(void* dev, const void* host, size_t bytes) {
        F3D_HIP(ctx, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
        return F3D_OK;
    }
};

// cell edge of a neighbour grid over a box of extent `ext`: a hair above the radius (two points within it are then provably in adjacent
// cells whatever the rounding of the cell index), grown by 1.25 until fits(cells per axis) holds; dim receives the cells per axis
template <typename Fits>
double neighbour_cell(double radius, const double ext[3], int dim[3], Fits fits) {
    for (double cell = radius * 1.000001 + 1e-300;; cell *= 1.25) {
        double d[3];
        for (int c = 0; c < 3; ++c) d[c] = floor(ext[c] / cell) + 1.0;
        if (fits(d)) { for (int c = 0; c < 3; ++c) dim[c] = (int)d[c]; return cell; }
    }
}

int ensure_table(f3d_ctx* ctx, int64_t hw);                                  // (f3d_capi.cpp, with the vote)

// What every f3d_ctx_reserve* does after its argument check: sizes the listed scratch buffers (an entry with wanted == false is
// passed over) and, with table_hw > 0, the vote table for frames of that many pixels.  Reserving is the one thing a strict context
// may allocate for: strict is lifted here and back in place on every path.
struct reservation { scratch_slot s; size_t bytes; bool wanted = true; };

int reserve(f3d_ctx* ctx, std::initializer_list<reservation> list, int64_t table_hw = 0);

#pragma GCC visibility pop
