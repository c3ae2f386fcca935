// The context of libf3d_hip.so's C-ABI layer (include/f3d.h): its entries, the scratch, staging and kept arenas, the decoding of the
// device error word and the other helpers f3d_ctx.h declares.  No CPU fallback: every compute entry point needs a HIP device.
#include "f3d_ctx.h"

static thread_local char g_create_err[512] = "";

int fail(f3d_ctx* ctx, int code, const char* fmt, ...) {
    char* dst = ctx ? ctx->err : g_create_err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
    return code;
}

// One buffer of the context with room for `bytes`: it grows (with 1/8 of headroom) when it is too small, which a strict context refuses.
int grow(f3d_ctx* ctx, devbuf* b, size_t bytes, const char* kind, int index, void** out) {
    if (bytes == 0) bytes = 16;
    if (b->cap < bytes) {
        if (ctx->strict)
            return fail(ctx, F3D_ERR_NOMEM, "strict context: %s buffer %d holds %zu bytes, %zu needed (f3d_ctx_reserve first)", kind, index, b->cap, bytes);
        if (b->p) { F3D_HIP(ctx, hipFree(b->p)); b->p = nullptr; b->cap = 0; }
        size_t want = bytes + bytes / 8;
        F3D_HIP(ctx, hipMalloc(&b->p, want));
        b->cap = want;
        ++ctx->allocs;
    }
    *out = b->p;
    return F3D_OK;
}

int enter(f3d_ctx* ctx) {
    if (!ctx) return fail(nullptr, F3D_ERR_INVALID, "null context");
    ctx->err[0] = 0;
    F3D_HIP(ctx, hipSetDevice(ctx->device));
    return F3D_OK;
}

int make_filter(f3d_ctx* ctx, const int32_t* filter, int nfilter, int ncols, bool cols_must_exist, hipStream_t s,
                f3d_filter_args* fa) {
    fa->nfilter = 0; fa->cls_dev = nullptr; fa->cls_host = nullptr;
    for (int k = 0; k < 8; ++k) fa->cls[k] = -1;
    if (nfilter < 0 || nfilter > F3D_MAX_FILTER) return fail(ctx, F3D_ERR_INVALID, "nfilter %d out of range", nfilter);
    if (nfilter == 0 || !filter) {
        if (nfilter != 0) return fail(ctx, F3D_ERR_INVALID, "filter is NULL");
        return F3D_OK;
    }
    for (int k = 0; k < nfilter; ++k) {
        // votes[:, filter_classes] raises IndexError for a column that does not exist (voting.py:121)
        if (cols_must_exist && (filter[k] >= ncols || filter[k] < -ncols))
            return fail(ctx, F3D_ERR_INDEX, "filter class %d is out of bounds for %d vote columns", filter[k], ncols);
    }
    fa->nfilter = nfilter;
    int32_t tmp[F3D_MAX_FILTER];
    for (int k = 0; k < nfilter; ++k) tmp[k] = filter[k] < 0 ? filter[k] + ncols : filter[k];   // NumPy negative index
    if (nfilter <= 8) for (int k = 0; k < nfilter; ++k) fa->cls[k] = tmp[k];
    // the device copy always exists (the fused kernel reads the list from memory, whatever its length)
    memcpy(ctx->filter_host, tmp, sizeof(int32_t) * nfilter);
    F3D_HIP(ctx, hipMemcpyAsync(ctx->filter_dev, ctx->filter_host, sizeof(int32_t) * nfilter, hipMemcpyHostToDevice, s));
    fa->cls_dev = ctx->filter_dev;
    fa->cls_host = ctx->filter_host;
    return F3D_OK;
}

// The sticky device error word's bits in the order take_error reports them (the first set bit wins), each with its message.
static const struct { int bit; const char* msg; } device_errors[] = {
    {F3D_DEVERR_FUSE, "project_vote_argmax: a sampled mask label exceeds nclasses (the reference raises IndexError at voting.py:98)"},
    {F3D_DEVERR_VOTE, "vote_uv2pt: point index or mask label out of bounds (the reference raises IndexError at voting.py:98)"},
    {F3D_DEVERR_CC, "components_same_class: neighbour index out of bounds"},
    {F3D_DEVERR_FLOOD, "flood_order: neighbour index out of bounds"},
    {F3D_DEVERR_COLOR, "color_segment: seed or neighbour index out of bounds"},
    {F3D_DEVERR_GROW, "region_grow: seed or neighbour index out of bounds, or a seed listed twice"},
    {F3D_DEVERR_QUADS, "door_window_quads: a triangle's vertex index is out of bounds"},
    {F3D_DEVERR_PVOTE, "point_vote_frames: a mask label exceeds nclasses on a pixel that has a neighbour (the reference raises IndexError at voting.py:257)"},
    {F3D_DEVERR_MESH, "mesh: a triangle's vertex index is outside [0, nv)"},
    {F3D_DEVERR_PLANES, "extract_planes: neighbour index outside [0, n)"},
    {F3D_DEVERR_SMOOTH, "smooth_votes: neighbour index outside [0, n), or offsets that do not ascend"},
    {F3D_DEVERR_LIFT, "lift: an instance id exceeds max_ids, or a lookup is not below npoints"},
    {F3D_DEVERR_RASTER, "mesh render: a triangle's vertex index is outside [0, nv)"},
    {F3D_DEVERR_ZVOTE, "vote_visible: the mask label of a visible sample exceeds nclasses (the reference raises IndexError at voting.py:98)"},
};

// the message of the first table entry with a bit in `bits`, NULL when the table has none
const char* device_error_message(int bits) {
    for (const auto& d : device_errors) if (bits & d.bit) return d.msg;
    return nullptr;
}

// Reads the sticky device error word and consumes the bits in `mask` (each operation owns one bit, so that an error
// recorded by one operation is never blamed on, or silently skips, another one that shares the context).
int take_error(f3d_ctx* ctx, hipStream_t s, int mask) {
    int e = 0;
    F3D_HIP(ctx, hipMemcpyAsync(&e, ctx->dev_err, sizeof(int), hipMemcpyDeviceToHost, s));
    F3D_HIP(ctx, hipStreamSynchronize(s));
    e &= mask;
    if (e) {
        F3D_HIP(ctx, f3d_launch_clear_error_bits(ctx->dev_err, e, s));
        F3D_HIP(ctx, hipStreamSynchronize(s));
        if (const char* msg = device_error_message(e)) return fail(ctx, F3D_ERR_INDEX, "%s", msg);   // (a bit the table does not list is cleared silently)
    }
    return F3D_OK;
}

int reserve(f3d_ctx* ctx, std::initializer_list<reservation> list, int64_t table_hw) {
    const int strict = ctx->strict;
    ctx->strict = 0;
    int rc = F3D_OK;
    void* p;
    for (const reservation& r : list) if (!rc && r.wanted) rc = ensure(ctx, r.s, r.bytes, &p);
    if (!rc && table_hw > 0) rc = ensure_table(ctx, table_hw);
    ctx->strict = strict;
    return rc;
}

int f3d_version(void) { return F3D_VERSION; }

f3d_ctx* f3d_ctx_create(int device) {
    g_create_err[0] = 0;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        fail(nullptr, F3D_ERR_HIP, "no HIP device available (%s); libf3d_hip has no CPU fallback",
             e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
        return nullptr;
    }
    if (device < 0 || device >= count) { fail(nullptr, F3D_ERR_INVALID, "device %d out of range [0,%d)", device, count); return nullptr; }
    f3d_ctx* ctx = (f3d_ctx*)calloc(1, sizeof(f3d_ctx));
    if (ctx) { ctx->graph_n = -1; ctx->grp_n = -1; ctx->qry_n = -1; ctx->tsdf_n = -1; }
    if (!ctx) { fail(nullptr, F3D_ERR_NOMEM, "out of host memory"); return nullptr; }
    ctx->device = device;
    bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess &&
              hipMalloc((void**)&ctx->dev_err, sizeof(int)) == hipSuccess &&
              hipMalloc((void**)&ctx->filter_dev, sizeof(int32_t) * F3D_MAX_FILTER) == hipSuccess &&
              hipMalloc((void**)&ctx->count_dev, sizeof(unsigned long long)) == hipSuccess &&
              hipMalloc((void**)&ctx->codebook, sizeof(f3d_codebook)) == hipSuccess &&
              hipMalloc((void**)&ctx->first_bad, sizeof(int)) == hipSuccess &&
              hipMalloc((void**)&ctx->pv_words, 4 * sizeof(int)) == hipSuccess &&
              hipMemset(ctx->dev_err, 0, sizeof(int)) == hipSuccess &&
              hipMemset(ctx->codebook, 0, sizeof(f3d_codebook)) == hipSuccess;       // (the presence set is kept zero between calls)
    if (!ok) {
        fail(nullptr, F3D_ERR_HIP, "context setup failed: %s", hipGetErrorString(hipGetLastError()));
        f3d_ctx_destroy(ctx);
        return nullptr;
    }
    return ctx;
}

void f3d_ctx_destroy(f3d_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (devbuf& b : ctx->scratch) if (b.p) (void)hipFree(b.p);
    for (devbuf& b : ctx->stage) if (b.p) (void)hipFree(b.p);
    for (devbuf& b : ctx->kept) if (b.p) (void)hipFree(b.p);
    if (ctx->dev_err) (void)hipFree(ctx->dev_err);
    if (ctx->table) (void)hipFree(ctx->table);
    if (ctx->filter_dev) (void)hipFree(ctx->filter_dev);
    if (ctx->count_dev) (void)hipFree(ctx->count_dev);
    if (ctx->codebook) (void)hipFree(ctx->codebook);
    if (ctx->first_bad) (void)hipFree(ctx->first_bad);
    if (ctx->pv_words) (void)hipFree(ctx->pv_words);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    free(ctx);
}

const char* f3d_last_error(const f3d_ctx* ctx) { return ctx ? ctx->err : g_create_err; }

int f3d_ctx_synchronize(f3d_ctx* ctx) {
    int rc = enter(ctx); if (rc) return rc;
    F3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return F3D_OK;
}

void* f3d_ctx_stream(f3d_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int f3d_ctx_reserve(f3d_ctx* ctx, int64_t n, int nviews, int h, int w) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n > 0x7fffffffLL || nviews < 0 || h < 0 || w < 0) return fail(ctx, F3D_ERR_INVALID, "ctx_reserve: bad arguments");
    const bool frames = h > 0 && w > 0;
    return reserve(ctx, {{SLOT_TODO, f3d_fuse_todo_layout(n, nviews, F3D_CODE_MAX_NCLASSES).bytes},           // (any number of classes)
                         {SLOT_SORT_PERM, (size_t)n * 4, n > 0},
                         {SLOT_SORT_SCRATCH, f3d_sort_scratch_bytes(n), n > 0},
                         {SLOT_TILED_MASKS, frames && nviews > 0 ? f3d_coded_masks_bytes(nviews, h, w) : 0, frames && nviews > 0},
                         {SLOT_FUSE_TABLES, f3d_fuse_tables_bytes(nviews > 0 ? nviews : 1)}},
                   frames ? (int64_t)h * w : 0);
}

int f3d_ctx_set_strict(f3d_ctx* ctx, int strict) {
    if (!ctx) return F3D_ERR_INVALID;
    ctx->strict = strict ? 1 : 0;
    return F3D_OK;
}

long long f3d_ctx_alloc_count(const f3d_ctx* ctx) { return ctx ? ctx->allocs : -1; }

// Test hook (include/f3d.h): every byte a call may find in the arenas becomes `byte`.  What the code documents as holding nothing
// between calls is filled; what carries an invariant across calls is left: dev_err (the sticky error word) and codebook (its
// presence set is kept zero between calls).  The vote set is filled and marked unstamped, so the next batched vote clears it as it
// does after a single-frame vote.  The sequences that keep state in the arenas are ended: their fill passes ask for the count pass.
int f3d_debug_poison(f3d_ctx* ctx, int byte, int64_t out[2]) {
    int rc = enter(ctx); if (rc) return rc;
    if (!out || byte < 0 || byte > 255) return fail(ctx, F3D_ERR_INVALID, "debug_poison: byte must be in [0, 255] and out not NULL");
    if (ctx->chunk.active) return fail(ctx, F3D_ERR_INVALID, "debug_poison: a view-chunked fused call is in progress (its coded masks and todo list live in the scratch)");
    F3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int64_t buffers = 0, bytes = 0;
    auto fill = [&](void* p, size_t n) -> hipError_t {
        if (!p || !n) return hipSuccess;
        ++buffers; bytes += (int64_t)n;
        return hipMemsetAsync(p, byte, n, ctx->stream);
    };
    for (devbuf& b : ctx->scratch) F3D_HIP(ctx, fill(b.p, b.cap));
    for (devbuf& b : ctx->stage) F3D_HIP(ctx, fill(b.p, b.cap));
    for (devbuf& b : ctx->kept) F3D_HIP(ctx, fill(b.p, b.cap));
    F3D_HIP(ctx, fill(ctx->filter_dev, sizeof(int32_t) * F3D_MAX_FILTER));
    F3D_HIP(ctx, fill(ctx->count_dev, sizeof(unsigned long long)));
    F3D_HIP(ctx, fill(ctx->first_bad, sizeof(int)));
    F3D_HIP(ctx, fill(ctx->pv_words, 4 * sizeof(int)));
    F3D_HIP(ctx, fill(ctx->table, ctx->table_slots * sizeof(unsigned long long)));
    ctx->table_stamped = false;
    ctx->graph_n = -1; ctx->graph_kept = false;
    ctx->qry_n = -1; ctx->qry_kept = false;
    ctx->grp_n = -1; ctx->grp_cloud = false;
    ctx->tsdf_n = -1; ctx->tsdf_kept = false;
    F3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    out[0] = buffers; out[1] = bytes;
    return F3D_OK;
}

int f3d_take_device_error(f3d_ctx* ctx, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    return take_error(ctx, pick(ctx, stream));
}
