// C-ABI layer of libf3d_hip.so (see include/f3d.h): the subsystems' entry points, their host-pointer
// wrappers, and the tiny per-view host geometry; the context and its arenas are in f3d_ctx.h / f3d_ctx.cpp.
// No CPU fallback: every compute entry point needs a HIP device.
#include "f3d_ctx.h"

namespace {

// ---- host geometry, mirrored operation for operation by oracle/np_ref.py::frustum_data ------
void inv3(const double K[9], double o[9]) {
    const double a = K[0], b = K[1], c = K[2], d = K[3], e = K[4], f = K[5], g = K[6], h = K[7], i = K[8];
    const double A = e * i - f * h, B = c * h - b * i, C = b * f - c * e;
    const double D = f * g - d * i, E = a * i - c * g, F = c * d - a * f;
    const double G = d * h - e * g, H = b * g - a * h, I = a * e - b * d;
    const double det = (a * A + b * D) + c * G;
    o[0] = A / det; o[1] = B / det; o[2] = C / det;
    o[3] = D / det; o[4] = E / det; o[5] = F / det;
    o[6] = G / det; o[7] = H / det; o[8] = I / det;
}

struct frustum { double eye[3], lookat[3], normal[4][3]; };

void frustum_of(const double K[9], double w, double h, const double q[4], const double t[3], frustum* fr) {
    double Ki[9];
    inv3(K, Ki);
    const double pix[6][3] = {{0, 0, 0}, {0, 0, 1}, {w, 0, 1}, {w, h, 1}, {0, h, 1}, {w / 2, h / 2, 1}};
    double world[6][3];
    for (int k = 0; k < 6; ++k) {
        f3d_p3 c;
        c.x = (Ki[0] * pix[k][0] + Ki[1] * pix[k][1]) + Ki[2] * pix[k][2];      // camera_utils.py:86
        c.y = (Ki[3] * pix[k][0] + Ki[4] * pix[k][1]) + Ki[5] * pix[k][2];
        c.z = (Ki[6] * pix[k][0] + Ki[7] * pix[k][1]) + Ki[8] * pix[k][2];
        c.x = c.x / 1; c.y = c.y / 1; c.z = c.z / 1;                           // rescale = 1 (:111)
        const f3d_p3 r = f3d_rotate(q, c);                                      // :128-129 (forward rotation)
        world[k][0] = r.x + t[0]; world[k][1] = r.y + t[1]; world[k][2] = r.z + t[2];
    }
    for (int c = 0; c < 3; ++c) fr->eye[c] = world[0][c];
    {                                                                           // lookat = unit(centre - eye) (:148-150)
        const double v0 = world[5][0] - world[0][0], v1 = world[5][1] - world[0][1], v2 = world[5][2] - world[0][2];
        const double nn = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
        fr->lookat[0] = v0 / nn; fr->lookat[1] = v1 / nn; fr->lookat[2] = v2 / nn;
    }
    for (int k = 0; k < 4; ++k) {                                               // camera_utils.py:163-170
        const double* ca = world[1 + k];
        const double* cb = world[1 + (k + 1) % 4];
        const double a0 = ca[0] - world[0][0], a1 = ca[1] - world[0][1], a2 = ca[2] - world[0][2];
        const double b0 = cb[0] - world[0][0], b1 = cb[1] - world[0][1], b2 = cb[2] - world[0][2];
        const double n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
        const double nn = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
        fr->normal[k][0] = n0 / nn; fr->normal[k][1] = n1 / nn; fr->normal[k][2] = n2 / nn;
    }
}

int quat_inverse(const double q[4], double o[4]) {
    const double ss = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    if (ss == 0.0) return F3D_ERR_ZERO_QUAT;
    o[0] = q[0] / ss; o[1] = -q[1] / ss; o[2] = -q[2] / ss; o[3] = -q[3] / ss;
    return F3D_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// host geometry
// ---------------------------------------------------------------------------------------------
int f3d_quat_inverse(const double q[4], double o[4]) {
    if (!q || !o) return F3D_ERR_INVALID;
    return quat_inverse(q, o);
}

int f3d_frustum_data(const double K[9], double w, double h, const double* q, const double* t, int nviews,
                     double* eyes, double* lookats, double* face_normals) {
    if (!K || !q || !t || nviews < 0) return F3D_ERR_INVALID;
    for (int v = 0; v < nviews; ++v) {
        frustum fr;
        frustum_of(K, w, h, q + 4 * v, t + 3 * v, &fr);
        if (eyes) memcpy(eyes + 3 * v, fr.eye, sizeof fr.eye);
        if (lookats) memcpy(lookats + 3 * v, fr.lookat, sizeof fr.lookat);
        if (face_normals) memcpy(face_normals + 12 * v, fr.normal, sizeof fr.normal);
    }
    return F3D_OK;
}

int f3d_views_build(const double K[9], double w, double h, const double* q, const double* t, int nviews, double max_depth,
                    f3d_view* out) {
    if (!K || !q || !t || !out || nviews < 0) return F3D_ERR_INVALID;
    for (int v = 0; v < nviews; ++v) {
        f3d_view* vw = out + v;
        memset(vw, 0, sizeof *vw);
        memcpy(vw->K, K, sizeof vw->K);
        const int rc = quat_inverse(q + 4 * v, vw->qinv);
        if (rc) return rc;
        memcpy(vw->t, t + 3 * v, sizeof vw->t);
        frustum fr;
        frustum_of(K, w, h, q + 4 * v, t + 3 * v, &fr);
        for (int m = 0; m < 4; ++m) {                                           // fusion.py:254 (spoke origins = eye)
            memcpy(vw->plane_pt[m], fr.eye, sizeof fr.eye);
            memcpy(vw->plane_n[m], fr.normal[m], sizeof fr.normal[m]);
        }
        for (int c = 0; c < 3; ++c) {                                           // fusion.py:255-256
            vw->plane_pt[4][c] = fr.eye[c] + max_depth * fr.lookat[c];
            vw->plane_n[4][c] = -fr.lookat[c];
        }
        double l1max = 0.0, nmax = 1.0;
        for (int m = 0; m < F3D_NPLANES; ++m) {
            const double nl1 = fabs(vw->plane_n[m][0]) + fabs(vw->plane_n[m][1]) + fabs(vw->plane_n[m][2]);
            const double l1 = (fabs(vw->plane_pt[m][0]) + fabs(vw->plane_pt[m][1]) + fabs(vw->plane_pt[m][2])) * (nl1 > 1 ? nl1 : 1);
            if (l1 > l1max) l1max = l1;
            for (int c = 0; c < 3; ++c) if (fabs(vw->plane_n[m][c]) > nmax) nmax = fabs(vw->plane_n[m][c]);
        }
        // float32 pre-cull a = n32.p32 - off32: inputs rounded to f32 (2^-24 relative each) + 3 f32 FMAs, against the
        // exact plane value that itself carries ~12 eps64 of rounding: 32 * 2^-24 * (|p|_1 + |pp|_1) covers both, 2x margin
        const double eps32 = 32.0 * 5.9604644775390625e-08;
        for (int m = 0; m < F3D_NPLANES; ++m) {
            for (int c = 0; c < 3; ++c) vw->cull_n32[m][c] = (float)vw->plane_n[m][c];
            const double off = fma(vw->plane_n[m][0], vw->plane_pt[m][0],
                               fma(vw->plane_n[m][1], vw->plane_pt[m][1], vw->plane_n[m][2] * vw->plane_pt[m][2]));
            vw->cull_off32[m] = (float)off;
            vw->plane_off[m] = off;
        }
        // float64 refinement: FMA value and exact value are both within ~12 eps64 * (|p|_1 + |pp|_1) of the real number
        vw->cull_rel64 = 64.0 * 2.220446049250313e-16 * nmax;
        vw->cull_abs64 = 64.0 * 2.220446049250313e-16 * l1max + 1e-300;
        vw->img_w = (float)w; vw->img_h = (float)h;
        vw->cull_rel32 = (float)(eps32 * nmax * 1.0000002);
        vw->cull_abs32 = (float)(eps32 * l1max * 1.0000002 + 1e-30);
        // fast projection operator M = K * Rot(qinv), Rot = the matrix of x -> q x q* for the un-normalised q
        {
            const long double w_ = vw->qinv[0], x = vw->qinv[1], y = vw->qinv[2], z = vw->qinv[3];
            const long double R[9] = {w_ * w_ + x * x - y * y - z * z, 2 * (x * y - w_ * z), 2 * (x * z + w_ * y),
                                      2 * (x * y + w_ * z), w_ * w_ - x * x + y * y - z * z, 2 * (y * z - w_ * x),
                                      2 * (x * z - w_ * y), 2 * (y * z + w_ * x), w_ * w_ - x * x - y * y + z * z};
            const long double q2 = w_ * w_ + x * x + y * y + z * z;
            for (int r = 0; r < 3; ++r) {
                long double l1 = 0;
                for (int c = 0; c < 3; ++c) {
                    long double acc = 0;
                    for (int k = 0; k < 3; ++k) acc += (long double)K[3 * r + k] * R[3 * k + c];
                    vw->M[3 * r + c] = (double)acc;
                    vw->M32[3 * r + c] = (float)vw->M[3 * r + c];
                    l1 += fabsl((long double)K[3 * r + c]);
                }
                vw->mnorm[r] = (double)(l1 * q2 * 1.000000001L);
            }
        }
    }
    return F3D_OK;
}

// ---------------------------------------------------------------------------------------------
// a1 rotate
// ---------------------------------------------------------------------------------------------
int f3d_rotate_f64(f3d_ctx* ctx, const double* xyz, int64_t n, const double q[4], double* out) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || (n > 0 && (!xyz || !out)) || !q) return fail(ctx, F3D_ERR_INVALID, "rotate: bad arguments");
    if (n == 0) return F3D_OK;
    staging st(ctx);
    const double* din = st.in(xyz, (size_t)n * 24);
    double* dout = st.out(out, (size_t)n * 24);
    if (!st.rc) st.rc = f3d_rotate_f64_dev(ctx, din, n, q, dout, ctx->stream);
    return st.finish();
}

int f3d_rotate_f64_dev(f3d_ctx* ctx, const double* xyz, int64_t n, const double q[4], double* out, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || (n > 0 && (!xyz || !out)) || !q) return fail(ctx, F3D_ERR_INVALID, "rotate: bad arguments");
    if (n == 0) return F3D_OK;
    F3D_HIP(ctx, f3d_launch_rotate(xyz, n, q, out, pick(ctx, stream)));
    return F3D_OK;
}

// ---------------------------------------------------------------------------------------------
// (f)#3 depth frame -> world points
// ---------------------------------------------------------------------------------------------
static size_t depth_bytes(int depth_type, int64_t n) { return (size_t)n * (depth_type == F3D_DEPTH_U16 ? 2 : depth_type == F3D_DEPTH_F32 ? 4 : 8); }

int f3d_unproject_depth_dev(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9], double depth_scale,
                            const double q_wxyz[4], const double t[3], double* xyz, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (h < 0 || w < 0 || !K || !q_wxyz || !t || (depth_type != F3D_DEPTH_U16 && depth_type != F3D_DEPTH_F32 && depth_type != F3D_DEPTH_F64) ||
        ((int64_t)h * w > 0 && (!depth || !xyz)))
        return fail(ctx, F3D_ERR_INVALID, "unproject_depth: bad arguments");
    F3D_HIP(ctx, f3d_launch_unproject_depth(depth, depth_type, h, w, K, depth_scale, q_wxyz, t, xyz, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_unproject_depth_batch_dev(f3d_ctx* ctx, const void* depth, int depth_type, int nframes, int h, int w, const double K[9], double depth_scale,
                                  const double* q_wxyz, const double* t, double* xyz, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (nframes < 0 || h < 0 || w < 0 || !K || (depth_type != F3D_DEPTH_U16 && depth_type != F3D_DEPTH_F32 && depth_type != F3D_DEPTH_F64) ||
        (nframes > 0 && (!q_wxyz || !t)) || ((int64_t)nframes * h * w > 0 && (!depth || !xyz)))
        return fail(ctx, F3D_ERR_INVALID, "unproject_depth_batch: bad arguments");
    if (nframes == 0) return F3D_OK;
    F3D_HIP(ctx, f3d_launch_unproject_depth_batch(depth, depth_type, nframes, h, w, K, depth_scale, q_wxyz, t, xyz, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_unproject_depth(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9], double depth_scale,
                        const double q_wxyz[4], const double t[3], double* xyz) {
    int rc = enter(ctx); if (rc) return rc;
    const int64_t n = (int64_t)h * w;
    if (h < 0 || w < 0 || (n > 0 && (!depth || !xyz))) return fail(ctx, F3D_ERR_INVALID, "unproject_depth: bad arguments");
    if (depth_type != F3D_DEPTH_U16 && depth_type != F3D_DEPTH_F32 && depth_type != F3D_DEPTH_F64)
        return fail(ctx, F3D_ERR_INVALID, "unproject_depth: unknown depth type %d", depth_type);
    if (n == 0) return F3D_OK;
    staging st(ctx);
    const void* din = st.in(depth, depth_bytes(depth_type, n));
    double* dout = st.out(xyz, (size_t)n * 24);
    if (!st.rc) st.rc = f3d_unproject_depth_dev(ctx, din, depth_type, h, w, K, depth_scale, q_wxyz, t, dout, ctx->stream);
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// a2 / a4 / single-view fused
// ---------------------------------------------------------------------------------------------
int f3d_project_view_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* view, int32_t* uv,
                         uint8_t* inside, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || !view || (!uv && !inside) || (n > 0 && !xyz)) return fail(ctx, F3D_ERR_INVALID, "project_view: bad arguments");
    F3D_HIP(ctx, f3d_launch_project_view(xyz, dtype, n, *view, uv, inside, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_project_view_f64(f3d_ctx* ctx, const double* xyz, int64_t n, const f3d_view* view, int32_t* uv, uint8_t* inside) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || !view || (!uv && !inside) || (n > 0 && !xyz)) return fail(ctx, F3D_ERR_INVALID, "project_view: bad arguments");
    if (n == 0) return F3D_OK;
    staging st(ctx);
    const double* din = st.in(xyz, (size_t)n * 24);
    int32_t* duv = st.out(uv, (size_t)n * 8);
    uint8_t* dinside = st.out(inside, (size_t)n);
    if (!st.rc) st.rc = f3d_project_view_dev(ctx, din, F3D_F64, n, view, duv, dinside, ctx->stream);
    return st.finish();
}

static int pose_view(f3d_ctx* ctx, const double K[9], const double q[4], const double t[3], f3d_view* vw) {
    if (!K || !q || !t) return fail(ctx, F3D_ERR_INVALID, "points2pixel: NULL camera");
    memset(vw, 0, sizeof *vw);
    memcpy(vw->K, K, sizeof vw->K);
    memcpy(vw->t, t, sizeof vw->t);
    if (quat_inverse(q, vw->qinv)) return fail(ctx, F3D_ERR_ZERO_QUAT, "a zero quaternion cannot be inverted");
    return F3D_OK;
}

int f3d_points2pixel_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const double K[9], const double q[4],
                         const double t[3], int32_t* uv, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    f3d_view vw;
    if ((rc = pose_view(ctx, K, q, t, &vw))) return rc;
    if (n < 0 || !uv || (n > 0 && !xyz)) return fail(ctx, F3D_ERR_INVALID, "points2pixel: bad arguments");
    F3D_HIP(ctx, f3d_launch_project_view(xyz, dtype, n, vw, uv, nullptr, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_points2pixel_f64(f3d_ctx* ctx, const double* xyz, int64_t n, const double K[9], const double q[4], const double t[3],
                         int32_t* uv) {
    int rc = enter(ctx); if (rc) return rc;
    f3d_view vw;
    if ((rc = pose_view(ctx, K, q, t, &vw))) return rc;
    return f3d_project_view_f64(ctx, xyz, n, &vw, uv, nullptr);
}

int f3d_inside_polyhedra_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const double* plane_pts,
                             const double* normals, int m, uint8_t* inside, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || m < 0 || !inside || (n > 0 && !xyz) || (m > 0 && (!plane_pts || !normals)))
        return fail(ctx, F3D_ERR_INVALID, "inside_polyhedra: bad arguments");
    hipStream_t s = pick(ctx, stream);
    int done = 0;
    do {                                                    // m == 0: every point is inside (signsum == 0 == len)
        f3d_plane_args pa;
        pa.m = (m - done) < F3D_PLANES_PER_LAUNCH ? (m - done) : F3D_PLANES_PER_LAUNCH;
        pa.accumulate = done > 0;
        memcpy(pa.pt, plane_pts + 3 * done, sizeof(double) * 3 * pa.m);
        memcpy(pa.n, normals + 3 * done, sizeof(double) * 3 * pa.m);
        F3D_HIP(ctx, f3d_launch_inside_polyhedra(xyz, dtype, n, pa, inside, s));
        done += pa.m;
    } while (done < m);
    return F3D_OK;
}

int f3d_inside_polyhedra_f64(f3d_ctx* ctx, const double* xyz, int64_t n, const double* plane_pts, const double* normals, int m,
                             uint8_t* inside) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || !inside || (n > 0 && !xyz)) return fail(ctx, F3D_ERR_INVALID, "inside_polyhedra: bad arguments");
    if (n == 0) return F3D_OK;
    staging st(ctx);
    const double* din = st.in(xyz, (size_t)n * 24);
    uint8_t* dout = st.out(inside, (size_t)n);
    if (!st.rc) st.rc = f3d_inside_polyhedra_dev(ctx, din, F3D_F64, n, plane_pts, normals, m, dout, ctx->stream);
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// fused multi-view path
// ---------------------------------------------------------------------------------------------
int f3d_cloud_sort_cells_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, void* sorted_xyz, int32_t* perm,
                             void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n > 0x7fffffffLL || (n > 0 && (!xyz || !perm)))
        return fail(ctx, F3D_ERR_INVALID, "cloud_sort_cells: bad arguments (n < 2^31)");
    if (n == 0) return F3D_OK;
    void* scratch;
    if ((rc = ensure(ctx, SLOT_SORT_SCRATCH, f3d_sort_scratch_bytes(n), &scratch))) return rc;   // grows on first use only
    F3D_HIP(ctx, f3d_launch_cell_sort(xyz, dtype, n, sorted_xyz, perm, scratch, pick(ctx, stream)));
    return F3D_OK;
}

// The context scratch of a fused call, ensured in one place: the todo block (laid out by `lay`) and the view tables always; the coded
// masks, the carried bins of a view-chunked call, the cell sort's permutation + scratch and `keep_bytes` of cell-ordered cloud as asked.
enum { FUSE_CODED = 1, FUSE_CARRY = 2, FUSE_SORT = 4 };
struct fuse_scratch { void *todo, *tables, *tm, *carry, *perm, *sort, *keep; };

static int ensure_fuse_scratch(f3d_ctx* ctx, const f3d_fuse_todo& lay, int64_t n, int nviews, int h, int w, int nclasses, unsigned which,
                               size_t keep_bytes, fuse_scratch* o) {
    int rc;
    *o = fuse_scratch{};
    if ((which & FUSE_SORT) && ((rc = ensure(ctx, SLOT_SORT_PERM, (size_t)n * 4, &o->perm)) ||
                                (rc = ensure(ctx, SLOT_SORT_SCRATCH, f3d_sort_scratch_bytes(n), &o->sort)))) return rc;
    if (keep_bytes && (rc = ensure(ctx, SLOT_FUSE_XYZ, keep_bytes, &o->keep))) return rc;
    if ((which & FUSE_CODED) && (rc = ensure(ctx, SLOT_TILED_MASKS, f3d_coded_masks_bytes(nviews, h, w), &o->tm))) return rc;
    if ((rc = ensure(ctx, SLOT_TODO, lay.bytes, &o->todo))) return rc;
    if ((rc = ensure(ctx, SLOT_FUSE_TABLES, f3d_fuse_tables_bytes(nviews > 0 ? nviews : 1), &o->tables))) return rc;
    if ((which & FUSE_CARRY) && (rc = ensure(ctx, SLOT_FUSE_CARRY, f3d_fuse_carry_bytes(n, nclasses), &o->carry))) return rc;
    return F3D_OK;
}

// F3D_FUSE_SORT: the cloud's cell order into the context's permutation (FUSE_SORT scratch); the kernel then reads xyz[perm[i]]
// ride (the one-shot call with coded masks, or NULL): presence, k_fuse_setup with the book, mask coding into sc.tm and the label fill run
// inside the sort's launches; the caller then skips f3d_launch_code_masks_with_setup
static int sort_into_perm(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const fuse_scratch& sc, hipStream_t s, const int32_t** perm,
                          f3d_fuse_job* ride = nullptr) {
    if (ride) F3D_HIP(ctx, f3d_launch_cell_sort_with_riders(*ride, (uint8_t*)sc.tm, ctx->codebook, (int32_t*)sc.perm, sc.sort));
    else F3D_HIP(ctx, f3d_launch_cell_sort(xyz, dtype, n, nullptr, (int32_t*)sc.perm, sc.sort, s));
    *perm = (const int32_t*)sc.perm;
    return F3D_OK;
}

int f3d_project_vote_argmax_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views_dev, int nviews,
                                const uint8_t* masks, int h, int w, int nclasses, const int32_t* filter, int nfilter,
                                double threshold, int64_t* classes, uint16_t* votes_u16, unsigned flags, const int32_t* perm,
                                void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || nviews < 0 || h <= 0 || w <= 0 || nclasses < 0 || nclasses > 65534 || !classes ||
        (n > 0 && !xyz) || (nviews > 0 && (!views_dev || !masks)))
        return fail(ctx, F3D_ERR_INVALID, "project_vote_argmax: bad arguments");
    if (nviews > 65535) return fail(ctx, F3D_ERR_INVALID, "project_vote_argmax: at most 65535 views");
    if ((int64_t)h * (int64_t)w >= (int64_t)1 << 31) return fail(ctx, F3D_ERR_INVALID, "project_vote_argmax: mask of %d x %d pixels is too large", h, w);
    if ((flags & F3D_FUSE_SORT) && perm) return fail(ctx, F3D_ERR_INVALID, "project_vote_argmax: F3D_FUSE_SORT and perm are exclusive");
    f3d_fuse_job job{};
    job.stream = pick(ctx, stream);
    if ((rc = make_filter(ctx, filter, nfilter, nclasses + 1, true, job.stream, &job.flt))) return rc;
    const bool sort = (flags & F3D_FUSE_SORT) && n > 512 && n <= 0x7fffffffLL;
    // the accelerated kernels address the coded masks with 32-bit offsets; beyond 4 GiB of them the exact kernel labels every point
    const bool coded = nviews > 0 && nclasses <= F3D_CODE_MAX_NCLASSES && f3d_coded_masks_bytes(nviews, h, w) < ((size_t)1 << 32);
    job.lay = f3d_fuse_todo_layout(n, nviews, nclasses);
    fuse_scratch sc;                                                                            // grows on first use only
    if ((rc = ensure_fuse_scratch(ctx, job.lay, n, nviews, h, w, nclasses, (coded ? FUSE_CODED : 0) | (sort ? FUSE_SORT : 0), 0, &sc))) return rc;
    // A call that sorts and codes hands presence, k_fuse_setup with the book, mask coding and the label fill to the sort as riders: extra
    // blocks of three of its launches (f3d_sort_riders), no second stream, no event.  Measured at C3 (profiles/fuse_riders.md): 0.888 -> 0.865 ms
    // per step, 0.299 -> 0.282 at 1.25M points; a step without that work at all would be 0.814 / 0.248.
    // (Measured and dropped earlier: coding the masks on a second stream forked from and joined into `stream` with events while the
    // cloud is sorted -- the two event dependencies cost more than the overlap they bought, 1.32 ms per C3 step instead of 1.26.)
    job.xyz = xyz; job.dtype = dtype; job.n = n; job.perm = perm; job.gather = (flags & F3D_FUSE_GATHER) && perm;
    job.views_dev = views_dev; job.nviews = nviews; job.v0 = 0; job.v1 = nviews; job.masks = masks; job.h = h; job.w = w;
    job.nclasses = nclasses; job.threshold = threshold; job.classes = classes; job.votes = votes_u16; job.err = ctx->dev_err;
    job.todo = sc.todo; job.cb = ctx->codebook; job.tables = sc.tables; job.occ = &ctx->fuse_occ;
    if (sort) {
        if ((rc = sort_into_perm(ctx, xyz, dtype, n, sc, job.stream, &job.perm, coded ? &job : nullptr))) return rc;
        job.gather = true;
    }
    if (coded) {                                                                                // coded, tiled copy for the fast kernel
        if (!sort) F3D_HIP(ctx, f3d_launch_code_masks_with_setup(job, (uint8_t*)sc.tm, ctx->codebook));
        job.cmasks = (const uint8_t*)sc.tm;
    }
    F3D_HIP(ctx, f3d_launch_fuse(job));
    return F3D_OK;
}

// ---- the same path with the views arriving in chunks (multi-GPU: the masks of chunk c+1 are still in flight while chunk c votes)
int f3d_mask_presence_dev(f3d_ctx* ctx, const uint8_t* masks, int nviews, int h, int w, uint8_t* present256, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (nviews < 0 || h <= 0 || w <= 0 || !present256 || (nviews > 0 && !masks)) return fail(ctx, F3D_ERR_INVALID, "mask_presence: bad arguments");
    hipStream_t s = pick(ctx, stream);
    F3D_HIP(ctx, f3d_launch_mask_presence(masks, (int64_t)nviews * h * w, ctx->codebook, s));
    F3D_HIP(ctx, f3d_launch_presence_bytes(ctx->codebook, present256, true, s));
    return F3D_OK;
}

int f3d_fuse_chunked_begin_dev(f3d_ctx* ctx, const uint8_t* present256, int64_t n, int nviews, int h, int w, int nclasses,
                               const int32_t* filter, int nfilter, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    ctx->chunk.active = 0;
    if (n < 0 || n > 0x7ffff000LL || nviews <= 0 || nviews > 255 || h <= 0 || w <= 0 || nclasses < 0 || nclasses > F3D_CODE_MAX_NCLASSES)
        return fail(ctx, F3D_ERR_INVALID, "fuse_chunked_begin: bad arguments (1..255 views, nclasses <= %d)", F3D_CODE_MAX_NCLASSES);
    if (f3d_coded_masks_bytes(nviews, h, w) >= ((size_t)1 << 32))
        return fail(ctx, F3D_ERR_INVALID, "fuse_chunked_begin: %d coded masks of %d x %d exceed 4 GiB; use f3d_project_vote_argmax_dev", nviews, h, w);
    hipStream_t s = pick(ctx, stream);
    f3d_filter_args fa;
    if ((rc = make_filter(ctx, filter, nfilter, nclasses + 1, true, s, &fa))) return rc;
    // every scratch buffer of the chunk calls, so that they allocate nothing: with n > 0 also what F3D_FUSE_SORT / a gathered cloud
    // needs (permutation, sort scratch, cell-order copy)
    ctx->chunk.lay = f3d_fuse_todo_layout(n, nviews, nclasses);
    fuse_scratch sc;
    if ((rc = ensure_fuse_scratch(ctx, ctx->chunk.lay, n, nviews, h, w, nclasses, FUSE_CODED | FUSE_CARRY | (n > 0 ? FUSE_SORT : 0),
                                  (size_t)n * 24, &sc))) return rc;
    if (present256) F3D_HIP(ctx, f3d_launch_presence_bytes(ctx->codebook, const_cast<uint8_t*>(present256), false, s));
    else F3D_HIP(ctx, hipMemsetAsync(ctx->codebook->presence, 0xFF, sizeof ctx->codebook->presence, s));     // every label gets a bin
    F3D_HIP(ctx, f3d_launch_code_book(ctx->codebook, nclasses, fa, false, s));
    ctx->chunk.active = 1; ctx->chunk.next = 0; ctx->chunk.nviews = nviews; ctx->chunk.h = h; ctx->chunk.w = w;
    ctx->chunk.nclasses = nclasses; ctx->chunk.n = n; ctx->chunk.perm = nullptr; ctx->chunk.gather = 0; ctx->chunk.xyz = nullptr;
    return F3D_OK;
}

int f3d_code_planes_dev(f3d_ctx* ctx, const uint8_t* masks, int nplanes, int h, int w, uint8_t* coded, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!ctx->chunk.active || ctx->chunk.h != h || ctx->chunk.w != w)
        return fail(ctx, F3D_ERR_INVALID, "code_planes: no view-chunked call with masks of %d x %d is in progress (f3d_fuse_chunked_begin_dev first)", h, w);
    if (nplanes < 0 || (nplanes > 0 && (!masks || !coded)) || ((uintptr_t)coded & 7)) return fail(ctx, F3D_ERR_INVALID, "code_planes: bad arguments (coded: 8-byte aligned)");
    F3D_HIP(ctx, f3d_launch_code_planes(masks, coded, nplanes, h, w, ctx->codebook, pick(ctx, stream)));
    return F3D_OK;
}

// The views [v_begin, v_end) of a view-chunked call, in the job record's terms: `j` arrives with the caller's cloud, views, masks, vote
// rule and labels.  masks: raw planes [nviews, H, W], coded here into context scratch -- or coded: planes some rank coded already
// (f3d_code_planes_dev with the same book), [nviews] x f3d_coded_plane_bytes, used where they lie
static int fuse_chunk_impl(f3d_ctx* ctx, f3d_fuse_job& j, const uint8_t* coded, const int32_t* filter, int nfilter, unsigned flags, void* stream) {
    int rc;
    const int64_t n = j.n;
    const int nviews = j.nviews, v_begin = j.v0, v_end = j.v1, h = j.h, w = j.w, nclasses = j.nclasses;
    if (!ctx->chunk.active || ctx->chunk.next != v_begin || ctx->chunk.nviews != nviews || ctx->chunk.h != h || ctx->chunk.w != w ||
        ctx->chunk.nclasses != nclasses || ctx->chunk.n != n || v_end <= v_begin || v_end > nviews)
        return fail(ctx, F3D_ERR_INVALID, "fuse_chunk: views [%d, %d) do not continue the call begun with f3d_fuse_chunked_begin_dev "
                    "(next view %d of %d, same n / h / w / nclasses required)", v_begin, v_end, ctx->chunk.active ? ctx->chunk.next : -1, ctx->chunk.nviews);
    if (!j.classes || (n > 0 && !j.xyz) || !j.views_dev) return fail(ctx, F3D_ERR_INVALID, "fuse_chunk: bad arguments");
    if ((flags & F3D_FUSE_SORT) && j.perm) return fail(ctx, F3D_ERR_INVALID, "fuse_chunk: F3D_FUSE_SORT and perm are exclusive");
    hipStream_t s = j.stream = pick(ctx, stream);
    if ((rc = make_filter(ctx, filter, nfilter, nclasses + 1, true, s, &j.flt))) return rc;
    const bool first = v_begin == 0, sort = first && (flags & F3D_FUSE_SORT) && n > 512;
    // a cloud read through a permutation and more chunks to come: the first chunk leaves it behind in cell order (context scratch),
    // the later chunks stream that copy instead of gathering 24-byte points again
    const bool keep = first && v_end < nviews && n > 0 && (sort || ((flags & F3D_FUSE_GATHER) && j.perm));
    fuse_scratch sc;
    if ((rc = ensure_fuse_scratch(ctx, ctx->chunk.lay, n, nviews, h, w, nclasses, FUSE_CODED | FUSE_CARRY | (sort ? FUSE_SORT : 0),
                                  keep ? xyz_bytes((f3d_dtype)j.dtype, n) : 0, &sc))) return rc;
    if (first) {                                               // the point order is fixed by the first chunk
        ctx->chunk.perm = j.perm; ctx->chunk.gather = ((flags & F3D_FUSE_GATHER) && j.perm) ? 1 : 0;
        if (sort) {
            if ((rc = sort_into_perm(ctx, j.xyz, (f3d_dtype)j.dtype, n, sc, s, &ctx->chunk.perm))) return rc;
            ctx->chunk.gather = 1;
        }
        ctx->chunk.xyz = j.xyz;
    }
    j.xyz = ctx->chunk.xyz; j.perm = ctx->chunk.perm; j.gather = ctx->chunk.gather != 0;
    const size_t plane = f3d_coded_masks_bytes(1, h, w);
    j.cmasks = coded ? coded : (const uint8_t*)sc.tm;          // the exchange delivered coded planes: no coding, no raw masks, the exact tier reads codes
    if (!coded) F3D_HIP(ctx, f3d_launch_code_planes(j.masks + (size_t)v_begin * h * w, (uint8_t*)sc.tm + (size_t)v_begin * plane, v_end - v_begin, h, w, ctx->codebook, s));
    j.err = ctx->dev_err; j.todo = sc.todo; j.lay = ctx->chunk.lay; j.cb = ctx->codebook; j.tables = sc.tables; j.carry = (uint32_t*)sc.carry; j.xyz_keep = sc.keep;
    j.occ = &ctx->fuse_occ;
    F3D_HIP(ctx, f3d_launch_fuse_setup(j, ctx->codebook, false));
    F3D_HIP(ctx, f3d_launch_fuse(j));
    if (sc.keep) { ctx->chunk.xyz = sc.keep; ctx->chunk.gather = 0; }
    ctx->chunk.next = v_end;
    if (v_end == nviews) ctx->chunk.active = 0;
    return F3D_OK;
}

int f3d_fuse_chunk_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views_dev, int nviews, int v_begin, int v_end,
                       const uint8_t* masks, int h, int w, int nclasses, const int32_t* filter, int nfilter, double threshold,
                       int64_t* classes, unsigned flags, const int32_t* perm, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!masks) return fail(ctx, F3D_ERR_INVALID, "fuse_chunk: bad arguments");
    f3d_fuse_job j{};
    j.xyz = xyz; j.dtype = dtype; j.n = n; j.perm = perm; j.views_dev = views_dev; j.nviews = nviews; j.v0 = v_begin; j.v1 = v_end;
    j.h = h; j.w = w; j.nclasses = nclasses; j.threshold = threshold; j.classes = classes;
    j.masks = masks;
    return fuse_chunk_impl(ctx, j, nullptr, filter, nfilter, flags, stream);
}

int f3d_fuse_chunk_coded_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views_dev, int nviews, int v_begin, int v_end,
                             const uint8_t* coded, int h, int w, int nclasses, const int32_t* filter, int nfilter, double threshold,
                             int64_t* classes, unsigned flags, const int32_t* perm, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!coded || ((uintptr_t)coded & 7)) return fail(ctx, F3D_ERR_INVALID, "fuse_chunk_coded: bad arguments (coded: 8-byte aligned)");
    f3d_fuse_job j{};
    j.xyz = xyz; j.dtype = dtype; j.n = n; j.perm = perm; j.views_dev = views_dev; j.nviews = nviews; j.v0 = v_begin; j.v1 = v_end;
    j.h = h; j.w = w; j.nclasses = nclasses; j.threshold = threshold; j.classes = classes;
    return fuse_chunk_impl(ctx, j, coded, filter, nfilter, flags, stream);
}

int f3d_debug_fastpath_audit(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views, int nviews, int w, int h,
                             uint64_t stats[4]) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n > 0x7fffffffLL || nviews < 0 || w <= 0 || h <= 0 || !stats || (n > 0 && !xyz) || (nviews > 0 && !views))
        return fail(ctx, F3D_ERR_INVALID, "fastpath_audit: bad arguments");
    staging st(ctx);
    const void* dxyz = st.in(xyz, xyz_bytes(dtype, n));
    void* dsorted = st.slot(xyz_bytes(dtype, n));
    int32_t* dperm = (int32_t*)st.slot((size_t)n * 4);
    const f3d_view* dviews = st.in(views, sizeof(f3d_view) * (size_t)nviews);
    void* dstats = st.slot(64);
    st.back(stats, dstats, 32);
    if (st.rc) return st.rc;
    // waves of 64 consecutive points must be spatial neighbours, as in the fused call: audit the cell-sorted copy
    if ((rc = f3d_cloud_sort_cells_dev(ctx, dxyz, dtype, n, dsorted, dperm, ctx->stream))) return rc;
    F3D_HIP(ctx, f3d_launch_fastpath_audit(dsorted, dtype, n, dviews, nviews, w, h, (unsigned long long*)dstats, ctx->stream));
    return st.finish();
}

int f3d_debug_fuse_deferred(f3d_ctx* ctx, void* stream, uint32_t counts[2]) {
    int rc = enter(ctx); if (rc) return rc;
    if (!counts || !ctx->scratch[SLOT_TODO].p) return fail(ctx, F3D_ERR_INVALID, "fuse_deferred: no fused call has run in this context");
    hipStream_t s = pick(ctx, stream);
    F3D_HIP(ctx, hipMemcpyAsync(counts, f3d_fuse_todo::counters(ctx->scratch[SLOT_TODO].p), 8, hipMemcpyDeviceToHost, s));
    F3D_HIP(ctx, hipStreamSynchronize(s));
    return F3D_OK;
}

int f3d_debug_fuse_decided(f3d_ctx* ctx, void* stream, uint32_t* count) {
    int rc = enter(ctx); if (rc) return rc;
    if (!count || !ctx->scratch[SLOT_TODO].p) return fail(ctx, F3D_ERR_INVALID, "fuse_decided: no fused call has run in this context");
    hipStream_t s = pick(ctx, stream);
    F3D_HIP(ctx, hipMemcpyAsync(count, f3d_fuse_todo::counters(ctx->scratch[SLOT_TODO].p) + 3, 4, hipMemcpyDeviceToHost, s));
    F3D_HIP(ctx, hipStreamSynchronize(s));
    return F3D_OK;
}

int f3d_project_vote_argmax(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views, int nviews,
                            const uint8_t* masks, int h, int w, int nclasses, const int32_t* filter, int nfilter,
                            double threshold, int64_t* classes, uint16_t* votes_u16) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || nviews < 0 || h <= 0 || w <= 0 || nclasses < 0 || !classes || (n > 0 && !xyz) || (nviews > 0 && (!views || !masks)))
        return fail(ctx, F3D_ERR_INVALID, "project_vote_argmax: bad arguments");
    if (n == 0) return F3D_OK;
    staging st(ctx);
    const void* dxyz = st.in(xyz, xyz_bytes(dtype, n));
    const f3d_view* dviews = st.in(views, sizeof(f3d_view) * (size_t)nviews);
    const uint8_t* dmasks = st.in(masks, (size_t)nviews * h * w);
    int64_t* dcls = st.out(classes, (size_t)n * 8);
    uint16_t* dvotes = st.out(votes_u16, (size_t)n * ((size_t)nclasses + 1) * 2);
    // NumPy callers hand over clouds in arbitrary order: cell-sort large ones (results are order-independent)
    const unsigned flags = n >= 65536 ? F3D_FUSE_SORT : 0u;
    if (!st.rc) st.rc = f3d_project_vote_argmax_dev(ctx, dxyz, dtype, n, dviews, nviews, dmasks, h, w, nclasses, filter, nfilter, threshold,
                                                    dcls, dvotes, flags, nullptr, ctx->stream);
    return st.finish(F3D_DEVERR_FUSE);
}

// ---------------------------------------------------------------------------------------------
// a7 vote, a8 segment
// ---------------------------------------------------------------------------------------------
int ensure_table(f3d_ctx* ctx, int64_t hw) {
    size_t want = 1024;
    while (want < (size_t)hw * 2) want <<= 1;
    if (ctx->table_slots < want) {
        if (ctx->strict) return fail(ctx, F3D_ERR_NOMEM, "strict context: the vote table holds %zu slots, %zu needed (f3d_ctx_reserve first)", ctx->table_slots, want);
        if (ctx->table) { F3D_HIP(ctx, hipFree(ctx->table)); ctx->table = nullptr; ctx->table_slots = 0; }
        F3D_HIP(ctx, hipMalloc((void**)&ctx->table, want * sizeof(unsigned long long)));
        ctx->table_slots = want;
        ctx->table_stamped = false;
        ++ctx->allocs;
    }
    return F3D_OK;
}

int f3d_vote_uv2pt_dev(f3d_ctx* ctx, const int32_t* uv2pt, const uint8_t* mask, int64_t hw, double* votes, int64_t npts,
                       int ncols, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (hw < 0 || npts < 0 || ncols <= 0 || (hw > 0 && (!uv2pt || !mask || !votes)))
        return fail(ctx, F3D_ERR_INVALID, "vote_uv2pt: bad arguments");
    if (hw == 0) return F3D_OK;
    if ((rc = ensure_table(ctx, hw))) return rc;              // grows only when a larger frame arrives
    size_t slots = 1024;
    while (slots < (size_t)hw * 2) slots <<= 1;
    F3D_HIP(ctx, f3d_launch_vote_uv2pt(uv2pt, mask, hw, votes, npts, ncols, ctx->table, slots, ctx->dev_err, pick(ctx, stream)));
    ctx->table_stamped = false;                               // raw keys in the table: a batched call clears it first
    return F3D_OK;
}

// frames per launch of the batched vote: at most 1023 (10 bits of the key) and at most 2^25 lookups (a 512 MiB set at load <= 1/2)
static int64_t vote_batch_frames(int64_t hw) {
    int64_t per = ((int64_t)1 << 25) / hw;
    if (per < 1) per = 1;
    return per > 1023 ? 1023 : per;
}

// The launches of f3d_vote_uv2pt_batch_dev, arguments checked (nframes, hw > 0): also the vote of f3d_vote_faces_dev's passes.
static int vote_batch_enqueue(f3d_ctx* ctx, const int32_t* luts, const uint8_t* masks, int64_t nframes, int h, int w, double* votes,
                              int64_t npts, int ncols, hipStream_t s) {
    int rc;
    const int64_t hw = (int64_t)h * w;
    const int64_t per = vote_batch_frames(hw);
    const int64_t first = nframes < per ? nframes : per;
    if ((rc = ensure_table(ctx, first * hw))) return rc;
    F3D_HIP(ctx, hipMemsetAsync(ctx->first_bad, 0x7f, sizeof(int), s));                        // 0x7f7f7f7f: no bad frame
    for (int64_t f0 = 0; f0 < nframes; f0 += per) {
        const int nf = (int)(nframes - f0 < per ? nframes - f0 : per);
        if (!ctx->table_stamped || ctx->vote_gen >= 16382u) {
            F3D_HIP(ctx, hipMemsetAsync(ctx->table, 0xFF, ctx->table_slots * sizeof(unsigned long long), s));   // generation 0x3FFF = never current
            ctx->table_stamped = true; ctx->vote_gen = 0;
        }
        const unsigned gen = ctx->vote_gen++;
        size_t slots = 1024;
        while (slots < (size_t)nf * hw * 2) slots <<= 1;      // the share of the table this launch hashes into (<= table_slots)
        F3D_HIP(ctx, f3d_launch_vote_uv2pt_batch(luts + f0 * hw, masks + f0 * hw, nf, h, w, votes, npts, ncols, ctx->table, slots, gen, (int)f0,
                                                 ctx->first_bad, ctx->dev_err, s));
    }
    return F3D_OK;
}

int f3d_vote_uv2pt_batch_dev(f3d_ctx* ctx, const int32_t* luts, const uint8_t* masks, int64_t nframes, int h, int w, double* votes,
                             int64_t npts, int ncols, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    const int64_t hw = (int64_t)h * w;
    if (nframes < 0 || h < 0 || w < 0 || npts < 0 || npts >= ((int64_t)1 << 31) || ncols <= 0 || ncols > 256 ||
        (nframes > 0 && hw > 0 && (!luts || !masks || !votes)))
        return fail(ctx, F3D_ERR_INVALID, "vote_uv2pt_batch: bad arguments (npts < 2^31, ncols <= 256)");
    if (nframes == 0 || hw == 0) return F3D_OK;
    return vote_batch_enqueue(ctx, luts, masks, nframes, h, w, votes, npts, ncols, pick(ctx, stream));
}

int f3d_vote_uv2pt_batch(f3d_ctx* ctx, const int32_t* luts, const uint8_t* masks, int64_t nframes, int h, int w, double* votes,
                         int64_t npts, int ncols) {
    int rc = enter(ctx); if (rc) return rc;
    const int64_t hw = (int64_t)h * w;
    if (nframes < 0 || h < 0 || w < 0 || npts < 0 || ncols <= 0 || (nframes > 0 && hw > 0 && (!luts || !masks || !votes)))
        return fail(ctx, F3D_ERR_INVALID, "vote_uv2pt_batch: bad arguments");
    if (nframes == 0 || hw == 0) return F3D_OK;
    staging st(ctx);                                          // every frame's lookup in ONE copy, the matrix once per BATCH
    const int32_t* dlut = st.in(luts, (size_t)nframes * hw * 4);
    const uint8_t* dmask = st.in(masks, (size_t)nframes * hw);
    double* dvotes = st.inout(votes, (size_t)npts * ncols * 8);
    if (!st.rc) st.rc = f3d_vote_uv2pt_batch_dev(ctx, dlut, dmask, nframes, h, w, dvotes, npts, ncols, ctx->stream);
    return st.finish(F3D_DEVERR_VOTE, true);                  // frames before a bad one stay applied, like NumPy
}

int f3d_vote_uv2pt(f3d_ctx* ctx, const int32_t* uv2pt, const uint8_t* mask, int64_t hw, double* votes, int64_t npts, int ncols) {
    int rc = enter(ctx); if (rc) return rc;
    if (hw < 0 || npts < 0 || ncols <= 0 || (hw > 0 && (!uv2pt || !mask || !votes)))
        return fail(ctx, F3D_ERR_INVALID, "vote_uv2pt: bad arguments");
    if (hw == 0) return F3D_OK;
    staging st(ctx);
    const int32_t* dlut = st.in(uv2pt, (size_t)hw * 4);
    const uint8_t* dmask = st.in(mask, (size_t)hw);
    double* dvotes = st.inout(votes, (size_t)npts * ncols * 8);
    if (!st.rc) st.rc = f3d_vote_uv2pt_dev(ctx, dlut, dmask, hw, dvotes, npts, ncols, ctx->stream);
    return st.finish(F3D_DEVERR_VOTE);                        // nothing is written back on an IndexError
}

int f3d_segment_votes_dev(f3d_ctx* ctx, const double* votes, int64_t npts, int ncols, int nclasses, double threshold,
                          const int32_t* filter, int nfilter, int64_t* classes, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (npts < 0 || ncols <= 0 || (npts > 0 && (!votes || !classes))) return fail(ctx, F3D_ERR_INVALID, "segment_votes: bad arguments");
    hipStream_t s = pick(ctx, stream);
    f3d_filter_args fa;
    if ((rc = make_filter(ctx, filter, nfilter, ncols, true, s, &fa))) return rc;
    F3D_HIP(ctx, f3d_launch_segment_votes(votes, npts, ncols, nclasses, threshold, fa, classes, s));
    return F3D_OK;
}

int f3d_segment_votes(f3d_ctx* ctx, const double* votes, int64_t npts, int ncols, int nclasses, double threshold,
                      const int32_t* filter, int nfilter, int64_t* classes) {
    int rc = enter(ctx); if (rc) return rc;
    if (npts < 0 || ncols <= 0 || (npts > 0 && (!votes || !classes))) return fail(ctx, F3D_ERR_INVALID, "segment_votes: bad arguments");
    if (npts == 0) return F3D_OK;
    staging st(ctx);
    const double* dvotes = st.in(votes, (size_t)npts * ncols * 8);
    int64_t* dcls = st.out(classes, (size_t)npts * 8);
    if (!st.rc) st.rc = f3d_segment_votes_dev(ctx, dvotes, npts, ncols, nclasses, threshold, filter, nfilter, dcls, ctx->stream);
    return st.finish();
}

int f3d_segment_votes_lastcol_dev(f3d_ctx* ctx, const double* votes, int64_t npts, int ncols, int nclasses, double threshold,
                                  const int32_t* filter, int nfilter, int64_t* classes, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (npts < 0 || ncols <= 0 || (npts > 0 && (!votes || !classes))) return fail(ctx, F3D_ERR_INVALID, "segment_votes_lastcol: bad arguments");
    if (ncols < 2 && nfilter == 0 && npts > 0)                 // votes[:, :-1] has no column: NumPy's argmax raises ValueError
        return fail(ctx, F3D_ERR_INVALID, "segment_votes_lastcol: attempt to get argmax of an empty sequence");
    hipStream_t s = pick(ctx, stream);
    f3d_filter_args fa;
    if ((rc = make_filter(ctx, filter, nfilter, ncols, true, s, &fa))) return rc;
    f3d_negmask neg = {};
    for (int k = 0; k < fa.nfilter; ++k) if (filter[k] < 0) neg.w[k >> 5] |= 1u << (k & 31);
    F3D_HIP(ctx, f3d_launch_segment_votes_lastcol(votes, npts, ncols, nclasses, threshold, fa, neg, classes, s));
    return F3D_OK;
}

int f3d_segment_votes_lastcol(f3d_ctx* ctx, const double* votes, int64_t npts, int ncols, int nclasses, double threshold,
                              const int32_t* filter, int nfilter, int64_t* classes) {
    int rc = enter(ctx); if (rc) return rc;
    if (npts < 0 || ncols <= 0 || (npts > 0 && (!votes || !classes))) return fail(ctx, F3D_ERR_INVALID, "segment_votes_lastcol: bad arguments");
    if (npts == 0) return F3D_OK;
    staging st(ctx);
    const double* dvotes = st.in(votes, (size_t)npts * ncols * 8);
    int64_t* dcls = st.out(classes, (size_t)npts * 8);
    if (!st.rc) st.rc = f3d_segment_votes_lastcol_dev(ctx, dvotes, npts, ncols, nclasses, threshold, filter, nfilter, dcls, ctx->stream);
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// a9 mask post-processing
// ---------------------------------------------------------------------------------------------
int f3d_sem_logits_to_mask_dev(f3d_ctx* ctx, const float* sem, int c, int64_t hw, float conf, int low_label, uint8_t* mask,
                               void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (c <= 0 || c > 256 || hw < 0 || low_label < 0 || low_label > 255 || (hw > 0 && (!sem || !mask)))
        return fail(ctx, F3D_ERR_INVALID, "sem_logits_to_mask: bad arguments (1 <= c <= 256)");
    F3D_HIP(ctx, f3d_launch_sem_to_mask(sem, 1, c, hw, conf, low_label, mask, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_sem_logits_to_masks_dev(f3d_ctx* ctx, const float* sem, int nimg, int c, int64_t hw, float conf, int low_label, uint8_t* masks,
                                void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (nimg < 0 || nimg > 65535 || c <= 0 || c > 256 || hw < 0 || low_label < 0 || low_label > 255 || (nimg > 0 && hw > 0 && (!sem || !masks)))
        return fail(ctx, F3D_ERR_INVALID, "sem_logits_to_masks: bad arguments (1 <= c <= 256, at most 65535 images per call)");
    F3D_HIP(ctx, f3d_launch_sem_to_mask(sem, nimg, c, hw, conf, low_label, masks, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_sem_logits_to_mask(f3d_ctx* ctx, const float* sem, int c, int64_t hw, float conf, int low_label, uint8_t* mask) {
    int rc = enter(ctx); if (rc) return rc;
    if (c <= 0 || hw < 0 || (hw > 0 && (!sem || !mask))) return fail(ctx, F3D_ERR_INVALID, "sem_logits_to_mask: bad arguments");
    if (hw == 0) return F3D_OK;
    staging st(ctx);
    const float* dsem = st.in(sem, (size_t)c * hw * 4);
    uint8_t* dmask = st.out(mask, (size_t)hw);
    if (!st.rc) st.rc = f3d_sem_logits_to_mask_dev(ctx, dsem, c, hw, conf, low_label, dmask, ctx->stream);
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// a10/a11 oriented boxes
// ---------------------------------------------------------------------------------------------
int f3d_points_in_obb_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_obb* boxes, int b,
                          uint32_t* inside_bits, uint8_t* cooc, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || b < 0 || b > F3D_OBB_MAX_BOXES || (b > 0 && !boxes) || (n > 0 && !xyz) || (!inside_bits && !cooc))
        return fail(ctx, F3D_ERR_INVALID, "points_in_obb: bad arguments (at most %d boxes per call)", F3D_OBB_MAX_BOXES);
    if (b == 0) return F3D_OK;
    hipStream_t s = pick(ctx, stream);
    void* dboxes;                                              // the cell table (8-byte aligned), the boxes, then their float32 bounds
    const size_t cells = f3d_obb_cells_bytes();
    if ((rc = ensure(ctx, SLOT_OBB_BOXES, cells + (sizeof(f3d_obb) + 6 * sizeof(float)) * (size_t)b, &dboxes))) return rc;
    char* base = (char*)dboxes + cells;
    F3D_HIP(ctx, hipMemcpyAsync(base, boxes, sizeof(f3d_obb) * (size_t)b, hipMemcpyHostToDevice, s));
    F3D_HIP(ctx, f3d_launch_points_in_obb(xyz, dtype, n, (const f3d_obb*)base, b, (float*)(base + sizeof(f3d_obb) * (size_t)b), dboxes, inside_bits, cooc, s));
    return F3D_OK;
}

int f3d_points_in_obb(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_obb* boxes, int b,
                      uint32_t* inside_bits, uint8_t* cooc) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || b < 0 || (n > 0 && !xyz) || (!inside_bits && !cooc)) return fail(ctx, F3D_ERR_INVALID, "points_in_obb: bad arguments");
    if (b == 0) return F3D_OK;
    staging st(ctx);
    const void* dxyz = st.in(xyz, xyz_bytes(dtype, n));
    uint32_t* dbits = st.out(inside_bits, (size_t)n * (((size_t)b + 31) / 32) * 4);
    uint8_t* dcooc = st.out(cooc, (size_t)b * b);
    if (st.rc) return st.rc;
    if (dcooc && n == 0) F3D_HIP(ctx, hipMemsetAsync(dcooc, 0, (size_t)b * b, ctx->stream));
    st.rc = f3d_points_in_obb_dev(ctx, dxyz, dtype, n, boxes, b, dbits, dcooc, ctx->stream);
    return st.finish();
}

int f3d_relabel_dev(f3d_ctx* ctx, int64_t* ids, int64_t n, int64_t from, int64_t to, int64_t* count_dev, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || (n > 0 && !ids)) return fail(ctx, F3D_ERR_INVALID, "relabel: bad arguments");
    hipStream_t s = pick(ctx, stream);
    if (count_dev) F3D_HIP(ctx, hipMemsetAsync(count_dev, 0, 8, s));
    F3D_HIP(ctx, f3d_launch_relabel(ids, n, from, to, (unsigned long long*)count_dev, s));
    return F3D_OK;
}

int f3d_relabel(f3d_ctx* ctx, int64_t* ids, int64_t n, int64_t from, int64_t to, int64_t* count) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || (n > 0 && !ids)) return fail(ctx, F3D_ERR_INVALID, "relabel: bad arguments");
    if (count) *count = 0;
    if (n == 0) return F3D_OK;
    staging st(ctx);
    int64_t* dids = st.inout(ids, (size_t)n * 8);
    st.back(count, ctx->count_dev, 8);
    if (!st.rc) st.rc = f3d_relabel_dev(ctx, dids, n, from, to, (int64_t*)ctx->count_dev, ctx->stream);
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// a12 remaining intersections.py primitives (host pointers)
// ---------------------------------------------------------------------------------------------
int f3d_ray_x_lines(f3d_ctx* ctx, const double origin[3], const double direction[3], const double* starts, const double* ends, int64_t n,
                    double* points, uint8_t* within) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || !origin || !direction || (n > 0 && (!starts || !ends || !points || !within))) return fail(ctx, F3D_ERR_INVALID, "ray_x_lines: bad arguments");
    if (n == 0) return F3D_OK;
    staging st(ctx);
    const double* ds = st.in(starts, (size_t)n * 24);
    const double* de = st.in(ends, (size_t)n * 24);
    double* dp = st.out(points, (size_t)n * 24);
    uint8_t* dw = st.out(within, (size_t)n);
    if (st.rc) return st.rc;
    F3D_HIP(ctx, f3d_launch_ray_x_lines(origin, direction, ds, de, n, dp, dw, ctx->stream));
    return st.finish();
}

int f3d_rays_x_plane(f3d_ctx* ctx, const double pp[3], const double pn[3], const double* origins, const double* dirs, int64_t n, double* points,
                     uint8_t* valid) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || !pp || !pn || (n > 0 && (!origins || !dirs || !points || !valid))) return fail(ctx, F3D_ERR_INVALID, "rays_x_plane: bad arguments");
    if (n == 0) return F3D_OK;
    staging st(ctx);
    const double* d_o = st.in(origins, (size_t)n * 24);
    const double* dd = st.in(dirs, (size_t)n * 24);
    double* dp = st.out(points, (size_t)n * 24);
    uint8_t* dv = st.out(valid, (size_t)n);
    if (st.rc) return st.rc;
    F3D_HIP(ctx, f3d_launch_rays_x_plane(pp, pn, d_o, dd, n, dp, dv, ctx->stream));
    return st.finish();
}

int f3d_lines_x_planes(f3d_ctx* ctx, const double* lo, const double* le, int64_t n, const double* pps, const double* pns, int m, double* points,
                       uint8_t* valid) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || m < 0 || (n > 0 && (!lo || !le)) || (m > 0 && (!pps || !pns)) || (n > 0 && m > 0 && (!points || !valid)))
        return fail(ctx, F3D_ERR_INVALID, "lines_x_planes: bad arguments");
    if (n != 1 && n != m) return fail(ctx, F3D_ERR_INVALID, "operands could not be broadcast together with shapes (%lld,%d,3) (%lld,3)", (long long)n, m, (long long)n);
    if (n == 0 || m == 0) return F3D_OK;
    staging st(ctx);
    const double* d_o = st.in(lo, (size_t)n * 24);
    const double* de = st.in(le, (size_t)n * 24);
    const double* dpp = st.in(pps, (size_t)m * 24);
    const double* dpn = st.in(pns, (size_t)m * 24);
    double* dp = st.out(points, (size_t)n * m * 24);
    uint8_t* dv = st.out(valid, (size_t)n * m);
    if (st.rc) return st.rc;
    F3D_HIP(ctx, f3d_launch_lines_x_planes(d_o, de, n, dpp, dpn, m, n == 1 ? 0 : 1, dp, dv, ctx->stream));
    return st.finish();
}

int f3d_point_inside_polygon(f3d_ctx* ctx, const double* points, int64_t n, const double* verts, int m, uint8_t* inside, uint8_t* within) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || m < 1 || !verts || (n > 0 && (!points || !inside || !within))) return fail(ctx, F3D_ERR_INVALID, "point_inside_polygon: bad arguments");
    if (n == 0) return F3D_OK;
    staging st(ctx);
    const double* dp = st.in(points, (size_t)n * 24);
    const double* dv = st.in(verts, (size_t)m * 24);
    uint8_t* di = st.out(inside, (size_t)n);
    uint8_t* dw = st.out(within, (size_t)n * m);
    if (st.rc) return st.rc;
    F3D_HIP(ctx, f3d_launch_point_inside_polygon(dp, n, dv, m, di, dw, ctx->stream));
    return st.finish();
}

int f3d_points_plane_projection(f3d_ctx* ctx, const double* points, int64_t n, const double pp[3], const double nr[3], double* out) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || !pp || !nr || (n > 0 && (!points || !out))) return fail(ctx, F3D_ERR_INVALID, "points_plane_projection: bad arguments");
    if (n == 0) return F3D_OK;
    staging st(ctx);
    const double* dp = st.in(points, (size_t)n * 24);
    double* d_o = st.out(out, (size_t)n * 24);
    if (st.rc) return st.rc;
    F3D_HIP(ctx, f3d_launch_points_plane_projection(dp, n, pp, nr, d_o, ctx->stream));
    return st.finish();
}

int f3d_lines_plane_projection(f3d_ctx* ctx, const double* starts, const double* ends, int64_t n, const double pp[3], const double nr[3],
                               double* sp, double* ep, double* dirs) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || !pp || !nr || (n > 0 && (!starts || !ends || !sp || !ep || !dirs))) return fail(ctx, F3D_ERR_INVALID, "lines_plane_projection: bad arguments");
    if (n == 0) return F3D_OK;
    staging st(ctx);
    const double* ds = st.in(starts, (size_t)n * 24);
    const double* de = st.in(ends, (size_t)n * 24);
    double* dsp = st.out(sp, (size_t)n * 24);
    double* dep = st.out(ep, (size_t)n * 24);
    double* dd = st.out(dirs, (size_t)n * 24);
    if (st.rc) return st.rc;
    F3D_HIP(ctx, f3d_launch_points_plane_projection(ds, n, pp, nr, dsp, ctx->stream));
    F3D_HIP(ctx, f3d_launch_points_plane_projection(de, n, pp, nr, dep, ctx->stream));
    F3D_HIP(ctx, f3d_launch_unit_difference(dsp, dep, n, dd, ctx->stream));
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// (f)#1 same-class connected components
// ---------------------------------------------------------------------------------------------
int f3d_components_same_class_dev(f3d_ctx* ctx, const int64_t* classes, int64_t n, const int64_t* offsets, const int32_t* nbrs,
                                  int32_t* parent, int64_t* root, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n > 0x7fffffffLL || (n > 0 && (!classes || !offsets || !parent || !root)))
        return fail(ctx, F3D_ERR_INVALID, "components_same_class: bad arguments (n < 2^31)");
    F3D_HIP(ctx, f3d_launch_components(classes, n, offsets, nbrs, parent, root, ctx->dev_err, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_components_same_class(f3d_ctx* ctx, const int64_t* classes, int64_t n, const int64_t* offsets, const int32_t* nbrs,
                              int64_t* root) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || (n > 0 && (!classes || !offsets || !root))) return fail(ctx, F3D_ERR_INVALID, "components_same_class: bad arguments");
    if (n == 0) return F3D_OK;
    const int64_t e = offsets[n];
    if (e < 0 || (e > 0 && !nbrs)) return fail(ctx, F3D_ERR_INVALID, "components_same_class: bad adjacency");
    staging st(ctx);
    const int64_t* dcls = st.in(classes, (size_t)n * 8);
    const int64_t* doffs = st.in(offsets, (size_t)(n + 1) * 8);
    const int32_t* dnb = st.in(nbrs, (size_t)e * 4);
    int32_t* dpar = (int32_t*)st.slot((size_t)n * 4);
    int64_t* droot = st.out(root, (size_t)n * 8);
    if (!st.rc) st.rc = f3d_components_same_class_dev(ctx, dcls, n, doffs, dnb, dpar, droot, ctx->stream);
    return st.finish(F3D_DEVERR_CC);
}

// ---------------------------------------------------------------------------------------------
// CVSegmentation: ordered same-class flood and colour growing
// ---------------------------------------------------------------------------------------------
#define F3D_CVSEG_RESERVED_LIST 4096         // instance classes / seeds that f3d_ctx_reserve_cvseg makes room for

int f3d_ctx_reserve_cvseg(f3d_ctx* ctx, int64_t n) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n > 0x7fffffffLL) return fail(ctx, F3D_ERR_INVALID, "ctx_reserve_cvseg: bad arguments");
    return reserve(ctx, {{SLOT_FLOOD, f3d_flood_scratch_bytes(n)}, {SLOT_COLOR, f3d_color_scratch_bytes(n)},
                         {SLOT_CVS_INST, F3D_CVSEG_RESERVED_LIST * 8}, {SLOT_CVS_STATS, 16}});
}

int f3d_flood_order_dev(f3d_ctx* ctx, const int64_t* classes, int64_t n, const int64_t* offsets, const int32_t* nbrs,
                        const int64_t* inst, int ninst, int64_t* root, int64_t* order, int64_t* coffs, uint8_t* flags,
                        int64_t stats[4], void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!stats || n < 0 || n > 0x7fffffffLL || ninst < 0 || (ninst > 0 && !inst) ||
        (n > 0 && (!classes || !offsets || !root || !order || !coffs || !flags)))
        return fail(ctx, F3D_ERR_INVALID, "flood_order: bad arguments (n < 2^31)");
    for (int q = 0; q < 4; ++q) stats[q] = 0;
    if (n == 0) return F3D_OK;
    hipStream_t s = pick(ctx, stream);
    void *scratch, *dinst;
    if ((rc = ensure(ctx, SLOT_FLOOD, f3d_flood_scratch_bytes(n), &scratch))) return rc;
    if ((rc = ensure(ctx, SLOT_CVS_INST, (size_t)(ninst > 0 ? ninst : 1) * 8, &dinst))) return rc;
    if (ninst > 0) F3D_HIP(ctx, hipMemcpyAsync(dinst, inst, (size_t)ninst * 8, hipMemcpyHostToDevice, s));   // the launch synchronises
    F3D_HIP(ctx, f3d_launch_flood_order(classes, n, offsets, nbrs, (const int64_t*)dinst, ninst, root, order, coffs, flags, scratch,
                                        ctx->dev_err, stats, s));
    return take_error(ctx, s, F3D_DEVERR_FLOOD);
}

int f3d_flood_order(f3d_ctx* ctx, const int64_t* classes, int64_t n, const int64_t* offsets, const int32_t* nbrs,
                    const int64_t* inst, int ninst, int64_t* root, int64_t* order, int64_t* coffs, uint8_t* flags, int64_t stats[4]) {
    int rc = enter(ctx); if (rc) return rc;
    if (!stats || n < 0 || (n > 0 && (!classes || !offsets || !root || !order || !coffs || !flags)))
        return fail(ctx, F3D_ERR_INVALID, "flood_order: bad arguments");
    for (int q = 0; q < 4; ++q) stats[q] = 0;
    if (n == 0) { coffs[0] = 0; return F3D_OK; }
    const int64_t e = offsets[n];
    if (e < 0 || (e > 0 && !nbrs)) return fail(ctx, F3D_ERR_INVALID, "flood_order: bad adjacency");
    staging st(ctx);
    const int64_t* dcls = st.in(classes, (size_t)n * 8);
    const int64_t* doffs = st.in(offsets, (size_t)(n + 1) * 8);
    const int32_t* dnb = st.in(nbrs, (size_t)e * 4);
    int64_t* droot = st.out(root, (size_t)n * 8);
    int64_t* dorder = st.out(order, (size_t)n * 8);
    int64_t* dcoffs = st.out(coffs, (size_t)(n + 1) * 8);
    uint8_t* dflags = st.out(flags, (size_t)n);
    if (!st.rc) st.rc = f3d_flood_order_dev(ctx, dcls, n, doffs, dnb, inst, ninst, droot, dorder, dcoffs, dflags, stats, ctx->stream);
    return st.finish();
}

static int color_args(f3d_ctx* ctx, const double threshold[3], const int64_t* neutral_ids, int nneutral, int max_level, f3d_color_args* a) {
    if (!threshold || nneutral < 0 || nneutral > F3D_COLOR_MAX_NEUTRAL || (nneutral > 0 && !neutral_ids))
        return fail(ctx, F3D_ERR_INVALID, "color_segment: bad threshold or neutral ids (at most %d)", F3D_COLOR_MAX_NEUTRAL);
    for (int c = 0; c < 3; ++c) a->thr[c] = threshold[c];
    a->max_level = max_level;
    a->nneutral = nneutral;
    for (int k = 0; k < F3D_COLOR_MAX_NEUTRAL; ++k) a->neutral[k] = k < nneutral ? neutral_ids[k] : 0;
    return F3D_OK;
}

int f3d_color_segment_dev(f3d_ctx* ctx, const void* colors, f3d_dtype dtype, int64_t n, const int64_t* offsets, const int32_t* nbrs,
                          int64_t* ids, const int64_t* seeds, int64_t nseeds, const double threshold[3], const int64_t* neutral_ids,
                          int nneutral, int max_level, int64_t* accepted_dev, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n > 0x7fffffffLL || nseeds < 0 || !dtype_ok(dtype) ||
        (n > 0 && nseeds > 0 && (!colors || !offsets || !ids || !seeds)))
        return fail(ctx, F3D_ERR_INVALID, "color_segment: bad arguments (n < 2^31, float64 or float32 colours)");
    f3d_color_args a;
    if ((rc = color_args(ctx, threshold, neutral_ids, nneutral, max_level, &a))) return rc;
    if (nseeds > 0 && n == 0) return fail(ctx, F3D_ERR_INDEX, "color_segment: seed index out of bounds");
    if (n == 0 || nseeds == 0) return F3D_OK;
    hipStream_t s = pick(ctx, stream);
    void* scratch;
    if ((rc = ensure(ctx, SLOT_COLOR, f3d_color_scratch_bytes(n), &scratch))) return rc;
    if (!accepted_dev) {
        void* p;
        if ((rc = ensure(ctx, SLOT_CVS_STATS, 16, &p))) return rc;
        accepted_dev = (int64_t*)p;
    }
    F3D_HIP(ctx, f3d_launch_color_segment(colors, dtype, n, offsets, nbrs, ids, seeds, nseeds, a, scratch, accepted_dev, ctx->dev_err, s));
    return F3D_OK;
}

int f3d_color_segment(f3d_ctx* ctx, const void* colors, f3d_dtype dtype, int64_t n, const int64_t* offsets, const int32_t* nbrs,
                      int64_t* ids, const int64_t* seeds, int64_t nseeds, const double threshold[3], const int64_t* neutral_ids,
                      int nneutral, int max_level, int64_t* accepted) {
    int rc = enter(ctx); if (rc) return rc;
    if (accepted) *accepted = 0;
    if (n < 0 || nseeds < 0 || !dtype_ok(dtype) || (n > 0 && nseeds > 0 && (!colors || !offsets || !ids || !seeds)))
        return fail(ctx, F3D_ERR_INVALID, "color_segment: bad arguments (float64 or float32 colours)");
    f3d_color_args a;
    if ((rc = color_args(ctx, threshold, neutral_ids, nneutral, max_level, &a))) return rc;
    if (nseeds > 0 && n == 0) return fail(ctx, F3D_ERR_INDEX, "color_segment: seed index out of bounds");
    if (n == 0 || nseeds == 0) return F3D_OK;
    for (int64_t k = 0; k < nseeds; ++k)
        if (seeds[k] < 0 || seeds[k] >= n) return fail(ctx, F3D_ERR_INDEX, "color_segment: seed index %lld out of bounds", (long long)seeds[k]);
    const int64_t e = offsets[n];
    if (e < 0 || (e > 0 && !nbrs)) return fail(ctx, F3D_ERR_INVALID, "color_segment: bad adjacency");
    staging st(ctx);
    const void* dclr = st.in((const char*)colors, xyz_bytes(dtype, n));
    const int64_t* doffs = st.in(offsets, (size_t)(n + 1) * 8);
    const int32_t* dnb = st.in(nbrs, (size_t)e * 4);
    const int64_t* dseeds = st.in(seeds, (size_t)nseeds * 8);
    int64_t* dids = st.inout(ids, (size_t)n * 8);
    int64_t* dacc = (int64_t*)st.slot(16);
    if (!st.rc) st.rc = hipMemsetAsync(dacc, 0, 8, ctx->stream) == hipSuccess ? F3D_OK : fail(ctx, F3D_ERR_HIP, "color_segment: memset");
    st.back(accepted, dacc, accepted ? 8 : 0);
    if (!st.rc) st.rc = f3d_color_segment_dev(ctx, dclr, dtype, n, doffs, dnb, dids, dseeds, nseeds, threshold, neutral_ids, nneutral,
                                              max_level, dacc, ctx->stream);
    return st.finish(F3D_DEVERR_COLOR);
}

// ---------------------------------------------------------------------------------------------
// refinement: region growing of a picked instance, distance to the wall plane
// ---------------------------------------------------------------------------------------------
int f3d_ctx_reserve_refine(f3d_ctx* ctx, int64_t n) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n > F3D_GROW_MAX_POINTS) return fail(ctx, F3D_ERR_INVALID, "ctx_reserve_refine: bad arguments (n <= 2^31 - 2049)");
    return reserve(ctx, {{SLOT_GROW, f3d_grow_scratch_bytes(n)}});
}

static int grow_args(f3d_ctx* ctx, f3d_dtype dtype, int nchan, int64_t n, int64_t nseeds, const double* sma0, int64_t npts0, int seeds_given,
                     const double* threshold, int max_level, f3d_grow_args* a) {
    if (n < 0 || n > F3D_GROW_MAX_POINTS || nseeds < 0 || npts0 < 0 || !sma0 || !threshold ||
        !((nchan == 1 && dtype == F3D_F64) || (nchan == 3 && dtype_ok(dtype))))
        return fail(ctx, F3D_ERR_INVALID, "region_grow: bad arguments (n <= 2^31 - 2049; float64 [n, 1], or float64 / float32 [n, 3] values)");
    for (int c = 0; c < 3; ++c) { a->thr[c] = c < nchan ? threshold[c] : 0; a->sma0[c] = c < nchan ? sma0[c] : 0; }
    a->npts0 = npts0;
    a->max_level = max_level;
    a->seeds_given = seeds_given != 0;
    if (nseeds > n) return fail(ctx, F3D_ERR_INDEX, "region_grow: more seeds than points (a seed is out of bounds or listed twice)");
    return F3D_OK;
}

int f3d_region_grow_dev(f3d_ctx* ctx, const void* values, f3d_dtype dtype, int nchan, int64_t n, const int64_t* offsets, const int32_t* nbrs,
                        const int64_t* seeds, int64_t nseeds, const double* sma0, int64_t npts0, int seeds_given, const double* threshold,
                        int max_level, int64_t* cluster, int64_t* count_dev, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    f3d_grow_args a;
    if ((rc = grow_args(ctx, dtype, nchan, n, nseeds, sma0, npts0, seeds_given, threshold, max_level, &a))) return rc;
    if (!count_dev || (n > 0 && (!values || !offsets || !cluster)) || (nseeds > 0 && !seeds))
        return fail(ctx, F3D_ERR_INVALID, "region_grow: NULL argument");
    hipStream_t s = pick(ctx, stream);
    if (n == 0) {
        F3D_HIP(ctx, hipMemsetAsync(count_dev, 0, 8, s));
        return F3D_OK;
    }
    void* scratch;
    if ((rc = ensure(ctx, SLOT_GROW, f3d_grow_scratch_bytes(n), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_region_grow(values, dtype, nchan, n, offsets, nbrs, seeds, nseeds, a, scratch, cluster, count_dev, ctx->dev_err, s));
    return F3D_OK;
}

int f3d_region_grow(f3d_ctx* ctx, const void* values, f3d_dtype dtype, int nchan, int64_t n, const int64_t* offsets, const int32_t* nbrs,
                    const int64_t* seeds, int64_t nseeds, const double* sma0, int64_t npts0, int seeds_given, const double* threshold,
                    int max_level, int64_t* cluster, int64_t* count) {
    int rc = enter(ctx); if (rc) return rc;
    if (count) *count = 0;
    f3d_grow_args a;
    if ((rc = grow_args(ctx, dtype, nchan, n, nseeds, sma0, npts0, seeds_given, threshold, max_level, &a))) return rc;
    if (!count || (n > 0 && (!values || !offsets || !cluster)) || (nseeds > 0 && !seeds)) return fail(ctx, F3D_ERR_INVALID, "region_grow: NULL argument");
    if (n == 0 || nseeds == 0) return F3D_OK;
    const int64_t e = offsets[n];
    if (e < 0 || (e > 0 && !nbrs)) return fail(ctx, F3D_ERR_INVALID, "region_grow: bad adjacency");
    staging st(ctx);
    const void* dval = st.in((const char*)values, (size_t)n * nchan * (dtype == F3D_F64 ? 8 : 4));
    const int64_t* doffs = st.in(offsets, (size_t)(n + 1) * 8);
    const int32_t* dnb = st.in(nbrs, (size_t)e * 4);
    const int64_t* dseeds = st.in(seeds, (size_t)nseeds * 8);
    int64_t* dcl = st.out(cluster, (size_t)n * 8);
    int64_t* dcount = st.out(count, 8);
    if (!st.rc) st.rc = f3d_region_grow_dev(ctx, dval, dtype, nchan, n, doffs, dnb, dseeds, nseeds, sma0, npts0, seeds_given, threshold,
                                            max_level, dcl, dcount, ctx->stream);
    return st.finish(F3D_DEVERR_GROW);
}

int f3d_plane_distance_dev(f3d_ctx* ctx, const double* points, int64_t n, const double plane_point[3], const double normal[3], double* out,
                           void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || !plane_point || !normal || (n > 0 && (!points || !out))) return fail(ctx, F3D_ERR_INVALID, "plane_distance: bad arguments");
    F3D_HIP(ctx, f3d_launch_plane_distance(points, n, plane_point, normal, out, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_plane_distance(f3d_ctx* ctx, const double* points, int64_t n, const double plane_point[3], const double normal[3], double* out) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || !plane_point || !normal || (n > 0 && (!points || !out))) return fail(ctx, F3D_ERR_INVALID, "plane_distance: bad arguments");
    if (n == 0) return F3D_OK;
    staging st(ctx);
    const double* dpts = st.in(points, (size_t)n * 24);
    double* dout = st.out(out, (size_t)n * 8);
    if (!st.rc) st.rc = f3d_plane_distance_dev(ctx, dpts, n, plane_point, normal, dout, ctx->stream);
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// door_window_bbox.generate_mesh: door / window quads on the mesh
// ---------------------------------------------------------------------------------------------
static bool quads_args_ok(int64_t n, int k, int64_t nv, int64_t nt) {
    return n >= 0 && n <= 0x7fffffffLL && k >= 0 && k <= F3D_QUADS_MAX_INST && nv >= 0 && nt >= 0 && nt <= 0x7fffffffLL;
}

int f3d_ctx_reserve_quads(f3d_ctx* ctx, int64_t n, int k, int64_t nt) {
    int rc = enter(ctx); if (rc) return rc;
    if (!quads_args_ok(n, k, 0, nt)) return fail(ctx, F3D_ERR_INVALID, "ctx_reserve_quads: bad arguments");
    return reserve(ctx, {{SLOT_QUADS, f3d_quads_scratch_bytes(n, k, nt)}});
}

// the argument test of f3d_door_window_quads and of its _dev twin
static int quads_check(f3d_ctx* ctx, const double* points, int64_t n, const int64_t* ids, const int64_t* inst, int k, const double* verts,
                       int64_t nv, const int64_t* tris, int64_t nt, const double* quads, const int32_t* status, const int32_t* tri) {
    if (!quads_args_ok(n, k, nv, nt) || (n > 0 && (!points || !ids)) || (k > 0 && (!inst || !quads || !status || !tri)) ||
        (nv > 0 && !verts) || (nt > 0 && !tris))
        return fail(ctx, F3D_ERR_INVALID, "door_window_quads: bad arguments (n, nt < 2^31, k <= %d)", F3D_QUADS_MAX_INST);
    return F3D_OK;
}

int f3d_door_window_quads_dev(f3d_ctx* ctx, const double* points, int64_t n, const int64_t* ids, const int64_t* inst, int k,
                              const double* verts, int64_t nv, const int64_t* tris, int64_t nt, double* quads, int32_t* status,
                              int32_t* tri, double* normals, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if ((rc = quads_check(ctx, points, n, ids, inst, k, verts, nv, tris, nt, quads, status, tri))) return rc;
    void* scratch;
    if ((rc = ensure(ctx, SLOT_QUADS, f3d_quads_scratch_bytes(n, k, nt), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_door_window_quads(points, n, ids, inst, k, verts, nv, tris, nt, quads, status, tri, normals, scratch,
                                              ctx->dev_err, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_door_window_quads(f3d_ctx* ctx, const double* points, int64_t n, const int64_t* ids, const int64_t* inst, int k,
                          const double* verts, int64_t nv, const int64_t* tris, int64_t nt, double* quads, int32_t* status,
                          int32_t* tri, double* normals) {
    int rc = enter(ctx); if (rc) return rc;
    if ((rc = quads_check(ctx, points, n, ids, inst, k, verts, nv, tris, nt, quads, status, tri))) return rc;
    staging st(ctx);
    const double* dpts = st.in(points, (size_t)n * 24);
    const int64_t* dids = st.in(ids, (size_t)n * 8);
    const int64_t* dinst = st.in(inst, (size_t)k * 8);
    const double* dverts = st.in(verts, (size_t)nv * 24);
    const int64_t* dtris = st.in(tris, (size_t)nt * 24);
    double* dquads = st.out(quads, (size_t)k * 96);
    int32_t* dstatus = st.out(status, (size_t)k * 4);
    int32_t* dtri = st.out(tri, (size_t)k * 4);
    double* dnrm = st.out(normals, (size_t)nt * 24);
    if (!st.rc) st.rc = f3d_door_window_quads_dev(ctx, dpts, n, dids, dinst, k, dverts, nv, dtris, nt, dquads, dstatus, dtri, dnrm,
                                                  ctx->stream);
    return st.finish(F3D_DEVERR_QUADS);
}

// ---------------------------------------------------------------------------------------------
// extract_planes: the plane table of a cloud over its adjacency
// ---------------------------------------------------------------------------------------------
int f3d_ctx_reserve_planes(f3d_ctx* ctx, int64_t n) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n > 0x7fffffffLL) return fail(ctx, F3D_ERR_INVALID, "ctx_reserve_planes: bad arguments (n < 2^31)");
    return reserve(ctx, {{SLOT_PLANES, f3d_planes_scratch_bytes(n)}});
}

static bool planes_args_bad(f3d_dtype dtype, int64_t n, const void* xyz, const void* offsets, int64_t min_points, int64_t max_rounds,
                            int64_t max_planes, const void* labels, const void* planes, const void* corners, const void* counts) {
    return !dtype_ok(dtype) || n < 0 || n > 0x7fffffffLL || min_points < 3 || max_rounds < 0 || max_planes < 0 || !counts ||
           (n > 0 && (!xyz || !offsets || !labels)) || (max_planes > 0 && (!planes || !corners));
}
#define F3D_PLANES_BAD "extract_planes: bad arguments (n < 2^31, min_points >= 3, max_rounds >= 0, max_planes >= 0)"

int f3d_extract_planes_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const int64_t* offsets, const int32_t* neighbours,
                           const double* normals, double cos_angle, double offset, double dist, double max_variation, int64_t min_points,
                           int64_t max_rounds, int64_t max_planes, int32_t* labels, double* planes, double* corners, int64_t* counts,
                           double* normals_out, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (planes_args_bad(dtype, n, xyz, offsets, min_points, max_rounds, max_planes, labels, planes, corners, counts))
        return fail(ctx, F3D_ERR_INVALID, F3D_PLANES_BAD);
    hipStream_t s = pick(ctx, stream);
    if (n == 0) {
        F3D_HIP(ctx, hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s));
        if (max_planes > 0) {
            F3D_HIP(ctx, hipMemsetAsync(planes, 0, (size_t)max_planes * 8 * sizeof(double), s));
            F3D_HIP(ctx, hipMemsetAsync(corners, 0, (size_t)max_planes * 12 * sizeof(double), s));
        }
        return F3D_OK;
    }
    void* scratch;
    if ((rc = ensure(ctx, SLOT_PLANES, f3d_planes_scratch_bytes(n), &scratch))) return rc;
    const f3d_planes_args a = {cos_angle, offset, dist, max_variation, min_points, max_rounds, max_planes};
    F3D_HIP(ctx, f3d_launch_extract_planes(xyz, dtype, n, offsets, neighbours, normals, a, labels, planes, corners, counts, normals_out,
                                           scratch, ctx->dev_err, s));
    return F3D_OK;
}

int f3d_extract_planes(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const int64_t* offsets, const int32_t* neighbours,
                       const double* normals, double cos_angle, double offset, double dist, double max_variation, int64_t min_points,
                       int64_t max_rounds, int64_t max_planes, int32_t* labels, double* planes, double* corners, int64_t* counts,
                       double* normals_out) {
    int rc = enter(ctx); if (rc) return rc;
    if (planes_args_bad(dtype, n, xyz, offsets, min_points, max_rounds, max_planes, labels, planes, corners, counts))
        return fail(ctx, F3D_ERR_INVALID, F3D_PLANES_BAD);
    const int64_t e = n > 0 ? offsets[n] : 0;
    if (e < 0 || (e > 0 && !neighbours)) return fail(ctx, F3D_ERR_INVALID, "extract_planes: bad adjacency");
    f3d_carve c;
    const size_t nb = (size_t)n * 24, pb = (size_t)max_planes * 64, cb = (size_t)max_planes * 96;
    const size_t o_xyz = c.take(xyz_bytes(dtype, n)), o_offs = c.take((size_t)(n + 1) * 8), o_nbrs = c.take((size_t)e * 4), o_nin = c.take(nb),
                 o_lab = c.take((size_t)n * 4), o_pl = c.take(pb), o_cr = c.take(cb), o_cnt = c.take(32), o_nout = c.take(nb);
    staging st(ctx);
    char* io = (char*)st.slot(c.off);
    if (st.rc) return st.rc;
    st.put(io + o_xyz, xyz, xyz_bytes(dtype, n));
    st.put(io + o_offs, offsets, (size_t)(n + 1) * 8);
    st.put(io + o_nbrs, neighbours, (size_t)e * 4);
    st.put(io + o_nin, normals, nb);
    st.back(labels, io + o_lab, (size_t)n * 4);
    st.back(planes, io + o_pl, pb);
    st.back(corners, io + o_cr, cb);
    st.back(counts, io + o_cnt, 32);
    if (!normals) st.back(normals_out, io + o_nout, nb);
    if (!st.rc) st.rc = f3d_extract_planes_dev(ctx, io + o_xyz, dtype, n, (const int64_t*)(io + o_offs), (const int32_t*)(io + o_nbrs),
                                               normals ? (const double*)(io + o_nin) : nullptr, cos_angle, offset, dist, max_variation, min_points,
                                               max_rounds, max_planes, (int32_t*)(io + o_lab), (double*)(io + o_pl), (double*)(io + o_cr),
                                               (int64_t*)(io + o_cnt), normals_out && !normals ? (double*)(io + o_nout) : nullptr, ctx->stream);
    return st.finish(F3D_DEVERR_PLANES);
}

// ---------------------------------------------------------------------------------------------
// smooth_votes / smooth_segment: neighbour-summed vote rows over an adjacency
// ---------------------------------------------------------------------------------------------
namespace {

struct smooth_in {                          // what the four entries share
    const void* votes; int vtype; int64_t n; int ncols; const int64_t* offsets; const int32_t* neighbours;
    const double* normals; double cos_angle; const void* colors; int cdtype; double max_color_dist; double self_weight; int iterations;
};
#define F3D_SMOOTH_BAD "smooth_votes: bad arguments (n < 2^31, 1 <= ncols <= 256, iterations >= 1, self_weight finite and >= 0, " \
                       "cos_angle not NaN with normals, max_color_dist >= 0 with colors)"

bool smooth_args_bad(const smooth_in& a, const void* out) {
    return (a.vtype != F3D_VOTES_F64 && a.vtype != F3D_VOTES_U16) || a.n < 0 || a.n > 0x7fffffffLL || a.ncols < 1 || a.ncols > 256 ||
           a.iterations < 1 || !(a.self_weight >= 0.0) || !isfinite(a.self_weight) || (a.normals && a.cos_angle != a.cos_angle) ||
           (a.colors && (!dtype_ok(a.cdtype) || !(a.max_color_dist >= 0.0))) || (a.n > 0 && (!a.votes || !a.offsets || !out));
}

size_t smooth_vote_bytes(const smooth_in& a) { return (size_t)a.n * a.ncols * (a.vtype == F3D_VOTES_U16 ? 2 : 8); }

bool ranges_overlap(const void* p, size_t pb, const void* q, size_t qb) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qb && b < a + pb;
}

// scratch matrices of a call: smooth_votes alternates between votes_out and one matrix; smooth_segment writes iterations - 1
// matrices, alternating between two
int smooth_matrices(int iterations, bool segment) { return segment ? (iterations > 2 ? 2 : iterations - 1) : (iterations > 1 ? 1 : 0); }

// the iterations of one call, enqueued on s.  seg NULL: the last one lands in out; else it produces classes
int smooth_enqueue(f3d_ctx* ctx, const smooth_in& a, double* out, const f3d_smooth_seg* seg, int64_t* classes, hipStream_t s) {
    const size_t mat = (size_t)a.n * a.ncols * 8;
    const int nmat = smooth_matrices(a.iterations, seg != nullptr);
    void* scratch = nullptr;
    int rc;
    if (nmat > 0 && (rc = ensure(ctx, SLOT_SMOOTH, mat * nmat, &scratch))) return rc;
    double* m[2] = {(double*)scratch, (double*)((char*)scratch + (nmat > 1 ? mat : 0))};
    const f3d_smooth_gates g = {a.normals, a.cos_angle, a.colors, a.cdtype, a.max_color_dist * a.max_color_dist};
    F3D_HIP(ctx, f3d_launch_smooth_check(a.n, a.offsets, a.neighbours, ctx->dev_err, s));
    const void* src = a.votes;
    int vtype = a.vtype;
    const int T = a.iterations;
    for (int t = 1; t <= T; ++t) {
        const bool last = t == T;
        double* dst = seg ? m[(t - 1) & 1] : (((T - t) & 1) ? m[0] : out);
        F3D_HIP(ctx, f3d_launch_smooth(src, vtype, a.n, a.ncols, a.offsets, a.neighbours, g, a.self_weight, last && seg ? nullptr : dst,
                                       last ? seg : nullptr, last ? classes : nullptr, ctx->dev_err, s));
        src = dst;
        vtype = F3D_VOTES_F64;
    }
    return F3D_OK;
}

// the epilogue's record: make_filter's list (device copy in flt.cls_dev) and, for lastcol, which entries were given negative
int smooth_seg_make(f3d_ctx* ctx, int ncols, int nclasses, double threshold, const int32_t* filter, int nfilter, int lastcol, hipStream_t s,
                    f3d_smooth_seg* sg) {
    *sg = f3d_smooth_seg{};
    sg->nclasses = nclasses; sg->threshold = threshold; sg->lastcol = lastcol ? 1 : 0;
    int rc;
    if ((rc = make_filter(ctx, filter, nfilter, ncols, true, s, &sg->flt))) return rc;
    if (lastcol) for (int k = 0; k < sg->flt.nfilter; ++k) if (filter[k] < 0) sg->neg.w[k >> 5] |= 1u << (k & 31);
    return F3D_OK;
}

// device copies of a host call's inputs (a NULL gate array stays NULL)
int smooth_stage(f3d_ctx* ctx, staging& st, const smooth_in& h, smooth_in* d) {
    const int64_t e = h.n > 0 ? h.offsets[h.n] : 0;
    if (e < 0 || (e > 0 && !h.neighbours)) return fail(ctx, F3D_ERR_INVALID, "smooth_votes: bad adjacency");
    *d = h;
    d->votes = st.in((const char*)h.votes, smooth_vote_bytes(h));
    d->offsets = st.in(h.offsets, (size_t)(h.n + 1) * 8);
    d->neighbours = st.in(h.neighbours, (size_t)e * 4);
    d->normals = h.normals ? st.in(h.normals, (size_t)h.n * 24) : nullptr;
    d->colors = h.colors ? st.in((const char*)h.colors, xyz_bytes((f3d_dtype)h.cdtype, h.n)) : nullptr;
    return st.rc;
}

}  // namespace

int f3d_ctx_reserve_smooth(f3d_ctx* ctx, int64_t n, int ncols, int iterations) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n > 0x7fffffffLL || ncols < 1 || ncols > 256 || iterations < 1)
        return fail(ctx, F3D_ERR_INVALID, "ctx_reserve_smooth: bad arguments (n < 2^31, 1 <= ncols <= 256, iterations >= 1)");
    const int nmat = smooth_matrices(iterations, true) > smooth_matrices(iterations, false) ? smooth_matrices(iterations, true)
                                                                                            : smooth_matrices(iterations, false);
    return reserve(ctx, {{SLOT_SMOOTH, (size_t)n * ncols * 8 * nmat, nmat > 0}});
}

int f3d_smooth_votes_dev(f3d_ctx* ctx, const void* votes, int vtype, int64_t n, int ncols, const int64_t* offsets,
                         const int32_t* neighbours, const double* normals, double cos_angle, const void* colors, f3d_dtype cdtype,
                         double max_color_dist, double self_weight, int iterations, double* votes_out, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    const smooth_in a = {votes, vtype, n, ncols, offsets, neighbours, normals, cos_angle, colors, cdtype, max_color_dist, self_weight, iterations};
    if (smooth_args_bad(a, votes_out)) return fail(ctx, F3D_ERR_INVALID, F3D_SMOOTH_BAD);
    if (n == 0) return F3D_OK;
    if (ranges_overlap(votes, smooth_vote_bytes(a), votes_out, (size_t)n * ncols * 8))
        return fail(ctx, F3D_ERR_INVALID, "smooth_votes: votes_out overlaps votes");
    return smooth_enqueue(ctx, a, votes_out, nullptr, nullptr, pick(ctx, stream));
}

int f3d_smooth_votes(f3d_ctx* ctx, const void* votes, int vtype, int64_t n, int ncols, const int64_t* offsets, const int32_t* neighbours,
                     const double* normals, double cos_angle, const void* colors, f3d_dtype cdtype, double max_color_dist,
                     double self_weight, int iterations, double* votes_out) {
    int rc = enter(ctx); if (rc) return rc;
    const smooth_in h = {votes, vtype, n, ncols, offsets, neighbours, normals, cos_angle, colors, cdtype, max_color_dist, self_weight, iterations};
    if (smooth_args_bad(h, votes_out)) return fail(ctx, F3D_ERR_INVALID, F3D_SMOOTH_BAD);
    if (n == 0) return F3D_OK;
    if (ranges_overlap(votes, smooth_vote_bytes(h), votes_out, (size_t)n * ncols * 8))
        return fail(ctx, F3D_ERR_INVALID, "smooth_votes: votes_out overlaps votes");
    staging st(ctx);
    smooth_in d;
    if ((rc = smooth_stage(ctx, st, h, &d))) return rc;
    double* dout = st.out(votes_out, (size_t)n * ncols * 8);
    if (!st.rc) st.rc = f3d_smooth_votes_dev(ctx, d.votes, vtype, n, ncols, d.offsets, d.neighbours, d.normals, cos_angle, d.colors, cdtype,
                                             max_color_dist, self_weight, iterations, dout, ctx->stream);
    return st.finish(F3D_DEVERR_SMOOTH);
}

int f3d_smooth_segment_dev(f3d_ctx* ctx, const void* votes, int vtype, int64_t n, int ncols, const int64_t* offsets,
                           const int32_t* neighbours, const double* normals, double cos_angle, const void* colors, f3d_dtype cdtype,
                           double max_color_dist, double self_weight, int iterations, int nclasses, double threshold,
                           const int32_t* filter, int nfilter, int lastcol, int64_t* classes, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    const smooth_in a = {votes, vtype, n, ncols, offsets, neighbours, normals, cos_angle, colors, cdtype, max_color_dist, self_weight, iterations};
    if (smooth_args_bad(a, classes)) return fail(ctx, F3D_ERR_INVALID, F3D_SMOOTH_BAD);
    if (lastcol && ncols < 2 && nfilter == 0 && n > 0)          // votes[:, :-1] has no column, as in f3d_segment_votes_lastcol
        return fail(ctx, F3D_ERR_INVALID, "smooth_segment: attempt to get argmax of an empty sequence");
    hipStream_t s = pick(ctx, stream);
    f3d_smooth_seg sg;
    if ((rc = smooth_seg_make(ctx, ncols, nclasses, threshold, filter, nfilter, lastcol, s, &sg))) return rc;
    if (n == 0) return F3D_OK;
    return smooth_enqueue(ctx, a, nullptr, &sg, classes, s);
}

int f3d_smooth_segment(f3d_ctx* ctx, const void* votes, int vtype, int64_t n, int ncols, const int64_t* offsets,
                       const int32_t* neighbours, const double* normals, double cos_angle, const void* colors, f3d_dtype cdtype,
                       double max_color_dist, double self_weight, int iterations, int nclasses, double threshold,
                       const int32_t* filter, int nfilter, int lastcol, int64_t* classes) {
    int rc = enter(ctx); if (rc) return rc;
    const smooth_in h = {votes, vtype, n, ncols, offsets, neighbours, normals, cos_angle, colors, cdtype, max_color_dist, self_weight, iterations};
    if (smooth_args_bad(h, classes)) return fail(ctx, F3D_ERR_INVALID, F3D_SMOOTH_BAD);
    if (n == 0) return F3D_OK;
    staging st(ctx);
    smooth_in d;
    if ((rc = smooth_stage(ctx, st, h, &d))) return rc;
    int64_t* dcls = st.out(classes, (size_t)n * 8);
    if (!st.rc) st.rc = f3d_smooth_segment_dev(ctx, d.votes, vtype, n, ncols, d.offsets, d.neighbours, d.normals, cos_angle, d.colors, cdtype,
                                               max_color_dist, self_weight, iterations, nclasses, threshold, filter, nfilter, lastcol, dcls,
                                               ctx->stream);
    return st.finish(F3D_DEVERR_SMOOTH);
}

// ---------------------------------------------------------------------------------------------
// lift_overlaps / lift_instances: 3D instances from per-frame 2D instance ids
// ---------------------------------------------------------------------------------------------
namespace {

#define F3D_LIFT_BAD "bad arguments (nframes, hw, npoints >= 1, 1 <= max_ids <= 65535, nframes * max_ids < 2^31, nframes * hw < 2^31)"

bool lift_shape_ok(int nframes, int64_t hw, int64_t npoints, int max_ids) {
    return nframes >= 1 && hw >= 1 && npoints >= 1 && npoints <= 0x7fffffffLL && max_ids >= 1 && max_ids <= 65535 &&
           (int64_t)nframes * max_ids <= 0x7fffffffLL && hw <= 0x7fffffffLL && (int64_t)nframes * hw <= 0x7fffffffLL;
}

uint64_t lift_pow2(uint64_t v) { uint64_t s = 1024; while (s < v) s <<= 1; return s; }
uint64_t lift_pair_bound(int64_t nseg) { return (uint64_t)nseg * (uint64_t)(nseg - 1) / 2; }
uint64_t lift_min64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// slots of the pair table of a first run (include/f3d.h)
uint64_t lift_first_slots(int64_t pixels, int64_t nseg) {
    const uint64_t guess = (uint64_t)pixels / 4 > 32768 ? (uint64_t)pixels / 4 : 32768;
    return lift_pow2(2 * lift_min64(lift_pair_bound(nseg), guess));
}

// incidence -> pair table, again with a larger one while it overflows -> stats as include/f3d.h states them
int lift_run(f3d_ctx* ctx, f3d_lift_job& j, int64_t* stats, hipStream_t s) {
    const int64_t pixels = (int64_t)j.nframes * j.hw, nseg = (int64_t)j.nframes * j.max_ids;
    const int64_t cap = j.instances ? 0 : j.cap;
    int rc;
    if ((rc = ensure(ctx, SLOT_LIFT, f3d_lift_scratch_bytes(pixels, j.npoints, nseg), &j.scratch))) return rc;
    uint64_t slots = lift_first_slots(pixels, nseg);
    while (f3d_lift_table_bytes(slots * 2, cap) <= ctx->scratch[SLOT_LIFT_TABLE].cap) slots *= 2;       // room that is there already is used
    j.err = ctx->dev_err; j.stream = s;
    F3D_HIP(ctx, f3d_launch_lift_incidence(j));
    int64_t st[F3D_LIFT_NSTATS];
    int64_t rounds = 1;
    for (;; ++rounds) {
        if ((rc = ensure(ctx, SLOT_LIFT_TABLE, f3d_lift_table_bytes(slots, cap), &j.table))) return rc;
        j.slots = slots;
        F3D_HIP(ctx, f3d_launch_lift_merge(j, st));
        if (st[6]) {
            if ((rc = take_error(ctx, s, F3D_DEVERR_LIFT))) return rc;
            return fail(ctx, F3D_ERR_INDEX, "%s", device_error_message(F3D_DEVERR_LIFT));
        }
        if (!st[5]) break;
        const uint64_t need = lift_pow2(2 * lift_min64((uint64_t)st[4], lift_pair_bound(nseg)));
        slots = need > slots * 2 ? need : slots * 2;
        if (slots > ((uint64_t)1 << 36)) return fail(ctx, F3D_ERR_NOMEM, "lift: the pair table would need %llu slots", (unsigned long long)slots);
    }
    stats[0] = st[0]; stats[1] = st[1]; stats[2] = st[2]; stats[3] = st[3]; stats[4] = st[4]; stats[5] = rounds;
    return F3D_OK;
}

f3d_lift_job lift_job(const int32_t* luts, const uint16_t* inst, int nframes, int64_t hw, int64_t npoints, int max_ids) {
    f3d_lift_job j = {};
    j.luts = luts; j.inst = inst; j.nframes = nframes; j.hw = hw; j.npoints = npoints; j.max_ids = max_ids;
    return j;
}

}  // namespace

int f3d_ctx_reserve_lift(f3d_ctx* ctx, int nframes, int64_t hw, int64_t npoints, int max_ids, int64_t max_pairs) {
    int rc = enter(ctx); if (rc) return rc;
    if (!lift_shape_ok(nframes, hw, npoints, max_ids) || max_pairs < 0 || max_pairs > 0x7fffffffLL)
        return fail(ctx, F3D_ERR_INVALID, "ctx_reserve_lift: " F3D_LIFT_BAD ", 0 <= max_pairs < 2^31");
    const int64_t pixels = (int64_t)nframes * hw, nseg = (int64_t)nframes * max_ids;
    const uint64_t first = lift_first_slots(pixels, nseg), room = lift_pow2(2 * (uint64_t)max_pairs);
    return reserve(ctx, {{SLOT_LIFT, f3d_lift_scratch_bytes(pixels, npoints, nseg)},
                         {SLOT_LIFT_TABLE, f3d_lift_table_bytes(first > room ? first : room, max_pairs)}});
}

int f3d_lift_overlaps_dev(f3d_ctx* ctx, const int32_t* luts, const uint16_t* inst, int nframes, int64_t hw, int64_t npoints, int max_ids,
                          int32_t* sizes, int32_t* pairs, int32_t* counts, int64_t cap, int64_t* stats, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!lift_shape_ok(nframes, hw, npoints, max_ids) || !luts || !inst || !sizes || !stats || cap < 0 || cap > 0x7fffffffLL ||
        (cap > 0 && (!pairs || !counts)))
        return fail(ctx, F3D_ERR_INVALID, "lift_overlaps: " F3D_LIFT_BAD ", 0 <= cap < 2^31");
    f3d_lift_job j = lift_job(luts, inst, nframes, hw, npoints, max_ids);
    j.sizes = sizes; j.pairs = pairs; j.counts = counts; j.cap = cap;
    return lift_run(ctx, j, stats, pick(ctx, stream));
}

int f3d_lift_overlaps(f3d_ctx* ctx, const int32_t* luts, const uint16_t* inst, int nframes, int64_t hw, int64_t npoints, int max_ids,
                      int32_t* sizes, int32_t* pairs, int32_t* counts, int64_t cap, int64_t* stats) {
    int rc = enter(ctx); if (rc) return rc;
    if (!lift_shape_ok(nframes, hw, npoints, max_ids) || !luts || !inst || !sizes || !stats || cap < 0 || cap > 0x7fffffffLL ||
        (cap > 0 && (!pairs || !counts)))
        return fail(ctx, F3D_ERR_INVALID, "lift_overlaps: " F3D_LIFT_BAD ", 0 <= cap < 2^31");
    const size_t pixels = (size_t)nframes * hw, nseg = (size_t)nframes * max_ids;
    f3d_carve c;
    const size_t o_luts = c.take(pixels * 4), o_inst = c.take(pixels * 2), o_sizes = c.take(nseg * 4), o_pairs = c.take((size_t)cap * 8),
                 o_counts = c.take((size_t)cap * 4);
    staging st(ctx);
    char* io = (char*)st.slot(c.off);
    if (st.rc) return st.rc;
    st.put(io + o_luts, luts, pixels * 4);
    st.put(io + o_inst, inst, pixels * 2);
    st.put(io + o_pairs, pairs, (size_t)cap * 8);             // what comes back when P > cap: the caller's own entries
    st.put(io + o_counts, counts, (size_t)cap * 4);
    st.back(sizes, io + o_sizes, nseg * 4);
    st.back(pairs, io + o_pairs, (size_t)cap * 8);
    st.back(counts, io + o_counts, (size_t)cap * 4);
    if (!st.rc) st.rc = f3d_lift_overlaps_dev(ctx, (const int32_t*)(io + o_luts), (const uint16_t*)(io + o_inst), nframes, hw, npoints, max_ids,
                                              (int32_t*)(io + o_sizes), (int32_t*)(io + o_pairs), (int32_t*)(io + o_counts), cap, stats, ctx->stream);
    return st.finish();
}

int f3d_lift_instances_dev(f3d_ctx* ctx, const int32_t* luts, const uint16_t* inst, int nframes, int64_t hw, int64_t npoints, int max_ids,
                           double ratio, int64_t min_overlap, const int32_t* seg_classes, int64_t min_points, int32_t* ids,
                           uint16_t* support, uint16_t* seen, int32_t* seg2inst, int64_t* inst_points, int64_t* stats, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!lift_shape_ok(nframes, hw, npoints, max_ids) || !luts || !inst || !ids || !support || !seen || !seg2inst || !inst_points || !stats)
        return fail(ctx, F3D_ERR_INVALID, "lift_instances: " F3D_LIFT_BAD);
    f3d_lift_job j = lift_job(luts, inst, nframes, hw, npoints, max_ids);
    j.instances = true; j.ratio = ratio; j.min_overlap = min_overlap; j.min_points = min_points; j.seg_classes = seg_classes;
    j.ids = ids; j.support = support; j.seen = seen; j.seg2inst = seg2inst; j.inst_points = inst_points;
    return lift_run(ctx, j, stats, pick(ctx, stream));
}

int f3d_lift_instances(f3d_ctx* ctx, const int32_t* luts, const uint16_t* inst, int nframes, int64_t hw, int64_t npoints, int max_ids,
                       double ratio, int64_t min_overlap, const int32_t* seg_classes, int64_t min_points, int32_t* ids, uint16_t* support,
                       uint16_t* seen, int32_t* seg2inst, int64_t* inst_points, int64_t* stats) {
    int rc = enter(ctx); if (rc) return rc;
    if (!lift_shape_ok(nframes, hw, npoints, max_ids) || !luts || !inst || !ids || !support || !seen || !seg2inst || !inst_points || !stats)
        return fail(ctx, F3D_ERR_INVALID, "lift_instances: " F3D_LIFT_BAD);
    const size_t pixels = (size_t)nframes * hw, nseg = (size_t)nframes * max_ids, np = (size_t)npoints;
    f3d_carve c;
    const size_t o_luts = c.take(pixels * 4), o_inst = c.take(pixels * 2), o_cls = c.take(seg_classes ? nseg * 4 : 0), o_ids = c.take(np * 4),
                 o_sup = c.take(np * 2), o_seen = c.take(np * 2), o_s2i = c.take(nseg * 4), o_ip = c.take((nseg + 1) * 8);
    staging st(ctx);
    char* io = (char*)st.slot(c.off);
    if (st.rc) return st.rc;
    st.put(io + o_luts, luts, pixels * 4);
    st.put(io + o_inst, inst, pixels * 2);
    if (seg_classes) st.put(io + o_cls, seg_classes, nseg * 4);
    st.put(io + o_ip, inst_points, (nseg + 1) * 8);           // the entries past I' come back as they were
    st.back(ids, io + o_ids, np * 4);
    st.back(support, io + o_sup, np * 2);
    st.back(seen, io + o_seen, np * 2);
    st.back(seg2inst, io + o_s2i, nseg * 4);
    st.back(inst_points, io + o_ip, (nseg + 1) * 8);
    if (!st.rc) st.rc = f3d_lift_instances_dev(ctx, (const int32_t*)(io + o_luts), (const uint16_t*)(io + o_inst), nframes, hw, npoints, max_ids, ratio,
                                               min_overlap, seg_classes ? (const int32_t*)(io + o_cls) : nullptr, min_points, (int32_t*)(io + o_ids),
                                               (uint16_t*)(io + o_sup), (uint16_t*)(io + o_seen), (int32_t*)(io + o_s2i), (int64_t*)(io + o_ip),
                                               stats, ctx->stream);
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// segUtils/meshUtils.py: face filtering, vertex maps, triangle clusters
// ---------------------------------------------------------------------------------------------
static bool mesh_args_ok(int64_t nv, int64_t nt, int itype, int vdtype) {
    return nv >= 0 && nv <= 0x7fffffffLL && nt >= 0 && 3 * nt <= 0x7fffffffLL && (itype == F3D_I64 || itype == F3D_I32) &&
           dtype_ok(vdtype);
}
#define F3D_MESH_BAD "bad arguments (nv < 2^31, 3 * nt < 2^31, int64 / int32 triangles, float64 / float32 vertices)"

static size_t tri_bytes(int itype, int64_t nt) { return (size_t)nt * 3 * (itype == F3D_I64 ? 8 : 4); }

int f3d_ctx_reserve_mesh(f3d_ctx* ctx, int64_t nv, int64_t nt) {
    int rc = enter(ctx); if (rc) return rc;
    if (!mesh_args_ok(nv, nt, F3D_I64, F3D_F64)) return fail(ctx, F3D_ERR_INVALID, "ctx_reserve_mesh: " F3D_MESH_BAD);
    return reserve(ctx, {{SLOT_MESH, f3d_mesh_scratch_bytes(nv, nt)}, {SLOT_FACE_GRAPH, f3d_face_graph_scratch_bytes(nt)}});
}

static bool mesh_vertex_map_bad(int64_t nv, int64_t nt, int itype, const void* tris, const void* offsets, const void* tri, const void* pos, const void* counts) {
    return !mesh_args_ok(nv, nt, itype, F3D_F64) || !offsets || !counts || (nt > 0 && (!tris || !tri || !pos));
}

int f3d_mesh_vertex_map_dev(f3d_ctx* ctx, const void* tris, int itype, int64_t nt, int64_t nv, int64_t* offsets, int32_t* tri,
                            int8_t* pos, int64_t* counts, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (mesh_vertex_map_bad(nv, nt, itype, tris, offsets, tri, pos, counts))
        return fail(ctx, F3D_ERR_INVALID, "mesh_vertex_map: " F3D_MESH_BAD);
    void* scratch;
    if ((rc = ensure(ctx, SLOT_MESH, f3d_mesh_scratch_bytes(nv, nt), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_mesh_vertex_map(tris, itype, nt, nv, offsets, tri, pos, scratch, counts, ctx->dev_err, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_mesh_vertex_map(f3d_ctx* ctx, const void* tris, int itype, int64_t nt, int64_t nv, int64_t* offsets, int32_t* tri,
                        int8_t* pos, int64_t* counts) {
    int rc = enter(ctx); if (rc) return rc;
    if (mesh_vertex_map_bad(nv, nt, itype, tris, offsets, tri, pos, counts))
        return fail(ctx, F3D_ERR_INVALID, "mesh_vertex_map: " F3D_MESH_BAD);
    f3d_carve c;
    const size_t o_tris = c.take(tri_bytes(itype, nt)), o_offs = c.take((size_t)(nv + 1) * 8), o_tri = c.take((size_t)nt * 12),
                 o_pos = c.take((size_t)nt * 3), o_cnt = c.take(32);
    staging st(ctx);
    char* io = (char*)st.slot(c.off);
    if (st.rc) return st.rc;
    st.put(io + o_tris, tris, tri_bytes(itype, nt));
    st.back(offsets, io + o_offs, (size_t)(nv + 1) * 8);
    st.back(tri, io + o_tri, (size_t)nt * 12);
    st.back(pos, io + o_pos, (size_t)nt * 3);
    st.back(counts, io + o_cnt, 32);
    if (!st.rc) st.rc = f3d_mesh_vertex_map_dev(ctx, io + o_tris, itype, nt, nv, (int64_t*)(io + o_offs), (int32_t*)(io + o_tri),
                                                (int8_t*)(io + o_pos), (int64_t*)(io + o_cnt), ctx->stream);
    return st.finish(F3D_DEVERR_MESH);
}

static bool mesh_remove_faces_bad(int64_t nv, int64_t nt, int itype, const void* tris, const void* mask, const void* not_removed, const void* remaining, const void* old2new,
                                  const void* counts) {
    return !mesh_args_ok(nv, nt, itype, F3D_F64) || !counts || (nv > 0 && (!mask || !old2new)) || (nt > 0 && (!tris || !not_removed || !remaining));
}

int f3d_mesh_remove_faces_dev(f3d_ctx* ctx, const void* tris, int itype, int64_t nt, int64_t nv, const uint8_t* mask,
                              uint8_t* not_removed, void* remaining, int64_t* old2new, int64_t* counts, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (mesh_remove_faces_bad(nv, nt, itype, tris, mask, not_removed, remaining, old2new, counts))
        return fail(ctx, F3D_ERR_INVALID, "mesh_remove_faces: " F3D_MESH_BAD);
    void* scratch;
    if ((rc = ensure(ctx, SLOT_MESH, f3d_mesh_scratch_bytes(nv, nt), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_mesh_remove_faces(tris, itype, nt, nv, mask, not_removed, remaining, old2new, scratch, counts, ctx->dev_err,
                                              pick(ctx, stream)));
    return F3D_OK;
}

int f3d_mesh_remove_faces(f3d_ctx* ctx, const void* tris, int itype, int64_t nt, int64_t nv, const uint8_t* mask,
                          uint8_t* not_removed, void* remaining, int64_t* old2new, int64_t* counts) {
    int rc = enter(ctx); if (rc) return rc;
    if (mesh_remove_faces_bad(nv, nt, itype, tris, mask, not_removed, remaining, old2new, counts))
        return fail(ctx, F3D_ERR_INVALID, "mesh_remove_faces: " F3D_MESH_BAD);
    f3d_carve c;
    const size_t tb = tri_bytes(itype, nt);
    const size_t o_tris = c.take(tb), o_mask = c.take((size_t)nv), o_nr = c.take((size_t)nt), o_rem = c.take(tb), o_o2n = c.take((size_t)nv * 8),
                 o_cnt = c.take(32);
    staging st(ctx);
    char* io = (char*)st.slot(c.off);
    if (st.rc) return st.rc;
    st.put(io + o_tris, tris, tb);
    st.put(io + o_mask, mask, (size_t)nv);
    st.back(not_removed, io + o_nr, (size_t)nt);
    st.back(remaining, io + o_rem, tb);
    st.back(old2new, io + o_o2n, (size_t)nv * 8);
    st.back(counts, io + o_cnt, 32);
    if (!st.rc) st.rc = f3d_mesh_remove_faces_dev(ctx, io + o_tris, itype, nt, nv, (const uint8_t*)(io + o_mask), (uint8_t*)(io + o_nr), io + o_rem,
                                                  (int64_t*)(io + o_o2n), (int64_t*)(io + o_cnt), ctx->stream);
    return st.finish(F3D_DEVERR_MESH);
}

static bool mesh_keep_faces_bad(int64_t nv, int64_t nt, int itype, int vdtype, const void* verts, const void* tris, const void* mask, const void* out_verts,
                                const void* out_tris, const void* counts) {
    return !mesh_args_ok(nv, nt, itype, vdtype) || !counts || (nv > 0 && (!verts || !mask)) || (nt > 0 && (!tris || !out_tris)) ||
           (nt > 0 && nv > 0 && !out_verts);
}

int f3d_mesh_keep_faces_dev(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                            const uint8_t* mask, void* out_verts, void* out_tris, int64_t* counts, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (mesh_keep_faces_bad(nv, nt, itype, vdtype, verts, tris, mask, out_verts, out_tris, counts))
        return fail(ctx, F3D_ERR_INVALID, "mesh_keep_faces: " F3D_MESH_BAD);
    void* scratch;
    if ((rc = ensure(ctx, SLOT_MESH, f3d_mesh_scratch_bytes(nv, nt), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_mesh_keep_faces(verts, vdtype, nv, tris, itype, nt, mask, out_verts, out_tris, scratch, counts, ctx->dev_err,
                                            pick(ctx, stream)));
    return F3D_OK;
}

int f3d_mesh_keep_faces(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                        const uint8_t* mask, void* out_verts, void* out_tris, int64_t* counts) {
    int rc = enter(ctx); if (rc) return rc;
    if (mesh_keep_faces_bad(nv, nt, itype, vdtype, verts, tris, mask, out_verts, out_tris, counts))
        return fail(ctx, F3D_ERR_INVALID, "mesh_keep_faces: " F3D_MESH_BAD);
    f3d_carve c;
    const size_t tb = tri_bytes(itype, nt), vb = xyz_bytes((f3d_dtype)vdtype, nv), ob = xyz_bytes((f3d_dtype)vdtype, 3 * nt < nv ? 3 * nt : nv);
    const size_t o_verts = c.take(vb), o_tris = c.take(tb), o_mask = c.take((size_t)nv), o_ov = c.take(ob), o_ot = c.take(tb), o_cnt = c.take(32);
    staging st(ctx);
    char* io = (char*)st.slot(c.off);
    if (st.rc) return st.rc;
    st.put(io + o_verts, verts, vb);
    st.put(io + o_tris, tris, tb);
    st.put(io + o_mask, mask, (size_t)nv);
    st.back(out_verts, io + o_ov, ob);
    st.back(out_tris, io + o_ot, tb);
    st.back(counts, io + o_cnt, 32);
    if (!st.rc) st.rc = f3d_mesh_keep_faces_dev(ctx, io + o_verts, vdtype, nv, io + o_tris, itype, nt, (const uint8_t*)(io + o_mask), io + o_ov,
                                                io + o_ot, (int64_t*)(io + o_cnt), ctx->stream);
    return st.finish(F3D_DEVERR_MESH);
}

static bool mesh_triangle_clusters_bad(int64_t nv, int64_t nt, int itype, int vdtype, const void* verts, const void* tris, const void* clusters, const void* cluster_n,
                                       const void* cluster_area, const void* counts) {
    return !mesh_args_ok(nv, nt, itype, vdtype) || !counts || (nv > 0 && !verts) || (nt > 0 && (!tris || !clusters || !cluster_n || !cluster_area));
}

int f3d_mesh_triangle_clusters_dev(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype,
                                   int64_t nt, int32_t* clusters, int64_t* cluster_n, double* cluster_area, double* tri_area,
                                   int64_t* counts, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (mesh_triangle_clusters_bad(nv, nt, itype, vdtype, verts, tris, clusters, cluster_n, cluster_area, counts))
        return fail(ctx, F3D_ERR_INVALID, "mesh_triangle_clusters: " F3D_MESH_BAD);
    void* scratch;
    if ((rc = ensure(ctx, SLOT_MESH, f3d_mesh_scratch_bytes(nv, nt), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_mesh_clusters(verts, vdtype, nv, tris, itype, nt, clusters, cluster_n, cluster_area, tri_area, scratch, counts,
                                          ctx->dev_err, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_mesh_triangle_clusters(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                               int32_t* clusters, int64_t* cluster_n, double* cluster_area, double* tri_area, int64_t* counts) {
    int rc = enter(ctx); if (rc) return rc;
    if (mesh_triangle_clusters_bad(nv, nt, itype, vdtype, verts, tris, clusters, cluster_n, cluster_area, counts))
        return fail(ctx, F3D_ERR_INVALID, "mesh_triangle_clusters: " F3D_MESH_BAD);
    f3d_carve c;
    const size_t tb = tri_bytes(itype, nt), vb = xyz_bytes((f3d_dtype)vdtype, nv);
    const size_t o_verts = c.take(vb), o_tris = c.take(tb), o_cl = c.take((size_t)nt * 4), o_n = c.take((size_t)nt * 8), o_a = c.take((size_t)nt * 8),
                 o_ta = c.take((size_t)nt * 8), o_cnt = c.take(32);
    staging st(ctx);
    char* io = (char*)st.slot(c.off);
    if (st.rc) return st.rc;
    st.put(io + o_verts, verts, vb);
    st.put(io + o_tris, tris, tb);
    st.back(clusters, io + o_cl, (size_t)nt * 4);
    st.back(cluster_n, io + o_n, (size_t)nt * 8);
    st.back(cluster_area, io + o_a, (size_t)nt * 8);
    st.back(tri_area, io + o_ta, (size_t)nt * 8);
    st.back(counts, io + o_cnt, 32);
    if (!st.rc) st.rc = f3d_mesh_triangle_clusters_dev(ctx, io + o_verts, vdtype, nv, io + o_tris, itype, nt, (int32_t*)(io + o_cl),
                                                       (int64_t*)(io + o_n), (double*)(io + o_a), tri_area ? (double*)(io + o_ta) : nullptr,
                                                       (int64_t*)(io + o_cnt), ctx->stream);
    return st.finish(F3D_DEVERR_MESH);
}

static bool mesh_clean_bad(int64_t nv, int64_t nt, int itype, int vdtype, const void* verts, const void* tris, const void* new_verts, const void* new_tris,
                           const void* kept_v, const void* kept_t, const void* counts) {
    return !mesh_args_ok(nv, nt, itype, vdtype) || !counts || (nv > 0 && (!verts || !new_verts || !kept_v)) || (nt > 0 && (!tris || !new_tris || !kept_t));
}

int f3d_mesh_clean_dev(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                       const uint8_t* remove_mask, int64_t min_triangles, double min_area, void* new_verts, void* new_tris,
                       uint8_t* kept_v, uint8_t* kept_t, int64_t* counts, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (mesh_clean_bad(nv, nt, itype, vdtype, verts, tris, new_verts, new_tris, kept_v, kept_t, counts))
        return fail(ctx, F3D_ERR_INVALID, "mesh_clean: " F3D_MESH_BAD);
    void* scratch;
    if ((rc = ensure(ctx, SLOT_MESH, f3d_mesh_scratch_bytes(nv, nt), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_mesh_clean(verts, vdtype, nv, tris, itype, nt, remove_mask, min_triangles, min_area, new_verts, new_tris, kept_v,
                                       kept_t, scratch, counts, ctx->dev_err, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_mesh_clean(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                   const uint8_t* remove_mask, int64_t min_triangles, double min_area, void* new_verts, void* new_tris,
                   uint8_t* kept_v, uint8_t* kept_t, int64_t* counts) {
    int rc = enter(ctx); if (rc) return rc;
    if (mesh_clean_bad(nv, nt, itype, vdtype, verts, tris, new_verts, new_tris, kept_v, kept_t, counts))
        return fail(ctx, F3D_ERR_INVALID, "mesh_clean: " F3D_MESH_BAD);
    f3d_carve c;
    const size_t tb = tri_bytes(itype, nt), vb = xyz_bytes((f3d_dtype)vdtype, nv);
    const size_t o_verts = c.take(vb), o_tris = c.take(tb), o_mask = c.take((size_t)nv), o_nv = c.take(vb), o_nt = c.take(tb),
                 o_kv = c.take((size_t)nv), o_kt = c.take((size_t)nt), o_cnt = c.take(32);
    staging st(ctx);
    char* io = (char*)st.slot(c.off);
    if (st.rc) return st.rc;
    st.put(io + o_verts, verts, vb);
    st.put(io + o_tris, tris, tb);
    st.put(io + o_mask, remove_mask, (size_t)nv);
    st.back(new_verts, io + o_nv, vb);
    st.back(new_tris, io + o_nt, tb);
    st.back(kept_v, io + o_kv, (size_t)nv);
    st.back(kept_t, io + o_kt, (size_t)nt);
    st.back(counts, io + o_cnt, 32);
    if (!st.rc) st.rc = f3d_mesh_clean_dev(ctx, io + o_verts, vdtype, nv, io + o_tris, itype, nt, remove_mask ? (const uint8_t*)(io + o_mask) : nullptr,
                                           min_triangles, min_area, io + o_nv, io + o_nt, (uint8_t*)(io + o_kv), (uint8_t*)(io + o_kt),
                                           (int64_t*)(io + o_cnt), ctx->stream);
    return st.finish(F3D_DEVERR_MESH);
}

static bool mesh_face_frames_bad(int64_t nv, int64_t nt, int itype, int vdtype, const void* verts, const void* tris, const void* normals, const void* counts) {
    return !mesh_args_ok(nv, nt, itype, vdtype) || !counts || (nv > 0 && !verts) || (nt > 0 && (!tris || !normals));
}

int f3d_mesh_face_frames_dev(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                             double* normals, double* centroids, double* areas, int64_t* counts, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (mesh_face_frames_bad(nv, nt, itype, vdtype, verts, tris, normals, counts))
        return fail(ctx, F3D_ERR_INVALID, "mesh_face_frames: " F3D_MESH_BAD);
    F3D_HIP(ctx, f3d_launch_mesh_face_frames(verts, vdtype, nv, tris, itype, nt, normals, centroids, areas, counts, ctx->dev_err,
                                             pick(ctx, stream)));
    return F3D_OK;
}

int f3d_mesh_face_frames(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                         double* normals, double* centroids, double* areas, int64_t* counts) {
    int rc = enter(ctx); if (rc) return rc;
    if (mesh_face_frames_bad(nv, nt, itype, vdtype, verts, tris, normals, counts))
        return fail(ctx, F3D_ERR_INVALID, "mesh_face_frames: " F3D_MESH_BAD);
    f3d_carve c;
    const size_t tb = tri_bytes(itype, nt), vb = xyz_bytes((f3d_dtype)vdtype, nv);
    const size_t o_verts = c.take(vb), o_tris = c.take(tb), o_n = c.take((size_t)nt * 24), o_c = c.take((size_t)nt * 24), o_a = c.take((size_t)nt * 8),
                 o_cnt = c.take(32);
    staging st(ctx);
    char* io = (char*)st.slot(c.off);
    if (st.rc) return st.rc;
    st.put(io + o_verts, verts, vb);
    st.put(io + o_tris, tris, tb);
    st.back(normals, io + o_n, (size_t)nt * 24);
    st.back(centroids, io + o_c, (size_t)nt * 24);
    st.back(areas, io + o_a, (size_t)nt * 8);
    st.back(counts, io + o_cnt, 32);
    if (!st.rc) st.rc = f3d_mesh_face_frames_dev(ctx, io + o_verts, vdtype, nv, io + o_tris, itype, nt, (double*)(io + o_n),
                                                 centroids ? (double*)(io + o_c) : nullptr, areas ? (double*)(io + o_a) : nullptr,
                                                 (int64_t*)(io + o_cnt), ctx->stream);
    return st.finish(F3D_DEVERR_MESH);
}

static bool mesh_face_graph_bad(int64_t nv, int64_t nt, int itype, int vdtype, const void* verts, const void* tris, int gate, const void* offsets,
                                const void* neighbours, int64_t cap, const void* counts) {
    return !mesh_args_ok(nv, nt, itype, vdtype) || !counts || !offsets || cap < 0 || (cap > 0 && !neighbours) || (nt > 0 && !tris) ||
           (gate && nv > 0 && !verts);
}
#define F3D_FACE_GRAPH_BAD F3D_MESH_BAD ", cap >= 0, vertices with a gate"

int f3d_mesh_face_graph_dev(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt, int gate,
                            double cos_crease, int64_t* offsets, int32_t* neighbours, int64_t cap, int64_t* counts, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (mesh_face_graph_bad(nv, nt, itype, vdtype, verts, tris, gate, offsets, neighbours, cap, counts))
        return fail(ctx, F3D_ERR_INVALID, "mesh_face_graph: " F3D_FACE_GRAPH_BAD);
    void* scratch;
    if ((rc = ensure(ctx, SLOT_FACE_GRAPH, f3d_face_graph_scratch_bytes(nt), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_mesh_face_graph(verts, vdtype, nv, tris, itype, nt, gate, cos_crease, offsets, cap > 0 ? neighbours : nullptr, cap,
                                            scratch, counts, ctx->dev_err, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_mesh_face_graph(f3d_ctx* ctx, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt, int gate,
                        double cos_crease, int64_t* offsets, int32_t* neighbours, int64_t cap, int64_t* counts) {
    int rc = enter(ctx); if (rc) return rc;
    if (mesh_face_graph_bad(nv, nt, itype, vdtype, verts, tris, gate, offsets, neighbours, cap, counts))
        return fail(ctx, F3D_ERR_INVALID, "mesh_face_graph: " F3D_FACE_GRAPH_BAD);
    f3d_carve c;
    const size_t tb = tri_bytes(itype, nt), vb = gate ? xyz_bytes((f3d_dtype)vdtype, nv) : 0;
    const size_t o_verts = c.take(vb), o_tris = c.take(tb), o_offs = c.take((size_t)(nt + 1) * 8), o_nb = c.take((size_t)cap * 4), o_cnt = c.take(32);
    staging st(ctx);
    char* io = (char*)st.slot(c.off);
    if (st.rc) return st.rc;
    st.put(io + o_verts, verts, vb);
    st.put(io + o_tris, tris, tb);
    st.put(io + o_nb, neighbours, (size_t)cap * 4);           // what comes back when nnz > cap: the caller's own entries
    st.back(offsets, io + o_offs, (size_t)(nt + 1) * 8);
    st.back(neighbours, io + o_nb, (size_t)cap * 4);
    st.back(counts, io + o_cnt, 32);
    if (!st.rc) st.rc = f3d_mesh_face_graph_dev(ctx, gate ? io + o_verts : nullptr, vdtype, nv, io + o_tris, itype, nt, gate, cos_crease,
                                                (int64_t*)(io + o_offs), (int32_t*)(io + o_nb), cap, (int64_t*)(io + o_cnt), ctx->stream);
    return st.finish(F3D_DEVERR_MESH);
}

// ---------------------------------------------------------------------------------------------
// a5 patch matching of Fusion.fuse
// ---------------------------------------------------------------------------------------------
int f3d_patch_owner_dev(f3d_ctx* ctx, const int32_t* uv, int64_t m, int h, int w, int half, double radius, double min_cosine,
                        const double* seed_pts, const double* seed_nrm, const double* q_pts, const double* q_nrm,
                        const uint8_t* free_px, int32_t* owner, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    const int64_t npx = (int64_t)h * w;
    if (h < 0 || w < 0 || m < 0 || half < 0 || npx > 0x7fffffffLL || m > 0x7fffffffLL || (m > 0 && (!uv || !seed_pts || !seed_nrm)) ||
        (npx > 0 && (!q_pts || !q_nrm || !free_px || !owner)))
        return fail(ctx, F3D_ERR_INVALID, "patch_owner: bad arguments");
    if (npx == 0) return F3D_OK;
    void* scratch;
    if ((rc = ensure(ctx, SLOT_PATCH, f3d_patch_scratch_bytes(h, w, m), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_patch_owner(uv, m, h, w, half, radius, min_cosine, seed_pts, seed_nrm, q_pts, q_nrm, free_px, owner, scratch,
                                        pick(ctx, stream)));
    return F3D_OK;
}

int f3d_patch_owner(f3d_ctx* ctx, const int32_t* uv, int64_t m, int h, int w, int half, double radius, double min_cosine,
                    const double* seed_pts, const double* seed_nrm, const double* q_pts, const double* q_nrm,
                    const uint8_t* free_px, int32_t* owner) {
    int rc = enter(ctx); if (rc) return rc;
    const int64_t npx = (int64_t)h * w;
    if (h < 0 || w < 0 || m < 0 || (m > 0 && (!uv || !seed_pts || !seed_nrm)) || (npx > 0 && (!q_pts || !q_nrm || !free_px || !owner)))
        return fail(ctx, F3D_ERR_INVALID, "patch_owner: bad arguments");
    if (npx == 0) return F3D_OK;
    staging st(ctx);
    const int32_t* duv = st.in(uv, (size_t)m * 8);
    const double* dsp = st.in(seed_pts, (size_t)m * 24);
    const double* dsn = st.in(seed_nrm, (size_t)m * 24);
    const double* dqp = st.in(q_pts, (size_t)npx * 24);
    const double* dqn = st.in(q_nrm, (size_t)npx * 24);
    const uint8_t* dfree = st.in(free_px, (size_t)npx);
    int32_t* down = st.out(owner, (size_t)npx * 4);
    if (!st.rc) st.rc = f3d_patch_owner_dev(ctx, duv, m, h, w, half, radius, min_cosine, dsp, dsn, dqp, dqn, dfree, down, ctx->stream);
    return st.finish();
}

// The matching of one frame of Fusion.fuse with the ordered sums of what every seed takes: the frame is uploaded once, the owner and
// the sums kernels run back to back on the resident arrays (colours optional).
int f3d_patch_match(f3d_ctx* ctx, const int32_t* uv, int64_t m, int h, int w, int half, double radius, double min_cosine,
                    const double* seed_pts, const double* seed_nrm, const double* q_pts, const double* q_nrm, const double* q_clr,
                    const uint8_t* free_px, int32_t* owner, double* sums, int32_t* counts) {
    int rc = enter(ctx); if (rc) return rc;
    const int64_t npx = (int64_t)h * w;
    if (h < 0 || w < 0 || m < 0 || half < 0 || npx > 0x7fffffffLL || m > 0x7fffffffLL || (m > 0 && (!uv || !seed_pts || !seed_nrm || !sums || !counts)) ||
        (npx > 0 && (!q_pts || !q_nrm || !free_px || !owner)))
        return fail(ctx, F3D_ERR_INVALID, "patch_match: bad arguments");
    if (npx == 0) return F3D_OK;
    staging st(ctx);
    const int32_t* duv = st.in(uv, (size_t)m * 8);
    const double* dsp = st.in(seed_pts, (size_t)m * 24);
    const double* dsn = st.in(seed_nrm, (size_t)m * 24);
    const double* dqp = st.in(q_pts, (size_t)npx * 24);
    const double* dqn = st.in(q_nrm, (size_t)npx * 24);
    const double* dqc = st.in(q_clr, (size_t)npx * 24);
    const uint8_t* dfree = st.in(free_px, (size_t)npx);
    int32_t* down = st.out(owner, (size_t)npx * 4);
    char* dsums = (char*)st.slot((size_t)m * 76 + 16);              // sums [m, 9], then the counts (16-byte aligned)
    if (st.rc) return st.rc;
    int32_t* dcnt = (int32_t*)(dsums + (((size_t)m * 72 + 15) & ~(size_t)15));
    st.back(sums, dsums, (size_t)m * 72);
    st.back(counts, dcnt, (size_t)m * 4);
    st.rc = f3d_patch_match_dev(ctx, duv, m, h, w, half, radius, min_cosine, dsp, dsn, dqp, dqn, q_clr ? dqc : nullptr, dfree, down,
                                (double*)dsums, dcnt, ctx->stream);
    return st.finish();
}

// patch_downsample with the ordered sums of every seed's members (sums [h*w, 9], counts [h*w]; only the self-owning pixels carry values)
int f3d_patch_seeds_sums(f3d_ctx* ctx, const double* pts, const double* nrm, const double* clr, const int32_t* prio, const uint8_t* free_px,
                         int h, int w, int half, double radius, double min_cosine, int32_t* owner, double* sums, int32_t* counts,
                         int32_t* rounds) {
    int rc = enter(ctx); if (rc) return rc;
    const int64_t npx = (int64_t)h * w;
    if (h < 0 || w < 0 || half < 0 || npx > 0x7fffffffLL || (npx > 0 && (!pts || !nrm || !prio || !free_px || !owner || !sums || !counts)))
        return fail(ctx, F3D_ERR_INVALID, "patch_seeds_sums: bad arguments");
    if (rounds) *rounds = 0;
    if (npx == 0) return F3D_OK;
    staging st(ctx);
    const double* dp = st.in(pts, (size_t)npx * 24);
    const double* dn = st.in(nrm, (size_t)npx * 24);
    const double* dc = st.in(clr, (size_t)npx * 24);
    const int32_t* dprio = st.in(prio, (size_t)npx * 4);
    const uint8_t* dfree = st.in(free_px, (size_t)npx);
    int32_t* down = st.out(owner, (size_t)npx * 4);
    char* dsums = (char*)st.slot((size_t)npx * 76 + 16);            // sums [h*w, 9], then the counts (16-byte aligned)
    if (st.rc) return st.rc;
    int32_t* dcnt = (int32_t*)(dsums + (((size_t)npx * 72 + 15) & ~(size_t)15));
    st.back(sums, dsums, (size_t)npx * 72);
    st.back(counts, dcnt, (size_t)npx * 4);
    st.rc = f3d_patch_seeds_sums_dev(ctx, dp, dn, clr ? dc : nullptr, dprio, dfree, h, w, half, radius, min_cosine, down, (double*)dsums, dcnt,
                                     rounds, ctx->stream);
    return st.finish();
}

int f3d_patch_match_dev(f3d_ctx* ctx, const int32_t* uv, int64_t m, int h, int w, int half, double radius, double min_cosine,
                        const double* seed_pts, const double* seed_nrm, const double* q_pts, const double* q_nrm, const double* q_clr,
                        const uint8_t* free_px, int32_t* owner, double* sums, int32_t* counts, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    const int64_t npx = (int64_t)h * w;
    if (h < 0 || w < 0 || m < 0 || half < 0 || npx > 0x7fffffffLL || m > 0x7fffffffLL || (m > 0 && (!uv || !seed_pts || !seed_nrm || !sums || !counts)) ||
        (npx > 0 && (!q_pts || !q_nrm || !free_px || !owner)))
        return fail(ctx, F3D_ERR_INVALID, "patch_match: bad arguments");
    if (npx == 0) return F3D_OK;
    void* scratch;
    if ((rc = ensure(ctx, SLOT_PATCH, f3d_patch_scratch_bytes(h, w, m), &scratch))) return rc;
    hipStream_t s = pick(ctx, stream);
    F3D_HIP(ctx, f3d_launch_patch_owner(uv, m, h, w, half, radius, min_cosine, seed_pts, seed_nrm, q_pts, q_nrm, free_px, owner, scratch, s));
    F3D_HIP(ctx, f3d_launch_patch_sums(owner, uv, m, h, w, half, q_pts, q_nrm, q_clr, sums, counts, s));
    return F3D_OK;
}

int f3d_patch_seeds_sums_dev(f3d_ctx* ctx, const double* pts, const double* nrm, const double* clr, const int32_t* prio, const uint8_t* free_px,
                             int h, int w, int half, double radius, double min_cosine, int32_t* owner, double* sums, int32_t* counts,
                             int32_t* rounds, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    const int64_t npx = (int64_t)h * w;
    if (h < 0 || w < 0 || half < 0 || npx > 0x7fffffffLL || (npx > 0 && (!pts || !nrm || !prio || !free_px || !owner || !sums || !counts)))
        return fail(ctx, F3D_ERR_INVALID, "patch_seeds_sums: bad arguments");
    if (rounds) *rounds = 0;
    if (npx == 0) return F3D_OK;
    void* dstat;
    if ((rc = ensure(ctx, SLOT_PATCH_STATUS, (size_t)npx * 4 + 256, &dstat))) return rc;
    hipStream_t s = pick(ctx, stream);
    int r = 0;
    int32_t* counter = (int32_t*)((char*)dstat + (((size_t)npx * 4 + 63) & ~(size_t)63));
    F3D_HIP(ctx, f3d_launch_patch_seeds(pts, nrm, prio, free_px, h, w, half, radius, min_cosine, (int32_t*)dstat, owner, counter, &r, s));
    F3D_HIP(ctx, f3d_launch_patch_sums(owner, nullptr, npx, h, w, half, pts, nrm, clr, sums, counts, s));
    if (rounds) *rounds = r;
    return F3D_OK;
}

// ---------------------------------------------------------------------------------------------
// a5 on a device-resident cloud (Fusion.fuse_device): the per-frame steps, enqueue only
// ---------------------------------------------------------------------------------------------
int f3d_fusion_hits_dev(f3d_ctx* ctx, const uint8_t* inside, const int32_t* uv_all, int64_t n, const int64_t* count, const double* pts,
                        const double* nrm, const uint8_t* valid, int64_t npx, int32_t* ids, int32_t* uv, double* hit_pts, double* hit_nrm,
                        int64_t* stats, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || npx < 0 || n > 0x7ffffffeLL || !count || !stats || (npx > 0 && !valid) ||
        (n > 0 && (!inside || !uv_all || !pts || !nrm || !ids || !uv || !hit_pts || !hit_nrm)))
        return fail(ctx, F3D_ERR_INVALID, "fusion_hits: bad arguments");
    void* scratch;
    if ((rc = ensure(ctx, SLOT_FUSION, f3d_fusion_scratch_bytes(n), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_fusion_hits(inside, uv_all, n, count, pts, nrm, valid, npx, ids, uv, hit_pts, hit_nrm, stats, scratch,
                                        pick(ctx, stream)));
    return F3D_OK;
}

static bool norm_mode_ok(int mode) { return mode == F3D_NORM_PLAIN || mode == F3D_NORM_FMA || mode == F3D_NORM_HOST; }

int f3d_fusion_seed_update_dev(f3d_ctx* ctx, const int32_t* ids, int64_t m, const double* sums, const int32_t* counts, int norm_mode,
                               double* pts, double* nrm, double* clr, int64_t* nmerges, uint32_t* occ, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (m < 0 || !norm_mode_ok(norm_mode) || (m > 0 && (!ids || !sums || !counts || !pts || !nrm || !clr || !nmerges || !occ)))
        return fail(ctx, F3D_ERR_INVALID, "fusion_seed_update: bad arguments");
    F3D_HIP(ctx, f3d_launch_fusion_seed_update(ids, m, sums, counts, norm_mode, pts, nrm, clr, nmerges, occ, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_fusion_lookup_dev(f3d_ctx* ctx, const int32_t* owner, const int32_t* ids, int64_t npx, int32_t* uv2pt, uint8_t* free_px, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (npx < 0 || (npx > 0 && (!owner || !ids || !uv2pt || !free_px))) return fail(ctx, F3D_ERR_INVALID, "fusion_lookup: bad arguments");
    F3D_HIP(ctx, f3d_launch_fusion_lookup(owner, ids, npx, uv2pt, free_px, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_fusion_frame_check_dev(f3d_ctx* ctx, const uint8_t* free_px, const double* pts, const double* nrm, int64_t npx, double radius,
                               double min_cosine, int64_t* stats, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (npx < 0 || !stats || (npx > 0 && (!free_px || !pts || !nrm))) return fail(ctx, F3D_ERR_INVALID, "fusion_frame_check: bad arguments");
    F3D_HIP(ctx, f3d_launch_fusion_check(free_px, pts, nrm, npx, radius, min_cosine, stats, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_fusion_prio_dev(f3d_ctx* ctx, const int64_t* order, int64_t npx, int32_t* prio, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (npx < 0 || npx > 0x7fffffffLL || (npx > 0 && (!order || !prio))) return fail(ctx, F3D_ERR_INVALID, "fusion_prio: bad arguments");
    F3D_HIP(ctx, f3d_launch_fusion_prio(order, npx, prio, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_fusion_new_seeds_dev(f3d_ctx* ctx, const int32_t* owner, const int32_t* prio, const double* sums, const int32_t* counts, int64_t npx,
                             int norm_mode, int64_t* count, int64_t cap, double* pts, double* nrm, double* clr, int64_t* nmerges,
                             uint32_t* occ, int32_t* uv2pt, uint8_t* free_px, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (npx < 0 || npx > 0x7ffffffeLL || cap < 0 || cap > 0x7fffffffLL || !norm_mode_ok(norm_mode) || !count ||
        (npx > 0 && (!owner || !prio || !sums || !counts || !pts || !nrm || !clr || !nmerges || !occ || !uv2pt || !free_px)))
        return fail(ctx, F3D_ERR_INVALID, "fusion_new_seeds: bad arguments");
    if (npx == 0) return F3D_OK;
    void* scratch;
    if ((rc = ensure(ctx, SLOT_FUSION, f3d_fusion_scratch_bytes(npx), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_fusion_new_seeds(owner, prio, sums, counts, npx, norm_mode, count, cap, pts, nrm, clr, nmerges, occ, uv2pt, free_px,
                                             scratch, pick(ctx, stream)));
    return F3D_OK;
}

// ---------------------------------------------------------------------------------------------
// (f)#1 adjacency: KDTree(points).query_radius(points, r) (fusion.py:374-375) as CSR
// ---------------------------------------------------------------------------------------------
// The one blocking readback of the grid builders: the bounding box of the cloud, as lo and ext = hi - lo.  NaN or infinity in the
// cloud, or an extent beyond 1e300, is F3D_ERR_INVALID (`op` names the operation).
static int cloud_bbox(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, hipStream_t s, const char* op, double lo[3], double ext[3]) {
    void* dbox;
    int rc = ensure(ctx, SLOT_GRAPH_BBOX, f3d_graph_bbox_bytes(), &dbox); if (rc) return rc;
    int nb = 0;
    F3D_HIP(ctx, f3d_launch_graph_bbox(xyz, dtype, n, dbox, &nb, s));
    std::vector<char> hbox(f3d_graph_bbox_bytes());
    F3D_HIP(ctx, hipMemcpyAsync(hbox.data(), dbox, hbox.size(), hipMemcpyDeviceToHost, s));
    F3D_HIP(ctx, hipStreamSynchronize(s));
    double hi[3];
    if (f3d_graph_reduce_bbox(hbox.data(), nb, lo, hi)) return fail(ctx, F3D_ERR_INVALID, "%s: the cloud contains NaN or infinity", op);
    for (int c = 0; c < 3; ++c) { ext[c] = hi[c] - lo[c]; if (!(ext[c] < 1e300)) return fail(ctx, F3D_ERR_INVALID, "%s: extent overflow", op); }
    return F3D_OK;
}

// a search grid fits when every axis has <= 1024 cells and the cell table <= 2^24 cells
constexpr int64_t GRID_MAX_CELLS = 16777216;
static bool search_grid_fits(const double d[3]) {
    return d[0] <= 1024.0 && d[1] <= 1024.0 && d[2] <= 1024.0 && d[0] * d[1] * d[2] <= (double)GRID_MAX_CELLS;
}

// What a radius search in a cloud needs (f3d_gridsearch), from the cloud's bounding box (cloud_bbox: synchronises): the grid with a
// cell edge a hair above the radius, the box grown by one cell and sklearn's reduced radius r ** 2.  radius < 0 or NaN: no pair at
// all (sklearn); the grid is built for radius 0 and no distance passes r2 = -1.
static int cloud_search(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, double radius, hipStream_t s, const char* op,
                        f3d_gridsearch* gs) {
    double lo[3], ext[3];
    int rc = cloud_bbox(ctx, xyz, dtype, n, s, op, lo, ext); if (rc) return rc;
    const bool none = !(radius >= 0.0);
    const double cell = neighbour_cell(none ? 0.0 : radius, ext, gs->g.dim, search_grid_fits);
    for (int c = 0; c < 3; ++c) { gs->g.lo[c] = lo[c]; gs->reach.lo[c] = lo[c] - cell; gs->reach.hi[c] = (lo[c] + ext[c]) + cell; }
    gs->g.inv_cell = 1.0 / cell; gs->g.pad = 0;
    gs->r2 = none ? -1.0 : radius * radius;
    return F3D_OK;
}

int f3d_radius_graph_count_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, double radius, int64_t* offsets,
                               int64_t* nnz, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n > 0x7fffffffLL || !nnz || (n > 0 && (!xyz || !offsets)) || !(radius >= 0.0) || !(radius < 1e300))
        return fail(ctx, F3D_ERR_INVALID, "radius_graph: bad arguments (n < 2^31, finite radius >= 0)");
    *nnz = 0; ctx->graph_n = -1; ctx->graph_kept = false;
    if (n == 0) return F3D_OK;
    hipStream_t s = pick(ctx, stream);
    f3d_gridsearch gs;
    if ((rc = cloud_search(ctx, xyz, dtype, n, radius, s, "radius_graph", &gs))) return rc;   // NaN: sklearn's KDTree raises ValueError
    void* scratch;
    if ((rc = ensure(ctx, SLOT_GRAPH, f3d_graph_scratch_bytes(n, f3d_ncells(gs.g)), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_graph_count(xyz, dtype, n, gs, scratch, offsets, s));
    F3D_HIP(ctx, hipMemcpyAsync(nnz, offsets + n, 8, hipMemcpyDeviceToHost, s));
    F3D_HIP(ctx, hipStreamSynchronize(s));
    ctx->graph = gs; ctx->graph_n = n;
    return F3D_OK;
}

int f3d_radius_graph_fill_dev(f3d_ctx* ctx, int64_t n, const int64_t* offsets, int32_t* nbrs, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n != ctx->graph_n || n < 0) return fail(ctx, F3D_ERR_INVALID, "radius_graph_fill: call f3d_radius_graph_count for this cloud first");
    if (n == 0) return F3D_OK;
    if (!offsets || !nbrs) return fail(ctx, F3D_ERR_INVALID, "radius_graph_fill: bad arguments");
    F3D_HIP(ctx, f3d_launch_graph_fill(n, ctx->graph, ctx->scratch[SLOT_GRAPH].p, offsets, nbrs, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_radius_graph_count(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, double radius, int64_t* offsets, int64_t* nnz) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || !nnz || (n > 0 && (!xyz || !offsets))) return fail(ctx, F3D_ERR_INVALID, "radius_graph: bad arguments");
    *nnz = 0;
    if (n == 0) { ctx->graph_n = 0; return F3D_OK; }
    staging st(ctx);
    const void* dxyz = st.in(xyz, xyz_bytes(dtype, n));
    int64_t* doffs = (int64_t*)st.keep(KEPT_GRAPH_OFFS, (size_t)(n + 1) * 8);   // f3d_radius_graph_fill reads them there
    st.back(offsets, doffs, (size_t)(n + 1) * 8);
    if (!st.rc) st.rc = f3d_radius_graph_count_dev(ctx, dxyz, dtype, n, radius, doffs, nnz, ctx->stream);
    if ((rc = st.finish())) { ctx->graph_n = -1; return rc; }
    ctx->graph_kept = true;
    return F3D_OK;
}

int f3d_radius_graph_fill(f3d_ctx* ctx, int64_t n, int32_t* nbrs) {
    int rc = enter(ctx); if (rc) return rc;
    if (n != ctx->graph_n || n < 0 || (n > 0 && !ctx->graph_kept))
        return fail(ctx, F3D_ERR_INVALID, "radius_graph_fill: call f3d_radius_graph_count for this cloud first");
    if (n == 0) return F3D_OK;
    hipStream_t s = ctx->stream;
    int64_t nnz = 0;
    const int64_t* doffs = (const int64_t*)ctx->kept[KEPT_GRAPH_OFFS].p;   // left there by f3d_radius_graph_count
    F3D_HIP(ctx, hipMemcpyAsync(&nnz, doffs + n, 8, hipMemcpyDeviceToHost, s));
    F3D_HIP(ctx, hipStreamSynchronize(s));
    if (nnz == 0) return F3D_OK;
    if (!nbrs) return fail(ctx, F3D_ERR_INVALID, "radius_graph_fill: nbrs is NULL");
    staging st(ctx);
    int32_t* dnb = st.out(nbrs, (size_t)nnz * 4);
    if (!st.rc) st.rc = f3d_radius_graph_fill_dev(ctx, n, doffs, dnb, s);
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// radius query: KDTree(data).query_radius(queries, r) inverted per query (correspondance.py:234-242) as CSR
// ---------------------------------------------------------------------------------------------
int f3d_radius_query_count_dev(f3d_ctx* ctx, const void* data, f3d_dtype ddtype, int64_t m, const void* queries, f3d_dtype qdtype, int64_t n,
                               double radius, int64_t* offsets, int64_t* nnz, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    ctx->qry_n = -1; ctx->qry_kept = false;
    if (!nnz || m < 0 || m > 0x7fffffffLL || n < 0 || n > 0x7fffffffLL || (m > 0 && !data) || (n > 0 && (!queries || !offsets)) ||
        !dtype_ok(ddtype) || !dtype_ok(qdtype) || radius >= 1e300)
        return fail(ctx, F3D_ERR_INVALID, "radius_query: bad arguments (m, n < 2^31, radius < 1e300)");
    if (m == 0) return fail(ctx, F3D_ERR_INVALID, "radius_query: the data set is empty (sklearn's KDTree raises ValueError)");
    *nnz = 0;
    if (n == 0) { ctx->qry_n = 0; return F3D_OK; }
    hipStream_t s = pick(ctx, stream);
    f3d_gridsearch gs;
    if ((rc = cloud_search(ctx, data, ddtype, m, radius, s, "radius_query", &gs))) return rc;
    void* scratch;
    if ((rc = ensure(ctx, SLOT_QRY, f3d_query_scratch_bytes(m, n, f3d_ncells(gs.g)), &scratch))) return rc;
    int64_t words[2] = {0, 0};
    F3D_HIP(ctx, f3d_launch_query_count(data, ddtype, m, queries, qdtype, n, gs, scratch, offsets, words, s));
    F3D_HIP(ctx, hipStreamSynchronize(s));
    if (words[1]) return fail(ctx, F3D_ERR_INVALID, "radius_query: the queries contain NaN or infinity");
    *nnz = words[0];
    ctx->qry = gs; ctx->qry_m = m; ctx->qry_n = n; ctx->qry_qdtype = qdtype; ctx->qry_queries = queries;
    return F3D_OK;
}

int f3d_radius_query_fill_dev(f3d_ctx* ctx, const void* queries, f3d_dtype qdtype, int64_t n, const int64_t* offsets, int32_t* nbrs,
                              void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n != ctx->qry_n || (n > 0 && (queries != ctx->qry_queries || qdtype != ctx->qry_qdtype)))
        return fail(ctx, F3D_ERR_INVALID, "radius_query_fill: call f3d_radius_query_count for these queries first");
    if (n == 0) return F3D_OK;
    if (!offsets || !nbrs) return fail(ctx, F3D_ERR_INVALID, "radius_query_fill: bad arguments");
    F3D_HIP(ctx, f3d_launch_query_fill(queries, qdtype, ctx->qry_m, n, ctx->qry, ctx->scratch[SLOT_QRY].p, offsets, nbrs, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_radius_query_count(f3d_ctx* ctx, const void* data, f3d_dtype ddtype, int64_t m, const void* queries, f3d_dtype qdtype, int64_t n,
                           double radius, int64_t* offsets, int64_t* nnz) {
    int rc = enter(ctx); if (rc) return rc;
    ctx->qry_n = -1;
    if (!nnz || m < 0 || n < 0 || (m > 0 && !data) || (n > 0 && (!queries || !offsets)) ||
        !dtype_ok(ddtype) || !dtype_ok(qdtype))
        return fail(ctx, F3D_ERR_INVALID, "radius_query: bad arguments");
    staging st(ctx);
    const void* ddata = st.in(data, xyz_bytes(ddtype, m));
    void* dq = st.keep(KEPT_QRY_IN, xyz_bytes(qdtype, n));                         // f3d_radius_query_fill reads them there
    st.put(dq, queries, xyz_bytes(qdtype, n));
    int64_t* doffs = (int64_t*)st.keep(KEPT_QRY_OFFS, (size_t)(n + 1) * 8);        // and these
    st.back(offsets, doffs, (size_t)(n + 1) * 8);
    if (!st.rc) st.rc = f3d_radius_query_count_dev(ctx, ddata, ddtype, m, dq, qdtype, n, radius, doffs, nnz, ctx->stream);
    if ((rc = st.finish())) { ctx->qry_n = -1; return rc; }
    ctx->qry_kept = true;
    return F3D_OK;
}

int f3d_radius_query_fill(f3d_ctx* ctx, int64_t n, int32_t* nbrs) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n != ctx->qry_n || (n > 0 && !ctx->qry_kept))
        return fail(ctx, F3D_ERR_INVALID, "radius_query_fill: call f3d_radius_query_count for these queries first");
    if (n == 0) return F3D_OK;
    hipStream_t s = ctx->stream;
    int64_t nnz = 0;
    const int64_t* doffs = (const int64_t*)ctx->kept[KEPT_QRY_OFFS].p;       // left there by f3d_radius_query_count
    F3D_HIP(ctx, hipMemcpyAsync(&nnz, doffs + n, 8, hipMemcpyDeviceToHost, s));
    F3D_HIP(ctx, hipStreamSynchronize(s));
    if (nnz == 0) return F3D_OK;
    if (!nbrs) return fail(ctx, F3D_ERR_INVALID, "radius_query_fill: nbrs is NULL");
    staging st(ctx);
    int32_t* dnb = st.out(nbrs, (size_t)nnz * 4);
    if (!st.rc) st.rc = f3d_radius_query_fill_dev(ctx, ctx->qry_queries, (f3d_dtype)ctx->qry_qdtype, n, doffs, dnb, s);
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// hybrid k-nearest search and label transfer (no reference counterpart; contract in f3d.h)
// ---------------------------------------------------------------------------------------------
int f3d_ctx_reserve_knn(f3d_ctx* ctx, int64_t m) {
    int rc = enter(ctx); if (rc) return rc;
    if (m < 0 || m > 0x7fffffffLL) return fail(ctx, F3D_ERR_INVALID, "ctx_reserve_knn: bad arguments");
    return reserve(ctx, {{SLOT_GRAPH_BBOX, f3d_graph_bbox_bytes()}, {SLOT_KNN_FLAG, 64},
                         {SLOT_KNN, f3d_graph_scratch_bytes(m, GRID_MAX_CELLS)}});                     // (any grid the radius allows)
}

// What f3d_knn_query_dev and f3d_transfer_labels_dev share: the argument checks, the one readback (the cloud's box and the queries'
// non-finite flag together) and the data's grid, built in SLOT_KNN.  *run = false: nothing to launch (n == 0).
static int knn_prepare(f3d_ctx* ctx, const char* op, const void* data, f3d_dtype ddtype, int64_t m, const void* queries, f3d_dtype qdtype,
                       int64_t n, int k, double radius, hipStream_t s, f3d_gridsearch* gs, f3d_gridview* gv, bool* run) {
    *run = false;
    if (k < 1 || k > F3D_KNN_MAX_K) return fail(ctx, F3D_ERR_INVALID, "%s: k %d outside [1, %d]", op, k, F3D_KNN_MAX_K);
    if (m < 0 || m > 0x7fffffffLL || n < 0 || n > 0x7fffffffLL || (m > 0 && !data) || (n > 0 && !queries) ||
        !dtype_ok(ddtype) || !dtype_ok(qdtype) || radius >= 1e300)
        return fail(ctx, F3D_ERR_INVALID, "%s: bad arguments (m, n < 2^31, radius < 1e300)", op);
    if (m == 0) return fail(ctx, F3D_ERR_INVALID, "%s: the data set is empty", op);
    if (n == 0) return F3D_OK;
    void *dbox, *dflag;
    int rc = ensure(ctx, SLOT_GRAPH_BBOX, f3d_graph_bbox_bytes(), &dbox); if (rc) return rc;
    if ((rc = ensure(ctx, SLOT_KNN_FLAG, 64, &dflag))) return rc;
    unsigned flag = 0;
    F3D_HIP(ctx, hipMemsetAsync(dflag, 0, 4, s));
    F3D_HIP(ctx, f3d_launch_knn_flag(queries, qdtype, n, (unsigned*)dflag, s));
    F3D_HIP(ctx, hipMemcpyAsync(&flag, dflag, 4, hipMemcpyDeviceToHost, s));
    if ((rc = cloud_search(ctx, data, ddtype, m, radius, s, op, gs))) return rc;                    // (synchronises)
    if (flag) return fail(ctx, F3D_ERR_INVALID, "%s: the queries contain NaN or infinity", op);
    void* scratch;
    if ((rc = ensure(ctx, SLOT_KNN, f3d_graph_scratch_bytes(m, f3d_ncells(gs->g)), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_graph_grid(data, ddtype, m, gs->g, scratch, gv, s));
    *run = true;
    return F3D_OK;
}

int f3d_knn_query_dev(f3d_ctx* ctx, const void* data, f3d_dtype ddtype, int64_t m, const void* queries, f3d_dtype qdtype, int64_t n, int k,
                      double radius, int32_t* idx, double* dist2, int32_t* counts, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n > 0 && !idx) return fail(ctx, F3D_ERR_INVALID, "knn_query: idx is NULL");
    hipStream_t s = pick(ctx, stream);
    f3d_gridsearch gs;
    f3d_gridview gv;
    bool run;
    if ((rc = knn_prepare(ctx, "knn_query", data, ddtype, m, queries, qdtype, n, k, radius, s, &gs, &gv, &run)) || !run) return rc;
    F3D_HIP(ctx, f3d_launch_knn_query(queries, qdtype, n, k, gv, gs, idx, dist2, counts, s));
    return F3D_OK;
}

int f3d_transfer_labels_dev(f3d_ctx* ctx, const void* data, f3d_dtype ddtype, int64_t m, const int64_t* labels, const void* queries,
                            f3d_dtype qdtype, int64_t n, int k, double radius, int64_t fill, int64_t* out, int32_t* support, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if ((n > 0 && !out) || (m > 0 && !labels)) return fail(ctx, F3D_ERR_INVALID, "transfer_labels: labels or out is NULL");
    hipStream_t s = pick(ctx, stream);
    f3d_gridsearch gs;
    f3d_gridview gv;
    bool run;
    if ((rc = knn_prepare(ctx, "transfer_labels", data, ddtype, m, queries, qdtype, n, k, radius, s, &gs, &gv, &run)) || !run) return rc;
    F3D_HIP(ctx, f3d_launch_knn_labels(queries, qdtype, n, k, gv, gs, labels, fill, out, support, s));
    return F3D_OK;
}

int f3d_knn_query(f3d_ctx* ctx, const void* data, f3d_dtype ddtype, int64_t m, const void* queries, f3d_dtype qdtype, int64_t n, int k,
                  double radius, int32_t* idx, double* dist2, int32_t* counts) {
    int rc = enter(ctx); if (rc) return rc;
    if (k < 1 || k > F3D_KNN_MAX_K) return fail(ctx, F3D_ERR_INVALID, "knn_query: k %d outside [1, %d]", k, F3D_KNN_MAX_K);
    if (m < 0 || n < 0 || (m > 0 && !data) || (n > 0 && (!queries || !idx)) || !dtype_ok(ddtype) ||
        !dtype_ok(qdtype))
        return fail(ctx, F3D_ERR_INVALID, "knn_query: bad arguments");
    staging st(ctx);
    const void* ddata = st.in(data, xyz_bytes(ddtype, m));
    const void* dq = st.in(queries, xyz_bytes(qdtype, n));
    int32_t* didx = st.out(idx, (size_t)n * k * 4);
    double* dd2 = st.out(dist2, (size_t)n * k * 8);
    int32_t* dcnt = st.out(counts, (size_t)n * 4);
    if (!st.rc) st.rc = f3d_knn_query_dev(ctx, ddata, ddtype, m, dq, qdtype, n, k, radius, didx, dd2, dcnt, ctx->stream);
    return st.finish();
}

int f3d_transfer_labels(f3d_ctx* ctx, const void* data, f3d_dtype ddtype, int64_t m, const int64_t* labels, const void* queries,
                        f3d_dtype qdtype, int64_t n, int k, double radius, int64_t fill, int64_t* out, int32_t* support) {
    int rc = enter(ctx); if (rc) return rc;
    if (k < 1 || k > F3D_KNN_MAX_K) return fail(ctx, F3D_ERR_INVALID, "transfer_labels: k %d outside [1, %d]", k, F3D_KNN_MAX_K);
    if (m < 0 || n < 0 || (m > 0 && (!data || !labels)) || (n > 0 && (!queries || !out)) || !dtype_ok(ddtype) ||
        !dtype_ok(qdtype))
        return fail(ctx, F3D_ERR_INVALID, "transfer_labels: bad arguments");
    staging st(ctx);
    const void* ddata = st.in(data, xyz_bytes(ddtype, m));
    const void* dq = st.in(queries, xyz_bytes(qdtype, n));
    const int64_t* dlab = st.in(labels, (size_t)m * 8);
    int64_t* dout = st.out(out, (size_t)n * 8);
    int32_t* dsup = st.out(support, (size_t)n * 4);
    if (!st.rc) st.rc = f3d_transfer_labels_dev(ctx, ddata, ddtype, m, dlab, dq, qdtype, n, k, radius, fill, dout, dsup, ctx->stream);
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// PointVotingSegmentation.vote: radius search of the frame pixels in a cloud fused with the frame vote (voting.py:224-265)
// ---------------------------------------------------------------------------------------------
int f3d_ctx_reserve_point_vote(f3d_ctx* ctx, int64_t m, int ncols) {
    int rc = enter(ctx); if (rc) return rc;
    if (m < 0 || m > 0x7fffffffLL || ncols <= 0) return fail(ctx, F3D_ERR_INVALID, "ctx_reserve_point_vote: bad arguments");
    return reserve(ctx, {{SLOT_GRAPH_BBOX, f3d_graph_bbox_bytes()},
                         {SLOT_PVOTE, f3d_graph_scratch_bytes(m, GRID_MAX_CELLS)},                     // (any grid the radius allows)
                         {SLOT_PVOTE_BITS, f3d_pvote_bits_bytes(m, ncols, f3d_pvote_group(m, ncols))}});
}

int f3d_point_vote_frames_dev(f3d_ctx* ctx, const void* cloud, f3d_dtype cdtype, int64_t m, const void* queries, f3d_dtype qdtype,
                              const uint8_t* masks, int64_t nframes, int64_t hw, double radius, double* votes, int ncols, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    ctx->pv_partial = 0;
    if (m < 0 || m > 0x7fffffffLL || nframes < 0 || nframes > 0x3fffffffLL || hw < 0 || ncols <= 0 || (m > 0 && (!cloud || !votes)) ||
        (nframes > 0 && hw > 0 && (!queries || !masks)) || !dtype_ok(cdtype) || !dtype_ok(qdtype) ||
        radius >= 1e300)
        return fail(ctx, F3D_ERR_INVALID, "point_vote_frames: bad arguments (m < 2^31, F < 2^30, radius < 1e300)");
    if (m == 0) return fail(ctx, F3D_ERR_INVALID, "point_vote_frames: the cloud is empty (sklearn's KDTree raises ValueError)");
    hipStream_t s = pick(ctx, stream);
    void* dbox;
    if ((rc = ensure(ctx, SLOT_GRAPH_BBOX, f3d_graph_bbox_bytes(), &dbox))) return rc;
    // one readback for the whole call: the cloud's box, and what the pre-pass saw in the masks and the queries
    int words[4] = {0, F3D_PVOTE_NONE, F3D_PVOTE_NONE, F3D_PVOTE_NONE};
    const bool work = nframes > 0 && hw > 0;
    if (work) {
        F3D_HIP(ctx, f3d_launch_pvote_prepass(queries, qdtype, masks, nframes, hw, ncols, ctx->pv_words, s));
        F3D_HIP(ctx, hipMemcpyAsync(words, ctx->pv_words, sizeof words, hipMemcpyDeviceToHost, s));
    }
    f3d_gridsearch gs;
    if ((rc = cloud_search(ctx, cloud, cdtype, m, radius, s, "point_vote_frames", &gs))) return rc;   // (synchronises)
    if (!work) return F3D_OK;
    const int64_t bad_query = words[1] == F3D_PVOTE_NONE ? nframes : words[1];                     // frames from here on never ran
    if (bad_query > 0) {
        const int group = (int)(bad_query < f3d_pvote_group(m, ncols) ? bad_query : f3d_pvote_group(m, ncols));
        void *scratch, *bits;
        if ((rc = ensure(ctx, SLOT_PVOTE, f3d_graph_scratch_bytes(m, f3d_ncells(gs.g)), &scratch))) return rc;
        if ((rc = ensure(ctx, SLOT_PVOTE_BITS, f3d_pvote_bits_bytes(m, ncols, group), &bits))) return rc;
        f3d_gridview gv;
        F3D_HIP(ctx, f3d_launch_graph_grid(cloud, cdtype, m, gs.g, scratch, &gv, s));
        if (words[0])                                                        // the second search: only when a label > nclasses exists
            F3D_HIP(ctx, f3d_launch_pvote_validate(queries, qdtype, masks, bad_query, hw, ncols, gv, gs, ctx->pv_words, s));
        F3D_HIP(ctx, f3d_launch_pvote_frames(queries, qdtype, masks, bad_query, hw, m, ncols, gv, gs, votes, (uint32_t*)bits, group,
                                             ctx->pv_words, ctx->dev_err, s));
        if (words[0]) F3D_HIP(ctx, f3d_launch_pvote_flag(ctx->pv_words, (int)bad_query, ctx->dev_err, s));
    }
    if (bad_query < nframes) {
        if (words[0] && bad_query > 0) {                                     // both offences in one call: the first offending frame decides
            F3D_HIP(ctx, hipMemcpyAsync(words, ctx->pv_words, sizeof words, hipMemcpyDeviceToHost, s));
            F3D_HIP(ctx, hipStreamSynchronize(s));
            if (words[2] < bad_query) return F3D_OK;                         // the IndexError, recorded for f3d_take_device_error
        }
        ctx->pv_partial = 1;
        return fail(ctx, F3D_ERR_INVALID, "point_vote_frames: the queries of frame %lld contain NaN or infinity (the frames before it are applied)",
                    (long long)bad_query);
    }
    return F3D_OK;
}

int f3d_point_vote_frames(f3d_ctx* ctx, const void* cloud, f3d_dtype cdtype, int64_t m, const void* queries, f3d_dtype qdtype,
                          const uint8_t* masks, int64_t nframes, int64_t hw, double radius, double* votes, int ncols) {
    int rc = enter(ctx); if (rc) return rc;
    if (m < 0 || nframes < 0 || hw < 0 || ncols <= 0 || (m > 0 && (!cloud || !votes)) || (nframes > 0 && hw > 0 && (!queries || !masks)) ||
        !dtype_ok(cdtype) || !dtype_ok(qdtype))
        return fail(ctx, F3D_ERR_INVALID, "point_vote_frames: bad arguments");
    staging st(ctx);
    const void* dcloud = st.in(cloud, xyz_bytes(cdtype, m));
    const void* dq = st.in(queries, xyz_bytes(qdtype, nframes * hw));
    const uint8_t* dmask = st.in(masks, (size_t)(nframes * hw));
    double* dvotes = st.inout(votes, (size_t)m * ncols * 8);
    if (st.rc) return st.rc;
    rc = f3d_point_vote_frames_dev(ctx, dcloud, cdtype, m, dq, qdtype, dmask, nframes, hw, radius, dvotes, ncols, ctx->stream);
    if (rc && !ctx->pv_partial) return rc;
    char msg[512];
    memcpy(msg, ctx->err, sizeof msg);
    const int rc2 = st.finish(F3D_DEVERR_PVOTE, true);                       // frames before an offending one stay applied, like NumPy
    if (rc && !rc2) memcpy(ctx->err, msg, sizeof msg);
    return rc2 ? rc2 : rc;
}

// ---------------------------------------------------------------------------------------------
// surface normals of depth frames: RTAB2Cache.surface_normal_estimation (ios_rtab.py:236-248)
// ---------------------------------------------------------------------------------------------
int f3d_estimate_normals_batch_dev(f3d_ctx* ctx, const double* xyz, int nframes, int64_t n, const double* cam_centres, double radius,
                                   int max_nn, int orient, double* normals, int32_t* counts, int32_t* neighbours, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (nframes < 0 || n < 0 || (int64_t)nframes * n > 0x7fffffffLL)
        return fail(ctx, F3D_ERR_INVALID, "estimate_normals: bad arguments (F >= 0, n >= 0, F * n < 2^31)");
    if (!(radius > 0.0) || !(radius < 1e300)) return fail(ctx, F3D_ERR_INVALID, "estimate_normals: radius must be finite and > 0");
    if (max_nn < 1 || max_nn > F3D_NORMALS_MAX_NN)
        return fail(ctx, F3D_ERR_INVALID, "estimate_normals: max_nn %d outside [1, %d]", max_nn, F3D_NORMALS_MAX_NN);
    const int64_t total = (int64_t)nframes * n;
    if (total == 0) return F3D_OK;
    if (!xyz || !normals || (orient && !cam_centres)) return fail(ctx, F3D_ERR_INVALID, "estimate_normals: bad arguments (NULL)");
    hipStream_t s = pick(ctx, stream);
    void *scratch, *dcams = nullptr;
    if ((rc = ensure(ctx, SLOT_NRM, f3d_normals_scratch_bytes(total), &scratch))) return rc;
    if (orient) {
        // staged before the readback below, which therefore also completes this upload from pageable memory
        if ((rc = ensure(ctx, SLOT_NRM_CAMS, (size_t)nframes * 24, &dcams))) return rc;
        F3D_HIP(ctx, hipMemcpyAsync(dcams, cam_centres, (size_t)nframes * 24, hipMemcpyHostToDevice, s));
    }
    double lo[3], ext[3];
    if ((rc = cloud_bbox(ctx, xyz, F3D_F64, total, s, "estimate_normals", lo, ext))) return rc;
    // the grid fits when frame + cell coordinates fit a 63-bit key.  No table over the cells: the key space may be sparse.
    const int fbits = f3d_bits_for(nframes, 0);
    f3d_nrmgrid g;
    const double cell = neighbour_cell(radius, ext, g.dim, [&](const double d[3]) {
        return d[0] <= 1073741824.0 && d[1] <= 1073741824.0 && d[2] <= 1073741824.0 &&
               fbits + f3d_bits_for((int64_t)d[0], 0) + f3d_bits_for((int64_t)d[1], 0) + f3d_bits_for((int64_t)d[2], 0) <= 63;
    });
    g.shift[0] = 0;
    for (int c = 0; c < 3; ++c) { g.lo[c] = lo[c]; g.shift[c + 1] = g.shift[c] + f3d_bits_for(g.dim[c], 0); }
    const int bits = fbits + g.shift[3];
    g.key_bits = bits < 1 ? 1 : bits;
    g.inv_cell = 1.0 / cell;
    F3D_HIP(ctx, f3d_launch_normals(xyz, nframes, n, g, radius * radius, max_nn, (const double*)dcams, orient, scratch, normals, counts,
                                    neighbours, s));
    return F3D_OK;
}

int f3d_estimate_normals(f3d_ctx* ctx, const double* xyz, int64_t n, const double cam_centre[3], double radius, int max_nn, int orient,
                         double* normals, int32_t* counts, int32_t* neighbours) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n > 0x7fffffffLL) return fail(ctx, F3D_ERR_INVALID, "estimate_normals: bad arguments (0 <= n < 2^31)");
    if (!(radius > 0.0) || !(radius < 1e300)) return fail(ctx, F3D_ERR_INVALID, "estimate_normals: radius must be finite and > 0");
    if (max_nn < 1 || max_nn > F3D_NORMALS_MAX_NN)
        return fail(ctx, F3D_ERR_INVALID, "estimate_normals: max_nn %d outside [1, %d]", max_nn, F3D_NORMALS_MAX_NN);
    if (n == 0) return F3D_OK;
    if (!xyz || !normals || (orient && !cam_centre)) return fail(ctx, F3D_ERR_INVALID, "estimate_normals: bad arguments (NULL)");
    staging st(ctx);
    const double* dxyz = st.in(xyz, (size_t)n * 24);
    double* dnrm = st.out(normals, (size_t)n * 24);
    int32_t* dcnt = st.out(counts, (size_t)n * 4);
    int32_t* dnb = st.out(neighbours, (size_t)n * max_nn * 4);
    if (!st.rc) st.rc = f3d_estimate_normals_batch_dev(ctx, dxyz, 1, n, cam_centre, radius, max_nn, orient, dnrm, dcnt, dnb, ctx->stream);
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// merge_bb support: grouping by instance id, hull candidates of every instance
// ---------------------------------------------------------------------------------------------
int f3d_group_by_id_dev(f3d_ctx* ctx, const int64_t* ids, int64_t n, int64_t nids, int32_t* order, uint32_t* sorted_ids, int64_t* starts,
                        void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n > 0x7fffffffLL || nids < 0 || nids >= 0x7fffffffLL || !starts || (n > 0 && (!ids || !order || !sorted_ids)))
        return fail(ctx, F3D_ERR_INVALID, "group_by_id: bad arguments (n, nids < 2^31)");
    void* scratch;
    if ((rc = ensure(ctx, SLOT_GRP_SCRATCH, f3d_group_scratch_bytes(n, nids), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_group_by_id(ids, n, nids, order, sorted_ids, starts, scratch, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_obb_extremes_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const int32_t* order, const uint32_t* sorted_ids,
                         int64_t nids, int32_t* extremes, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || nids < 0 || (nids > 0 && !extremes) || (n > 0 && (!xyz || !order || !sorted_ids)))
        return fail(ctx, F3D_ERR_INVALID, "obb_extremes: bad arguments");
    void* table;
    if ((rc = ensure(ctx, SLOT_OBB_TABLE, (size_t)nids * F3D_OBB_NDIR * 8, &table))) return rc;
    F3D_HIP(ctx, f3d_launch_obb_extremes(xyz, dtype, n, order, sorted_ids, nids, (unsigned long long*)table, extremes, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_obb_hull_filter_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const int32_t* order, const uint32_t* sorted_ids,
                            const int64_t* starts, int64_t nids, const int32_t* facet_start, const double* facets, const double* margin,
                            int32_t* cand, int32_t* cand_count, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || nids < 0 || (nids > 0 && (!facet_start || !margin || !cand_count || !starts)) || (n > 0 && (!xyz || !order || !sorted_ids || !cand)))
        return fail(ctx, F3D_ERR_INVALID, "obb_hull_filter: bad arguments");
    F3D_HIP(ctx, f3d_launch_obb_hull_filter(xyz, dtype, n, order, sorted_ids, starts, nids, facet_start, facets, margin, cand, cand_count,
                                            pick(ctx, stream)));
    return F3D_OK;
}

int f3d_obb_candidates_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const int32_t* order, const uint32_t* sorted_ids,
                           const int64_t* starts, int64_t nids, int min_members, int32_t* cand, int64_t* cand_start, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n > 0x7fffffffLL || nids < 0 || nids >= 0x7fffffffLL || (nids > 0 && (!starts || !cand_start)) ||
        (n > 0 && (!xyz || !order || !sorted_ids || !cand)))
        return fail(ctx, F3D_ERR_INVALID, "obb_candidates: bad arguments");
    void *table, *scratch;
    if ((rc = ensure(ctx, SLOT_OBB_TABLE, (size_t)nids * F3D_OBB_NDIR * 8, &table))) return rc;
    if ((rc = ensure(ctx, SLOT_OBB_FACETS, f3d_obb_candidates_scratch_bytes(n, nids), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_obb_candidates(xyz, dtype, n, order, sorted_ids, starts, nids, min_members, (unsigned long long*)table, scratch, cand,
                                           cand_start, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_gather_points_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, const int32_t* idx, int64_t count, double* out, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (count < 0 || (count > 0 && (!xyz || !idx || !out))) return fail(ctx, F3D_ERR_INVALID, "gather_points: bad arguments");
    F3D_HIP(ctx, f3d_launch_gather_points(xyz, dtype, idx, count, out, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_obb_fit_dev(f3d_ctx* ctx, const double* pts, const int64_t* start, int nfit, int64_t total, double* boxes, int32_t* status, uint8_t* isvert,
                    int32_t* nvert, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (nfit < 0 || total < 0 || (nfit > 0 && (!start || !boxes || !status || !isvert))) return fail(ctx, F3D_ERR_INVALID, "obb_fit: bad arguments");
    void* vlist;                                               // the vertices of every instance as a list (grows on first use only)
    if ((rc = ensure(ctx, SLOT_OBB_CAND, (size_t)total * 4, &vlist))) return rc;
    F3D_HIP(ctx, f3d_launch_obb_fit(pts, start, nfit, boxes, status, isvert, (int32_t*)vlist, nvert, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_obb_fit(f3d_ctx* ctx, const double* pts, const int64_t* start, int nfit, double* boxes, int32_t* status, uint8_t* isvert, int32_t* nvert) {
    int rc = enter(ctx); if (rc) return rc;
    if (nfit < 0 || (nfit > 0 && (!start || !boxes || !status))) return fail(ctx, F3D_ERR_INVALID, "obb_fit: bad arguments");
    if (nfit == 0) return F3D_OK;
    const int64_t total = start[nfit];
    if (total < 0 || start[0] != 0 || (total > 0 && !pts)) return fail(ctx, F3D_ERR_INVALID, "obb_fit: start must run from 0 to the number of points");
    for (int k = 0; k < nfit; ++k) if (start[k + 1] < start[k]) return fail(ctx, F3D_ERR_INVALID, "obb_fit: start must be non-decreasing");
    staging st(ctx);
    const double* dpts = st.in(pts, (size_t)total * 24);
    const int64_t* dstart = st.in(start, (size_t)(nfit + 1) * 8);
    double* dboxes = st.out(boxes, (size_t)nfit * sizeof(f3d_obb));
    int32_t* dstatus = (int32_t*)st.slot((size_t)nfit * 8);            // status, then the vertex counts
    uint8_t* dvert = (uint8_t*)st.slot((size_t)total);                 // written whether or not the caller wants it
    if (st.rc) return st.rc;
    st.back(status, dstatus, (size_t)nfit * 4);
    st.back(isvert, dvert, (size_t)total);
    st.back(nvert, dstatus + nfit, (size_t)nfit * 4);
    st.rc = f3d_obb_fit_dev(ctx, dpts, dstart, nfit, total, dboxes, dstatus, dvert, dstatus + nfit, ctx->stream);
    return st.finish();
}

// host-pointer sequence; the grouping (and, from the extremes call on, the cloud) stays in the context between the calls
int f3d_group_by_id(f3d_ctx* ctx, const int64_t* ids, int64_t n, int64_t nids, int32_t* order, int64_t* starts) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || nids < 0 || !starts || (n > 0 && (!ids || !order))) return fail(ctx, F3D_ERR_INVALID, "group_by_id: bad arguments");
    ctx->grp_n = -1; ctx->grp_cloud = false;
    staging st(ctx);
    const int64_t* dids = st.in(ids, (size_t)n * 8);
    int32_t* dorder = (int32_t*)st.keep(KEPT_GRP_ORDER, (size_t)n * 4);
    st.back(order, dorder, (size_t)n * 4);
    uint32_t* dkeys = (uint32_t*)st.keep(KEPT_GRP_KEYS, (size_t)n * 4);
    int64_t* dstarts = (int64_t*)st.keep(KEPT_GRP_STARTS, (size_t)(nids + 2) * 8);
    st.back(starts, dstarts, (size_t)(nids + 2) * 8);
    if (!st.rc) st.rc = f3d_group_by_id_dev(ctx, dids, n, nids, dorder, dkeys, dstarts, ctx->stream);
    if ((rc = st.finish())) return rc;
    ctx->grp_n = n; ctx->grp_nids = nids;
    return F3D_OK;
}

int f3d_obb_extremes(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, int32_t* extremes) {
    int rc = enter(ctx); if (rc) return rc;
    if (n != ctx->grp_n || n < 0) return fail(ctx, F3D_ERR_INVALID, "obb_extremes: call f3d_group_by_id for this cloud first");
    const int64_t nids = ctx->grp_nids;
    if ((n > 0 && !xyz) || (nids > 0 && !extremes)) return fail(ctx, F3D_ERR_INVALID, "obb_extremes: bad arguments");
    ctx->grp_cloud = false;
    staging st(ctx);
    void* dxyz = st.keep(KEPT_GRP_XYZ, xyz_bytes(dtype, n));                       // stays there for f3d_obb_hull_filter
    st.put(dxyz, xyz, xyz_bytes(dtype, n));
    int32_t* dext = st.out(extremes, (size_t)nids * F3D_OBB_NDIR * 4);
    if (!st.rc) st.rc = f3d_obb_extremes_dev(ctx, dxyz, dtype, n, (const int32_t*)ctx->kept[KEPT_GRP_ORDER].p,
                                             (const uint32_t*)ctx->kept[KEPT_GRP_KEYS].p, nids, dext, ctx->stream);
    if ((rc = st.finish())) return rc;
    ctx->grp_dtype = dtype; ctx->grp_cloud = true;
    return F3D_OK;
}

int f3d_obb_hull_filter(f3d_ctx* ctx, int64_t n, const int32_t* facet_start, const double* facets, const double* margin, int32_t* cand,
                        int32_t* cand_count) {
    int rc = enter(ctx); if (rc) return rc;
    if (n != ctx->grp_n || n < 0 || !ctx->grp_cloud)
        return fail(ctx, F3D_ERR_INVALID, "obb_hull_filter: call f3d_group_by_id and f3d_obb_extremes for this cloud first");
    const int64_t nids = ctx->grp_nids;
    if (nids > 0 && (!facet_start || !margin || !cand_count)) return fail(ctx, F3D_ERR_INVALID, "obb_hull_filter: bad arguments");
    if (nids == 0) return F3D_OK;
    const int64_t nf = facet_start[nids];
    if (nf < 0 || (nf > 0 && !facets) || (n > 0 && !cand)) return fail(ctx, F3D_ERR_INVALID, "obb_hull_filter: bad facet table");
    staging st(ctx);
    const int32_t* dfs = st.in(facet_start, (size_t)(nids + 1) * 4);
    const double* deq = st.in(facets, (size_t)nf * 32);
    const double* dmg = st.in(margin, (size_t)nids * 8);
    int32_t* dcand = st.out(cand, (size_t)n * 4);
    int32_t* dcnt = st.out(cand_count, (size_t)nids * 4);
    if (!st.rc) st.rc = f3d_obb_hull_filter_dev(ctx, ctx->kept[KEPT_GRP_XYZ].p, (f3d_dtype)ctx->grp_dtype, n, (const int32_t*)ctx->kept[KEPT_GRP_ORDER].p,
                                                (const uint32_t*)ctx->kept[KEPT_GRP_KEYS].p, (const int64_t*)ctx->kept[KEPT_GRP_STARTS].p, nids,
                                                dfs, deq, dmg, dcand, dcnt, ctx->stream);
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// occlusion-aware forward voting: point-splat z-buffer renders of the cloud (f3d_render.hip)
// ---------------------------------------------------------------------------------------------
#define F3D_ZKEY_BUDGET ((size_t)256 << 20)          // keys of an automatic pass
#define F3D_RENDER_BAD "bad arguments (n < 2^31, float64 / float32 cloud, h, w > 0, splat in [0, 8])"

static bool render_args_ok(const void* xyz, f3d_dtype dtype, int64_t n, const void* views, int nviews, int h, int w, int splat) {
    return n >= 0 && n <= 0x7fffffffLL && dtype_ok(dtype) && nviews >= 0 && h > 0 && w > 0 && splat >= 0 && splat <= 8 &&
           (n == 0 || xyz) && (nviews == 0 || views);
}

// views of one pass: views_per_pass, or with 0 as many as fit the budget; at least 1, at most nviews
static int render_pass_views(int nviews, int h, int w, int views_per_pass) {
    int64_t per = views_per_pass > 0 ? (int64_t)views_per_pass : (int64_t)(F3D_ZKEY_BUDGET / ((size_t)h * w * 8));
    if (per < 1) per = 1;
    return (int)(per < nviews ? per : nviews);
}

int f3d_ctx_reserve_render(f3d_ctx* ctx, int64_t n, int nviews, int h, int w) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || n > 0x7fffffffLL || nviews < 0 || h <= 0 || w <= 0) return fail(ctx, F3D_ERR_INVALID, "ctx_reserve_render: bad arguments");
    return reserve(ctx, {{SLOT_ZKEY, (size_t)render_pass_views(nviews, h, w, 0) * h * w * 8}});
}

int f3d_render_lookups_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views_dev, int nviews, int h, int w,
                           int splat, float* depth, int32_t* uv2pt, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!render_args_ok(xyz, dtype, n, views_dev, nviews, h, w, splat)) return fail(ctx, F3D_ERR_INVALID, "render_lookups: " F3D_RENDER_BAD);
    if (nviews == 0 || (!depth && !uv2pt)) return F3D_OK;
    hipStream_t s = pick(ctx, stream);
    const size_t hw = (size_t)h * w;
    const int per = render_pass_views(nviews, h, w, 0);
    void* zk;
    if ((rc = ensure(ctx, SLOT_ZKEY, (size_t)per * hw * 8, &zk))) return rc;
    unsigned long long* zkey = (unsigned long long*)zk;
    for (int v0 = 0; v0 < nviews; v0 += per) {
        const int nv = nviews - v0 < per ? nviews - v0 : per;
        F3D_HIP(ctx, f3d_launch_zkey_fill(zkey, (size_t)nv * hw, s));
        F3D_HIP(ctx, f3d_launch_zsplat(xyz, dtype, n, views_dev + v0, nv, h, w, splat, zkey, nullptr, s));
        F3D_HIP(ctx, f3d_launch_zkey_unpack(zkey, (size_t)nv * hw, depth ? depth + (size_t)v0 * hw : nullptr,
                                            uv2pt ? uv2pt + (size_t)v0 * hw : nullptr, nullptr, s));
    }
    return F3D_OK;
}

int f3d_render_lookups(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views, int nviews, int h, int w, int splat,
                       float* depth, int32_t* uv2pt) {
    int rc = enter(ctx); if (rc) return rc;
    if (!render_args_ok(xyz, dtype, n, views, nviews, h, w, splat)) return fail(ctx, F3D_ERR_INVALID, "render_lookups: " F3D_RENDER_BAD);
    if (nviews == 0) return F3D_OK;
    const size_t cells = (size_t)nviews * h * w;
    staging st(ctx);
    const void* dxyz = st.in(xyz, xyz_bytes(dtype, n));
    const f3d_view* dviews = st.in(views, sizeof(f3d_view) * (size_t)nviews);
    float* ddepth = st.out(depth, cells * 4);
    int32_t* dlut = st.out(uv2pt, cells * 4);
    if (!st.rc) st.rc = f3d_render_lookups_dev(ctx, dxyz, dtype, n, dviews, nviews, h, w, splat, ddepth, dlut, ctx->stream);
    return st.finish();
}

int f3d_vote_visible_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views_dev, int nviews, const uint8_t* masks,
                         int h, int w, int splat, double depth_tol, double* votes, int ncols, int views_per_pass, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!render_args_ok(xyz, dtype, n, views_dev, nviews, h, w, splat) || !(depth_tol >= 0.0) || ncols <= 0 || views_per_pass < 0 ||
        (n > 0 && !votes) || (nviews > 0 && !masks))
        return fail(ctx, F3D_ERR_INVALID, "vote_visible: " F3D_RENDER_BAD ", depth_tol >= 0, views_per_pass >= 0");
    if (n == 0 || nviews == 0) return F3D_OK;
    hipStream_t s = pick(ctx, stream);
    const size_t hw = (size_t)h * w;
    const int per = render_pass_views(nviews, h, w, views_per_pass);
    void* zk;
    if ((rc = ensure(ctx, SLOT_ZKEY, (size_t)per * hw * 8, &zk))) return rc;
    unsigned long long* zkey = (unsigned long long*)zk;
    for (int v0 = 0; v0 < nviews; v0 += per) {                               // a pass: render, then vote (votes are sums over views)
        const int nv = nviews - v0 < per ? nviews - v0 : per;
        F3D_HIP(ctx, f3d_launch_zkey_fill(zkey, (size_t)nv * hw, s));
        F3D_HIP(ctx, f3d_launch_zsplat(xyz, dtype, n, views_dev + v0, nv, h, w, splat, zkey, nullptr, s));
        F3D_HIP(ctx, f3d_launch_vote_visible(xyz, dtype, n, views_dev + v0, nv, masks + (size_t)v0 * hw, h, w, zkey, depth_tol, votes, ncols,
                                             nullptr, ctx->dev_err, s));
    }
    return F3D_OK;
}

int f3d_vote_visible(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views, int nviews, const uint8_t* masks,
                     int h, int w, int splat, double depth_tol, double* votes, int ncols, int views_per_pass) {
    int rc = enter(ctx); if (rc) return rc;
    if (!render_args_ok(xyz, dtype, n, views, nviews, h, w, splat) || !(depth_tol >= 0.0) || ncols <= 0 || views_per_pass < 0 ||
        (n > 0 && !votes) || (nviews > 0 && !masks))
        return fail(ctx, F3D_ERR_INVALID, "vote_visible: " F3D_RENDER_BAD ", depth_tol >= 0, views_per_pass >= 0");
    if (n == 0 || nviews == 0) return F3D_OK;
    staging st(ctx);
    const void* dxyz = st.in(xyz, xyz_bytes(dtype, n));
    const f3d_view* dviews = st.in(views, sizeof(f3d_view) * (size_t)nviews);
    const uint8_t* dmasks = st.in(masks, (size_t)nviews * h * w);
    double* dvotes = st.inout(votes, (size_t)n * ncols * 8);
    if (!st.rc) st.rc = f3d_vote_visible_dev(ctx, dxyz, dtype, n, dviews, nviews, dmasks, h, w, splat, depth_tol, dvotes, ncols, views_per_pass,
                                             ctx->stream);
    return st.finish(F3D_DEVERR_ZVOTE);                                      // nothing is written back on an IndexError
}

int f3d_debug_render_counts(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views_dev, int nviews, int h, int w,
                            int splat, uint64_t counts[3], double ms[2], void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!render_args_ok(xyz, dtype, n, views_dev, nviews, h, w, splat) || !counts) return fail(ctx, F3D_ERR_INVALID, "debug_render_counts: " F3D_RENDER_BAD);
    hipStream_t s = pick(ctx, stream);
    const size_t hw = (size_t)h * w;
    const int per = render_pass_views(nviews, h, w, 0);
    void *zk, *cnt;
    if ((rc = ensure(ctx, SLOT_ZKEY, (size_t)per * hw * 8, &zk))) return rc;
    if ((rc = ensure(ctx, SLOT_ZCOUNTS, 3 * sizeof(unsigned long long), &cnt))) return rc;
    F3D_HIP(ctx, hipMemsetAsync(cnt, 0, 3 * sizeof(unsigned long long), s));
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; ++k) F3D_HIP(ctx, hipEventCreate(&ev[k]));
    double fill_ms = 0.0, splat_ms = 0.0;
    hipError_t e = hipSuccess;
    for (int v0 = 0; v0 < nviews && e == hipSuccess; v0 += per) {            // one synchronisation per pass: the events are read back
        const int nv = nviews - v0 < per ? nviews - v0 : per;
        float a = 0.f, b = 0.f;
        if ((e = hipEventRecord(ev[0], s)) != hipSuccess) break;
        if ((e = f3d_launch_zkey_fill((unsigned long long*)zk, (size_t)nv * hw, s)) != hipSuccess) break;
        if ((e = hipEventRecord(ev[1], s)) != hipSuccess) break;
        if ((e = f3d_launch_zsplat(xyz, dtype, n, views_dev + v0, nv, h, w, splat, (unsigned long long*)zk, (unsigned long long*)cnt, s)) != hipSuccess) break;
        if ((e = hipEventRecord(ev[2], s)) != hipSuccess) break;
        if ((e = hipEventSynchronize(ev[2])) != hipSuccess) break;
        if ((e = hipEventElapsedTime(&a, ev[0], ev[1])) != hipSuccess || (e = hipEventElapsedTime(&b, ev[1], ev[2])) != hipSuccess) break;
        fill_ms += a; splat_ms += b;
    }
    for (int k = 0; k < 3; ++k) (void)hipEventDestroy(ev[k]);
    F3D_HIP(ctx, e);
    F3D_HIP(ctx, hipMemcpyAsync(counts, cnt, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    F3D_HIP(ctx, hipStreamSynchronize(s));
    if (ms) { ms[0] = fill_ms; ms[1] = splat_ms; }
    return F3D_OK;
}

// ---------------------------------------------------------------------------------------------
// triangle-mesh z-buffer renders: face voting and mesh occlusion (f3d_raster.hip)
// ---------------------------------------------------------------------------------------------
#define F3D_RASTER_BAD "bad arguments (nv < 2^31, nt < 2^31, float64 / float32 vertices, int64 / int32 triangles, h, w > 0, h * w <= 2^30, z_far not NaN)"

struct raster_mesh { const void* verts; f3d_dtype vdtype; int64_t nv; const void* tris; int itype; int64_t nt; };

static bool raster_args_ok(const raster_mesh& m, const void* views, int nviews, int h, int w, double z_far) {
    return m.nv >= 0 && m.nv <= 0x7fffffffLL && m.nt >= 0 && m.nt <= 0x7fffffffLL && dtype_ok(m.vdtype) && (m.itype == F3D_I64 || m.itype == F3D_I32) &&
           nviews >= 0 && h > 0 && w > 0 && (int64_t)h * w <= ((int64_t)1 << 30) && z_far == z_far &&
           (m.nv == 0 || m.verts) && (m.nt == 0 || m.tris) && (nviews == 0 || views);
}

// views of a face-vote pass: a pass is also one launch of the batched vote
static int raster_vote_pass_views(int nviews, int h, int w, int views_per_pass) {
    const int per = render_pass_views(nviews, h, w, views_per_pass);
    const int64_t frames = vote_batch_frames((int64_t)h * w);
    return per < frames ? per : (int)frames;
}

int f3d_ctx_reserve_mesh_render(f3d_ctx* ctx, int nviews, int h, int w) {
    int rc = enter(ctx); if (rc) return rc;
    if (nviews < 0 || h <= 0 || w <= 0 || (int64_t)h * w > ((int64_t)1 << 30)) return fail(ctx, F3D_ERR_INVALID, "ctx_reserve_mesh_render: bad arguments");
    const size_t hw = (size_t)h * w;
    const int vper = raster_vote_pass_views(nviews, h, w, 0);
    return reserve(ctx, {{SLOT_ZKEY, (size_t)render_pass_views(nviews, h, w, 0) * hw * 8}, {SLOT_RASTER, f3d_raster_scratch_bytes(F3D_RASTER_LIST_CAP)},
                         {SLOT_ZLUT, (size_t)vper * hw * 4}}, (int64_t)vper * (int64_t)hw);
}

// the scratch every mesh render starts with: keys of `per` views, the rasteriser's block (cleared, the index pre-pass enqueued)
static int raster_begin(f3d_ctx* ctx, const raster_mesh& m, int nviews, int per, size_t hw, int64_t* straddling, hipStream_t s,
                        unsigned long long** zkey, void** rs) {
    int rc;
    void* zk;
    if ((rc = ensure(ctx, SLOT_ZKEY, (size_t)per * hw * 8, &zk))) return rc;
    if ((rc = ensure(ctx, SLOT_RASTER, f3d_raster_scratch_bytes(F3D_RASTER_LIST_CAP), rs))) return rc;
    *zkey = (unsigned long long*)zk;
    F3D_HIP(ctx, f3d_launch_raster_check(m.tris, m.itype, m.nt, m.nv, *rs, nviews, (long long*)straddling, ctx->dev_err, s));
    return F3D_OK;
}

static int raster_pass(f3d_ctx* ctx, const raster_mesh& m, const f3d_view* views_dev, int v0, int nv, int h, int w, double z_far,
                       unsigned long long* zkey, int64_t* straddling, void* rs, unsigned list_cap, bool stats, hipStream_t s) {
    F3D_HIP(ctx, f3d_launch_zkey_fill(zkey, (size_t)nv * h * w, s));       // (also under a bad index: the keys then stay empty)
    F3D_HIP(ctx, f3d_launch_raster(m.verts, m.vdtype, m.tris, m.itype, m.nt, views_dev, v0, nv, h, w, z_far, zkey, (long long*)straddling, rs, list_cap,
                                   stats, s));
    return F3D_OK;
}

static const int* raster_flag(const void* rs) { return (const int*)((const char*)rs + f3d_raster_scratch_layout(0).flag); }

int f3d_render_mesh_lookups_dev(f3d_ctx* ctx, const void* verts, f3d_dtype vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                                const f3d_view* views_dev, int nviews, int h, int w, double z_far, float* depth, int32_t* uv2tri,
                                int64_t* straddling, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    const raster_mesh m{verts, vdtype, nv, tris, itype, nt};
    if (!raster_args_ok(m, views_dev, nviews, h, w, z_far)) return fail(ctx, F3D_ERR_INVALID, "render_mesh_lookups: " F3D_RASTER_BAD);
    if (nviews == 0 || (!depth && !uv2tri && !straddling)) return F3D_OK;
    hipStream_t s = pick(ctx, stream);
    const size_t hw = (size_t)h * w;
    const int per = render_pass_views(nviews, h, w, 0);
    unsigned long long* zkey; void* rs;
    if ((rc = raster_begin(ctx, m, nviews, per, hw, straddling, s, &zkey, &rs))) return rc;
    for (int v0 = 0; v0 < nviews; v0 += per) {
        const int nvp = nviews - v0 < per ? nviews - v0 : per;
        if ((rc = raster_pass(ctx, m, views_dev, v0, nvp, h, w, z_far, zkey, straddling, rs, F3D_RASTER_LIST_CAP, false, s))) return rc;
        F3D_HIP(ctx, f3d_launch_zkey_unpack(zkey, (size_t)nvp * hw, depth ? depth + (size_t)v0 * hw : nullptr,
                                            uv2tri ? uv2tri + (size_t)v0 * hw : nullptr, raster_flag(rs), s));
    }
    return F3D_OK;
}

int f3d_render_mesh_lookups(f3d_ctx* ctx, const void* verts, f3d_dtype vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                            const f3d_view* views, int nviews, int h, int w, double z_far, float* depth, int32_t* uv2tri, int64_t* straddling) {
    int rc = enter(ctx); if (rc) return rc;
    const raster_mesh m{verts, vdtype, nv, tris, itype, nt};
    if (!raster_args_ok(m, views, nviews, h, w, z_far)) return fail(ctx, F3D_ERR_INVALID, "render_mesh_lookups: " F3D_RASTER_BAD);
    if (nviews == 0) return F3D_OK;
    const size_t cells = (size_t)nviews * h * w;
    staging st(ctx);
    const void* dverts = st.in(verts, xyz_bytes(vdtype, nv));
    const void* dtris = st.in(tris, tri_bytes(itype, nt));
    const f3d_view* dviews = st.in(views, sizeof(f3d_view) * (size_t)nviews);
    float* ddepth = st.out(depth, cells * 4);
    int32_t* dlut = st.out(uv2tri, cells * 4);
    int64_t* dstr = st.out(straddling, (size_t)nviews * 8);
    if (!st.rc) st.rc = f3d_render_mesh_lookups_dev(ctx, dverts, vdtype, nv, dtris, itype, nt, dviews, nviews, h, w, z_far, ddepth, dlut, dstr, ctx->stream);
    return st.finish(F3D_DEVERR_RASTER);                                     // nothing is written back on a bad index
}

int f3d_vote_faces_dev(f3d_ctx* ctx, const void* verts, f3d_dtype vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                       const f3d_view* views_dev, int nviews, const uint8_t* masks, int h, int w, double z_far, double* votes, int ncols,
                       int views_per_pass, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    const raster_mesh m{verts, vdtype, nv, tris, itype, nt};
    if (!raster_args_ok(m, views_dev, nviews, h, w, z_far) || ncols <= 0 || ncols > 256 || views_per_pass < 0 || (nt > 0 && !votes) || (nviews > 0 && !masks))
        return fail(ctx, F3D_ERR_INVALID, "vote_faces: " F3D_RASTER_BAD ", 0 < ncols <= 256, views_per_pass >= 0");
    if (nt == 0 || nviews == 0) return F3D_OK;
    hipStream_t s = pick(ctx, stream);
    const size_t hw = (size_t)h * w;
    const int per = raster_vote_pass_views(nviews, h, w, views_per_pass);
    unsigned long long* zkey; void *rs, *lut;
    if ((rc = raster_begin(ctx, m, nviews, per, hw, nullptr, s, &zkey, &rs))) return rc;
    if ((rc = ensure(ctx, SLOT_ZLUT, (size_t)per * hw * 4, &lut))) return rc;
    for (int v0 = 0; v0 < nviews; v0 += per) {                               // a pass: raster, unpack, the batched uv2pt vote over its lookups
        const int nvp = nviews - v0 < per ? nviews - v0 : per;
        if ((rc = raster_pass(ctx, m, views_dev, v0, nvp, h, w, z_far, zkey, nullptr, rs, F3D_RASTER_LIST_CAP, false, s))) return rc;
        // (under a bad index the keys stay empty, the lookups are all -1 and nothing votes)
        F3D_HIP(ctx, f3d_launch_zkey_unpack(zkey, (size_t)nvp * hw, nullptr, (int32_t*)lut, nullptr, s));
        if ((rc = vote_batch_enqueue(ctx, (const int32_t*)lut, masks + (size_t)v0 * hw, nvp, h, w, votes, nt, ncols, s))) return rc;
    }
    return F3D_OK;
}

int f3d_vote_faces(f3d_ctx* ctx, const void* verts, f3d_dtype vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                   const f3d_view* views, int nviews, const uint8_t* masks, int h, int w, double z_far, double* votes, int ncols,
                   int views_per_pass) {
    int rc = enter(ctx); if (rc) return rc;
    const raster_mesh m{verts, vdtype, nv, tris, itype, nt};
    if (!raster_args_ok(m, views, nviews, h, w, z_far) || ncols <= 0 || ncols > 256 || views_per_pass < 0 || (nt > 0 && !votes) || (nviews > 0 && !masks))
        return fail(ctx, F3D_ERR_INVALID, "vote_faces: " F3D_RASTER_BAD ", 0 < ncols <= 256, views_per_pass >= 0");
    if (nt == 0 || nviews == 0) return F3D_OK;
    staging st(ctx);
    const void* dverts = st.in(verts, xyz_bytes(vdtype, nv));
    const void* dtris = st.in(tris, tri_bytes(itype, nt));
    const f3d_view* dviews = st.in(views, sizeof(f3d_view) * (size_t)nviews);
    const uint8_t* dmasks = st.in(masks, (size_t)nviews * h * w);
    double* dvotes = st.inout(votes, (size_t)nt * ncols * 8);
    if (!st.rc) st.rc = f3d_vote_faces_dev(ctx, dverts, vdtype, nv, dtris, itype, nt, dviews, nviews, dmasks, h, w, z_far, dvotes, ncols, views_per_pass,
                                           ctx->stream);
    return st.finish(F3D_DEVERR_RASTER | F3D_DEVERR_VOTE);                   // nothing is written back on an IndexError
}

static bool visible_mesh_args_ok(const void* xyz, f3d_dtype dtype, int64_t n, const raster_mesh& m, const void* views, int nviews, const void* masks,
                                 int h, int w, double z_far, double depth_tol, const void* votes, int ncols, int views_per_pass) {
    return render_args_ok(xyz, dtype, n, views, nviews, h, w, 0) && raster_args_ok(m, views, nviews, h, w, z_far) && depth_tol >= 0.0 && ncols > 0 &&
           views_per_pass >= 0 && (n == 0 || votes) && (nviews == 0 || masks);
}

int f3d_vote_visible_mesh_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const void* verts, f3d_dtype vdtype, int64_t nv,
                              const void* tris, int itype, int64_t nt, const f3d_view* views_dev, int nviews, const uint8_t* masks, int h, int w,
                              double z_far, double depth_tol, double* votes, int ncols, int views_per_pass, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    const raster_mesh m{verts, vdtype, nv, tris, itype, nt};
    if (!visible_mesh_args_ok(xyz, dtype, n, m, views_dev, nviews, masks, h, w, z_far, depth_tol, votes, ncols, views_per_pass))
        return fail(ctx, F3D_ERR_INVALID, "vote_visible_mesh: " F3D_RASTER_BAD ", n < 2^31, depth_tol >= 0, views_per_pass >= 0");
    if (n == 0 || nviews == 0) return F3D_OK;
    hipStream_t s = pick(ctx, stream);
    const size_t hw = (size_t)h * w;
    const int per = render_pass_views(nviews, h, w, views_per_pass);
    unsigned long long* zkey; void* rs;
    if ((rc = raster_begin(ctx, m, nviews, per, hw, nullptr, s, &zkey, &rs))) return rc;
    for (int v0 = 0; v0 < nviews; v0 += per) {
        const int nvp = nviews - v0 < per ? nviews - v0 : per;
        if ((rc = raster_pass(ctx, m, views_dev, v0, nvp, h, w, z_far, zkey, nullptr, rs, F3D_RASTER_LIST_CAP, false, s))) return rc;
        F3D_HIP(ctx, f3d_launch_vote_visible(xyz, dtype, n, views_dev + v0, nvp, masks + (size_t)v0 * hw, h, w, zkey, depth_tol, votes, ncols,
                                             raster_flag(rs), ctx->dev_err, s));
    }
    return F3D_OK;
}

int f3d_vote_visible_mesh(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const void* verts, f3d_dtype vdtype, int64_t nv,
                          const void* tris, int itype, int64_t nt, const f3d_view* views, int nviews, const uint8_t* masks, int h, int w,
                          double z_far, double depth_tol, double* votes, int ncols, int views_per_pass) {
    int rc = enter(ctx); if (rc) return rc;
    const raster_mesh m{verts, vdtype, nv, tris, itype, nt};
    if (!visible_mesh_args_ok(xyz, dtype, n, m, views, nviews, masks, h, w, z_far, depth_tol, votes, ncols, views_per_pass))
        return fail(ctx, F3D_ERR_INVALID, "vote_visible_mesh: " F3D_RASTER_BAD ", n < 2^31, depth_tol >= 0, views_per_pass >= 0");
    if (n == 0 || nviews == 0) return F3D_OK;
    staging st(ctx);
    const void* dxyz = st.in(xyz, xyz_bytes(dtype, n));
    const void* dverts = st.in(verts, xyz_bytes(vdtype, nv));
    const void* dtris = st.in(tris, tri_bytes(itype, nt));
    const f3d_view* dviews = st.in(views, sizeof(f3d_view) * (size_t)nviews);
    const uint8_t* dmasks = st.in(masks, (size_t)nviews * h * w);
    double* dvotes = st.inout(votes, (size_t)n * ncols * 8);
    if (!st.rc) st.rc = f3d_vote_visible_mesh_dev(ctx, dxyz, dtype, n, dverts, vdtype, nv, dtris, itype, nt, dviews, nviews, dmasks, h, w, z_far, depth_tol,
                                                  dvotes, ncols, views_per_pass, ctx->stream);
    return st.finish(F3D_DEVERR_RASTER | F3D_DEVERR_ZVOTE);
}

int f3d_debug_raster_counts(f3d_ctx* ctx, const void* verts, f3d_dtype vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                            const f3d_view* views_dev, int nviews, int h, int w, double z_far, int64_t list_capacity, float* depth, int32_t* uv2tri,
                            uint64_t counts[4], double ms[2], void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    const raster_mesh m{verts, vdtype, nv, tris, itype, nt};
    if (!raster_args_ok(m, views_dev, nviews, h, w, z_far) || !counts || list_capacity < 0 || list_capacity > (int64_t)F3D_RASTER_LIST_CAP)
        return fail(ctx, F3D_ERR_INVALID, "debug_raster_counts: " F3D_RASTER_BAD ", list_capacity in [0, %u]", F3D_RASTER_LIST_CAP);
    hipStream_t s = pick(ctx, stream);
    const size_t hw = (size_t)h * w;
    const unsigned cap = list_capacity ? (unsigned)list_capacity : F3D_RASTER_LIST_CAP;
    const int per = render_pass_views(nviews, h, w, 0);
    unsigned long long* zkey; void* rs;
    if ((rc = raster_begin(ctx, m, nviews, per, hw, nullptr, s, &zkey, &rs))) return rc;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; ++k) F3D_HIP(ctx, hipEventCreate(&ev[k]));
    double fill_ms = 0.0, raster_ms = 0.0;
    hipError_t e = hipSuccess;
    for (int v0 = 0; v0 < nviews && e == hipSuccess; v0 += per) {            // one synchronisation per pass: the events are read back
        const int nvp = nviews - v0 < per ? nviews - v0 : per;
        float a = 0.f, b = 0.f;
        if ((e = hipEventRecord(ev[0], s)) != hipSuccess) break;
        if ((e = f3d_launch_zkey_fill(zkey, (size_t)nvp * hw, s)) != hipSuccess) break;
        if ((e = hipEventRecord(ev[1], s)) != hipSuccess) break;
        if ((e = f3d_launch_raster(verts, vdtype, tris, itype, nt, views_dev, v0, nvp, h, w, z_far, zkey, nullptr, rs, cap, true, s)) != hipSuccess) break;
        if ((e = hipEventRecord(ev[2], s)) != hipSuccess) break;
        if ((e = f3d_launch_zkey_unpack(zkey, (size_t)nvp * hw, depth ? depth + (size_t)v0 * hw : nullptr, uv2tri ? uv2tri + (size_t)v0 * hw : nullptr,
                                        raster_flag(rs), s)) != hipSuccess) break;
        if ((e = hipEventSynchronize(ev[2])) != hipSuccess) break;
        if ((e = hipEventElapsedTime(&a, ev[0], ev[1])) != hipSuccess || (e = hipEventElapsedTime(&b, ev[1], ev[2])) != hipSuccess) break;
        fill_ms += a; raster_ms += b;
    }
    for (int k = 0; k < 3; ++k) (void)hipEventDestroy(ev[k]);
    F3D_HIP(ctx, e);
    F3D_HIP(ctx, hipMemcpyAsync(counts, (const char*)rs + f3d_raster_scratch_layout(0).stats, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    F3D_HIP(ctx, hipStreamSynchronize(s));
    if (ms) { ms[0] = fill_ms; ms[1] = raster_ms; }
    return F3D_OK;
}

// ---------------------------------------------------------------------------------------------
// TSDF reconstruction: depth frames -> signed distance volume -> surface-nets mesh (include/f3d.h)
// ---------------------------------------------------------------------------------------------
static bool pos_finite(double x) { return x > 0.0 && x < INFINITY; }

// voxels of a volume, or -1 for dims the entries refuse
static int64_t tsdf_voxels(int nx, int ny, int nz) {
    if (nx <= 0 || ny <= 0 || nz <= 0) return -1;
    const int64_t xy = (int64_t)nx * ny;
    if (xy >= ((int64_t)1 << 31) || xy * nz >= ((int64_t)1 << 31)) return -1;
    return xy * nz;
}

static size_t depth_bytes(int depth_type, int nframes, int h, int w) {
    return (size_t)nframes * h * w * (depth_type == F3D_DEPTH_U16 ? 2 : depth_type == F3D_DEPTH_F32 ? 4 : 8);
}

#define F3D_TSDF_BAD "bad arguments (dims >= 1 with a product < 2^31; vs, trunc, depth_scale, max_depth finite and > 0; max_weight in [1, 2^24]; a known depth type)"
static bool tsdf_integrate_ok(const float* tsdf, const float* weight, int nx, int ny, int nz, const double* lo, double vs, double trunc,
                              float max_weight, const void* depth, int depth_type, int nframes, int h, int w, double depth_scale,
                              double max_depth, const f3d_view* views) {
    return tsdf && weight && lo && tsdf_voxels(nx, ny, nz) > 0 && pos_finite(vs) && pos_finite(trunc) && pos_finite(depth_scale) &&
           pos_finite(max_depth) && max_weight >= 1.0f && max_weight <= F3D_TSDF_MAX_WEIGHT &&
           (depth_type == F3D_DEPTH_U16 || depth_type == F3D_DEPTH_F32 || depth_type == F3D_DEPTH_F64) && nframes >= 0 && h > 0 && w > 0 &&
           (int64_t)h * w < ((int64_t)1 << 31) && (nframes == 0 || (depth && views));
}

int f3d_ctx_reserve_tsdf(f3d_ctx* ctx, int64_t nvoxels) {
    int rc = enter(ctx); if (rc) return rc;
    if (nvoxels < 0 || nvoxels >= ((int64_t)1 << 31)) return fail(ctx, F3D_ERR_INVALID, "ctx_reserve_tsdf: nvoxels must be in [0, 2^31)");
    ctx->tsdf_n = -1;                                                          // the buffer may move: a counted sequence ends here
    return reserve(ctx, {{SLOT_TSDF, f3d_tsdf_scratch_bytes(nvoxels)}});
}

int f3d_debug_tsdf_grid_cap(f3d_ctx* ctx, int blocks) {
    int rc = enter(ctx); if (rc) return rc;
    if (blocks < 0) return fail(ctx, F3D_ERR_INVALID, "debug_tsdf_grid_cap: blocks must not be negative");
    ctx->tsdf_grid_cap = blocks;
    return F3D_OK;
}

int f3d_debug_grid_cap(f3d_ctx* ctx, int blocks) {
    int rc = enter(ctx); if (rc) return rc;
    if (blocks < 0) return fail(ctx, F3D_ERR_INVALID, "debug_grid_cap: blocks must not be negative");
    f3d_grid_debug_state.blocks.store(blocks, std::memory_order_relaxed);
    return F3D_OK;
}

int f3d_debug_grid_cap_stats(f3d_ctx* ctx, int64_t out[2]) {
    int rc = enter(ctx); if (rc) return rc;
    if (!out) return fail(ctx, F3D_ERR_INVALID, "debug_grid_cap_stats: out must not be NULL");
    out[0] = f3d_grid_debug_state.calls.exchange(0, std::memory_order_relaxed);
    out[1] = f3d_grid_debug_state.lowered.exchange(0, std::memory_order_relaxed);
    return F3D_OK;
}

int f3d_tsdf_integrate_dev(f3d_ctx* ctx, float* tsdf, float* weight, int nx, int ny, int nz, const double lo[3], double vs, double trunc,
                           float max_weight, const void* depth, int depth_type, int nframes, int h, int w, double depth_scale,
                           double max_depth, const f3d_view* views_dev, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!tsdf_integrate_ok(tsdf, weight, nx, ny, nz, lo, vs, trunc, max_weight, depth, depth_type, nframes, h, w, depth_scale, max_depth, views_dev))
        return fail(ctx, F3D_ERR_INVALID, "tsdf_integrate: " F3D_TSDF_BAD);
    if (nframes == 0) return F3D_OK;
    F3D_HIP(ctx, f3d_launch_tsdf_integrate(tsdf, weight, nx, ny, nz, lo, vs, trunc, (double)max_weight, depth, depth_type, nframes, h, w, depth_scale,
                                           max_depth, views_dev, ctx->tsdf_grid_cap, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_tsdf_integrate(f3d_ctx* ctx, float* tsdf, float* weight, int nx, int ny, int nz, const double lo[3], double vs, double trunc,
                       float max_weight, const void* depth, int depth_type, int nframes, int h, int w, double depth_scale, double max_depth,
                       const f3d_view* views) {
    int rc = enter(ctx); if (rc) return rc;
    if (!tsdf_integrate_ok(tsdf, weight, nx, ny, nz, lo, vs, trunc, max_weight, depth, depth_type, nframes, h, w, depth_scale, max_depth, views))
        return fail(ctx, F3D_ERR_INVALID, "tsdf_integrate: " F3D_TSDF_BAD);
    if (nframes == 0) return F3D_OK;
    const size_t vol = (size_t)tsdf_voxels(nx, ny, nz) * 4;
    staging st(ctx);
    float* dt = st.inout(tsdf, vol);
    float* dw = st.inout(weight, vol);
    const void* dd = st.in((const char*)depth, depth_bytes(depth_type, nframes, h, w));
    const f3d_view* dviews = st.in(views, sizeof(f3d_view) * (size_t)nframes);
    if (!st.rc) st.rc = f3d_tsdf_integrate_dev(ctx, dt, dw, nx, ny, nz, lo, vs, trunc, max_weight, dd, depth_type, nframes, h, w, depth_scale, max_depth,
                                               dviews, ctx->stream);
    return st.finish();
}

int f3d_tsdf_extract_count_dev(f3d_ctx* ctx, const float* tsdf, const float* weight, int nx, int ny, int nz, float min_weight, int64_t* nv,
                               int64_t* nt, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    const int64_t n = tsdf_voxels(nx, ny, nz);
    if (!tsdf || !weight || !nv || !nt || n <= 0 || !(min_weight >= 1.0f))
        return fail(ctx, F3D_ERR_INVALID, "tsdf_extract_count: bad arguments (dims >= 1 with a product < 2^31, min_weight >= 1)");
    *nv = 0; *nt = 0; ctx->tsdf_n = -1; ctx->tsdf_kept = false;
    hipStream_t s = pick(ctx, stream);
    void* scratch;
    if ((rc = ensure(ctx, SLOT_TSDF, f3d_tsdf_scratch_bytes(n), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_tsdf_count(tsdf, weight, nx, ny, nz, min_weight, scratch, ctx->tsdf_counts, ctx->tsdf_grid_cap, s));
    F3D_HIP(ctx, hipStreamSynchronize(s));
    if (ctx->tsdf_counts[1] >= ((unsigned long long)1 << 30))
        return fail(ctx, F3D_ERR_INVALID, "tsdf_extract_count: %llu quads give 2^31 triangles or more", ctx->tsdf_counts[1]);
    ctx->tsdf_n = n; ctx->tsdf_dims[0] = nx; ctx->tsdf_dims[1] = ny; ctx->tsdf_dims[2] = nz;
    ctx->tsdf_nv = (int64_t)ctx->tsdf_counts[0]; ctx->tsdf_nq = (int64_t)ctx->tsdf_counts[1];
    *nv = ctx->tsdf_nv; *nt = 2 * ctx->tsdf_nq;
    return F3D_OK;
}

static bool tsdf_counted(const f3d_ctx* ctx, int nx, int ny, int nz) {
    return ctx->tsdf_n > 0 && ctx->tsdf_dims[0] == nx && ctx->tsdf_dims[1] == ny && ctx->tsdf_dims[2] == nz;
}

int f3d_tsdf_extract_fill_dev(f3d_ctx* ctx, const float* tsdf, int nx, int ny, int nz, const double lo[3], double vs, double* verts,
                              int32_t* tris, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!tsdf_counted(ctx, nx, ny, nz)) return fail(ctx, F3D_ERR_INVALID, "tsdf_extract_fill: call f3d_tsdf_extract_count for this volume first");
    if (!tsdf || !lo || !pos_finite(vs)) return fail(ctx, F3D_ERR_INVALID, "tsdf_extract_fill: bad arguments (vs finite and > 0)");
    if (ctx->tsdf_nv == 0) return F3D_OK;
    F3D_HIP(ctx, f3d_launch_tsdf_fill(tsdf, nx, ny, nz, lo, vs, ctx->scratch[SLOT_TSDF].p, verts, ctx->tsdf_nq ? tris : nullptr, ctx->tsdf_grid_cap,
                                      pick(ctx, stream)));
    return F3D_OK;
}

int f3d_tsdf_extract_count(f3d_ctx* ctx, const float* tsdf, const float* weight, int nx, int ny, int nz, float min_weight, int64_t* nv, int64_t* nt) {
    int rc = enter(ctx); if (rc) return rc;
    const int64_t n = tsdf_voxels(nx, ny, nz);
    if (!tsdf || !weight || !nv || !nt || n <= 0 || !(min_weight >= 1.0f))
        return fail(ctx, F3D_ERR_INVALID, "tsdf_extract_count: bad arguments (dims >= 1 with a product < 2^31, min_weight >= 1)");
    staging st(ctx);
    float* dt = (float*)st.keep(KEPT_TSDF, (size_t)n * 4);                     // f3d_tsdf_extract_fill reads the samples there
    st.put(dt, tsdf, (size_t)n * 4);
    const float* dw = st.in(weight, (size_t)n * 4);
    if (!st.rc) st.rc = f3d_tsdf_extract_count_dev(ctx, dt, dw, nx, ny, nz, min_weight, nv, nt, ctx->stream);
    if ((rc = st.finish())) { ctx->tsdf_n = -1; return rc; }
    ctx->tsdf_kept = true;
    return F3D_OK;
}

int f3d_tsdf_extract_fill(f3d_ctx* ctx, int nx, int ny, int nz, const double lo[3], double vs, double* verts, int32_t* tris) {
    int rc = enter(ctx); if (rc) return rc;
    if (!tsdf_counted(ctx, nx, ny, nz) || !ctx->tsdf_kept)
        return fail(ctx, F3D_ERR_INVALID, "tsdf_extract_fill: call f3d_tsdf_extract_count for this volume first");
    if (!lo || !pos_finite(vs)) return fail(ctx, F3D_ERR_INVALID, "tsdf_extract_fill: bad arguments (vs finite and > 0)");
    if (ctx->tsdf_nv == 0) return F3D_OK;
    staging st(ctx);
    double* dv = st.out(verts, (size_t)ctx->tsdf_nv * 24);
    int32_t* dtri = ctx->tsdf_nq ? st.out(tris, (size_t)ctx->tsdf_nq * 24) : nullptr;
    if (!st.rc) st.rc = f3d_tsdf_extract_fill_dev(ctx, (const float*)ctx->kept[KEPT_TSDF].p, nx, ny, nz, lo, vs, dv, dtri, ctx->stream);
    return st.finish();
}

// colour: the integrate arguments plus the colour state and the colour images; the vertex colours of a counted volume
#define F3D_TSDF_COLOR_BAD "bad arguments (those of tsdf_integrate; color and rgb not NULL, the device color 16-byte aligned; hc, wc_img > 0 with a product < 2^31)"
static bool tsdf_color_ok(const float* color, const uint8_t* rgb, int nframes, int hc, int wc_img) {
    return color && hc > 0 && wc_img > 0 && (int64_t)hc * wc_img < ((int64_t)1 << 31) && (nframes == 0 || rgb);
}
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }     // a host color needs none: its staging copy has it

int f3d_tsdf_integrate_color_dev(f3d_ctx* ctx, float* tsdf, float* weight, float* color, int nx, int ny, int nz, const double lo[3], double vs,
                                 double trunc, float max_weight, const void* depth, int depth_type, const uint8_t* rgb, int nframes, int h, int w,
                                 int hc, int wc_img, double depth_scale, double max_depth, const f3d_view* views_dev, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!tsdf_integrate_ok(tsdf, weight, nx, ny, nz, lo, vs, trunc, max_weight, depth, depth_type, nframes, h, w, depth_scale, max_depth, views_dev) ||
        !tsdf_color_ok(color, rgb, nframes, hc, wc_img) || !aligned16(color))
        return fail(ctx, F3D_ERR_INVALID, "tsdf_integrate_color: " F3D_TSDF_COLOR_BAD);
    if (nframes == 0) return F3D_OK;
    F3D_HIP(ctx, f3d_launch_tsdf_integrate_color(tsdf, weight, color, nx, ny, nz, lo, vs, trunc, (double)max_weight, depth, depth_type, rgb, nframes, h, w,
                                                 hc, wc_img, depth_scale, max_depth, views_dev, ctx->tsdf_grid_cap, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_tsdf_integrate_color(f3d_ctx* ctx, float* tsdf, float* weight, float* color, int nx, int ny, int nz, const double lo[3], double vs,
                             double trunc, float max_weight, const void* depth, int depth_type, const uint8_t* rgb, int nframes, int h, int w, int hc,
                             int wc_img, double depth_scale, double max_depth, const f3d_view* views) {
    int rc = enter(ctx); if (rc) return rc;
    if (!tsdf_integrate_ok(tsdf, weight, nx, ny, nz, lo, vs, trunc, max_weight, depth, depth_type, nframes, h, w, depth_scale, max_depth, views) ||
        !tsdf_color_ok(color, rgb, nframes, hc, wc_img))
        return fail(ctx, F3D_ERR_INVALID, "tsdf_integrate_color: " F3D_TSDF_COLOR_BAD);
    if (nframes == 0) return F3D_OK;
    const size_t vol = (size_t)tsdf_voxels(nx, ny, nz) * 4;
    staging st(ctx);
    float* dt = st.inout(tsdf, vol);
    float* dw = st.inout(weight, vol);
    float* dc = st.inout(color, 4 * vol);
    const void* dd = st.in((const char*)depth, depth_bytes(depth_type, nframes, h, w));
    const uint8_t* drgb = st.in(rgb, (size_t)nframes * hc * wc_img * 3);
    const f3d_view* dviews = st.in(views, sizeof(f3d_view) * (size_t)nframes);
    if (!st.rc) st.rc = f3d_tsdf_integrate_color_dev(ctx, dt, dw, dc, nx, ny, nz, lo, vs, trunc, max_weight, dd, depth_type, drgb, nframes, h, w, hc, wc_img,
                                                     depth_scale, max_depth, dviews, ctx->stream);
    return st.finish();
}

int f3d_tsdf_extract_colors_dev(f3d_ctx* ctx, const float* tsdf, const float* color, int nx, int ny, int nz, uint8_t* rgb, uint8_t* colored,
                                void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!tsdf_counted(ctx, nx, ny, nz)) return fail(ctx, F3D_ERR_INVALID, "tsdf_extract_colors: call f3d_tsdf_extract_count for this volume first");
    if (!tsdf || !color || !aligned16(color) || !rgb)
        return fail(ctx, F3D_ERR_INVALID, "tsdf_extract_colors: bad arguments (tsdf, color and rgb not NULL, color 16-byte aligned)");
    if (ctx->tsdf_nv == 0) return F3D_OK;
    F3D_HIP(ctx, f3d_launch_tsdf_vert_colors(tsdf, color, nx, ny, nz, ctx->scratch[SLOT_TSDF].p, rgb, colored, ctx->tsdf_grid_cap, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_tsdf_extract_colors(f3d_ctx* ctx, const float* color, int nx, int ny, int nz, uint8_t* rgb, uint8_t* colored) {
    int rc = enter(ctx); if (rc) return rc;
    if (!tsdf_counted(ctx, nx, ny, nz) || !ctx->tsdf_kept)
        return fail(ctx, F3D_ERR_INVALID, "tsdf_extract_colors: call f3d_tsdf_extract_count for this volume first");
    if (!color || !rgb) return fail(ctx, F3D_ERR_INVALID, "tsdf_extract_colors: bad arguments (color and rgb not NULL)");
    if (ctx->tsdf_nv == 0) return F3D_OK;
    staging st(ctx);
    const float* dc = st.in(color, (size_t)ctx->tsdf_n * 16);
    uint8_t* drgb = st.out(rgb, (size_t)ctx->tsdf_nv * 3);
    uint8_t* dcol = st.out(colored, (size_t)ctx->tsdf_nv);
    if (!st.rc) st.rc = f3d_tsdf_extract_colors_dev(ctx, (const float*)ctx->kept[KEPT_TSDF].p, dc, nx, ny, nz, drgb, dcol, ctx->stream);
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// registration: TSDF raycast and point-to-plane ICP (f3d_icp.hip; the contract is in include/f3d.h)
// ---------------------------------------------------------------------------------------------
static bool all_finite(const double* v, int n) {
    for (int k = 0; k < n; ++k) if (!(fabs(v[k]) < INFINITY)) return false;
    return true;
}

// qn = q / |q| by component division; false for a zero or non-finite quaternion
static bool unit_quat(const double q[4], double qn[4]) {
    if (!all_finite(q, 4)) return false;
    const double len = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    if (!(len > 0.0 && len < INFINITY)) return false;
    for (int k = 0; k < 4; ++k) qn[k] = q[k] / len;
    return true;
}

static bool image_ok(int h, int w) { return h > 0 && w > 0 && (int64_t)h * w < ((int64_t)1 << 31); }

#define F3D_RAYCAST_BAD "bad arguments (dims >= 1 with a product < 2^31; vs and step finite and > 0; min_weight >= 1; znear >= 0; nsteps >= 1; h * w in [1, 2^31); finite lo, K and t; a finite non-zero quaternion)"
static bool raycast_ok(const float* tsdf, const float* weight, int nx, int ny, int nz, const double* lo, double vs, float min_weight, const double* K,
                       const double* q, const double* t, int h, int w, double znear, double step, int nsteps, double qn[4]) {
    return tsdf && weight && lo && K && q && t && tsdf_voxels(nx, ny, nz) > 0 && pos_finite(vs) && min_weight >= 1.0f && image_ok(h, w) &&
           znear >= 0.0 && znear < INFINITY && pos_finite(step) && nsteps >= 1 && all_finite(lo, 3) && all_finite(K, 9) && all_finite(t, 3) &&
           unit_quat(q, qn);
}

int f3d_tsdf_raycast_dev(f3d_ctx* ctx, const float* tsdf, const float* weight, int nx, int ny, int nz, const double lo[3], double vs, float min_weight,
                         const double K[9], const double q_wxyz[4], const double t[3], int h, int w, double znear, double step, int nsteps,
                         double* vertex, double* normal, double* depth, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    double qn[4];
    if (!raycast_ok(tsdf, weight, nx, ny, nz, lo, vs, min_weight, K, q_wxyz, t, h, w, znear, step, nsteps, qn))
        return fail(ctx, F3D_ERR_INVALID, "tsdf_raycast: " F3D_RAYCAST_BAD);
    if (!vertex && !normal && !depth) return F3D_OK;
    F3D_HIP(ctx, f3d_launch_tsdf_raycast(tsdf, weight, nx, ny, nz, lo, vs, min_weight, K, qn, t, h, w, znear, step, nsteps, vertex, normal, depth,
                                         ctx->tsdf_grid_cap, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_tsdf_raycast(f3d_ctx* ctx, const float* tsdf, const float* weight, int nx, int ny, int nz, const double lo[3], double vs, float min_weight,
                     const double K[9], const double q_wxyz[4], const double t[3], int h, int w, double znear, double step, int nsteps,
                     double* vertex, double* normal, double* depth) {
    int rc = enter(ctx); if (rc) return rc;
    double qn[4];
    if (!raycast_ok(tsdf, weight, nx, ny, nz, lo, vs, min_weight, K, q_wxyz, t, h, w, znear, step, nsteps, qn))
        return fail(ctx, F3D_ERR_INVALID, "tsdf_raycast: " F3D_RAYCAST_BAD);
    const size_t vol = (size_t)tsdf_voxels(nx, ny, nz) * 4, px = (size_t)h * w * 8;
    staging st(ctx);
    const float* dt = st.in(tsdf, vol);
    const float* dw = st.in(weight, vol);
    double* dv = st.out(vertex, 3 * px);
    double* dn = st.out(normal, 3 * px);
    double* dd = st.out(depth, px);
    if (!st.rc) st.rc = f3d_tsdf_raycast_dev(ctx, dt, dw, nx, ny, nz, lo, vs, min_weight, K, q_wxyz, t, h, w, znear, step, nsteps, dv, dn, dd, ctx->stream);
    return st.finish();
}

#define F3D_ICP_BAD "bad arguments (h * w and hm * wm in [1, 2^31); depth_scale, max_depth and max_dist finite and > 0; a known depth type; finite K and t; a finite non-zero quaternion)"
static bool icp_ok(const void* depth, int depth_type, int h, int w, const double* K, double depth_scale, double max_depth, const double* q,
                   const double* t, const double* mv, const double* mn, int hm, int wm, const f3d_view* view, double max_dist) {
    double qn[4];
    return depth && K && q && t && mv && mn && view && image_ok(h, w) && image_ok(hm, wm) && pos_finite(depth_scale) && pos_finite(max_depth) &&
           pos_finite(max_dist) && (depth_type == F3D_DEPTH_U16 || depth_type == F3D_DEPTH_F32 || depth_type == F3D_DEPTH_F64) &&
           all_finite(K, 9) && all_finite(t, 3) && unit_quat(q, qn);
}

static f3d_icp_args icp_args(const void* depth, int depth_type, int h, int w, const double* K, double depth_scale, double max_depth, const double* mv,
                             const double* mn, int hm, int wm, const f3d_view* view, double max_dist) {
    f3d_icp_args a;
    a.depth = depth; a.depth_type = depth_type; a.h = h; a.w = w; a.K = K; a.depth_scale = depth_scale; a.max_depth = max_depth;
    a.model_vertex = mv; a.model_normal = mn; a.hm = hm; a.wm = wm; a.model_view = view; a.max_dist = max_dist;
    return a;
}

int f3d_ctx_reserve_icp(f3d_ctx* ctx, int64_t npixels) {
    int rc = enter(ctx); if (rc) return rc;
    if (npixels < 0 || npixels >= ((int64_t)1 << 31)) return fail(ctx, F3D_ERR_INVALID, "ctx_reserve_icp: npixels must be in [0, 2^31)");
    return reserve(ctx, {{SLOT_ICP, f3d_icp_scratch_bytes(npixels)}});
}

int f3d_icp_sums_dev(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9], double depth_scale, double max_depth,
                     const double q_wxyz[4], const double t[3], const double* model_vertex, const double* model_normal, int hm, int wm,
                     const f3d_view* model_view, double max_dist, double* sums, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!sums || !icp_ok(depth, depth_type, h, w, K, depth_scale, max_depth, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view, max_dist))
        return fail(ctx, F3D_ERR_INVALID, "icp_sums: " F3D_ICP_BAD);
    void* scratch;
    if ((rc = ensure(ctx, SLOT_ICP, f3d_icp_scratch_bytes((int64_t)h * w), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_icp_sums(icp_args(depth, depth_type, h, w, K, depth_scale, max_depth, model_vertex, model_normal, hm, wm, model_view, max_dist),
                                     q_wxyz, t, scratch, sums, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_icp_sums(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9], double depth_scale, double max_depth,
                 const double q_wxyz[4], const double t[3], const double* model_vertex, const double* model_normal, int hm, int wm,
                 const f3d_view* model_view, double max_dist, double* sums) {
    int rc = enter(ctx); if (rc) return rc;
    if (!sums || !icp_ok(depth, depth_type, h, w, K, depth_scale, max_depth, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view, max_dist))
        return fail(ctx, F3D_ERR_INVALID, "icp_sums: " F3D_ICP_BAD);
    staging st(ctx);
    const void* dd = st.in((const char*)depth, depth_bytes(depth_type, 1, h, w));
    const double* dv = st.in(model_vertex, (size_t)hm * wm * 24);
    const double* dn = st.in(model_normal, (size_t)hm * wm * 24);
    const f3d_view* dview = st.in(model_view, sizeof(f3d_view));
    double* ds = st.out(sums, F3D_ICP_NSUMS * sizeof(double));
    if (!st.rc) st.rc = f3d_icp_sums_dev(ctx, dd, depth_type, h, w, K, depth_scale, max_depth, q_wxyz, t, dv, dn, hm, wm, dview, max_dist, ds, ctx->stream);
    return st.finish();
}

int f3d_icp_dev(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9], double depth_scale, double max_depth,
                const double q_wxyz[4], const double t[3], const double* model_vertex, const double* model_normal, int hm, int wm,
                const f3d_view* model_view, double max_dist, int iterations, int min_pairs, double* pose, double* stats, int32_t* status,
                void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!pose || !stats || !icp_ok(depth, depth_type, h, w, K, depth_scale, max_depth, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view, max_dist))
        return fail(ctx, F3D_ERR_INVALID, "icp: " F3D_ICP_BAD);
    if (iterations < 1 || min_pairs < 6) return fail(ctx, F3D_ERR_INVALID, "icp: iterations must be at least 1 and min_pairs at least 6");
    void* scratch;
    if ((rc = ensure(ctx, SLOT_ICP, f3d_icp_scratch_bytes((int64_t)h * w), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_icp(icp_args(depth, depth_type, h, w, K, depth_scale, max_depth, model_vertex, model_normal, hm, wm, model_view, max_dist),
                                q_wxyz, t, iterations, min_pairs, scratch, pose, stats, status, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_icp(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9], double depth_scale, double max_depth,
            const double q_wxyz[4], const double t[3], const double* model_vertex, const double* model_normal, int hm, int wm,
            const f3d_view* model_view, double max_dist, int iterations, int min_pairs, double* pose, double* stats, int32_t* status) {
    int rc = enter(ctx); if (rc) return rc;
    if (!pose || !stats || !status ||
        !icp_ok(depth, depth_type, h, w, K, depth_scale, max_depth, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view, max_dist))
        return fail(ctx, F3D_ERR_INVALID, "icp: " F3D_ICP_BAD);
    if (iterations < 1 || min_pairs < 6) return fail(ctx, F3D_ERR_INVALID, "icp: iterations must be at least 1 and min_pairs at least 6");
    staging st(ctx);
    const void* dd = st.in((const char*)depth, depth_bytes(depth_type, 1, h, w));
    const double* dv = st.in(model_vertex, (size_t)hm * wm * 24);
    const double* dn = st.in(model_normal, (size_t)hm * wm * 24);
    const f3d_view* dview = st.in(model_view, sizeof(f3d_view));
    double* dp = st.out(pose, 7 * sizeof(double));
    double* ds = st.out(stats, (size_t)iterations * 3 * sizeof(double));
    int32_t* dst = st.out(status, sizeof(int32_t));
    if (!st.rc) st.rc = f3d_icp_dev(ctx, dd, depth_type, h, w, K, depth_scale, max_depth, q_wxyz, t, dv, dn, hm, wm, dview, max_dist, iterations, min_pairs,
                                    dp, ds, dst, ctx->stream);
    return st.finish();
}

// colour: the raycast arguments plus the colour state and two more outputs; the ICP arguments plus the model's intensity map, the
// source colour image and the weight of the photometric system
#define F3D_RAYCAST_COLOR_BAD F3D_RAYCAST_BAD "; color not NULL, the device color 16-byte aligned"
int f3d_tsdf_raycast_color_dev(f3d_ctx* ctx, const float* tsdf, const float* weight, const float* color, int nx, int ny, int nz, const double lo[3],
                               double vs, float min_weight, const double K[9], const double q_wxyz[4], const double t[3], int h, int w, double znear,
                               double step, int nsteps, double* vertex, double* normal, double* depth, double* rgb, double* intensity, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    double qn[4];
    if (!raycast_ok(tsdf, weight, nx, ny, nz, lo, vs, min_weight, K, q_wxyz, t, h, w, znear, step, nsteps, qn) || !color || !aligned16(color))
        return fail(ctx, F3D_ERR_INVALID, "tsdf_raycast_color: " F3D_RAYCAST_COLOR_BAD);
    if (!vertex && !normal && !depth && !rgb && !intensity) return F3D_OK;
    F3D_HIP(ctx, f3d_launch_tsdf_raycast_color(tsdf, weight, color, nx, ny, nz, lo, vs, min_weight, K, qn, t, h, w, znear, step, nsteps, vertex, normal,
                                               depth, rgb, intensity, ctx->tsdf_grid_cap, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_tsdf_raycast_color(f3d_ctx* ctx, const float* tsdf, const float* weight, const float* color, int nx, int ny, int nz, const double lo[3],
                           double vs, float min_weight, const double K[9], const double q_wxyz[4], const double t[3], int h, int w, double znear,
                           double step, int nsteps, double* vertex, double* normal, double* depth, double* rgb, double* intensity) {
    int rc = enter(ctx); if (rc) return rc;
    double qn[4];
    if (!raycast_ok(tsdf, weight, nx, ny, nz, lo, vs, min_weight, K, q_wxyz, t, h, w, znear, step, nsteps, qn) || !color)
        return fail(ctx, F3D_ERR_INVALID, "tsdf_raycast_color: " F3D_RAYCAST_COLOR_BAD);
    const size_t vol = (size_t)tsdf_voxels(nx, ny, nz) * 4, px = (size_t)h * w * 8;
    staging st(ctx);
    const float* dt = st.in(tsdf, vol);
    const float* dw = st.in(weight, vol);
    const float* dc = st.in(color, 4 * vol);
    double* dv = st.out(vertex, 3 * px);
    double* dn = st.out(normal, 3 * px);
    double* dd = st.out(depth, px);
    double* drgb = st.out(rgb, 3 * px);
    double* di = st.out(intensity, px);
    if (!st.rc) st.rc = f3d_tsdf_raycast_color_dev(ctx, dt, dw, dc, nx, ny, nz, lo, vs, min_weight, K, q_wxyz, t, h, w, znear, step, nsteps, dv, dn, dd,
                                                   drgb, di, ctx->stream);
    return st.finish();
}

#define F3D_ICP_COLOR_BAD F3D_ICP_BAD "; model_intensity and rgb not NULL; hc, wc_img > 0 with a product < 2^31; color_weight finite and >= 0"
static bool icp_color_ok(const double* model_intensity, const uint8_t* rgb, int hc, int wc_img, double color_weight) {
    return model_intensity && rgb && image_ok(hc, wc_img) && color_weight >= 0.0 && color_weight < INFINITY;
}

static f3d_icp_color_args icp_color_args(const double* model_intensity, const uint8_t* rgb, int hc, int wc_img, double color_weight) {
    f3d_icp_color_args c;
    c.model_intensity = model_intensity; c.rgb = rgb; c.hc = hc; c.wc_img = wc_img; c.color_weight = color_weight;
    return c;
}

int f3d_ctx_reserve_icp_color(f3d_ctx* ctx, int64_t npixels) {
    int rc = enter(ctx); if (rc) return rc;
    if (npixels < 0 || npixels >= ((int64_t)1 << 31)) return fail(ctx, F3D_ERR_INVALID, "ctx_reserve_icp_color: npixels must be in [0, 2^31)");
    return reserve(ctx, {{SLOT_ICP, f3d_icp_color_scratch_bytes(npixels)}});
}

int f3d_icp_color_sums_dev(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9], double depth_scale, double max_depth,
                           const double q_wxyz[4], const double t[3], const double* model_vertex, const double* model_normal, int hm, int wm,
                           const f3d_view* model_view, double max_dist, const double* model_intensity, const uint8_t* rgb, int hc, int wc_img,
                           double color_weight, double* sums, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!sums || !icp_ok(depth, depth_type, h, w, K, depth_scale, max_depth, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view, max_dist) ||
        !icp_color_ok(model_intensity, rgb, hc, wc_img, color_weight))
        return fail(ctx, F3D_ERR_INVALID, "icp_color_sums: " F3D_ICP_COLOR_BAD);
    void* scratch;
    if ((rc = ensure(ctx, SLOT_ICP, f3d_icp_color_scratch_bytes((int64_t)h * w), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_icp_color_sums(icp_args(depth, depth_type, h, w, K, depth_scale, max_depth, model_vertex, model_normal, hm, wm, model_view,
                                                    max_dist),
                                           icp_color_args(model_intensity, rgb, hc, wc_img, color_weight), q_wxyz, t, scratch, sums, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_icp_color_sums(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9], double depth_scale, double max_depth,
                       const double q_wxyz[4], const double t[3], const double* model_vertex, const double* model_normal, int hm, int wm,
                       const f3d_view* model_view, double max_dist, const double* model_intensity, const uint8_t* rgb, int hc, int wc_img,
                       double color_weight, double* sums) {
    int rc = enter(ctx); if (rc) return rc;
    if (!sums || !icp_ok(depth, depth_type, h, w, K, depth_scale, max_depth, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view, max_dist) ||
        !icp_color_ok(model_intensity, rgb, hc, wc_img, color_weight))
        return fail(ctx, F3D_ERR_INVALID, "icp_color_sums: " F3D_ICP_COLOR_BAD);
    staging st(ctx);
    const void* dd = st.in((const char*)depth, depth_bytes(depth_type, 1, h, w));
    const double* dv = st.in(model_vertex, (size_t)hm * wm * 24);
    const double* dn = st.in(model_normal, (size_t)hm * wm * 24);
    const f3d_view* dview = st.in(model_view, sizeof(f3d_view));
    const double* di = st.in(model_intensity, (size_t)hm * wm * 8);
    const uint8_t* drgb = st.in(rgb, (size_t)hc * wc_img * 3);
    double* ds = st.out(sums, F3D_ICP_NSUMS_COLOR * sizeof(double));
    if (!st.rc) st.rc = f3d_icp_color_sums_dev(ctx, dd, depth_type, h, w, K, depth_scale, max_depth, q_wxyz, t, dv, dn, hm, wm, dview, max_dist, di, drgb,
                                               hc, wc_img, color_weight, ds, ctx->stream);
    return st.finish();
}

int f3d_icp_color_dev(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9], double depth_scale, double max_depth,
                      const double q_wxyz[4], const double t[3], const double* model_vertex, const double* model_normal, int hm, int wm,
                      const f3d_view* model_view, double max_dist, const double* model_intensity, const uint8_t* rgb, int hc, int wc_img,
                      double color_weight, int iterations, int min_pairs, double* pose, double* stats, int32_t* status, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!pose || !stats || !icp_ok(depth, depth_type, h, w, K, depth_scale, max_depth, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view, max_dist) ||
        !icp_color_ok(model_intensity, rgb, hc, wc_img, color_weight))
        return fail(ctx, F3D_ERR_INVALID, "icp_color: " F3D_ICP_COLOR_BAD);
    if (iterations < 1 || min_pairs < 6) return fail(ctx, F3D_ERR_INVALID, "icp_color: iterations must be at least 1 and min_pairs at least 6");
    void* scratch;
    if ((rc = ensure(ctx, SLOT_ICP, f3d_icp_color_scratch_bytes((int64_t)h * w), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_icp_color(icp_args(depth, depth_type, h, w, K, depth_scale, max_depth, model_vertex, model_normal, hm, wm, model_view, max_dist),
                                      icp_color_args(model_intensity, rgb, hc, wc_img, color_weight), q_wxyz, t, iterations, min_pairs, scratch, pose,
                                      stats, status, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_icp_color(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, const double K[9], double depth_scale, double max_depth,
                  const double q_wxyz[4], const double t[3], const double* model_vertex, const double* model_normal, int hm, int wm,
                  const f3d_view* model_view, double max_dist, const double* model_intensity, const uint8_t* rgb, int hc, int wc_img,
                  double color_weight, int iterations, int min_pairs, double* pose, double* stats, int32_t* status) {
    int rc = enter(ctx); if (rc) return rc;
    if (!pose || !stats || !status ||
        !icp_ok(depth, depth_type, h, w, K, depth_scale, max_depth, q_wxyz, t, model_vertex, model_normal, hm, wm, model_view, max_dist) ||
        !icp_color_ok(model_intensity, rgb, hc, wc_img, color_weight))
        return fail(ctx, F3D_ERR_INVALID, "icp_color: " F3D_ICP_COLOR_BAD);
    if (iterations < 1 || min_pairs < 6) return fail(ctx, F3D_ERR_INVALID, "icp_color: iterations must be at least 1 and min_pairs at least 6");
    staging st(ctx);
    const void* dd = st.in((const char*)depth, depth_bytes(depth_type, 1, h, w));
    const double* dv = st.in(model_vertex, (size_t)hm * wm * 24);
    const double* dn = st.in(model_normal, (size_t)hm * wm * 24);
    const f3d_view* dview = st.in(model_view, sizeof(f3d_view));
    const double* di = st.in(model_intensity, (size_t)hm * wm * 8);
    const uint8_t* drgb = st.in(rgb, (size_t)hc * wc_img * 3);
    double* dp = st.out(pose, 7 * sizeof(double));
    double* ds = st.out(stats, (size_t)iterations * 5 * sizeof(double));
    int32_t* dst = st.out(status, sizeof(int32_t));
    if (!st.rc) st.rc = f3d_icp_color_dev(ctx, dd, depth_type, h, w, K, depth_scale, max_depth, q_wxyz, t, dv, dn, hm, wm, dview, max_dist, di, drgb, hc,
                                          wc_img, color_weight, iterations, min_pairs, dp, ds, dst, ctx->stream);
    return st.finish();
}

// coarse-to-fine: one pyramid step of a depth frame and of model maps, and the rounds over a list of levels
#define F3D_DEPTH_HALF_BAD "bad arguments (h, w >= 2 with h * w < 2^31; depth_scale, max_depth and gate finite and > 0; a known depth type)"
static bool depth_half_ok(const void* depth, int depth_type, int h, int w, double depth_scale, double max_depth, double gate, const double* out) {
    return depth && out && h >= 2 && w >= 2 && image_ok(h, w) && pos_finite(depth_scale) && pos_finite(max_depth) && pos_finite(gate) &&
           (depth_type == F3D_DEPTH_U16 || depth_type == F3D_DEPTH_F32 || depth_type == F3D_DEPTH_F64);
}

int f3d_depth_half_dev(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, double depth_scale, double max_depth, double gate, double* out,
                       void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!depth_half_ok(depth, depth_type, h, w, depth_scale, max_depth, gate, out)) return fail(ctx, F3D_ERR_INVALID, "depth_half: " F3D_DEPTH_HALF_BAD);
    F3D_HIP(ctx, f3d_launch_depth_half(depth, depth_type, h, w, depth_scale, max_depth, gate, out, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_depth_half(f3d_ctx* ctx, const void* depth, int depth_type, int h, int w, double depth_scale, double max_depth, double gate, double* out) {
    int rc = enter(ctx); if (rc) return rc;
    if (!depth_half_ok(depth, depth_type, h, w, depth_scale, max_depth, gate, out)) return fail(ctx, F3D_ERR_INVALID, "depth_half: " F3D_DEPTH_HALF_BAD);
    staging st(ctx);
    const void* dd = st.in((const char*)depth, depth_bytes(depth_type, 1, h, w));
    double* dout = st.out(out, (size_t)(h / 2) * (w / 2) * sizeof(double));
    if (!st.rc) st.rc = f3d_depth_half_dev(ctx, dd, depth_type, h, w, depth_scale, max_depth, gate, dout, ctx->stream);
    return st.finish();
}

#define F3D_MAPS_HALF_BAD "bad arguments (hm, wm >= 2 with hm * wm < 2^31; gate finite and > 0; intensity_out given iff model_intensity is)"
static bool maps_half_ok(const double* mv, const double* mn, const double* mi, int hm, int wm, const f3d_view* view, double gate, const double* vo,
                         const double* no, const double* io) {
    return mv && mn && view && vo && no && !mi == !io && hm >= 2 && wm >= 2 && image_ok(hm, wm) && pos_finite(gate);
}

int f3d_maps_half_dev(f3d_ctx* ctx, const double* model_vertex, const double* model_normal, const double* model_intensity, int hm, int wm,
                      const f3d_view* model_view, double gate, double* vertex_out, double* normal_out, double* intensity_out, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!maps_half_ok(model_vertex, model_normal, model_intensity, hm, wm, model_view, gate, vertex_out, normal_out, intensity_out))
        return fail(ctx, F3D_ERR_INVALID, "maps_half: " F3D_MAPS_HALF_BAD);
    F3D_HIP(ctx, f3d_launch_maps_half(model_vertex, model_normal, model_intensity, hm, wm, model_view, gate, vertex_out, normal_out, intensity_out,
                                      pick(ctx, stream)));
    return F3D_OK;
}

int f3d_maps_half(f3d_ctx* ctx, const double* model_vertex, const double* model_normal, const double* model_intensity, int hm, int wm,
                  const f3d_view* model_view, double gate, double* vertex_out, double* normal_out, double* intensity_out) {
    int rc = enter(ctx); if (rc) return rc;
    if (!maps_half_ok(model_vertex, model_normal, model_intensity, hm, wm, model_view, gate, vertex_out, normal_out, intensity_out))
        return fail(ctx, F3D_ERR_INVALID, "maps_half: " F3D_MAPS_HALF_BAD);
    const size_t px = (size_t)hm * wm * 8, px2 = (size_t)(hm / 2) * (wm / 2) * 8;
    staging st(ctx);
    const double* dv = st.in(model_vertex, 3 * px);
    const double* dn = st.in(model_normal, 3 * px);
    const double* di = model_intensity ? st.in(model_intensity, px) : nullptr;
    const f3d_view* dview = st.in(model_view, sizeof(f3d_view));
    double* dvo = st.out(vertex_out, 3 * px2);
    double* dno = st.out(normal_out, 3 * px2);
    double* dio = st.out(intensity_out, px2);
    if (!st.rc) st.rc = f3d_maps_half_dev(ctx, dv, dn, di, hm, wm, dview, gate, dvo, dno, dio, ctx->stream);
    return st.finish();
}

#define F3D_ICP_LEVELS_BAD "bad arguments (nlevels in [1, 6]; per level: " F3D_ICP_BAD ", iterations >= 1, min_pairs >= 6; model_intensity on every level and rgb, or on none and no rgb; with rgb: hc, wc_img > 0 with a product < 2^31, color_weight finite and >= 0)"
// the total of the levels' rounds, or -1 for a call the contract refuses
static int64_t icp_levels_rounds(const f3d_icp_level* lv, int nlevels, double max_depth, const double* q, const double* t, const uint8_t* rgb, int hc,
                                 int wc_img, double color_weight) {
    if (!lv || nlevels < 1 || nlevels > F3D_ICP_MAX_LEVELS) return -1;
    int64_t rounds = 0;
    for (int l = 0; l < nlevels; ++l) {
        if (!icp_ok(lv[l].depth, lv[l].depth_type, lv[l].h, lv[l].w, lv[l].K, lv[l].depth_scale, max_depth, q, t, lv[l].model_vertex, lv[l].model_normal,
                    lv[l].hm, lv[l].wm, lv[l].model_view, lv[l].max_dist) ||
            lv[l].iterations < 1 || lv[l].min_pairs < 6 || !lv[l].model_intensity != !rgb)
            return -1;
        rounds += lv[l].iterations;
    }
    if (rgb && !icp_color_ok(lv[0].model_intensity, rgb, hc, wc_img, color_weight)) return -1;
    return rounds;
}

static int64_t icp_levels_pixels(const f3d_icp_level* lv, int nlevels) {
    int64_t most = 0;
    for (int l = 0; l < nlevels; ++l) {
        const int64_t npix = (int64_t)lv[l].h * lv[l].w;
        if (npix > most) most = npix;
    }
    return most;
}

int f3d_icp_levels_dev(f3d_ctx* ctx, const f3d_icp_level* levels, int nlevels, double max_depth, const double q_wxyz[4], const double t[3],
                       const uint8_t* rgb, int hc, int wc_img, double color_weight, double* pose, double* stats, int32_t* status, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!pose || !stats || icp_levels_rounds(levels, nlevels, max_depth, q_wxyz, t, rgb, hc, wc_img, color_weight) < 0)
        return fail(ctx, F3D_ERR_INVALID, "icp_levels: " F3D_ICP_LEVELS_BAD);
    const int64_t most = icp_levels_pixels(levels, nlevels);
    void* scratch;
    if ((rc = ensure(ctx, SLOT_ICP, rgb ? f3d_icp_color_scratch_bytes(most) : f3d_icp_scratch_bytes(most), &scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_icp_levels(levels, nlevels, max_depth, q_wxyz, t, rgb, hc, wc_img, color_weight, scratch, pose, stats, status,
                                       pick(ctx, stream)));
    return F3D_OK;
}

// The host entry stages every input of every level in one buffer (a call may hold 6 levels of five arrays each, more than the
// staging buffers a call has): each piece starts on a 256-byte boundary of it.
int f3d_icp_levels(f3d_ctx* ctx, const f3d_icp_level* levels, int nlevels, double max_depth, const double q_wxyz[4], const double t[3],
                   const uint8_t* rgb, int hc, int wc_img, double color_weight, double* pose, double* stats, int32_t* status) {
    int rc = enter(ctx); if (rc) return rc;
    const int64_t rounds = icp_levels_rounds(levels, nlevels, max_depth, q_wxyz, t, rgb, hc, wc_img, color_weight);
    if (!pose || !stats || !status || rounds < 0) return fail(ctx, F3D_ERR_INVALID, "icp_levels: " F3D_ICP_LEVELS_BAD);
    struct piece { size_t depth, vertex, normal, intensity, view; } at[F3D_ICP_MAX_LEVELS];
    f3d_carve c;
    for (int l = 0; l < nlevels; ++l) {
        const f3d_icp_level& lv = levels[l];
        const size_t px = (size_t)lv.hm * lv.wm * 8;
        at[l].depth = c.take(depth_bytes(lv.depth_type, 1, lv.h, lv.w));
        at[l].vertex = c.take(3 * px);
        at[l].normal = c.take(3 * px);
        at[l].intensity = c.take(rgb ? px : 0);
        at[l].view = c.take(sizeof(f3d_view));
    }
    const size_t rgb_at = c.take(rgb ? (size_t)hc * wc_img * 3 : 0);
    staging st(ctx);
    char* in = (char*)st.slot(c.off);
    f3d_icp_level dev[F3D_ICP_MAX_LEVELS];
    for (int l = 0; l < nlevels && !st.rc; ++l) {
        const f3d_icp_level& lv = levels[l];
        const size_t px = (size_t)lv.hm * lv.wm * 8;
        dev[l] = lv;
        st.put(in + at[l].depth, lv.depth, depth_bytes(lv.depth_type, 1, lv.h, lv.w));
        st.put(in + at[l].vertex, lv.model_vertex, 3 * px);
        st.put(in + at[l].normal, lv.model_normal, 3 * px);
        if (rgb) st.put(in + at[l].intensity, lv.model_intensity, px);
        st.put(in + at[l].view, lv.model_view, sizeof(f3d_view));
        dev[l].depth = in + at[l].depth;
        dev[l].model_vertex = (const double*)(in + at[l].vertex);
        dev[l].model_normal = (const double*)(in + at[l].normal);
        dev[l].model_intensity = rgb ? (const double*)(in + at[l].intensity) : nullptr;
        dev[l].model_view = (const f3d_view*)(in + at[l].view);
    }
    if (rgb) st.put(in + rgb_at, rgb, (size_t)hc * wc_img * 3);
    double* dp = st.out(pose, 7 * sizeof(double));
    double* ds = st.out(stats, (size_t)rounds * (rgb ? 5 : 3) * sizeof(double));
    int32_t* dst = st.out(status, sizeof(int32_t));
    if (!st.rc) st.rc = f3d_icp_levels_dev(ctx, dev, nlevels, max_depth, q_wxyz, t, rgb ? (const uint8_t*)(in + rgb_at) : nullptr, hc, wc_img, color_weight,
                                           dp, ds, dst, ctx->stream);
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// cloud-to-cloud ICP: nearest-point search in the target's grid fused with the sums (f3d_icp.hip; contract in f3d.h)
// ---------------------------------------------------------------------------------------------
#define F3D_CLOUD_ICP_BAD "bad arguments (n, m < 2^31; float32 / float64 clouds; a known mode, normals in plane mode; max_dist finite, > 0 and < 1e300; a finite t; a finite non-zero quaternion)"
static bool cloud_icp_ok(const void* source, int sdtype, int64_t n, const void* target, int tdtype, int64_t m, const double* normals, int mode,
                         const double* q, const double* t, double max_dist) {
    double qn[4];
    return n >= 0 && n <= 0x7fffffffLL && m >= 0 && m <= 0x7fffffffLL && (n == 0 || source) && (m == 0 || target) && dtype_ok(sdtype) &&
           dtype_ok(tdtype) && (mode == F3D_CLOUD_ICP_POINT || (mode == F3D_CLOUD_ICP_PLANE && (normals || m == 0))) && q && t &&
           pos_finite(max_dist) && max_dist < 1e300 && all_finite(t, 3) && unit_quat(q, qn);
}

int f3d_ctx_reserve_cloud_icp(f3d_ctx* ctx, int64_t m, int64_t n) {
    int rc = enter(ctx); if (rc) return rc;
    if (m < 0 || m > 0x7fffffffLL || n < 0 || n > 0x7fffffffLL) return fail(ctx, F3D_ERR_INVALID, "ctx_reserve_cloud_icp: m and n must be in [0, 2^31)");
    return reserve(ctx, {{SLOT_GRAPH_BBOX, f3d_graph_bbox_bytes()}, {SLOT_KNN_FLAG, 64},
                         {SLOT_KNN, f3d_graph_scratch_bytes(m, GRID_MAX_CELLS)},                       // (any grid the radius allows)
                         {SLOT_ICP, f3d_icp_scratch_bytes(n)}});
}

// What the two _dev entries share after their argument checks: the one readback (the target's box and the source's non-finite flag
// together), the target's grid, built once in SLOT_KNN, and the round scratch in SLOT_ICP.
static int cloud_icp_prepare(f3d_ctx* ctx, const char* op, const void* source, f3d_dtype sdtype, int64_t n, const void* target, f3d_dtype tdtype,
                             int64_t m, const double* normals, int mode, double max_dist, hipStream_t s, f3d_cloud_icp_args* a, void** scratch) {
    if (m == 0) return fail(ctx, F3D_ERR_INVALID, "%s: the target is empty", op);
    void *dbox, *dflag, *grid;
    int rc = ensure(ctx, SLOT_GRAPH_BBOX, f3d_graph_bbox_bytes(), &dbox); if (rc) return rc;
    if ((rc = ensure(ctx, SLOT_KNN_FLAG, 64, &dflag))) return rc;
    unsigned flag = 0;
    F3D_HIP(ctx, hipMemsetAsync(dflag, 0, 4, s));
    if (n > 0) F3D_HIP(ctx, f3d_launch_knn_flag(source, sdtype, n, (unsigned*)dflag, s));
    F3D_HIP(ctx, hipMemcpyAsync(&flag, dflag, 4, hipMemcpyDeviceToHost, s));
    if ((rc = cloud_search(ctx, target, tdtype, m, max_dist, s, op, &a->gs))) return rc;               // (synchronises)
    if (flag) return fail(ctx, F3D_ERR_INVALID, "%s: the source contains NaN or infinity", op);
    if ((rc = ensure(ctx, SLOT_KNN, f3d_graph_scratch_bytes(m, f3d_ncells(a->gs.g)), &grid))) return rc;
    if ((rc = ensure(ctx, SLOT_ICP, f3d_icp_scratch_bytes(n), scratch))) return rc;
    F3D_HIP(ctx, f3d_launch_graph_grid(target, tdtype, m, a->gs.g, grid, &a->gv, s));
    a->source = source; a->source_dtype = sdtype; a->n = n; a->normals = normals; a->mode = mode;
    return F3D_OK;
}

int f3d_cloud_icp_sums_dev(f3d_ctx* ctx, const void* source, f3d_dtype source_dtype, int64_t n, const void* target, f3d_dtype target_dtype, int64_t m,
                           const double* target_normals, int mode, const double q_wxyz[4], const double t[3], double max_dist, double* sums,
                           int32_t* pairs, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!sums || !cloud_icp_ok(source, source_dtype, n, target, target_dtype, m, target_normals, mode, q_wxyz, t, max_dist))
        return fail(ctx, F3D_ERR_INVALID, "cloud_icp_sums: " F3D_CLOUD_ICP_BAD);
    hipStream_t s = pick(ctx, stream);
    f3d_cloud_icp_args a;
    void* scratch;
    if ((rc = cloud_icp_prepare(ctx, "cloud_icp_sums", source, source_dtype, n, target, target_dtype, m, target_normals, mode, max_dist, s, &a, &scratch)))
        return rc;
    F3D_HIP(ctx, f3d_launch_cloud_icp_sums(a, q_wxyz, t, scratch, sums, pairs, s));
    return F3D_OK;
}

int f3d_cloud_icp_dev(f3d_ctx* ctx, const void* source, f3d_dtype source_dtype, int64_t n, const void* target, f3d_dtype target_dtype, int64_t m,
                      const double* target_normals, int mode, const double q_wxyz[4], const double t[3], double max_dist, int iterations,
                      int min_pairs, double* pose, double* stats, int32_t* status, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!pose || !stats || !cloud_icp_ok(source, source_dtype, n, target, target_dtype, m, target_normals, mode, q_wxyz, t, max_dist))
        return fail(ctx, F3D_ERR_INVALID, "cloud_icp: " F3D_CLOUD_ICP_BAD);
    if (iterations < 1 || min_pairs < 6) return fail(ctx, F3D_ERR_INVALID, "cloud_icp: iterations must be at least 1 and min_pairs at least 6");
    hipStream_t s = pick(ctx, stream);
    f3d_cloud_icp_args a;
    void* scratch;
    if ((rc = cloud_icp_prepare(ctx, "cloud_icp", source, source_dtype, n, target, target_dtype, m, target_normals, mode, max_dist, s, &a, &scratch)))
        return rc;
    F3D_HIP(ctx, f3d_launch_cloud_icp(a, q_wxyz, t, iterations, min_pairs, scratch, pose, stats, status, s));
    return F3D_OK;
}

int f3d_cloud_icp_sums(f3d_ctx* ctx, const void* source, f3d_dtype source_dtype, int64_t n, const void* target, f3d_dtype target_dtype, int64_t m,
                       const double* target_normals, int mode, const double q_wxyz[4], const double t[3], double max_dist, double* sums,
                       int32_t* pairs) {
    int rc = enter(ctx); if (rc) return rc;
    if (!sums || !cloud_icp_ok(source, source_dtype, n, target, target_dtype, m, target_normals, mode, q_wxyz, t, max_dist))
        return fail(ctx, F3D_ERR_INVALID, "cloud_icp_sums: " F3D_CLOUD_ICP_BAD);
    staging st(ctx);
    const void* dsrc = st.in(source, xyz_bytes(source_dtype, n));
    const void* dtgt = st.in(target, xyz_bytes(target_dtype, m));
    const double* dnrm = mode == F3D_CLOUD_ICP_PLANE ? st.in(target_normals, (size_t)m * 24) : nullptr;
    double* ds = st.out(sums, F3D_ICP_NSUMS * sizeof(double));
    int32_t* dpr = st.out(pairs, (size_t)n * 4);
    if (!st.rc) st.rc = f3d_cloud_icp_sums_dev(ctx, dsrc, source_dtype, n, dtgt, target_dtype, m, dnrm, mode, q_wxyz, t, max_dist, ds, dpr, ctx->stream);
    return st.finish();
}

int f3d_cloud_icp(f3d_ctx* ctx, const void* source, f3d_dtype source_dtype, int64_t n, const void* target, f3d_dtype target_dtype, int64_t m,
                  const double* target_normals, int mode, const double q_wxyz[4], const double t[3], double max_dist, int iterations, int min_pairs,
                  double* pose, double* stats, int32_t* status) {
    int rc = enter(ctx); if (rc) return rc;
    if (!pose || !stats || !status || !cloud_icp_ok(source, source_dtype, n, target, target_dtype, m, target_normals, mode, q_wxyz, t, max_dist))
        return fail(ctx, F3D_ERR_INVALID, "cloud_icp: " F3D_CLOUD_ICP_BAD);
    if (iterations < 1 || min_pairs < 6) return fail(ctx, F3D_ERR_INVALID, "cloud_icp: iterations must be at least 1 and min_pairs at least 6");
    staging st(ctx);
    const void* dsrc = st.in(source, xyz_bytes(source_dtype, n));
    const void* dtgt = st.in(target, xyz_bytes(target_dtype, m));
    const double* dnrm = mode == F3D_CLOUD_ICP_PLANE ? st.in(target_normals, (size_t)m * 24) : nullptr;
    double* dp = st.out(pose, 7 * sizeof(double));
    double* ds = st.out(stats, (size_t)iterations * 3 * sizeof(double));
    int32_t* dst = st.out(status, sizeof(int32_t));
    if (!st.rc) st.rc = f3d_cloud_icp_dev(ctx, dsrc, source_dtype, n, dtgt, target_dtype, m, dnrm, mode, q_wxyz, t, max_dist, iterations, min_pairs, dp, ds,
                                          dst, ctx->stream);
    return st.finish();
}

// ---------------------------------------------------------------------------------------------
// feature fusion: per-point pooling of per-pixel feature maps over views (f3d_features.hip)
// ---------------------------------------------------------------------------------------------
#define F3D_FEAT_BAD F3D_RENDER_BAD ", hf, wf >= 1 with hf * wf < 2^31, d in [1, 4096], float16 / float32 features, depth_tol >= 0, views_per_pass >= 0"

static bool features_args_ok(const void* xyz, f3d_dtype dtype, int64_t n, const void* views, int nviews, int h, int w, const void* feats,
                             f3d_ftype ftype, int hf, int wf, int d, int splat, double depth_tol, const float* sums, const int32_t* counts,
                             int views_per_pass) {
    return render_args_ok(xyz, dtype, n, views, nviews, h, w, splat) && (ftype == F3D_FEAT_F16 || ftype == F3D_FEAT_F32) && hf >= 1 && wf >= 1 &&
           (int64_t)hf * wf <= 0x7fffffffLL && d >= 1 && d <= 4096 && depth_tol >= 0.0 && views_per_pass >= 0 &&
           (n == 0 || (sums && counts)) && (nviews == 0 || feats);
}

int f3d_fuse_features_dev(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views_dev, int nviews, int h, int w,
                          const void* feats, f3d_ftype ftype, int hf, int wf, int d, int splat, double depth_tol, float* sums, int32_t* counts,
                          int views_per_pass, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (!features_args_ok(xyz, dtype, n, views_dev, nviews, h, w, feats, ftype, hf, wf, d, splat, depth_tol, sums, counts, views_per_pass))
        return fail(ctx, F3D_ERR_INVALID, "fuse_features: " F3D_FEAT_BAD);
    if (n == 0 || nviews == 0) return F3D_OK;
    hipStream_t s = pick(ctx, stream);
    const size_t hw = (size_t)h * w, fbytes = (size_t)hf * wf * d * (ftype == F3D_FEAT_F16 ? 2 : 4);
    const bool occl = depth_tol < INFINITY;                                  // +inf: every sample is visible, no keys
    const int per = render_pass_views(nviews, h, w, views_per_pass);
    unsigned long long* zkey = nullptr;
    if (occl) {
        void* zk;
        if ((rc = ensure(ctx, SLOT_ZKEY, (size_t)per * hw * 8, &zk))) return rc;
        zkey = (unsigned long long*)zk;
    }
    for (int v0 = 0; v0 < nviews; v0 += per) {                               // a pass: render, then gather (sums in ascending view order)
        const int nv = nviews - v0 < per ? nviews - v0 : per;
        if (occl) {
            F3D_HIP(ctx, f3d_launch_zkey_fill(zkey, (size_t)nv * hw, s));
            F3D_HIP(ctx, f3d_launch_zsplat(xyz, dtype, n, views_dev + v0, nv, h, w, splat, zkey, nullptr, s));
        }
        F3D_HIP(ctx, f3d_launch_fuse_features(xyz, dtype, n, views_dev + v0, nv, h, w, (const char*)feats + (size_t)v0 * fbytes, ftype, hf, wf, d,
                                              zkey, depth_tol, sums, counts, s));
    }
    return F3D_OK;
}

int f3d_fuse_features(f3d_ctx* ctx, const void* xyz, f3d_dtype dtype, int64_t n, const f3d_view* views, int nviews, int h, int w,
                      const void* feats, f3d_ftype ftype, int hf, int wf, int d, int splat, double depth_tol, float* sums, int32_t* counts,
                      int views_per_pass) {
    int rc = enter(ctx); if (rc) return rc;
    if (!features_args_ok(xyz, dtype, n, views, nviews, h, w, feats, ftype, hf, wf, d, splat, depth_tol, sums, counts, views_per_pass))
        return fail(ctx, F3D_ERR_INVALID, "fuse_features: " F3D_FEAT_BAD);
    if (n == 0 || nviews == 0) return F3D_OK;
    staging st(ctx);
    const void* dxyz = st.in(xyz, xyz_bytes(dtype, n));
    const f3d_view* dviews = st.in(views, sizeof(f3d_view) * (size_t)nviews);
    const char* dfeats = st.in((const char*)feats, (size_t)nviews * hf * wf * d * (ftype == F3D_FEAT_F16 ? 2 : 4));
    float* dsums = st.inout(sums, (size_t)n * d * 4);
    int32_t* dcounts = st.inout(counts, (size_t)n * 4);
    if (!st.rc) st.rc = f3d_fuse_features_dev(ctx, dxyz, dtype, n, dviews, nviews, h, w, dfeats, ftype, hf, wf, d, splat, depth_tol, dsums, dcounts,
                                              views_per_pass, ctx->stream);
    return st.finish();
}

int f3d_features_finalize_dev(f3d_ctx* ctx, const float* sums, const int32_t* counts, int64_t n, int d, int normalize, float* out, void* stream) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || d < 1 || d > 4096 || (n > 0 && (!sums || !counts || !out)))
        return fail(ctx, F3D_ERR_INVALID, "features_finalize: bad arguments (n >= 0, d in [1, 4096])");
    if (n == 0) return F3D_OK;
    F3D_HIP(ctx, f3d_launch_features_finalize(sums, counts, n, d, normalize, out, pick(ctx, stream)));
    return F3D_OK;
}

int f3d_features_finalize(f3d_ctx* ctx, const float* sums, const int32_t* counts, int64_t n, int d, int normalize, float* out) {
    int rc = enter(ctx); if (rc) return rc;
    if (n < 0 || d < 1 || d > 4096 || (n > 0 && (!sums || !counts || !out)))
        return fail(ctx, F3D_ERR_INVALID, "features_finalize: bad arguments (n >= 0, d in [1, 4096])");
    if (n == 0) return F3D_OK;
    staging st(ctx);
    float* drows = st.in(sums, (size_t)n * d * 4);                           // finalised in place on the device copy
    const int32_t* dcounts = st.in(counts, (size_t)n * 4);
    st.back(out, drows, (size_t)n * d * 4);
    if (!st.rc) st.rc = f3d_features_finalize_dev(ctx, drows, dcounts, n, d, normalize, drows, ctx->stream);
    return st.finish();
}
