// door_window_bbox.generate_mesh (Fusion3DSeg/segUtils/door_window_bbox.py:65-150) on gfx950: every door / window instance is
// snapped to the mesh triangle its points lie on and replaced by a quad in that triangle's plane.
//
// The reference forms [M, T, 3] float64 temporaries per instance (M points x T triangles).  Here nothing of size M x T is stored:
//   k_quad_tri_setup : per triangle the Open3D normal, the vertex differences and the np.dot scalars of _point_in_triangle;
//   k_quad_rank_ids,
//   k_quad_slot_keys : point -> slot of its instance (or k), then f3d_launch_group_by_id lists every instance's members in
//                      ascending point index (box_pts = pts[ids == id]);
//   k_quad_tri_dist  : one thread per (instance, triangle) runs the sequential float64 sum of |perp| in point order, the
//                      instance's points staged through LDS in tiles (every lane reads the same point: broadcast);
//   k_quad_candidates: one wave per instance: the minimum (NaN -> no candidate), the band tri_dist < min + 0.05 * min and the
//                      candidates in triangle order;
//   k_quad_inside    : per (point, candidate) the projection and the _point_in_triangle test, counted with integer atomics;
//   k_quad_choose    : per instance the first maximum, the horizontal test and _get_perpendicular_vectors;
//   k_quad_extents   : per point the x / y coordinates in that basis, min / max through order-preserving integer atomics;
//   k_quad_build     : the quad corners.
// Arithmetic: -ffp-contract=off; every np.dot / np.linalg.norm of the reference is the fma chain fma(x2,y2, fma(x1,y1, x0*y0))
// (the BLAS kernel's order), every einsum is (a0b0 + a2b2) + a1b1, np.cross is plain multiply and subtract.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "f3d.h"
#include "f3d_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int QB = 256;
constexpr double COS10 = 0x1.f838b8c811c17p-1;          // np.cos(np.deg2rad(10)) (:85)
constexpr double ALLCLOSE_TOL = 0x1.4fe13ec9bf514p-17;  // np.allclose(x, 1.0): atol + rtol * 1.0 = 1e-08 + 1e-05 (:55)

struct tri_rec {                        // 128 bytes per triangle
    double t0[3];                       // triangle[0]
    double e0[3];                       // triangle[2] - triangle[0]  (the reference's v0, :36)
    double e1[3];                       // triangle[1] - triangle[0]  (v1, :37)
    double n[3];                        // Open3D triangle normal
    double d00, d01, d11, inv;          // np.dot(v0, v0), np.dot(v0, v1), np.dot(v1, v1), 1 / (d00 * d11 - d01 * d01)
};

struct inst_rec {                       // the chosen plane of an instance
    double origin[3], i[3], j[3];
    int tri, status;
};

__device__ __forceinline__ double blas_dot(double a0, double a1, double a2, double b0, double b1, double b2) {
    return fma(a2, b2, fma(a1, b1, a0 * b0));
}

// perp_dist[m, n] = einsum('mnc,nc->mn', box_pts - v0, normals) (:93-94)
__device__ __forceinline__ double perp_of(double px, double py, double pz, const tri_rec& r) {
    const double d0 = px - r.t0[0], d1 = py - r.t0[1], d2 = pz - r.t0[2];
    return (d0 * r.n[0] + d2 * r.n[2]) + d1 * r.n[1];
}

// projection onto the triangle's plane (:103-104) and _point_in_triangle (:26-47)
__device__ __forceinline__ bool inside_of(double px, double py, double pz, const tri_rec& r) {
    const double perp = perp_of(px, py, pz, r);
    const double qx = px - r.n[0] * perp, qy = py - r.n[1] * perp, qz = pz - r.n[2] * perp;
    const double v0 = qx - r.t0[0], v1 = qy - r.t0[1], v2 = qz - r.t0[2];
    const double d02 = (r.e0[0] * v0 + r.e0[2] * v2) + r.e0[1] * v1;
    const double d12 = (r.e1[0] * v0 + r.e1[2] * v2) + r.e1[1] * v1;
    const double u = (r.d11 * d02 - r.d01 * d12) * r.inv;
    const double v = (r.d00 * d12 - r.d01 * d02) * r.inv;
    return (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0);
}

__device__ __forceinline__ void load_pt(const double* __restrict__ pts, int64_t i, double& x, double& y, double& z) {
    x = pts[3 * i]; y = pts[3 * i + 1]; z = pts[3 * i + 2];
}

__global__ __launch_bounds__(QB) void k_quad_tri_setup(const double* __restrict__ verts, int64_t nv, const int64_t* __restrict__ tris,
                                                       int64_t nt, tri_rec* __restrict__ rec, double* __restrict__ normals, int* err) {
    for (int64_t t = (int64_t)blockIdx.x * QB + threadIdx.x; t < nt; t += (int64_t)gridDim.x * QB) {
        double v[3][3];
        bool bad = false;
        for (int c = 0; c < 3; ++c) {
            int64_t ix = tris[3 * t + c];
            if (ix < 0) ix += nv;                                   // NumPy indexing of vertices[triangles]
            if (ix < 0 || ix >= nv) { bad = true; v[c][0] = v[c][1] = v[c][2] = 0.0; continue; }
            v[c][0] = verts[3 * ix]; v[c][1] = verts[3 * ix + 1]; v[c][2] = verts[3 * ix + 2];
        }
        if (bad) atomicOr(err, F3D_DEVERR_QUADS);
        tri_rec r;
        // Open3D compute_triangle_normals: cross(v1 - v0, v2 - v0), normalised unless its squared norm is 0; a NaN -> (0, 0, 1)
        const double a0 = v[1][0] - v[0][0], a1 = v[1][1] - v[0][1], a2 = v[1][2] - v[0][2];
        const double b0 = v[2][0] - v[0][0], b1 = v[2][1] - v[0][1], b2 = v[2][2] - v[0][2];
        double n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
        const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
        if (nn > 0.0) {
            const double s = sqrt(nn);
            n0 = n0 / s; n1 = n1 / s; n2 = n2 / s;
        }
        if (isnan(n0)) { n0 = 0.0; n1 = 0.0; n2 = 1.0; }
        r.n[0] = n0; r.n[1] = n1; r.n[2] = n2;
        for (int c = 0; c < 3; ++c) {
            r.t0[c] = v[0][c];
            r.e0[c] = v[2][c] - v[0][c];
            r.e1[c] = v[1][c] - v[0][c];
        }
        r.d00 = blas_dot(r.e0[0], r.e0[1], r.e0[2], r.e0[0], r.e0[1], r.e0[2]);
        r.d01 = blas_dot(r.e0[0], r.e0[1], r.e0[2], r.e1[0], r.e1[1], r.e1[2]);
        r.d11 = blas_dot(r.e1[0], r.e1[1], r.e1[2], r.e1[0], r.e1[1], r.e1[2]);
        r.inv = 1.0 / (r.d00 * r.d11 - r.d01 * r.d01);
        rec[t] = r;
        if (normals) { normals[3 * t] = n0; normals[3 * t + 1] = n1; normals[3 * t + 2] = n2; }
    }
}

// rank of every wanted id in (id, position) order: sorted_ids / sorted_slot for the binary search of k_quad_slot_keys
__global__ __launch_bounds__(QB) void k_quad_rank_ids(const int64_t* __restrict__ inst, int k, int64_t* __restrict__ sorted_ids,
                                                      int32_t* __restrict__ sorted_slot) {
    for (int64_t e = (int64_t)blockIdx.x * QB + threadIdx.x; e < k; e += (int64_t)gridDim.x * QB) {
        const int64_t id = inst[e];
        int r = 0;
        for (int f = 0; f < k; ++f) {
            const int64_t g = inst[f];
            r += (g < id) | ((g == id) & (f < e));
        }
        sorted_ids[r] = id;
        sorted_slot[r] = (int32_t)e;
    }
}

// keys[i] = slot of ids[i] among the wanted ids (the first slot of a repeated id), k if none
__global__ __launch_bounds__(QB) void k_quad_slot_keys(const int64_t* __restrict__ ids, int64_t n, const int64_t* __restrict__ sorted_ids,
                                                       const int32_t* __restrict__ sorted_slot, int k, int64_t* __restrict__ keys) {
    for (int64_t i = (int64_t)blockIdx.x * QB + threadIdx.x; i < n; i += (int64_t)gridDim.x * QB) {
        const int64_t id = ids[i];
        int lo = 0, hi = k;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sorted_ids[mid] < id) lo = mid + 1; else hi = mid;
        }
        keys[i] = (lo < k && sorted_ids[lo] == id) ? (int64_t)sorted_slot[lo] : (int64_t)k;
    }
}

// tri_dist[s, t] = sum over the members m of instance s, in ascending point index, of |perp[m, t]| (:95): a sequential float64
// sum per thread.  Block = QB triangles of one instance (blockIdx.y); its members go through LDS QB at a time.
__global__ __launch_bounds__(QB) void k_quad_tri_dist(const double* __restrict__ pts, const int32_t* __restrict__ order,
                                                      const int64_t* __restrict__ starts, const tri_rec* __restrict__ rec, int64_t nt,
                                                      double* __restrict__ dist) {
    __shared__ double sp[QB][3];
    const int s = blockIdx.y;
    const int64_t t = (int64_t)blockIdx.x * QB + threadIdx.x;
    const int64_t b = starts[s], e = starts[s + 1];
    tri_rec r;
    const int64_t tt = t < nt ? t : nt - 1;                         // lanes past the end work on the last triangle, store nothing
    r.t0[0] = rec[tt].t0[0]; r.t0[1] = rec[tt].t0[1]; r.t0[2] = rec[tt].t0[2];
    r.n[0] = rec[tt].n[0]; r.n[1] = rec[tt].n[1]; r.n[2] = rec[tt].n[2];
    double acc = 0.0;
    for (int64_t base = b; base < e; base += QB) {
        __syncthreads();
        const int64_t p = base + threadIdx.x;
        if (p < e) load_pt(pts, order[p], sp[threadIdx.x][0], sp[threadIdx.x][1], sp[threadIdx.x][2]);
        __syncthreads();
        const int cnt = (int)(e - base < QB ? e - base : QB);
#pragma unroll 4
        for (int m = 0; m < cnt; ++m) acc = acc + fabs(perp_of(sp[m][0], sp[m][1], sp[m][2], r));
    }
    if (t < nt) dist[(int64_t)s * nt + t] = acc;
}

// one wave per instance: closest = argmin (a NaN wins, as in np.argmin), band tri_dist < min + 0.05 * min (:96-99), the candidates
// in triangle order; their inside counts start at 0
__global__ __launch_bounds__(64) void k_quad_candidates(const double* __restrict__ dist, int64_t nt, int32_t* __restrict__ cand,
                                                        int32_t* __restrict__ ncand, int32_t* __restrict__ counts) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const double* d = dist + (int64_t)s * nt;
    double mn = INFINITY;
    bool nan = false;
    for (int64_t t = lane; t < nt; t += 64) {
        const double v = d[t];
        nan |= isnan(v);
        mn = v < mn ? v : mn;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(mn, off);
        mn = o < mn ? o : mn;
    }
    const bool any_nan = __any(nan);
    const double upper = mn + 0.05 * mn;
    int base = 0;
    for (int64_t t0 = 0; t0 < nt && !any_nan; t0 += 64) {
        const int64_t t = t0 + lane;
        const bool pred = t < nt && d[t] < upper;
        const unsigned long long bal = __ballot(pred);
        if (pred) {
            const int64_t at = (int64_t)s * nt + base + __popcll(bal & ((1ull << lane) - 1));
            cand[at] = (int32_t)t;
            counts[at] = 0;
        }
        base += __popcll(bal);
    }
    if (lane == 0) ncand[s] = base;
}

// inside counts per (instance, candidate) (:106-110): waves walk the grouped member list; a wave whose lanes all belong to one
// instance adds one count per candidate
__global__ __launch_bounds__(QB) void k_quad_inside(const double* __restrict__ pts, const int32_t* __restrict__ order,
                                                    const uint32_t* __restrict__ skeys, const int64_t* __restrict__ starts, int k,
                                                    const tri_rec* __restrict__ rec, int64_t nt, const int32_t* __restrict__ cand,
                                                    const int32_t* __restrict__ ncand, int32_t* __restrict__ counts) {
    const int64_t P = starts[k];
    const int lane = threadIdx.x & 63;
    for (int64_t w = (int64_t)blockIdx.x * QB + threadIdx.x - lane; w < P; w += (int64_t)gridDim.x * QB) {
        const int64_t p = w + lane;
        const bool act = p < P;
        int s = -1;
        double x = 0.0, y = 0.0, z = 0.0;
        if (act) { s = (int)skeys[p]; load_pt(pts, order[p], x, y, z); }
        const int s0 = __shfl(s, 0);
        if (__ballot(act && s != s0) == 0) {
            const int nc = ncand[s0];
            const int64_t row = (int64_t)s0 * nt;
            for (int c = 0; c < nc; ++c) {
                const bool in = act && inside_of(x, y, z, rec[cand[row + c]]);
                const int nin = __popcll(__ballot(in));
                if (lane == 0 && nin) atomicAdd(&counts[row + c], nin);
            }
        } else if (act) {
            const int nc = ncand[s];
            const int64_t row = (int64_t)s * nt;
            for (int c = 0; c < nc; ++c)
                if (inside_of(x, y, z, rec[cand[row + c]])) atomicAdd(&counts[row + c], 1);
        }
    }
}

// per instance: idx = argmax (first maximum) (:111), the horizontal test (:117), _get_perpendicular_vectors (:50-62, :119) and the
// origin = the projection of the first member (:120)
__global__ __launch_bounds__(QB) void k_quad_choose(const double* __restrict__ pts, const int32_t* __restrict__ order,
                                                    const int64_t* __restrict__ starts, int k, const tri_rec* __restrict__ rec, int64_t nt,
                                                    const int32_t* __restrict__ cand, const int32_t* __restrict__ ncand,
                                                    const int32_t* __restrict__ counts, inst_rec* __restrict__ irec,
                                                    unsigned long long* __restrict__ ext) {
    for (int64_t s = (int64_t)blockIdx.x * QB + threadIdx.x; s < k; s += (int64_t)gridDim.x * QB) {
        ext[4 * s] = ~0ull; ext[4 * s + 1] = 0ull; ext[4 * s + 2] = ~0ull; ext[4 * s + 3] = 0ull;
        inst_rec o;
        for (int c = 0; c < 3; ++c) o.origin[c] = o.i[c] = o.j[c] = NAN;
        const int nc = ncand[s];
        if (nc == 0) { o.tri = -1; o.status = F3D_QUAD_NO_CANDIDATE; irec[s] = o; continue; }
        const int64_t row = (int64_t)s * nt;
        int best = counts[row], bc = 0;
        for (int c = 1; c < nc; ++c) if (counts[row + c] > best) { best = counts[row + c]; bc = c; }
        o.tri = cand[row + bc];
        const tri_rec r = rec[o.tri];
        if (COS10 < r.n[2]) { o.status = F3D_QUAD_HORIZONTAL; irec[s] = o; continue; }
        const double len = sqrt(blas_dot(r.n[0], r.n[1], r.n[2], r.n[0], r.n[1], r.n[2]));
        const double a0 = r.n[0] / len, a1 = r.n[1] / len, a2 = r.n[2] / len;
        double b0 = 0.0, b1 = 0.0, b2 = 1.0;                                 // arbitrary = [0, 0, 1]
        if (fabs(fabs(blas_dot(a0, a1, a2, b0, b1, b2)) - 1.0) <= ALLCLOSE_TOL) { b1 = 1.0; b2 = 0.0; }
        const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;       // np.cross(normal, arbitrary)
        const double e0 = a1 * c2 - a2 * c1, e1 = a2 * c0 - a0 * c2, e2 = a0 * c1 - a1 * c0;       // np.cross(normal, vector1)
        const double l1 = sqrt(blas_dot(c0, c1, c2, c0, c1, c2)), l2 = sqrt(blas_dot(e0, e1, e2, e0, e1, e2));
        o.i[0] = c0 / l1; o.i[1] = c1 / l1; o.i[2] = c2 / l1;
        o.j[0] = e0 / l2; o.j[1] = e1 / l2; o.j[2] = e2 / l2;
        double x, y, z;
        load_pt(pts, order[starts[s]], x, y, z);                             // nc > 0: the instance has members
        const double perp = perp_of(x, y, z, r);
        o.origin[0] = x - r.n[0] * perp; o.origin[1] = y - r.n[1] * perp; o.origin[2] = z - r.n[2] * perp;
        o.status = F3D_QUAD_OK;
        irec[s] = o;
    }
}

__device__ __forceinline__ void wave_minmax(unsigned long long& mn, unsigned long long& mx) {
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long a = __shfl_xor(mn, off), b = __shfl_xor(mx, off);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
}

// x = einsum('nc,c->n', box_pts - origin, i), y likewise with j (:122-125); min / max per instance
__global__ __launch_bounds__(QB) void k_quad_extents(const double* __restrict__ pts, const int32_t* __restrict__ order,
                                                     const uint32_t* __restrict__ skeys, const int64_t* __restrict__ starts, int k,
                                                     const tri_rec* __restrict__ rec, const inst_rec* __restrict__ irec,
                                                     unsigned long long* __restrict__ ext) {
    const int64_t P = starts[k];
    const int lane = threadIdx.x & 63;
    for (int64_t w = (int64_t)blockIdx.x * QB + threadIdx.x - lane; w < P; w += (int64_t)gridDim.x * QB) {
        const int64_t p = w + lane;
        int s = p < P ? (int)skeys[p] : -1;
        const bool act = s >= 0 && irec[s].status == F3D_QUAD_OK;
        unsigned long long xn = ~0ull, xx = 0ull, yn = ~0ull, yx = 0ull;
        if (act) {
            double px, py, pz;
            load_pt(pts, order[p], px, py, pz);
            const inst_rec& o = irec[s];
            const tri_rec& r = rec[o.tri];
            const double perp = perp_of(px, py, pz, r);
            const double d0 = (px - r.n[0] * perp) - o.origin[0];
            const double d1 = (py - r.n[1] * perp) - o.origin[1];
            const double d2 = (pz - r.n[2] * perp) - o.origin[2];
            const double x = (d0 * o.i[0] + d2 * o.i[2]) + d1 * o.i[1];
            const double y = (d0 * o.j[0] + d2 * o.j[2]) + d1 * o.j[1];
            xn = xx = f3d_ord_enc(x);
            yn = yx = f3d_ord_enc(y);
        }
        const int s0 = __shfl(s, 0);
        if (__ballot(s != s0) == 0) {
            if (s0 < 0 || irec[s0].status != F3D_QUAD_OK) continue;
            wave_minmax(xn, xx);
            wave_minmax(yn, yx);
            if (lane == 0) {
                atomicMin(&ext[4 * s0], xn); atomicMax(&ext[4 * s0 + 1], xx);
                atomicMin(&ext[4 * s0 + 2], yn); atomicMax(&ext[4 * s0 + 3], yx);
            }
        } else if (act) {
            atomicMin(&ext[4 * s], xn); atomicMax(&ext[4 * s + 1], xx);
            atomicMin(&ext[4 * s + 2], yn); atomicMax(&ext[4 * s + 3], yx);
        }
    }
}

// bbox = [origin + xmin*i + ymax*j, origin + xmin*i + ymin*j, origin + xmax*i + ymin*j, origin + xmax*i + ymax*j] (:126-131)
__global__ __launch_bounds__(QB) void k_quad_build(const inst_rec* __restrict__ irec, const unsigned long long* __restrict__ ext, int k,
                                                   double* __restrict__ quads, int32_t* __restrict__ status, int32_t* __restrict__ tri) {
    for (int64_t s = (int64_t)blockIdx.x * QB + threadIdx.x; s < k; s += (int64_t)gridDim.x * QB) {
        const inst_rec o = irec[s];
        status[s] = o.status;
        tri[s] = o.tri;
        const bool ok = o.status == F3D_QUAD_OK;
        const double xmin = f3d_ord_dec(ext[4 * s]), xmax = f3d_ord_dec(ext[4 * s + 1]);
        const double ymin = f3d_ord_dec(ext[4 * s + 2]), ymax = f3d_ord_dec(ext[4 * s + 3]);
        const double cx[4] = {xmin, xmin, xmax, xmax}, cy[4] = {ymax, ymin, ymin, ymax};
        for (int q = 0; q < 4; ++q)
            for (int c = 0; c < 3; ++c)
                quads[12 * (int64_t)s + 3 * q + c] = ok ? (o.origin[c] + cx[q] * o.i[c]) + cy[q] * o.j[c] : NAN;
    }
}

struct quad_layout { size_t keys, order, skeys, starts, group, rec, dist, cand, counts, ncand, sids, sslot, irec, ext, total; };
quad_layout quad_layout_for(int64_t n, int k, int64_t nt) {
    quad_layout L;
    f3d_carve c;
    const size_t kt = (size_t)k * (size_t)nt;
    L.keys = c.take((size_t)n * 8);
    L.order = c.take((size_t)n * 4);
    L.skeys = c.take((size_t)n * 4);
    L.starts = c.take((size_t)(k + 2) * 8);
    L.group = c.take(f3d_group_scratch_bytes(n, k));
    L.rec = c.take((size_t)nt * sizeof(tri_rec));
    L.dist = c.take(kt * 8);
    L.cand = c.take(kt * 4);
    L.counts = c.take(kt * 4);
    L.ncand = c.take((size_t)k * 4);
    L.sids = c.take((size_t)k * 8);
    L.sslot = c.take((size_t)k * 4);
    L.irec = c.take((size_t)k * sizeof(inst_rec));
    L.ext = c.take((size_t)k * 32);
    L.total = c.off;
    return L;
}

}  // namespace

size_t f3d_quads_scratch_bytes(int64_t n, int k, int64_t nt) { return quad_layout_for(n, k, nt).total; }

hipError_t f3d_launch_door_window_quads(const double* pts, int64_t n, const int64_t* ids, const int64_t* inst, int k, const double* verts,
                                        int64_t nv, const int64_t* tris, int64_t nt, double* quads, int32_t* status, int32_t* tri,
                                        double* normals, void* scratch, int* err, hipStream_t s) {
    if (n < 0 || n > 0x7fffffffLL || k < 0 || k > F3D_QUADS_MAX_INST || nt < 0 || nt > 0x7fffffffLL || nv < 0) return hipErrorInvalidValue;
    const quad_layout L = quad_layout_for(n, k, nt);
    char* base = reinterpret_cast<char*>(scratch);
    int64_t* keys = reinterpret_cast<int64_t*>(base + L.keys);
    int32_t* order = reinterpret_cast<int32_t*>(base + L.order);
    uint32_t* skeys = reinterpret_cast<uint32_t*>(base + L.skeys);
    int64_t* starts = reinterpret_cast<int64_t*>(base + L.starts);
    tri_rec* rec = reinterpret_cast<tri_rec*>(base + L.rec);
    double* dist = reinterpret_cast<double*>(base + L.dist);
    int32_t* cand = reinterpret_cast<int32_t*>(base + L.cand);
    int32_t* counts = reinterpret_cast<int32_t*>(base + L.counts);
    int32_t* ncand = reinterpret_cast<int32_t*>(base + L.ncand);
    int64_t* sids = reinterpret_cast<int64_t*>(base + L.sids);
    int32_t* sslot = reinterpret_cast<int32_t*>(base + L.sslot);
    inst_rec* irec = reinterpret_cast<inst_rec*>(base + L.irec);
    unsigned long long* ext = reinterpret_cast<unsigned long long*>(base + L.ext);
    const dim3 b(QB);
    hipError_t e;
    if (nt > 0) {
        hipLaunchKernelGGL(k_quad_tri_setup, dim3(f3d_grid_for(nt, QB, 8192)), b, 0, s, verts, nv, tris, nt, rec, normals, err);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (k == 0) return hipSuccess;
    const dim3 gk(f3d_grid_for(k, QB, 65536));
    hipLaunchKernelGGL(k_quad_rank_ids, gk, b, 0, s, inst, k, sids, sslot);
    if (n > 0) hipLaunchKernelGGL(k_quad_slot_keys, dim3(f3d_grid_for(n, QB, 8192)), b, 0, s, ids, n, sids, sslot, k, keys);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = f3d_launch_group_by_id(keys, n, k, order, skeys, starts, base + L.group, s)) != hipSuccess) return e;
    if (nt > 0) hipLaunchKernelGGL(k_quad_tri_dist, dim3((unsigned)((nt + QB - 1) / QB), (unsigned)k), b, 0, s, pts, order, starts, rec, nt, dist);
    hipLaunchKernelGGL(k_quad_candidates, dim3(k), dim3(64), 0, s, dist, nt, cand, ncand, counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dim3 gp(f3d_grid_for(n, QB, 8192));
    hipLaunchKernelGGL(k_quad_inside, gp, b, 0, s, pts, order, skeys, starts, k, rec, nt, cand, ncand, counts);
    hipLaunchKernelGGL(k_quad_choose, gk, b, 0, s, pts, order, starts, k, rec, nt, cand, ncand, counts, irec, ext);
    hipLaunchKernelGGL(k_quad_extents, gp, b, 0, s, pts, order, skeys, starts, k, rec, irec, ext);
    hipLaunchKernelGGL(k_quad_build, gk, b, 0, s, irec, ext, k, quads, status, tri);
    return hipGetLastError();
}
