// Mesh topology of segUtils/meshUtils.py (reference :235-333, :360-375) on gfx950, plus clean_mesh, their composition.
//
// The slot of a triangle corner is s = 3 * f + j.  Three building blocks serve every entry:
//   group   : f3d_group_pairs (f3d_groups.h) of (key, position) pairs -> a CSR whose rows list their members in ascending position
//             (vertex -> slots for vertex_triangle_mapping, cluster -> triangles for the area sums);
//   compact : 0 / 1 flags of the vertices and of the faces in ONE array, one exclusive scan, one kernel that writes the
//             renumbered faces (face order kept), the old -> new vertex ids and, when wanted, the surviving vertex rows;
//   cluster : 3 edge keys (min << b | max, b = bits of nv) per triangle, radix sort limited to 2b (+1) bits, union of the triangles
//             of equal neighbouring keys (f3d_uf_link: a root is its component's lowest triangle), compression, roots flagged
//             and scanned -> clusters numbered by their lowest triangle.
// keep_faces_by_vertices' first-appearance numbering: first[v] = atomicMin of the slots of kept faces that hold v; slot s is a
// first occurrence iff first[tri[s]] == s; the scan of those flags over the slots is the new id.  Minima, not timing, decide.
// Areas: 0.5 * sqrt((cx*cx + cy*cy) + cz*cz), c = cross(p0 - p1, p0 - p2) by plain multiply and subtract (no contraction).  A
// cluster's members, in ascending triangle index, are cut into chunks of 4096; a chunk is summed by one wave (f3d_wave_sum) and the
// chunk sums are summed the same way (f3d_groups.h).  The shape depends on the member count alone; no float atomics.
// Every kernel after k_mesh_check returns at once when counts[2] is set (an index outside [0, nv)): nothing is written.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include "f3d.h"
#include "f3d_kernels.h"
#include "f3d_groups.h"

#pragma clang fp contract(off)

namespace {

constexpr int MB = 256;
constexpr int MGRID = 8192;
constexpr int AREA_CHUNK = 4096;          // members per chunk of a cluster's area sum

#define MESH_LOOP(i, n) for (int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x; i < (n); i += (int64_t)gridDim.x * MB)

__device__ __forceinline__ int64_t tri_at(const void* __restrict__ tris, int itype, int64_t s) {
    return itype == F3D_I32 ? (int64_t)reinterpret_cast<const int32_t*>(tris)[s] : reinterpret_cast<const int64_t*>(tris)[s];
}

__device__ __forceinline__ void tri_put(void* __restrict__ tris, int itype, int64_t s, int64_t v) {
    if (itype == F3D_I32) reinterpret_cast<int32_t*>(tris)[s] = (int32_t)v; else reinterpret_cast<int64_t*>(tris)[s] = v;
}

// row `from` of src -> row `to` of dst, [*, 3] of float64 or float32, bit for bit
__device__ __forceinline__ void row_copy(const void* __restrict__ src, void* __restrict__ dst, int vdtype, int64_t from, int64_t to) {
    if (vdtype == F3D_F64) {
        const uint64_t* a = reinterpret_cast<const uint64_t*>(src) + 3 * from;
        uint64_t* b = reinterpret_cast<uint64_t*>(dst) + 3 * to;
        b[0] = a[0]; b[1] = a[1]; b[2] = a[2];
    } else {
        const uint32_t* a = reinterpret_cast<const uint32_t*>(src) + 3 * from;
        uint32_t* b = reinterpret_cast<uint32_t*>(dst) + 3 * to;
        b[0] = a[0]; b[1] = a[1]; b[2] = a[2];
    }
}

__device__ __forceinline__ double coord(const void* __restrict__ verts, int vdtype, int64_t i) {
    return vdtype == F3D_F64 ? reinterpret_cast<const double*>(verts)[i] : (double)reinterpret_cast<const float*>(verts)[i];
}

// counts[2] = 1 and the error bit when a corner is outside [0, nv)
__global__ __launch_bounds__(MB) void k_mesh_check(const void* __restrict__ tris, int itype, int64_t n3, int64_t nv, int64_t* counts,
                                                   int* err, int errbit) {
    bool bad = false;
    MESH_LOOP(s, n3) {
        const int64_t v = tri_at(tris, itype, s);
        bad |= (v < 0) | (v >= nv);
    }
    if (bad) { counts[2] = 1; atomicOr(err, errbit); }
}

// ---- group ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MB) void k_mesh_corner_keys(const void* __restrict__ tris, int itype, int64_t n3, const int64_t* counts,
                                                         uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    if (counts[2]) return;
    MESH_LOOP(s, n3) { keys[s] = (uint32_t)tri_at(tris, itype, s); vals[s] = (uint32_t)s; }
}

__global__ __launch_bounds__(MB) void k_mesh_vmap_out(const uint32_t* __restrict__ slots, int64_t n3, const int64_t* counts,
                                                      int32_t* __restrict__ tri, int8_t* __restrict__ pos) {
    if (counts[2]) return;
    MESH_LOOP(i, n3) {
        const uint32_t s = slots[i];
        tri[i] = (int32_t)(s / 3u);
        pos[i] = (int8_t)(s % 3u);
    }
}

// ---- compact ----------------------------------------------------------------------------------------------------------
// face_off[f] = 1 when a corner of f has vmask set (else 0), or the reverse with `invert`
__global__ __launch_bounds__(MB) void k_mesh_face_touch(const void* __restrict__ tris, int itype, int64_t nt, const uint8_t* __restrict__ vmask,
                                                        int invert, const int64_t* counts, uint8_t* __restrict__ out) {
    if (counts[2]) return;
    MESH_LOOP(f, nt) {
        const bool touch = vmask[tri_at(tris, itype, 3 * f)] | vmask[tri_at(tris, itype, 3 * f + 1)] | vmask[tri_at(tris, itype, 3 * f + 2)];
        out[f] = (uint8_t)(touch != (invert != 0));
    }
}

// flags[0 .. nv) = vertex kept (vmask != 0, reversed with `invert`), flags[nv .. nv + nt) = fkeep, flags[nv + nt] = 0
__global__ __launch_bounds__(MB) void k_mesh_flags(int64_t nv, int64_t nt, const uint8_t* __restrict__ vmask, int invert,
                                                   const uint8_t* __restrict__ fkeep, const int64_t* counts, uint32_t* __restrict__ flags) {
    if (counts[2]) return;
    MESH_LOOP(i, nv + nt + 1) {
        uint32_t v = 0;
        if (i < nv) v = (vmask[i] != 0) != (invert != 0);
        else if (i < nv + nt) v = fkeep[i - nv] != 0;
        flags[i] = v;
    }
}

// scan = the exclusive scan of k_mesh_flags' array.  old2new (may be NULL): the new id of a kept vertex, 0 for a dropped one;
// out_verts (may be NULL): the kept rows; out_tris: the kept faces renumbered, in face order; counts = {faces, vertices}
__global__ __launch_bounds__(MB) void k_mesh_compact(const void* __restrict__ tris, int itype, int64_t nt, int64_t nv,
                                                     const uint32_t* __restrict__ scan, const void* __restrict__ verts, int vdtype,
                                                     void* __restrict__ out_tris, int64_t* __restrict__ old2new, void* __restrict__ out_verts,
                                                     int64_t* counts) {
    if (counts[2]) return;
    const uint32_t fbase = scan[nv];
    MESH_LOOP(i, nv + nt) {
        const uint32_t at = scan[i];
        const bool kept = scan[i + 1] != at;
        if (i < nv) {
            if (old2new) old2new[i] = kept ? (int64_t)at : 0;
            if (out_verts && kept) row_copy(verts, out_verts, vdtype, i, at);
        } else if (kept) {
            const int64_t f = i - nv, to = (int64_t)(at - fbase);
            for (int j = 0; j < 3; ++j) tri_put(out_tris, itype, 3 * to + j, (int64_t)scan[tri_at(tris, itype, 3 * f + j)]);
        }
        if (i == 0) { counts[0] = (int64_t)(scan[nv + nt] - fbase); counts[1] = (int64_t)fbase; }
    }
}

// ---- keep_faces_by_vertices -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MB) void k_mesh_keep_first(const void* __restrict__ tris, int itype, int64_t nt, const uint8_t* __restrict__ mask,
                                                        const int64_t* counts, uint32_t* first, uint8_t* __restrict__ fkeep) {
    if (counts[2]) return;
    MESH_LOOP(f, nt) {
        const int64_t a = tri_at(tris, itype, 3 * f), b = tri_at(tris, itype, 3 * f + 1), c = tri_at(tris, itype, 3 * f + 2);
        const bool k = mask[a] | mask[b] | mask[c];
        fkeep[f] = k;
        if (k) {
            atomicMin(first + a, (uint32_t)(3 * f));
            atomicMin(first + b, (uint32_t)(3 * f + 1));
            atomicMin(first + c, (uint32_t)(3 * f + 2));
        }
    }
}

// flags[0 .. 3nt) = the slot is its vertex's first occurrence over the kept faces, flags[3nt .. 4nt) = fkeep, flags[4nt] = 0
__global__ __launch_bounds__(MB) void k_mesh_keep_flags(const void* __restrict__ tris, int itype, int64_t nt, const uint32_t* __restrict__ first,
                                                        const uint8_t* __restrict__ fkeep, const int64_t* counts, uint32_t* __restrict__ flags) {
    if (counts[2]) return;
    const int64_t n3 = 3 * nt;
    MESH_LOOP(i, n3 + nt + 1) {
        uint32_t v = 0;
        if (i < n3) v = fkeep[i / 3] && first[tri_at(tris, itype, i)] == (uint32_t)i;
        else if (i < n3 + nt) v = fkeep[i - n3] != 0;
        flags[i] = v;
    }
}

__global__ __launch_bounds__(MB) void k_mesh_keep_out(const void* __restrict__ verts, int vdtype, const void* __restrict__ tris, int itype,
                                                      int64_t nt, const uint32_t* __restrict__ first, const uint32_t* __restrict__ scan,
                                                      void* __restrict__ out_verts, void* __restrict__ out_tris, int64_t* counts) {
    if (counts[2]) return;
    const int64_t n3 = 3 * nt;
    const uint32_t fbase = scan[n3];
    MESH_LOOP(i, n3 + nt) {
        const uint32_t at = scan[i];
        if (scan[i + 1] != at) {
            if (i < n3) row_copy(verts, out_verts, vdtype, tri_at(tris, itype, i), at);
            else {
                const int64_t f = i - n3, to = (int64_t)(at - fbase);
                for (int j = 0; j < 3; ++j) tri_put(out_tris, itype, 3 * to + j, (int64_t)scan[first[tri_at(tris, itype, 3 * f + j)]]);
            }
        }
        if (i == 0) { counts[0] = (int64_t)fbase; counts[1] = (int64_t)(scan[n3 + nt] - fbase); }
    }
}

// ---- cluster ----------------------------------------------------------------------------------------------------------
// the corners of face f widened to float64 and c = cross(p0 - p1, p0 - p2), every product and difference rounded alone
__device__ __forceinline__ void face_cross(const void* __restrict__ verts, int vdtype, const void* __restrict__ tris, int itype, int64_t f,
                                           double p[3][3], double c[3]) {
    for (int j = 0; j < 3; ++j) {
        const int64_t v = tri_at(tris, itype, 3 * f + j);
        for (int k = 0; k < 3; ++k) p[j][k] = coord(verts, vdtype, 3 * v + k);
    }
    const double a0 = p[0][0] - p[1][0], a1 = p[0][1] - p[1][1], a2 = p[0][2] - p[1][2];
    const double b0 = p[0][0] - p[2][0], b1 = p[0][1] - p[2][1], b2 = p[0][2] - p[2][2];
    c[0] = a1 * b2 - a2 * b1; c[1] = a2 * b0 - a0 * b2; c[2] = a0 * b1 - a1 * b0;
}

__global__ __launch_bounds__(MB) void k_mesh_area(const void* __restrict__ verts, int vdtype, const void* __restrict__ tris, int itype,
                                                  int64_t nt, const int64_t* counts, double* __restrict__ area) {
    if (counts[2]) return;
    MESH_LOOP(f, nt) {
        double p[3][3], c[3];
        face_cross(verts, vdtype, tris, itype, f, p, c);
        area[f] = 0.5 * sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    }
}

__device__ __forceinline__ uint64_t edge_key(uint64_t u, uint64_t v, int b) { return u < v ? (u << b | v) : (v << b | u); }

// the edges (0,1), (0,2), (1,2) of every triangle as min << b | max; a face that is not active carries bit 2b instead
__global__ __launch_bounds__(MB) void k_mesh_edge_keys(const void* __restrict__ tris, int itype, int64_t nt, const uint8_t* __restrict__ active,
                                                       int b, const int64_t* counts, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                       int32_t* __restrict__ parent) {
    if (counts[2]) return;
    MESH_LOOP(f, nt) {
        parent[f] = (int32_t)f;
        const uint64_t v0 = (uint64_t)tri_at(tris, itype, 3 * f), v1 = (uint64_t)tri_at(tris, itype, 3 * f + 1),
                       v2 = (uint64_t)tri_at(tris, itype, 3 * f + 2);
        const bool on = !active || active[f];
        const uint64_t off = (uint64_t)1 << (2 * b);
        keys[3 * f] = on ? edge_key(v0, v1, b) : off;
        keys[3 * f + 1] = on ? edge_key(v0, v2, b) : off;
        keys[3 * f + 2] = on ? edge_key(v1, v2, b) : off;
        vals[3 * f] = vals[3 * f + 1] = vals[3 * f + 2] = (uint32_t)f;
    }
}

__global__ __launch_bounds__(MB) void k_mesh_union(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t n3, int b,
                                                   const int64_t* counts, int32_t* parent) {
    if (counts[2]) return;
    MESH_LOOP(i, n3) {
        if (i == 0) continue;
        const uint64_t k = keys[i];
        if (k != keys[i - 1] || (k >> (2 * b))) continue;
        f3d_uf_link(parent, (int32_t)vals[i - 1], (int32_t)vals[i]);
    }
}

// root[f] = lowest triangle of f's component; flags[f] = f is the root of an active component; flags[nt] = 0
__global__ __launch_bounds__(MB) void k_mesh_roots(const int32_t* parent, int64_t nt, const uint8_t* __restrict__ active, const int64_t* counts,
                                                   int32_t* __restrict__ root, uint32_t* __restrict__ flags) {
    if (counts[2]) return;
    MESH_LOOP(f, nt + 1) {
        if (f == nt) { flags[f] = 0; continue; }
        const int32_t x = f3d_uf_root(parent, (int32_t)f);
        root[f] = x;
        flags[f] = x == (int32_t)f && (!active || active[f]);
    }
}

// clusters[f] = number of f's cluster (-1 for a face that is not active); the grouping keys of the area sums; counts[0] = clusters
__global__ __launch_bounds__(MB) void k_mesh_labels(const int32_t* __restrict__ root, const uint32_t* __restrict__ scan, int64_t nt,
                                                    const uint8_t* __restrict__ active, int32_t* __restrict__ clusters,
                                                    uint32_t* __restrict__ gkeys, uint32_t* __restrict__ gvals, int64_t* counts) {
    if (counts[2]) return;
    MESH_LOOP(f, nt) {
        const bool on = !active || active[f];
        const uint32_t c = scan[root[f]];
        clusters[f] = on ? (int32_t)c : -1;
        gkeys[f] = on ? c : (uint32_t)nt;
        gvals[f] = (uint32_t)f;
        if (f == 0) counts[0] = (int64_t)scan[nt];
    }
}

// partial[q] = f3d_wave_sum of the chunk of AREA_CHUNK consecutive members that starts at grouped position q
__global__ __launch_bounds__(MB) void k_mesh_chunk_sums(const double* __restrict__ tri_area, const uint32_t* __restrict__ order,
                                                        const uint32_t* __restrict__ skeys, const int64_t* __restrict__ starts,
                                                        const uint32_t* __restrict__ nclusters, int64_t nt, const int64_t* counts,
                                                        double* __restrict__ partial) {
    if (counts[2]) return;
    const int lane = threadIdx.x & 63;
    f3d_chunk_heads<AREA_CHUNK, MB>(skeys, starts, nt, (int64_t)*nclusters, [&](int64_t q, int64_t len, int64_t) {
        const double sum = f3d_wave_sum(len, lane, [&](int64_t i) { return tri_area[order[q + i]]; });
        if (lane == 0) partial[q] = sum;
    });
}

// one wave per cluster: the member count, and the area = the sum of the cluster's chunk sums
__global__ __launch_bounds__(MB) void k_mesh_cluster_sums(const double* __restrict__ partial, const int64_t* __restrict__ starts,
                                                          const uint32_t* __restrict__ nclusters, const int64_t* counts,
                                                          int64_t* __restrict__ cluster_n, double* __restrict__ cluster_area) {
    if (counts[2]) return;
    const int lane = threadIdx.x & 63;
    f3d_group_waves<MB>(starts, (int64_t)*nclusters, [&](int64_t c, int64_t b, int64_t e) {
        const double sum = f3d_chunks_sum<AREA_CHUNK>(b, e, lane, [&](int64_t q) { return partial[q]; });
        if (lane == 0) { cluster_n[c] = e - b; cluster_area[c] = sum; }
    });
}

// ---- clean_mesh -------------------------------------------------------------------------------------------------------
// kept_t[f] = f's cluster has at least min_triangles members and its area is not below min_area; kept_v (zeroed before) = 1 at
// the corners of the kept faces
__global__ __launch_bounds__(MB) void k_mesh_clean_keep(const void* __restrict__ tris, int itype, int64_t nt, const int32_t* __restrict__ clusters,
                                                        const int64_t* __restrict__ cluster_n, const double* __restrict__ cluster_area,
                                                        int64_t min_triangles, double min_area, const int64_t* counts,
                                                        uint8_t* __restrict__ kept_t, uint8_t* kept_v) {
    if (counts[2]) return;
    MESH_LOOP(f, nt) {
        const int32_t c = clusters[f];
        const bool k = c >= 0 && cluster_n[c] >= min_triangles && !(cluster_area[c] < min_area);
        kept_t[f] = k;
        if (k) for (int j = 0; j < 3; ++j) kept_v[tri_at(tris, itype, 3 * f + j)] = 1;
    }
}

struct mesh_layout {
    size_t keys_a, keys_b, vals_a, vals_b, flags, parent, root, first, fkeep, active, clusters, cluster_n, cluster_area, tri_area, partial, starts, temp,
        total;
    size_t temp_bytes;
};

mesh_layout mesh_layout_for(int64_t nv, int64_t nt) {
    if (nv < 1) nv = 1;
    if (nt < 1) nt = 1;
    mesh_layout L;
    const size_t n3 = (size_t)nt * 3, nflags = (size_t)(nv + nt > 4 * nt ? nv + nt : 4 * nt) + 1;
    size_t a = 0, b = f3d_group_temp_bytes((int64_t)n3), c = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n3, 0u, 64u);
    (void)rocprim::exclusive_scan(nullptr, c, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t)0, nflags, rocprim::plus<uint32_t>());
    L.temp_bytes = (a > b ? (a > c ? a : c) : (b > c ? b : c)) + 256;
    f3d_carve k;
    L.keys_a = k.take(n3 * 8); L.keys_b = k.take(n3 * 8); L.vals_a = k.take(n3 * 4); L.vals_b = k.take(n3 * 4);
    L.flags = k.take(nflags * 4);
    L.parent = k.take((size_t)nt * 4); L.root = k.take((size_t)nt * 4); L.first = k.take((size_t)nv * 4);
    L.fkeep = k.take((size_t)nt); L.active = k.take((size_t)nt);
    L.clusters = k.take((size_t)nt * 4); L.cluster_n = k.take((size_t)nt * 8); L.cluster_area = k.take((size_t)nt * 8);
    L.tri_area = k.take((size_t)nt * 8); L.partial = k.take((size_t)nt * 8); L.starts = k.take((size_t)(nt + 2) * 8);
    L.temp = k.take(L.temp_bytes);
    L.total = k.off;
    return L;
}

bool mesh_sizes_ok(int64_t nv, int64_t nt) { return nv >= 0 && nv <= 0x7fffffffLL && nt >= 0 && 3 * nt <= 0x7fffffffLL; }

dim3 grid_of(int64_t n) { return dim3(f3d_grid_for(n, MB, MGRID)); }

// counts = 0, then the index check
hipError_t mesh_begin(const void* tris, int itype, int64_t nt, int64_t nv, int64_t* counts, int* err, hipStream_t s) {
    F3D_TRY(hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s));
    if (nt > 0) hipLaunchKernelGGL(k_mesh_check, grid_of(3 * nt), dim3(MB), 0, s, tris, itype, 3 * nt, nv, counts, err, F3D_DEVERR_MESH);
    return hipGetLastError();
}

hipError_t mesh_scan(const mesh_layout& L, char* base, size_t n, hipStream_t s) {
    size_t tb = L.temp_bytes;
    uint32_t* flags = reinterpret_cast<uint32_t*>(base + L.flags);
    return rocprim::exclusive_scan(base + L.temp, tb, flags, flags, (uint32_t)0, n, rocprim::plus<uint32_t>(), s);
}

// the n (key, position) pairs in keys_a / vals_a grouped by the low `bits` of the key -> keys_b / vals_b and the rows' starts.
// The early-out flag counts[2] is an int64 that holds 0 or 1: its low word is the 32-bit flag f3d_group_pairs reads.
hipError_t mesh_group(const mesh_layout& L, char* base, int64_t n, int bits, int64_t nkeys, const uint32_t* nkeys_dev, const int64_t* counts,
                      int64_t* starts, hipStream_t s) {
    return f3d_group_pairs(reinterpret_cast<uint32_t*>(base + L.keys_a), reinterpret_cast<uint32_t*>(base + L.keys_b),
                           reinterpret_cast<uint32_t*>(base + L.vals_a), reinterpret_cast<uint32_t*>(base + L.vals_b), n, bits, base + L.temp,
                           L.temp_bytes, nkeys, nkeys_dev, reinterpret_cast<const int32_t*>(counts + 2), starts, s);
}

// the compaction: flags from vmask / fkeep, their scan, the outputs (k_mesh_compact)
hipError_t mesh_compact(const mesh_layout& L, char* base, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                        const uint8_t* vmask, int invert, const uint8_t* fkeep, void* out_tris, int64_t* old2new, void* out_verts,
                        int64_t* counts, hipStream_t s) {
    uint32_t* flags = reinterpret_cast<uint32_t*>(base + L.flags);
    hipLaunchKernelGGL(k_mesh_flags, grid_of(nv + nt + 1), dim3(MB), 0, s, nv, nt, vmask, invert, fkeep, counts, flags);
    F3D_TRY(hipGetLastError());
    F3D_TRY(mesh_scan(L, base, (size_t)(nv + nt + 1), s));
    hipLaunchKernelGGL(k_mesh_compact, grid_of(nv + nt), dim3(MB), 0, s, tris, itype, nt, nv, flags, verts, vdtype, out_tris, old2new, out_verts,
                       counts);
    return hipGetLastError();
}

// clusters of the active faces (all when active == NULL); cluster_n / cluster_area / tri_area hold nt entries
hipError_t mesh_clusters(const mesh_layout& L, char* base, const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt,
                         const uint8_t* active, int32_t* clusters, int64_t* cluster_n, double* cluster_area, double* tri_area, int64_t* counts,
                         hipStream_t s) {
    uint64_t *ka = reinterpret_cast<uint64_t*>(base + L.keys_a), *kb = reinterpret_cast<uint64_t*>(base + L.keys_b);
    uint32_t *va = reinterpret_cast<uint32_t*>(base + L.vals_a), *vb = reinterpret_cast<uint32_t*>(base + L.vals_b);
    uint32_t* flags = reinterpret_cast<uint32_t*>(base + L.flags);
    int32_t *parent = reinterpret_cast<int32_t*>(base + L.parent), *root = reinterpret_cast<int32_t*>(base + L.root);
    int64_t* starts = reinterpret_cast<int64_t*>(base + L.starts);
    const dim3 g(grid_of(nt + 1)), g3(grid_of(3 * nt)), b(MB);
    const int vb_bits = f3d_bits_for(nv, 1);
    hipLaunchKernelGGL(k_mesh_area, g, b, 0, s, verts, vdtype, tris, itype, nt, counts, tri_area);
    hipLaunchKernelGGL(k_mesh_edge_keys, g, b, 0, s, tris, itype, nt, active, vb_bits, counts, ka, va, parent);
    F3D_TRY(hipGetLastError());
    size_t tb = L.temp_bytes;
    F3D_TRY(rocprim::radix_sort_pairs(base + L.temp, tb, ka, kb, va, vb, (size_t)(3 * nt), 0u, (unsigned)(2 * vb_bits + (active ? 1 : 0)), s));
    hipLaunchKernelGGL(k_mesh_union, g3, b, 0, s, kb, vb, 3 * nt, vb_bits, counts, parent);
    hipLaunchKernelGGL(k_mesh_roots, g, b, 0, s, parent, nt, active, counts, root, flags);
    F3D_TRY(hipGetLastError());
    F3D_TRY(mesh_scan(L, base, (size_t)(nt + 1), s));
    hipLaunchKernelGGL(k_mesh_labels, g, b, 0, s, root, flags, nt, active, clusters, reinterpret_cast<uint32_t*>(ka), va, counts);
    F3D_TRY(hipGetLastError());
    F3D_TRY(mesh_group(L, base, nt, f3d_bits_for(nt + 1, 1), nt, flags + nt, counts, starts, s));
    double* partial = reinterpret_cast<double*>(base + L.partial);
    hipLaunchKernelGGL(k_mesh_chunk_sums, g, b, 0, s, tri_area, vb, reinterpret_cast<const uint32_t*>(kb), starts, flags + nt, nt, counts, partial);
    hipLaunchKernelGGL(k_mesh_cluster_sums, dim3(f3d_grid_for(nt, MB / 64, MGRID)), b, 0, s, partial, starts, flags + nt, counts, cluster_n,
                       cluster_area);
    return hipGetLastError();
}

}  // namespace

size_t f3d_mesh_scratch_bytes(int64_t nv, int64_t nt) { return mesh_layout_for(nv, nt).total; }

hipError_t f3d_launch_mesh_vertex_map(const void* tris, int itype, int64_t nt, int64_t nv, int64_t* offsets, int32_t* tri, int8_t* pos,
                                      void* scratch, int64_t* counts, int* err, hipStream_t s) {
    if (!mesh_sizes_ok(nv, nt)) return hipErrorInvalidValue;
    F3D_TRY(mesh_begin(tris, itype, nt, nv, counts, err, s));
    if (nt == 0) return hipMemsetAsync(offsets, 0, (size_t)(nv + 1) * 8, s);
    const mesh_layout L = mesh_layout_for(nv, nt);
    char* base = reinterpret_cast<char*>(scratch);
    const int64_t n3 = 3 * nt;
    hipLaunchKernelGGL(k_mesh_corner_keys, grid_of(n3), dim3(MB), 0, s, tris, itype, n3, counts, reinterpret_cast<uint32_t*>(base + L.keys_a),
                       reinterpret_cast<uint32_t*>(base + L.vals_a));
    F3D_TRY(hipGetLastError());
    F3D_TRY(mesh_group(L, base, n3, f3d_bits_for(nv, 1), nv, nullptr, counts, offsets, s));
    hipLaunchKernelGGL(k_mesh_vmap_out, grid_of(n3), dim3(MB), 0, s, reinterpret_cast<const uint32_t*>(base + L.vals_b), n3, counts, tri, pos);
    return hipGetLastError();
}

hipError_t f3d_launch_mesh_remove_faces(const void* tris, int itype, int64_t nt, int64_t nv, const uint8_t* mask, uint8_t* not_removed,
                                        void* remaining, int64_t* old2new, void* scratch, int64_t* counts, int* err, hipStream_t s) {
    if (!mesh_sizes_ok(nv, nt)) return hipErrorInvalidValue;
    F3D_TRY(mesh_begin(tris, itype, nt, nv, counts, err, s));
    const mesh_layout L = mesh_layout_for(nv, nt);
    char* base = reinterpret_cast<char*>(scratch);
    if (nt > 0) hipLaunchKernelGGL(k_mesh_face_touch, grid_of(nt), dim3(MB), 0, s, tris, itype, nt, mask, 1, counts, not_removed);
    F3D_TRY(hipGetLastError());
    return mesh_compact(L, base, nullptr, F3D_F64, nv, tris, itype, nt, mask, 1, not_removed, remaining, old2new, nullptr, counts, s);
}

hipError_t f3d_launch_mesh_keep_faces(const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt, const uint8_t* mask,
                                      void* out_verts, void* out_tris, void* scratch, int64_t* counts, int* err, hipStream_t s) {
    if (!mesh_sizes_ok(nv, nt)) return hipErrorInvalidValue;
    F3D_TRY(mesh_begin(tris, itype, nt, nv, counts, err, s));
    if (nt == 0) return hipSuccess;
    const mesh_layout L = mesh_layout_for(nv, nt);
    char* base = reinterpret_cast<char*>(scratch);
    uint32_t *first = reinterpret_cast<uint32_t*>(base + L.first), *flags = reinterpret_cast<uint32_t*>(base + L.flags);
    uint8_t* fkeep = reinterpret_cast<uint8_t*>(base + L.fkeep);
    F3D_TRY(hipMemsetAsync(first, 0xff, (size_t)nv * 4, s));
    hipLaunchKernelGGL(k_mesh_keep_first, grid_of(nt), dim3(MB), 0, s, tris, itype, nt, mask, counts, first, fkeep);
    hipLaunchKernelGGL(k_mesh_keep_flags, grid_of(4 * nt + 1), dim3(MB), 0, s, tris, itype, nt, first, fkeep, counts, flags);
    F3D_TRY(hipGetLastError());
    F3D_TRY(mesh_scan(L, base, (size_t)(4 * nt + 1), s));
    hipLaunchKernelGGL(k_mesh_keep_out, grid_of(4 * nt), dim3(MB), 0, s, verts, vdtype, tris, itype, nt, first, flags, out_verts, out_tris, counts);
    return hipGetLastError();
}

hipError_t f3d_launch_mesh_clusters(const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt, int32_t* clusters,
                                    int64_t* cluster_n, double* cluster_area, double* tri_area, void* scratch, int64_t* counts, int* err,
                                    hipStream_t s) {
    if (!mesh_sizes_ok(nv, nt)) return hipErrorInvalidValue;
    F3D_TRY(mesh_begin(tris, itype, nt, nv, counts, err, s));
    if (nt == 0) return hipSuccess;
    const mesh_layout L = mesh_layout_for(nv, nt);
    char* base = reinterpret_cast<char*>(scratch);
    if (!tri_area) tri_area = reinterpret_cast<double*>(base + L.tri_area);
    return mesh_clusters(L, base, verts, vdtype, nv, tris, itype, nt, nullptr, clusters, cluster_n, cluster_area, tri_area, counts, s);
}

hipError_t f3d_launch_mesh_clean(const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt, const uint8_t* remove_mask,
                                 int64_t min_triangles, double min_area, void* new_verts, void* new_tris, uint8_t* kept_v, uint8_t* kept_t,
                                 void* scratch, int64_t* counts, int* err, hipStream_t s) {
    if (!mesh_sizes_ok(nv, nt)) return hipErrorInvalidValue;
    F3D_TRY(mesh_begin(tris, itype, nt, nv, counts, err, s));
    if (nv > 0) F3D_TRY(hipMemsetAsync(kept_v, 0, (size_t)nv, s));
    if (nt == 0) return hipSuccess;
    const mesh_layout L = mesh_layout_for(nv, nt);
    char* base = reinterpret_cast<char*>(scratch);
    uint8_t* active = nullptr;
    if (remove_mask) {
        active = reinterpret_cast<uint8_t*>(base + L.active);
        hipLaunchKernelGGL(k_mesh_face_touch, grid_of(nt), dim3(MB), 0, s, tris, itype, nt, remove_mask, 1, counts, active);
        F3D_TRY(hipGetLastError());
    }
    int32_t* clusters = reinterpret_cast<int32_t*>(base + L.clusters);
    int64_t* cluster_n = reinterpret_cast<int64_t*>(base + L.cluster_n);
    double* cluster_area = reinterpret_cast<double*>(base + L.cluster_area);
    F3D_TRY(mesh_clusters(L, base, verts, vdtype, nv, tris, itype, nt, active, clusters, cluster_n, cluster_area,
                           reinterpret_cast<double*>(base + L.tri_area), counts, s));
    hipLaunchKernelGGL(k_mesh_clean_keep, grid_of(nt), dim3(MB), 0, s, tris, itype, nt, clusters, cluster_n, cluster_area, min_triangles, min_area,
                       counts, kept_t, kept_v);
    F3D_TRY(hipGetLastError());
    return mesh_compact(L, base, verts, vdtype, nv, tris, itype, nt, kept_v, 0, kept_t, new_tris, nullptr, new_verts, counts, s);
}

// ---- face graph -------------------------------------------------------------------------------------------------------
// The cluster path's edge keys, sorted with the half-edge slot s = 3 f + j as the value (bit 31: the face runs through the edge
// from its lower to its higher vertex).  The sort is stable and slots ascend with f, so a run of equal keys lists its faces in
// ascending order and a face that holds the edge twice sits on adjacent entries.  Every sorted position scatters its run
// [first, last) back to its slot (k_fg_runs); a face's row is then the three-way merge, duplicates skipped, of the runs of its
// three slots (fg_row), once to count and once to fill.  A run of k faces costs O(k) per member: a fan of k faces on one edge is
// quadratic in k, as is its output.
namespace {

constexpr uint32_t FG_SLOT = 0x7fffffffu;           // the slot of a sorted value; bit 31 is the direction
constexpr uint32_t FG_END = 0xffffffffu;

__global__ __launch_bounds__(MB) void k_face_frames(const void* __restrict__ verts, int vdtype, const void* __restrict__ tris, int itype,
                                                    int64_t nt, const int64_t* counts, double* __restrict__ normals,
                                                    double* __restrict__ centroids, double* __restrict__ areas) {
    if (counts[2]) return;
    MESH_LOOP(f, nt) {
        double p[3][3], c[3];
        face_cross(verts, vdtype, tris, itype, f, p, c);
        const double len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
        const bool ok = len > 0.0 && len < INFINITY;
        for (int k = 0; k < 3; ++k) normals[3 * f + k] = ok ? c[k] / len : 0.0;
        if (centroids) for (int k = 0; k < 3; ++k) centroids[3 * f + k] = ((p[0][k] + p[1][k]) + p[2][k]) / 3.0;
        if (areas) areas[f] = 0.5 * len;
    }
}

// winding v0 -> v1 -> v2 -> v0: edge (0,1) runs v0 -> v1, edge (0,2) runs v2 -> v0, edge (1,2) runs v1 -> v2
__global__ __launch_bounds__(MB) void k_fg_keys(const void* __restrict__ tris, int itype, int64_t nt, int b, const int64_t* counts,
                                                uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    if (counts[2]) return;
    MESH_LOOP(f, nt) {
        const uint64_t v0 = (uint64_t)tri_at(tris, itype, 3 * f), v1 = (uint64_t)tri_at(tris, itype, 3 * f + 1),
                       v2 = (uint64_t)tri_at(tris, itype, 3 * f + 2);
        const uint32_t s = (uint32_t)(3 * f);
        keys[3 * f] = edge_key(v0, v1, b);     vals[3 * f] = s | (uint32_t)(v0 < v1) << 31;
        keys[3 * f + 1] = edge_key(v0, v2, b); vals[3 * f + 1] = (s + 1) | (uint32_t)(v2 < v0) << 31;
        keys[3 * f + 2] = edge_key(v1, v2, b); vals[3 * f + 2] = (s + 2) | (uint32_t)(v1 < v2) << 31;
    }
}

// bounds[slot] = first | last << 32 | direction << 63 of the slot's run in the sorted order; the head of a run counts it as a
// boundary edge (one half-edge, counts[3]) or a non-manifold one (more than two, counts[1])
__global__ __launch_bounds__(MB) void k_fg_runs(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t n3,
                                                int64_t* counts, uint64_t* __restrict__ bounds) {
    if (counts[2]) return;
    unsigned long long boundary = 0, fans = 0;
    MESH_LOOP(i, n3) {
        const uint64_t k = keys[i];
        int64_t lo = i, hi = i + 1;
        while (lo > 0 && keys[lo - 1] == k) --lo;
        while (hi < n3 && keys[hi] == k) ++hi;
        const uint32_t v = vals[i];
        bounds[v & FG_SLOT] = (uint64_t)lo | (uint64_t)hi << 32 | (uint64_t)(v >> 31) << 63;
        if (lo == i) { boundary += hi - lo == 1; fans += hi - lo > 2; }
    }
    for (int o = 32; o; o >>= 1) { boundary += __shfl_xor(boundary, o); fans += __shfl_xor(fans, o); }
    if ((threadIdx.x & 63) == 0) {
        if (fans) atomicAdd(reinterpret_cast<unsigned long long*>(counts + 1), fans);
        if (boundary) atomicAdd(reinterpret_cast<unsigned long long*>(counts + 3), boundary);
    }
}

// Row f: every face g != f, ascending, that shares an edge with f through which the pair passes -> emit(g).  Through an edge the pair
// passes when there is no gate, or when s * dot(nf, ng) >= cos_crease, s = +1 where the two faces run through the edge in opposite
// directions (consistent orientation) and -1 where they run the same way; a face that holds the edge twice counts by its first entry.
template <class Emit>
__device__ __forceinline__ void fg_row(int64_t f, const uint32_t* __restrict__ vals, const uint64_t* __restrict__ bounds,
                                       const double* __restrict__ normals, double cos_crease, Emit emit) {
    uint32_t p[3], e[3], face[3], dir[3], own[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const uint64_t w = bounds[3 * f + j];
        p[j] = (uint32_t)w; e[j] = (uint32_t)(w >> 32) & FG_SLOT; own[j] = (uint32_t)(w >> 63);
        const uint32_t v = vals[p[j]];                                  // a slot's run holds the slot: never empty
        face[j] = (v & FG_SLOT) / 3u; dir[j] = v >> 31;
    }
    double nf[3] = {0.0, 0.0, 0.0};
    if (normals) for (int k = 0; k < 3; ++k) nf[k] = normals[3 * f + k];
    for (;;) {
        const uint32_t g = min(face[0], min(face[1], face[2]));
        if (g == FG_END) break;
        bool pass = !normals, have = false;
        double dot = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (face[j] != g) continue;
            if (normals && g != (uint32_t)f) {
                if (!have) {
                    const double* ng = normals + 3 * (int64_t)g;
                    dot = (nf[0] * ng[0] + nf[1] * ng[1]) + nf[2] * ng[2];
                    have = true;
                }
                pass |= (dir[j] != own[j] ? dot : -dot) >= cos_crease;
            }
            uint32_t next = FG_END, d = 0;
            while (++p[j] < e[j]) {
                const uint32_t v = vals[p[j]];
                if ((v & FG_SLOT) / 3u != g) { next = (v & FG_SLOT) / 3u; d = v >> 31; break; }
            }
            face[j] = next; dir[j] = d;
        }
        if (pass && g != (uint32_t)f) emit((int32_t)g);
    }
}

// FILL == false: rowoff[f] = the length of row f, rowoff[nt] = 0 (the scan turns them into the offsets).  FILL == true: the rows,
// unless they need more than `cap` entries
template <bool FILL>
__global__ __launch_bounds__(MB) void k_fg_rows(const uint32_t* __restrict__ vals, const uint64_t* __restrict__ bounds,
                                                const double* __restrict__ normals, double cos_crease, int64_t nt, const int64_t* counts,
                                                int64_t* rowoff, int32_t* __restrict__ neighbours, int64_t cap) {
    if (counts[2]) return;
    if (FILL && rowoff[nt] > cap) return;
    MESH_LOOP(f, nt + (FILL ? 0 : 1)) {
        int64_t n = 0;
        if (f < nt) {
            int32_t* row = FILL ? neighbours + rowoff[f] : nullptr;
            fg_row(f, vals, bounds, normals, cos_crease, [&](int32_t g) { if (FILL) row[n] = g; ++n; });
        }
        if (!FILL) rowoff[f] = n;
    }
}

__global__ __launch_bounds__(MB) void k_fg_offsets(const int64_t* __restrict__ rowoff, int64_t nt, int64_t* counts, int64_t* __restrict__ offsets) {
    if (counts[2]) return;
    MESH_LOOP(i, nt + 1) {
        offsets[i] = rowoff[i];
        if (i == nt) counts[0] = rowoff[nt];
    }
}

struct fg_layout { size_t keys_a, keys_b, vals_a, vals_b, normals, rowoff, temp, total, temp_bytes; };

fg_layout fg_layout_for(int64_t nt) {
    if (nt < 1) nt = 1;
    fg_layout L;
    const size_t n3 = (size_t)nt * 3;
    size_t a = 0, b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n3, 0u, 64u);
    (void)rocprim::exclusive_scan(nullptr, b, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)nt + 1, rocprim::plus<int64_t>());
    L.temp_bytes = (a > b ? a : b) + 256;
    f3d_carve k;
    L.keys_a = k.take(n3 * 8); L.keys_b = k.take(n3 * 8); L.vals_a = k.take(n3 * 4); L.vals_b = k.take(n3 * 4);
    L.normals = k.take((size_t)nt * 24); L.rowoff = k.take((size_t)(nt + 1) * 8);
    L.temp = k.take(L.temp_bytes);
    L.total = k.off;
    return L;
}

}  // namespace

size_t f3d_face_graph_scratch_bytes(int64_t nt) { return fg_layout_for(nt).total; }

hipError_t f3d_launch_mesh_face_frames(const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt, double* normals,
                                       double* centroids, double* areas, int64_t* counts, int* err, hipStream_t s) {
    if (!mesh_sizes_ok(nv, nt)) return hipErrorInvalidValue;
    F3D_TRY(mesh_begin(tris, itype, nt, nv, counts, err, s));
    if (nt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_face_frames, grid_of(nt), dim3(MB), 0, s, verts, vdtype, tris, itype, nt, counts, normals, centroids, areas);
    return hipGetLastError();
}

hipError_t f3d_launch_mesh_face_graph(const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt, int gate,
                                      double cos_crease, int64_t* offsets, int32_t* neighbours, int64_t cap, void* scratch, int64_t* counts,
                                      int* err, hipStream_t s) {
    if (!mesh_sizes_ok(nv, nt) || cap < 0) return hipErrorInvalidValue;
    F3D_TRY(mesh_begin(tris, itype, nt, nv, counts, err, s));
    if (nt == 0) return hipMemsetAsync(offsets, 0, 8, s);
    const fg_layout L = fg_layout_for(nt);
    char* base = reinterpret_cast<char*>(scratch);
    uint64_t *ka = reinterpret_cast<uint64_t*>(base + L.keys_a), *kb = reinterpret_cast<uint64_t*>(base + L.keys_b);
    uint32_t *va = reinterpret_cast<uint32_t*>(base + L.vals_a), *vb = reinterpret_cast<uint32_t*>(base + L.vals_b);
    double* normals = gate ? reinterpret_cast<double*>(base + L.normals) : nullptr;
    int64_t* rowoff = reinterpret_cast<int64_t*>(base + L.rowoff);
    const dim3 g(grid_of(nt + 1)), g3(grid_of(3 * nt)), b(MB);
    const int bits = f3d_bits_for(nv, 1);
    hipLaunchKernelGGL(k_fg_keys, g, b, 0, s, tris, itype, nt, bits, counts, ka, va);
    if (gate) hipLaunchKernelGGL(k_face_frames, g, b, 0, s, verts, vdtype, tris, itype, nt, counts, normals, (double*)nullptr, (double*)nullptr);
    F3D_TRY(hipGetLastError());
    size_t tb = L.temp_bytes;
    F3D_TRY(rocprim::radix_sort_pairs(base + L.temp, tb, ka, kb, va, vb, (size_t)(3 * nt), 0u, (unsigned)(2 * bits), s));
    uint64_t* bounds = ka;                                                  // the unsorted keys are done with
    hipLaunchKernelGGL(k_fg_runs, g3, b, 0, s, kb, vb, 3 * nt, counts, bounds);
    hipLaunchKernelGGL(k_fg_rows<false>, g, b, 0, s, vb, bounds, normals, cos_crease, nt, counts, rowoff, (int32_t*)nullptr, cap);
    F3D_TRY(hipGetLastError());
    tb = L.temp_bytes;
    F3D_TRY(rocprim::exclusive_scan(base + L.temp, tb, rowoff, rowoff, (int64_t)0, (size_t)(nt + 1), rocprim::plus<int64_t>(), s));
    hipLaunchKernelGGL(k_fg_offsets, g, b, 0, s, rowoff, nt, counts, offsets);
    if (neighbours) hipLaunchKernelGGL(k_fg_rows<true>, g, b, 0, s, vb, bounds, normals, cos_crease, nt, counts, rowoff, neighbours, cap);
    return hipGetLastError();
}
