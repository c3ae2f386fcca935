// The layout of the fused call's todo block (f3d_fuse_todo, f3d_kernels.h): plain host code, no HIP, so that
// tests compile it for the host (tests/test_fuse_todo_layout_cpu.py).  f3d_fuse_todo_layout is declared in f3d_kernels.h and DEFINED
// here, not inline: f3d_fuse.hip is the one source of the library that includes this header.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include "f3d_kernels.h"

#define F3D_PART_MAX_GROUPS 16            // view groups whose open-view masks a parked point carries (more: the point is redone from nothing)

// The layout of the todo block (f3d_fuse_todo, f3d_kernels.h).  The slots of the first list whose points can be parked (bins + view
// masks) are n / 16 + 4096; deferred points beyond them are redone from nothing.
f3d_fuse_todo f3d_fuse_todo_layout(int64_t n, int nviews, int nclasses) {
    int64_t k = 0;
    if (nviews > 0 && nviews <= 64 * F3D_PART_MAX_GROUPS) {
        k = n / 16 + 4096;
        if (const char* e = getenv("F3D_DEBUG_PARK_SLOTS")) k = atoll(e);   // tests: force the overflow path (deferred points beyond the parked slots)
        k = k < n ? (k < 0 ? 0 : k) : n;
    }
    f3d_fuse_todo t;
    t.park_slots = (int)k;
    t.park_stride = (nclasses + 1 + 2 + 3) >> 2;              // every label 0..nclasses present, plus the codes "no sample" and "rejected"
    t.ngroups = (nviews + 63) / 64;
    t.list2_off = 4 * sizeof(unsigned int) + (size_t)n * sizeof(int32_t);
    t.umask_off = t.list2_off + (size_t)n * sizeof(int32_t);
    t.park_off = t.umask_off + (size_t)k * t.ngroups * sizeof(unsigned long long);
    t.bytes = t.park_off + (size_t)k * t.park_stride * sizeof(uint32_t);
    return t;
}
