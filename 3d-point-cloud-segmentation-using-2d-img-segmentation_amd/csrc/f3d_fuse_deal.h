// How k_fuse's tiles are dealt to its blocks (no HIP beyond the qualifiers: tests compile this header for the host).
//
// Every XCD owns a list of tile positions (f3d_xcd_list_of: chunks of consecutive tiles taken by the XCDs in turn).  The blocks of one
// XCD, bx = 0 .. width[0] - 1, share that list in LAYERS: layer k holds the positions [start[k], start[k] + width[k]), and block bx
// walks start[k] + bx for every k with bx < width[k], in increasing k.  Widths do not increase, so the low block indices -- the
// hardware dispatches blocks in index order -- take the most tiles and the blocks dispatched last take one: few start-ups (code
// book, view tables, a barrier) and many tile starts hidden behind a predecessor early on, and a tail one tile long.  That is loop
// scheduling by factoring, laid out statically: batch i hands each of `slots` blocks (the blocks an XCD holds at a time)
// ceil(R_i / (F * slots)) of the R_i positions still open.
// Beyond the last layer a block goes on with that layer's width as its stride, so a deal of ONE layer of `width` blocks is the plain
// stride walk bx, bx + width, bx + 2 width, ...: what every cloud got before, and what a cloud too large for the layers still gets.
#pragma once

#ifndef __host__
#define __host__
#define __device__
#endif

#define F3D_DEAL_LAYERS 16
#ifndef F3D_DEAL_FACTOR
#define F3D_DEAL_FACTOR 2                // F of the factoring rule: a batch takes 1/F of what is left (measured: profiles/fuse_deal.md)
#endif
#ifndef F3D_DEAL_MAX_TILES
#define F3D_DEAL_MAX_TILES 3             // most tiles one block walks in the layers (at most F3D_DEAL_LAYERS: a block's tiles are its layers).
#endif                                   // Longer blocks save more start-ups but their tiles run slower (measured: profiles/fuse_deal.md)
#ifndef F3D_XCD_CHUNK_LOG2
#define F3D_XCD_CHUNK_LOG2 6             // 64 tiles per chunk of the XCD-aware tile mapping (64 .. 256 measured alike)
#endif
#ifndef F3D_XCD_MIN_ROWS
#define F3D_XCD_MIN_ROWS 8               // chunk rows per XCD at least (small clouds: 1.25M points 0.349 -> 0.314 ms per step with 8 instead of 4)
#endif

struct f3d_deal { int nlayers; int width[F3D_DEAL_LAYERS]; int start[F3D_DEAL_LAYERS]; };

// one XCD's list: chunks of 2^xlog tiles (smaller for small clouds), `positions` of them (the last chunk row may hold fewer tiles)
struct f3d_xcd_list { int xlog; int positions; };
__host__ __device__ inline f3d_xcd_list f3d_xcd_list_of(int ntiles) {
    int xlog = F3D_XCD_CHUNK_LOG2;
    while (xlog > 0 && ntiles < ((8 * F3D_XCD_MIN_ROWS) << xlog)) --xlog;
    const int chunk_rows = (ntiles + (8 << xlog) - 1) >> (xlog + 3);
    return {xlog, chunk_rows << xlog};
}

// The walker: block bx's position in the first layer after layer k (k = -1: its first), or k < 0 when it has none left.
struct f3d_deal_pos { int k; int pos; };
__host__ __device__ inline f3d_deal_pos f3d_deal_next(const f3d_deal& d, int positions, int bx, int k) {
    ++k;
    const int kk = k < d.nlayers ? k : d.nlayers - 1;                   // past the layers: the last one's stride
    const int w = d.width[kk];
    const long long pos = (long long)d.start[kk] + (long long)(k - kk) * w + bx;
    if (bx < w && pos < positions) return {k, (int)pos};
    return {-1, -1};
}

// one layer of `width` blocks: the stride walk
__host__ inline f3d_deal f3d_deal_uniform(int width) {
    f3d_deal d = {};
    d.nlayers = 1; d.width[0] = width < 1 ? 1 : width; d.start[0] = 0;
    return d;
}

// The factoring deal of `positions` positions for an XCD that holds `slots` blocks at a time, with at most `max_blocks` blocks.
// A cloud of more than 2 slots' worth of positions keeps its last `slots` positions for one-tile blocks whatever the batches before
// them leave over; one that fits the slots gets the stride walk.
__host__ inline f3d_deal f3d_deal_make(int positions, int slots, int max_blocks) {
    if (slots < 1) slots = 1;
    if (max_blocks < 1) max_blocks = 1;
    if (positions <= slots) return f3d_deal_uniform(positions < max_blocks ? positions : max_blocks);
    const int most = F3D_DEAL_MAX_TILES < F3D_DEAL_LAYERS ? (F3D_DEAL_MAX_TILES < 1 ? 1 : F3D_DEAL_MAX_TILES) : F3D_DEAL_LAYERS;
    const int tail = positions > 2 * slots ? slots : 0;
    int count[F3D_DEAL_LAYERS + 1] = {0};                                // blocks of 1 .. F3D_DEAL_LAYERS tiles
    long long blocks = tail;
    count[1] = tail;
    for (int left = positions - tail; left > 0;) {
        int each = (int)(((double)left + (double)F3D_DEAL_FACTOR * slots - 1.0) / ((double)F3D_DEAL_FACTOR * slots));   // ceil(left / (F slots))
        each = each < 1 ? 1 : (each > most ? most : each);
        for (int b = 0; b < slots && left > 0; ++b) {
            const int t = each < left ? each : left;
            ++count[t]; ++blocks; left -= t;
        }
    }
    if (blocks > max_blocks) {
        // more blocks than the launch may have: max_blocks blocks all the same, the tail of one-tile blocks and the others sharing the rest
        // evenly (sizes q + 1 and q) -- or, where that takes more than F3D_DEAL_LAYERS tiles a block, the stride walk
        const int nb = max_blocks - tail, rest = positions - tail;
        if (tail == 0 || nb < 1 || (rest + nb - 1) / nb > F3D_DEAL_LAYERS) return f3d_deal_uniform(max_blocks);
        for (int t = 0; t <= F3D_DEAL_LAYERS; ++t) count[t] = 0;
        count[rest / nb] += nb - rest % nb;                               // (rest / nb >= 1: the factoring deal had more blocks than this)
        if (rest % nb) count[rest / nb + 1] += rest % nb;
        count[1] += tail;
    }
    // sizes in non-increasing order -> layer k holds the blocks of more than k tiles
    f3d_deal d = {};
    int w = 0, at = 0;
    for (int t = F3D_DEAL_LAYERS; t >= 1; --t) {
        w += count[t];
        if (w > 0 && d.nlayers == 0) d.nlayers = t;
        d.width[t - 1] = w;
    }
    for (int k = 0; k < d.nlayers; ++k) { d.start[k] = at; at += d.width[k]; }
    for (int k = d.nlayers; k < F3D_DEAL_LAYERS; ++k) d.width[k] = d.start[k] = 0;
    return d;
}
